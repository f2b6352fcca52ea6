"""The evidence that tests/test_gpu_deepfm_forms.py would fail on a subtly wrong DeepFM forward kernel.

At the input scale of tests/deepfm_fwd_ref.py and the project's logit bound TOL = 1e-4 against float64:
the fp32 oracle is within TOL / 10, a float64 emulation of the kernels' bf16x3 DNN products within
TOL / 3, and every wrong variant (one `lo` image of a bf16x3 product dropped, a field missing from the FM
term or the first-order sum, a row reading its neighbour's ids) is beyond 3 * TOL on at least 10 % of the
rows (the row-shift variant: on its one row). Also the argument errors of the forward's C ABI, which return
before any launch and so need no device."""
import ctypes

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native
from tests import deepfm_fwd_ref as D
from tests.deepfm_fwd_ref import TOL

ROWS = 2048
_CASES = {}


def _case(F):
    if F not in _CASES:
        c = D.make_case(F, ROWS, seed=1)
        _CASES[F] = (c, D.reference(c)[0])
    return _CASES[F]


def test_case_layout():
    c, _ = _case(39)
    assert c["vocab"][0] == D.BIG_VOCAB and 1 in c["vocab"] and max(c["vocab"][1:]) < 100
    x, last = c["x"], c["last"]
    assert (x >= 0).all() and (x <= last).all()
    assert (x[0] == 0).all() and (x[1] == last).all() and (x[-1] == last).all()
    assert all((x[:, f] == last[f]).any() for f in range(39))
    one = D.make_case(5, 1, seed=1)
    assert one["x"].shape == (1, 5) and (one["x"] == 0).all()
    # NULL first-order tables contribute zero
    a = D.reference(c, rows=slice(0, 64))[0]
    b = D.reference(c, rows=slice(0, 64), w_null=(0, 38))[0]
    first = c["W"][0][x[:64, 0]].double() + c["W"][38][x[:64, 38]].double()
    assert (a - b - first).abs().max() < 1e-12
    assert (D.lin_reference(c, slice(0, 64), w_null=(0, 38)) + first - D.lin_reference(c, slice(0, 64))).abs().max() < 1e-12


@pytest.mark.parametrize("F", [1, 5, 25, 39, 64])
def test_tolerance_separates_correct_from_wrong(F):
    c, ref = _case(F)
    print(f"\nF={F}: logit std {ref.std().item():.3f}")
    e32 = (D.reference_fp32(c) - ref).abs().max().item()
    ex3 = (D.bf16x3_model(c) - ref).abs().max().item()
    print(f"  fp32 oracle floor {e32:.3e} (bound {TOL / 10:.1e}); bf16x3 floor {ex3:.3e} (bound {TOL / 3:.1e})")
    assert e32 <= TOL / 10
    assert ex3 <= TOL / 3
    muts = D.mutants(c)
    assert len(muts) == 8
    if F == 1:
        # one field: no pairs, so the FM term vanishes and that mutant is the reference itself; "missing
        # the last field" and "missing field 0" of the first-order sum are the same mutant
        emb, _ = D._gather(c, c["x"])
        assert torch.equal(D._fm(emb), torch.zeros(ROWS, dtype=torch.float64))
        assert torch.equal(muts["last field missing from the first-order sum"],
                           muts["first-order weight of field 0 missing"])
        del muts["last field missing from the FM term"]
    for name, got in muts.items():
        err = (got - ref).abs()
        if name == D.SHIFT_MUTANT:
            r = D.shifted_row(c)
            assert not torch.equal(c["x"][r], c["x"][r - 1])
            others = torch.cat([err[:r], err[r + 1:]]).max().item()
            print(f"  {name}: row {r} off by {err[r].item():.3e} = {err[r].item() / (3 * TOL):.1f} x 3 TOL")
            assert others == 0.0
            assert err[r].item() > 3 * TOL
            continue
        frac = (err > 3 * TOL).double().mean().item()
        print(f"  {name}: max {err.max().item():.3e} median {err.median().item():.3e} = "
              f"{err.median().item() / (3 * TOL):.1f} x 3 TOL; {100 * frac:.0f} % of rows beyond 3 TOL")
        assert frac >= 0.10, (name, frac)


# ---- argument errors: returned before any launch ----------------------------------------------------------
FAKE = ctypes.c_void_p(256)  # a non-NULL pointer that no error path dereferences


def _ptrs(n, null_at=()):
    arr = (ctypes.c_void_p * n)()
    for k in range(n):
        arr[k] = None if k in null_at else 256
    return arr


def _run(lib, F, V, packed):
    return lib.rsx_deepfm_fused_run(FAKE, 4, F, V, None, packed, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)


def test_forward_argument_errors():
    lib = _native.load()
    for F in (0, 65):
        assert lib.rsx_deepfm_fused_workspace_bytes(F) == -1
        assert _run(lib, F, _ptrs(64), None) == 1 and b"F must be" in lib.rsx_last_error()
        assert lib.rsx_deepfm_fused_prep(F, FAKE, FAKE, FAKE, None) == 1 and b"F must be" in lib.rsx_last_error()
        rc = lib.rsx_deepfm_fused(FAKE, 4, F, _ptrs(64), None, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
        assert rc == 1 and b"F must be" in lib.rsx_last_error()
        rc = lib.rsx_deepfm_embed(FAKE, 4, F, 16, _ptrs(64), None, 0.0, None, FAKE, None)
        assert rc == 1 and b"F must be" in lib.rsx_last_error()
    for F in (5, 39, 40):
        assert _run(lib, F, _ptrs(F, null_at=(F - 1,)), None) == 1 and b"null field table" in lib.rsx_last_error()
    for F in (39, 40):
        assert _run(lib, F, _ptrs(F), _ptrs(F, null_at=(F // 2,))) == 1
        assert b"null packed table" in lib.rsx_last_error()
    rc = lib.rsx_deepfm_embed(FAKE, 4, 5, 8, _ptrs(5), None, 0.0, None, FAKE, None)
    assert rc == 1 and b"embedding dim" in lib.rsx_last_error()
    rc = lib.rsx_deepfm_embed(FAKE, 4, 5, 16, _ptrs(5, null_at=(2,)), None, 0.0, None, FAKE, None)
    assert rc == 1 and b"null field table" in lib.rsx_last_error()


def test_dispatch_table():
    """The packed forms are exactly F in [25, 48]; the workspace covers every form's weight images."""
    lib = _native.load()
    for F in range(1, 65):
        assert lib.rsx_deepfm_fused_uses_packed(F) == (1 if 25 <= F <= 48 else 0), F
        w2 = 2 * 2 * D.H2 * D.H1                                  # W2 hi + lo, bf16
        if F == 39:
            used = 39 * 8192 * 2 + w2                             # deepfm_prep3_k: [F][8192] bf16
        else:
            fc = 8 if 25 <= F <= 48 else 13
            used = 2 * 2 * (-(-F // fc) * fc) * D.H1 * 16 + w2   # W1 hi + lo in whole chunks
        assert used <= lib.rsx_deepfm_fused_workspace_bytes(F), F
