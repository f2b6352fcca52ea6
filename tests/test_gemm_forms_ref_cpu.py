"""The references of tests/test_gpu_gemm_forms.py checked without a GPU: what the lo probes claim, how far
the fp32 emulation of the bf16x3 product sits under the project's bound, the form rsx_gemm_x3_form reports
for every shape of the table (256 CUs, the host fallback and the MI355X's count), and the argument refusals
of the weight-stationary route (they return before any launch)."""
import ctypes
import os

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native
from tests import gemm_forms_ref as R

PROBE_K = (16, 32, 288, 384, 544, 2048, 3072)


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


def _is_f32(x64):
    return torch.equal(x64.float().double(), x64)


@pytest.mark.parametrize("K", PROBE_K)
def test_integer_operands_have_no_lo_and_exact_sums(K):
    a, w, b = R.int_case(37, 128, K, seed=K)
    for t in (a, w):
        hi, lo = R.split(t)
        assert torch.equal(hi, t) and not lo.any()
    z = a.double() @ w.double().T + b.double()
    assert _is_f32(z) and torch.equal(R.emulate32(a, w).double() + b.double(), z)
    assert z.abs().max() < 2 ** 24 and bool((z != 0).all())


@pytest.mark.parametrize("K", PROBE_K)
@pytest.mark.parametrize("which", ["a", "b", "ab"])
def test_lo_probes_are_exact_and_see_the_lo_fragments(which, K):
    a, w, b, z = R.probe_case(which, 37, 128, K, seed=K + 1)
    for t, lo_side in ((a, which in ("a", "ab")), (w, which in ("b", "ab"))):
        hi, lo = R.split(t)
        if lo_side:
            assert torch.equal(hi, torch.ones_like(t))                 # hi = 1 on both sides of 1.0
            assert torch.equal(lo * 4096.0, (t - 1.0) * 4096.0)        # lo = i / 4096 exactly
            assert lo.min() == -7 / 4096 and lo.max() == 7 / 4096
        else:
            assert torch.equal(hi, t) and not lo.any()
    # the expected value is fp32-representable and the fp32 emulation reproduces it in any order
    assert _is_f32(z) and _is_f32(z - b.double())
    assert torch.equal(R.emulate32(a, w).double() + b.double(), z)
    assert torch.equal((R.emulate32(a, w) + b).double(), z)
    true = a.double() @ w.double().T + b.double()
    if which == "ab":      # the documented sum drops lo * lo': it is not the true product
        i, j = (a.double() - 1) * 4096, (w.double() - 1) * 4096
        assert torch.equal(z, K + (i.sum(1)[:, None] + j.sum(1)[None, :]) / 4096 + b.double())
        assert torch.equal(true - z, (i @ j.T) / 2 ** 24)
    else:
        assert torch.equal(true, z)
    # a kernel that lost the lo fragments would return the hi-only product
    miss = (R.hi_only64(a, w) + b.double() != z).double().mean().item()
    if which == "ab":
        assert miss > 0.98, miss
    else:
        assert miss > 0.9 or K <= 32, miss
        assert miss > 0.7, miss


def test_minus_eight_would_break_the_probe():
    """Why i stops at -7: 1 - 8/4096 lies halfway between two bf16 values below 1.0."""
    x = torch.tensor([1.0 - 8.0 / 4096.0, 1.0 - 9.0 / 4096.0])
    assert not torch.equal(R.split(x)[0], torch.ones(2))


FLOAT_SHAPES = [(129, 256, K) for K in (16, 32, 48, 96, 128, 256, 272, 288, 304, 320, 352, 384, 512, 544, 768,
                                        1024, 2048)] + [(1, 128, 16), (257, 128, 3072)]


@pytest.mark.parametrize("M,N,K", FLOAT_SHAPES)
def test_emulation_stays_under_half_the_project_bound(M, N, K):
    a, w, _ = R.float_case(M, N, K, seed=M + N + K)
    ref = a.double() @ w.double().T
    err = (R.emulate32(a, w).double() - ref).abs()
    ratio = (err / R.bound(a, w)).max().item()
    print(f"  K {K}: emulation / bound {ratio:.3f}")
    assert ratio <= 0.5, ratio
    # and the three-term sum itself (no fp32 rounding) is not the exact product: lo * lo' is missing
    assert (R.three_term64(a, w) - ref).abs().max() > 0


def test_epilogue_restatements_agree_between_dtypes():
    """fp32 and float64 restatements of every epilogue differ by fp32 rounding only, masks included."""
    M, N, K = 33, 128, 32
    a, w, b = R.float_case(M, N, K, seed=5)
    acc = a.double() @ w.double().T
    g = torch.Generator().manual_seed(6)
    aux = torch.randn(M, N, generator=g)
    table, ridx = torch.randn(5, N, generator=g), torch.randint(0, 5, (M,), generator=g)
    x = torch.randn(M, N, generator=g)
    for kind in ("bias", "gelu", "dgelu", "relu", "relu_train", "rowadd", "addln"):
        for p in (0.0, 0.3):
            kw = dict(bias=b, p=p, aux=aux, table=table, ridx=ridx, x=x)
            c64, x64 = R.epilogue(kind, acc, R.F64, **kw)
            c32, x32 = R.epilogue(kind, acc, R.F32, **kw)
            assert c64.dtype == R.F64 and c32.dtype == R.F32
            assert (c32.double() - c64).abs().max() <= 4 * 2.0 ** -24 * c64.abs().max() + 1e-7, (kind, p)
            if x64 is not None:
                assert (x32.double() - x64).abs().max() <= 1e-6, (kind, p)
            if p > 0 and kind in ("gelu", "dgelu", "relu_train"):
                keep = R.keep_mask(R.SEED, p, M, N)
                assert bool((c64[~keep] == 0).all()) and abs(keep.double().mean().item() - 0.7) < 0.03
    s = R.epilogue("addln", acc, R.F64, bias=b, x=x)[0]
    y, mean, rstd = R.layer_norm(s, torch.ones(N), torch.zeros(N), 1e-5)
    want = torch.nn.functional.layer_norm(s, (N,), eps=1e-5)
    assert (y - want).abs().max() < 1e-12
    assert torch.allclose(rstd, 1 / torch.sqrt(s.var(-1, unbiased=False) + 1e-5), rtol=1e-12, atol=0)


def test_form_table_at_256_cus():
    lib = _lib()
    rows = R.form_table()
    groups = {r[0] for r in rows}
    assert groups == {"two", "two_big", "four32", "four16", "split", "ws"}
    for group, M, N, K, e, with_ws, form, S in rows:
        floats = lib.rsx_gemm_x3_split_floats(M, N, K)
        s_host = R.split_count(M, N, K)
        assert floats == (s_host * M * N if s_host > 1 else 0), (M, N, K, floats)
        got = lib.rsx_gemm_x3_form(M, N, K, R.EPI[e], floats if with_ws else 0)
        assert got == form, (group, M, N, K, e, with_ws, got, form)
        if form == R.FORM_SPLIT:
            assert floats // (M * N) == S and floats % (M * N) == 0, (M, N, K, floats)
            # one float short of the workspace: no split (four stages, or two for the dGELU epilogue)
            assert lib.rsx_gemm_x3_form(M, N, K, R.EPI[e], floats - 1) == \
                (R.FORM_TWO if e == "dgelu" else R.FORM_FOUR32)
    # stage counts of the four-stage BK 32 cases cover every residue mod 4, those of BK 16 are odd
    assert {K // 32 % 4 for g, _, _, K, *_ in rows if g == "four32"} == {0, 1, 2, 3}
    assert all(K % 32 == 16 for g, _, _, K, *_ in rows if g == "four16")
    # the strip-loop shapes are weight-stationary too
    for N, K in ((1024, 128), (1024, 256), (1024, 384), (128, 128), (128, 256)):
        M = R.strip_rows(256, N, K)
        assert M == {(1024, 384): 4129, (1024, 128): 8225, (1024, 256): 8225}.get((N, K), 65569)
        assert lib.rsx_gemm_x3_form(M, N, K, 0, 0) == R.FORM_WS


def test_form_refuses_what_the_entry_refuses():
    lib = _lib()
    for M, N, K, epi in ((-1, 128, 32, 0), (4, 96, 32, 0), (4, 0, 32, 0), (4, 128, 24, 0), (4, 128, 0, 0),
                         (4, 128, 32, 5), (4, 128, 32, -1), (1 << 25, 128, 32, 0)):
        assert lib.rsx_gemm_x3_form(M, N, K, epi, 0) == -1, (M, N, K, epi)
    assert lib.rsx_gemm_x3_form((1 << 25) - 1, 128, 32, 0, 0) == R.FORM_TWO


P = ctypes.c_void_p(64)   # a non-null, 16-byte aligned pointer that is never dereferenced
Q = ctypes.c_void_p(68)   # non-null, not 16-byte aligned


def _call(lib, entry, **kw):
    a = dict(K=128, epi=0, aux=None, ldaux=0, C=P, ldc=512)
    a.update(kw)
    head = (P, a["K"], P, a["K"], None, 4, 512, a["K"], a["epi"], a["aux"], a["ldaux"], 0.0, 0, a["C"], a["ldc"])
    if entry == "ws":
        return lib.rsx_gemm_x3_ws(*head, None, 0, None)
    return lib.rsx_gemm_x3(*head, None)


@pytest.mark.parametrize("entry", ["plain", "ws"])
@pytest.mark.parametrize("K", [128, 256, 384])
def test_weight_stationary_route_refuses_unaligned_outputs(entry, K):
    """K 128 / 256 / 384 goes to the float4-storing kernel: C, ldc and a given aux / ldaux are checked as
    rsx_gemm_x3_tn and rsx_gemm_x3_relu_train check them. Every call returns 1 before any launch."""
    lib = _lib()
    assert lib.rsx_gemm_x3_form(4, 512, K, 0, 0) == R.FORM_WS
    for kw, msg in (({"C": Q}, b"C must be"), ({"ldc": 514}, b"C must be"), ({"ldc": 513}, b"C must be"),
                    ({"epi": 1, "aux": Q, "ldaux": 512}, b"aux must be"),
                    ({"epi": 1, "aux": P, "ldaux": 514}, b"aux must be"),
                    ({"epi": 2, "aux": Q, "ldaux": 512}, b"aux must be"),
                    ({"epi": 2, "aux": P, "ldaux": 518}, b"aux must be"),
                    ({"ldc": 508}, b"leading dimensions")):
        assert _call(lib, entry, K=K, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())


@pytest.mark.parametrize("entry", ["plain", "ws"])
def test_streamed_forms_are_not_refused_for_alignment(entry):
    """The LDS-staged kernels store scalars: the new refusals belong to form 0 only. With M = 0 the accepted
    call returns 0 and launches nothing."""
    lib = _lib()
    assert lib.rsx_gemm_x3_form(0, 512, 64, 0, 0) == R.FORM_TWO
    head = (P, 64, P, 64, None, 0, 512, 64, 0, None, 0, 0.0, 0, Q, 514)
    rc = lib.rsx_gemm_x3_ws(*head, None, 0, None) if entry == "ws" else lib.rsx_gemm_x3(*head, None)
    assert rc == 0, lib.rsx_last_error()
    head = (P, 128, P, 128, None, 0, 512, 128, 0, None, 0, 0.0, 0, Q, 512)
    rc = lib.rsx_gemm_x3_ws(*head, None, 0, None) if entry == "ws" else lib.rsx_gemm_x3(*head, None)
    assert rc == 1 and b"C must be" in lib.rsx_last_error()
