"""HybridUserTower's training pieces without a GPU: the argument checks of rsx_gemm_x3_relu_train and of
the label-without-bias flag (18) of the plain contrastive kernels, and the two in-batch losses of
tower_code/mined_inference.py on CPU tensors against tests/tower_loss_ref.py (float64)."""
import ctypes
import os

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native, ops
from recsys_amd.tower_code import mined_inference as MI
from tests import tower_loss_ref as LR


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


P = ctypes.c_void_p(64)   # a non-null, 16-byte aligned pointer that is never dereferenced
Q = ctypes.c_void_p(68)   # non-null, not 16-byte aligned


def _relu_train(lib, **kw):
    a = dict(A=P, lda=128, B=P, ldb=128, M=4, N=512, K=128, aux=P, ldaux=512, p=0.0, C=P, ldc=512)
    a.update(kw)
    return lib.rsx_gemm_x3_relu_train(a["A"], a["lda"], a["B"], a["ldb"], None, a["M"], a["N"], a["K"], a["aux"],
                                      a["ldaux"], a["p"], 0, a["C"], a["ldc"], None, 0, None)


def test_relu_train_rejects_bad_arguments():
    lib = _lib()
    for kw, msg in (({"aux": None}, b"needs aux"), ({"ldaux": 256}, b"needs aux"), ({"ldaux": 514}, b"needs aux"),
                    ({"aux": Q}, b"needs aux"), ({"C": Q}, b"C must be"), ({"A": None}, b"null tensor"),
                    ({"C": None}, b"null tensor"), ({"N": 96}, b"multiple of 128"), ({"K": 100}, b"multiple of 128"),
                    ({"lda": 64}, b"leading dimensions"), ({"p": 1.0}, b"p_drop"), ({"p": -0.1}, b"p_drop"),
                    ({"M": 1 << 24}, b"2^32")):
        assert _relu_train(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
    assert _relu_train(lib, M=0) == 0   # no rows: nothing is launched


def _nce_fwd(lib, flags, k1=P):
    return lib.rsx_nce_fwd(P, P, None, k1, k1, None, None, 4, 4, 128, 128, 0, 0.1, flags, 8, P, P, None)


def test_label_without_bias_flag_is_valid_only_with_the_item_mask():
    lib = _lib()
    assert ops.NCE_MASK_ITEM_POS == 18 and ops.NCE_MASK_ITEM == 2
    for flags in (16, 17, 19, 22, 24, 25, 26, 32, 3):
        assert _nce_fwd(lib, flags) == 1, flags
        assert b"unsupported flag combination" in lib.rsx_last_error(), flags
        assert lib.rsx_nce_fwd_x3(P, P, None, P, P, None, None, 4, 4, 128, 128, 0, 0.1, flags, P, P, None) == 1
        assert b"unsupported flag combination" in lib.rsx_last_error(), flags
        assert lib.rsx_nce_bwd(P, P, None, P, P, None, None, 4, 4, 128, 128, 0, 0.1, flags, 8, 8, P, P, P, P, 0,
                               None) == 1
        assert b"unsupported flag combination" in lib.rsx_last_error(), flags
        assert lib.rsx_nce_bwd_x3(P, P, None, P, P, None, None, 4, 4, 128, 128, 0, 0.1, flags, P, P, P, P, 0,
                                  None) == 1
        assert b"unsupported flag combination" in lib.rsx_last_error(), flags
    # 18 passes the flag check: the next check (its keys) is the one that answers
    assert _nce_fwd(lib, 18, k1=None) == 1 and b"k1 keys required" in lib.rsx_last_error()
    assert lib.rsx_nce_fwd_x3(P, P, None, None, None, None, None, 4, 4, 128, 128, 0, 0.1, 18, P, P, None) == 1
    assert b"k1 keys required" in lib.rsx_last_error()


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("lam", [0.0, 0.1])
def test_losses_on_cpu_tensors_match_float64(B, lam):
    u, v, pos, probs, log_q = LR.make_case(B, seed=B)
    for fn, ref, table, tau in ((MI.logq_correction_loss, LR.logq_correction, probs, 0.07),
                                (MI.efficient_corrected_logq_loss, LR.efficient_corrected_logq, log_q, 0.1)):
        ug, vg = u.clone().requires_grad_(), v.clone().requires_grad_()
        got = fn(ug, vg, pos, table, temperature=tau, lambda_logq=lam)
        got.backward()
        ur, vr = u.clone().requires_grad_(), v.clone().requires_grad_()
        want = ref(ur, vr, pos, table, tau, lam)
        want.backward()
        got, want = float(got.detach()), float(want.detach())
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (fn.__name__, got, want)
        for a, r in ((ug.grad, ur.grad), (vg.grad, vr.grad)):
            assert float((a.double() - r).abs().max()) <= 1e-5 * float(r.abs().max()) + 1e-9, fn.__name__


def test_loss_defaults_are_the_reference_ones():
    import inspect
    a = inspect.signature(MI.logq_correction_loss).parameters
    assert list(a) == ["user_emb", "item_emb", "pos_item_ids", "item_probs", "temperature", "lambda_logq"]
    assert a["temperature"].default == 0.07 and a["lambda_logq"].default == 0.0
    b = inspect.signature(MI.efficient_corrected_logq_loss).parameters
    assert list(b) == ["user_emb", "item_emb", "pos_item_ids", "precomputed_log_q", "temperature", "lambda_logq"]
    assert b["temperature"].default == 0.1 and b["lambda_logq"].default == 0.1


def test_efficient_loss_reports_an_id_outside_the_table_on_cpu():
    u, v, pos, _, log_q = LR.make_case(5, seed=1)
    pos[2] = log_q.numel()
    with pytest.raises(IndexError):
        MI.efficient_corrected_logq_loss(u, v, pos, log_q)


def test_ffn_relu_on_cpu_keeps_the_unfused_form():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(3, 128, generator=g, requires_grad=True)
    w1, w2 = torch.randn(512, 128, generator=g) / 11, torch.randn(128, 512, generator=g) / 22
    out = ops.ffn(h, w1, None, w2, None, p_drop=0.0, training=True, act="relu")
    want = torch.relu(h.detach() @ w1.T) @ w2.T
    assert torch.allclose(out.detach(), want, atol=1e-5)
    out.sum().backward()
    assert h.grad is not None


# ---------------------------------------------------------------- the module's dispatch, without a GPU
def test_native_train_ok_is_false_on_cpu_and_for_l65():
    from tests import hybrid_ref as R
    m = R.build(MI.HybridUserTower)
    for L, lengths in ((7, (7, 3)), (65, (65, 3))):
        inp = R.make_inputs(2, L, lengths, seed=4)
        assert not m.native_train_ok(inp["seq_ids"]) and not m.native_ok(inp["seq_ids"])
        m.train()
        assert not m.native_train_ok(inp["seq_ids"])
        m.eval()
    assert MI.HybridUserTower.native_training is True

    class OnDevice:   # the predicate reads attributes only: a stand-in for a device tensor
        is_cuda = True

        def __init__(self, L):
            self.shape = (2, L)

        def dim(self):
            return 2

    # CPU weights: false whatever the ids are
    assert not m.native_train_ok(OnDevice(7)) and not m.native_train_ok(OnDevice(65))


# ------------------------------------------------- argument checks of the adapter / fusion training entries
def _adapter_train(lib, **kw):
    a = dict(content=P, ldc=128, Dc=128, Dg=64, ids=P, R=8, wc=P, p=0.0, merged=P, seq_in=None, deltas=None, xc=P,
             zg=P)
    a.update(kw)
    return lib.rsx_hybrid_adapter_train_fwd(a["content"], a["ldc"], 41, a["Dc"], P, 64, 41, a["Dg"], a["ids"], a["R"],
                                            a["wc"], P, P, P, P, P, P, P, 1e-5, a["deltas"], None, 1.0, a["p"], 1, 2,
                                            a["merged"], a["seq_in"], a["xc"], P, P, a["zg"], P, None)


def test_adapter_train_rejects_bad_arguments():
    lib = _lib()
    for kw, msg in (({"Dc": 64}, b"128 wide"), ({"Dg": 128}, b"64 wide"), ({"ids": None}, b"null tensor (ids)"),
                    ({"content": None}, b"null tensor"), ({"wc": None}, b"null tensor"),
                    ({"merged": None}, b"no output"), ({"seq_in": P}, b"deltas"), ({"ldc": 126}, b"leading dimensions"),
                    ({"p": 1.0}, b"p_drop"), ({"xc": None}, b"saved rows"), ({"zg": Q}, b"16-byte aligned")):
        assert _adapter_train(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
        assert b"rsx_hybrid_adapter_train_fwd" in lib.rsx_last_error()
    assert _adapter_train(lib, R=0, ids=None) == 0


def _adapter_bwd(lib, **kw):
    a = dict(dy=P, R=8, zc=P, p=0.0, dzc=P, dln=P, ws=P, ws_floats=512, eps=1e-5)
    a.update(kw)
    return lib.rsx_hybrid_adapter_bwd(a["dy"], 1.0, a["R"], a["zc"], P, P, P, P, P, P, P, a["eps"], a["p"], 1, 2,
                                      a["dzc"], P, P, P, a["dln"], a["ws"], a["ws_floats"], None)


def test_adapter_bwd_rejects_bad_arguments():
    lib = _lib()
    for kw, msg in (({"R": -1}, b"negative size"), ({"eps": 0.0}, b"eps must be positive"), ({"p": 1.0}, b"p_drop"),
                    ({"dln": None}, b"null tensor"), ({"dy": None}, b"null tensor"), ({"dzc": None}, b"null tensor"),
                    ({"zc": Q}, b"16-byte aligned"), ({"ws": None}, b"workspace"), ({"ws_floats": 511}, b"workspace")):
        assert _adapter_bwd(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
    assert lib.rsx_hybrid_adapter_bwd_workspace_floats(0) == 0
    assert lib.rsx_hybrid_adapter_bwd_workspace_floats(33) == 2 * 512


def _fuse_train(lib, **kw):
    a = dict(seq_out=P, B=2, L=7, u=P, p=0.0, out=P, gate=None, ws=None, ws_bytes=0)
    a.update(kw)
    return lib.rsx_hybrid_fuse_train_fwd(a["seq_out"], a["B"], a["L"], a["u"], P, P, P, P, P, P, P, 1e-5, 1e-12, a["p"],
                                         1, 2, a["out"], None, a["gate"], a["ws"], a["ws_bytes"], P, None)


def _fuse_bwd(lib, **kw):
    a = dict(seq_out=P, B=2, L=7, p=0.0, dout=P, dv=None, dx=P, dsmall=P, ws=P, ws_floats=2 * 14 * 128 + 386)
    a.update(kw)
    return lib.rsx_hybrid_fuse_bwd(a["seq_out"], a["B"], a["L"], P, P, P, P, P, P, P, P, 1e-5, 1e-12, a["p"], 1, 2,
                                   a["dout"], a["dv"], a["dx"], P, P, P, a["dsmall"], a["ws"], a["ws_floats"], None)


def test_fuse_train_and_bwd_reject_bad_arguments():
    lib = _lib()
    for kw, msg in (({"L": 65}, b"L must be"), ({"L": 0}, b"L must be"), ({"seq_out": None}, b"null tensor"),
                    ({"u": None}, b"null tensor"), ({"out": None}, b"null tensor"), ({"gate": P}, b"workspace"),
                    ({"p": 1.0}, b"p_drop")):
        assert _fuse_train(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
        assert b"rsx_hybrid_fuse_train_fwd" in lib.rsx_last_error()
    for kw, msg in (({"L": 65}, b"L must be"), ({"B": -1}, b"negative size"), ({"p": -0.5}, b"p_drop"),
                    ({"dsmall": None}, b"null tensor"), ({"dout": None}, b"null tensor"),
                    ({"dx": None}, b"null tensor"),
                    ({"dv": Q}, b"16-byte aligned"), ({"ws": None}, b"workspace"),
                    ({"ws_floats": 2 * 14 * 128 + 385}, b"workspace")):
        assert _fuse_bwd(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
    assert lib.rsx_hybrid_fuse_bwd_workspace_floats(2, 7) == 2 * 14 * 128 + 386
    assert lib.rsx_hybrid_fuse_bwd_workspace_floats(0, 7) == 0


def test_training_ops_reject_cpu_tensors_and_bad_shapes():
    z = torch.zeros
    params = [z(128, 128), z(128), z(128), z(128), z(128, 64), z(128), z(128), z(128)]
    with pytest.raises(ValueError):
        ops.hybrid_adapter_train(z(4, 64), z(4, 64), None, torch.zeros(2, dtype=torch.long), None, params)
    with pytest.raises(ValueError):
        ops.hybrid_adapter_train(z(4, 128), z(4, 64), None, torch.zeros(2, dtype=torch.long), None, params[:7])
    with pytest.raises(ValueError):
        ops.hybrid_adapter_train(z(4, 128), z(4, 64), None, torch.zeros(2, dtype=torch.long),
                                 torch.zeros(2, dtype=torch.long), params)     # deltas without time_tab
    with pytest.raises(TypeError):
        ops.hybrid_adapter_train(z(4, 128), z(4, 64), None, torch.zeros(2), None, params)
    with pytest.raises(ValueError):
        ops.hybrid_fuse_train(z(2, 65, 128), z(2, 128), z(2, 128), z(64, 128), z(64), z(2, 64), z(2), z(128), z(128))
    with pytest.raises(ValueError):
        ops.hybrid_fuse_train(z(2, 7, 128), z(3, 128), z(2, 128), z(64, 128), z(64), z(2, 64), z(2), z(128), z(128))
    with pytest.raises(ValueError):
        ops.hybrid_fuse_train(z(2, 7, 128), z(2, 128), z(2, 128), z(64, 128), z(64), z(2, 64), z(2), z(128), z(128),
                              p_drop=1.0)
