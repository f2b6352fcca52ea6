"""HybridUserTower on the device against tests/hybrid_ref.py (float64): the adapter kernel, the ReLU
epilogue of rsx_gemm_x3, the fusion kernel, the module end to end, and its vectors fed to the ensemble
evaluator.

Bounds. csrc/hybrid.hip multiplies on the exact fp32 MFMA, so its kernels are held to the bound of
tests/test_gpu_distill.py's forward: 1e-6 absolute on unit vectors (KERNEL_UNIT_ATOL). merged and
seq_in / sqrt(128) are not unit rows; unit = merged / |merged|, so the same bound at a row's own scale is
1e-6 max(1, |merged row|) per element. The ReLU epilogue and the end-to-end run go through the bf16x3
GEMMs and attention: the project's bf16x3 forward bound, atol 2e-5 and rtol 1e-4
(tests/test_gpu_tower.py).
"""
import functools
import math

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.tower_code import mined_inference as MI
from tests import ensemble_ref as EREF
from tests import hybrid_ref as R

pytestmark = pytest.mark.gpu

KERNEL_UNIT_ATOL = 1e-6
X3_ATOL, X3_RTOL = 2e-5, 1e-4
SCALE = math.sqrt(128.0)


@functools.lru_cache(maxsize=None)
def _cpu_model(n_items=R.N_ITEMS, n_users=R.N_USERS):
    return R.build(MI.HybridUserTower, n_items, n_users)


@functools.lru_cache(maxsize=None)
def _sd(n_items=R.N_ITEMS, n_users=R.N_USERS):
    return R.f64(_cpu_model(n_items, n_users).state_dict())


_DEV = {}


def _model(gpu, n_items=R.N_ITEMS, n_users=R.N_USERS):
    key = (n_items, n_users)
    if key not in _DEV:
        m = R.build(MI.HybridUserTower, n_items, n_users)
        _DEV[key] = m.to(gpu).eval()
    return _DEV[key]


def _within_x3(got, want, what):
    err = (got.cpu().double() - want).abs()
    print(f"{what}: max |err| {float(err.max()):.3g}, max |f64| {float(want.abs().max()):.3g}")
    assert bool((err <= X3_ATOL + X3_RTOL * want.abs()).all()), what


def _within_rows(got, want, scale_rows, what):
    """|err| <= 1e-6 max(1, scale_rows) per element, scale_rows [n, 1]."""
    err = (got.cpu().double() - want).abs()
    print(f"{what}: max |err| {float(err.max()):.3g}, max row scale {float(scale_rows.max()):.3g}")
    assert bool((err <= KERNEL_UNIT_ATOL * scale_rows.clamp_min(1.0)).all()), what


# ------------------------------------------------------------------------------------------ adapter
def _adapter_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, R.N_ITEMS, (n,), generator=g)
    ids[0] = 0
    if n >= 3:
        ids[2] = ids[1]
    deltas = torch.tensor([0, 1, 1000, 1001, 50000])[torch.arange(n) % 5]
    return ids, deltas


def _adapter(gpu, **kw):
    m = _model(gpu)
    return ops.hybrid_adapter(m.item_content_emb.weight, m.gnn_item_emb.weight, m.seq_adapter.native_params(),
                              time_tab=m.time_emb.weight, scale=SCALE, want_unit=True, **kw)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_adapter_rows_by_id(gpu, n):
    ids, deltas = _adapter_case(n, n)
    merged, unit, seq_in = _adapter(gpu, ids=ids.to(gpu), deltas=deltas.to(gpu))
    sd = _sd()
    want = R.adapter(sd, ids)
    norm = want.norm(dim=1, keepdim=True)
    assert merged.shape == unit.shape == seq_in.shape == (n, 128)
    _within_rows(unit, R.normalize(want), torch.ones_like(norm), f"unit n={n}")
    _within_rows(merged, want, norm, f"merged n={n}")
    _within_rows(seq_in / SCALE, R.seq_input(sd, ids, deltas) / SCALE, norm, f"seq_in / sqrt(128) n={n}")
    again = _adapter(gpu, ids=ids.to(gpu), deltas=deltas.to(gpu))
    assert all(torch.equal(a, b) for a, b in zip((merged, unit, seq_in), again))
    # the same ids in another order: the same rows, bit for bit (a row does not depend on its tile or slot)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    shuffled = _adapter(gpu, ids=ids[perm].to(gpu), deltas=deltas[perm].to(gpu))
    assert all(torch.equal(a[perm.to(gpu)], b) for a, b in zip((merged, unit, seq_in), shuffled))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 40])
def test_adapter_table_rows_and_gather(gpu, n):
    """ids = None, first_row = 1: rows 1 .. n of the tables; then seq_in as a gather from that table
    equals the per-token form bit for bit."""
    m = _model(gpu)
    merged, unit, none = _adapter(gpu, first_row=1, rows=n)
    assert none is None and merged.shape == (n, 128)
    ids = torch.arange(1, n + 1)
    by_id = _adapter(gpu, ids=ids.to(gpu))
    assert torch.equal(merged, by_id[0]) and torch.equal(unit, by_id[1])
    want = R.adapter(_sd(), ids)
    _within_rows(merged, want, want.norm(dim=1, keepdim=True), f"table merged n={n}")
    g = torch.Generator().manual_seed(n)
    tok = torch.randint(1, n + 1, (3, 11), generator=g)
    deltas = torch.randint(0, 1200, (3, 11), generator=g)
    deltas[0, :5] = torch.tensor([0, 1, 1000, 1001, 50000])
    _, _, per_token = _adapter(gpu, ids=tok.to(gpu), deltas=deltas.to(gpu))
    gathered = ops.hybrid_seq_gather(merged, tok.to(gpu), deltas.to(gpu), m.time_emb.weight, scale=SCALE, first_row=1)
    assert torch.equal(gathered, per_token)
    # the padding id of a table that starts at row 1 reads a zero row: the time row alone
    pad = ops.hybrid_seq_gather(merged, torch.zeros(2, dtype=torch.long, device=gpu),
                                torch.tensor([3, 2000], device=gpu), m.time_emb.weight, scale=SCALE, first_row=1)
    assert torch.equal(pad, m.time_emb.weight.detach()[[3, 1000]])
    ops._HYBRID_IDS.check()


def test_adapter_reports_ids_out_of_range(gpu):
    _adapter(gpu, ids=torch.tensor([1, R.N_ITEMS], device=gpu))
    with pytest.raises(IndexError):
        ops._HYBRID_IDS.check()


# --------------------------------------------------------------------------------------- epilogue 3
@pytest.mark.parametrize("M", [1, 127, 129])
@pytest.mark.parametrize("NK", [(512, 128), (128, 512)])
def test_relu_epilogue(gpu, M, NK):
    n, k = NK
    g = torch.Generator().manual_seed(M + n)
    a, w, b = torch.randn(M, k, generator=g), torch.randn(n, k, generator=g) / math.sqrt(k), torch.randn(n, generator=g)
    got = ops.gemm_x3(a.to(gpu), w.to(gpu), b.to(gpu), ops.EPI_RELU)
    _within_x3(got, torch.relu(a.double() @ w.double().T + b.double()), f"relu epilogue M={M} N={n} K={k}")
    # integer-valued operands are exact in the bf16 split and in the fp32 sums: exact zeros and negatives
    ai = torch.randint(-3, 4, (M, k), generator=g).float()
    wi = torch.randint(-2, 3, (n, k), generator=g).float()
    bi = torch.randint(-4, 5, (n,), generator=g).float()
    wi[0] = 0.0; bi[0] = 0.0      # column 0: every pre-activation exactly 0
    wi[1] = 0.0; bi[1] = -2.0     # column 1: every pre-activation -2
    pre = ai.double() @ wi.double().T + bi.double()
    assert bool((pre == 0).any()) and bool((pre < 0).any()) and bool((pre > 0).any())
    got = ops.gemm_x3(ai.to(gpu), wi.to(gpu), bi.to(gpu), ops.EPI_RELU).cpu()
    assert torch.equal(got.double(), torch.relu(pre))
    assert not bool(torch.signbit(got[pre <= 0]).any())   # +0 where the pre-activation is 0 or negative


def test_ffn_relu_matches_the_unfused_form(gpu):
    g = torch.Generator().manual_seed(3)
    h = torch.randn(2, 9, 128, generator=g)
    w1, b1 = torch.randn(512, 128, generator=g) / math.sqrt(128), 0.1 * torch.randn(512, generator=g)
    w2, b2 = torch.randn(128, 512, generator=g) / math.sqrt(512), 0.1 * torch.randn(128, generator=g)
    want = R.relu_ffn(h.double(), w1.double(), b1.double(), w2.double(), b2.double())
    dev = [t.to(gpu) for t in (h, w1, b1, w2, b2)]
    with torch.no_grad():
        got = ops.ffn(*dev, p_drop=0.3, training=False, act="relu")
    _within_x3(got, want, "ffn relu (fused, no grad)")
    hg = dev[0].clone().requires_grad_(True)
    out = ops.ffn(hg, *dev[1:], p_drop=0.0, training=True, act="relu")    # gradients on: the PyTorch form
    out.sum().backward()
    assert hg.grad is not None
    _within_x3(out.detach(), want, "ffn relu (autograd)")


# ------------------------------------------------------------------------------------------- fusion
def _fusion_case(B, L, init_gate, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, 128, generator=g) * (0.25 + 4.0 * torch.rand(B, L, 1, generator=g))
    if B * L > 1:
        x[B - 1, L // 2] = 0.0    # |x| = 0: the 1e-12 floor
    p = {"u_gnn": torch.randn(B, 128, generator=g), "u_meta": torch.randn(B, 128, generator=g),
         "w1": torch.randn(64, 128, generator=g) / math.sqrt(128), "b1": 0.1 * torch.randn(64, generator=g),
         "w2": torch.randn(2, 64, generator=g) / 8, "b2": 0.1 * torch.randn(2, generator=g),
         "ln_w": 1 + 0.1 * torch.randn(128, generator=g), "ln_b": 0.1 * torch.randn(128, generator=g)}
    if init_gate:   # the reference's initial gate
        p["w2"] = torch.zeros(2, 64)
        p["b2"] = torch.full((2,), -5.0)
    lengths = [(L + 1) // 2, L, 1][:B]
    return x, p, torch.tensor([b * L + n - 1 for b, n in enumerate(lengths)])


@pytest.mark.parametrize("init_gate", [False, True])
@pytest.mark.parametrize("L", [1, 7, 50, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_fusion(gpu, B, L, init_gate):
    x, p, last = _fusion_case(B, L, init_gate, 10 * B + L)
    names = ("u_gnn", "u_meta", "w1", "b1", "w2", "b2", "ln_w", "ln_b")
    want_out, want_v, want_g = R.fuse(x.double(), *(p[k].double() for k in names))
    dev = [p[k].to(gpu) for k in names]
    out, v, gate = ops.hybrid_fuse(x.to(gpu), *dev)
    one = torch.ones(B * L, 1, dtype=torch.float64)
    assert out.shape == v.shape == (B * L, 128) and gate.shape == (2,)
    assert torch.isfinite(out).all() and torch.isfinite(v).all()
    _within_rows(out, want_out.reshape(-1, 128), one, f"fusion out B={B} L={L}")
    _within_rows(v, want_v.reshape(-1, 128), one, f"fusion v B={B} L={L}")
    gerr = (gate.cpu().double() - want_g.reshape(-1, 2).mean(0)).abs().max()
    print(f"gate means {gate.tolist()}, max |err| {float(gerr):.3g}")
    assert float(gerr) <= 1e-6
    again = ops.hybrid_fuse(x.to(gpu), *dev)
    assert all(torch.equal(a, b) for a, b in zip((out, v, gate), again))
    # rows = the last valid positions: those rows of the full pass, bit for bit, and their own gate means
    sub, sub_v, sub_gate = ops.hybrid_fuse(x.to(gpu), *dev, rows=last.to(gpu))
    assert torch.equal(sub, out[last.to(gpu)]) and torch.equal(sub_v, v[last.to(gpu)])
    assert float((sub_gate.cpu().double() - want_g.reshape(-1, 2)[last].mean(0)).abs().max()) <= 1e-6
    only, no_v, no_gate = ops.hybrid_fuse(x.to(gpu), *dev, rows=last.to(gpu), want_v=False, want_gate=False)
    assert no_v is None and no_gate is None and torch.equal(only, sub)
    ops._HYBRID_IDS.check()


# --------------------------------------------------------------------------------------- end to end
def _e2e_inputs(name):
    if name == "golden":
        t, _ = R.load_golden()
        return {k[3:]: v for k, v in t.items() if k.startswith("in.")}
    B, L, lengths = {"b3_l50": (3, 50, (50, 17, 1)), "b2_l64": (2, 64, (33, 64))}[name]
    return R.make_inputs(B, L, lengths, seed=L)


def _to(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


def _order(inp):
    return [inp[k] for k in ("u_idx", "seq_ids", "seq_deltas", "seq_mask", "u_dense", "u_cat")]


@pytest.mark.parametrize("name", ["golden", "b3_l50", "b2_l64"])
def test_module_end_to_end(gpu, name):
    """Measured on the MI355X (max |err| against float64 over valid positions, output / v_seq): see
    DESIGN.md section 4, "HybridUserTower". The plain fp32 PyTorch composition on the same GPU is printed
    beside the native path as the yardstick of the reference arithmetic."""
    inp = _e2e_inputs(name)
    m = _model(gpu)
    d = _to(inp, gpu)
    want_out, want_v, want_ratios = R.forward(_sd(), inp)
    val = R.valid(inp["seq_mask"])
    with torch.no_grad():
        assert m.native_ok(d["seq_ids"])
        out, v, ratios = m(*_order(d))
        t_out, t_v, t_ratios = m._torch_forward(*_order(d))
    B, L = inp["seq_ids"].shape
    assert out.shape == v.shape == (B, L, 128) and torch.isfinite(out).all()
    for what, got, torch_got, want in (("output", out, t_out, want_out), ("v_seq", v, t_v, want_v)):
        e_native = float((got.cpu().double() - want)[val].abs().max())
        e_torch = float((torch_got.cpu().double() - want)[val].abs().max())
        print(f"{name} {what}: native max |err| {e_native:.3g}, PyTorch fp32 on the GPU {e_torch:.3g}")
        _within_x3(got[val.to(gpu)], want[val], f"{name} {what}")
    print(f"{name} gate ratios: native {ratios}, PyTorch {t_ratios}, f64 {want_ratios}")
    assert all(abs(a - b) <= X3_ATOL + X3_RTOL * abs(b) for a, b in zip(ratios, want_ratios))
    # encode_users: the last valid position's row of the full forward, bit for bit, from either sequence input
    last = inp["seq_mask"].sum(1) - 1
    rows = out[torch.arange(B, device=gpu), last.to(gpu)]
    merged, unit = MI.hybrid_item_vectors(m)
    assert merged.shape == (R.N_ITEMS - 1, 128)
    assert torch.equal(MI.encode_users(m, *_order(d)), rows)
    assert torch.equal(MI.encode_users(m, *_order(d), merged=merged), rows)
    ops._HYBRID_IDS.check()


def test_module_with_gradients_takes_the_pytorch_composition(gpu):
    inp = _to(_e2e_inputs("golden"), gpu)
    m = _model(gpu)
    assert not m.native_ok(inp["seq_ids"])    # gradients are enabled here
    out, _, _ = m(*_order(inp))
    assert out.requires_grad


# ---------------------------------------------------------------------------------- into the evaluators
def test_vectors_feed_the_ensemble_evaluator(gpu):
    n_users, n_items, L = 40, 300, 12
    m = _model(gpu, n_items + 1, n_users)
    g = torch.Generator().manual_seed(77)
    lengths = torch.randint(1, L + 1, (n_users,), generator=g).tolist()
    inp = R.make_inputs(n_users, L, lengths, n_items=n_items + 1, n_users=n_users, seed=9)
    inp["u_idx"] = torch.arange(n_users)
    merged, item_unit = MI.hybrid_item_vectors(m)
    assert item_unit.shape == (n_items, 128)
    users = MI.encode_users(m, *_order(_to(inp, gpu)), merged=merged)
    gnn_u = torch.nn.functional.normalize(torch.randn(n_users, 64, generator=g), dim=1).to(gpu)
    gnn_i = torch.nn.functional.normalize(torch.randn(n_items, 64, generator=g), dim=1).to(gpu)
    top = torch.topk(users @ item_unit.T, 4, dim=1).indices.cpu().tolist()
    gt = {u: ({top[u][3], int(u * 7 % n_items)} if u % 3 else {int(u * 11 % n_items)}) for u in range(n_users)}
    k_list = [5, 20]
    got = MI.evaluate_weighted_score_ensemble(users, item_unit, gnn_u, gnn_i, gt, gpu, k_list=k_list, batch_size=16,
                                              candidate_pool_size=50, assume_normalized=True)
    as_np = lambda t: t.cpu().numpy().astype(np.float32)  # noqa: E731
    want = EREF.evaluate_fused(as_np(users), as_np(item_unit), as_np(gnn_u), as_np(gnn_i), gt, k_list, 0.1, 50,
                               EREF.MINMAX)
    assert got["users"] == want["users"] == n_users
    assert got["hits"] == want["hits"] and got["best_alpha"] == want["best_alpha"]
    assert sum(got["hits"][0.0].values()) > 0    # the sequence retriever alone finds its own fourth-best item
    ops._HYBRID_IDS.check()
