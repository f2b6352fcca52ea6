"""HybridUserTower with gradients on the device, end to end, against tests/hybrid_train_ref.py (float64,
every dropout mask rebuilt on the host from the replayed seeds).

Bounds: the path runs through the bf16x3 encoder, so the project's bf16x3 bounds hold (tests/
test_gpu_tower.py): forward atol 2e-5 + rtol 1e-4, in eval and in training mode alike, gradients 2e-3 max|grad| + 1e-6 per tensor. ReLU makes the gradient discontinuous in the feed-forward
pre-activations, so each gradient case asserts in float64 that |z| >= 1e-4 at every valid token; the inputs
(tests/hybrid_ref.make_inputs seeds) and, with dropout, the torch seeds were searched on the CPU for that.
"""
import functools

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.tower_code import mined_inference as MI
from tests import hybrid_ref as R
from tests import hybrid_train_ref as TR

pytestmark = pytest.mark.gpu

X3_ATOL, X3_RTOL = 2e-5, 1e-4
Z_MIN = 1e-4
# (B, L, lengths, make_inputs seed, torch seed for training mode)
CASES = {"b2l7": (2, 7, (7, 3), 24, 24), "b3l9": (3, 9, (9, 4, 1), 23, 31)}
DEAD = ("gnn_projector.", "gnn_user_emb.")   # reference :672: no gradient reaches them


@functools.lru_cache(maxsize=None)
def _cpu_model():
    return R.build(MI.HybridUserTower)


def _dev_model(gpu, training):
    m = R.build(MI.HybridUserTower).to(gpu)
    return m.train() if training else m.eval()


def _call(m, inp, gpu):
    d = {k: v.to(gpu) for k, v in inp.items()}
    return m(d["u_idx"], d["seq_ids"], d["seq_deltas"], d["seq_mask"], d["u_dense"], d["u_cat"])


def _weights(inp, seed):
    g = torch.Generator().manual_seed(seed)
    B, L = inp["seq_ids"].shape
    return torch.randn(B, L, 128, generator=g) * R.valid(inp["seq_mask"])[..., None]


def _run_dev(gpu, inp, training, torch_seed, w):
    m = _dev_model(gpu, training)
    torch.manual_seed(torch_seed)
    out, v, ratios = _call(m, inp, gpu)
    (out * w.to(gpu)).sum().backward()
    return m, out.detach(), v.detach(), ratios


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_module_forward_and_every_gradient(gpu, case, training):
    B, L, lengths, in_seed, torch_seed = CASES[case]
    inp = R.make_inputs(B, L, lengths, seed=in_seed)
    val = R.valid(inp["seq_mask"])
    w = _weights(inp, 5)
    seeds = TR.module_seeds(torch_seed, training)
    P = TR.leaves(_cpu_model())
    out_r, v_r, g_r, zs = TR.module_forward(P, inp, training, seeds)
    zmin = float(zs[:, val].abs().min())
    print(f"{case} training={training}: min |z| at valid tokens {zmin:.3g}")
    assert zmin >= Z_MIN
    (out_r * w.double()).sum().backward()

    m, out, v, ratios = _run_dev(gpu, inp, training, torch_seed, w)
    assert m.native_train_ok(inp["seq_ids"].to(gpu)) and not m.native_ok(inp["seq_ids"].to(gpu))
    for name, a, r in (("output", out, out_r), ("v_seq", v, v_r)):
        err = (a.cpu().double() - r.detach()).abs()[val]
        print(f"    {name}: max err {float(err.max()):.3e}")
        assert bool((err <= X3_ATOL + X3_RTOL * r.detach().abs()[val]).all()), name
    want_ratio = g_r.detach().reshape(-1, 2).mean(0).tolist()
    assert max(abs(a - b) for a, b in zip(ratios, want_ratio)) <= 1e-5, (ratios, want_ratio)
    for name, p in m.named_parameters():
        if name.startswith(DEAD) or name == "logit_scale":
            assert p.grad is None, name
            continue
        r = P[name].grad if P[name].grad is not None else torch.zeros_like(P[name])
        assert p.grad is not None, name
        err, top = float((p.grad.cpu().double() - r).abs().max()), float(r.abs().max())
        print(f"    d {name}: max err {err:.3e}, max |f64| {top:.3e}")
        assert err <= 2e-3 * top + 1e-6, (name, err, top)
    assert float(m.fusion_layer.gnn_proj[0].weight.grad.abs().max()) == 0.0   # a zero input: exact zeros
    # the same call again: identical bits
    m2, out2, v2, ratios2 = _run_dev(gpu, inp, training, torch_seed, w)
    assert torch.equal(out, out2) and torch.equal(v, v2) and ratios == ratios2
    for (n1, p1), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None and p2.grad is None) or torch.equal(p1.grad, p2.grad), n1
    if training:   # negative control: one site's seed off by one breaks the agreement
        bad, _, _, _ = TR.module_forward(TR.leaves(_cpu_model()), inp, True, seeds, wrong="ffn2")
        assert float((out.cpu().double() - bad.detach()).abs()[val].max()) > 1e-3


def test_native_training_false_gives_the_composition(gpu):
    B, L, lengths, in_seed, _ = CASES["b2l7"]
    inp = R.make_inputs(B, L, lengths, seed=in_seed)
    m = _dev_model(gpu, False)
    m.native_training = False
    assert not m.native_train_ok(inp["seq_ids"].to(gpu))
    out, _, _ = _call(m, inp, gpu)
    want, _, _ = m._torch_forward(*[inp[k].to(gpu) for k in ("u_idx", "seq_ids", "seq_deltas", "seq_mask", "u_dense",
                                                              "u_cat")])
    assert torch.equal(out, want)
    assert MI.HybridUserTower.native_training is True    # the class default is untouched


@pytest.mark.parametrize("shape", [(3, 50, (50, 17, 1)), (2, 64, (33, 64))])
def test_training_mode_forward_at_long_lengths(gpu, shape):
    B, L, lengths = shape
    inp = R.make_inputs(B, L, lengths, seed=7)
    val = R.valid(inp["seq_mask"])
    seeds = TR.module_seeds(3, True)
    with torch.no_grad():
        out_r, v_r, g_r, _ = TR.module_forward(TR.leaves(_cpu_model()), inp, True, seeds)
    m = _dev_model(gpu, True)
    torch.manual_seed(3)
    with torch.no_grad():
        out, v, ratios = _call(m, inp, gpu)
    for name, a, r in (("output", out, out_r), ("v_seq", v, v_r)):
        err = (a.cpu().double() - r).abs()[val]
        print(f"L={L} {name}: max err {float(err.max()):.3e}")
        assert bool((err <= X3_ATOL + X3_RTOL * r.abs()[val]).all()), name


def _adamw_step(gpu, inp, targets, log_q, last, lr, tau, lam, native):
    """The parameters after one AdamW step of the module on the device (native path or composition)."""
    B = inp["seq_ids"].shape[0]
    m = _dev_model(gpu, False)
    m.native_training = native
    opt = torch.optim.AdamW(m.parameters(), lr=lr)
    out, _, _ = _call(m, inp, gpu)
    ad = m.seq_adapter
    params = [ad.content_proj[0].weight, ad.content_proj[0].bias, ad.content_proj[1].weight, ad.content_proj[1].bias,
              ad.gnn_proj[0].weight, ad.gnn_proj[0].bias, ad.gnn_proj[1].weight, ad.gnn_proj[1].bias]
    if native:
        items = ops.l2_normalize(ops.hybrid_adapter_train(m.item_content_emb.weight, m.gnn_item_emb.weight, None,
                                                          targets.to(gpu), None, params, training=False))
    else:
        items = torch.nn.functional.normalize(ad(m.item_content_emb(targets.to(gpu)), m.gnn_item_emb(targets.to(gpu))),
                                              p=2, dim=1)
    loss = MI.efficient_corrected_logq_loss(out[torch.arange(B, device=gpu), last.to(gpu)], items, targets.to(gpu),
                                            log_q.to(gpu), tau, lam)
    loss.backward()
    opt.step()
    return {n: p.detach().cpu().double() for n, p in m.named_parameters()}


def test_one_adamw_step_on_the_efficient_loss(gpu):
    """Last-position outputs against l2_normalize(hybrid_adapter_train(targets)) under
    efficient_corrected_logq_loss, one AdamW step (lr 1e-3), against the same step in float64, wherever the
    float64 gradient exceeds 1e-6 of its tensor's maximum. The bound is one figure for the whole step: 1e-5,
    which neither path meets, so 8x the largest error of the module's PyTorch-fp32 composition on the same GPU
    in the same run (the fallback DESIGN.md section 4 names). Measured: native 1.08e-4 (layer 2's in_proj
    weight), composition 9.49e-5 (layer 2's out_proj weight), so a bound of 7.6e-4; every bias, LayerNorm
    vector, embedding table and the user side stay below 1e-5 on both paths. Why 1e-5 is out of reach of either:
    AdamW's first step is lr g / (|g| + 1e-8); the encoder's weight gradients reach 2e-3 at most here, so the
    mask keeps entries down to 2e-9, where the step turns an absolute gradient error dg into lr dg / 1e-8:
    1e-5 asks for dg <= 1e-10, five parts in 1e8 of the tensor's largest gradient, below fp32 accumulation."""
    B, L, lengths, in_seed, _ = CASES["b2l7"]
    inp = R.make_inputs(B, L, lengths, seed=in_seed)
    targets = torch.tensor([5, 9])
    log_q = torch.log(torch.linspace(0.5, 1.5, R.N_ITEMS) / R.N_ITEMS)
    last = torch.tensor([n - 1 for n in lengths])
    lr, tau, lam = 1e-3, 0.1, 0.1

    P = TR.leaves(_cpu_model())
    out_r, _, _, zs = TR.module_forward(P, inp, False, TR.module_seeds(0, False))
    assert float(zs[:, R.valid(inp["seq_mask"])].abs().min()) >= Z_MIN
    items_r = R.normalize(TR.adapter(P["item_content_emb.weight"], P["gnn_item_emb.weight"], None, targets, None,
                                     [P[k] for k in TR.ADAPTER_KEYS]))
    from tests import tower_loss_ref as LR
    LR.efficient_corrected_logq(out_r[torch.arange(B), last], items_r, targets, log_q, tau, lam).backward()

    native = _adamw_step(gpu, inp, targets, log_q, last, lr, tau, lam, True)
    plain = _adamw_step(gpu, inp, targets, log_q, last, lr, tau, lam, False)
    rows = []
    for name in native:
        g = P[name].grad
        if g is None or name.startswith(DEAD):
            continue
        # AdamW's first step in float64: p (1 - lr wd) - lr g / (|g| + eps)
        want = P[name].detach() * (1 - lr * 0.01) - lr * g / (g.abs() + 1e-8)
        sel = g.abs() > 1e-6 * g.abs().max()
        if not bool(sel.any()):
            continue
        err = float((native[name] - want)[sel].abs().max())
        err_plain = float((plain[name] - want)[sel].abs().max())
        print(f"    step {name}: native {err:.3e}, composition {err_plain:.3e}, max |g| {float(g.abs().max()):.3e}, "
              f"{int(sel.sum())} entries")
        rows.append((name, err, err_plain))
    assert len(rows) >= 30
    bound = max(1e-5, 8 * max(r[2] for r in rows))
    worst = max(rows, key=lambda r: r[1])
    print(f"    bound {bound:.3e}; worst native {worst[0]} {worst[1]:.3e}")
    assert worst[1] <= bound, (worst, bound)
