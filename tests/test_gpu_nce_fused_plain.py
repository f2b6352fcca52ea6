"""The plain-family view of the fused grouped kernels (ops.nce_sum(precision="bf16x3" | "f16"):
rsx_nce_fwd_grad / rsx_nce_bwd_cols) against float64, for flags 0 (DuoRec-unsup) and 9 (SupCon).

Shapes: the smallest at which the pieces can go wrong -- 128-row owner blocks, 32-column tiles, the 8
column / row splits' boundaries and the tail geometry (N = M in {1, 33, 129, 300, 1029}), and one
multi-rank shape (N = 96 rows of M = 288 columns, diag_offset = 96).
Keys of flags 9: all zero (N = 1: no valid row), all singletons (N = 33: no valid row), a mix of zeros,
singletons and pairs (N = 129), one key with 40 members beside zeros and small groups (N = 300; its
positives span tiles), random keys with a 100-member key spread over the whole batch (N = 1029; its
positives span splits and owner blocks).
Bounds (the project's: oracle/agreement.py LOSS_TOL / GRAD_TOL, the `check` of tests/test_gpu_nce_paths.py):
mean loss within 1e-4 absolute, each gradient within 1e-3 of its scale max|ref|; n_valid exact. Where the
reference gradient is identically zero because no row is valid, the kernels' must be exactly zero.
N = M = 1 at flags 0 also has a zero reference gradient, but by cancellation: the one column's softmax
weight 1 against the label's -1, two terms of size GOUT max|x| / tau each. A bound relative to max|ref| = 0
is undefined there, so that case is held to the number format instead: the view carries every product to
2^-16 relative (bf16 hi + lo: 16 significand bits), so |err| <= 2^-16 GOUT max|x| / tau.

Both precision names run the same kernels: the view forms bf16x3 products in the "f16" mode too. The f16
mode's own products (one fp16 MFMA per gradient product, weights and rows rounded to 11 bits) were built
and measured on these cases first and missed the near-converged case, where the gradient is what is
left after the softmax-weighted sum of B's rows cancels against the label / the positives' mean: an
absolute error of ~3.6e-4 whatever the scale, dA 1.25e-3 of scale at flags 0 and 2.45e-2 at flags 9 (bf16x3:
3.2e-5 and 6.7e-4). So the view does not offer them, and "f16" stays a case here to pin that choice.
At bf16x3 the same bounds also hold against ops.nce_sum(precision=None) (the plain kernels), and the
measured error against float64 is printed beside the plain kernels' own atol 2e-6 / rtol 1e-4."""
import functools

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops, synth
from recsys_amd.tower_code import v1_usertower_train as TT
from tests.helpers import paired_towers, small_cfg, small_universe, to_dev

pytestmark = pytest.mark.gpu

TAU = 0.1
GOUT = 0.37  # upstream gradient of the row-loss sum
LOSS_TOL = 1e-4
GRAD_TOL = 1e-3


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _keys(n, m, off):
    """(k1a [n], k1b [m]) of the case; rows are columns off .. off + n - 1."""
    g = torch.Generator().manual_seed(100 + m)
    if m == 1:
        kb = torch.zeros(1, dtype=torch.int64)
    elif m == 33:
        kb = torch.arange(1, m + 1)
    elif m == 129:
        kb = torch.arange(1, m + 1)
        kb[:20] = 0
        kb[40:80] = torch.arange(40) // 2 + 500  # pairs
    elif m == 300:
        kb = torch.randint(1, 60, (m,), generator=g)
        kb[::9] = 0
        kb[torch.randperm(m, generator=g)[:40]] = 777  # > 32 members
        kb[5] = 9999  # a singleton
    elif m == 288:
        kb = torch.randint(0, 40, (m,), generator=g)
    else:
        kb = torch.randint(0, 200, (m,), generator=g)
        kb[torch.randperm(m, generator=g)[:100]] = 4242
        kb[7] = 99999
    return kb[off:off + n].clone(), kb


@functools.lru_cache(maxsize=None)
def _case(n, m, off, flags, same, kind):
    """Inputs and the float64 reference, computed once per case: (A, B, k1a, k1b, mean, n_valid, dA, dB).
    same: A is B (one leaf, its gradient the sum of both sides')."""
    g = torch.Generator().manual_seed(7 * n + m + off)
    if kind == "converged":
        # clusters of 5 rows around unit centres; A ~ B: every row's softmax sits on its own cluster
        centres = _unit(torch.randn((m + 4) // 5, 128, generator=g, dtype=torch.float64))
        B = _unit(centres.repeat_interleave(5, 0)[:m] + 0.02 * torch.randn(m, 128, generator=g, dtype=torch.float64))
        A = _unit(B[off:off + n] + 0.005 * torch.randn(n, 128, generator=g, dtype=torch.float64))
        kb = torch.arange(m) // 5 + 1
        ka = kb[off:off + n].clone()
    else:
        B = _unit(torch.randn(m, 128, generator=g, dtype=torch.float64))
        A = B if same else _unit(torch.randn(n, 128, generator=g, dtype=torch.float64))
        ka, kb = _keys(n, m, off)
    A32 = A.float()
    B32 = A32 if same else B.float()
    Ad = A32.double().requires_grad_()
    Bd = Ad if same else B32.double().requires_grad_()
    S = Ad @ Bd.T / TAU
    diag = torch.arange(n)[:, None] + off == torch.arange(m)[None, :]
    if flags == 0:
        rows = torch.logsumexp(S, 1) - S[diag]
        valid = torch.ones(n, dtype=torch.bool)
    else:
        lse = torch.logsumexp(S.masked_fill(diag, float("-inf")), 1)
        pos = (ka[:, None] == kb[None, :]) & (ka[:, None] != 0) & ~diag
        cnt = pos.sum(1)
        valid = cnt > 0
        rows = torch.where(valid, lse - (S * pos).sum(1) / cnt.clamp(min=1), torch.zeros_like(lse))
    total = rows[valid].sum() if valid.any() else (S * 0).sum()
    (total * GOUT).backward()
    nv = int(valid.sum())
    dA = Ad.grad
    dB = None if same else Bd.grad
    return A32, B32, ka, kb, total.item() / max(nv, 1), nv, dA, dB


def _run(gpu, case, flags, off, same, precision):
    A32, B32, ka, kb = case[:4]
    A = A32.to(gpu).requires_grad_()
    B = A if same else B32.to(gpu).requires_grad_()
    k = (None, None) if flags == 0 else (ka.to(gpu), kb.to(gpu))
    ops.timing_start()
    total, cnt = ops.nce_sum(A, B, None, k[0], k[1], tau=TAU, flags=flags, diag_offset=off, tag="t", precision=precision)
    (total * GOUT).backward()
    timers = ops.timing_stop()
    # the fused path ran (no row pass) exactly when a precision was given
    assert ("t/nce_bwd_rows" in timers) == (precision is None), sorted(timers)
    nv = int(cnt.item())
    return total.item() / max(nv, 1), nv, A.grad.double().cpu(), None if same else B.grad.double().cpu()


def _check(name, got, ref, report, cancel_floor=0.0, scale_of=None):
    """cancel_floor: the bound where the reference vanishes by cancellation (module docstring); 0 where it
    vanishes because no row is valid. scale_of: the tensor whose max|.| is the scale (default: ref; the
    cross-check against the plain kernels keeps the float64 reference's scale)."""
    scale = (ref if scale_of is None else scale_of).abs().max().item()
    err = (got - ref).abs().max().item()
    report.append(f"{name}: max|err| {err:.3e} scale {scale:.3e} rel {err / max(scale, 1e-30):.3e}")
    if scale == 0.0:
        assert err <= cancel_floor, f"{name}: reference gradient is zero, got max |g| = {err} > {cancel_floor}"
    else:
        assert err <= GRAD_TOL * scale, f"{name}: {err} > {GRAD_TOL} * {scale}"
    return err, scale


def _compare(gpu, n, m, off, flags, same, kind, precision):
    case = _case(n, m, off, flags, same, kind)
    mean_r, nv_r, dA_r, dB_r = case[4:]
    mean, nv, dA, dB = _run(gpu, case, flags, off, same, precision)
    xmax = max(case[0].abs().max().item(), case[1].abs().max().item())
    floor = 2.0 ** -16 * GOUT * xmax / TAU if (flags == 0 and m == 1) else 0.0
    report = [f"n={n} m={m} off={off} flags={flags} same={same} {kind} {precision}: "
              f"loss {mean:.7f} ref {mean_r:.7f} |diff| {abs(mean - mean_r):.3e} n_valid {nv}"]
    try:
        assert nv == nv_r
        assert abs(mean - mean_r) <= LOSS_TOL, (mean, mean_r)
        _check("dA", dA, dA_r, report, floor)
        if not same:
            _check("dB", dB, dB_r, report, floor)
        if precision == "bf16x3":
            # the plain kernels on the same inputs, same bounds; and whether the fused route meets the
            # plain kernels' own tolerance (atol 2e-6 / rtol 1e-4) against float64: reported, not asserted
            mean_p, nv_p, dA_p, dB_p = _run(gpu, case, flags, off, same, None)
            assert nv == nv_p and abs(mean - mean_p) <= LOSS_TOL
            _check("dA vs plain", dA, dA_p, report, floor, dA_r)
            if not same:
                _check("dB vs plain", dB, dB_p, report, floor, dB_r)
            pairs = [(dA, dA_r)] + ([] if same else [(dB, dB_r)])
            tight = all(bool(((a - b).abs() <= 2e-6 + 1e-4 * b.abs()).all()) for a, b in pairs)
            report.append(f"meets the plain kernels' atol 2e-6 / rtol 1e-4: {tight}")
    finally:
        print("\n".join(report))


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("n", [1, 33, 129, 300, 1029])
def test_fused_plain_flags0(gpu, n, precision):
    _compare(gpu, n, n, 0, 0, False, "gauss", precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("n", [1, 33, 129, 300, 1029])
def test_fused_plain_flags9(gpu, n, same, precision):
    _compare(gpu, n, n, 0, 9, same, "gauss", precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("flags", [0, 9])
def test_fused_plain_multi_rank(gpu, flags, precision):
    _compare(gpu, 96, 288, 96, flags, False, "gauss", precision)


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("flags", [0, 9])
def test_fused_plain_near_converged(gpu, flags, precision):
    _compare(gpu, 300, 300, 0, flags, False, "converged", precision)


def test_fused_plain_falls_back(gpu):
    """Unsupported cases keep the plain kernels: another flag combination, a bias with flags 9, fp32,
    and rows that need no gradient."""
    g = torch.Generator().manual_seed(3)
    A = _unit(torch.randn(40, 128, generator=g)).to(gpu)
    k = torch.randint(0, 5, (40,), generator=g).to(gpu)
    bias = torch.zeros(40, device=gpu)
    for kw, grad in [(dict(flags=2, k1a=k, k1b=k, precision="f16"), True),
                     (dict(flags=9, k1a=k, k1b=k, bias=bias, precision="f16"), True),
                     (dict(flags=0, precision="fp32"), True), (dict(flags=0, precision="f16"), False)]:
        a = A.clone().requires_grad_(grad)
        b = A.clone().requires_grad_()
        ops.timing_start()
        total, _ = ops.nce_sum(a, b, tau=TAU, tag="t", **kw)
        total.backward()
        timers = ops.timing_stop()
        assert ("t/nce_bwd_rows" in timers) == grad and "t/nce_fwd" in timers, (kw, sorted(timers))


def test_step_terms_agree_and_skip_the_row_pass(gpu):
    """contrastive_losses and dist.contrastive_objective_dp choose the two small terms' kernels the same
    way (equal cl on the 64-user batch of test_dp_objective_single_rank_equals_single_gpu_step), and in
    f16 mode (the step's default) the DuoRec and SupCon terms run no row pass."""
    from recsys_amd import dist as Dd
    assert ops.nce_precision() == "f16"
    cfg = small_cfg(num_items=500)
    items = small_universe(500)
    bd = to_dev(synth.make_batch(items, 64, seed=21), gpu)
    _, dut = paired_towers(cfg, gpu)
    dut.train()
    it = TT.SASRecItemTower(500, 128, items.log_q.clone()).to(gpu)
    it.init_from_pretrained(items.pretrained.to(gpu))
    it.set_freeze_state(False)
    pv = TT.lookup_pretrained(items.pretrained.to(gpu), bd["item_ids"])
    _, _, cl = TT.contrastive_losses(dut, it, it.log_q, bd, cfg, pv)
    ops.timing_start()
    obj, _, _, cl2 = Dd.contrastive_objective_dp(dut, it, it.log_q, bd, cfg, pretrained_vecs=pv)
    obj.backward()
    timers = ops.timing_stop()
    print(f"cl {cl.item():.7f} dp {cl2.item():.7f}; timers {sorted(t for t in timers if '/nce_' in t)}")
    assert abs(cl.item() - cl2.item()) < 1e-5
    assert "duorec/nce_fwd" in timers and "duorec/nce_bwd_cols" in timers
    assert "duorec/nce_bwd_rows" not in timers and "supcon/nce_bwd_rows" not in timers
