"""HybridUserTower's adapter and fusion with gradients on the device (ops.hybrid_adapter_train,
ops.hybrid_fuse_train; csrc/hybrid.hip) against tests/hybrid_train_ref.py: float64 with host-rebuilt keep
masks, autograd's gradients.

Bounds. The kernels multiply on the exact fp32 MFMA: forward as tests/test_gpu_hybrid.py (1e-6 at a row's
own scale, max(1, |row|); unit rows 1e-6 absolute), every gradient within 1e-4 of its float64 maximum
(GRAD_TOL of tests/test_gpu_distill.py and test_gpu_lightgcl.py). The same bounds hold with dropout on.
"""
import math

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import hybrid_ref as R
from tests import hybrid_train_ref as TR

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
KERNEL_UNIT_ATOL = 1e-6
SCALE = math.sqrt(128.0)
N_TAB = 41


def _grad_check(what, names, got, want):
    for name, a, r in zip(names, got, want):
        assert a is not None, (what, name)
        err, top = float((a.detach().cpu().double() - r).abs().max()), float(r.abs().max())
        print(f"    {what} d {name}: max err {err:.3e}, max |f64| {top:.3e}")
        assert err <= GRAD_TOL * top + 1e-30, (what, name, err, top)


# ------------------------------------------------------------------------------------------ adapter
def _adapter_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    gu, gi, ct = R.make_tables(N_TAB, 6, seed=77)
    time_tab = 0.5 * torch.randn(1001, 128, generator=g)
    ids = torch.randint(0, N_TAB, (n,), generator=g)
    ids[0] = 0                       # id 0 is an ordinary row
    if n > 2:
        ids[n - 1] = ids[1]          # repeats
        ids[n // 2] = 0
    deltas = torch.randint(0, 1200, (n,), generator=g)
    for j, d in enumerate((0, 1, 1000, 1001, 50000)[:n]):   # three of them land in time row 1000
        deltas[j] = d
    params = [torch.randn(128, 128, generator=g) / math.sqrt(128), 0.1 * torch.randn(128, generator=g),
              1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g),
              torch.randn(128, 64, generator=g) / 8, 0.1 * torch.randn(128, generator=g),
              1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)]
    dy = torch.randn(n, 128, generator=g)
    return ct, gi, time_tab, ids, deltas, params, dy


ADAPTER_NAMES = ["content", "gnn", "time", "wc", "bc", "lnc_w", "lnc_b", "wg", "bg", "lng_w", "lng_b"]


def _adapter_ref(case, p, seeds, merged, wrong=None):
    ct, gi, tt, ids, deltas, params, dy = case
    leaves = [t.double().requires_grad_() for t in (ct, gi, tt, *params)]
    out = TR.adapter(leaves[0], leaves[1], leaves[2], ids, None if merged else deltas, leaves[3:], p, seeds,
                     scale=SCALE, wrong=wrong)
    (out * dy.double()).sum().backward()
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]
    return out.detach(), grads


def _adapter_dev(case, gpu, p, torch_seed, merged):
    ct, gi, tt, ids, deltas, params, dy = case
    leaves = [t.to(gpu).requires_grad_() for t in (ct, gi, tt, *params)]
    torch.manual_seed(torch_seed)
    out = ops.hybrid_adapter_train(leaves[0], leaves[1], None if merged else leaves[2], ids.to(gpu),
                                   None if merged else deltas.to(gpu), leaves[3:], scale=SCALE, p_drop=p,
                                   training=True)
    (out * dy.to(gpu)).sum().backward()
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_adapter_train_forward_and_gradients(gpu, n, p):
    case = _adapter_case(n, seed=n)
    s = TR.draw_seeds(2, 900 + n)
    seeds = {"content": s[0], "gnn": s[1]}
    state = torch.random.get_rng_state()
    out, grads = _adapter_dev(case, gpu, p, 900 + n, merged=False)
    if p == 0:    # no seed is drawn at p = 0: the generator stands where manual_seed left it
        assert ops.next_seed() == s[0]
    torch.random.set_rng_state(state)
    want, ref = _adapter_ref(case, p, seeds, merged=False)
    rows = (want / SCALE).norm(dim=1, keepdim=True).clamp_min(1.0)
    err = (out.cpu().double() - want).abs() / SCALE
    print(f"adapter train n={n} p={p}: forward max err / sqrt(128) {float(err.max()):.3e}")
    assert bool((err <= KERNEL_UNIT_ATOL * rows).all())
    # every gradient: three tables, eight adapter tensors; the time table's is exact sums of dy rows
    _grad_check(f"adapter n={n} p={p}", ADAPTER_NAMES, grads, ref)
    assert float(grads[2][1000].abs().max()) > 0 or n < 3
    # the same call again: identical bits
    out2, grads2 = _adapter_dev(case, gpu, p, 900 + n, merged=False)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    if p > 0 and n > 1:
        bad, _ = _adapter_ref(case, p, seeds, merged=False, wrong="gnn")
        assert float((out.cpu().double() - bad).abs().max()) > 1e-2     # the wrong seed breaks agreement
    ops._HYBRID_IDS.check()


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_adapter_train_merged_form(gpu, p):
    case = _adapter_case(33, seed=5)
    s = TR.draw_seeds(2, 17)
    out, grads = _adapter_dev(case, gpu, p, 17, merged=True)
    want, ref = _adapter_ref(case, p, {"content": s[0], "gnn": s[1]}, merged=True)
    rows = want.norm(dim=1, keepdim=True).clamp_min(1.0)
    assert bool(((out.cpu().double() - want).abs() <= KERNEL_UNIT_ATOL * rows).all())
    assert grads[2] is None                     # no time table in the merged form
    names = [n for n in ADAPTER_NAMES if n != "time"]
    _grad_check(f"adapter merged p={p}", names, grads[:2] + grads[3:], ref[:2] + ref[3:])


@pytest.mark.parametrize("site", ["content", "gnn"])
def test_adapter_train_kept_fraction_on_the_device(gpu, site):
    """The kept fraction of each dropout site, counted on the device's output: the other branch's LayerNorm
    weight and bias are zero, so it gives gelu(0) = 0 exactly and merged - c is the site's dropped branch
    alone ((0 + c) + 0 - c = 0 exactly where dropped). Counted where float64's branch value is at least 1e-3
    (a kept entry then differs from 0 by far more than the rounding of the sum with c)."""
    n, p = 257, 0.3
    ct, gi, tt, ids, _, params, _ = _adapter_case(n, seed=11)
    other = (6, 7) if site == "content" else (2, 3)
    params[other[0]], params[other[1]] = torch.zeros(128), torch.zeros(128)
    dev = [t.to(gpu) for t in (ct, gi, *params)]
    torch.manual_seed(5)
    out = ops.hybrid_adapter_train(dev[0], dev[1], None, ids.to(gpu), None, dev[2:], p_drop=p, training=True)
    branch = (out.cpu() - ct[ids]).double()
    P = [t.double() for t in params]
    if site == "content":
        y = R.gelu(R.layer_norm(ct[ids].double() @ P[0].T + P[1], P[2], P[3]))
    else:
        y = R.gelu(R.layer_norm(gi[ids].double() @ P[4].T + P[5], P[6], P[7]))
    big = y.abs() >= 1e-3
    cnt = int(big.sum())
    kept = float((branch[big] != 0).double().mean())
    sigma = math.sqrt(p * (1 - p) / cnt)
    print(f"adapter {site} site: kept {kept:.4f} of {cnt} entries (1 - p = {1 - p}, sigma {sigma:.4f})")
    assert cnt > 10000 and abs(kept - (1 - p)) <= 4 * sigma, (kept, cnt)
    # the kept entries carry the factor 1 / (1 - p)
    sel = big & (branch != 0)
    assert float((branch[sel] * (1 - p) - y[sel]).abs().max()) <= 1e-5


def test_adapter_train_backward_stays_in_bounds_for_an_id_out_of_range(gpu):
    """An id outside the tables followed by backward(): the op replaces the id by 0 before the forward and
    saves the replaced ids, so the forward reads row 0 and the table gradients' scatter writes row 0. The
    IndexError arrives at the first point where the guard's flag is visible: inside the call, at a later
    call or at check(); whichever it is, nothing was read or written outside a table."""
    ct, gi, tt, ids, deltas, params, dy = _adapter_case(33, seed=8)
    bad = ids.clone()
    bad[2], bad[7] = N_TAB + 5, -3
    good = ids.clone()
    good[2], good[7] = 0, 0
    # what the op hands its kernels and saves for the backward
    replaced = ops._HYBRID_IDS(bad.to(gpu), N_TAB)
    assert torch.equal(replaced.cpu(), good)
    with pytest.raises(IndexError):
        ops._HYBRID_IDS.check()

    def run(which):
        leaves = [t.to(gpu).requires_grad_() for t in (ct, gi, tt, *params)]
        out = ops.hybrid_adapter_train(leaves[0], leaves[1], leaves[2], which.to(gpu), deltas.to(gpu), leaves[3:],
                                       scale=SCALE)
        (out * dy.to(gpu)).sum().backward()
        return [t.grad for t in leaves]

    with pytest.raises(IndexError):
        run(bad)
        ops._HYBRID_IDS.check()
    torch.cuda.synchronize()          # no fault was left behind; the device still works
    ops._HYBRID_IDS.pending.clear()   # drop what the interrupted call left queued
    grads = run(good)
    ops._HYBRID_IDS.check()
    for a, t in zip(grads, (ct, gi, tt, *params)):
        assert a.shape == t.shape and bool(torch.isfinite(a).all())


def test_adapter_train_eval_mode_matches_the_inference_kernel(gpu):
    """No seed, no mask; the two kernels are separate instantiations (the compiler may contract their
    multiply-adds differently), so they agree to the kernels' forward bound, not bit for bit."""
    ct, gi, tt, ids, deltas, params, _ = _adapter_case(33, seed=6)
    dev = [t.to(gpu) for t in (ct, gi, tt, *params)]
    state = torch.random.get_rng_state()
    out = ops.hybrid_adapter_train(dev[0], dev[1], dev[2], ids.to(gpu), deltas.to(gpu), dev[3:], scale=SCALE,
                                   p_drop=0.3, training=False)
    assert torch.equal(torch.random.get_rng_state(), state)     # eval mode draws no seed
    _, _, want = ops.hybrid_adapter(dev[0], dev[1], ops.AdapterParams(*dev[3:]), ids=ids.to(gpu),
                                    deltas=deltas.to(gpu), time_tab=dev[2], scale=SCALE, want_merged=False)
    rows = (want / SCALE).norm(dim=1, keepdim=True).clamp_min(1.0)
    assert bool(((out - want).abs() / SCALE <= KERNEL_UNIT_ATOL * rows).all())


def test_adapter_train_reports_ids_out_of_range(gpu):
    ct, gi, tt, ids, deltas, params, _ = _adapter_case(5, seed=7)
    ids[2] = N_TAB
    dev = [t.to(gpu) for t in (ct, gi, tt, *params)]
    with pytest.raises(IndexError):   # inside the call if the flag is already visible, else at check()
        ops.hybrid_adapter_train(dev[0], dev[1], dev[2], ids.to(gpu), deltas.to(gpu), dev[3:], scale=SCALE)
        ops._HYBRID_IDS.check()
    ops._HYBRID_IDS.pending.clear()


# ------------------------------------------------------------------------------------------- fusion
def _fusion_case(B, L, init_gate, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, 128, generator=g) * (0.25 + 4.0 * torch.rand(B, L, 1, generator=g))
    zero_row = None
    if B * L > 1:
        zero_row = (B - 1, L // 2)
        x[zero_row] = 0.0            # a padded position: |x| = 0
    t = [x, torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g),
         torch.randn(64, 128, generator=g) / math.sqrt(128), 0.1 * torch.randn(64, generator=g),
         torch.randn(2, 64, generator=g) / 8, 0.1 * torch.randn(2, generator=g),
         1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)]
    if init_gate:   # the reference's initial gate
        t[5], t[6] = torch.zeros(2, 64), torch.full((2,), -5.0)
    dout, dv = torch.randn(B, L, 128, generator=g), torch.randn(B, L, 128, generator=g)
    if zero_row is not None:
        dout[zero_row] = 0.0
        dv[zero_row] = 0.0
    return t, dout, dv, zero_row


FUSE_NAMES = ["seq_out", "u_gnn", "u_meta", "w1", "b1", "w2", "b2", "ln_w", "ln_b"]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("init_gate", [False, True])
@pytest.mark.parametrize("L", [1, 7, 50, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_fuse_train_forward_and_gradients(gpu, B, L, init_gate, p):
    tensors, dout, dv, zero_row = _fusion_case(B, L, init_gate, seed=10 * B + L)
    s = TR.draw_seeds(2, 300 + L)
    seeds = {"gnn": s[0], "meta": s[1]}
    for with_dv in (True, False):
        lv = [t.double().requires_grad_() for t in tensors]
        out_r, v_r, g_r = TR.fuse(*lv, p=p, seeds=seeds)
        ((out_r * dout.double()).sum() + ((v_r * dv.double()).sum() if with_dv else 0.0)).backward()
        ref = [t.grad if t.grad is not None else torch.zeros_like(t) for t in lv]

        def run():
            dl = [t.to(gpu).requires_grad_() for t in tensors]
            torch.manual_seed(300 + L)
            out, v, gate = ops.hybrid_fuse_train(*dl, p_drop=p, training=True)
            assert not gate.requires_grad
            ((out * dout.to(gpu)).sum() + ((v * dv.to(gpu)).sum() if with_dv else 0.0)).backward()
            return out.detach(), v.detach(), gate, [t.grad for t in dl]

        out, v, gate, grads = run()
        what = f"fuse B={B} L={L} init={init_gate} p={p} dv={with_dv}"
        for name, a, r in (("out", out, out_r), ("v", v, v_r)):
            err = float((a.cpu().double() - r.detach()).abs().max())
            print(f"{what} {name}: max err {err:.3e}")
            assert err <= KERNEL_UNIT_ATOL, (what, name)
        want_gate = g_r.detach().reshape(-1, 2).mean(0)
        assert float((gate.cpu().double() - want_gate).abs().max()) <= 1e-6
        for a in grads:
            assert bool(torch.isfinite(a).all()), what
        if init_gate:
            # w2 = 0: nothing reaches w1 / b1 (exact zeros on both sides); skip their relative bound
            assert float(grads[3].abs().max()) == 0.0 and float(ref[3].abs().max()) == 0.0
            keep = [i for i in range(9) if i not in (3, 4)]
            _grad_check(what, [FUSE_NAMES[i] for i in keep], [grads[i] for i in keep], [ref[i] for i in keep])
        else:
            _grad_check(what, FUSE_NAMES, grads, ref)
        if zero_row is not None:    # the padded position with zero upstream gradients: exact zeros
            assert float(grads[0][zero_row].abs().max()) == 0.0
        out2, v2, gate2, grads2 = run()
        assert torch.equal(out, out2) and torch.equal(v, v2) and torch.equal(gate, gate2)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    if p > 0 and B * L > 1:
        bad, _, _ = TR.fuse(*[t.double() for t in tensors], p=p, seeds=seeds, wrong="meta")
        assert float((out.cpu().double() - bad).abs().max()) > 1e-3


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fuse_train_user_gradients_are_sums_over_the_users_rows(gpu, p):
    """d u_gnn and d u_meta of a batch are, bit for bit, the fp32 sums in position order of the single-token
    contributions of the user's own L rows. A token's contribution is what the same call gives when dout is
    zero everywhere else (a row's gradients depend on that row's dout alone, and the other rows then add
    exact zeros); the token keeps its row index, so its keep masks are the batch's."""
    B, L = 3, 7
    tensors, dout, _, _ = _fusion_case(B, L, False, seed=3)

    def run(d):
        dl = [t.to(gpu).requires_grad_() for t in tensors]
        torch.manual_seed(41)
        out, _, _ = ops.hybrid_fuse_train(*dl, p_drop=p, training=True)
        (out * d.to(gpu)).sum().backward()
        return dl[1].grad.clone(), dl[2].grad.clone()

    full_g, full_m = run(dout)
    sum_g = torch.zeros(B, 128, device=gpu)
    sum_m = torch.zeros(B, 128, device=gpu)
    for b in range(B):
        for l in range(L):
            one = torch.zeros_like(dout)
            one[b, l] = dout[b, l]
            g, m = run(one)
            others = [u for u in range(B) if u != b]
            assert float(g[others].abs().max()) == 0.0 and float(m[others].abs().max()) == 0.0
            sum_g[b] += g[b]
            sum_m[b] += m[b]
    assert float(full_g.abs().max()) > 0 and float(full_m.abs().max()) > 0
    assert torch.equal(full_g, sum_g) and torch.equal(full_m, sum_m)


def test_fuse_train_eval_mode_matches_the_inference_kernel(gpu):
    tensors, _, _, _ = _fusion_case(3, 50, False, seed=4)
    dl = [t.to(gpu) for t in tensors]
    state = torch.random.get_rng_state()
    out, v, gate = ops.hybrid_fuse_train(*dl, p_drop=0.1, training=False)
    assert torch.equal(torch.random.get_rng_state(), state)
    o2, v2, g2 = ops.hybrid_fuse(*dl)
    for a, b in ((out.view(-1, 128), o2), (v.view(-1, 128), v2), (gate, g2)):
        assert float((a - b).abs().max()) <= KERNEL_UNIT_ATOL
