"""HybridUserTower's two in-batch losses on the device (tower_code/mined_inference.py: ops.nce_sum flags 2
and 18) against tests/tower_loss_ref.py, the float64 restatement of the reference's formulas with their
finite collision fills: loss within 1e-5 relative, both input gradients within 1e-3 of their maximum, for
the bf16x3 and the fp32 products of the plain kernels."""
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.tower_code import mined_inference as MI
from tests import tower_loss_ref as LR

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_TOL = 1e-3


@pytest.fixture(params=["bf16x3", "fp32"])
def precision(request):
    prev = ops.set_nce_precision(request.param)
    yield request.param
    ops.set_nce_precision(prev)


def _check(what, got, ug, vg, want, ur, vr):
    got, want = float(got.detach()), float(want.detach())
    rel = abs(got - want) / abs(want)
    print(f"{what}: loss {got:.7f} (f64 {want:.7f}, rel {rel:.2e})")
    assert rel <= LOSS_RTOL, what
    for name, a, r in (("d user", ug.grad, ur.grad), ("d item", vg.grad, vr.grad)):
        err, top = float((a.cpu().double() - r).abs().max()), float(r.abs().max())
        print(f"    {name}: max err {err:.3e}, max |f64| {top:.3e}")
        assert err <= GRAD_TOL * top, (what, name)


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("lam", [0.0, 0.1])
def test_losses_match_float64(gpu, precision, B, lam):
    u, v, pos, probs, log_q = LR.make_case(B, seed=B)
    if B > 1:
        assert pos.unique().numel() < B   # repeated positives: the collision mask is exercised
    for fn, ref, table, tau in ((MI.logq_correction_loss, LR.logq_correction, probs, 0.07),
                                (MI.efficient_corrected_logq_loss, LR.efficient_corrected_logq, log_q, 0.1)):
        ug, vg = u.to(gpu).requires_grad_(), v.to(gpu).requires_grad_()
        got = fn(ug, vg, pos.to(gpu), table.to(gpu), temperature=tau, lambda_logq=lam)
        assert "_NCE" in type(got.grad_fn.next_functions[0][0]).__name__   # the fused kernels, not a matmul
        got.backward()
        ur, vr = u.clone().requires_grad_(), v.clone().requires_grad_()
        want = ref(ur, vr, pos, table, tau, lam)
        want.backward()
        if B == 1:   # one row: the loss is log 1 = 0 and so are the gradients
            assert abs(float(got.detach())) <= 1e-6 and float(ug.grad.abs().max()) <= 1e-6
            assert float(want.detach()) == 0.0
            continue
        _check(f"{fn.__name__} B={B} lambda={lam} {precision}", got, ug, vg, want, ur, vr)
    ops._LOGQ_IDS.check()


@pytest.mark.parametrize("B", [5, 130])
def test_flags_18_is_flags_2_with_the_bias_put_back_on_the_diagonal(gpu, precision, B):
    """With all-distinct ids no column is masked, so the logits of flags 18 are those of flags 2 plus
    diag(bias). Both sums are held to float64 over the written-out matrices, and so is their difference
    (the part the flag changes)."""
    u, v, _, _, log_q = LR.make_case(B, seed=7 + B, n_items=B)
    pos = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    bias = 0.1 * log_q[pos]
    ud, vd, posd, bd = u.to(gpu), v.to(gpu), pos.to(gpu), bias.to(gpu)
    s18, n18 = ops.nce_sum(ud, vd, bd, k1a=posd, k1b=posd, tau=0.1, flags=ops.NCE_MASK_ITEM_POS)
    s2, n2 = ops.nce_sum(ud, vd, bd, k1a=posd, k1b=posd, tau=0.1, flags=ops.NCE_MASK_ITEM)
    assert float(n18) == B and float(n2) == B
    S = (u.double() @ v.double().T) / 0.1 - bias.double()[None, :]
    eye = torch.eye(B, dtype=torch.bool)
    S18 = torch.where(eye, S + bias.double()[None, :], S)
    lab = torch.arange(B)
    want2 = torch.nn.functional.cross_entropy(S, lab, reduction="sum")
    want18 = torch.nn.functional.cross_entropy(S18, lab, reduction="sum")
    print(f"B={B} {precision}: flags 2 {float(s2):.6f} (f64 {float(want2):.6f}), "
          f"flags 18 {float(s18):.6f} (f64 {float(want18):.6f})")
    assert abs(float(s2) - float(want2)) <= LOSS_RTOL * float(want2)
    assert abs(float(s18) - float(want18)) <= LOSS_RTOL * float(want18)
    assert abs((float(s18) - float(s2)) - float(want18 - want2)) <= 2 * LOSS_RTOL * float(want18)


def test_an_id_outside_the_table_raises_index_error(gpu):
    u, v, pos, probs, log_q = LR.make_case(5, seed=3)
    pos[2] = log_q.numel()
    for fn, table in ((MI.efficient_corrected_logq_loss, log_q), (MI.logq_correction_loss, probs)):
        loss = fn(u.to(gpu), v.to(gpu), pos.to(gpu), table.to(gpu), lambda_logq=0.1)
        assert torch.isfinite(loss)          # the read was clamped: no fault, a finite value
        with pytest.raises(IndexError):
            ops._LOGQ_IDS.check()
    ops._LOGQ_IDS.check()                     # the guard is clean again


def test_losses_fall_back_for_other_widths(gpu):
    g = torch.Generator().manual_seed(0)
    u, v = torch.randn(6, 64, generator=g), torch.randn(6, 64, generator=g)
    pos = torch.tensor([1, 2, 3, 1, 0, 4])
    log_q = torch.log(torch.full((5,), 0.2))
    got = MI.efficient_corrected_logq_loss(u.to(gpu), v.to(gpu), pos.to(gpu), log_q.to(gpu))
    want = LR.efficient_corrected_logq(u, v, pos, log_q)
    assert abs(float(got) - float(want)) <= 1e-4 * abs(float(want))
