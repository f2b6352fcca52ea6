"""The ReLU feed-forward with gradients on the device: rsx_gemm_x3_relu_train (forward, the 0/1 mask it
saves, its dropout keep mask) and ops._FFN / ops.ffn(act="relu") against float64 with host-rebuilt masks.

Bounds. Integer-valued operands and half-integer biases are exact in the bf16 split and in the fp32 sums,
so those cases are compared for equality. Through the bf16x3 GEMMs: forward atol 2e-5 + rtol 1e-4,
gradients 2e-3 max|grad| + 1e-6 (tests/test_gpu_tower.py). ReLU makes the gradient discontinuous in the
pre-activation, so every gradient case asserts in float64 that |z| >= 1e-4 (5x the forward atol) for
every pre-activation: no unit can round across 0. The seeds of the random cases were searched on the CPU
for that condition and are pinned.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import dropout_ref as DR

pytestmark = pytest.mark.gpu

X3_ATOL, X3_RTOL = 2e-5, 1e-4
Z_MIN = 1e-4
SEED = 0x1234567855AA


def _keep_scale(seed, p, M, n):
    """[M, n] float64: keep / (1 - p) of the GEMM epilogues (index m * n + col), the fp32 scale."""
    return torch.from_numpy(DR.keep(seed, p, DR.gemm_index(M, n)).astype(np.float64) * float(DR.scale32(p)))


def _int_case(M, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, k), generator=g).float()
    w = torch.randint(-2, 3, (n, k), generator=g).float()
    b = torch.randint(-4, 4, (n,), generator=g).float() + 0.5    # half-integers: z is never 0
    return a, w, b


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("M", [1, 127, 129])
@pytest.mark.parametrize("NK", [(512, 128), (128, 512)])
def test_relu_train_forward_is_exact_on_integers(gpu, M, NK, p):
    n, k = NK
    a, w, b = _int_case(M, n, k, seed=M + n)
    z = a.double() @ w.double().T + b.double()
    assert bool((z != 0).all()) and bool((z < 0).any()) and bool((z > 0).any())
    aux = torch.full((M, n), 7.0, device=gpu)
    got = ops.gemm_x3_relu_train(a.to(gpu), w.to(gpu), b.to(gpu), aux, p, SEED)
    assert torch.equal(aux.cpu().double(), (z > 0).double())
    # fp32 relu(z) times the fp32 keep scale, as the epilogue multiplies
    want = (torch.relu(z).float() * _keep_scale(SEED, p, M, n).float()).double()
    assert torch.equal(got.cpu().double(), want)
    if p > 0:
        kept = float((got.cpu()[z > 0] != 0).double().mean())
        cnt = int((z > 0).sum())
        assert abs(kept - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / cnt), (kept, cnt)
    again = ops.gemm_x3_relu_train(a.to(gpu), w.to(gpu), b.to(gpu), torch.empty_like(aux), p, SEED)
    assert torch.equal(again, got)


def test_relu_train_backward_epilogue_takes_the_saved_mask(gpu):
    """epi 2 over the saved mask: dZ = (dC W2) * keep / (1 - p) * (z > 0), exact on integers."""
    M, n, k, p = 129, 512, 128, 0.3
    a, w, b = _int_case(M, n, k, seed=5)
    aux = torch.empty(M, n, device=gpu)
    ops.gemm_x3_relu_train(a.to(gpu), w.to(gpu), b.to(gpu), aux, p, SEED)
    g = torch.Generator().manual_seed(6)
    df = torch.randint(-2, 3, (M, 128), generator=g).float()
    w2 = torch.randint(-2, 3, (128, n), generator=g).float()
    got = ops.gemm_x3_tn(df.to(gpu), w2.to(gpu), ops.EPI_DGELU_DROP, aux, p, SEED)
    z = a.double() @ w.double().T + b.double()
    want = ((df.double() @ w2.double()).float() * (z > 0).float() * _keep_scale(SEED, p, M, n).float()).double()
    assert torch.equal(got.cpu().double(), want)


def _ffn_reference(tensors, gy, p, seed):
    lv = [t.double().requires_grad_() for t in tensors]
    z = F.linear(lv[0], lv[1], lv[2])
    y = F.linear(torch.relu(z) * _keep_scale(seed, p, z.shape[0], z.shape[1]), lv[3], lv[4])
    (y * gy.double()).sum().backward()
    return z.detach(), [y.detach()] + [t.grad for t in lv]


def _float_case(M, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, 128, generator=g)
    w1, b1 = torch.randn(512, 128, generator=g) / math.sqrt(128), 0.1 * torch.randn(512, generator=g)
    w2, b2 = torch.randn(128, 512, generator=g) / math.sqrt(512), 0.1 * torch.randn(128, generator=g)
    return [h, w1, b1, w2, b2], torch.randn(M, 128, generator=g)


def _int_ffn_case(M, seed):
    h, w1, b1 = _int_case(M, 512, 128, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w2, b2 = torch.randn(128, 512, generator=g) / math.sqrt(512), 0.1 * torch.randn(128, generator=g)
    return [h, w1, b1, w2, b2], torch.randn(M, 128, generator=g)


FLOAT_SEEDS = {1: 0, 9: 1}   # M -> torch seed with min |z| >= 1e-4 (searched on the CPU)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("case", ["float1", "float9", "int1", "int127", "int129"])
def test_ffn_relu_value_and_gradients(gpu, case, p):
    M = int(case.lstrip("floatin"))
    tensors, gy = _float_case(M, FLOAT_SEEDS[M]) if case.startswith("float") else _int_ffn_case(M, 40 + M)
    z, refs = _ffn_reference(tensors, gy, p, SEED)
    print(f"ffn relu {case} p={p}: min |z| {float(z.abs().min()):.3g}")
    assert float(z.abs().min()) >= Z_MIN
    dv = [t.to(gpu).requires_grad_() for t in tensors]
    y = ops._FFN.apply(*dv, p, SEED, "relu")
    (y * gy.to(gpu)).sum().backward()
    got = [y] + [t.grad for t in dv]
    _, bad = _ffn_reference(tensors, gy, p, SEED + 1)
    worst = 0.0
    for name, a, r, rb in zip(["y", "dh", "dw1", "db1", "dw2", "db2"], got, refs, bad):
        err = (a.detach().cpu().double() - r).abs()
        if name == "y" and case.startswith("float"):
            bound = X3_ATOL + X3_RTOL * r.abs()
        else:   # gradients; and the integer cases' y, whose scale (|z| up to hundreds) is not a unit one
            bound = torch.full_like(r, 2e-3 * float(r.abs().max()) + 1e-6)
        print(f"    {name}: max err {float(err.max()):.3e}, max |f64| {float(r.abs().max()):.3e}")
        assert bool((err <= bound).all()), (case, p, name)
        worst = max(worst, float(((a.detach().cpu().double() - rb).abs() / bound).max()))
    if p > 0 and M > 1:
        print(f"    control (seed + 1): excess {worst:.1f}")
        assert worst >= 100.0, worst
    # the same call again: identical bits, value and gradients
    dv2 = [t.to(gpu).requires_grad_() for t in tensors]
    y2 = ops._FFN.apply(*dv2, p, SEED, "relu")
    (y2 * gy.to(gpu)).sum().backward()
    assert torch.equal(y2, y) and all(torch.equal(a.grad, b.grad) for a, b in zip(dv, dv2))


def test_ffn_relu_with_gradients_runs_the_fused_pair(gpu):
    tensors, _ = _float_case(9, FLOAT_SEEDS[9])
    dv = [t.to(gpu) for t in tensors]
    h = dv[0].view(1, 9, 128).clone().requires_grad_()
    torch.manual_seed(11)
    out = ops.ffn(h, *dv[1:], p_drop=0.3, training=True, act="relu")
    assert "_FFN" in type(out.grad_fn).__name__ or "_FFN" in type(out.grad_fn.next_functions[0][0]).__name__
    # the seed is the generator's next draw: the same generator state gives the same mask
    torch.manual_seed(11)
    seed = ops.next_seed()
    want = ops._FFN.apply(dv[0], *dv[1:], 0.3, seed, "relu")
    assert torch.equal(out.detach().view(9, 128), want)
    # eval mode draws no seed and drops nothing
    state = torch.random.get_rng_state()
    ev = ops.ffn(h, *dv[1:], p_drop=0.3, training=False, act="relu")
    assert torch.equal(torch.random.get_rng_state(), state)
    with torch.no_grad():
        inf = ops.ffn(h, *dv[1:], p_drop=0.3, training=False, act="relu")
    assert torch.equal(ev.detach(), inf)
