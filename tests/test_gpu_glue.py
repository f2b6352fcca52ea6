"""The small kernels between the large ones, each against a float64 restatement: the LayerNorm
family (ln.hip), row gather / scatter, segment sums, loss_combine and ids_check (rows.hip), the
cross network (dcn.hip) and the packed BERT embedding (item_re.hip).

Comparison rule (one helper, `_cmp`, per output tensor):
  * results that arithmetic makes exact (gathers, scatters, x + res at p = 0, a kept dropout
    element res * float32(1 / (1 - p)), masks, ids_check, sums of dyadic inputs) are compared
    with torch.equal;
  * everything else: the formula is evaluated in float64 and once more in plain fp32 torch on the
    CPU (the fp32 restatement, which never involves the kernel), and
        max|kernel - f64| <= 8 * max|fp32 restatement - f64| + 8 * 2^-24 * max|f64|.
    The factor 8 allows for a different summation order and the device's erff / __expf against
    libm; a wrong formula or index (biased / unbiased variance, a misplaced eps, a mask indexed by
    the wrong element, a dropped row, a missing segment tail) lands orders of magnitude outside.
Run with -s to see both errors and their ratio per tensor, and the largest ratio per test.
Largest kernel / fp32-restatement error ratios seen on an MI355X: LayerNorm edge rows 2.7,
backward multi-iteration 2.3, forward grid-stride 1.3, inference form 1.5; gathers 1.6; segment
sums 3.4, segment mean 2.6; loss_combine 1.5; BERT embedding 1.2; cross network 3.7 on x_out, 1.2
on the head at B >= 1031 and up to 14 on one- and three-row head outputs whose fp32 restatement happened to land within 4e-9 of
float64 (those pass on the 2^-24 term). No output needed a widening, the GELU gradient included.

No test passes an out-of-range index, a too-short buffer or a wrong dtype to a kernel; the
refusal tests cover only arguments that the host code rejects before launching.
"""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_U = 2.0 ** -24
_RATIO = [0.0]


@pytest.fixture(autouse=True)
def _ratio_report(request):
    _RATIO[0] = 0.0
    yield
    print(f"\n[max ratio] {request.node.name}: {_RATIO[0]:.2f}")


def _cmp(name, got, f64, f32):
    """The comparison rule for one tensor: kernel result, float64 reference, fp32 restatement."""
    got = got.detach().cpu()
    f64, f32 = f64.detach(), f32.detach()
    assert got.dtype == F32 and f64.dtype == F64 and f32.dtype == F32, name
    assert tuple(got.shape) == tuple(f64.shape), (name, tuple(got.shape), tuple(f64.shape))
    if f64.numel() == 0:
        return
    assert torch.isfinite(got).all(), name
    ek = (got.double() - f64).abs().max().item()
    er = (f32.double() - f64).abs().max().item()
    bound = 8.0 * er + 8.0 * _U * f64.abs().max().item()
    ratio = ek / er if er > 0 else (0.0 if ek == 0 else math.inf)
    if math.isfinite(ratio):
        _RATIO[0] = max(_RATIO[0], ratio)
    print(f"  {name}: kernel {ek:.3e}  fp32 {er:.3e}  ratio {ratio:.2f}  bound {bound:.3e}")
    assert ek <= bound, f"{name}: kernel error {ek:.3e} > bound {bound:.3e} (fp32 restatement {er:.3e})"


def _exact(name, got, ref):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, tuple(got.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}")


def _grads(outs, gouts, leaves):
    loss = None
    for o, g in zip(outs, gouts):
        if g is not None:
            t = (o * g.to(device=o.device, dtype=o.dtype)).sum()
            loss = t if loss is None else loss + t
    return torch.autograd.grad(loss, leaves, allow_unused=True)


def _check_op(tag, dev, op, ref, inputs, gouts, out_names, in_names, eps_rows=None):
    """op on the device against ref in float64 / fp32 on the CPU: every output and every input
    gradient (upstream gradients gouts, None = that output is left out of the loss). eps_rows:
    rows of an input whose gradient is dy / eps ~ 1e12 (the normalisation's eps branch); they are
    compared apart from the other rows, whose errors their magnitude would otherwise hide."""
    cpu = []
    for dt in (F64, F32):
        leaves = [t.to(dt).requires_grad_() for t in inputs]
        outs = ref(*leaves)
        cpu.append(([o.detach() for o in outs], _grads(outs, gouts, leaves)))
    leaves = [t.to(dev).requires_grad_() for t in inputs]
    outs = op(*leaves)
    gr = _grads(outs, gouts, leaves)
    (o64, g64), (o32, g32) = cpu
    for n, a, r, q in zip(out_names, outs, o64, o32):
        _cmp(f"{tag} {n}", a, r, q)
    for n, a, r, q in zip(in_names, gr, g64, g32):
        if r is None:
            assert a is None or not a.any().item(), f"{tag} d{n}: gradient of an unused input"
        else:
            assert a is not None, f"{tag} d{n}: missing gradient"
            if eps_rows is not None and eps_rows.numel() > 0:
                rest = torch.ones(r.shape[0], dtype=torch.bool)
                rest[eps_rows] = False
                a = a.detach().cpu()
                _cmp(f"{tag} d{n} (eps rows)", a[eps_rows], r[eps_rows], q[eps_rows])
                a, r, q = a[rest], r[rest], q[rest]
            _cmp(f"{tag} d{n}", a, r, q)
    return outs, gr


# =========================================================================== LayerNorm family
def _ln(s, w, b, eps, act=0):
    mu = s.mean(-1, keepdim=True)
    d = s - mu
    var = (d * d).mean(-1, keepdim=True)        # biased variance, eps inside the square root
    y = d / torch.sqrt(var + eps) * w + b
    if act == 2:
        y = 0.5 * y * (1.0 + torch.erf(y * 0.7071067811865476))
    return y


def _ln_inputs(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, D, generator=g) * 3 + 1
    res = torch.randn(T, D, generator=g)
    w = torch.rand(D, generator=g) + 0.5
    b = torch.randn(D, generator=g)
    gy = torch.randn(T, D, generator=g)
    gs = torch.randn(T, D, generator=g)
    return x, res, w, b, gy, gs


def _check_layer_norm(dev, T, D, act, seed):
    x, _, w, b, gy, _ = _ln_inputs(T, D, seed)
    _check_op(f"layer_norm[{T}x{D} act{act}]", dev, lambda x, w, b: (ops.layer_norm(x, w, b, 1e-5, act=act),),
              lambda x, w, b: (_ln(x, w, b, 1e-5, act),), [x, w, b], [gy], ["y"], ["x", "w", "b"])


def _check_add_layer_norm(dev, T, D, seed):
    """s = x + res (p = 0, bit-exact), y = LN(s); dx and dres carry the incoming gradient of s."""
    x, res, w, b, gy, gs = _ln_inputs(T, D, seed)
    outs, _ = _check_op(f"add_layer_norm[{T}x{D}]", dev, lambda x, r, w, b: ops.add_layer_norm(x, r, w, b, 1e-5, 0.0),
                        lambda x, r, w, b: (x + r, _ln(x + r, w, b, 1e-5)), [x, res, w, b], [gs, gy], ["s", "y"],
                        ["x", "res", "w", "b"])
    _exact("add_layer_norm s", outs[0], x + res)


def _check_layer_norm_pass(dev, T, D, seed, use=(True, True)):
    """(x, LN(x)): the pass-through gradient is added inside the LayerNorm backward."""
    x, _, w, b, gy, gs = _ln_inputs(T, D, seed)
    gouts = [gs if use[0] else None, gy if use[1] else None]
    outs, _ = _check_op(f"layer_norm_pass[{T}x{D} use{use}]", dev, lambda x, w, b: ops.layer_norm_pass(x, w, b, 1e-5),
                        lambda x, w, b: (x * 1.0, _ln(x, w, b, 1e-5)), [x, w, b], gouts, ["pass", "y"], ["x", "w", "b"])
    _exact("layer_norm_pass x", outs[0], x)


LN_WIDTHS = [64, 128, 256, 512, 768, 1024, 2048]


@pytest.mark.parametrize("T", [1, 3, 17])
@pytest.mark.parametrize("D", LN_WIDTHS)
def test_ln_edge_rows(gpu, D, T):
    """Row counts that leave row groups idle and give a ragged last wave: forward and every
    gradient of layer_norm (act 0 and 2), add_layer_norm, layer_norm_pass; add_dropout at p = 0."""
    for act in (0, 2):
        _check_layer_norm(gpu, T, D, act, seed=D + T + act)
    _check_add_layer_norm(gpu, T, D, seed=D + T + 7)
    _check_layer_norm_pass(gpu, T, D, seed=D + T + 9)
    x, res, _, _, _, gs = _ln_inputs(T, D, D + T + 11)
    xd, rd = x.to(gpu).requires_grad_(), res.to(gpu).requires_grad_()
    s = ops.add_dropout(xd, rd, 0.0)
    _exact("add_dropout(p=0) s", s, x + res)
    dx, dr = torch.autograd.grad((s * gs.to(gpu)).sum(), [xd, rd])
    _exact("add_dropout(p=0) dx", dx, gs)
    _exact("add_dropout(p=0) dres", dr, gs)


# T = 1024 q + q + 1 (q rows per block-iteration): the backward's grid is capped at 1024 blocks, so
# every block walks two quanta (dw / db accumulate across iterations) and the last block is ragged
@pytest.mark.parametrize("D,T", [(64, 16401), (128, 8201), (256, 4101), (512, 4101), (768, 4101)])
def test_ln_backward_multi_iteration(gpu, D, T):
    _check_layer_norm(gpu, T, D, 2, seed=D)
    _check_add_layer_norm(gpu, T, D, seed=D + 1)
    for use in ((True, False), (False, True), (True, True)):
        _check_layer_norm_pass(gpu, T, D, seed=D + 2, use=use)


# T = cap + 5: the forward's grid is capped at 8192 blocks, then strides
@pytest.mark.parametrize("D,T", [(64, 131077), (256, 32773), (512, 32773)])
def test_ln_forward_grid_stride(gpu, D, T):
    x, res, w, b, gy, gs = _ln_inputs(T, D, D)
    with torch.no_grad():
        y = ops.layer_norm(x.to(gpu), w.to(gpu), b.to(gpu), 1e-5, act=2)
        _cmp(f"layer_norm[{T}x{D}] y", y, _ln(x.double(), w.double(), b.double(), 1e-5, 2), _ln(x, w, b, 1e-5, 2))
        if D != 512:
            s, y = ops.add_layer_norm(x.to(gpu), res.to(gpu), w.to(gpu), b.to(gpu), 1e-5, 0.0)
            _exact("add_layer_norm s", s, x + res)
            s64 = x.double() + res.double()
            _cmp(f"add_layer_norm[{T}x{D}] y", y, _ln(s64, w.double(), b.double(), 1e-5), _ln(x + res, w, b, 1e-5))
    if D == 512:  # the backward reads the saved mean / rstd of the strided rows
        _check_add_layer_norm(gpu, T, D, seed=D + 1)


def _scale32(p):
    """The kernels' fp32 keep scale 1 / (1 - p)."""
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_is_a_function_of_seed_and_flat_index(gpu, p):
    """One flat buffer viewed at four row widths (64 and 256: the narrow kernel, 512 and 2048: the
    wide one, which computes its element index separately): the add-only forward, the
    add + LayerNorm forward, rsx_dropout_bwd and rsx_ln_bwd all keep exactly the same elements."""
    n = 2048 * 37
    g = torch.Generator().manual_seed(int(p * 100))
    x = torch.randn(n, generator=g)
    res = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    ds = torch.randn(n, generator=g)
    seed = 0x1234_5678_9ABC + int(p * 100)
    sc = _scale32(p)
    zero = torch.zeros(n, device=gpu)
    # x = 0: the output is dropout(res) itself, a kept element exactly res * float32(1 / (1 - p))
    d0 = ops._AddDropout.apply(zero.view(-1, 128), res.to(gpu).view(-1, 128), p, seed).reshape(-1).cpu()
    kept = d0 != 0
    _exact("dropout(res)", d0, torch.where(kept, res * sc, torch.zeros(())))
    frac = kept.double().mean().item()
    tol = 5.0 * math.sqrt(p * (1 - p) / n)
    print(f"  kept fraction {frac:.5f} vs {1 - p} (tolerance {tol:.5f})")
    assert abs(frac - (1 - p)) <= tol
    s_ref = None
    for D in (64, 256, 512, 2048):
        xd = x.to(gpu).view(-1, D).requires_grad_()
        rd = res.to(gpu).view(-1, D).requires_grad_()
        s = ops._AddDropout.apply(xd, rd, p, seed)
        flat = s.detach().reshape(-1).cpu()
        if s_ref is None:
            s_ref = flat
            _exact("dropped elements leave x", flat[~kept], x[~kept])
            _cmp("x + dropout(res), kept", flat[kept], x[kept].double() + (res[kept] * sc).double(), x[kept] + res[kept] * sc)
        _exact(f"add_dropout s, D={D}", flat, s_ref)
        dx, dr = torch.autograd.grad((s * ds.to(gpu).view(-1, D)).sum(), [xd, rd])
        _exact(f"add_dropout dx, D={D}", dx.reshape(-1), ds)
        _exact(f"rsx_dropout_bwd dres, D={D}", dr.reshape(-1), torch.where(kept, ds * sc, torch.zeros(())))
        # add + LayerNorm with the same seed: the same sum, and the same mask on dres in rsx_ln_bwd
        w = (torch.rand(D, generator=g) + 0.5).to(gpu)
        b = torch.randn(D, generator=g).to(gpu)
        xd = x.to(gpu).view(-1, D).requires_grad_()
        rd = res.to(gpu).view(-1, D).requires_grad_()
        s2, y2 = ops._AddLayerNorm.apply(xd, rd, w, b, 1e-5, p, seed)
        _exact(f"add_layer_norm s, D={D}", s2.reshape(-1), s_ref)
        gy = torch.randn(n, generator=g).to(gpu).view(-1, D)
        dx2, dr2 = torch.autograd.grad((s2 * ds.to(gpu).view(-1, D)).sum() + (y2 * gy).sum(), [xd, rd])
        dx2 = dx2.reshape(-1).cpu()
        _exact(f"rsx_ln_bwd dres, D={D}", dr2.reshape(-1), torch.where(kept, dx2 * sc, torch.zeros(())))
        assert (dx2 != 0).all()  # so dres != 0 exactly on the kept set


def test_add_dropout_eval_and_p0_are_plain_adds(gpu):
    x, res, *_ = _ln_inputs(77, 512, 3)
    for kw in (dict(p_drop=0.3, training=False), dict(p_drop=0.0, training=True)):
        _exact(f"add_dropout {kw}", ops.add_dropout(x.to(gpu), res.to(gpu), **kw), x + res)
    x3 = x.view(7, 11, 512)
    _exact("add_dropout 3-D", ops.add_dropout(x3.to(gpu), res.view(7, 11, 512).to(gpu), 0.0), x3 + res.view(7, 11, 512))


@pytest.mark.parametrize("D", [768, 1024])
def test_add_layer_norm_infer(gpu, D):
    x, res, w, b, _, _ = _ln_inputs(37, D, D)
    xd, rd, wd, bd = (t.to(gpu) for t in (x, res, w, b))
    y = ops.add_layer_norm_infer(xd, rd, wd, bd, 1e-12)
    s64 = x.double() + res.double()
    _cmp(f"add_layer_norm_infer[{D}] y", y, _ln(s64, w.double(), b.double(), 1e-12), _ln(x + res, w, b, 1e-12))
    _, y_train = ops.add_layer_norm(xd, rd, wd, bd, 1e-12, 0.0)
    _exact("add_layer_norm_infer == add_layer_norm(p=0)", y, y_train.cpu())


@pytest.mark.parametrize("D", [128, 768])
def test_ln_no_rows(gpu, D):
    """T = 0: empty outputs and input gradients, zero dw / db, no launch on empty tensors."""
    w = (torch.rand(D) + 0.5).to(gpu).requires_grad_()
    b = torch.randn(D, device=gpu).requires_grad_()
    x = torch.zeros(0, D, device=gpu).requires_grad_()
    r = torch.zeros(0, D, device=gpu).requires_grad_()
    y = ops.layer_norm(x, w, b, 1e-5, act=2)
    assert tuple(y.shape) == (0, D)
    dx, dw, db = torch.autograd.grad(y.sum(), [x, w, b])
    assert tuple(dx.shape) == (0, D)
    _exact("dw", dw, torch.zeros(D))
    _exact("db", db, torch.zeros(D))
    s, y = ops.add_layer_norm(x, r, w, b, 1e-5, 0.1)
    assert tuple(s.shape) == (0, D) and tuple(y.shape) == (0, D)
    dx, dr, dw, db = torch.autograd.grad(s.sum() + y.sum(), [x, r, w, b])
    assert tuple(dx.shape) == (0, D) and tuple(dr.shape) == (0, D)
    _exact("dw", dw, torch.zeros(D))
    _exact("db", db, torch.zeros(D))
    s = ops.add_dropout(x, r, 0.1)
    dx, dr = torch.autograd.grad(s.sum(), [x, r])
    assert tuple(s.shape) == (0, D) and tuple(dx.shape) == (0, D) and tuple(dr.shape) == (0, D)
    assert tuple(ops.add_layer_norm_infer(x.detach(), r.detach(), w.detach(), b.detach()).shape) == (0, D)


# =========================================================================== row gather / scatter
def _gather_case(n, D, form, strided, seed):
    """(source leaf, source view, idx, a row of idx, a row outside idx or -1). Row 0 is zero and
    the last row is 1e-20: both take the eps branch of the normalisation."""
    g = torch.Generator().manual_seed(seed)
    if form == "all":
        nsrc, idx = n, None
    elif form == "unique":
        nsrc = n + 2
        mid = (1 + torch.randperm(nsrc - 2, generator=g))[:max(n - 2, 0)]
        idx = torch.cat([torch.tensor([0]), mid, torch.tensor([nsrc - 1])])[:n] if n > 1 else torch.tensor([0])
        idx = idx[torch.randperm(n, generator=g)]
    else:
        nsrc = n // 3 + 2
        idx = torch.randint(0, nsrc, (n,), generator=g)
        idx[0] = 0
        idx[-1] = nsrc - 1 if n > 1 else 0
    ld = D + 8 if strided else D
    wide = torch.randn(nsrc, ld, generator=g)
    c0 = 4 if strided else 0
    wide[0, c0:c0 + D] = 0.0
    if nsrc > 1:
        wide[nsrc - 1, c0:c0 + D] = 1e-20
    used = torch.arange(nsrc) if idx is None else idx
    present = int(used[n // 2])
    free = sorted(set(range(nsrc)) - set(used.tolist()))
    absent = free[0] if free else -1
    return wide, c0, idx, present, absent


def _gather_ref(src, idx, normalize, skip):
    """float64 / fp32 restatement with the skipped row's gradient cut."""
    if skip >= 0:
        keep = torch.ones(src.shape[0], 1, dtype=src.dtype)
        keep[skip] = 0.0
        src = src * keep + (src * (1 - keep)).detach()
    rows = src if idx is None else src[idx]
    return F.normalize(rows, p=2, dim=-1, eps=1e-12) if normalize else rows


def _run_gather(gpu, n, D, form, strided, normalize, skip_present, seed):
    wide, c0, idx, present, absent = _gather_case(n, D, form, strided, seed)
    skip = present if skip_present else absent
    tag = f"gather[{n}x{D} {form} strided={strided} norm={normalize} skip={skip}]"
    g = torch.Generator().manual_seed(seed + 1)
    idx_d = None if idx is None else idx.to(gpu)

    def op(wide_d):
        src = wide_d[:, c0:c0 + D]
        assert src.stride(0) == wide.shape[1]
        return (ops.gather_rows(src, idx_d, normalize=normalize, unique=(form == "unique"), skip_idx=skip),)

    def ref(w):
        return (_gather_ref(w[:, c0:c0 + D], idx, normalize, skip),)

    if not normalize:
        # plain rows are copied bit for bit; with dyadic dy the scatter-add is exact in any order
        dy = torch.randint(-8, 9, (n, D), generator=g).float() * 0.25
        wd = wide.to(gpu).requires_grad_()
        out = op(wd)[0]
        _exact(f"{tag} out", out, ref(wide)[0])
        w64 = wide.double().requires_grad_()
        (gr64,) = torch.autograd.grad((ref(w64)[0] * dy.double()).sum(), [w64])
        (gr,) = torch.autograd.grad((out * dy.to(gpu)).sum(), [wd])
        _exact(f"{tag} dsrc (dyadic dy)", gr, gr64.float())
    dy = torch.randn(n, D, generator=g)
    eps_rows = torch.tensor(sorted({0, wide.shape[0] - 1})) if normalize else None
    _check_op(tag, gpu, op, ref, [wide], [dy], ["out"], ["src"], eps_rows=eps_rows)


@pytest.mark.parametrize("n", [1, 5, 1000])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_gather_rows_forms(gpu, D, n):
    """Identity / duplicate-free accumulate / atomic scatter, each with skip_idx on a row that does
    and does not occur and with normalize on and off; a strided source (ld_src > D) where n != 1000
    or D == 256."""
    strided = not (n == 1000 and D != 256)
    for form in ("all", "unique", "dup"):
        for normalize in (False, True):
            for skip_present in (False, True):
                _run_gather(gpu, n, D, form, strided, normalize, skip_present, seed=D + n)


# n = 16384 rows_per_block + 5: the grid is capped at 16384 blocks, then strides
@pytest.mark.parametrize("D,n", [(256, 65541), (64, 262149)])
@pytest.mark.parametrize("skip_present", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("form", ["all", "unique", "dup"])
def test_gather_rows_grid_stride(gpu, D, n, form, normalize, skip_present):
    _run_gather(gpu, n, D, form, False, normalize, skip_present, seed=D)


def test_l2_normalize_3d(gpu):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 7, 64, generator=g)
    x[1, 2] = 0.0
    x[2, 6] = 1e-20
    dy = torch.randn(3, 7, 64, generator=g)
    outs, _ = _check_op("l2_normalize", gpu, lambda x: (ops.l2_normalize(x.view(3, 7, 64)).view(21, 64),),
                        lambda x: (F.normalize(x, p=2, dim=-1, eps=1e-12),), [x.view(21, 64)], [dy.view(21, 64)],
                        ["y"], ["x"], eps_rows=torch.tensor([9, 20]))
    assert tuple(ops.l2_normalize(x.to(gpu)).shape) == (3, 7, 64)


@pytest.mark.parametrize("leave_out", [None, 0, 1])
def test_gather_rows_multi(gpu, leave_out):
    """Three duplicate-free index lists that share rows, mixed normalize flags, one output left
    out of the loss (its dy is None): float64 autograd of the three separate gathers."""
    g = torch.Generator().manual_seed(6)
    D, nsrc = 128, 41
    src = torch.randn(nsrc, D, generator=g)
    src[3] = 0.0
    idxs = [torch.randperm(nsrc, generator=g)[:k] for k in (17, 9, 30)]
    idxs[0][0], idxs[2][0] = 3, 3
    idxs[0][1:] = torch.tensor([r for r in torch.randperm(nsrc, generator=g).tolist() if r != 3][:16])
    idxs[2][1:] = torch.tensor([r for r in torch.randperm(nsrc, generator=g).tolist() if r != 3][:29])
    assert all(len(set(i.tolist())) == i.numel() for i in idxs)
    assert set(idxs[0].tolist()) & set(idxs[1].tolist()) & set(idxs[2].tolist())
    norms = (True, False, True)
    gouts = [None if k == leave_out else torch.randn(i.numel(), D, generator=g) for k, i in enumerate(idxs)]
    idx_d = [i.to(gpu) for i in idxs]
    outs, _ = _check_op(f"gather_rows_multi[leave_out={leave_out}]", gpu,
                        lambda s: tuple(ops.gather_rows_multi(s, list(zip(idx_d, norms)))),
                        lambda s: tuple(_gather_ref(s, i, nz, -1) for i, nz in zip(idxs, norms)),
                        [src], gouts, ["out0", "out1", "out2"], ["src"], eps_rows=torch.tensor([3]))
    _exact("plain gather", outs[1], src[idxs[1]])


# =========================================================================== segment sums
SEG_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 100]     # the 16-wide unrolled loop and its < 16 tail


def _segments(seed, reps=3):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(SEG_LENS * reps)[torch.randperm(len(SEG_LENS) * reps, generator=g)]
    seg = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(lens, 0)
    return lens, seg, g


def _segsum_ref(src, perm, seg, rows, scale, skip, dst0, acc, dt):
    out = dst0.to(dt).clone()
    s = src.to(dt)
    for u in range(seg.numel() - 1):
        row = u if rows is None else int(rows[u])
        if row == skip:
            continue
        ks = torch.arange(int(seg[u]), int(seg[u + 1]))
        v = s[ks if perm is None else perm[ks]].sum(0) * scale
        out[row] = out[row] + v if acc else v
    return out


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_segment_sum_rows(gpu, D, strided):
    """rsx_segment_sum_rows with and without perm / rows (one of them the skipped row, which must
    keep its prefilled value) / a device scale / accumulate, contiguous and with ld_src, ld_dst > D;
    27 segments (not a multiple of the rows per wave). Dyadic inputs are exact, random ones go
    under the comparison rule. The whole destination buffer is compared, padding columns included."""
    lens, seg, g = _segments(D + strided)
    nseg, ntok, ndst = lens.numel(), int(seg[-1]), lens.numel() + 5
    lds, ldd, c0 = (D + 8, D + 12, 4) if strided else (D, D, 0)
    for dyadic in (True, False):
        if dyadic:
            wide_src = torch.randint(-8, 9, (ntok, lds), generator=g).float() * 0.125
            wide_dst0 = torch.randint(-8, 9, (ndst, ldd), generator=g).float() * 0.5
            scale = 0.5
        else:
            wide_src = torch.randn(ntok, lds, generator=g)
            wide_dst0 = torch.randn(ndst, ldd, generator=g)
            scale = 0.37
        perm_t = torch.randperm(ntok, generator=g)
        rows_t = torch.randperm(ndst, generator=g)[:nseg]
        src_d = wide_src.to(gpu)
        perm_d, rows_d = perm_t.to(gpu), rows_t.to(gpu)
        seg_d = seg.to(gpu)
        scale_d = torch.tensor([scale], device=gpu)
        for use_perm in (False, True):
            for use_rows in (False, True):
                for use_scale in (False, True):
                    for acc in (0, 1):
                        perm = perm_t if use_perm else None
                        rows = rows_t if use_rows else None
                        skip = int(rows_t[nseg // 2]) if use_rows else -1
                        sc = scale if use_scale else 1.0
                        dst_d = wide_dst0.to(gpu)
                        rc = N.lib().rsx_segment_sum_rows(
                            N.ptr(src_d[:, c0:]), lds, N.ptr(perm_d if use_perm else None), N.ptr(seg_d),
                            N.ptr(rows_d if use_rows else None), nseg, D,
                            N.ptr(scale_d if use_scale else None), skip, N.ptr(dst_d[:, c0:]), ldd, acc, N.stream())
                        N.check(rc, "segment_sum_rows")
                        tag = f"segsum[D={D} perm={use_perm} rows={use_rows} scale={use_scale} acc={acc}]"
                        exp = []
                        for dt in (F64, F32):
                            e = wide_dst0.to(dt).clone()
                            e[:, c0:c0 + D] = _segsum_ref(wide_src[:, c0:c0 + D], perm, seg, rows, sc, skip,
                                                          wide_dst0[:, c0:c0 + D], acc, dt)
                            exp.append(e)
                        if dyadic:
                            _exact(tag + " dyadic", dst_d, exp[0].float())
                        else:
                            _cmp(tag, dst_d, exp[0], exp[1])
                            out = dst_d.cpu()
                            untouched = torch.ones(ndst, ldd, dtype=torch.bool)
                            wr = torch.arange(nseg) if rows is None else rows[rows != skip]
                            untouched[wr, c0:c0 + D] = False
                            _exact(tag + " untouched", out[untouched], wide_dst0[untouched])


@pytest.mark.parametrize("D", [64, 128, 256])
def test_segment_mean(gpu, D):
    """Forward and backward against the float64 masked mean sum / clamp(count, 1e-9), empty
    segments included (they give 0)."""
    lens, seg, g = _segments(D + 50)
    U, T = lens.numel(), int(seg[-1])
    tok_seg = torch.repeat_interleave(torch.arange(U), lens)
    counts = lens.float()
    x = torch.randn(T, D, generator=g)
    dv = torch.randn(U, D, generator=g)

    def ref(x):
        s = torch.zeros(U, D, dtype=x.dtype).index_add(0, tok_seg, x)
        return (s / counts.to(x.dtype).clamp(min=1e-9).unsqueeze(1),)

    seg_d, tok_d, cnt_d = seg.to(gpu), tok_seg.to(gpu), counts.to(gpu)
    outs, _ = _check_op(f"segment_mean[D={D}]", gpu, lambda x: (ops.segment_mean(x, seg_d, tok_d, cnt_d),), ref, [x],
                        [dv], ["mean"], ["x"])
    _exact("empty segments", outs[0].detach().cpu()[lens == 0], torch.zeros(int((lens == 0).sum()), D))
    # dyadic rows: the segment sums are exact, so is the mean of a power-of-two-sized segment
    xq = torch.randint(-8, 9, (T, D), generator=g).float() * 0.25
    out = ops.segment_mean(xq.to(gpu), seg_d, tok_d, cnt_d)
    pow2 = (lens == 1) | (lens == 16) | (lens == 32)
    _exact("dyadic means", out.cpu()[pow2], ref(xq.double())[0][pow2].float())


# =========================================================================== cross network
def _cross_ref(x, ks, bs, wh):
    x0, xl = x, x
    for k, b in zip(ks, bs):
        xl = x0 * ((xl * k).sum(-1, keepdim=True) + b) + xl
    return xl, (xl * wh).sum(-1)


def _cross_inputs(B, D, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    ks = [torch.randn(D, 1, generator=g) / math.sqrt(D) * 0.5 for _ in range(L)]
    bs = [torch.randn(D, generator=g) * 0.5 for _ in range(L)]
    wh = torch.randn(D, generator=g) / math.sqrt(D)
    return x, ks, bs, wh


def _check_cross(tag, x, ks, bs, wh, x_out, head):
    f64 = _cross_ref(x.double(), [k.double().reshape(-1) for k in ks], [b.double() for b in bs], wh.double())
    f32 = _cross_ref(x, [k.reshape(-1) for k in ks], bs, wh)
    if x_out is not None:
        _cmp(f"{tag} x_out", x_out, f64[0], f32[0])
    if head is not None:
        _cmp(f"{tag} head", head, f64[1], f32[1])


# both template instances and the c < n4 guards on each side of 256; B = 65541 at D = 4 strides
@pytest.mark.parametrize("D,B", [(D, B) for D in (4, 252, 256, 260, 508, 512) for B in (1, 3, 1031)] + [(4, 65541)])
def test_crossnet(gpu, D, B):
    for L in (0, 1, 8):
        x, ks, bs, wh = _cross_inputs(B, D, L, seed=D + B + L)
        xd, kd, bd, wd = x.to(gpu), [k.to(gpu) for k in ks], [b.to(gpu) for b in bs], wh.to(gpu)
        tag = f"crossnet[{B}x{D} L={L}]"
        xo, part = ops.crossnet(xd, kd, bd, None, want_x=True)
        assert part is None
        _check_cross(tag + " x only", x, ks, bs, wh, xo, None)
        if L == 0:
            _exact("x_0", xo, x)
        xo2, part = ops.crossnet(xd, kd, bd, wd, want_x=False)
        assert xo2 is None
        _check_cross(tag + " head only", x, ks, bs, wh, None, part)
        xo3, part3 = ops.crossnet(xd, kd, bd, wd, want_x=True)
        _check_cross(tag + " both", x, ks, bs, wh, xo3, part3)
        _exact("x_out, both == x only", xo3, xo.cpu())
        _exact("head, both == head only", part3, part.cpu())


def _crossnet_c(x, ldx, B, D, ks, bs, wh, x_out, part):
    return N.lib().rsx_crossnet(N.ptr(x), ldx, B, D, len(ks), N.ptr_array(ks), N.ptr_array(bs), N.ptr(wh),
                                N.ptr(x_out), N.ptr(part), N.stream())


def test_crossnet_strided_input(gpu):
    B, D, L = 1031, 252, 3
    x, ks, bs, wh = _cross_inputs(B, D, L, seed=9)
    wide = torch.randn(B, D + 4)
    wide[:, 4:] = x
    wd = wide.to(gpu)
    kd, bd = [k.reshape(-1).to(gpu) for k in ks], [b.to(gpu) for b in bs]
    whd = wh.to(gpu)
    xo = torch.empty(B, D, device=gpu)
    part = torch.empty(B, device=gpu)
    N.check(_crossnet_c(wd[:, 4:], D + 4, B, D, kd, bd, whd, xo, part), "crossnet")
    _check_cross("crossnet[ldx = D + 4]", x, ks, bs, wh, xo, part)


def test_crossnet_refusals(gpu):
    """Refused by rsx_crossnet's argument checks, before any launch."""
    def call(D, L, with_head_weight=True):
        x = torch.zeros(2, D, device=gpu)
        ks = [torch.zeros(D, device=gpu) for _ in range(L)]
        bs = [torch.zeros(D, device=gpu) for _ in range(L)]
        wh = torch.zeros(D, device=gpu) if with_head_weight else None
        part = torch.zeros(2, device=gpu)
        N.check(_crossnet_c(x, D, 2, D, ks, bs, wh, None, part), "crossnet")

    call(8, 2)
    for D, L, hw, msg in ((6, 1, True, "multiple of 4"), (516, 1, True, "multiple of 4"), (8, 9, True, "L must be"),
                          (8, 1, False, "w_head")):
        with pytest.raises(RuntimeError, match=msg):
            call(D, L, hw)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.crossnet(torch.zeros(2, 516, device=gpu), [torch.zeros(516, device=gpu)], [torch.zeros(516, device=gpu)],
                     want_x=True)


# =========================================================================== loss_combine
@pytest.mark.parametrize("n", [0, 12])
@pytest.mark.parametrize("cnt", [0.0, 0.5, 1.0, 7.0])
@pytest.mark.parametrize("has_sup", [False, True])
@pytest.mark.parametrize("has_main", [False, True])
def test_loss_combine(gpu, has_main, has_sup, cnt, n):
    """total = s_main / n + lambda_cl (s_un / b + lambda_sup s_sup / max(cnt, 1)), its three logged
    values and every input gradient under an upstream gradient of 3, against float64 autograd."""
    b, lsup, lcl = 5, 0.3, 0.7
    vals = [torch.tensor(v) for v in (41.37, 9.123, 17.77)]

    def ref(s_main, s_un, s_sup):
        main = s_main / n if (has_main and n) else s_un * 0.0
        cl = s_un / b
        if has_sup:
            cl = cl + lsup * (s_sup / max(cnt, 1.0))
        total = main + lcl * cl
        return total, torch.stack([total, main, cl]).detach()

    def op(s_main, s_un, s_sup):
        total, logs = ops.loss_combine(s_main if has_main else None, s_un, s_sup if has_sup else None,
                                       torch.tensor(cnt, device=gpu) if has_sup else None, n, b, lsup, lcl)
        assert not logs.requires_grad and tuple(logs.shape) == (3,) and tuple(total.shape) == ()
        return total, logs

    _check_op(f"loss_combine[main={has_main} sup={has_sup} cnt={cnt} n={n}]", gpu, op, ref, vals,
              [torch.tensor(3.0), None], ["total", "logs"], ["s_main", "s_un", "s_sup"])


# =========================================================================== packed BERT embedding
def _bert_embeddings(word, pos, typ, w, b, eps):
    ns = types.SimpleNamespace
    return ns(word_embeddings=ns(weight=word), position_embeddings=ns(weight=pos), token_type_embeddings=ns(weight=typ),
              LayerNorm=ns(weight=w, bias=b, eps=eps), dropout=ns(p=0.1), training=False)


@pytest.mark.parametrize("D,T", [(D, T) for D in (256, 512, 768, 1024) for T in (1, 5, 1000)] + [(256, 65541)])
def test_bert_embed_packed(gpu, D, T):
    """((word + type) + pos) then LayerNorm at eps 1e-12, a strided word table; T = 65541 strides."""
    g = torch.Generator().manual_seed(D + T)
    V, P = 97, 32
    wide = torch.randn(V, D + 8, generator=g) * 0.05
    pos = torch.randn(P, D, generator=g) * 0.05
    typ = torch.randn(2, D, generator=g) * 0.05
    w = torch.rand(D, generator=g) + 0.5
    b = torch.randn(D, generator=g) * 0.1
    ids = torch.randint(0, V, (T,), generator=g)
    tp = torch.randint(0, P, (T,), generator=g)
    ids[0], ids[-1], tp[0], tp[-1] = V - 1, 0, P - 1, 0
    wide_d = wide.to(gpu)
    emb = _bert_embeddings(wide_d[:, 4:4 + D], pos.to(gpu), typ.to(gpu), w.to(gpu), b.to(gpu), 1e-12)
    assert emb.word_embeddings.weight.stride(0) == D + 8
    out = ops.bert_embed_packed(emb, ids.to(gpu), tp.to(gpu))

    def ref(dt):
        word = wide[:, 4:4 + D].to(dt)
        return _ln((word[ids] + typ[0].to(dt)) + pos.to(dt)[tp], w.to(dt), b.to(dt), 1e-12)

    _cmp(f"bert_embed_packed[{T}x{D}]", out, ref(F64), ref(F32))


# =========================================================================== ids_check
def _ids_check(ids, lo, hi, flag0, gpu):
    ids_d = ids.to(gpu)
    out = torch.full_like(ids_d, -77)
    flag = torch.tensor([flag0], device=gpu, dtype=torch.int32)
    N.check(N.lib().rsx_ids_check(N.ptr(ids_d), ids.numel(), lo, hi, N.ptr(out), N.ptr(flag), N.stream()), "ids_check")
    return out.cpu(), int(flag.item())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262149])
def test_ids_check(gpu, n):
    """out == where(lo <= id < hi, id, 0) exactly; the flag becomes 1 iff any id is outside and is
    left as initialised otherwise (preset 0 and preset 1)."""
    lo, hi = -5, 1000
    special = [lo - 1, lo, hi - 1, hi, -123456, 2 ** 62, -2 ** 62]
    g = torch.Generator().manual_seed(n)
    cases = []
    if n == 1:
        cases = [torch.tensor([v], dtype=torch.int64) for v in special]
    else:
        good = torch.randint(lo, hi, (n,), generator=g)
        good[0], good[-1] = lo, hi - 1
        cases.append(good)
        for k, v in enumerate(special):            # one special value at a time, at the ends and inside
            t = good.clone()
            t[(0, n - 1, n // 2, 63, 64, 254, n - 2)[k]] = v
            cases.append(t)
        mixed = good.clone()
        mixed[torch.randperm(n, generator=g)[:len(special)]] = torch.tensor(special)
        cases.append(mixed)
    for ids in cases:
        ok = (ids >= lo) & (ids < hi)
        exp = torch.where(ok, ids, torch.zeros_like(ids))
        for flag0 in (0, 1):
            out, flag = _ids_check(ids, lo, hi, flag0, gpu)
            _exact("ids_check out", out, exp)
            assert flag == (flag0 if bool(ok.all()) else 1), (flag, flag0, bool(ok.all()))
