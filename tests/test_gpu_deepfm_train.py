"""DeepFM training on the device (ops.deepfm_train_step, DeepFM.make_trainer / fit) against the
float64 CPU reference of tests/deepfm_train_ref.py: oracle forward, binary_cross_entropy_with_logits,
autograd, torch.optim.SparseAdam on the tables and Adam on the dense parameters.
init_std 0.05, non-zero biases and lr 1e-2 so that every term matters."""
import functools

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.temp_model.ranker_skelet import DeepFM
from oracle import deepfm as OD
from tests import deepfm_train_ref as REF

pytestmark = pytest.mark.gpu

LR = 1e-2
ID_BITS = 40
ID_MASK = (1 << ID_BITS) - 1

# (R, per-field vocab sizes, id distribution)
SHAPES = {
    "tail_dups": (77, [50] * 5, "uniform"),          # row tail, F not a multiple of 4 or 13, every id duplicated
    "zipf_hot": (1000, [500] * 39, "zipf"),           # hundreds of duplicates on the hot id: chunks straddle
    "config_f": (4099, [3000] * 39, "zipf"),          # rows past the last 64-row block at the config's F
    "one_row": (1, [10] * 2, "uniform"),
    "unequal": (60, [50, 7, 1000, 3, 64], "uniform"),
}


def _batch(R, vocabs, dist, seed):
    g = torch.Generator().manual_seed(seed)
    if dist == "zipf":
        x = REF.zipf_ids(R, vocabs, g)
    else:
        x = torch.stack([torch.randint(0, v, (R,), generator=g) for v in vocabs], dim=1)
    return x, REF.labels(R, g)


@functools.lru_cache(maxsize=None)
def _case(name):
    R, vocabs, dist = SHAPES[name]
    x, y = _batch(R, vocabs, dist, seed=3)
    return REF.make_params(vocabs, seed=1), x, y


@functools.lru_cache(maxsize=None)
def _ref_grads(name, reduction):
    params, x, y = _case(name)
    return REF.gradients(params, x, y, reduction)


def _gpu_state(params, dev, m=None, v=None, pad=0):
    """Device copies of the tables (optionally the first rows of allocations `pad` rows longer),
    their moments (zeros, or m / v in emb-then-lin order) and the dense parameters."""
    nf = len(params["emb"])
    full = {"emb": [], "lin": [], "emb_m": [], "emb_v": [], "lin_m": [], "lin_v": []}
    for k, src in (("emb", params["emb"]), ("lin", params["lin"])):
        for f, t in enumerate(src):
            i = f if k == "emb" else nf + f
            for key, val in ((k, t), (k + "_m", torch.zeros_like(t) if m is None else m[i].reshape(t.shape)),
                             (k + "_v", torch.zeros_like(t) if v is None else v[i].reshape(t.shape))):
                guard = torch.full((pad,) + tuple(t.shape[1:]), 0.25)
                full[key].append(torch.cat([val, guard]).to(dev).contiguous())
    st = {k: [t[:t.shape[0] - pad] for t in ts] for k, ts in full.items()}
    st["full"] = full
    for k in REF.DENSE:
        st[k] = params[k].to(dev).contiguous()
    return st


def _step(st, x, y, step=1, reduction="mean", return_grads=False, id_flag=None):
    return ops.deepfm_train_step(x, y, st["emb"], st["lin"], st["emb_m"], st["emb_v"], st["lin_m"], st["lin_v"],
                                 st["bias"], [st["w1"], st["w2"]], [st["b1"], st["b2"]], st["wo"], step, lr=LR,
                                 reduction=reduction, return_grads=return_grads, id_flag=id_flag)


def _ratio(got, ref):
    """max |got - ref| over the reference tensor's max-abs."""
    ref = ref.double()
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _check_gradients(res, ref, x, label):
    loss_r, logit_r, dense_r, sparse_r = ref
    ratios = {}
    for name, got in zip(("w1", "b1", "w2", "b2", "wo", "bias"), res.dense):
        ratios[name] = _ratio(got, dense_r[name])
    got_sparse = res.sparse_grads()
    assert len(got_sparse) == x.shape[1]
    ratios["dV"] = ratios["dW"] = 0.0
    for f, ((ids, dv, dw, cnt), (ids_r, dv_r, dw_r)) in enumerate(zip(got_sparse, sparse_r)):
        assert torch.equal(ids.cpu(), ids_r), f"field {f}: distinct ids differ"
        assert int(cnt) == ids_r.numel()
        ratios["dV"] = max(ratios["dV"], _ratio(dv, dv_r))
        ratios["dW"] = max(ratios["dW"], _ratio(dw, dw_r))
    loss_err = abs(float(res.loss) - float(loss_r))
    logit_err = float((res.logit.cpu().double() - logit_r).abs().max())
    print(f"[{label}] max error / max-abs per tensor: " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items())
          + f"; loss err {loss_err:.2e}, logit err {logit_err:.2e}")
    for k, v in ratios.items():
        assert v <= 1e-3, f"{k}: {v:.3e} of the reference's max-abs"
    assert loss_err <= 1e-4 and logit_err <= 1e-4, (loss_err, logit_err)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_match_float64_autograd(gpu, name, reduction):
    """Largest error / max-abs observed on an MI355X over these cases: W1 4.3e-6, b1 4.9e-6, W2 3.3e-7,
    b2 1.9e-7, w_out 7.0e-7, out.bias 5.7e-7, dV 1.8e-6, dW 2.6e-7; loss 3.1e-6, logits 3.8e-7."""
    params, x, y = _case(name)
    res = _step(_gpu_state(params, gpu), x.to(gpu), y.to(gpu), reduction=reduction, return_grads=True)
    _check_gradients(res, _ref_grads(name, reduction), x, f"{name}/{reduction}")


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_degenerate_id_patterns(gpu, reduction):
    """Field 0 constant at the table's last row (one segment across every chunk), field 1 a
    permutation (all distinct, id 0 included), field 2 random."""
    R = vocab = 300
    g = torch.Generator().manual_seed(5)
    x = torch.stack([torch.full((R,), vocab - 1), torch.randperm(vocab, generator=g),
                     torch.randint(0, vocab, (R,), generator=g)], dim=1)
    y = REF.labels(R, g)
    params = REF.make_params([vocab] * 3, seed=2)
    res = _step(_gpu_state(params, gpu), x.to(gpu), y.to(gpu), reduction=reduction, return_grads=True)
    _check_gradients(res, REF.gradients(params, x, y, reduction), x, f"degenerate/{reduction}")


def test_sparse_update_from_its_gradient(gpu):
    """The row update alone: moments seeded non-zero and step 4 -> 5 (smooth in g), the GPU's own
    fp32 contribution rows coalesced in float64 on the CPU and stepped by SparseAdam in float64.
    Error <= 1e-4 of the reference's largest change per tensor kind; untouched rows bit-identical."""
    params, x, y = _case("config_f")
    nf = len(params["emb"])
    g = torch.Generator().manual_seed(9)
    shapes = [t.shape for t in params["emb"] + params["lin"]]
    m = [torch.randn(s, generator=g) * 1e-3 for s in shapes]
    v = [torch.rand(s, generator=g) * (1e-5 - 1e-7) + 1e-7 for s in shapes]
    st = _gpu_state(params, gpu, m, v)
    res = _step(st, x.to(gpu), y.to(gpu), step=5, return_grads=True)
    keys, gV, gW = (t.cpu() for t in res.contributions())
    fld, ids = keys >> ID_BITS, keys & ID_MASK
    sparse = []
    for f in range(nf):
        pos = fld == f
        uniq, inverse = torch.unique(ids[pos], return_inverse=True)
        dv = torch.zeros(uniq.numel(), 16, dtype=torch.float64).index_add_(0, inverse, gV[pos].double())
        dw = torch.zeros(uniq.numel(), dtype=torch.float64).index_add_(0, inverse, gW[pos].double())
        sparse.append((uniq, dv, dw))
    ref = REF.RefTrainer(params, lr=LR)
    ref.seed_moments(m, v, 4)
    ref.apply_sparse(sparse)
    ref_m, ref_v = ref.moments()
    old = params["emb"] + params["lin"]
    new = st["emb"] + st["lin"]
    new_m, new_v = st["emb_m"] + st["lin_m"], st["emb_v"] + st["lin_v"]
    worst = {}
    for what, got_l, ref_l, old_l in (("p", new, ref.tables, old), ("m", new_m, ref_m, m), ("v", new_v, ref_v, v)):
        worst[what] = 0.0
        for i, (got, r, o) in enumerate(zip(got_l, ref_l, old_l)):
            got, o = got.cpu().reshape(r.shape), o.reshape(r.shape)
            change = float((r - o.double()).abs().max())
            err = float((got.double() - r).abs().max())
            worst[what] = max(worst[what], err / change)
            touched = torch.zeros(r.shape[0], dtype=torch.bool)
            touched[torch.unique(x[:, i % nf])] = True
            assert torch.equal(got[~touched], o[~touched]), f"{what}[{i}]: an untouched row changed"
    print("sparse update: max error / max reference change: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    for what, e in worst.items():
        assert e <= 1e-4, f"{what}: {e:.3e} of the reference's largest change"


def _model(params, dev):
    vocabs = [t.shape[0] for t in params["emb"]]
    model = DeepFM(vocabs, init_std=0.05, device=dev)
    with torch.no_grad():
        for n, e, l in zip(model.field_names, params["emb"], params["lin"]):
            model.embedding_dict[n].weight.copy_(e)
            model.linear_model.embedding_dict[n].weight.copy_(l)
        for lin, w, b in zip(model.dnn.linears, (params["w1"], params["w2"]), (params["b1"], params["b2"])):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        model.dnn_linear.weight.copy_(params["wo"])
        model.out.bias.copy_(params["bias"])
    return model


def _model_tensors(model):
    emb, lin, ws, bs, wo = model._param_lists()
    return ([(f"emb{f}", t) for f, t in enumerate(emb)] + [(f"lin{f}", t) for f, t in enumerate(lin)]
            + [("w1", ws[0]), ("b1", bs[0]), ("w2", ws[1]), ("b2", bs[1]), ("wo", wo), ("bias", model.out.bias)])


@pytest.mark.parametrize("name", ["tail_dups", "zipf_hot"])
def test_three_steps_end_to_end(gpu, name):
    """Zero moments, fresh Zipf batches. Adam's first step is sign-like, so a near-zero gradient may
    flip: per tensor at most 0.1 % of elements beyond 1e-2 lr of the float64 reference, none beyond 3 lr."""
    R, vocabs, _ = SHAPES[name]
    params = REF.make_params(vocabs, seed=4)
    model = _model(params, gpu)
    tr = model.make_trainer(lr=LR)
    ref = REF.RefTrainer(params, lr=LR)
    for s in range(3):
        x, y = _batch(R, vocabs, "zipf", seed=20 + s)
        loss = float(tr.step(x.to(gpu), y.to(gpu)))
        loss_r = float(ref.step(x, y))
        print(f"[{name}] step {s + 1}: loss {loss:.7f} reference {loss_r:.7f}")
        assert abs(loss - loss_r) <= 1e-4
    tr.check_ids()
    worst_frac = worst_max = 0.0
    for (n, got), (_, r) in zip(_model_tensors(model), REF.all_tensors(ref.p)):
        frac, mx = REF.cap_violations(got.detach().cpu().reshape(r.shape), r, LR)
        worst_frac, worst_max = max(worst_frac, frac), max(worst_max, mx)
        assert frac <= 1e-3 and mx <= 3.0, f"{n}: {frac:.2e} of elements beyond 1e-2 lr, max {mx:.3f} lr"
    print(f"[{name}] after 3 steps: worst fraction beyond 1e-2 lr {worst_frac:.2e}, worst difference {worst_max:.3e} lr")


def test_step_is_deterministic(gpu):
    R, vocabs, _ = SHAPES["zipf_hot"]
    params = REF.make_params(vocabs, seed=6)
    x, y = _batch(R, vocabs, "zipf", seed=30)
    runs = []
    for _ in range(2):
        model = _model(params, gpu)
        tr = model.make_trainer(lr=LR)
        for _s in range(2):
            tr.step(x.to(gpu), y.to(gpu))
        runs.append([t for _, t in _model_tensors(model)] + tr.emb_m + tr.emb_v + tr.lin_m + tr.lin_v)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_inference_sees_the_update(gpu):
    """The packed tables / bf16 images are warm from a call before the step; the step's raw-pointer
    writes must invalidate them."""
    R, vocabs = 1000, [500] * 39
    params = REF.make_params(vocabs, seed=7)
    model = _model(params, gpu)
    x, y = _batch(R, vocabs, "zipf", seed=31)
    before, _ = model.forward_logits(x.to(gpu))
    before = before.clone()
    tr = model.make_trainer(lr=LR)
    tr.step(x.to(gpu), y.to(gpu))
    after, _ = model.forward_logits(x.to(gpu))
    names = model.field_names
    ref_l, _ = OD.deepfm_forward(
        x, [model.embedding_dict[n].weight.detach().cpu() for n in names],
        [model.linear_model.embedding_dict[n].weight.detach().cpu() for n in names], float(model.out.bias.item()),
        [l.weight.detach().cpu() for l in model.dnn.linears], [l.bias.detach().cpu() for l in model.dnn.linears],
        model.dnn_linear.weight.detach().cpu())
    torch.testing.assert_close(after.cpu().double(), ref_l, atol=1e-4, rtol=1e-5)
    assert float((after - before).abs().max()) > 1e-3


def test_bad_id_is_made_safe(gpu):
    """One id equal to its field's vocab. Every table and moment is the first `vocab` rows of an
    allocation 8 rows longer, so that id lies inside allocated memory whatever the code does."""
    R, vocabs, pad = 64, [20, 30, 20], 8
    bad_r, bad_f = 5, 1
    params = REF.make_params(vocabs, seed=8)
    x, y = _batch(R, vocabs, "uniform", seed=32)
    x_bad = x.clone()
    x_bad[bad_r, bad_f] = vocabs[bad_f]
    x_safe = x.clone()
    x_safe[bad_r, bad_f] = 0      # what the gathers read
    st = _gpu_state(params, gpu, pad=pad)
    guards = {k: [t[-pad:].clone() for t in ts] for k, ts in st["full"].items()}
    flag = torch.zeros(1, device=gpu, dtype=torch.int32)
    res = _step(st, x_bad.to(gpu), y.to(gpu), return_grads=True, id_flag=flag)
    guard = ops.IdRangeGuard("test ids")
    guard.watch(flag)
    with pytest.raises(IndexError):
        guard.check()
    for k, ts in st["full"].items():
        for t, gd in zip(ts, guards[k]):
            assert torch.equal(t[-pad:], gd), f"{k}: a row past the vocab was written"
    ref = REF.gradients(params, x_safe, y, "mean", drop=[(bad_r, bad_f)])
    _check_gradients(res, ref, x_safe, "bad id")
    # the update itself: one SparseAdam step of the reference from the same gradients
    rt = REF.RefTrainer(params, lr=LR)
    rt.step(x_safe, y, drop=[(bad_r, bad_f)])
    for got, r in zip(st["emb"] + st["lin"], rt.tables):
        frac, mx = REF.cap_violations(got.cpu().reshape(r.shape), r, LR)
        assert frac <= 1e-3 and mx <= 3.0
    # the moments are linear / quadratic in the gradient (zero before the step), so they show a leaked
    # contribution that a sign-like first update would hide: the gradient bound, on every row
    ref_m, ref_v = rt.moments()
    for what, got_l, ref_l in (("m", st["emb_m"] + st["lin_m"], ref_m), ("v", st["emb_v"] + st["lin_v"], ref_v)):
        for i, (got, r) in enumerate(zip(got_l, ref_l)):
            assert _ratio(got, r) <= 1e-3, f"{what}[{i}]"
            untouched = r.reshape(r.shape[0], -1).abs().sum(1) == 0
            assert not got.cpu().reshape(r.shape[0], -1)[untouched].any(), f"{what}[{i}]: an untouched row has moments"

    # the trainer reports it
    model = _model(params, gpu)
    emb, lin, _, _, _ = model._param_lists()
    for n, fe, fl in zip(model.field_names, st["full"]["emb"], st["full"]["lin"]):
        model.embedding_dict[n].weight = torch.nn.Parameter(fe[:-pad])
        model.linear_model.embedding_dict[n].weight = torch.nn.Parameter(fl[:-pad])
    tr = model.make_trainer(lr=LR)
    tr.emb_m, tr.emb_v, tr.lin_m, tr.lin_v = st["emb_m"], st["emb_v"], st["lin_m"], st["lin_v"]
    tr.step(x_bad.to(gpu), y.to(gpu))
    with pytest.raises(IndexError):
        tr.check_ids()


def test_fit(gpu):
    R, vocabs, bs = 1000, [50] * 5, 384
    params = REF.make_params(vocabs, seed=10)
    x, y = _batch(R, vocabs, "zipf", seed=33)
    means = _model(params, gpu).fit(x, y, batch_size=bs, epochs=2, lr=LR)
    assert len(means) == 2 and all(torch.isfinite(torch.tensor(means)))
    fitted = _model(params, gpu).fit(x, y, batch_size=bs, epochs=2, shuffle=False, lr=LR)
    model = _model(params, gpu)
    tr = model.make_trainer(lr=LR)
    manual = []
    for _ in range(2):
        total = torch.zeros((), device=gpu, dtype=torch.float64)
        for s in range(0, R, bs):
            xb, yb = x[s:s + bs].to(gpu), y[s:s + bs].to(gpu)
            total += tr.step(xb, yb) * xb.shape[0]
        manual.append(float((total / R).item()))
    assert fitted == manual


def test_state_dict_resumes_identically(gpu):
    """Save after one step, take a second step; a fresh model + trainer loaded from the saved state
    takes the same second step bit for bit. The snapshot holds copies, not the live moments."""
    R, vocabs, _ = SHAPES["tail_dups"]
    params = REF.make_params(vocabs, seed=12)
    b1, b2 = _batch(R, vocabs, "zipf", seed=40), _batch(R, vocabs, "zipf", seed=41)
    model = _model(params, gpu)
    tr = model.make_trainer(lr=LR)
    tr.step(b1[0].to(gpu), b1[1].to(gpu))
    sd = tr.state_dict()
    weights = {k: v.clone() for k, v in model.state_dict().items()}
    saved_m = [t.clone() for t in sd["emb_m"]]
    tr.step(b2[0].to(gpu), b2[1].to(gpu))
    assert sd["step"] == 1 and all(torch.equal(a, b) for a, b in zip(sd["emb_m"], saved_m))
    model2 = _model(params, gpu)
    model2.load_state_dict(weights)
    tr2 = model2.make_trainer(lr=LR)
    tr2.load_state_dict(sd)
    tr2.step(b2[0].to(gpu), b2[1].to(gpu))
    assert tr2.step_count == tr.step_count == 2
    for (n, a), (_, b) in zip(_model_tensors(model), _model_tensors(model2)):
        assert torch.equal(a, b), n
    for name in ("emb_m", "emb_v", "lin_m", "lin_v"):
        for a, b in zip(getattr(tr, name), getattr(tr2, name)):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("native", [True, False])
def test_max_grad_norm_clips_the_dense_gradients(gpu, monkeypatch, native):
    """One step with max_grad_norm at half the dense gradient norm, through rsx_clip_adamw and through
    the clip_grad_norm_ + optimizer.step() fallback: Adam's exp_avg after the step is 0.1 x the clipped
    gradient, so it shows the clip factor (the gradient bound: 1e-3 of the reference's max-abs)."""
    R, vocabs, _ = SHAPES["tail_dups"]
    params = REF.make_params(vocabs, seed=13)
    x, y = _batch(R, vocabs, "zipf", seed=42)
    _, _, dense, _ = REF.gradients(params, x, y)
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in dense.values())))
    rt = REF.RefTrainer(params, lr=LR)
    rt.step(x, y, max_grad_norm=0.5 * norm)
    monkeypatch.setattr(ops, "_CLIP_ADAMW", native)
    model = _model(params, gpu)
    tr = model.make_trainer(lr=LR, max_grad_norm=0.5 * norm)
    tr.step(x.to(gpu), y.to(gpu))
    unclipped = 0.1 * dense["w1"]
    for p, k in zip(tr.dense, REF.DENSE):
        got, ref = tr.optimizer.state[p]["exp_avg"], rt.dense_opt.state[rt.p[k]]["exp_avg"]
        assert _ratio(got, ref) <= 1e-3, k
    assert _ratio(tr.optimizer.state[tr.dense[0]]["exp_avg"], unclipped) > 0.4   # the clip halved it
    for (n, got), (_, r) in zip(_model_tensors(model), REF.all_tensors(rt.p)):
        frac, mx = REF.cap_violations(got.detach().cpu().reshape(r.shape), r, LR)
        assert frac <= 1e-3 and mx <= 3.0, n
