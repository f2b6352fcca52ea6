"""gnn_model.distill_mag_to_cos_l2 on the device against the float64 reference of tests/distill_ref.py:
the eval forward per element, one step's loss / gradients / scores at every batch size where the tiling
changes (with and without dropout, masks rebuilt on the host), bit-reproducibility, three fused Adam
steps, the out-of-range id flag, train_projector against a manual step loop and project_tables through
the retrieval kernel.

Tables of 301 users x 200 items (unit directions times a log-normal length, item 0 the zero padding
row); batches with repeated users, repeated items and item 0. Tolerances are the project's for this
model family (tests/test_gpu_lightgcl.py): loss 1e-5 relative, each gradient within 1e-4 of its float64
max, parameters after Adam steps at lr 1e-3 within 1e-5 wherever every step's float64 gradient is
resolved (oracle/agreement.py's rule), the unresolved share capped at 1 % of any tensor.
The tile size T and the slot rule are read from the library."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import recsys_amd  # noqa: F401
from recsys_amd import _native, ops
from recsys_amd.gnn_model import distill_mag_to_cos_l2 as DM
from recsys_amd.gnn_model import v1_evaluate_lightgcl as EV
from recsys_amd.gnn_model import v1_lightgcl as G
from tests import distill_ref as REF

pytestmark = pytest.mark.gpu

NU, NI = 301, 200
LOSS_RTOL, GRAD_TOL, PARAM_TOL, SCORE_RTOL, LR = 1e-5, 1e-4, 1e-5, 1e-5, 1e-3
UNRESOLVED_CAP = 0.01
NAMES = ("w1", "b1", "w2", "b2", "logit_scale")


@functools.lru_cache(maxsize=None)
def _tables():
    return REF.make_tables(NU, NI, 24)   # a seed whose first eight users have no near-tie (see the last test)


@functools.lru_cache(maxsize=None)
def _state():
    torch.manual_seed(0)
    return {k: v.clone() for k, v in DM.MagnitudeEncoder().state_dict().items()}


def _module(gpu, zero_w2=False):
    m = DM.MagnitudeEncoder()
    m.load_state_dict(_state())
    if zero_w2:
        with torch.no_grad():
            m.encoder[3].weight.zero_()
            m.encoder[3].bias.zero_()
    return m.to(gpu)


def _params(m):
    return [m.encoder[0].weight, m.encoder[0].bias, m.encoder[3].weight, m.encoder[3].bias, m.logit_scale]


def _cpu(ps):
    return [p.detach().cpu().clone() for p in ps]


@functools.lru_cache(maxsize=None)
def _batch(B, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    users, items = torch.randint(0, NU, (B,), generator=g), torch.randint(1, NI, (B,), generator=g)
    k = B // 8
    if k:
        users[:k] = users[k:2 * k]              # repeated users
        items[2 * k:3 * k] = items[3 * k:4 * k]  # repeated items
    if B > 1:
        items[B // 2] = 0                       # the padding row
    return users, items


def _tile_sizes():
    lib = _native.lib()
    T = int(lib.rsx_distill_rows_per_workgroup())
    return T, (lambda b: (b + T - 1) // T), (lambda b: int(lib.rsx_distill_slots(b)))


def _batch_size(label):
    T, tiles, slots = _tile_sizes()
    fixed = {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "257": 257}
    if label in fixed:
        return fixed[label]
    b = 1     # the tile count changes at B = k T + 1 only
    while True:
        assert b < (1 << 20)
        second = tiles(b) > slots(b)
        if label == "second_tile" and second:
            return b
        if label == "short_last" and second and tiles(b) % slots(b):
            return b
        b += T


def _check_loss(got, want, what):
    got = float(got)
    print(f"{what} loss: got {got:.9g} f64 {want:.9g} rel {abs(got - want) / abs(want):.3g}")
    assert abs(got - want) <= LOSS_RTOL * abs(want), (what, got, want)


def _check_grads(got, want, what):
    errs = []
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, name
        errs.append(float((g.cpu().double() - w).abs().max()) / float(w.abs().max()))
        print(f"{what} grad {name}: max err / max |f64 grad| = {errs[-1]:.3g}")
    assert max(errs) <= GRAD_TOL, (what, errs)


def _check_scores(out, ref, what):
    for name, g, w in (("student", out.student_scores, ref["student"]), ("teacher", out.teacher_scores, ref["teacher"])):
        err = float((g.cpu().double() - w).abs().max())
        scale = float(w.abs().max())
        print(f"{what} {name} scores: max err {err:.3g}, max |f64| {scale:.3g}")
        assert err <= SCORE_RTOL * scale, (what, name)


def _step(gpu, m, users, items, **kw):
    U, I = _tables()
    lin1, act, _, lin2 = m.encoder
    return ops.distill_step(U.to(gpu), I.to(gpu), users.to(gpu), items.to(gpu), lin1.weight, lin1.bias, lin2.weight,
                            lin2.bias, m.logit_scale, slope=act.negative_slope, **kw)


# ---------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n", ["1", "63", "64", "65", "4T+1"])
def test_forward_against_float64(gpu, n):
    T = _tile_sizes()[0]
    n = 4 * T + 1 if n == "4T+1" else int(n)
    U, I = _tables()
    x = torch.cat([I[:3], U])[:n].contiguous()    # starts with the zero row
    assert x.shape[0] == n
    m = _module(gpu).eval()
    with torch.no_grad():
        y = m(x.to(gpu))
    want = REF.forward(x.double(), _cpu(_params(m)))[5]
    assert y.shape == (n, 64) and y.dtype == torch.float32
    err = float((y.cpu().double() - want).abs().max())
    print(f"N={n}: max |y - f64| {err:.3g}")
    assert err <= 1e-6
    assert float((y.double().norm(dim=1) - 1).abs().max()) <= 1e-6


def test_forward_of_degenerate_rows_is_exactly_zero(gpu):
    m = _module(gpu, zero_w2=True).eval()
    with torch.no_grad():
        y = m(_tables()[0][:70].to(gpu))
    assert y.shape == (70, 64) and int(torch.count_nonzero(y)) == 0


def test_forward_reads_strided_rows(gpu):
    U = _tables()[0].to(gpu)
    wide = torch.zeros(NU, 72, device=gpu)
    wide[:, 4:68] = U
    m = _module(gpu).eval()
    with torch.no_grad():
        assert torch.equal(m(wide[:, 4:68]), m(U))


def test_module_forward_paths(gpu, monkeypatch):
    calls = []
    real = ops.magnitude_encode
    monkeypatch.setattr(ops, "magnitude_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = _module(gpu)
    x = _tables()[0][:10].to(gpu)
    m.eval()
    with torch.no_grad():
        y = m(x)
    assert len(calls) == 1 and not y.requires_grad
    m.train()                                      # dropout p = 0.1 is active: the torch composition
    with torch.no_grad():
        m(x)
    assert len(calls) == 1
    m.eval()
    xg = x.clone().requires_grad_(True)            # autograd is recording: the torch composition
    yg = m(xg)
    assert len(calls) == 1 and yg.requires_grad
    assert float((yg.detach() - y).abs().max()) <= 1e-6
    m.encoder[2].p = 0.0                           # p == 0: the kernel also in train mode
    m.train()
    with torch.no_grad():
        assert torch.equal(m(x), y)
    assert len(calls) == 2
    with torch.no_grad():                          # other dtypes: the torch composition
        m.double()(x.double())
    assert len(calls) == 2


# ---------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("label", ["1", "2", "T-1", "T", "T+1", "257", "second_tile", "short_last"])
def test_step_loss_gradients_and_scores(gpu, label, p):
    B = _batch_size(label)
    T, tiles, slots = _tile_sizes()
    if label == "second_tile":
        assert tiles(B) > slots(B) and tiles(B - 1) <= slots(B - 1)
    if label == "short_last":
        assert tiles(B) % slots(B) and tiles(B) > slots(B)
    users, items = _batch(B)
    U, I = _tables()
    m = _module(gpu)
    seed = 0x5EED0000 + B
    ref = REF.step(REF.stack(U, I, users, items), _cpu(_params(m)), 0.2, REF.keep_scale(seed, p, B))
    out = _step(gpu, m, users, items, p_drop=p, seed=seed, update=False, return_grads=True, return_scores=True)
    what = f"B={B} p={p}"
    assert out.loss.dtype == torch.float64 and out.loss.dim() == 0 and out.loss.device.type == "cuda"
    _check_loss(out.loss, float(ref["loss"]), what)
    _check_grads(out.grads, ref["grads"], what)
    _check_scores(out, ref, what)
    assert int(out.flag) == 0
    assert all(torch.equal(p_.detach().cpu(), _state()[k]) for k, p_ in m.state_dict().items())   # update=False


def test_step_with_degenerate_rows(gpu):
    """W2 = 0, b2 = 0: every |Z| < eps, dZ = dY / eps with dY = 0: finite gradients, float64's (all 0)."""
    users, items = _batch(40)
    U, I = _tables()
    m = _module(gpu, zero_w2=True)
    ref = REF.step(REF.stack(U, I, users, items), _cpu(_params(m)))
    out = _step(gpu, m, users, items, update=False, return_grads=True, return_scores=True)
    _check_loss(out.loss, float(ref["loss"]), "W2 = 0")
    for name, g, w in zip(NAMES, out.grads, ref["grads"]):
        assert torch.isfinite(g).all(), name
        assert float(w.abs().max()) == 0.0 and int(torch.count_nonzero(g)) == 0, name
    assert int(torch.count_nonzero(out.student_scores)) == 0


def test_step_forward_is_the_eval_forward_bit_for_bit(gpu):
    """The step's forward at p = 0 against ops.magnitude_encode over the same stacked rows. The
    comparison is on the normalised rows (the step's optional rows output): the scores' own reduction
    (fmaf chains and a shuffle tree, then exp(logit_scale) from the device's expf) has no bit-exact
    torch restatement, so the scores are only checked to follow from those rows within rounding."""
    T = _tile_sizes()[0]
    B = 2 * T + 5
    users, items = _batch(B)
    U, I = _tables()
    m = _module(gpu)
    out = _step(gpu, m, users, items, update=False, return_scores=True, return_rows=True)
    X = torch.cat([U[users], I[items]]).to(gpu)
    ps = _params(m)
    y = ops.magnitude_encode(X, *ps[:4])
    assert out.rows.shape == (2 * B, 64) and torch.equal(out.rows, y)
    s = (y[:B].double() * y[B:].double()).sum(1) * ps[4].detach().double().exp()
    assert float((out.student_scores.double() - s).abs().max()) <= 1e-5 * float(s.abs().max())
    # dropout's mask at p = 0 is the identity whatever the seed
    again = _step(gpu, m, users, items, seed=12345, update=False, return_rows=True)
    assert torch.equal(again.rows, y)


def test_step_is_bit_reproducible(gpu):
    users, items = _batch(257)
    runs = []
    for _ in range(2):
        m = _module(gpu)
        out = _step(gpu, m, users, items, p_drop=0.1, seed=99, update=False, return_grads=True, return_scores=True,
                    return_rows=True)
        runs.append([out.loss, out.student_scores, out.teacher_scores, out.rows] + list(out.grads))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------- Adam
def _check_params(got, steps, what):
    """got against the last of the float64 steps, wherever no step's gradient is unresolved."""
    for k, (name, p) in enumerate(zip(NAMES, got)):
        unres = torch.zeros(p.shape, dtype=torch.bool)
        for st in steps:
            gr = st["grads"][k]
            unres |= gr.abs() <= GRAD_TOL * float(gr.abs().max())
        share = float(unres.double().mean())
        diff = (p.detach().cpu().double() - steps[-1]["params"][k]).abs()
        worst = float(diff[~unres].max())
        print(f"{what} {name}: unresolved {share:.4f}, worst resolved diff {worst:.3g}, worst diff {float(diff.max()):.3g}")
        assert share <= UNRESOLVED_CAP, (what, name, share)
        assert worst <= PARAM_TOL, (what, name, worst)


def test_three_adam_steps_track_float64(gpu):
    B = 257
    U, I = _tables()
    Ug, Ig = U.to(gpu), I.to(gpu)
    torch.manual_seed(77)
    seeds = [ops.next_seed() for _ in range(3)]
    batches = [_batch(B, s) for s in range(3)]
    m = _module(gpu).train()
    ref = REF.adam_train(_cpu(_params(m)), [(REF.stack(U, I, u, i), REF.keep_scale(sd, 0.1, B), None)
                                            for (u, i), sd in zip(batches, seeds)], lr=LR)
    tr = m.make_trainer(lr=LR)
    torch.manual_seed(77)      # the trainer draws the same three seeds
    ls0 = float(m.logit_scale.detach())
    for s, (u, i) in enumerate(batches):
        loss = tr.step(Ug, Ig, u.to(gpu), i.to(gpu))
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.device.type == "cuda"
        _check_loss(loss, ref[s]["loss"], f"step {s + 1}")
        _check_params(_params(m), ref[:s + 1], f"step {s + 1}")
    assert tr.steps == 3
    assert abs(float(m.logit_scale.detach()) - ls0) > 1e-3
    tr.check()
    # the same three steps through a fresh trainer, seeds given: identical bits, moments included
    m2 = _module(gpu).train()
    tr2 = m2.make_trainer(lr=LR)
    for (u, i), sd in zip(batches, seeds):
        tr2.step(Ug, Ig, u.to(gpu), i.to(gpu), seed=sd)
    for a, b in zip(_params(m), _params(m2)):
        assert torch.equal(a, b)
    assert torch.equal(tr.exp_avg, tr2.exp_avg) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)
    assert float(tr.exp_avg_sq.min()) >= 0 and int(torch.count_nonzero(tr.exp_avg)) > 16000


def test_eval_mode_trainer_uses_no_dropout(gpu):
    users, items = _batch(40)
    U, I = _tables()
    m = _module(gpu).eval()
    ref = REF.adam_train(_cpu(_params(m)), [(REF.stack(U, I, users, items), None, None)], lr=LR)
    state = torch.random.get_rng_state()
    loss = m.make_trainer(lr=LR).step(U.to(gpu), I.to(gpu), users.to(gpu), items.to(gpu))
    assert torch.equal(torch.random.get_rng_state(), state)     # no seed drawn
    _check_loss(loss, ref[0]["loss"], "eval")
    _check_params(_params(m), ref, "eval")


def test_out_of_range_id_raises_at_check_and_contributes_nothing(gpu):
    B = 40
    users, items = (t.clone() for t in _batch(B))
    users[5] = NU
    U, I = _tables()
    m = _module(gpu).eval()
    tr = m.make_trainer(lr=LR)
    loss = tr.step(U.to(gpu), I.to(gpu), users.to(gpu), items.to(gpu))
    with pytest.raises(IndexError, match="out of range"):
        tr.check()
    tr.check()       # reported once
    keep = torch.arange(B) != 5
    ref = REF.adam_train(_cpu(_params(_module(gpu))), [(REF.stack(U, I, users[keep], items[keep]), None, B)], lr=LR)
    _check_loss(loss, ref[0]["loss"], "pair dropped")
    _check_params(_params(m), ref, "pair dropped")
    items[7] = -1
    out = _step(gpu, m, users, items, update=False)
    assert int(out.flag) == 1


# ---------------------------------------------------------------------------------------- train_projector
class _Teacher(nn.Module):
    def __init__(self):
        super().__init__()
        U, I = _tables()
        self.embedding_user = nn.Embedding.from_pretrained(U.clone(), freeze=False)
        self.embedding_item = nn.Embedding.from_pretrained(I.clone(), freeze=False)


def test_train_projector_is_the_manual_step_loop(gpu):
    g = torch.Generator().manual_seed(3)
    edges = torch.stack([torch.randint(0, NU, (1000,), generator=g), torch.randint(1, NI, (1000,), generator=g)])
    ds = G.TrainDataset(edges.to(gpu), NU, NI)
    bs, epochs = 96, 2
    assert 1000 % bs
    teacher = _Teacher().to(gpu).train()
    lines = []
    torch.manual_seed(5)
    proj = DM.train_projector(teacher, DM.edge_batches(ds, bs, generator=torch.Generator().manual_seed(9)), gpu,
                              epochs=epochs, lr=LR, log=lines.append)
    assert not teacher.training and isinstance(proj, DM.MagnitudeEncoder)
    assert len(lines) == 1 + epochs
    # the same steps by hand, seeds and batches recorded for the float64 loop
    torch.manual_seed(5)
    m = DM.MagnitudeEncoder().to(gpu)
    start = _cpu(_params(m))
    tr = m.make_trainer(lr=LR)
    loader = DM.edge_batches(ds, bs, generator=torch.Generator().manual_seed(9))
    U, I = _tables()
    Ug, Ig = U.to(gpu), I.to(gpu)
    record, losses = [], []
    for _ in range(epochs):
        m.train()
        for users, items, _ in loader:
            state = torch.random.get_rng_state()
            seed = ops.next_seed()
            torch.random.set_rng_state(state)
            losses.append(tr.step(Ug, Ig, users, items))
            record.append((users.cpu(), items.cpu(), seed))
    for a, b in zip(_params(proj), _params(m)):
        assert torch.equal(a, b)
    per_epoch = len(loader)
    assert per_epoch == 11 and len(losses) == epochs * per_epoch
    ref = REF.adam_train(start, [(REF.stack(U, I, u, i), REF.keep_scale(sd, 0.1, u.numel()), None)
                                 for u, i, sd in record], lr=LR)
    for e in range(epochs):
        got = float(torch.stack(losses[e * per_epoch:(e + 1) * per_epoch]).sum()) / per_epoch
        want = sum(r["loss"] for r in ref[e * per_epoch:(e + 1) * per_epoch]) / per_epoch
        _check_loss(got, want, f"epoch {e + 1} mean")
        assert lines[1 + e] == f"Epoch {e + 1}/{epochs} | Distillation Loss: {got:.4f}"


def test_train_projector_reports_an_out_of_range_id(gpu):
    teacher = _Teacher().to(gpu)
    bad = [(torch.tensor([1, 2, NU]), torch.tensor([3, 4, 5]), None)]
    with pytest.raises(IndexError, match="out of range"):
        DM.train_projector(teacher, bad, gpu, epochs=1, log=lambda s: None)


def test_project_tables_feed_the_retrieval(gpu):
    teacher = _Teacher().to(gpu)
    proj = _module(gpu).train()
    user_unit, item_unit = DM.project_tables(proj, teacher)
    assert proj.training
    assert user_unit.shape == (NU, 64) and item_unit.shape == (NI, 64)
    for t in (user_unit, item_unit):
        assert float((t.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    scores = (user_unit[:8].cpu().double() @ item_unit.cpu().double().t()).numpy()[:, 1:]
    order = np.argsort(-scores, axis=1, kind="stable")
    top6 = np.take_along_axis(scores, order[:, :6], axis=1)
    gap = float((top6[:, :-1] - top6[:, 1:]).min())
    print(f"smallest gap among the float64 top-6 scores: {gap:.3g}")
    assert gap > 1e-5          # the fixture: no ties a rounding could reorder
    top = EV.topk_items(user_unit[:8], item_unit, 5)
    assert np.array_equal(top.cpu().numpy(), order[:, :5] + 1)
