"""The QuerySoftMax kernels (csrc/gbdt_rank.hip) against the float64 softmax and the int64 oracle of
tests/gbdt_rank_ref.py: the gradients, their exact properties (row order, run to run, groups without a
positive), the monitoring loss and the argument checks. The rows of every case and their references are
made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import _native as N
from recsys_amd import ops
from tests import gbdt_rank_ref as Q
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

LAYOUTS = ("shared", "singles", "long", "one")


def _rows(name):
    """(F float32, y float32, gid int64) of a layout: N(0, 4) scores with +-30 planted; in the shared layout
    the group of 257 rows spans 200 (its E underflows to 0) and the group of 65 rows has equal scores."""
    rng = np.random.default_rng(LAYOUTS.index(name) + 40)
    if name == "shared":
        gid = Q.layout(4096, 7)
    elif name == "singles":
        gid = 2 * rng.permutation(3001).astype(np.int64)
    elif name == "long":
        gid = np.full(70001, 12, np.int64)
    else:
        gid = np.asarray([7], np.int64)
    R = len(gid)
    F = (2.0 * rng.standard_normal(R)).astype(np.float32)
    y = (rng.random(R) < 0.3).astype(np.float32)
    if R > 1:
        F[rng.choice(R, 2, replace=False)] = (30.0, -30.0)
    else:
        y[:] = 1.0
    if name == "shared":
        ids, counts = np.unique(gid, return_counts=True)
        wide, flat = (np.flatnonzero(gid == ids[list(counts).index(n)]) for n in (257, 65))
        F[wide] = np.linspace(-100.0, 100.0, 257).astype(np.float32)
        F[flat] = np.float32(0.75)
        y[wide], y[wide[:3]] = 0.0, 1.0
        y[flat[:2]], y[flat[2:]] = 1.0, 0.0
    return F, y, gid


def _device(gpu, F, y, gid):
    """(qg, qh) int64 in the rows' own order, the plan, and the grouped device tensors."""
    plan = ops.GBDTGroupPlan(torch.from_numpy(gid), gpu)
    order = plan.order.cpu().numpy()
    Fg, yg = torch.from_numpy(F[order]).to(gpu), torch.from_numpy(y[order]).to(gpu)
    qg, qh = ops.gbdt_grad_query_softmax(Fg, yg, plan)
    out = np.empty((2, len(F)), np.int64)
    out[0, order], out[1, order] = qg.cpu().numpy(), qh.cpu().numpy()
    return out[0], out[1], plan, Fg, yg


@pytest.fixture(scope="module")
def cases(gpu):
    out = {}
    for name in LAYOUTS:
        F, y, gid = _rows(name)
        out[name] = {"rows": (F, y, gid), "dev": _device(gpu, F, y, gid), "g64": Q.grad_plain64(F, y, gid),
                     "oracle": Q.grad(F, y, gid), "loss": Q.loss_sum(F, y, gid)}
    return out


def test_plan_is_the_stable_sort_of_the_ids(cases):
    F, y, gid = cases["shared"]["rows"]
    plan = cases["shared"]["dev"][2]
    order = np.argsort(gid, kind="stable")
    ids, counts = np.unique(gid, return_counts=True)
    assert np.array_equal(plan.order.cpu().numpy(), order) and plan.G == len(ids) and plan.R == len(gid)
    assert np.array_equal(plan.goff.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(plan.row_group.cpu().numpy(), np.searchsorted(ids, gid[order]))
    assert plan.goff.dtype == torch.int32 and plan.row_group.dtype == torch.int32


@pytest.mark.parametrize("name", LAYOUTS)
def test_gradients_match_the_float64_softmax(cases, name):
    """|g - g64| and |h - h64| <= 2e-6, the margin of the Logloss gradient test: 2^-33 in E, two fp32 roundings
    (6e-8 each at |x| <= 1) and 2^-31 in the quantisation. The rows whose integers differ from the oracle's are
    counted, not asserted: the device and numpy may round one fp64 exp differently."""
    c = cases[name]
    qg, qh = c["dev"][:2]
    g64, h64 = c["g64"]
    eg, eh = np.abs(qg / G.SCALE - g64).max(), np.abs(qh / G.SCALE - h64).max()
    differ = int(((qg != c["oracle"][0]) | (qh != c["oracle"][1])).sum())
    print(f"{name}: max |g - g64| {eg:.3e}, max |h - h64| {eh:.3e}; {differ} of {len(qg)} rows differ from the oracle")
    assert eg <= 2e-6 and eh <= 2e-6
    assert np.abs(qg).max() <= 2 ** 30 and qh.min() >= 0 and qh.max() <= 2 ** 28


def test_underflow_equal_scores_and_a_single_row(cases):
    F, y, gid = cases["shared"]["rows"]
    qg, qh = cases["shared"]["dev"][:2]
    ids, counts = np.unique(gid, return_counts=True)
    wide, flat = (np.flatnonzero(gid == ids[list(counts).index(n)]) for n in (257, 65))
    low = wide[F[wide] < -50.0]
    assert len(low) > 50 and not qh[low].any()                       # E = 0: p = 0 exactly
    assert (y[low] == 1).sum() == 3                                  # the group's three positives: g = t = 1 / 3
    assert np.array_equal(qg[low], G.quantise(np.where(y[low] == 1, np.float32(1.0 / 3.0), np.float32(0))))
    p = np.float32(1.0 / 65.0)                                        # equal scores: p = 1 / n
    assert np.array_equal(qh[flat], G.quantise(np.full(65, p * (np.float32(1) - p), np.float32)))
    assert np.array_equal(qg[flat], G.quantise(np.where(y[flat] == 1, np.float32(0.5), np.float32(0)) - p))
    one = cases["one"]
    assert one["dev"][0].tolist() == [0] and one["dev"][1].tolist() == [0]     # p = 1, t = 1


@pytest.mark.parametrize("name", ["shared", "long"])
def test_row_order_does_not_change_a_rows_gradients(gpu, cases, name):
    F, y, gid = cases[name]["rows"]
    qg, qh = cases[name]["dev"][:2]
    perm = np.random.default_rng(5).permutation(len(F))
    pg, ph = _device(gpu, F[perm], y[perm], gid[perm])[:2]
    assert np.array_equal(pg, qg[perm]) and np.array_equal(ph, qh[perm])


@pytest.mark.parametrize("name", ["shared", "long"])
def test_two_runs_give_the_same_bits(cases, name):
    _, _, plan, Fg, yg = cases[name]["dev"]
    a = ops.gbdt_grad_query_softmax(Fg, yg, plan)
    b = ops.gbdt_grad_query_softmax(Fg, yg, plan, out=(torch.empty_like(a[0]), torch.empty_like(a[1])))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    l1, l2 = ops.query_softmax_eval(Fg, yg, plan), ops.query_softmax_eval(Fg, yg, plan)
    assert torch.equal(l1._buf, l2._buf)


@pytest.mark.parametrize("name", ["shared", "singles"])
def test_groups_without_a_positive_give_exact_zeros(cases, name):
    F, y, gid = cases[name]["rows"]
    qg, qh = cases[name]["dev"][:2]
    inv, _, _, _, S = Q.group_sums(F, y, gid)
    dead = S[inv] == 0
    assert dead.any() and (~dead).any()
    assert not qg[dead].any() and not qh[dead].any()
    if name == "shared":       # (a group of one row has p = 1: its h is 0 too)
        assert qh[~dead].any() and qg[~dead].any()


@pytest.mark.parametrize("name", LAYOUTS)
def test_eval_matches_the_oracles_loss(cases, name):
    _, _, plan, Fg, yg = cases[name]["dev"]
    want, live = cases[name]["loss"]
    ev = ops.query_softmax_eval(Fg, yg, plan)
    res = ev.result()
    got = float(ev.loss_sum.cpu()[0])
    print(f"{name}: loss_sum {got!r} (oracle {want!r}), live groups {res['live_groups']} ({live})")
    assert res["live_groups"] == live
    assert abs(got - want) <= 1e-9 * abs(want)
    assert abs(res["loss"] - want / live) <= 1e-9 * abs(want / live)


def test_argument_checks_raise(gpu, cases):
    _, _, plan, Fg, yg = cases["shared"]["dev"]
    with pytest.raises(ValueError, match=">= 0"):
        ops.GBDTGroupPlan(torch.tensor([3, -1, 3]), gpu)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.GBDTGroupPlan(torch.tensor([0.5, 1.0]), gpu)
    with pytest.raises(ValueError):
        ops.gbdt_grad_query_softmax(Fg[:100].contiguous(), yg[:100].contiguous(), plan)
    with pytest.raises(TypeError):
        ops.gbdt_grad_query_softmax(Fg.double(), yg, plan)
    with pytest.raises(TypeError):
        ops.query_softmax_eval(Fg, yg, None)
    lib = N.lib()
    R, Gn = plan.R, plan.G
    qg, qh = (torch.empty(R, device=gpu, dtype=torch.int32) for _ in range(2))
    args = [N.ptr(Fg), N.ptr(yg), N.ptr(plan.row_group), N.ptr(plan.goff), R, Gn, N.ptr(plan.ws), plan.ws.numel(),
            N.ptr(qg), N.ptr(qh), N.stream()]
    for k, bad in ((0, None), (4, 0), (4, 2 ** 31), (5, 0), (5, R + 1), (7, plan.ws.numel() - 1), (6, N.ptr(plan.ws) + 4)):
        call = list(args)
        call[k] = bad
        assert lib.rsx_gbdt_grad_query_softmax(*call) != 0, k
        assert b"invalid argument" in lib.rsx_last_error()
    out = torch.empty(2, device=gpu, dtype=torch.int64)
    ev = args[:8] + [N.ptr(out), N.stream()]
    for k, bad in ((8, None), (5, R + 1), (7, 0)):
        call = list(ev)
        call[k] = bad
        assert lib.rsx_query_softmax_eval(*call) != 0, k
    assert lib.rsx_gbdt_grad_query_softmax_workspace_bytes(10, 11) < 0
    assert lib.rsx_gbdt_grad_query_softmax_workspace_bytes(0, 0) < 0
    assert lib.rsx_gbdt_grad_query_softmax(*args) == 0                 # the untouched arguments still run
