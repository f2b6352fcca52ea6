"""The explanation kernels (csrc/gbdt_explain.hip) against the float64 oracle of tests/gbdt_explain_ref.py.
Row counts: 1 (a single lane), 63 (under one wave), 257 (one row past a workgroup) and 4097 (many workgroups
with a ragged tail); 1, 12 and 32 columns; depth 1, 3 and 6. rsx_gbdt_shap stages its trees through LDS
rsx_gbdt_shap_tree_chunk() at a time, so its 6 more trees cross a chunk boundary. Among the random trees: one
feature on every level, categorical splits on every level, a split no row passes (a zero-weight half-tree), a
feature out of range (read as feature 0), and, in the weights the plan and the SHAP tests use, a zeroed half
and a tree without any weight."""
import numpy as np
import pytest
import torch

from recsys_amd import _native, ops
from tests import gbdt_explain_ref as E
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 257, 4097]
COLS = [1, 12, 32]
DEPTHS = [1, 3, 6]
F0 = np.float32(-1.3)


def _dev(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


def _chunk():
    return int(_native.lib().rsx_gbdt_shap_tree_chunk())


_CASES = {}


def _case(R, F, depth):
    """The rows of gbdt_ref.make (column 0 rebinned to use every bin; 20 more random columns for F = 32), T random
    trees and the oracle's weights, table, pvc and SHAP values. Built once per (R, F, depth), never changed."""
    key = (R, F, depth)
    if key in _CASES:
        return _CASES[key]
    num, cat, _ = G.make(R, 100 + R)
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    rng = np.random.default_rng(1000 * R + 10 * F + depth)
    bins[0] = rng.integers(0, 256, R)
    n_bins = n_bins.copy()
    n_bins[0] = 256
    if F > 12:
        bins = np.concatenate([bins, rng.integers(0, 256, (F - 12, R)).astype(np.uint8)])
        is_cat = np.concatenate([is_cat, np.zeros(F - 12, np.uint8)])
        n_bins = np.concatenate([n_bins, np.full(F - 12, 256, np.int32)])
    bins, is_cat, n_bins = np.ascontiguousarray(bins[:F]), is_cat[:F].copy(), n_bins[:F]
    T = _chunk() + 6
    f = rng.integers(0, F, (T, 6))
    b = (rng.random((T, 6)) * (n_bins[f] - 1)).astype(np.int64)
    f[1] = F - 1                                   # one feature on every level
    if F >= 12:
        f[2] = [7, 8, 9, 10, 11, 9]                # categorical splits on every level
        b[2] = [1, 0, 3, 2, 1, 7]
    f[3, 0], b[3, 0] = 0, 255                      # no bin is above 255: the right half has no weight
    f[4, 1] = F + 3                                # out of range: reads as feature 0
    splits = np.zeros((T, 6, 2), np.int64)         # levels at and beyond depth stay 0 and are never read
    splits[:, :depth, 0], splits[:, :depth, 1] = f[:, :depth], b[:, :depth]
    values = np.zeros((T, 64), np.float32)
    values[:, :1 << depth] = (rng.standard_normal((T, 1 << depth)) * 0.1).astype(np.float32)
    used = E.clamp_features(splits[:, :depth], F)
    w = E.leaf_weights(bins, used, is_cat)
    w2 = w.copy()
    w2[5, (1 << depth) // 2:1 << depth] = 0        # a zeroed half
    w2[6] = 0                                      # a tree without any weight
    n = 1 << depth
    c = {"bins": bins, "is_cat": is_cat, "splits": splits, "used": used, "values": values, "w": w, "w2": w2, "T": T,
         "table": np.stack([E.cond_table(values[t, :n], w2[t, :n], depth) for t in range(T)]),
         "pvc": np.stack([E.level_pvc(values[t, :n], w2[t, :n], depth) for t in range(T)]),
         "phi": {end: E.shap(bins, F0, used, values, is_cat, w2, end) for end in (0, 1, T)}}
    _CASES[key] = c
    return c


def _model(c, depth, gpu):
    return ops.GBDTModel(_dev(c["splits"], gpu, torch.int32), _dev(c["values"], gpu), _dev(c["is_cat"], gpu), depth,
                         float(F0), c["T"])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("F", COLS)
@pytest.mark.parametrize("R", ROWS)
def test_leaf_weights_are_bit_exact(gpu, R, F, depth):
    c = _case(R, F, depth)
    model, bins = _model(c, depth, gpu), _dev(c["bins"], gpu)
    got = ops.gbdt_leaf_weights(bins, model)
    assert got.dtype == torch.int64 and got.shape == (c["T"], 64)
    assert np.array_equal(got.cpu().numpy(), c["w"])
    assert (c["w"].sum(1) == R).all() and not c["w"][:, 1 << depth:].any()
    if R >= 63:
        assert not c["w"][3, (1 << depth) // 2:].any()       # the zero-weight half-tree
    assert torch.equal(ops.gbdt_leaf_weights(bins, model), got)
    head = ops.gbdt_leaf_weights(bins, model, ntree_end=3).cpu().numpy()
    assert np.array_equal(head[:3], c["w"][:3]) and not head[3:].any()
    # a tree sub-range zeroes and counts its own rows only
    buf = torch.full((c["T"], 64), 7, dtype=torch.int64, device=gpu)
    t0, t1 = 2, c["T"] - 1
    _native.check(_native.lib().rsx_gbdt_leaf_weights(_native.ptr(bins), R, F, _native.ptr(model.splits),
                                                      _native.ptr(model.is_cat), depth, t0, t1, _native.ptr(buf),
                                                      _native.stream()), "gbdt_leaf_weights")
    sub = buf.cpu().numpy()
    assert np.array_equal(sub[t0:t1], c["w"][t0:t1]) and (sub[:t0] == 7).all() and (sub[t1:] == 7).all()
    # a second call into the same tensor over other rows replaces the counts
    if R > 1:
        other = np.ascontiguousarray(c["bins"][:, R // 2:])
        assert ops.gbdt_leaf_weights(_dev(other, gpu), model, out=got) is got
        assert np.array_equal(got.cpu().numpy(), E.leaf_weights(other, c["used"], c["is_cat"]))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("R", [63, 4097])
def test_plan_against_the_float64_recursion(gpu, R, depth):
    """table within 1e-14 max|leaf_t|: four roundings per level at depth <= 6 are 24 x 2^-53 = 2.7e-15, with about
    4x margin (contraction may change bits, so bit equality is not asked); pvc within 1e-14 (sum w) (2 max|leaf_t|)^2."""
    c = _case(R, 12, depth)
    model = _model(c, depth, gpu)
    plan = ops.gbdt_explain_plan(model, _dev(c["w2"], gpu))
    assert plan.table.shape == (c["T"], 729) and plan.pvc.shape == (c["T"], 6) and plan.n_trees == c["T"]
    table, pvc = plan.table.cpu().numpy(), plan.pvc.cpu().numpy()
    peak = np.abs(c["values"]).max(1).astype(np.float64)
    n = 3 ** depth
    err = np.abs(table[:, :n] - c["table"]).max(1)
    print(f"R {R}, depth {depth}: max table error / max|leaf| {np.max(err / peak):.2e}")
    assert (err <= 1e-14 * peak).all()
    tol = 1e-14 * c["w2"].sum(1) * (2 * peak) ** 2
    perr = np.abs(pvc[:, :depth] - c["pvc"]).max(1)
    print(f"R {R}, depth {depth}: max pvc error {perr.max():.2e} (bound {tol.max():.2e})")
    assert (perr <= tol).all() and not pvc[:, depth:].any()
    assert not c["pvc"][6].any() and not pvc[6].any()          # the tree without weights
    assert torch.equal(ops.gbdt_explain_plan(model, _dev(c["w2"], gpu)).table, plan.table)
    head = ops.gbdt_explain_plan(model, _dev(c["w2"], gpu), ntree_end=2)
    assert head.n_trees == 2 and torch.equal(head.table[:2], plan.table[:2]) and not head.table[2:].any()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("F", COLS)
@pytest.mark.parametrize("R", ROWS)
def test_shap_against_the_float64_oracle(gpu, R, F, depth):
    """Every entry within 1e-12 B, B = |f0| + sum_t max|leaf_t|: per (row, tree) the table's error, 64 weighted
    differences of size <= 2 max|leaf_t| and a sequential sum over the trees stay below about 10^3 2^-53 B."""
    c = _case(R, F, depth)
    T = c["T"]
    assert T > _chunk()
    model, bins = _model(c, depth, gpu), _dev(c["bins"], gpu)
    plan = ops.gbdt_explain_plan(model, _dev(c["w2"], gpu))
    for end in (0, 1, T):
        s64, _, bound = G.predict(c["bins"], F0, c["used"], c["values"], c["is_cat"], end)
        phi = ops.gbdt_shap(bins, model, plan, ntree_end=end)
        assert phi.dtype == torch.float64 and phi.shape == (F + 1, R)
        got = phi.cpu().numpy()
        err = np.abs(got - c["phi"][end]).max()
        add = np.abs(got.sum(0) - s64).max()
        print(f"R {R}, F {F}, depth {depth}, {end} trees: max |phi - oracle| {err:.2e}, max |sum - score| {add:.2e} "
              f"(bound {1e-12 * bound:.2e})")
        assert err <= 1e-12 * bound
        assert add <= 1e-12 * bound
        absent = [j for j in range(F) if j not in set(c["used"][:end, :, 0].ravel().tolist())]
        assert not got[absent].any()                         # exactly 0
        if end == 1 and F == 32:
            assert len(absent) >= F - depth
        if end == 0:
            assert (got[F] == np.float64(F0)).all()
    assert torch.equal(ops.gbdt_shap(bins, model, plan), phi)         # two calls, equal bits
    if R > 1:
        half = R // 2
        first = ops.gbdt_shap(_dev(c["bins"][:, :half], gpu), model, plan)
        assert torch.equal(first, phi[:, :half])                      # the bits do not depend on R or the grid
    out = torch.empty(F + 1, R, dtype=torch.float64, device=gpu)
    assert ops.gbdt_shap(bins, model, plan, out=out) is out and torch.equal(out, phi)


def test_argument_checks(gpu):
    c = _case(63, 12, 3)
    model, bins = _model(c, 3, gpu), _dev(c["bins"], gpu)
    w = _dev(c["w2"], gpu)
    plan = ops.gbdt_explain_plan(model, w)
    with pytest.raises(TypeError):
        ops.gbdt_leaf_weights(bins.int(), model)
    with pytest.raises(ValueError):
        ops.gbdt_leaf_weights(bins, model, ntree_end=c["T"] + 1)
    with pytest.raises(ValueError):
        ops.gbdt_leaf_weights(bins, model, out=torch.zeros(c["T"], 32, dtype=torch.int64, device=gpu))
    with pytest.raises(TypeError):
        ops.gbdt_leaf_weights(bins, model, out=torch.zeros(c["T"], 64, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        ops.gbdt_leaf_weights(bins[:5], model)               # is_cat holds 12 columns
    with pytest.raises(TypeError):
        ops.gbdt_explain_plan(model, w.int())
    with pytest.raises(ValueError):
        ops.gbdt_explain_plan(model, w[:3])
    with pytest.raises(RuntimeError):
        ops.gbdt_explain_plan(model, w.cpu())
    with pytest.raises(TypeError):
        ops.gbdt_shap(bins, model, (plan.table, plan.pvc))
    with pytest.raises(ValueError):
        ops.gbdt_shap(bins, model, ops.gbdt_explain_plan(model, w, ntree_end=2), ntree_end=3)
    with pytest.raises(ValueError):
        ops.gbdt_shap(bins, model, plan, ntree_end=c["T"] + 1)
    with pytest.raises(ValueError):
        ops.gbdt_shap(bins, model, plan, out=torch.empty(63, 13, dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError):
        ops.gbdt_shap(bins, ops.GBDTModel(model.splits, model.leaf_values, model.is_cat, 4, 0.0, c["T"]), plan)
