"""The explanation oracle (tests/gbdt_explain_ref.py) against itself: the table-based Shapley values equal a
table-free brute force (the recursion run once per coalition), on random trees of depth 1-4, with repeated
features (down to one feature on every level) and with zero-cover subtrees; additivity, absent features,
symmetry and a hand-computed PredictionValuesChange. No GPU."""
import itertools

import numpy as np
import pytest

from tests import gbdt_explain_ref as E

F = 5


def _tree(rng, depth, feats=None, zero=None):
    """(splits [depth, 2], values [2^depth], w [2^depth]); zero: leaves whose weight is 0."""
    f = rng.integers(0, F, depth) if feats is None else np.asarray(feats)
    splits = np.stack([f, rng.integers(0, 3, depth)], axis=1)
    values = rng.standard_normal(1 << depth)
    w = rng.integers(1, 50, 1 << depth)
    if zero is not None:
        w[zero] = 0
    return splits, values, w


def _all_bits(depth):
    return np.array(list(itertools.product((0, 1), repeat=depth)), np.int64).T      # [depth, 2^depth]


CASES = []
for _depth in (1, 2, 3, 4):
    CASES.append((f"random-d{_depth}", _depth, None, None))
    CASES.append((f"one-feature-d{_depth}", _depth, [2] * _depth, None))
    CASES.append((f"zero-right-half-d{_depth}", _depth, None, slice(1 << (_depth - 1), None)))
CASES += [("repeat-d3", 3, [1, 3, 1], None), ("repeat-d4", 4, [0, 4, 4, 0], None),
          ("repeat-zero-d4", 4, [0, 1, 0, 1], slice(4, 8)), ("all-zero-d3", 3, None, slice(None)),
          ("zero-quarter-d4", 4, [3, 2, 1, 0], slice(0, 4))]


@pytest.mark.parametrize("name,depth,feats,zero", CASES, ids=[c[0] for c in CASES])
def test_table_equals_brute_force_and_is_additive(name, depth, feats, zero):
    rng = np.random.default_rng(len(name) * 31 + depth)
    splits, values, w = _tree(rng, depth, feats, zero)
    r = _all_bits(depth)                       # every leaf once
    phi = E.tree_shap(splits, values, w, r, F)
    brute = E.tree_shap_brute(splits, values, w, r, F)
    assert np.abs(phi - brute).max() <= 1e-15 * max(1.0, np.abs(values).max())
    table = E.cond_table(values, w, depth)
    assert table.shape == (3 ** depth,)
    for state in itertools.product((0, 1, 2), repeat=depth):
        idx = sum(s * 3 ** (depth - 1 - d) for d, s in enumerate(state))
        assert abs(table[idx] - E.cond_value(values, w, depth, state)) <= 1e-15 * np.abs(values).max()
    leaf = (r * (1 << np.arange(depth - 1, -1, -1))[:, None]).sum(0)
    err = np.abs(phi.sum(0) + table[-1] - values[leaf]).max()
    assert err <= 2e-15 * max(1.0, np.abs(values).max()), err       # sum phi + E(*...*) = value[leaf]
    absent = [j for j in range(F) if j not in E.players(splits)]
    assert absent and not phi[absent].any()    # exactly 0


def test_exchanged_columns_get_exchanged_values():
    rng = np.random.default_rng(5)
    splits, values, w = _tree(rng, 4, [0, 3, 1, 3])
    r = _all_bits(4)
    phi = E.tree_shap(splits, values, w, r, F)
    swapped = splits.copy()
    swapped[:, 0] = [{0: 3, 3: 0}.get(int(f), int(f)) for f in splits[:, 0]]
    phi2 = E.tree_shap(swapped, values, w, r, F)
    assert np.array_equal(phi2[[3, 1, 2, 0, 4]], phi)


def test_two_symmetric_players_share_equally():
    # value = a AND b, uniform weights: both features get the same phi on every row
    splits = np.array([[0, 0], [1, 0]])
    values, w = np.array([0.0, 0.0, 0.0, 1.0]), np.array([5, 5, 5, 5])
    phi = E.tree_shap(splits, values, w, _all_bits(2), F)
    assert np.array_equal(phi[0, [0, 3]], phi[1, [0, 3]])
    assert np.allclose(phi[:2, 3], [0.375, 0.375]) and np.isclose(E.cond_table(values, w, 2)[-1], 0.25)


def test_prediction_values_change_of_a_hand_computed_tree():
    # depth 2, level 0 on feature 1, level 1 on feature 3; leaves (r0 r1) = 00, 01, 10, 11
    splits = np.array([[[1, 0], [3, 0]]])
    values = np.array([[1.0, 3.0, 2.0, 6.0]])
    w = np.array([[2, 2, 1, 3]])
    # level 0 pairs (00, 10), (01, 11): 2*1/3 * 1 + 2*3/5 * 9; level 1 pairs (00, 01), (10, 11): 2*2/4 * 4 + 1*3/4 * 16
    lvl0, lvl1 = 2 / 3 + 54 / 5, 4.0 + 12.0
    assert np.allclose(E.level_pvc(values[0], w[0], 2), [lvl0, lvl1], rtol=1e-15)
    imp = E.prediction_values_change(splits, values, w, F)
    want = np.zeros(F)
    want[1], want[3] = lvl0, lvl1
    assert np.allclose(imp, want * 100 / (lvl0 + lvl1), rtol=1e-14) and abs(imp.sum() - 100) < 1e-12
    assert not E.prediction_values_change(splits, values, np.zeros((1, 4), np.int64), F).any()
    # an empty pair adds nothing
    assert np.allclose(E.level_pvc(values[0], np.array([2, 0, 0, 3]), 2), [0.0, 0.0])


def test_leaf_weights_and_model_shap_on_binned_rows():
    from tests import gbdt_ref as G
    num, cat, _ = G.make(500, 3)
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    rng = np.random.default_rng(8)
    T, depth = 5, 3
    f = rng.integers(0, 12, (T, depth))
    f[1] = 4                                    # one feature on every level
    f[2, 0] = 40                                # out of range: reads as feature 0
    b = (rng.random((T, depth)) * (n_bins[np.minimum(f, 11)] - 1)).astype(np.int64)
    splits = np.stack([f, b], axis=2)
    values = (rng.standard_normal((T, 64)) * 0.1).astype(np.float32)
    clamped = E.clamp_features(splits, 12)
    w = E.leaf_weights(bins, clamped, is_cat)
    assert w.shape == (T, 64) and (w.sum(1) == 500).all() and not w[:, 8:].any()
    phi = E.shap(bins, -0.75, splits, values, is_cat, w)
    s64, _, bound = G.predict(bins, np.float32(-0.75), clamped, values, is_cat)
    assert np.abs(phi.sum(0) - s64).max() <= 1e-14 * bound
    # the expected value is the weighted mean of the leaves when the weights are the rows' own
    mean = -0.75 + sum(float((values[t, :8].astype(np.float64) * w[t, :8]).sum() / 500) for t in range(T))
    assert abs(phi[12, 0] - mean) <= 1e-14 * bound and (phi[12] == phi[12, 0]).all()


def test_native_entry_points_reject_bad_arguments_without_a_gpu():
    import os

    from recsys_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.load()
    p, err = 16, lib.rsx_last_error
    assert lib.rsx_gbdt_shap_tree_chunk() >= 1
    weights = lambda R, F, depth, t0, t1, b=p, w=p: lib.rsx_gbdt_leaf_weights(b, R, F, p, p, depth, t0, t1, w, None)   # noqa: E731
    shap = lambda R, F, depth, t0, t1, tb=p, out=p: lib.rsx_gbdt_shap(p, R, F, p, p, depth, t0, t1, tb, 0.0, out, None)  # noqa: E731
    for fn in (weights, shap):
        assert fn(0, 12, 6, 0, 1) == 1 and b"R < 2^31" in err()
        assert fn(1 << 31, 12, 6, 0, 1) == 1 and b"R < 2^31" in err()
        assert fn(10, 0, 6, 0, 1) == 1 and b"F <= 32" in err()
        assert fn(10, 33, 6, 0, 1) == 1 and b"F <= 32" in err()
        assert fn(10, 12, 0, 0, 1) == 1 and b"depth" in err()
        assert fn(10, 12, 7, 0, 1) == 1 and b"depth" in err()
        assert fn(10, 12, 6, 2, 1) == 1 and b"tree_begin" in err()
        assert fn(10, 12, 6, -1, 1) == 1 and b"tree_begin" in err()
        assert fn(10, 12, 6, 0, 1, None) == 1 and b"null tensor" in err()
    assert weights(10, 12, 6, 0, 1, p, None) == 1 and b"null tensor" in err()
    assert shap(10, 12, 6, 0, 1, p, None) == 1 and b"null tensor" in err()
    plan = lambda depth, t0, t1, lv=p, tb=p: lib.rsx_gbdt_explain_plan(p, lv, p, depth, t0, t1, tb, p, None)     # noqa: E731
    assert plan(0, 0, 1) == 1 and b"depth" in err()
    assert plan(7, 0, 1) == 1 and b"depth" in err()
    assert plan(6, 3, 1) == 1 and b"tree_begin" in err()
    assert plan(6, 0, 1, None) == 1 and b"null tensor" in err()
    assert plan(6, 0, 1, p, None) == 1 and b"null tensor" in err()
    assert plan(6, 2, 2, None, None) == 0       # an empty range touches nothing
