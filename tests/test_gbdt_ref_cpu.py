"""CPU checks of the oblivious-tree boosting oracle (tests/gbdt_ref.py) and of the host-side pieces of
the model: borders and bins against brute force, the oracle's scores against a direct evaluation of every
partition, the tie rule, the native argument checks, and the end-to-end preconditions the GPU tests of the
fit rely on, asserted on the oracle itself."""
import os

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native
from recsys_amd.temp_model import oblivious_gbdt as OG
from tests import gbdt_ref as G


def _brute_borders(x, border_count=254):
    vals = sorted(set(float(v) for v in x if not np.isnan(v)))
    mids = [np.float32(np.float32(a) * np.float32(0.5) + np.float32(b) * np.float32(0.5)) for a, b in zip(vals, vals[1:])]
    if len(mids) <= border_count:
        return np.asarray(mids, np.float32)
    return np.asarray([mids[((2 * j + 1) * len(mids)) // (2 * border_count)] for j in range(border_count)], np.float32)


def _columns():
    rng = np.random.default_rng(0)
    many = rng.standard_normal(3000).astype(np.float32)
    with_nan = many.copy()
    with_nan[::7] = np.nan
    return {
        "many distinct": many,
        "with NaN": with_nan,
        "repeated": np.round(rng.standard_normal(3000) * 2).astype(np.float32) / 2,
        "255 distinct": np.resize(np.arange(255, dtype=np.float32) * 0.37, 3000),
        "256 distinct": np.resize(np.arange(256, dtype=np.float32) * 0.37, 3000),
        "257 distinct": np.resize(np.arange(257, dtype=np.float32) * 0.37, 3000),
        "one value": np.full(3000, 2.5, np.float32),
        "two values": np.resize(np.asarray([1.0, -1.0], np.float32), 3000),
        "all NaN": np.full(3000, np.nan, np.float32),
        "signed zeros": np.resize(np.asarray([0.0, -0.0, 1.0], np.float32), 3000),
    }


@pytest.mark.parametrize("border_count", [254, 16])
def test_borders_match_brute_force(border_count):
    cols = _columns()
    x = torch.from_numpy(np.stack(list(cols.values())))
    borders, n_borders = OG.build_borders(x, border_count)
    assert borders.shape == (len(cols), 256) and n_borders.dtype == torch.int32
    for k, (name, col) in enumerate(cols.items()):
        want = _brute_borders(col, border_count)
        assert np.array_equal(G.build_borders(col, border_count), want), name
        n = int(n_borders[k])
        assert n == len(want) <= border_count, name
        assert np.array_equal(borders[k, :n].numpy(), want), name
        assert torch.isinf(borders[k, n:]).all() and (borders[k, n:] > 0).all(), name
        assert np.all(np.diff(want) >= 0), name


def test_border_counts_at_the_threshold():
    cols = _columns()
    assert len(G.build_borders(cols["255 distinct"])) == 254      # every midpoint
    assert len(G.build_borders(cols["256 distinct"])) == 254      # 254 of 255
    assert len(G.build_borders(cols["one value"])) == 0 and len(G.build_borders(cols["all NaN"])) == 0
    assert np.array_equal(G.build_borders(cols["two values"]), np.asarray([0.0], np.float32))


def test_bins_match_brute_force():
    for name, col in _columns().items():
        borders = G.build_borders(col)
        probe = np.concatenate([col[:500], borders, np.asarray([np.nan, -np.inf, np.inf, -1e30, 1e30], np.float32)])
        want = np.asarray([0 if np.isnan(v) else int(np.sum(borders < v)) for v in probe])
        got = G.bin_column(probe, borders)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert want.max(initial=0) <= 254


def _direct_score(bins, leaf, qg, qh, n_leaves, f, b, cat, l2):
    total = 0.0
    for l in range(n_leaves):
        rows = leaf == l
        right = rows & ((bins[f] == b) if cat else (bins[f] > b))
        left = rows & ~right
        for side in (left, right):
            g = int(qg[side].sum()) / G.SCALE
            h = int(qh[side].sum()) / G.SCALE
            total += g * g / (h + l2)
    return total


def test_scores_match_a_direct_evaluation_of_every_partition():
    rng = np.random.default_rng(3)
    R, l2 = 64, 3.0
    bins = np.stack([rng.integers(0, 9, R), rng.integers(0, 255, R), rng.integers(0, 5, R)]).astype(np.uint8)
    bins[1, 0] = 255
    is_cat, n_bins = np.asarray([0, 0, 1], np.uint8), np.asarray([9, 256, 5], np.int32)
    qg, qh = G.grad(rng.standard_normal(R).astype(np.float32) * 3, (rng.random(R) < 0.3).astype(np.float32))
    for n_leaves in (1, 4):
        leaf = rng.integers(0, n_leaves, R)
        S = G.scores(G.histogram(bins, leaf, qg, qh, n_leaves), is_cat, n_bins, l2)
        parent = sum((int(qg[leaf == l].sum()) / G.SCALE) ** 2 / (int(qh[leaf == l].sum()) / G.SCALE + l2)
                     for l in range(n_leaves))
        for f in range(3):
            assert np.all(np.isneginf(S[f, n_bins[f]:]))
            for b in range(n_bins[f]):
                want = _direct_score(bins, leaf, qg, qh, n_leaves, f, b, bool(is_cat[f]), l2)
                assert abs(S[f, b] - want) <= 1e-13 * abs(want), (f, b)
        # An empty right side scores the parent term. (A real split can score below it: each side pays l2 in
        # its denominator. The argmax then keeps the empty split and the level leaves the leaves as they are.)
        assert abs(S[0, 8] - parent) <= 1e-13 * parent


def test_ties_go_to_the_lowest_feature_then_the_lowest_bin():
    rng = np.random.default_rng(4)
    R = 200
    col = rng.integers(0, 6, R).astype(np.uint8)
    gapped = col * 2                                              # bins 1, 3, ... empty: b and b + 1 tie
    bins = np.stack([gapped, rng.integers(0, 3, R).astype(np.uint8), gapped])
    is_cat, n_bins = np.zeros(3, np.uint8), np.asarray([12, 3, 12], np.int32)
    y = (col >= 3).astype(np.float32)
    qg, qh = G.grad(np.zeros(R, np.float32), y)
    S = G.scores(G.histogram(bins, np.zeros(R, np.int64), qg, qh, 1), is_cat, n_bins, 3.0)
    assert np.array_equal(S[0], S[2]) and S[0, 4] == S[0, 5] == S.max()
    assert G.best_split(S) == (0, 4)
    one = G.scores(G.histogram(bins[:, :1], np.zeros(1, np.int64), qg[:1], qh[:1], 1), is_cat, n_bins, 3.0)
    assert G.best_split(one) == (0, 0)                            # every candidate scores the parent


def test_native_entry_points_reject_bad_arguments_without_a_gpu():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.load()
    p = 16
    assert lib.rsx_gbdt_histogram(p, p, p, p, 100, 12, 3, p, p, None) == 1 and b"n_leaves" in lib.rsx_last_error()
    assert lib.rsx_gbdt_histogram(p, p, p, p, 100, 33, 4, p, p, None) == 1 and b"F <= 32" in lib.rsx_last_error()
    assert lib.rsx_gbdt_histogram(p, p, p, p, 1 << 31, 12, 4, p, p, None) == 1 and b"R < 2^31" in lib.rsx_last_error()
    assert lib.rsx_gbdt_best_split(p, p, p, 12, 4, 0.0, p, p, None, None) == 1 and b"l2" in lib.rsx_last_error()
    assert lib.rsx_gbdt_predict(p, 10, 12, p, p, p, 7, 0, 1, None, 0.0, p, None) == 1 and b"depth" in lib.rsx_last_error()
    assert lib.rsx_gbdt_predict(p, 10, 12, p, p, p, 6, 2, 1, None, 0.0, p, None) == 1
    assert lib.rsx_gbdt_grad(None, p, 10, p, p, None) == 1 and b"null tensor" in lib.rsx_last_error()
    assert lib.rsx_rerank_tabular(p, p, p, p, p, p, 0, 5, 10, 8, p, p, p, None) == 1
    assert lib.rsx_gbdt_tree_chunk() == 64
    assert lib.rsx_gbdt_histogram_slabs(70001, 12) > 1 and lib.rsx_gbdt_histogram_slabs(1000, 12) == 1


@pytest.fixture(scope="module")
def oracle_fit():
    num, cat, y = G.make(4096, 1)
    nv, cv, yv = G.make(2048, 2)
    bins, is_cat, n_bins, borders = G.bin_data(num, cat)
    bins_v = G.bin_data(nv, cv, borders)[0]
    model = G.fit(bins, y, is_cat, n_bins, 60)
    Fv = np.full(len(yv), model["f0"], np.float32)
    aucs = []
    for t in range(60):
        Fv = Fv + model["values"][t][G.tree_leaves(bins_v, model["splits"][t], is_cat)]
        aucs.append(G.auc(Fv, yv))
    return {"model": model, "y": y, "aucs": aucs, "bins": bins, "is_cat": is_cat}


def test_data_generator_shapes():
    num, cat, y = G.make(1000, 5)
    assert num.dtype == np.float32 and num.shape == (1000, 7) and cat.shape == (1000, 5) and y.shape == (1000,)
    assert np.array_equal(num[:, 6], num[:, 0]) and np.array_equal(num[:, 3] * 2, np.round(num[:, 3] * 2))
    assert len(np.unique(num[:, 3])) < 30 and [int(cat[:, j].max()) + 1 for j in range(5)] == list(G.CARDS)
    assert set(np.unique(y)) == {0.0, 1.0}


def test_learn_logloss_falls_every_tree(oracle_fit):
    ll = [G.logloss(a, oracle_fit["y"]) for a in oracle_fit["model"]["approx"]]
    assert all(b < a for a, b in zip(ll, ll[1:]))
    print(f"learn Logloss {ll[0]:.4f} -> {ll[-1]:.4f}")


def test_early_stopping_after_ten_rounds_stops_well_before_sixty(oracle_fit):
    aucs = oracle_fit["aucs"]
    best, since, stop = None, 0, None
    for i, a in enumerate(aucs):
        if best is None or a > aucs[best]:
            best, since = i, 0
        else:
            since += 1
            if since >= 10:
                stop = i
                break
    assert stop is not None and stop <= 40, (stop, best)
    margin = aucs[best] - max(aucs[best + 1:stop + 1])
    assert margin > 1e-4          # hundreds of pair flips of the 2048 validation rows
    print(f"validation AUC peaks at tree {best} ({aucs[best]:.5f}), the fit stops after tree {stop}, margin {margin:.2e}")


def test_best_candidates_are_well_separated_and_the_copy_ties(oracle_fit):
    """The replay on the device follows the device's own splits and scores them with the oracle's fp64: what
    it needs is that float32 rounding of a gradient (relative 1e-7 on a score at the very most) does not
    reorder the two best distinct scores. The duplicated column makes the exact ties."""
    model = oracle_fit["model"]
    assert min(model["gap"]) > 1e-7, min(model["gap"])
    assert not np.any(model["splits"][:, :, 0] == 6)        # column 6 copies column 0: the lower index wins
    assert np.any(model["splits"][:, :, 0] == 0) and np.any(model["splits"][:, :, 0] >= 7)
    print(f"smallest relative gap between the two best distinct scores: {min(model['gap']):.2e}")
