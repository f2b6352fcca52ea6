"""ObliviousBoostingClassifier end to end on the device: 60 trees on gbdt_ref.make(4096, 1), validated on
make(2048, 2). The fits are made once per module and shared; the oracle replays single trees of the
device's model from the device's own approximants (tests/gbdt_ref.py)."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

TREES = 60
KEEP = (1, 7, 59, 60)      # approximants kept: after t trees (59 = the input of the last tree's replay)


def _fit(gpu, train, **kw):
    num, cat, y = train
    clf = ObliviousBoostingClassifier(iterations=TREES, device=gpu, **kw.pop("ctor", {}))
    return clf.fit((torch.from_numpy(num), torch.from_numpy(cat)), torch.from_numpy(y), **kw)


@pytest.fixture(scope="module")
def sets():
    return G.make(4096, 1), G.make(2048, 2)


@pytest.fixture(scope="module")
def plain(gpu, sets):
    return _fit(gpu, sets[0], record_approximants=KEEP)


@pytest.fixture(scope="module")
def validated(gpu, sets):
    nv, cv, yv = sets[1]
    return _fit(gpu, sets[0], eval_set=((torch.from_numpy(nv), torch.from_numpy(cv)), torch.from_numpy(yv)),
                use_best_model=False)


@pytest.fixture(scope="module")
def stopped(gpu, sets):
    nv, cv, yv = sets[1]
    return _fit(gpu, sets[0], ctor={"early_stopping_rounds": 10},
                eval_set=((torch.from_numpy(nv), torch.from_numpy(cv)), torch.from_numpy(yv)))


def _X(block):
    return torch.from_numpy(block[0]), torch.from_numpy(block[1])


def test_two_fits_give_the_same_model_bit_for_bit(gpu, sets, plain):
    again = _fit(gpu, sets[0])
    assert plain.tree_count_ == again.tree_count_ == TREES
    assert torch.equal(plain.model_.splits, again.model_.splits)
    assert torch.equal(plain.model_.leaf_values, again.model_.leaf_values)
    assert plain.model_.f0 == again.model_.f0 == float(G.base_logit(sets[0][2]))
    assert torch.equal(plain.borders_, again.borders_)


def test_borders_and_bins_match_the_oracle(gpu, sets, plain):
    num, cat, _ = sets[0]
    bins, is_cat, _, borders = G.bin_data(num, cat)
    n = plain.n_borders_.cpu().numpy()
    for j, bj in enumerate(borders):
        assert n[j] == len(bj) and np.array_equal(plain.borders_[j, :n[j]].cpu().numpy(), bj)
    assert np.array_equal(plain._bins(_X(sets[0])).cpu().numpy(), bins)
    assert np.array_equal(plain.model_.is_cat.cpu().numpy(), is_cat)


@pytest.mark.parametrize("t", [1, 7, 60])
def test_prediction_equals_the_training_approximant_bit_for_bit(gpu, sets, plain, t):
    assert torch.equal(plain.predict_logits(_X(sets[0]), ntree_end=t), plain.approximants_[t])


@pytest.mark.parametrize("t", [0, 1, 59])
def test_replay_of_a_tree_from_the_devices_own_approximant(gpu, sets, plain, t):
    """The oracle recomputes g, h, the histograms and the scores of tree t from the device's approximant
    before it, along the device's own splits: every level's split must score at least max (1 - 1e-12) in the
    oracle's fp64, and the leaf values must agree within 2.5e-7 relative (one fp32 rounding). The gradients
    agree bit for bit because both sides round one float64 sigmoid to fp32."""
    num, cat, y = sets[0]
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    before = (np.full(len(y), plain.model_.f0, np.float32) if t == 0
              else plain.approximants_[t].cpu().numpy())
    splits = plain.model_.splits[t].cpu().numpy()
    rep = G.grow_tree(bins, before, y, is_cat, n_bins, 6, plain.learning_rate, plain.l2_leaf_reg, splits=splits)
    for d in range(6):
        print(f"tree {t} level {d}: split {tuple(splits[d])} scores {rep['chosen_score'][d]!r}, max {rep['max_score'][d]!r}")
        assert rep["chosen_score"][d] >= rep["max_score"][d] * (1 - 1e-12)
    got = plain.model_.leaf_values[t].cpu().numpy()
    sums = rep["sums"]
    exact = plain.learning_rate * ((sums[:, 0] / G.SCALE) / (sums[:, 1] / G.SCALE + plain.l2_leaf_reg))
    err = np.abs(got - exact)
    print(f"tree {t}: max relative |leaf value - oracle| {np.max(err / np.maximum(np.abs(exact), 1e-300)):.3e}")
    assert np.all(err <= 2.5e-7 * np.abs(exact))
    assert np.all(got[np.bincount(rep["leaf"], minlength=64) == 0] == 0.0)


def test_replay_with_the_devices_own_gradients_is_within_one_rounding(gpu, sets, plain):
    """The same replay of tree 7 with the gradients the device itself quantised (ops.gbdt_grad): the leaf
    values then agree within 2.5e-7 relative, one fp32 rounding, with no slack, and the sums exactly."""
    num, cat, y = sets[0]
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    before = plain.approximants_[7]
    qg, qh = ops.gbdt_grad(before, torch.from_numpy(y).to(gpu))
    qg, qh = qg.cpu().numpy().astype(np.int64), qh.cpu().numpy().astype(np.int64)
    splits = plain.model_.splits[7].cpu().numpy()
    leaf = np.zeros(len(y), np.int64)
    for d in range(6):
        S = G.scores(G.histogram(bins, leaf, qg, qh, 1 << d), is_cat, n_bins, plain.l2_leaf_reg)
        f, b = (int(v) for v in splits[d])
        assert S[f, b] >= S.max() * (1 - 1e-12)
        assert (f, b) == G.best_split(S)
        leaf = 2 * leaf + G.go_right(bins, f, b, is_cat)
    sums, want = G.leaf_values(leaf, qg, qh, 64, plain.learning_rate, plain.l2_leaf_reg)
    got = plain.model_.leaf_values[7].cpu().numpy()
    exact = plain.learning_rate * ((sums[:, 0] / G.SCALE) / (sums[:, 1] / G.SCALE + plain.l2_leaf_reg))
    assert np.all(np.abs(got - exact) <= 2.5e-7 * np.abs(exact))
    assert np.array_equal(got, want)


def test_learn_logloss_is_strictly_decreasing(validated):
    ll = validated.evals_result_["learn"]["Logloss"]
    assert len(ll) == TREES and validated.tree_count_ == TREES
    print(f"learn Logloss {ll[0]:.4f} -> {ll[-1]:.4f}")
    assert all(b < a for a, b in zip(ll, ll[1:]))


def test_early_stopping_and_the_recorded_metrics(gpu, sets, stopped):
    aucs = stopped.evals_result_["validation"]["AUC"]
    print(f"stopped after {len(aucs)} trees, best_iteration_ {stopped.best_iteration_}, AUC {max(aucs):.5f}")
    assert len(aucs) < TREES                                        # the fit stopped early
    assert stopped.best_iteration_ == int(np.argmax(aucs))           # the first maximum
    assert len(aucs) == stopped.best_iteration_ + 1 + 10
    assert stopped.tree_count_ == stopped.best_iteration_ + 1
    assert stopped.best_score_["validation"]["AUC"] == aucs[stopped.best_iteration_]
    assert len(stopped.evals_result_["learn"]["Logloss"]) == len(aucs) == len(stopped.evals_result_["validation"]["Logloss"])
    Xv, yv = _X(sets[1]), torch.from_numpy(sets[1][2]).to(gpu)
    for i, (auc, ll) in enumerate(zip(aucs, stopped.evals_result_["validation"]["Logloss"])):
        res = ops.binary_eval(stopped.predict_logits(Xv, ntree_end=i + 1), yv).result()
        assert res["auc"] == auc and res["logloss"] == ll, i
    # use_best_model: the default prediction is the best iteration's
    assert torch.equal(stopped.predict_logits(Xv), stopped.predict_logits(Xv, ntree_end=stopped.best_iteration_ + 1))
    proba = stopped.predict_proba(Xv)
    assert proba.shape == (2048, 2) and np.allclose(proba.sum(1), 1.0, atol=1e-6)
    assert abs(G.auc(proba[:, 1], sets[1][2]) - max(aucs)) < 1e-4


def test_the_device_fit_tracks_the_oracle(sets, validated):
    """The oracle's own 60 trees against the device's: the learn Logloss after them within 1e-4 (the models
    agree unless two candidates score within fp64 rounding of each other; the counts are printed)."""
    num, cat, y = sets[0]
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    ref = G.fit(bins, y, is_cat, n_bins, TREES)
    want = G.logloss(ref["approx"][-1], y)
    got = validated.evals_result_["learn"]["Logloss"][-1]
    same = int((validated.model_.splits[:, :, :].cpu().numpy() == ref["splits"]).all(axis=(1, 2)).sum())
    print(f"learn Logloss after {TREES} trees: device {got:.6f}, oracle {want:.6f}; {same} of {TREES} trees split alike")
    assert abs(got - want) < 1e-4


def test_grouped_eval_metric_runs(gpu, sets):
    nv, cv, yv = sets[1]
    groups = np.arange(2048) // 6
    clf = ObliviousBoostingClassifier(iterations=8, device=gpu, metric_period=3)
    clf.fit(_X(sets[0]), sets[0][2], eval_set=(_X(sets[1]), yv), eval_metric="NDCG:top=10", eval_group_id=groups)
    ev = clf.evals_result_["validation"]
    assert len(ev["NDCG"]) == len(ev["QueryAUC"]) == len(ev["AUC"]) == 3          # after trees 3, 6 and 8
    assert all(0.0 < v <= 1.0 for v in ev["NDCG"])
    assert clf.best_iteration_ in (2, 5, 7) and clf.tree_count_ == clf.best_iteration_ + 1
    assert clf.best_score_["validation"]["NDCG"] == max(ev["NDCG"])
    with pytest.raises(ValueError):
        clf.fit(_X(sets[0]), sets[0][2], eval_set=(_X(sets[1]), yv), eval_metric="NDCG")


def test_save_and_load_round_trip(gpu, sets, stopped, tmp_path):
    path = str(tmp_path / "ranker.pt")
    stopped.save_model(path)
    loaded = ObliviousBoostingClassifier(device=gpu).load_model(path)
    Xv = _X(sets[1])
    assert loaded.tree_count_ == stopped.tree_count_ and loaded.best_iteration_ == stopped.best_iteration_
    assert torch.equal(loaded.predict_logits(Xv), stopped.predict_logits(Xv))
    assert np.array_equal(loaded.predict_proba(Xv), stopped.predict_proba(Xv))


def test_columns_by_name_with_a_vocabulary(gpu, tmp_path):
    """Dict input: string categories coded by a host vocabulary, an unseen value predicts as code 0."""
    rng = np.random.default_rng(5)
    R = 600
    colour = rng.choice(["red", "green", "blue"], R)
    x = rng.standard_normal(R).astype(np.float32)
    y = ((colour == "green") ^ (x > 1.0)).astype(np.float32)
    clf = ObliviousBoostingClassifier(iterations=20, depth=3, learning_rate=0.3, cat_features=["colour"], device=gpu)
    clf.fit({"x": x, "colour": colour}, y)
    assert clf.feature_names_ == ["x", "colour"] and clf.vocab_ == [{v: i + 1 for i, v in enumerate(dict.fromkeys(colour))}]
    p = clf.predict_proba({"colour": colour, "x": x})[:, 1]           # looked up by name, not by position
    assert G.auc(p, y) > 0.99
    unseen = clf.predict_logits({"x": x[:4], "colour": np.asarray(["mauve"] * 4)})
    code0 = clf.predict_logits((torch.from_numpy(x[:4, None]), torch.zeros(4, 1, dtype=torch.int64)))
    assert torch.equal(unseen, code0)
    path = str(tmp_path / "named.pt")
    clf.save_model(path)
    again = ObliviousBoostingClassifier(device=gpu).load_model(path)
    assert np.array_equal(again.predict_proba({"x": x, "colour": colour}), clf.predict_proba({"x": x, "colour": colour}))


def test_too_many_categories_raise(gpu):
    y = np.resize(np.asarray([0.0, 1.0], np.float32), 512)
    x = np.zeros((512, 1), np.float32)
    clf = ObliviousBoostingClassifier(iterations=2, device=gpu)
    with pytest.raises(ValueError, match="at most 255"):
        clf.fit((x, np.resize(np.arange(257), 512)[:, None]), y)          # codes 0..256
    with pytest.raises(ValueError, match="at most 255"):
        ObliviousBoostingClassifier(iterations=2, cat_features=["c"], device=gpu).fit(
            {"c": [f"v{i % 256}" for i in range(512)]}, y)                # 256 distinct values
    clf.fit((x, np.resize(np.arange(256), 512)[:, None]), y)                # codes 0..255 fit a uint8 bin
    ObliviousBoostingClassifier(iterations=2, cat_features=["c"], device=gpu).fit(
        {"c": [f"v{i % 255}" for i in range(512)]}, y)
    with pytest.raises(ValueError, match="single class"):
        clf.fit((x, None), np.zeros(512, np.float32))
    with pytest.raises(ValueError, match="0 or 1"):
        clf.fit((x, None), np.full(512, 0.5, np.float32))
