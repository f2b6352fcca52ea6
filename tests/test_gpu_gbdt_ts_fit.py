"""The oblivious-tree models with target-statistic columns end to end on the device: 20 trees on
gbdt_ts_ref.make(4096, 1) (gbdt_ref's columns plus a 1000-value one), validated on make(2048, 2), with
one_hot_max_size=16: the 40-value and the 1000-value columns are TS columns, the other four stay one-hot. The
oracle is tests/gbdt_ts_ref.py feeding tests/gbdt_ref.py. The fits and the oracle's are made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier, ObliviousBoostingRanker
from tests import gbdt_rank_ref as Q
from tests import gbdt_ref as G
from tests import gbdt_ts_ref as TS

pytestmark = pytest.mark.gpu

TREES, OHM = 20, 16


def _X(block):
    return torch.from_numpy(block[0]), torch.from_numpy(block[1])


@pytest.fixture(scope="module")
def sets():
    return TS.make(4096, 1), TS.make(2048, 2)


def _fit(gpu, train, **kw):
    clf = ObliviousBoostingClassifier(iterations=TREES, device=gpu, one_hot_max_size=OHM, **kw)
    return clf.fit(_X(train), torch.from_numpy(train[2]))


@pytest.fixture(scope="module")
def fitted(gpu, sets):
    clf = _fit(gpu, sets[0])
    ops._GBDT_TS_GUARD.check()
    return clf


@pytest.fixture(scope="module")
def oracle(sets):
    num, cat, y = sets[0]
    bins, is_cat, n_bins, state = TS.bin_data(num, cat, y, OHM)
    model = G.fit(bins, y, is_cat, n_bins, TREES)
    bins_v = TS.bin_data(sets[1][0], sets[1][1], None, OHM, fitted=state)[0]
    return {"bins": bins, "is_cat": is_cat, "n_bins": n_bins, "state": state, "model": model, "bins_v": bins_v}


def test_the_fit_needs_the_parameter(gpu, sets, fitted):
    assert fitted.tree_count_ == TREES
    with pytest.raises(ValueError, match="at most 255"):
        ObliviousBoostingClassifier(iterations=2, device=gpu).fit(_X(sets[0]), sets[0][2])
    with pytest.raises(ValueError):
        ObliviousBoostingClassifier(one_hot_max_size=256, device=gpu)
    with pytest.raises(ValueError):
        ObliviousBoostingClassifier(one_hot_max_size=16, ts_prior=(0.5, 0.0), device=gpu)


def test_the_columns_are_numeric_then_ts_then_one_hot(fitted, oracle):
    assert fitted.ts_cols_ == [2, 5] == oracle["state"]["ts_cols"]
    assert fitted._cat_rows(7, 6) == [9, 10, 7, 11, 12, 8]
    assert np.array_equal(fitted.model_.is_cat.cpu().numpy(), [0] * 9 + [1] * 4)      # <= 16 values: still one-hot
    assert np.array_equal(fitted.model_.is_cat.cpu().numpy(), oracle["is_cat"])
    assert np.array_equal(fitted.n_bins_.cpu().numpy(), oracle["n_bins"])


def test_tables_borders_and_byte_tables_equal_the_oracle(fitted, oracle):
    state = oracle["state"]
    n = fitted.ts_n_borders_.cpu().numpy()
    for j in range(2):
        assert np.array_equal(fitted.ts_table_[j].cpu().numpy(), state["tables"][j])
        assert np.array_equal(fitted.ts_totals_[j].cpu().numpy(), state["totals"][j])
        want = state["ts_borders"][j]
        assert n[j] == len(want) and np.array_equal(fitted.ts_borders_[j, :n[j]].cpu().numpy(), want)
        assert fitted.ts_bins_[j].dtype == torch.uint8
        assert np.array_equal(fitted.ts_bins_[j].cpu().numpy(), G.bin_column(state["tables"][j], want))


def test_the_model_is_the_oracles_exactly(fitted, oracle):
    got_s, got_v = fitted.model_.splits[:TREES].cpu().numpy(), fitted.model_.leaf_values[:TREES].cpu().numpy()
    want_s, want_v = oracle["model"]["splits"], oracle["model"]["values"]
    same = [t for t in range(TREES) if np.array_equal(got_s[t], want_s[t])]
    used = sorted(set(got_s[:, :, 0].reshape(-1).tolist()))
    print(f"trees with the oracle's splits: {len(same)} of {TREES}; max |leaf value - oracle| "
          f"{np.abs(got_v - want_v).max():.3e}; split features used {used}")
    assert np.array_equal(got_s, want_s) and np.array_equal(got_v, want_v)
    assert fitted.model_.f0 == float(oracle["model"]["f0"])
    assert 8 in used                                    # the wide TS column splits


def test_validation_scores_equal_the_oracles(sets, fitted, oracle):
    """ops.gbdt_predict's comparison in tests/test_gpu_gbdt_kernels.py: within T 2^-23 bound of the float64 sum
    and equal to the fp32 sum in tree order bit for bit."""
    m = oracle["model"]
    assert np.array_equal(fitted._bins(_X(sets[1])).cpu().numpy(), oracle["bins_v"])
    s64, s32, bound = G.predict(oracle["bins_v"], m["f0"], m["splits"], m["values"], oracle["is_cat"])
    got = fitted.predict_logits(_X(sets[1])).cpu().numpy()
    err = np.abs(got - s64).max()
    print(f"max |device - float64| {err:.2e} (bound {TREES * 2.0 ** -23 * bound:.2e}); AUC {G.auc(got, sets[1][2]):.4f}")
    assert err <= TREES * 2.0 ** -23 * bound
    assert np.array_equal(got, s32)


def test_a_code_outside_the_table_serves_as_code_zero(fitted, sets):
    num, cat, _ = sets[1]
    cat = cat[:64].copy()
    zero = cat.copy()
    cat[:, 5], zero[:, 5] = 1001 + np.arange(64), 0
    cat[::2, 2], zero[::2, 2] = -3, 0
    a = fitted.predict_logits((torch.from_numpy(num[:64]), torch.from_numpy(cat)))
    assert torch.equal(a, fitted.predict_logits((torch.from_numpy(num[:64]), torch.from_numpy(zero))))


def test_two_fits_give_the_same_bits(gpu, sets, fitted):
    again = _fit(gpu, sets[0])
    assert torch.equal(again.model_.splits, fitted.model_.splits)
    assert torch.equal(again.model_.leaf_values, fitted.model_.leaf_values)
    assert all(torch.equal(a, b) for a, b in zip(again.ts_table_ + again.ts_bins_, fitted.ts_table_ + fitted.ts_bins_))
    other = _fit(gpu, sets[0], ts_seed=1)               # another permutation, another model
    assert not torch.equal(other.ts_borders_, fitted.ts_borders_)


def test_save_and_load_round_trip(gpu, sets, fitted, tmp_path):
    path = str(tmp_path / "ts.pt")
    fitted.save_model(path)
    assert torch.load(path, map_location="cpu", weights_only=False)["format"] == "oblivious_gbdt/2"
    loaded = ObliviousBoostingClassifier(device=gpu).load_model(path)
    assert loaded.ts_cols_ == [2, 5] and loaded.one_hot_max_size == OHM and loaded.tree_count_ == TREES
    assert torch.equal(loaded.predict_logits(_X(sets[1])), fitted.predict_logits(_X(sets[1])))
    # without TS columns: format 1 with its keys, as before, and it loads
    num, cat, y = G.make(1024, 1)
    for ohm in (None, 64):
        plain = ObliviousBoostingClassifier(iterations=3, device=gpu, one_hot_max_size=ohm).fit(_X((num, cat)), y)
        assert plain.ts_cols_ == []
        plain.save_model(path)
        sd = torch.load(path, map_location="cpu", weights_only=False)
        assert sd["format"] == "oblivious_gbdt/1" and "ts" not in sd and "one_hot_max_size" not in sd["params"]
        again = ObliviousBoostingClassifier(device=gpu).load_model(path)
        assert torch.equal(again.predict_logits(_X((num, cat))), plain.predict_logits(_X((num, cat))))


def test_columns_by_name_with_a_wide_vocabulary(gpu):
    """Dict input: 300 string values become a TS column, an unseen value serves as code 0."""
    rng = np.random.default_rng(6)
    R = 3000
    eff = rng.standard_normal(300)
    which = rng.integers(0, 300, R)
    which[:300] = np.arange(300)
    y = (rng.random(R) < G.sigmoid64(2.0 * eff[which])).astype(np.float32)
    X = {"x": rng.standard_normal(R).astype(np.float32), "shop": np.asarray([f"s{v}" for v in which])}
    with pytest.raises(ValueError, match="at most 255"):
        ObliviousBoostingClassifier(iterations=2, cat_features=["shop"], device=gpu).fit(X, y)
    clf = ObliviousBoostingClassifier(iterations=20, depth=4, cat_features=["shop"], one_hot_max_size=255, device=gpu).fit(X, y)
    assert clf.ts_cols_ == [0] and len(clf.vocab_[0]) == 300 and clf.ts_bins_[0].numel() == 301
    table = TS.ordered_ts([clf.vocab_[0][v] for v in X["shop"]], y, 300)[2]
    assert np.array_equal(clf.ts_table_[0].cpu().numpy(), table)
    assert G.auc(clf.predict_logits(X).cpu().numpy(), y) > 0.7
    unseen = clf.predict_logits({"x": X["x"][:4], "shop": np.asarray(["nowhere"] * 4)})
    code0 = clf.predict_logits((torch.from_numpy(X["x"][:4, None]), torch.zeros(4, 1, dtype=torch.int64)))
    assert torch.equal(unseen, code0)


def test_the_ranker_with_group_ids(gpu, sets, tmp_path):
    """ObliviousBoostingRanker: the statistics on the caller's row order, then the rows permuted into group order.
    The oracle: the same bins permuted, gbdt_rank_ref's fit."""
    (num, cat, y), (nv, cv, yv) = sets
    rng = np.random.default_rng(8)
    gid, gv = rng.integers(0, 500, len(y)), np.arange(len(yv)) // 8
    rk = ObliviousBoostingRanker(iterations=TREES, device=gpu, one_hot_max_size=OHM)
    with pytest.raises(ValueError, match="at most 255"):
        ObliviousBoostingRanker(iterations=2, device=gpu).fit(_X(sets[0]), y, gid)
    rk.fit(_X(sets[0]), y, gid, eval_set=(_X(sets[1]), yv), eval_group_id=gv, use_best_model=False)
    ops._GBDT_TS_GUARD.check()
    assert rk.ts_cols_ == [2, 5] and rk.tree_count_ == TREES
    bins, is_cat, n_bins, state = TS.bin_data(num, cat, y, OHM)
    for j in range(2):
        assert np.array_equal(rk.ts_table_[j].cpu().numpy(), state["tables"][j])
    order = rk.group_plan_.order.cpu().numpy()
    assert np.array_equal(rk._bins(_X(sets[1])).cpu().numpy(), TS.bin_data(nv, cv, None, OHM, fitted=state)[0])
    again = ObliviousBoostingRanker(iterations=TREES, device=gpu, one_hot_max_size=OHM).fit(_X(sets[0]), y, gid)
    assert torch.equal(again.model_.splits, rk.model_.splits) and torch.equal(again.model_.leaf_values, rk.model_.leaf_values)
    ref = Q.fit(bins[:, order], y[order], gid[order], is_cat, n_bins, TREES)
    got_s = rk.model_.splits[:TREES].cpu().numpy()
    same = [t for t in range(TREES) if np.array_equal(got_s[t], ref["splits"][t])]
    print(f"ranker trees with the oracle's splits: {len(same)} of {TREES}")
    assert np.array_equal(got_s, np.asarray(ref["splits"]))
    assert np.array_equal(rk.model_.leaf_values[:TREES].cpu().numpy(), np.asarray(ref["values"]))
    path = str(tmp_path / "rk.pt")
    rk.save_model(path)
    assert torch.load(path, map_location="cpu", weights_only=False)["format"] == "oblivious_gbdt/2"
    loaded = ObliviousBoostingRanker(device=gpu).load_model(path)
    assert torch.equal(loaded.predict(_X(sets[1])), rk.predict(_X(sets[1])))
    assert len(rk.evals_result_["validation"]["NDCG"]) == TREES
