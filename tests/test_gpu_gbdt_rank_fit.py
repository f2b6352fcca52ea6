"""ObliviousBoostingRanker end to end on the device: 60 trees of depth 6 at learning rate 0.05 on the shared
rows of tests/gbdt_rank_ref.py (gbdt_ref.make(4096, 1) in the group layout of seed 7, validated on make(2048,
2) in that of seed 8). The fits are made once per module and shared; the oracle replays single trees from
the device's own approximants and gradients, and its own fit is made once."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier, ObliviousBoostingRanker
from recsys_amd.temp_model.ranker_skelet import RecommendationRanker, ReRankingSystem
from tests import gbdt_rank_ref as Q
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

TREES = 60
KEEP = (1, 7, 59, 60)      # approximants kept: after t trees (7 and 59 = the inputs of the replayed trees)


def _X(block):
    return torch.from_numpy(block[0]), torch.from_numpy(block[1])


def _fit(gpu, train, ctor=None, **kw):
    rk = ObliviousBoostingRanker(iterations=TREES, device=gpu, **(ctor or {}))
    return rk.fit(_X(train), torch.from_numpy(train[2]), torch.from_numpy(train[3]), **kw)


def _eval_kw(val):
    return {"eval_set": (_X(val), torch.from_numpy(val[2])), "eval_group_id": torch.from_numpy(val[3])}


@pytest.fixture(scope="module")
def sets():
    return Q.make_sets()


@pytest.fixture(scope="module")
def grouped(sets):
    """The train rows as the fit sees them: (bins, y, gid) in group order, is_cat, n_bins, the order."""
    num, cat, y, gid = sets[0]
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    order = np.argsort(gid, kind="stable")
    return np.ascontiguousarray(bins[:, order]), y[order], gid[order], is_cat, n_bins, order


@pytest.fixture(scope="module")
def plain(gpu, sets):
    return _fit(gpu, sets[0], record_approximants=KEEP)


@pytest.fixture(scope="module")
def validated(gpu, sets):
    return _fit(gpu, sets[0], use_best_model=False, **_eval_kw(sets[1]))


@pytest.fixture(scope="module")
def stopped(gpu, sets):
    return _fit(gpu, sets[0], ctor={"early_stopping_rounds": 10}, **_eval_kw(sets[1]))


@pytest.fixture(scope="module")
def oracle(sets, grouped):
    bins, y, gid, is_cat, n_bins, _ = grouped
    return Q.fit(bins, y, gid, is_cat, n_bins, TREES)


# ---- determinism and replay ---------------------------------------------------------------------------------
def test_two_fits_give_the_same_model_bit_for_bit(gpu, sets, plain):
    again = _fit(gpu, sets[0])
    assert plain.tree_count_ == again.tree_count_ == TREES and plain.model_.f0 == again.model_.f0 == 0.0
    assert torch.equal(plain.model_.splits, again.model_.splits)
    assert torch.equal(plain.model_.leaf_values, again.model_.leaf_values)


def test_a_fit_on_shuffled_rows_gives_the_same_model_bit_for_bit(gpu, sets, plain):
    perm = np.random.default_rng(12).permutation(len(sets[0][2]))
    shuffled = _fit(gpu, tuple(a[perm] for a in sets[0]))
    assert not np.array_equal(sets[0][3][perm], sets[0][3])
    assert torch.equal(plain.model_.splits, shuffled.model_.splits)
    assert torch.equal(plain.model_.leaf_values, shuffled.model_.leaf_values)


@pytest.mark.parametrize("t", [0, 7, 59])
def test_replay_of_a_tree_with_the_devices_own_gradients(gpu, plain, grouped, t):
    """Tree t again from the device's approximant before it: ops.gbdt_tree(groups=...) rebuilds the model's tree
    bit for bit, and on the device's own quantised gradients the oracle picks the same split at every level,
    sums the same integers into the leaves and rounds the same leaf values."""
    bins, y, gid, is_cat, n_bins, _ = grouped
    plan = plain.group_plan_
    before = torch.zeros(len(y), device=gpu) if t == 0 else plain.approximants_[t].clone()
    yg = torch.from_numpy(y).to(gpu)
    qg, qh = ops.gbdt_grad_query_softmax(before, yg, plan)
    qg, qh = qg.cpu().numpy().astype(np.int64), qh.cpu().numpy().astype(np.int64)
    scratch = ops.GBDTScratch(len(y), bins.shape[0], 6, gpu)
    splits = torch.zeros(6, 2, device=gpu, dtype=torch.int32)
    values = torch.zeros(64, device=gpu, dtype=torch.float32)
    ops.gbdt_tree(torch.from_numpy(bins).to(gpu), yg, before, plain.model_.is_cat, plain.n_bins_, 6, plain.learning_rate,
                  plain.l2_leaf_reg, splits, values, scratch, groups=plan)
    assert torch.equal(splits, plain.model_.splits[t]) and torch.equal(values, plain.model_.leaf_values[t])
    assert np.array_equal(scratch.qg.cpu().numpy(), qg) and np.array_equal(scratch.qh.cpu().numpy(), qh)
    if t + 1 in plain.approximants_:
        assert torch.equal(before, plain.approximants_[t + 1])           # the tree's update of the approximant
    rep = Q.grow_tree(bins, qg, qh, is_cat, n_bins, 6, plain.learning_rate, plain.l2_leaf_reg,
                      splits=splits.cpu().numpy())
    print(f"tree {t}: splits {rep['splits']}, smallest relative gap to the runner-up {min(rep['gap']):.2e}")
    assert rep["splits"] == rep["best"]
    assert np.array_equal(scratch.sums.cpu().numpy(), rep["sums"])
    assert np.array_equal(values.cpu().numpy(), rep["values"])


@pytest.mark.parametrize("t", [1, 7, 60])
def test_prediction_equals_the_training_approximant_bit_for_bit(sets, plain, grouped, t):
    order = torch.from_numpy(grouped[5]).to(plain.device)
    assert torch.equal(plain.group_plan_.order, order)
    assert torch.equal(plain.predict(_X(sets[0]), ntree_end=t)[order], plain.approximants_[t])


# ---- the learn loss -------------------------------------------------------------------------------------------
def test_learn_loss_is_strictly_decreasing_and_tracks_the_oracle(validated, oracle, grouped):
    """The oracle's own 60 trees: its loss falls from 1.832975 (no tree) to 1.380682, by at least 1.7e-3 per tree,
    and its best candidate leads the runner-up by at least 1.6e-5 relative, far above fp64 rounding, so the
    device grows the same trees; the final losses agree within 1e-4."""
    ll = validated.evals_result_["learn"]["QuerySoftMax"]
    assert len(ll) == TREES and validated.tree_count_ == TREES
    start = Q.loss(np.zeros(len(grouped[1]), np.float32), grouped[1], grouped[2])
    same = int((validated.model_.splits.cpu().numpy() == oracle["splits"]).all(axis=(1, 2)).sum())
    print(f"learn QuerySoftMax {start:.6f} -> {ll[0]:.6f} -> {ll[-1]:.6f} (oracle {oracle['loss'][-1]:.6f}); smallest decrease "
          f"{min(a - b for a, b in zip([start] + ll, ll)):.2e}; {same} of {TREES} trees split alike; oracle gap "
          f"{min(oracle['gap']):.2e}")
    assert all(b < a for a, b in zip([start] + ll, ll))
    assert abs(ll[-1] - oracle["loss"][-1]) < 1e-4


# ---- validation -----------------------------------------------------------------------------------------------
def test_recorded_metrics_equal_group_eval_of_the_prediction(gpu, sets, validated):
    val = sets[1]
    ev = validated.evals_result_["validation"]
    assert len(ev["NDCG"]) == len(ev["QueryAUC"]) == len(ev["QuerySoftMax"]) == TREES
    yv, gv = torch.from_numpy(val[2]).to(gpu), torch.from_numpy(val[3]).to(gpu)
    plan = ops.GBDTGroupPlan(gv, gpu)
    for i in range(TREES):
        z = validated.predict(_X(val), ntree_end=i + 1)
        res = ops.group_eval(z, yv, gv, top=10).result()
        assert res["ndcg"] == ev["NDCG"][i] and res["query_auc"] == ev["QueryAUC"][i], i
        if i in (0, 30, TREES - 1):
            loss = ops.query_softmax_eval(z[plan.order].contiguous(), yv[plan.order].contiguous(), plan).result()["loss"]
            assert loss == ev["QuerySoftMax"][i], i
            assert abs(loss - Q.loss(z.cpu().numpy(), val[2], val[3])) <= 1e-9 * loss
    last = validated.predict(_X(val)).cpu().numpy()
    print(f"validation NDCG@10 {ev['NDCG'][0]:.4f} -> {ev['NDCG'][-1]:.4f}, QueryAUC {ev['QueryAUC'][-1]:.4f}")
    assert abs(Q.ndcg(last, val[2], val[3]) - ev["NDCG"][-1]) < 1e-9
    assert ev["NDCG"][-1] > 0.75            # the oracle reaches 0.833, a constant score 0.624 on these rows


def test_early_stopping_and_use_best_model(sets, stopped):
    ndcg = stopped.evals_result_["validation"]["NDCG"]
    print(f"stopped after {len(ndcg)} trees, best_iteration_ {stopped.best_iteration_}, NDCG {max(ndcg):.5f}")
    assert len(ndcg) < TREES
    assert stopped.best_iteration_ == int(np.argmax(ndcg))           # the first maximum
    assert len(ndcg) == stopped.best_iteration_ + 1 + 10
    assert stopped.tree_count_ == stopped.best_iteration_ + 1
    assert stopped.best_score_["validation"]["NDCG"] == ndcg[stopped.best_iteration_]
    assert len(stopped.evals_result_["learn"]["QuerySoftMax"]) == len(ndcg)
    Xv = _X(sets[1])
    assert torch.equal(stopped.predict(Xv), stopped.predict(Xv, ntree_end=stopped.best_iteration_ + 1))


def test_eval_metric_and_metric_period(gpu, sets):
    rk = ObliviousBoostingRanker(iterations=8, device=gpu, metric_period=3)
    rk.fit(_X(sets[0]), sets[0][2], sets[0][3], eval_metric="QuerySoftMax", **_eval_kw(sets[1]))
    ev = rk.evals_result_["validation"]
    assert len(ev["QuerySoftMax"]) == len(ev["NDCG"]) == 3               # after trees 3, 6 and 8
    assert rk.best_iteration_ == 7 and rk.tree_count_ == 8               # the loss still falls
    assert rk.best_score_["validation"]["QuerySoftMax"] == min(ev["QuerySoftMax"])
    rk.fit(_X(sets[0]), sets[0][2], sets[0][3], eval_metric="QueryAUC", **_eval_kw(sets[1]))
    assert rk.best_score_["validation"]["QueryAUC"] == max(rk.evals_result_["validation"]["QueryAUC"])
    for bad in ({"eval_metric": "AUC"}, {"eval_metric": "NDCG:top=0"}, {"eval_group_id": None},
                {"eval_set": None}, {"eval_set": None, "eval_group_id": None, "use_best_model": True}):
        with pytest.raises(ValueError):
            rk.fit(_X(sets[0]), sets[0][2], sets[0][3], **{**_eval_kw(sets[1]), **bad})
    with pytest.raises(ValueError, match="positive"):
        rk.fit(_X(sets[0]), np.zeros(4096, np.float32), sets[0][3])
    with pytest.raises(ValueError, match=">= 0"):
        rk.fit(_X(sets[0]), sets[0][2], sets[0][3] - 6)
    with pytest.raises(ValueError, match="ids for"):
        rk.fit(_X(sets[0]), sets[0][2], sets[0][3][:100])


# ---- persistence and wiring -----------------------------------------------------------------------------------
def test_save_and_load_round_trip(gpu, sets, stopped, tmp_path):
    path = str(tmp_path / "ranker.pt")
    stopped.save_model(path)
    loaded = ObliviousBoostingRanker(device=gpu).load_model(path)
    Xv = _X(sets[1])
    assert loaded.tree_count_ == stopped.tree_count_ and loaded.best_iteration_ == stopped.best_iteration_
    assert loaded.evals_result_ == stopped.evals_result_
    assert torch.equal(loaded.predict(Xv), stopped.predict(Xv))
    with pytest.raises(ValueError, match="QuerySoftMax"):
        ObliviousBoostingClassifier(device=gpu).load_model(path)


def test_a_logloss_file_is_refused_by_the_ranker(gpu, sets, tmp_path):
    clf = ObliviousBoostingClassifier(iterations=3, device=gpu).fit(_X(sets[0]), sets[0][2])
    path = str(tmp_path / "classifier.pt")
    clf.save_model(path)
    with pytest.raises(ValueError, match="Logloss"):
        ObliviousBoostingRanker(device=gpu).load_model(path)
    sd = torch.load(path, weights_only=False)
    assert sd.pop("loss_function") == "Logloss"
    torch.save(sd, path)                                  # a file from before the key existed
    with pytest.raises(ValueError, match="Logloss"):
        ObliviousBoostingRanker(device=gpu).load_model(path)
    old = ObliviousBoostingClassifier(device=gpu).load_model(path)
    assert torch.equal(old.predict_logits(_X(sets[1])), clf.predict_logits(_X(sets[1])))


def test_recommendation_ranker_trains_and_reranks_by_the_raw_score(gpu):
    """RecommendationRanker(backend="native", loss_function="QuerySoftMax") on FeatureEngineer rows with a
    group_id per row (the user), and rerank_batch with it: the final scores are the per-user path's raw scores,
    descending, with no sigmoid."""
    rng = np.random.default_rng(7)
    N, D, K, U0 = 300, 128, 100, 4
    V = rng.integers(-1, 2, (N, D)).astype(np.float32)         # exact in fp32 whatever the order of the sums
    U = rng.integers(-1, 2, (U0 + 30, D)).astype(np.float32)
    cats = ("top", "dress", "shoe")
    items = {i: {"category": cats[rng.integers(3)], "material": "cotton", "fit": "slim",
                 "price": float(rng.integers(4, 400)) / 4} for i in range(N)}
    users = [{"season": "SS", "gender": "F", "avg_price": float(2 ** rng.integers(3, 7))} for _ in range(U0 + 30)]
    rows = []
    for u in range(U0, U0 + 30):
        for i in rng.choice(N, 12, replace=False):
            s = float(U[u] @ V[i])
            z = 0.15 * s + 1.5 * (items[int(i)]["category"] == "dress") - 1.0
            rows.append({"user_meta": users[u], "item_meta": items[int(i)], "two_tower_score": s, "user_vector": U[u],
                         "item_vector": V[int(i)], "label": int(rng.random() < G.sigmoid64(z)), "group_id": u})
    assert RecommendationRanker(backend="native").loss_function == "Logloss"          # the default stays
    with pytest.raises(ValueError):
        RecommendationRanker(backend="native", loss_function="YetiRank")
    ranker = RecommendationRanker(backend="native", loss_function="QuerySoftMax")
    assert isinstance(ranker.model, ObliviousBoostingRanker)
    assert (ranker.model.iterations, ranker.model.learning_rate, ranker.model.depth) == (1000, 0.05, 6)
    ranker.model.iterations = 30
    with pytest.raises(ValueError, match="group_id"):
        ranker.train(rows[:100] + [{k: v for k, v in rows[100].items() if k != "group_id"}])
    ranker.train(rows[:288], rows[288:])
    assert ranker.is_fitted and ranker.model.tree_count_ == ranker.model.best_iteration_ + 1 <= 30
    assert set(ranker.model.evals_result_["validation"]) == {"QuerySoftMax", "NDCG", "QueryAUC"}
    with pytest.raises(TypeError):
        ranker.predict_proba(ranker.engineer.prepare_batch(rows[:4]))

    system = ReRankingSystem(None, None, ranker, items, torch.from_numpy(V).to(gpu))
    cand = np.stack([rng.permutation(N)[:K] for _ in range(U0)])
    score = np.einsum("qd,qkd->qk", U[:U0], V[cand]).astype(np.float32)
    ids, sc, top = system.rerank_batch(torch.from_numpy(cand).to(gpu), torch.from_numpy(score).to(gpu), final_k=K,
                                       user_vectors=torch.from_numpy(U[:U0]).to(gpu), user_meta=users[:U0])
    ops._RERANK_GUARD.check()
    ids, top = ids.cpu().numpy(), top.cpu().numpy()
    for q in range(U0):
        frame = ranker.engineer.prepare_batch([{"user_meta": users[q], "item_meta": items[int(i)], "two_tower_score": float(s),
                                                "user_vector": U[q], "item_vector": V[int(i)]}
                                               for i, s in zip(cand[q], score[q])])
        raw = ranker.predict(frame)
        assert np.array_equal(top[q], np.sort(raw)[::-1]), q
        where = {int(i): k for k, i in enumerate(cand[q])}
        assert np.array_equal(top[q], raw[[where[int(i)] for i in ids[q]]]), q
    assert len(np.unique(top)) > 5 and top.min() < 0 < top.max()         # raw scores, not probabilities
    recs = system.recommend(torch.from_numpy(U[0]).to(gpu), users[0], top_k_retrieval=K, final_k=5)
    assert len(recs) == 5 and [r["final_score"] for r in recs] == sorted((r["final_score"] for r in recs), reverse=True)
