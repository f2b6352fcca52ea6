"""The batched tabular rerank path: ops.rerank_tabular (rsx_rerank_tabular) against float64 numpy, the bins
of its columns against np.searchsorted, and ReRankingSystem.rerank_batch with the native tree ranker against
the per-user path (FeatureEngineer rows on the host -> predict_proba). Q = 5 queries, K = 100 candidates,
300 items, d = 128."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.ranker_skelet import RecommendationRanker, ReRankingSystem
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

Q, K, N, D = 5, 100, 300, 128
CATEGORY, MATERIAL, FIT = ("top", "dress", "shoe", "bag"), ("cotton", "wool", "linen"), ("slim", "regular")
SEASON, GENDER = ("SS", "FW"), ("F", "M", "U")


def _norm(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_features_against_float64(gpu):
    rng = np.random.default_rng(0)
    U, V = _norm(rng.standard_normal((Q, D))).astype(np.float32), _norm(rng.standard_normal((N, D))).astype(np.float32)
    price = (rng.random(N) * 90 + 5).astype(np.float32)
    avg = np.asarray([30.0, 0.0, 55.5, 12.25, 80.0], np.float32)
    cand = rng.integers(0, N, (Q, K))
    score = rng.standard_normal((Q, K)).astype(np.float32)
    feats, ids = ops.rerank_tabular(*(torch.from_numpy(a).to(gpu) for a in (cand, score, U, V, price, avg)))
    ops._RERANK_GUARD.check()
    assert feats.shape == (7, Q * K) and ops.RERANK_TABULAR_COLUMNS[4:] == ("item_price", "user_avg_price", "price_diff_ratio")
    f = feats.cpu().numpy().reshape(7, Q, K)
    assert np.array_equal(ids.cpu().numpy(), cand.reshape(-1))
    prod = U.astype(np.float64)[:, None, :] * V.astype(np.float64)[cand]          # [Q, K, D]
    tol = 128 * 2.0 ** -23 * np.abs(prod).max()
    errs = [np.abs(f[1] - prod.mean(-1)).max(), np.abs(f[2] - prod.max(-1)).max(), np.abs(f[3] - prod.std(-1)).max()]
    print(f"max error of mean / max / std: {errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e} (bound {tol:.2e})")
    assert max(errs) <= tol
    assert np.array_equal(f[0], score)
    assert np.array_equal(f[4], price[cand]) and np.array_equal(f[5], np.broadcast_to(avg[:, None], (Q, K)))   # exact
    a64, p64 = avg.astype(np.float64)[:, None], price.astype(np.float64)[cand]
    ratio = np.where(a64 > 0, (p64 - a64) / np.where(a64 > 0, a64, 1.0), 0.0)
    assert np.all(np.abs(f[6] - ratio) <= 2.0 ** -22 * np.abs(ratio))              # two fp32 roundings
    assert np.all(f[6, 1] == 0.0)                                                  # avg_price 0 gives ratio 0


def test_an_item_id_out_of_range_reads_item_zero_and_is_reported(gpu):
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((2, 16)).astype(np.float32), rng.standard_normal((10, 16)).astype(np.float32)
    cand = np.asarray([[0, 10, 3], [9, -1, 2]])
    t = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    ops._RERANK_GUARD.check()
    feats, ids = ops.rerank_tabular(t(cand), t(np.zeros((2, 3), np.float32)), t(U), t(V), t(np.arange(10, dtype=np.float32)),
                                    t(np.ones(2, np.float32)))
    assert ids.cpu().tolist() == [0, 0, 3, 9, 0, 2]
    assert feats[4].cpu().tolist() == [0.0, 0.0, 3.0, 9.0, 0.0, 2.0]
    with pytest.raises(IndexError):
        ops._RERANK_GUARD.check()


@pytest.fixture(scope="module")
def world(gpu):
    """Item and user vectors with entries in {-1, 0, 1} and prices on a dyadic grid, so that every
    FeatureEngineer column is exact in fp32 whatever the order of its sums: the host's float32 numpy and
    the kernel then see the same values, and a row falls into the same bins on both paths."""
    rng = np.random.default_rng(7)
    V = rng.integers(-1, 2, (N, D)).astype(np.float32)
    U = rng.integers(-1, 2, (Q + 40, D)).astype(np.float32)
    items = {i: {"category": CATEGORY[rng.integers(4)], "material": MATERIAL[rng.integers(3)], "fit": FIT[rng.integers(2)],
                 "price": float(rng.integers(4, 400)) / 4} for i in range(N)}
    del items[17]["material"]                       # a missing key reads "unknown"
    del items[23]                                   # an item without metadata
    users = [{"season": SEASON[rng.integers(2)], "gender": GENDER[rng.integers(3)],
              "avg_price": float(2 ** rng.integers(3, 7))} for _ in range(Q + 40)]
    users[1]["avg_price"] = 0.0
    users[2] = {"season": "AW"}                     # an unseen season, nothing else
    rows = []
    for _ in range(1500):
        u, i = int(rng.integers(Q, Q + 40)), int(rng.integers(N))
        meta = items.get(i, {})
        s = float(U[u] @ V[i])
        z = 0.15 * s + 1.0 * (meta.get("category") == "dress") - 0.02 * (meta.get("price", 0) - users[u].get("avg_price", 0.0))
        rows.append({"user_meta": users[u], "item_meta": meta, "two_tower_score": s, "user_vector": U[u],
                     "item_vector": V[i], "label": int(rng.random() < G.sigmoid64(z - 0.5))})
    ranker = RecommendationRanker(backend="native")
    ranker.model.iterations = 50
    ranker.train(rows[:1200], rows[1200:])
    system = ReRankingSystem(None, None, ranker, items, torch.from_numpy(V).to(gpu))
    return {"system": system, "ranker": ranker, "U": U, "V": V, "items": items, "users": users}


def test_the_native_ranker_has_the_references_hyper_parameters(gpu, world):
    try:
        import catboost  # noqa: F401
        have_catboost = True
    except ImportError:
        have_catboost = False
    assert RecommendationRanker(backend="auto").backend == ("catboost" if have_catboost else "native")
    if not have_catboost:
        with pytest.raises(ImportError):
            RecommendationRanker(backend="catboost")
    fresh = RecommendationRanker(backend="native")
    m = fresh.model
    assert not fresh.is_fitted
    assert (m.iterations, m.learning_rate, m.depth, m.early_stopping_rounds) == (1000, 0.05, 6, 50)
    with pytest.raises(ValueError):
        RecommendationRanker(backend="xgboost")
    r = world["ranker"]
    assert r.is_fitted and r.model.tree_count_ == r.model.best_iteration_ + 1 <= 50
    assert r.model.feature_names_ == ["two_tower_score", "vec_prod_mean", "vec_prod_max", "vec_prod_std", "user_avg_price",
                                      "item_price", "price_diff_ratio", "season", "gender", "item_category",
                                      "item_material", "item_fit"]


def test_bins_match_searchsorted_on_the_devices_own_features(gpu, world):
    rng = np.random.default_rng(3)
    clf = world["ranker"].model
    cand = torch.from_numpy(rng.integers(0, N, (Q, K))).to(gpu)
    score = torch.from_numpy(rng.standard_normal((Q, K)).astype(np.float32)).to(gpu)
    tab = world["system"]._tabular_tables(clf)
    avg = torch.tensor([16.0, 0.0, 8.0, 64.0, 32.0], device=gpu)
    feats, _ = ops.rerank_tabular(cand, score, torch.from_numpy(world["U"][:Q]).to(gpu), world["system"].item_vectors,
                                  tab["price"], avg)
    x = feats.index_select(0, tab["rows"]) if tab["rows"] is not None else feats
    bins = ops.gbdt_bin(x, clf.borders_, clf.n_borders_).cpu().numpy()
    n = clf.n_borders_.cpu().numpy()
    for j in range(7):
        borders = clf.borders_[j, :n[j]].cpu().numpy()
        assert np.array_equal(bins[j], np.searchsorted(borders, x[j].cpu().numpy(), side="left")), clf.feature_names_[j]
    assert n.max() > 10


def test_rerank_batch_equals_the_per_user_path(gpu, world):
    system, ranker = world["system"], world["ranker"]
    rng = np.random.default_rng(9)
    U, metas = world["U"][:Q], world["users"][:Q]
    cand = np.stack([rng.permutation(N)[:K] for _ in range(Q)])
    score = np.einsum("qd,qkd->qk", U, world["V"][cand]).astype(np.float32)
    ids, sc, top_p = system.rerank_batch(torch.from_numpy(cand).to(gpu), torch.from_numpy(score).to(gpu), final_k=10,
                                         user_vectors=torch.from_numpy(U).to(gpu), user_meta=metas)
    ops._RERANK_GUARD.check()
    ids, sc, top_p = ids.cpu().numpy(), sc.cpu().numpy(), top_p.cpu().numpy()
    for q in range(Q):
        rows = [{"user_meta": metas[q], "item_meta": world["items"].get(int(i), {}), "two_tower_score": float(s),
                 "user_vector": U[q], "item_vector": world["V"][int(i)]} for i, s in zip(cand[q], score[q])]
        probs = ranker.predict_proba(ranker.engineer.prepare_batch(rows))          # the per-user path's scores
        assert np.array_equal(top_p[q], np.sort(probs)[::-1][:10]), q
        where = {int(i): k for k, i in enumerate(cand[q])}
        assert np.array_equal(top_p[q], probs[[where[int(i)] for i in ids[q]]]), q
        assert np.array_equal(sc[q], score[q][[where[int(i)] for i in ids[q]]]), q
    assert len(np.unique(top_p)) > 5


def test_recommend_and_recommend_batch_run_with_the_native_ranker(gpu, world):
    system = world["system"]
    U, metas = torch.from_numpy(world["U"][:Q]).to(gpu), world["users"][:Q]
    ids, sc, top_p = system.recommend_batch(U, top_k_retrieval=K, final_k=10, user_meta=metas)
    assert ids.shape == sc.shape == top_p.shape == (Q, 10)
    assert (top_p[:, :-1] >= top_p[:, 1:]).all() and (top_p > 0).all() and (top_p < 1).all()
    recs = system.recommend(U[0], metas[0], top_k_retrieval=K, final_k=10)
    assert len(recs) == 10 and all(0 <= r["product_id"] < N for r in recs)
    got = np.asarray([r["final_score"] for r in recs], np.float32)
    assert np.all(got[:-1] >= got[1:]) and np.all((got > 0) & (got < 1))
    with pytest.raises(ValueError):
        system.rerank_batch(ids, sc, final_k=5)               # the native ranker needs user_vectors
