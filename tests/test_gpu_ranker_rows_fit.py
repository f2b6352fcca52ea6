"""Logs -> rows -> columns -> fit on the device: HMLogImporter against the reference's loop restated by
tests/ranker_rows_ref.py, RecommendationRanker.train_rows against fit called on the ops' outputs and against
tests/gbdt_ref.py, and the trained model served by ReRankingSystem with the columns it was trained on. A world
of 300 items and 40 customers, d = 128, 20 trees; the fits are made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier
from recsys_amd.temp_model.ranker_skelet import RecommendationRanker, ReRankingSystem
from recsys_amd.utils.monitor.log_importer import HMLogImporter, RankerRows
from tests import gbdt_ref as G
from tests import ranker_rows_ref as RR

pytestmark = pytest.mark.gpu

N, C, D, TREES = 300, 40, 128, 20
CATEGORY, MATERIAL, FIT = ("top", "dress", "shoe", "bag"), ("cotton", "wool", "linen"), ("slim", "regular")
SEASON, GENDER = ("SS", "FW"), ("F", "M", "U")


def _write(path, lines):
    with open(path, "w") as f:
        f.write("t_dat,customer_id,article_id,price,sales_channel_id\n")
        for c, a in lines:
            f.write(f"2020-09-01,{c},{a},0.01,2\n")
    return str(path)


def test_load_and_preprocess_equals_the_references_loop(gpu, tmp_path):
    rng = np.random.default_rng(5)
    keys = [f"0{700000 + 7 * i}" for i in rng.permutation(40)]               # 40 articles, store order not sorted
    store = {k: rng.standard_normal(128).astype(np.float32) for k in keys}
    customers = [f"{rng.integers(1 << 60):016x}" for _ in range(20)]
    lines = [(customers[rng.integers(20)], keys[rng.integers(40)] if rng.random() < 0.85 else "0999999999")
             for _ in range(150)]
    lines += [lines[3], lines[3], (customers[0], "0999999999")]               # repeated purchases, an unknown article
    imp = HMLogImporter(_write(tmp_path / "t.csv", lines), store, device=gpu)
    for limit, K in ((100000, 5), (60, 2)):
        X_user, X_item, y, groups = imp.load_and_preprocess(limit=limit, negative_ratio=K, seed=42)
        items, wy, wg = RR.importer(lines, keys, limit, K, 42)
        assert (X_user.dtype, X_item.dtype, y.dtype, groups.dtype) == (np.float32, np.float32, np.float32, np.int32)
        R = len(wy)
        assert X_user.shape == (R, 128) and not X_user.any() and X_item.shape == (R, 128)
        table = np.stack([store[k] for k in keys])
        assert np.array_equal(X_item, table[items]) and np.array_equal(y, wy) and np.array_equal(groups, wg)
        assert np.all(np.diff(groups) >= 0) and y.reshape(-1, K + 1)[:, 0].all() and y.sum() == R // (K + 1)
        by = {}
        for c, a in lines[:limit]:
            by.setdefault(c, set()).add(a)
        bought = [{keys.index(a) for a in by[c] if a in store} for c in sorted(by)]
        neg = y == 0
        assert all(i not in bought[g] for i, g in zip(items[neg], groups[neg]))      # a negative was never bought
        assert all(i in bought[g] for i, g in zip(items[~neg], groups[~neg]))


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    """Vectors with entries in {-1, 0, 1} and prices on a dyadic grid (as tests/test_gpu_gbdt_rerank.py): every
    column is exact in fp32, so the retrieval score of a pair and its dot product are the same number."""
    rng = np.random.default_rng(11)
    V = rng.integers(-1, 2, (N, D)).astype(np.float32)
    U = rng.integers(-1, 2, (C, D)).astype(np.float32)
    items = {i: {"category": CATEGORY[rng.integers(4)], "material": MATERIAL[rng.integers(3)], "fit": FIT[rng.integers(2)],
                 "price": float(rng.integers(4, 400)) / 4} for i in range(N)}
    del items[17]["material"]
    del items[23]
    users = [{"season": SEASON[rng.integers(2)], "gender": GENDER[rng.integers(3)],
              "avg_price": float(2 ** rng.integers(3, 7))} for _ in range(C)]
    users[1]["avg_price"] = 0.0
    users[2] = {"season": "AW"}
    keys = [f"a{i:03d}" for i in range(N)]
    customers = [f"c{i:02d}" for i in range(C)]
    score = U @ V.T
    lines = []
    for _ in range(600):                        # a customer buys among the items its vector scores highest
        u = int(rng.integers(C))
        liked = np.argsort(-score[u])[:60]
        lines.append((customers[u], keys[int(liked[rng.integers(60)])]))
    path = _write(tmp_path_factory.mktemp("log") / "t.csv", lines)
    store = {k: V[i] for i, k in enumerate(keys)}
    dU, dV = torch.from_numpy(U).to(gpu), torch.from_numpy(V).to(gpu)
    imp = HMLogImporter(path, store, device=gpu)
    rows = imp.load_rows(negative_ratio=5, seed=42, user_vectors=dU,
                         customer_index={c: i for i, c in reversed(list(enumerate(customers)))})
    ops._RANKER_ROWS_GUARD.check()
    ranker = RecommendationRanker(backend="native")
    ranker.model.iterations = TREES
    ranker.train_rows(rows, dV, dU, items, users)
    system = ReRankingSystem(None, None, ranker, items, dV)
    return {"U": U, "V": V, "dU": dU, "dV": dV, "items": items, "users": users, "rows": rows, "ranker": ranker,
            "system": system, "lines": lines, "keys": keys, "customers": customers, "importer": imp}


def _columns(world, clf, row_user, row_item, score, user_vectors, user_meta):
    """(numeric [R, 7], codes [R, 5]) of the rows through ops.pair_tabular and the model's vocabularies."""
    gpu = row_user.device
    items, n = world["items"], N
    price = torch.tensor([float(items.get(i, {}).get("price", 0)) for i in range(n)], device=gpu)
    avg = torch.tensor([float(m.get("avg_price", 0.0)) for m in user_meta], device=gpu)
    feats = ops.pair_tabular(row_user, row_item, score, user_vectors, world["dV"], price, avg)
    cols = []
    for name, vocab in zip(clf._fitted_names[1], clf.vocab_):
        side, key = ReRankingSystem._TABULAR_CATS[name]
        metas = [items.get(i, {}) for i in range(n)] if side == "item" else user_meta
        table = torch.tensor([vocab.get(m.get(key, "unknown"), 0) for m in metas], device=gpu)
        cols.append(table.index_select(0, (row_item if side == "item" else row_user).long()))
    return feats.t(), torch.stack(cols, dim=1)


def test_the_rows_are_the_importers(gpu, world):
    rows = world["rows"]
    items, y, groups = RR.importer(world["lines"], world["keys"], 100000, 5, 42)
    assert isinstance(rows, RankerRows) and rows.score is None and len(rows) == len(y) == 3600
    assert rows.row_user.dtype == rows.row_item.dtype == rows.group_id.dtype == torch.int32 and rows.y.dtype == torch.float32
    assert np.array_equal(rows.row_item.cpu().numpy(), items) and np.array_equal(rows.y.cpu().numpy(), y)
    assert np.array_equal(rows.group_id.cpu().numpy(), groups)
    assert np.array_equal(rows.row_user.cpu().numpy(), groups)           # customer c<i> is row i of the user vectors
    with pytest.raises(KeyError):
        world["importer"].load_rows(customer_index={"c00": 0})
    with pytest.raises(ValueError):
        world["importer"].load_rows(user_vectors=world["dU"][:10])
    tr, va = rows.split(0.25, seed=3)
    gt, gv = set(tr.group_id.cpu().tolist()), set(va.group_id.cpu().tolist())
    assert len(tr) + len(va) == len(rows) and not gt & gv and gv and len(gv) < len(gt)        # whole groups move
    again = rows.split(0.25, seed=3)[1]
    assert torch.equal(again.row_item, va.row_item) and torch.equal(again.y, va.y)


def test_train_rows_equals_fit_on_the_ops_outputs_and_the_oracle(gpu, world):
    ranker, rows = world["ranker"], world["rows"]
    clf = ranker.model
    assert ranker.is_fitted and clf.tree_count_ == TREES
    assert clf.feature_names_ == list(ops.RERANK_TABULAR_COLUMNS) + ["season", "gender", "item_category", "item_material",
                                                                     "item_fit"]
    assert set(clf.vocab_[0]) == {"SS", "FW", "AW"} and all("unknown" in v for v in clf.vocab_[1:])
    X = _columns(world, clf, rows.row_user, rows.row_item, None, world["dU"], world["users"])
    direct = ObliviousBoostingClassifier(iterations=TREES, learning_rate=0.05, depth=6, device=gpu).fit(X, rows.y)
    assert torch.equal(direct.model_.splits, clf.model_.splits) and torch.equal(direct.model_.leaf_values, clf.model_.leaf_values)
    assert torch.equal(direct.borders_, clf.borders_) and direct.model_.f0 == clf.model_.f0
    bins = clf._bins(X).cpu().numpy()
    is_cat, n_bins = clf.model_.is_cat.cpu().numpy(), clf.n_bins_.cpu().numpy()
    oracle = G.fit(bins, rows.y.cpu().numpy(), is_cat, n_bins, TREES)
    got_s, got_v = clf.model_.splits[:TREES].cpu().numpy(), clf.model_.leaf_values[:TREES].cpu().numpy()
    want_s, want_v = np.asarray(oracle["splits"]), np.asarray(oracle["values"])
    same = [t for t in range(TREES) if np.array_equal(got_s[t], want_s[t])]
    print(f"trees with the oracle's splits: {len(same)} of {TREES}; max |leaf value - oracle| "
          f"{np.abs(got_v - want_v).max():.3e}")
    assert np.array_equal(got_s, want_s) and np.array_equal(got_v, want_v)
    assert float(oracle["f0"]) == clf.model_.f0
    catboost_like = RecommendationRanker(backend="native")
    catboost_like.backend = "catboost"
    with pytest.raises(TypeError):
        catboost_like.train_rows(rows, world["dV"], world["dU"], world["items"], world["users"])


def test_serving_scores_are_the_training_columns_scores_bit_for_bit(gpu, world):
    system, clf = world["system"], world["ranker"].model
    Q, K = 6, 100
    rng = np.random.default_rng(9)
    cand = np.stack([rng.permutation(N)[:K] for _ in range(Q)])
    score = np.einsum("qd,qkd->qk", world["U"][:Q], world["V"][cand]).astype(np.float32)
    dcand, dscore = torch.from_numpy(cand).to(gpu), torch.from_numpy(score).to(gpu)
    metas = world["users"][:Q]
    ids, sc, top = system.rerank_batch(dcand, dscore, final_k=K, user_vectors=world["dU"][:Q], user_meta=metas)
    ops._RERANK_GUARD.check()
    row_user = torch.arange(Q, device=gpu, dtype=torch.int32).repeat_interleave(K)
    X = _columns(world, clf, row_user, dcand.reshape(-1).to(torch.int32), dscore.reshape(-1), world["dU"][:Q].contiguous(), metas)
    ops._PAIR_GUARD.check()
    prob = torch.sigmoid(clf.predict_logits(X)).view(Q, K)
    want_p, want_j = torch.topk(prob, K, dim=1)
    assert torch.equal(top, want_p)                                        # the same bits, every candidate
    where = torch.gather(prob, 1, torch.argsort(dcand, 1).gather(1, torch.searchsorted(dcand.sort(1).values, ids)))
    assert torch.equal(where, top)                                         # ... and each with its own item
    assert len(torch.unique(top)) > 20
    # the rows' own columns: with score None the two-tower score is the dot product, here the same number
    again = _columns(world, clf, row_user, dcand.reshape(-1).to(torch.int32), None, world["dU"][:Q].contiguous(), metas)
    assert torch.equal(again[0], X[0])


def test_a_query_softmax_fit_from_training_rows_runs_and_serves(gpu, world):
    system, U, V = world["system"], world["U"], world["V"]
    rng = np.random.default_rng(2)
    score = U @ V.T
    truth = [sorted(set(np.argsort(-score[u], kind="stable")[:3].tolist()) | set(rng.integers(0, N, 2).tolist()))
             for u in range(C)]
    truth[5] = []
    off = np.zeros(C + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in truth])
    flat = np.asarray([i for s in truth for i in s], np.int32)
    with pytest.raises(ValueError):
        system.training_rows(world["dU"], torch.from_numpy(off).to(gpu), torch.from_numpy(flat).to(gpu), top_k_retrieval=N + 1)
    rows = system.training_rows(world["dU"], torch.from_numpy(off).to(gpu), torch.from_numpy(flat).to(gpu), top_k_retrieval=100)
    ops._PAIR_GUARD.check()
    assert len(rows) == C * 100 and rows.score is not None
    item, y = rows.row_item.cpu().numpy().reshape(C, 100), rows.y.cpu().numpy().reshape(C, 100)
    for u in range(C):
        assert np.array_equal(y[u], np.isin(item[u], truth[u]).astype(np.float32)), u
        assert np.array_equal(np.sort(rows.score.cpu().numpy().reshape(C, 100)[u])[::-1], np.sort(score[u])[::-1][:100])
    assert y[5].sum() == 0 and y.sum() >= 3 * (C - 1)
    assert np.array_equal(rows.group_id.cpu().numpy(), np.repeat(np.arange(C), 100))
    ranker = RecommendationRanker(backend="native", loss_function="QuerySoftMax")
    ranker.model.iterations = TREES
    train, val = rows.split(0.3, seed=1)
    ranker.train_rows(train, world["dV"], world["dU"], world["items"], world["users"], val_rows=val)
    clf = ranker.model
    assert ranker.is_fitted and 1 <= clf.tree_count_ == clf.best_iteration_ + 1 <= TREES
    assert len(clf.evals_result_["validation"]["NDCG"]) >= clf.tree_count_
    served = ReRankingSystem(None, None, ranker, world["items"], world["dV"])
    ids, sc, final = served.recommend_batch(world["dU"][:8], top_k_retrieval=100, final_k=10, user_meta=world["users"][:8])
    ops._RERANK_GUARD.check()
    assert ids.shape == final.shape == (8, 10) and (final[:, :-1] >= final[:, 1:]).all()
    X = _columns(world, clf, train.row_user, train.row_item, train.score, world["dU"], world["users"])
    ll = clf.evals_result_["learn"]["QuerySoftMax"]
    assert ll[-1] < ll[0]
    assert clf.predict(X).shape == (len(train),)


def test_save_and_load_round_trip_the_names_the_vocabularies_and_the_scores(gpu, world, tmp_path):
    ranker, system = world["ranker"], world["system"]
    path = str(tmp_path / "ranker.pt")
    ranker.save_model(path)
    loaded = RecommendationRanker(model_path=path, backend="native")
    assert loaded.is_fitted and loaded.model.feature_names_ == ranker.model.feature_names_
    assert loaded.model.vocab_ == ranker.model.vocab_ and loaded.model.tree_count_ == TREES
    again = ReRankingSystem(None, None, loaded, world["items"], world["dV"])
    a = system.recommend_batch(world["dU"][:5], top_k_retrieval=100, final_k=10, user_meta=world["users"][:5])
    b = again.recommend_batch(world["dU"][:5], top_k_retrieval=100, final_k=10, user_meta=world["users"][:5])
    ops._RERANK_GUARD.check()
    assert all(torch.equal(x, z) for x, z in zip(a, b))
