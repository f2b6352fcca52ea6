"""RecommendationRanker.train_rows and ReRankingSystem with a target-statistic column: the 300-item, 40-customer
world of tests/test_gpu_ranker_rows_fit.py with every item's material distinct, 300 values where a one-hot
column takes 255. 20 trees; the world and the fit are made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.temp_model.ranker_skelet import RecommendationRanker, ReRankingSystem
from recsys_amd.utils.monitor.log_importer import HMLogImporter

pytestmark = pytest.mark.gpu

N, C, D, TREES = 300, 40, 128, 20
CATEGORY, FIT, SEASON, GENDER = ("top", "dress", "shoe", "bag"), ("slim", "regular"), ("SS", "FW"), ("F", "M", "U")


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    rng = np.random.default_rng(11)
    V = rng.integers(-1, 2, (N, D)).astype(np.float32)
    U = rng.integers(-1, 2, (C, D)).astype(np.float32)
    items = {i: {"category": CATEGORY[rng.integers(4)], "material": f"blend-{i}", "fit": FIT[rng.integers(2)],
                 "price": float(rng.integers(4, 400)) / 4} for i in range(N)}
    users = [{"season": SEASON[rng.integers(2)], "gender": GENDER[rng.integers(3)],
              "avg_price": float(2 ** rng.integers(3, 7))} for _ in range(C)]
    keys, customers = [f"a{i:03d}" for i in range(N)], [f"c{i:02d}" for i in range(C)]
    score = U @ V.T
    path = tmp_path_factory.mktemp("log") / "t.csv"
    with open(path, "w") as f:
        f.write("t_dat,customer_id,article_id,price,sales_channel_id\n")
        for _ in range(600):                    # a customer buys among the items its vector scores highest
            u = int(rng.integers(C))
            f.write(f"2020-09-01,{customers[u]},{keys[int(np.argsort(-score[u])[rng.integers(60)])]},0.01,2\n")
    dU, dV = torch.from_numpy(U).to(gpu), torch.from_numpy(V).to(gpu)
    imp = HMLogImporter(str(path), {k: V[i] for i, k in enumerate(keys)}, device=gpu)
    rows = imp.load_rows(negative_ratio=5, seed=42, user_vectors=dU, customer_index={c: i for i, c in enumerate(customers)})
    ops._RANKER_ROWS_GUARD.check()
    ranker = RecommendationRanker(backend="native", one_hot_max_size=32)
    ranker.model.iterations = TREES
    ranker.train_rows(rows, dV, dU, items, users)
    ops._GBDT_TS_GUARD.check()
    return {"U": U, "V": V, "dU": dU, "dV": dV, "items": items, "users": users, "rows": rows, "ranker": ranker}


def _columns(world, clf, items, row_user, row_item, score, user_vectors, user_meta):
    """(numeric [R, 7], codes [R, 5]) of the rows through ops.pair_tabular and the model's vocabularies."""
    gpu = row_user.device
    price = torch.tensor([float(items[i].get("price", 0)) for i in range(N)], device=gpu)
    avg = torch.tensor([float(m.get("avg_price", 0.0)) for m in user_meta], device=gpu)
    feats = ops.pair_tabular(row_user, row_item, score, user_vectors, world["dV"], price, avg)
    cols = []
    for name, vocab in zip(clf._fitted_names[1], clf.vocab_):
        side, key = ReRankingSystem._TABULAR_CATS[name]
        metas = [items[i] for i in range(N)] if side == "item" else user_meta
        table = torch.tensor([vocab.get(m.get(key, "unknown"), 0) for m in metas], device=gpu)
        cols.append(table.index_select(0, (row_item if side == "item" else row_user).long()))
    return feats.t(), torch.stack(cols, dim=1)


def test_train_rows_fits_with_the_parameter_and_raises_without(world):
    ranker, clf = world["ranker"], world["ranker"].model
    assert ranker.is_fitted and clf.tree_count_ == TREES
    assert clf._fitted_names[1][3] == "item_material" and clf.ts_cols_ == [3] and len(clf.vocab_[3]) == N
    assert clf.model_.is_cat.cpu().tolist() == [0] * 8 + [1] * 4
    assert clf.ts_bins_[0].dtype == torch.uint8 and clf.ts_bins_[0].numel() <= N + 1
    plain = RecommendationRanker(backend="native")
    plain.model.iterations = 2
    with pytest.raises(ValueError, match="at most 255"):
        plain.train_rows(world["rows"], world["dV"], world["dU"], world["items"], world["users"])


def _serve(world, items, Q=6, K=100):
    gpu = world["dU"].device
    clf = world["ranker"].model
    rng = np.random.default_rng(9)
    cand = np.stack([rng.permutation(N)[:K] for _ in range(Q)])
    score = np.einsum("qd,qkd->qk", world["U"][:Q], world["V"][cand]).astype(np.float32)
    dcand, dscore = torch.from_numpy(cand).to(gpu), torch.from_numpy(score).to(gpu)
    metas = world["users"][:Q]
    system = ReRankingSystem(None, None, world["ranker"], items, world["dV"])
    ids, _, top = system.rerank_batch(dcand, dscore, final_k=K, user_vectors=world["dU"][:Q], user_meta=metas)
    ops._RERANK_GUARD.check()
    row_user = torch.arange(Q, device=gpu, dtype=torch.int32).repeat_interleave(K)
    X = _columns(world, clf, items, row_user, dcand.reshape(-1).to(torch.int32), dscore.reshape(-1),
                 world["dU"][:Q].contiguous(), metas)
    ops._PAIR_GUARD.check()
    return dcand, ids, top, X


def test_serving_scores_are_predict_logits_of_the_pairs_columns_bit_for_bit(world):
    clf = world["ranker"].model
    dcand, ids, top, X = _serve(world, world["items"])
    prob = torch.sigmoid(clf.predict_logits(X)).view(dcand.shape)
    assert torch.equal(top, torch.topk(prob, dcand.shape[1], dim=1).values)          # the same bits, every candidate
    where = torch.gather(prob, 1, torch.argsort(dcand, 1).gather(1, torch.searchsorted(dcand.sort(1).values, ids)))
    assert torch.equal(where, top)                                                     # ... and each with its own item
    assert len(torch.unique(top)) > 20
    used = set(clf.model_.splits[:TREES, :, 0].reshape(-1).tolist())
    print(f"split features used: {sorted(used)} (7 is item_material's statistic)")


def test_an_unseen_material_serves_as_code_zero(world):
    clf = world["ranker"].model
    items = {i: dict(m) for i, m in world["items"].items()}
    for i in (7, 150, 299):
        items[i]["material"] = "never seen"
    dcand, ids, top, X = _serve(world, items)
    changed = torch.isin(dcand, torch.tensor([7, 150, 299], device=dcand.device))
    assert changed.sum() > 0 and torch.equal(X[1][:, 3] == 0, changed.reshape(-1))     # the vocabulary gives them code 0
    prob = torch.sigmoid(clf.predict_logits(X)).view(dcand.shape)
    where = torch.gather(prob, 1, torch.argsort(dcand, 1).gather(1, torch.searchsorted(dcand.sort(1).values, ids)))
    assert torch.equal(where, top)
    base = _serve(world, world["items"])
    assert torch.equal(torch.sigmoid(clf.predict_logits(base[3])).view(dcand.shape)[~changed], prob[~changed])


def test_save_and_load_round_trip(world, tmp_path):
    path = str(tmp_path / "ranker.pt")
    world["ranker"].save_model(path)
    assert torch.load(path, map_location="cpu", weights_only=False)["format"] == "oblivious_gbdt/2"
    loaded = RecommendationRanker(model_path=path, backend="native")
    assert loaded.model.ts_cols_ == [3] and loaded.model.vocab_ == world["ranker"].model.vocab_
    a = ReRankingSystem(None, None, world["ranker"], world["items"], world["dV"]).recommend_batch(
        world["dU"][:5], top_k_retrieval=100, final_k=10, user_meta=world["users"][:5])
    b = ReRankingSystem(None, None, loaded, world["items"], world["dV"]).recommend_batch(
        world["dU"][:5], top_k_retrieval=100, final_k=10, user_meta=world["users"][:5])
    ops._RERANK_GUARD.check()
    assert all(torch.equal(x, z) for x, z in zip(a, b))
