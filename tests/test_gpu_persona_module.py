"""staticstics/preprocess_clustering.py end to end on a synthetic log of about 3,000 rows, 120 customers and 60 items
with five items per three-character category (tests/persona_ref.persona_log), against the pandas / scipy / numpy
oracle: the seven columns one by one (basket_size, weekend_ratio and repurchase_rate are ratios of integers: exact;
the others within 1e-12 relative), the clustering against the oracle's seeding and Lloyd on the same standardised
columns, and the persona list as the same dicts. The frame and the fit are made once per module."""
import json

import numpy as np
import pytest
import torch

from recsys_amd import ops
from recsys_amd.staticstics import preprocess_clustering as PC
from tests import persona_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames(gpu):
    df = PR.persona_log()
    tab = PC.TransactionTable.from_frame(df, gpu)
    got = PC.persona_features(tab)
    again = PC.persona_features(PC.TransactionTable.from_frame(df, gpu))
    return df, tab, got, again, PR.features(df)


def test_persona_features_equal_the_oracle_column_by_column(frames):
    df, tab, got, again, want = frames
    assert 2900 <= len(df) <= 3100 and len(want) == 120 and tab.n_items == 60
    assert list(got.columns) == ["customer_id"] + PR.COLS and got["customer_id"].tolist() == want["customer_id"].tolist()
    for name in ("basket_size", "weekend_ratio", "repurchase_rate"):
        assert got[name].dtype == np.float64 and (got[name].to_numpy() == want[name].to_numpy()).all(), name
    for name in ("avg_price", "cat_entropy", "long_tail_ratio", "relative_price_pos"):
        g, w = got[name].to_numpy(), want[name].to_numpy()
        err = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        print(f"{name}: largest relative error {np.where(w == 0, np.abs(g), err).max():.3e}")
        assert (np.abs(g - w) <= 1e-12 * np.abs(w)).all(), name
    assert (want["cat_entropy"] == 0).any() and (want["cat_entropy"] > 1).any()
    assert 0 < want["long_tail_ratio"].mean() < 1 and (want["repurchase_rate"] > 0).any()
    for name in PR.COLS:                                           # a second table: the same bits
        assert got[name].to_numpy().tobytes() == again[name].to_numpy().tobytes(), name
    # the towers' repurchase_ratio is another quantity and still there
    ratio = tab.user_features()[1][ops.TX_USER_COLUMNS.index("repurchase_ratio")].cpu().numpy()
    assert not np.allclose(ratio, got["repurchase_rate"].to_numpy(), atol=1e-3)
    tab.check()


def test_the_head_items_break_ties_by_item_index_on_the_device(frames):
    df, tab, got, _, want = frames
    counts = tab.item_stats()["count"].cpu().numpy()
    n_head = max(int(0.2 * tab.n_items), 1)
    order = np.lexsort((np.arange(tab.n_items), -counts))
    assert counts[order[n_head - 1]] == counts[order[n_head]] or len(set(counts.tolist())) < len(counts)      # there are ties
    assert {str(a) for a in tab.article_ids[order[:n_head]]} == PR.head_items(df["article_id"].astype(str))


@pytest.fixture(scope="module")
def clustering(frames, gpu):
    _, _, got, _, _ = frames
    labels, model, mean, scale = PC.cluster_personas(got, n_clusters=6, random_state=42)
    return labels, model, mean, scale, PC.cluster_personas(got, n_clusters=6, random_state=42)


def test_cluster_personas_is_the_oracles_seeding_and_fit_of_the_standardised_columns(frames, clustering, gpu):
    _, _, got, _, _ = frames
    labels, model, mean, scale, again = clustering
    X = got[PR.COLS].to_numpy(dtype=np.float64).T
    Z, w_mean, w_scale, _ = PR.standardize(X)
    assert np.abs(mean - w_mean).max() <= 1e-13 * np.abs(w_mean).max() and np.abs(scale - w_scale).max() <= 1e-12
    # the oracle runs on the device's standardised columns: the grid points must be the same integers
    Zd = ops.standardize_columns(torch.from_numpy(np.ascontiguousarray(X)).to(gpu))[0].cpu().numpy()
    assert np.abs(Zd - Z).max() <= 1e-11
    bits = PR.frac_bits(Zd)
    q = PR.quantize(Zd, bits)
    assert bits == model.frac_bits_
    x = (q.astype(np.float64) * 2.0 ** -bits).T
    rows = PR.seeds(q, bits, 6, 42)
    tol_abs = 1e-4 * float(ops.standardize_columns(torch.from_numpy(np.ascontiguousarray(x.T)).to(gpu), out=False)[3].mean())
    centres, w_labels, dmin, n_iter, counts = PR.lloyd(q, bits, x[rows], tol_abs)
    assert labels.dtype == np.int32 and labels.tolist() == w_labels.tolist() == model.labels_.tolist()
    assert model.cluster_centers_.tobytes() == centres.tobytes() and model.n_iter_ == n_iter
    assert abs(model.inertia_ - dmin.sum()) <= len(labels) * 2.0 ** -52 * dmin.sum()
    assert model.predict(Zd.T).tolist() == labels.tolist()                     # predict on the training rows
    assert model.predict(torch.from_numpy(Zd.T.copy()).to(gpu)).tolist() == labels.tolist()
    assert again[0].tolist() == labels.tolist() and again[1].cluster_centers_.tobytes() == centres.tobytes()
    assert PC.DeviceKMeans(6, random_state=42, n_init=3).fit(Zd.T).inertia_ <= model.inertia_
    given = PC.DeviceKMeans(6, init=x[rows]).fit(Zd.T)
    assert given.labels_.tolist() == labels.tolist() and given.n_iter_ == n_iter
    with pytest.raises(ValueError, match="n_samples"):
        PC.DeviceKMeans(8).fit(Zd.T[:5])


def test_persona_stats_equal_the_references_json(frames, clustering):
    _, _, got, _, want = frames
    labels = clustering[0]
    stats = PC.persona_stats(got, labels)
    assert stats == PR.persona_json(got, labels)
    assert stats == PR.persona_json(want, labels)                              # and from the oracle's own columns
    assert sum(p["user_count"] for p in stats) == len(got) and json.loads(PC.personas_json(stats)) == stats
    # a cluster nobody is in is left out; a cluster of one has std 0.0
    moved = labels.copy()
    moved[moved == 1] = 0
    moved[0] = 7
    out = PC.persona_stats(got, moved)
    assert out == PR.persona_json(got, moved) and [p["cluster_id"] for p in out][-1] == 7
    assert 1 not in [p["cluster_id"] for p in out] and out[-1]["stats"]["basket_size"]["std"] == 0.0
    assert PC.persona_stats(got, torch.from_numpy(moved), n_clusters=9) == out
