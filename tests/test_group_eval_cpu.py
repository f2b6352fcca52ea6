"""CPU checks of the grouped evaluation: the per-group reference of tests/group_eval_ref.py against
scikit-learn (ndcg_score with ties averaged, roc_auc_score), the discount table, fit's metric-name
parsing, and the entry points' workspace size and argument checks (no GPU: every native call below is
rejected before a launch, or computes a size on the host)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native, ops
from recsys_amd.temp_model import ranker_skelet as RS
from tests import group_eval_ref as GREF


def _tie_heavy(seed=0, R=3000, G=200):
    rng = np.random.default_rng(seed)
    z = np.round(rng.standard_normal(R), 1).astype(np.float32)      # one decimal: ties are common
    y = (rng.random(R) < 0.3).astype(np.int64)
    g = rng.integers(0, G, R)
    return z, y, g


@pytest.mark.parametrize("top", [1, 5, 10, 1000])
def test_reference_matches_sklearn(top):
    from sklearn.metrics import ndcg_score, roc_auc_score
    z, y, g = _tie_heavy()
    assert top != 1000 or np.bincount(g).max() < top      # "larger than every group"
    groups = GREF.per_group(z, y, g, top)
    assert [r["gid"] for r in groups] == sorted(set(g.tolist()))
    D = ops.ndcg_discounts(top).tolist()
    worst_n = worst_a = 0.0
    n_ndcg = n_auc = 0
    for r in groups:
        sel = g == r["gid"]
        zz, yy = z[sel].astype(np.float64), y[sel]
        assert (r["rows"], r["P"], r["N"]) == (len(yy), int(yy.sum()), len(yy) - int(yy.sum()))
        assert 0 <= r["U2"] <= 2 * r["P"] * r["N"]
        if r["P"] > 0:
            ref = 1.0 if len(yy) == 1 else ndcg_score(yy[None, :], zz[None, :], k=top)
            worst_n = max(worst_n, abs(r["dcg"] / D[min(r["P"], top)] - ref))
            n_ndcg += 1
            if r["N"] > 0:
                worst_a = max(worst_a, abs(r["U2"] / (2 * r["P"] * r["N"]) - roc_auc_score(yy, zz)))
                n_auc += 1
    print(f"top {top}: {n_ndcg} groups with a positive, worst NDCG difference {worst_n:.2e}; "
          f"{n_auc} two-class groups, worst AUC difference {worst_a:.2e}")
    assert n_ndcg >= 100 and n_auc >= 100
    assert worst_n <= 1e-12 and worst_a <= 1e-12
    s = GREF.summary(groups, top)
    assert (s["groups"], s["ndcg_groups"], s["auc_groups"]) == (len(groups), n_ndcg, n_auc)
    assert 0.0 < s["ndcg"] <= 1.0 and 0.0 < s["query_auc"] < 1.0


def test_reference_small_cases():
    # one group, descending scores 3 > 2 > 1 with the positive in the middle: DCG = 1 / log2(3)
    (r,) = GREF.per_group([1.0, 3.0, 2.0], [0, 0, 1], [4, 4, 4], 10)
    assert (r["gid"], r["P"], r["N"], r["U2"]) == (4, 1, 2, 2) and r["dcg"] == 1.0 / math.log2(3)
    # all tied: every position shares the discounts; AUC_g = 1/2
    (r,) = GREF.per_group([0.0, -0.0, 0.0, 0.0], [1, 0, 0, 1], [0] * 4, 2)
    D = ops.ndcg_discounts(2).tolist()
    assert r["U2"] == r["P"] * r["N"] == 4 and r["dcg"] == 2 * D[2] / 4
    # no qualifying group
    s = GREF.summary(GREF.per_group([0.5, 0.25], [0, 0], [1, 2], 10), 10)
    assert math.isnan(s["ndcg"]) and math.isnan(s["query_auc"]) and s["groups"] == 2


@pytest.mark.parametrize("top", [1, 2, 10, 1000, 65536])
def test_discount_table(top):
    D = ops.ndcg_discounts(top)
    assert D.dtype == torch.float64 and D.device.type == "cpu" and tuple(D.shape) == (top + 1,)
    assert D[0] == 0.0 and D[1] == 1.0
    ref = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(top, dtype=np.float64) + 2.0))])
    rel = np.abs(D.numpy() - ref) / np.maximum(ref, 1.0)
    print(f"top {top}: worst relative difference to numpy's cumulative sum {rel.max():.2e}")
    assert rel.max() <= 1e-15      # both are sequential float64 sums; the two log2 may differ in the last bit
    assert ops.ndcg_discounts(top) is D      # cached


def test_discount_table_rejects_bad_top():
    for top in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError, match="top must be"):
            ops.ndcg_discounts(top)


def test_metric_names():
    assert RS._parse_eval_metric("AUC") == ("AUC", 10) and RS._parse_eval_metric("Logloss") == ("Logloss", 10)
    assert RS._parse_eval_metric("NDCG") == ("NDCG", 10) and RS._parse_eval_metric("QueryAUC") == ("QueryAUC", 10)
    assert RS._parse_eval_metric("NDCG:top=5") == ("NDCG", 5)
    assert RS._parse_eval_metric("NDCG:top=65536") == ("NDCG", 65536)
    for bad in ("NDCG:top=", "NDCG:top=five", "NDCG:k=5", "NDCG:top=-3", "NDCG:top=5;x", "NDCG:"):
        with pytest.raises(ValueError, match="eval_metric"):
            RS._parse_eval_metric(bad)
    for bad in ("NDCG:top=0", "NDCG:top=65537"):
        with pytest.raises(ValueError, match=r"eval_metric.*top must be"):
            RS._parse_eval_metric(bad)
    for bad in ("ndcg", "PFound", "QueryAUC:top=3", None, 7):
        with pytest.raises(ValueError, match="eval_metric must be"):
            RS._parse_eval_metric(bad)


@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_fit_argument_checks_need_no_data(kind):
    """The checks come before any row is touched: a CPU model and empty rows are enough."""
    if kind == "deepfm":
        model = RS.DeepFM([10] * 3)
        rows, val = (torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4)), (None, None)
    else:
        model = RS.RankingModel(8, 8, 4)
        rows, val = (torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 4), torch.zeros(4)), (None,) * 4
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match="eval_metric must be"):
        model.fit(*rows, batch_size=2, eval_set=val, eval_metric="PFound")
    for metric in ("NDCG", "NDCG:top=5", "QueryAUC"):
        with pytest.raises(ValueError, match="eval_metric.*eval_group_id"):
            model.fit(*rows, batch_size=2, eval_set=val, eval_metric=metric)
    with pytest.raises(ValueError, match="eval_metric"):
        model.fit(*rows, batch_size=2, eval_set=val, eval_metric="NDCG:top=x", eval_group_id=[0] * 4)
    with pytest.raises(ValueError, match="top must be"):
        model.fit(*rows, batch_size=2, eval_set=val, eval_metric="NDCG:top=0", eval_group_id=[0] * 4)
    with pytest.raises(ValueError, match="eval_group_id needs an eval_set"):
        model.fit(*rows, batch_size=2, eval_group_id=[0] * 4)
    for a, b in zip(model.parameters(), before):
        assert torch.equal(a, b)


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


P16 = ctypes.c_void_p(256)   # a non-null, aligned pointer that is never dereferenced: the calls are rejected first


def test_group_eval_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    need = lib.rsx_group_eval_workspace_bytes(1000)
    assert need > 0

    def call(R=1000, top=10, max_gid=-1, ws_bytes=need, **ptrs):
        p = {n: ptrs.get(n, P16) for n in ("logit", "y", "gid_in", "D", "ws", "summary", "gid", "P", "N", "U2", "dcg",
                                           "flag")}
        return lib.rsx_group_eval(p["logit"], p["y"], p["gid_in"], R, top, p["D"], max_gid, p["ws"], ws_bytes,
                                  p["summary"], p["gid"], p["P"], p["N"], p["U2"], p["dcg"], p["flag"], None)

    assert call(R=0) == 1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    assert call(R=1 << 31) == 1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    assert call(top=0) == 1 and b"1 <= top <= 65536" in lib.rsx_last_error()
    assert call(top=65537) == 1 and b"1 <= top <= 65536" in lib.rsx_last_error()
    assert call(max_gid=-2) == 1 and b"max_group_id" in lib.rsx_last_error()
    assert call(max_gid=1 << 31) == 1 and b"max_group_id" in lib.rsx_last_error()
    for name in ("logit", "y", "gid_in", "D", "ws", "summary", "gid", "P", "N", "U2", "dcg", "flag"):
        assert call(**{name: None}) == 1 and b"null tensor" in lib.rsx_last_error(), name
    assert call(ws_bytes=need - 1) == 1 and b"workspace too small" in lib.rsx_last_error()
    assert call(summary=ctypes.c_void_p(260)) == 1 and b"misaligned" in lib.rsx_last_error()
    assert lib.rsx_group_eval_workspace_bytes(0) == -1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    assert lib.rsx_group_eval_workspace_bytes(1 << 31) == -1


def test_workspace_bytes_is_non_decreasing():
    """Over the tile size (2048 rows), the powers of two and their neighbours, and the largest R."""
    lib = _lib()
    sweep = set(range(1, 70)) | {(1 << 31) - 1}
    for p in range(6, 31):
        sweep |= {(1 << p) - 1, 1 << p, (1 << p) + 1, 3 << (p - 1)}
    sweep |= {k * 2048 + d for k in (1, 2, 3, 33, 34) for d in (-1, 0, 1)}
    sweep |= {1000, 4099, 65536, 70001, 100000, 300000, 1048576, 5000000}
    sizes = [(R, lib.rsx_group_eval_workspace_bytes(R)) for R in sorted(sweep)]
    for (r0, s0), (r1, s1) in zip(sizes, sizes[1:]):
        assert 0 < s0 <= s1, f"workspace shrinks from R = {r0} ({s0} B) to R = {r1} ({s1} B)"
    # the four pair arrays alone are 18 bytes a row
    assert all(s >= 18 * R for R, s in sizes)
