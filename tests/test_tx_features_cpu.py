"""CPU checks of the transaction features: the oracle tests/tx_features_ref.py against pandas (the calendar over
every day from 1970 to 2100, the quantile buckets where the specification agrees with pd.qcut exactly) and against
aggregates worked out by hand on a ten-row log, the package surface, and the native entry points' ABI (arity;
argument checks that return before any launch)."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native
from recsys_amd.staticstics import preprosess_agg_parallel as PA
from tests import tx_features_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calendar_equals_pandas_on_every_day_from_1970_to_2100():
    dates = pd.Series(pd.date_range("1970-01-01", "2100-01-01", freq="D"))
    day = np.arange(len(dates))
    assert TR.days_since_epoch(dates).tolist() == day.tolist()
    weekend, month, week = TR.calendar(day)
    dow = dates.dt.dayofweek.to_numpy()
    assert (weekend == (dow >= 5)).all()
    per = dates.dt.to_period("M")
    assert (month == per.dt.year.to_numpy() * 12 + per.dt.month.to_numpy() - 1).all()
    week_start = TR.days_since_epoch(dates - pd.to_timedelta(dow, unit="D"))      # the reference's week_start
    assert (week == (week_start + 3) // 7).all()
    assert (np.diff(week) == (dow[1:] == 0)).all()                                # a new week exactly on Mondays
    assert len(np.unique(week)) == len(np.unique(week_start))


def _columns(n):
    rng = np.random.default_rng(n)
    near = np.full(n, 5.0)
    near[rng.permutation(n)[:3]] = [1.0, 7.5, 9.0]
    return {"ties": rng.integers(1, 8, n).astype(np.float64), "continuous": rng.gamma(2.0, 0.01, n), "near_constant": near}


@pytest.mark.parametrize("n", [11, 101, 701])
@pytest.mark.parametrize("kind", ["ties", "continuous", "near_constant"])
def test_the_quantile_buckets_equal_pd_qcut_where_q_divides_n_minus_1(n, kind):
    x = _columns(n)[kind]
    want = pd.qcut(x, q=10, labels=False, duplicates="drop").astype(np.int8) + 1
    got = TR.qcut_bucket(x, 10)
    assert got.dtype == np.int8 and got.tolist() == want.tolist()
    assert got.min() == 1 and got.max() == len(TR.qcut_edges(x, 10)) - 1


def test_the_quantile_edges_interpolate_and_a_constant_column_is_all_ones():
    assert TR.qcut_bucket(np.full(37, 0.25), 10).tolist() == [1] * 37
    assert TR.qcut_bucket(np.asarray([3.0]), 10).tolist() == [1]
    x = np.asarray([0.0, 1.0, 2.0, 4.0])                      # h = 3 k / 4: 0, .75, 1.5, 2.25, 3
    assert TR.qcut_edges(x, 4).tolist() == [0.0, 0.75, 1.5, 2.5, 4.0]
    assert TR.qcut_bucket(x, 4).tolist() == [1, 2, 3, 4]
    for n in (2, 10, 12, 997, 1276):                         # arbitrary n: the edges are pandas' bit for bit
        x = np.random.default_rng(n).gamma(2.0, 0.01, n)
        assert TR.qcut_edges(x, 10).tolist() == pd.Series(x).quantile(np.linspace(0, 1, 11)).unique().tolist()
        assert TR.qcut_bucket(x, 10).tolist() == (pd.qcut(x, q=10, labels=False, duplicates="drop") + 1).tolist()


# a ten-row log: customer A with a same-day tie (file order decides last_price), B over two months and all on
# weekends, C twice the same item; i1 first sold 13 days before the last day (imputed), i2 15 days (not)
TOY = pd.DataFrame(
    [("2020-09-14", "A", "i1", 0.5, 2), ("2020-09-07", "A", "i2", 0.25, 2), ("2020-09-12", "B", "i1", 1.0, 1),
     ("2020-09-14", "A", "i2", 0.75, 1), ("2020-08-01", "B", "i3", 0.5, 1), ("2020-09-13", "B", "i1", 0.25, 2),
     ("2020-09-22", "C", "i3", 2.0, 2), ("2020-09-12", "B", "i2", 0.125, 1), ("2020-09-22", "C", "i3", 2.0, 2),
     ("2020-09-09", "A", "i1", 0.5, 1)], columns=["t_dat", "customer_id", "article_id", "price", "sales_channel_id"])


def test_the_toy_logs_aggregates_equal_the_ones_worked_out_by_hand():
    d, customers, articles = TR.prepare(TOY)
    assert customers.tolist() == ["A", "B", "C"] and articles.tolist() == ["i1", "i2", "i3"]
    assert d["article_id"].tolist() == ["i2", "i1", "i1", "i2", "i3", "i1", "i2", "i1", "i3", "i3"]
    u = TR.user_columns(d, 3)
    assert u["total_cnt"].tolist() == [4, 4, 2]
    assert u["user_avg_price"].tolist() == [0.5, 1.875 / 4, 2.0]
    assert u["last_price_diff"].tolist() == [0.25, 0.25 - 1.875 / 4, 0.0]       # A: the later line of 09-14
    assert u["repurchase_ratio"].tolist() == [0.5, 0.25, 0.5]
    assert u["weekend_ratio"].tolist() == [0.0, 1.0, 0.0]
    assert u["preferred_channel"].tolist() == [1, 1, 2]                         # A: a mean of exactly 1.5 is not above it
    assert u["active_months"].tolist() == [1, 2, 1]
    assert u["recency_days"].tolist() == [8, 9, 0]
    assert u["price_std"][0] == np.sqrt(0.125 / 3) and u["price_std"][2] == 0.0
    w, weeks = TR.weekly_sales(d, 3)
    assert w.tolist() == [[0, 3, 1, 0], [0, 2, 1, 0], [1, 0, 0, 2]]             # the five empty weeks of August: no column
    assert np.diff(weeks).tolist() == [6, 1, 1]
    cols, is_new = TR.item_columns(d, 3)
    assert is_new.tolist() == [True, False, False]
    raw = dict(zip(TR.ITEM_COLS, cols))
    assert raw["raw_probability"].tolist() == [0.4, 0.3, 0.3]
    assert raw["pop_1w_log"][1:].tolist() == [0.0, np.log1p(2.0)] and raw["pop_1m_log"][2] == np.log1p(3.0)
    assert raw["velocity_1w"][1:].tolist() == [-0.5, 2.0] and raw["velocity_1m"][1:].tolist() == [3.0, 3.0]
    assert raw["days_since_release_log"].tolist() == [np.log1p(13.0), np.log1p(15.0), np.log1p(52.0)]
    # the imputed value: the mean over all three items of the float32 column, i1's own value included
    assert raw["velocity_1w"][0] == (-0.5 - 0.5 + 2.0) / 3
    seqs = TR.sequences(d, 3, [True, False, True])
    assert [s[0].tolist() for s in seqs] == [[0, 0], [2, 0, 0], [2, 2]]
    assert [s[1].tolist() for s in seqs] == [[5, 0], [43, 1, 0], [0, 0]]
    assert [s[0].tolist() for s in TR.sequences(d, 3, [True, True, True], max_len=2)] == [[0, 1], [1, 0], [2, 2]]
    frame = TR.sequence_frame(TOY, ["i2"])
    assert frame["customer_id"].tolist() == ["A", "B"] and frame["sequence_ids"].tolist() == [["i2", "i2"], ["i2"]]
    uf = TR.user_frame(TOY)
    assert list(uf.columns) == TR.USER_FINAL_COLS and uf["active_months"].dtype == np.int16
    assert uf["total_cnt_bucket"].dtype == np.int8 and uf["price_std_scaled"].dtype == np.float32


def test_the_package_has_the_references_functions_and_no_module_level_paths():
    for name in ("make_validation_target_file", "make_item_features", "make_user_features", "make_cleaned_sequences",
                 "make_validation_user_features", "make_validation_sequences", "TransactionTable"):
        assert hasattr(PA, name), name
    assert not [k for k, v in vars(PA).items() if isinstance(v, str) and not k.startswith("__") and os.sep in v]
    assert PA.USER_FINAL_COLS == TR.USER_FINAL_COLS and PA.USER_LEGACY_COLS == TR.USER_LEGACY_COLS
    with pytest.raises(ValueError, match="sales_channel_id"):
        PA.TransactionTable.from_frame(TOY.drop(columns=["sales_channel_id"]))
    assert PA.days_since_epoch(TOY["t_dat"]).tolist() == TR.days_since_epoch(TOY["t_dat"]).tolist()
    truth = PA.make_validation_target_file(TOY, "2020-09-14", "2020-09-22")
    assert truth["customer_id"].tolist() == ["A", "C"] and truth["target_ids"].tolist() == [["i1", "i2"], ["i3", "i3"]]
    assert PA.make_validation_target_file(TOY, "2021-01-01", "2021-01-07") is None
    meta = pd.DataFrame({"customer_id": ["A", "B"], "age": [30.0, None], "FN": [1.0, None], "Active": [None, 1.0],
                         "club_member_status": ["active", None], "fashion_news_frequency": ["Regularly", "NONE"],
                         "postal_code": ["x", "y"]})
    got = TR.customer_meta(meta)
    assert got["club_member_status_idx"].tolist() == [1, 0] and got["fashion_news_frequency_idx"].tolist() == [1, 0]
    assert got["FN"].tolist() == [1, 0] and got["Active"].tolist() == [0, 1] and got["age_bucket"].tolist() == [1, 1]


ENTRIES = ("rsx_tx_calendar", "rsx_tx_segment_rows", "rsx_tx_segment_stats", "rsx_tx_segment_distinct",
           "rsx_tx_weekly_sales", "rsx_tx_item_features", "rsx_tx_user_features", "rsx_quantile_bucket",
           "rsx_tx_sequence_ranks", "rsx_tx_sequences")


def test_the_native_entry_points_have_the_headers_arity_and_reject_bad_arguments_without_a_gpu():
    text = open(os.path.join(ROOT, "include", "recsys_amd.h")).read()
    for name in ENTRIES:
        m = re.search(r"^int\s+" + name + r"\(([^;]*?)\);", text, flags=re.M | re.S)
        assert m, name
        assert len(_native._SIGS[name][1]) == m.group(1).count(",") + 1, name
    assert _native.ABI_VERSION == 19
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.load()
    assert lib.rsx_abi_version() == 19
    p, T = 16, 1000
    err = lib.rsx_last_error
    assert lib.rsx_tx_workspace_bytes(T) == 64 * 4 and lib.rsx_tx_workspace_bytes(0) == -1
    assert lib.rsx_tx_workspace_bytes(1 << 31) == -1
    assert lib.rsx_tx_calendar(p, T, p, p, p, None, None) == 1 and b"null tensor" in err()
    assert lib.rsx_tx_calendar(p, 0, p, p, p, p, None) == 1 and b"2^31" in err()
    assert lib.rsx_tx_segment_rows(p, 3, T, p, 256, None, p, None) == 1 and b"null tensor" in err()
    assert lib.rsx_tx_segment_rows(p, 0, T, p, 256, p, p, None) == 1 and b"segments" in err()
    assert lib.rsx_tx_segment_rows(p, 3, T, p, 255, p, p, None) == 1 and b"workspace" in err()
    assert lib.rsx_tx_segment_rows(p, 3, T, 8, 256, p, p, None) == 1 and b"aligned" in err()
    stats = lambda S, T, ws, nbytes, flag: lib.rsx_tx_segment_stats(p, S, T, None, p, p, p, p, ws, nbytes, p, p, p, p, p, p,  # noqa: E731
                                                                    p, p, flag, None)
    assert stats(3, T, p, 256, None) == 1 and b"null tensor" in err()
    assert stats(3, 1 << 31, p, 1 << 40, p) == 1 and b"2^31" in err()
    assert stats((1 << 31) - 1, T, p, 256, p) == 1 and b"segments" in err()
    assert stats(3, T, p, 64, p) == 1 and b"workspace" in err()
    assert lib.rsx_tx_segment_distinct(p, 3, T, None, p, 256, p, p, None) == 1 and b"null tensor" in err()
    assert lib.rsx_tx_segment_distinct(p, 3, T, p, None, 256, p, p, None) == 1 and b"workspace" in err()
    assert lib.rsx_tx_weekly_sales(p, p, T, p, 0, 5, p, p, None) == 1 and b"weeks" in err()
    assert lib.rsx_tx_weekly_sales(p, p, T, p, 65536, 1 << 15, p, p, None) == 1 and b"N W < 2^31" in err()
    assert lib.rsx_tx_weekly_sales(p, p, T, None, 4, 5, p, p, None) == 1 and b"null tensor" in err()
    assert lib.rsx_tx_item_features(p, 5, 4, p, p, p, T, 100, -1, p, 8, p, None) == 1 and b"cold_days" in err()
    assert lib.rsx_tx_item_features(p, 0, 4, p, p, p, T, 100, 14, p, 8, p, None) == 1 and b"items" in err()
    assert lib.rsx_tx_item_features(p, 5, 4, p, p, p, T, 100, 14, None, 8, p, None) == 1 and b"null tensor" in err()
    assert lib.rsx_tx_item_features(p, 5, 4, p, p, p, T, 100, 14, p, 7, p, None) == 1 and b"col_sum" in err()
    user = lambda C, ws, nbytes: lib.rsx_tx_user_features(p, p, p, p, p, p, p, p, p, C, 100, ws, nbytes, p, p, p, p, None)  # noqa: E731
    assert user(0, p, 1 << 20) == 1 and b"customers" in err()
    assert user(10, p, 52 * 8 - 1) == 1 and b"workspace" in err()
    assert lib.rsx_tx_user_features(p, p, p, p, p, p, p, None, p, 10, 100, p, 1 << 20, p, p, p, p, None) == 1
    assert b"null tensor" in err()
    assert lib.rsx_quantile_bucket(p, p, 10, 0, p, p, p, None) == 1 and b"q" in err()
    assert lib.rsx_quantile_bucket(p, p, 10, 127, p, p, p, None) == 1 and b"126" in err()
    assert lib.rsx_quantile_bucket(p, p, 0, 10, p, p, p, None) == 1 and b"values" in err()
    assert lib.rsx_quantile_bucket(p, None, 10, 10, p, p, p, None) == 1 and b"null tensor" in err()
    ranks = lambda C, N, nbytes: lib.rsx_tx_sequence_ranks(p, C, T, p, p, p, N, p, nbytes, p, p, p, p, None)  # noqa: E731
    assert ranks(3, 0, 256) == 1 and b"items" in err()
    assert ranks(0, 5, 256) == 1 and b"customers" in err()
    assert ranks(3, 5, 255) == 1 and b"workspace" in err()
    assert lib.rsx_tx_sequences(p, 3, T, p, p, p, p, p, 0, 10, p, p, p, None) == 1 and b"max_len" in err()
    assert lib.rsx_tx_sequences(p, 3, T, p, p, p, p, p, 50, T + 1, p, p, p, None) == 1 and b"n_out" in err()
    assert lib.rsx_tx_sequences(p, 3, T, p, p, p, p, p, 50, 10, None, p, p, None) == 1 and b"n_out" in err()
    assert lib.rsx_tx_sequences(p, 3, T, p, p, p, p, None, 50, 10, p, p, p, None) == 1 and b"null tensor" in err()
