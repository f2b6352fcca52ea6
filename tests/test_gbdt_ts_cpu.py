"""CPU checks of the ordered target statistics: the oracle tests/gbdt_ts_ref.py against a brute-force double
loop and against its own definition at the edges, the sort-key route the device takes against the (hash, row)
order of the specification, the two native entry points' ABI (arity; argument checks that return before any
launch), and what the encoding is for: a 1000-value column that carries signal lifts the held-out AUC."""
import os
import re

import numpy as np
import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native
from tests import gbdt_ref as G
from tests import gbdt_ts_ref as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _column(R, V, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, V + 1, R), (rng.random(R) < 0.4).astype(np.float32)


def test_the_oracle_equals_the_brute_force_double_loop():
    codes, y = _column(300, 7, 0)
    for seed, prior in ((0, TS.PRIOR), (12345, (0.3, 2.5))):
        ts, totals, _ = TS.ordered_ts(codes, y, 7, seed=seed, prior=prior)
        assert ts.dtype == np.float32 and np.array_equal(ts, TS.brute_force(codes, y, seed=seed, prior=prior))
        assert np.array_equal(totals[:, 0], np.bincount(codes, minlength=8))
        assert np.array_equal(totals[:, 1], np.bincount(codes, weights=y, minlength=8).astype(np.int64))
    assert len(np.unique(ts)) > 20                    # a statistic, not a constant


def test_distinct_codes_leak_no_label():
    R = 500
    codes = np.random.default_rng(1).permutation(R)
    for y in (np.ones(R, np.float32), np.zeros(R, np.float32)):
        ts, _, table = TS.ordered_ts(codes, y, R - 1)
        assert np.all(ts == np.float32(0.5))          # every row is the first of its code: exactly p
        assert np.all(table == np.float32((y[0] + 0.5) / 2.0))
    ts, _, _ = TS.ordered_ts(codes, np.ones(R, np.float32), R - 1, prior=(0.25, 3.0))
    assert np.all(ts == np.float32(0.25))


def test_the_table_is_the_totals_formula_and_an_unused_code_gets_p():
    codes, y = _column(400, 9, 2)
    codes[codes == 4] = 5                             # nobody has code 4
    p, a = 0.3, 2.0
    _, totals, table = TS.ordered_ts(codes, y, 9, prior=(p, a))
    for c in range(10):
        N, S = int((codes == c).sum()), int(y[codes == c].sum())
        assert (totals[c, 0], totals[c, 1]) == (N, S)
        assert table[c] == np.float32((S + a * p) / (N + a))
    assert totals[4].tolist() == [0, 0] and table[4] == np.float32(p)
    assert np.array_equal(TS.serve([3, -1, 10, 4], table), table[[3, 0, 0, 4]])


def test_a_second_column_uses_the_next_seed():
    codes, y = _column(300, 5, 3)
    first = TS.ordered_ts(codes, y, 5, seed=7, column=0)[0]
    second = TS.ordered_ts(codes, y, 5, seed=7, column=1)[0]
    assert np.array_equal(second, TS.ordered_ts(codes, y, 5, seed=8, column=0)[0])
    assert not np.array_equal(first, second)


def test_the_sort_key_route_gives_the_order_of_the_definition():
    """hash_u32 ends in murmur3's finaliser, a bijection of 32-bit words, and for a row index below 2^32 it
    starts from index ^ (a function of the seed): two rows of one column never hash alike, and a search over
    the hash finds no pair (checked here on 2^18 rows under three seeds). The tie-break by the row index is
    therefore exercised with two hashes made equal by hand: the stable sort of the keys must still give the
    (hash, row) order of the definition."""
    for seed in (0, 7, 2 ** 40 + 3):
        assert len(np.unique(TS.hashes(seed, 0, 1 << 18))) == 1 << 18
    seed, R, i, j = 5, 3000, 1234, 2345
    codes, y = _column(R, 7, 4)
    k = TS.hashes(seed, 0, R)
    assert np.array_equal(TS.sort_key_order(codes, k), np.lexsort((np.arange(R), k, codes)))
    forced = k.copy()
    forced[[i, j]] = max(k[i], k[j])
    codes[i] = codes[j] = 3
    order = TS.sort_key_order(codes, forced)
    assert np.array_equal(order, np.lexsort((np.arange(R), forced, codes)))   # by code, inside a code by (k, row)
    where = np.empty(R, np.int64)
    where[order] = np.arange(R)
    assert where[j] == where[i] + 1                                           # the tie falls to the row index
    order = TS.sort_key_order(codes, k)
    # the statistic along that order: cumulative counts minus the count at each run's start
    c_sorted, pos = codes[order], (y[order] == 1).astype(np.int64)
    start = np.nonzero(np.r_[True, c_sorted[1:] != c_sorted[:-1]])[0]
    run = np.repeat(start, np.diff(np.r_[start, R]))
    ones, hits = np.arange(R), np.cumsum(pos) - pos
    ts = np.empty(R, np.float32)
    ts[order] = TS.value(hits - hits[run], ones - ones[run])
    assert np.array_equal(ts, TS.ordered_ts(codes, y, 7, seed=seed)[0])


def test_the_native_entry_points_have_the_headers_arity_and_reject_bad_arguments_without_a_gpu():
    text = open(os.path.join(ROOT, "include", "recsys_amd.h")).read()
    for name in ("rsx_gbdt_ts_keys", "rsx_gbdt_ordered_ts"):
        m = re.search(r"^int\s+" + name + r"\(([^;]*?)\);", text, flags=re.M | re.S)
        assert m, name
        assert len(_native._SIGS[name][1]) == m.group(1).count(",") + 1, name
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.load()
    p = 16
    assert lib.rsx_gbdt_ts_keys(None, 10, 1, 0, p, None) == 1 and b"null tensor" in lib.rsx_last_error()
    assert lib.rsx_gbdt_ts_keys(p, 1 << 31, 1, 0, p, None) == 1 and b"2^31" in lib.rsx_last_error()
    assert lib.rsx_gbdt_ts_keys(p, 10, 33, 0, p, None) == 1
    ok = dict(R=10, Fts=1, Vmax=5, ap=0.5, a=1.0)

    def call(flag=p, ts=p, **kw):
        v = dict(ok, **kw)
        return lib.rsx_gbdt_ordered_ts(p, p, p, p, v["R"], v["Fts"], v["Vmax"], v["ap"], v["a"], p, 1 << 20, ts, p, p, flag, None)

    assert call(ts=None) == 1 and b"null tensor" in lib.rsx_last_error()
    assert call(flag=None) == 1 and b"null tensor" in lib.rsx_last_error()
    assert call(R=1 << 31) == 1 and b"2^31" in lib.rsx_last_error()
    assert call(R=0) == 1
    assert call(Vmax=(1 << 22) + 1) == 1 and b"GBDT_TS_MAX_CODES" in lib.rsx_last_error()
    assert call(a=0.0) == 1 and b"a > 0" in lib.rsx_last_error()
    assert call(a=-1.0) == 1
    assert call(a=float("nan")) == 1
    assert lib.rsx_gbdt_ordered_ts(p, p, p, p, 1000, 2, 5, 0.5, 1.0, p, 16 * 2 * 4 - 1, p, p, p, p, None) == 1
    assert b"workspace" in lib.rsx_last_error()


def test_a_wide_column_that_carries_signal_lifts_the_held_out_auc():
    """20 oracle trees on TS.make(4096, 1), scored on make(2048, 2): with the 1000-value column (and the
    40-value one) as TS columns against the same fit without the wide column. On the CPU the oracle gives AUC
    0.7840 with it and 0.7379 without, 0.046 apart; the test asks for 0.02, under half of that margin. The
    device test demands the oracle's trees exactly and so needs no threshold of its own."""
    tr, va = TS.make(4096, 1), TS.make(2048, 2)
    out = {}
    for name, cols in (("with", slice(None)), ("without", slice(0, 5))):
        bins, is_cat, n_bins, fitted = TS.bin_data(tr[0], tr[1][:, cols], tr[2], 16)
        model = G.fit(bins, tr[2], is_cat, n_bins, 20)
        bins_v = TS.bin_data(va[0], va[1][:, cols], None, 16, fitted=fitted)[0]
        out[name] = G.auc(G.predict(bins_v, model["f0"], model["splits"], model["values"], is_cat)[0], va[2])
    print(f"held-out AUC with the wide column {out['with']:.4f}, without {out['without']:.4f}")
    assert out["with"] > out["without"] + 0.02
