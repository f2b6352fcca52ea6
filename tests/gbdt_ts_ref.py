"""Numpy oracle of the ordered target statistics (a helper, not a test): the specification of
include/recsys_amd.h ("ordered target statistics") restated with integer counts and float64 arithmetic, and
the data the TS tests share.

One TS column: codes c_i in [0, V], labels y_i in {0, 1}, rows in the caller's order. k_i = hash_u32(seed +
column, i); row j precedes row i iff (k_j, j) < (k_i, i). n_i, s_i count the preceding rows of the same code and
their positives: ts_i = float32((s_i + ap) / (n_i + a)) in float64 with ap = a * p formed once; table[c] =
float32((S_c + ap) / (N_c + a)) over the totals, the prior value float32(ap / a) for a code nobody had."""
import numpy as np

from tests import gbdt_ref as G
from tests.ranker_rows_ref import hash_u32

PRIOR = (0.5, 1.0)


def hashes(seed, column, R):
    """k_i of the R rows of TS column `column`: uint32 values as int64."""
    return hash_u32(int(seed) + int(column), np.arange(R, dtype=np.int64))


def precedence(seed, column, R):
    """The rows in the order of the definition: ascending (k_i, i)."""
    return np.lexsort((np.arange(R), hashes(seed, column, R)))


def sort_key_order(codes, k):
    """The rows in the order the device walks: a stable sort of c_i << 32 | k_i."""
    return np.argsort((np.asarray(codes, np.int64) << 32) | np.asarray(k, np.int64), kind="stable")


def value(s, n, prior=PRIOR):
    p, a = float(prior[0]), float(prior[1])
    ap = a * p
    return ((np.asarray(s, np.float64) + ap) / (np.asarray(n, np.float64) + a)).astype(np.float32)


def ordered_ts(codes, y, V, seed=0, column=0, prior=PRIOR):
    """(ts float32 [R], totals int64 [V + 1, 2] = (N_c, S_c), table float32 [V + 1]) of one column: the rows
    visited in the order of the definition with one pair of counters per code."""
    codes = np.asarray(codes, np.int64)
    pos = np.asarray(y) == 1
    R = len(codes)
    totals = np.zeros((V + 1, 2), np.int64)
    n, s = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for i in precedence(seed, column, R):
        c = codes[i]
        n[i], s[i] = totals[c]
        totals[c, 0] += 1
        totals[c, 1] += int(pos[i])
    return value(s, n, prior), totals, value(totals[:, 1], totals[:, 0], prior)


def brute_force(codes, y, seed=0, column=0, prior=PRIOR):
    """ts by the O(R^2) double loop over the definition."""
    codes = np.asarray(codes, np.int64)
    R = len(codes)
    k = hashes(seed, column, R)
    n, s = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for i in range(R):
        for j in range(R):
            if codes[j] == codes[i] and (k[j], j) < (k[i], i):
                n[i] += 1
                s[i] += int(y[j] == 1)
    return value(s, n, prior)


def serve(codes, table):
    """The served value of every code: table[c], table[0] for a code outside [0, V]."""
    codes = np.asarray(codes, np.int64)
    return table[np.where((codes < 0) | (codes >= len(table)), 0, codes)]


# ---- the model with TS columns ----------------------------------------------------------------------------
def bin_data(num, cat, y, one_hot_max_size, seed=0, prior=PRIOR, fitted=None):
    """gbdt_ref.bin_data with the categorical columns of more than one_hot_max_size known values (the largest
    code) as TS columns: (bins uint8 [F, R], is_cat, n_bins, fitted), the columns in the model's internal order
    numeric, TS, one-hot. fitted None: the training rows (ordered values, borders built from them); else the
    dict a training call returned, for served rows (table values under the training borders)."""
    train = fitted is None
    if train:
        known = [int(cat[:, k].max()) for k in range(cat.shape[1])]
        ts_cols = [k for k, v in enumerate(known) if v > one_hot_max_size]
        fitted = {"borders": [G.build_borders(num[:, j]) for j in range(num.shape[1])], "ts_cols": ts_cols,
                  "known": known, "tables": [], "totals": [], "ts_borders": []}
    rows = [G.bin_column(num[:, j], fitted["borders"][j]) for j in range(num.shape[1])]
    for j, k in enumerate(fitted["ts_cols"]):
        if train:
            ts, totals, table = ordered_ts(cat[:, k], y, fitted["known"][k], seed, j, prior)
            fitted["tables"].append(table)
            fitted["totals"].append(totals)
            fitted["ts_borders"].append(G.build_borders(ts))
        else:
            ts = serve(cat[:, k], fitted["tables"][j])
        rows.append(G.bin_column(ts, fitted["ts_borders"][j]))
    one_hot = [k for k in range(cat.shape[1]) if k not in fitted["ts_cols"]]
    rows += [cat[:, k].astype(np.uint8) for k in one_hot]
    n_ts = num.shape[1] + len(fitted["ts_cols"])
    is_cat = np.array([0] * n_ts + [1] * len(one_hot), np.uint8)
    n_bins = np.array([255] * n_ts + [fitted["known"][k] + 1 for k in one_hot], np.int32)
    return np.stack(rows), is_cat, n_bins, fitted


WIDE = 1000
_WIDE_EFF = (1.5 * np.random.default_rng(92).standard_normal(WIDE + 1)).astype(np.float64)


def make(R, seed):
    """gbdt_ref.make(R, seed) plus a sixth categorical column of codes in [1, 1000] that carries signal: (num
    float32 [R, 7], cat int64 [R, 6], y float32 [R]), z = gbdt_ref's z + eff[c5]."""
    num, cat, _ = G.make(R, seed)
    rng = np.random.default_rng(1000 + seed)
    wide = rng.integers(1, WIDE + 1, R)
    if R >= WIDE:
        wide[:WIDE] = np.arange(1, WIDE + 1)       # every value known: the largest code is 1000
    z = (1.2 * num[:, 0].astype(np.float64) - 0.8 * (num[:, 1] > 0.3) + 0.6 * num[:, 2] * (cat[:, 0] == 2)
         + G._EFF[cat[:, 2]] + _WIDE_EFF[wide] - 1.6)
    y = (rng.random(R) < G.sigmoid64(z)).astype(np.float32)
    return num, np.concatenate([cat, wide[:, None]], axis=1).astype(np.int64), y
