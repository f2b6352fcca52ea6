"""Numpy oracle of the boosted ranker's explanations (a helper, not a test): the specification of
include/recsys_amd.h ("explaining the boosted ranker") restated in float64, on the trees of tests/gbdt_ref.py.

A tree is (splits [(f, b)] per level, values [2^depth]); its leaf weights w [2^depth] count the rows of a data
set per leaf. table[idx] = E(s) for the states s in {0, 1, *}^depth, idx = sum_d s_d 3^(depth-1-d) with * = 2:
Lundberg's path-dependent conditional expectation, a level whose state is * mixing its children by their
covers (1/2 each where both are 0). The players of a tree are its distinct split features; v(S) reads the
table with the levels of the features in S at the row's bits and * elsewhere."""
import itertools
import math

import numpy as np

from tests import gbdt_ref as G

LEAF_STRIDE = 64
TABLE_STRIDE = 729


def clamp_features(splits, F):
    """The splits with a feature outside [0, F) read as feature 0, as the kernels read them."""
    s = np.array(splits, np.int64).copy()
    s[..., 0] = np.where((s[..., 0] < 0) | (s[..., 0] >= F), 0, s[..., 0])
    return s


def row_bits(bins, splits, is_cat):
    """r [depth, R] in {0, 1}: go right per level."""
    return np.stack([G.go_right(bins, int(f), int(b), is_cat).astype(np.int64) for f, b in splits])


def leaf_weights(bins, splits, is_cat):
    """int64 [T, 64] of the trees splits [T, depth, 2] over the rows of bins."""
    T, depth = len(splits), len(splits[0])
    w = np.zeros((T, LEAF_STRIDE), np.int64)
    for t in range(T):
        w[t, :1 << depth] = np.bincount(G.tree_leaves(bins, splits[t], is_cat), minlength=1 << depth)
    return w


def _mix(a, b, c0, c1):
    return (c0 * a + c1 * b) / (c0 + c1) if c0 + c1 > 0 else 0.5 * a + 0.5 * b


def cond_table(values, w, depth):
    """table float64 [3^depth], level by level from the leaves up: level d holds per node the array over the
    states of the levels d .. depth-1, s_d leading."""
    values, w = np.asarray(values, np.float64), np.asarray(w, np.float64)
    cur = [np.array([values[n]]) for n in range(1 << depth)]
    cov = [w[n] for n in range(1 << depth)]
    for d in range(depth - 1, -1, -1):
        cur = [np.concatenate([cur[2 * n], cur[2 * n + 1], _mix(cur[2 * n], cur[2 * n + 1], cov[2 * n], cov[2 * n + 1])])
               for n in range(1 << d)]
        cov = [cov[2 * n] + cov[2 * n + 1] for n in range(1 << d)]
    return cur[0]


def cond_value(values, w, depth, state):
    """E(state) by the recursion itself, no table: state is a sequence over {0, 1, 2 = *}."""
    w = np.asarray(w, np.float64)

    def cover(n, d):
        width = 1 << (depth - d)
        return float(w[n * width:(n + 1) * width].sum())

    def ev(n, d):
        if d == depth:
            return float(values[n])
        if state[d] < 2:
            return ev(2 * n + state[d], d + 1)
        return _mix(ev(2 * n, d + 1), ev(2 * n + 1, d + 1), cover(2 * n, d + 1), cover(2 * n + 1, d + 1))

    return ev(0, 0)


def players(splits):
    """The distinct split features in level order."""
    out = []
    for f, _ in splits:
        if int(f) not in out:
            out.append(int(f))
    return out


def shapley_weight(s, m):
    return math.factorial(s) * math.factorial(m - s - 1) / math.factorial(m)


def _tree_shap(splits, r, F, value_of):
    """phi float64 [F, R] of one tree: r [depth, R] the rows' bits, value_of(state [depth, R]) -> v [R]."""
    depth, R = r.shape
    feats = [int(f) for f, _ in splits]
    U = players(splits)
    m = len(U)
    phi = np.zeros((F, R), np.float64)

    def v(S):
        state = np.stack([r[d] if feats[d] in S else np.full(R, 2, np.int64) for d in range(depth)])
        return value_of(state)

    cache = {S: v(S) for k in range(m + 1) for S in itertools.combinations(U, k)}
    for j in U:
        rest = [u for u in U if u != j]
        for k in range(m):
            for S in itertools.combinations(rest, k):
                with_j = tuple(u for u in U if u in S or u == j)
                phi[j] += shapley_weight(k, m) * (cache[with_j] - cache[S])
    return phi


def tree_shap(splits, values, w, r, F):
    """phi [F, R] from the table."""
    depth = len(splits)
    table = cond_table(values, w, depth)
    p3 = 3 ** np.arange(depth - 1, -1, -1)
    return _tree_shap(splits, r, F, lambda state: table[(state * p3[:, None]).sum(0)])


def tree_shap_brute(splits, values, w, r, F):
    """phi [F, R] with the recursion run once per (coalition, row): no table."""
    depth = len(splits)
    return _tree_shap(splits, r, F, lambda state: np.array([cond_value(values, w, depth, tuple(int(x) for x in state[:, i]))
                                                            for i in range(state.shape[1])]))


def shap(bins, f0, splits, values, is_cat, weights, ntree_end=None):
    """phi float64 [F + 1, R] of the first ntree_end trees: rows 0..F-1 the features, row F the expected value."""
    F, R = bins.shape
    T = len(splits) if ntree_end is None else ntree_end
    phi = np.zeros((F + 1, R), np.float64)
    phi[F] = np.float64(f0)
    for t in range(T):
        sp = clamp_features(splits[t], F)
        depth = len(sp)
        phi[:F] += tree_shap(sp, values[t][:1 << depth], weights[t][:1 << depth], row_bits(bins, sp, is_cat), F)
        phi[F] += cond_table(values[t][:1 << depth], weights[t][:1 << depth], depth)[-1]
    return phi


def level_pvc(values, w, depth):
    """pvc float64 [depth]: per level the sum over the pairs of leaves that differ only in that level's bit."""
    values, w = np.asarray(values, np.float64), np.asarray(w, np.float64)
    out = np.zeros(depth, np.float64)
    for d in range(depth):
        bit = 1 << (depth - 1 - d)
        for l in range(1 << depth):
            if l & bit:
                continue
            c1, c2 = w[l], w[l + bit]
            if c1 + c2 > 0:
                out[d] += c1 * c2 / (c1 + c2) * (values[l] - values[l + bit]) ** 2
    return out


def prediction_values_change(splits, values, weights, F):
    """The importances float64 [F], summing to 100 (all zeros stay zeros)."""
    imp = np.zeros(F, np.float64)
    for t in range(len(splits)):
        sp = clamp_features(splits[t], F)
        depth = len(sp)
        pvc = level_pvc(values[t][:1 << depth], weights[t][:1 << depth], depth)
        for d in range(depth):
            imp[sp[d][0]] += pvc[d]
    total = imp.sum()
    return imp * (100.0 / total) if total > 0 else imp
