"""Numpy oracle of the QuerySoftMax objective of the oblivious-tree model (a helper, not a test): the
specification of include/recsys_amd.h ("QuerySoftMax") restated with int64 sums and float64 scores on top
of tests/gbdt_ref.py (whose histograms, scores, splits and leaf values it reuses), and the group layout
the ranker's tests share.

Objective: rows carry y in {0, 1} and a group id; F0 = 0. Per group q with the float32 approximant a:
m_q = max a_i; E_i = rint(exp(float64(a_i) - float64(m_q)) 2^32) as int64; Z_q = sum E_i; p_i =
float32(E_i / Z_q); S_q = #{y_i = 1}. Per row: S_q = 0 -> g = h = 0, else t = y ? float32(1 / S_q) : 0, g = t -
p, h = p (1 - p) in float32, quantised to rint(x 2^30). Loss: L_q = -(1 / S_q) sum_{y_i = 1} [a_i - m_q -
log(Z_q 2^-32)] in float64, averaged over the groups with a positive. Nothing here depends on the order of
the rows."""
import numpy as np

from tests import gbdt_ref as G

TWO32 = float(2 ** 32)


# ---- the objective --------------------------------------------------------------------------------------
def group_index(gid):
    """(dense group index per row, number of groups): the groups ascending by id."""
    ids, inv = np.unique(np.asarray(gid), return_inverse=True)
    return inv.reshape(-1), len(ids)


def group_sums(F, y, gid):
    """(inv, m float32 [G], E int64 [R], Z int64 [G], S int64 [G])."""
    inv, n = group_index(gid)
    a = np.asarray(F, np.float32)
    m = np.full(n, -np.inf, np.float32)
    np.maximum.at(m, inv, a)
    E = np.rint(np.exp(a.astype(np.float64) - m[inv].astype(np.float64)) * TWO32).astype(np.int64)
    Z = np.zeros(n, np.int64)
    np.add.at(Z, inv, E)
    S = np.zeros(n, np.int64)
    np.add.at(S, inv, (np.asarray(y) == 1).astype(np.int64))
    return inv, m, E, Z, S


def grad_float(F, y, gid):
    """(g, h) float32 per row, in the float32 arithmetic of the kernel."""
    inv, _, E, Z, S = group_sums(F, y, gid)
    p = (E.astype(np.float64) / Z[inv].astype(np.float64)).astype(np.float32)
    live = S[inv] > 0
    t = np.where(np.asarray(y) == 1, (1.0 / np.maximum(S[inv], 1)).astype(np.float32), np.float32(0))
    g = np.where(live, t - p, np.float32(0)).astype(np.float32)
    h = np.where(live, p * (np.float32(1) - p), np.float32(0)).astype(np.float32)
    return g, h


def grad(F, y, gid):
    """(qg, qh) int64 per row."""
    g, h = grad_float(F, y, gid)
    return G.quantise(g), G.quantise(h)


def grad_plain64(F, y, gid):
    """(g, h) in float64 by a loop over the groups: the plain softmax the fixed-point one is checked against."""
    F, y, gid = np.asarray(F, np.float32), np.asarray(y), np.asarray(gid)
    g, h = np.zeros(len(F)), np.zeros(len(F))
    order = np.argsort(gid, kind="stable")
    cuts = np.flatnonzero(np.diff(gid[order])) + 1
    for rows in np.split(order, cuts):
        s = int((y[rows] == 1).sum())
        if s == 0:
            continue
        a = F[rows].astype(np.float64)
        e = np.exp(a - a.max())
        p = e / e.sum()
        g[rows] = (y[rows] == 1) / s - p
        h[rows] = p * (1 - p)
    return g, h


def loss_sum(F, y, gid):
    """(sum of L_q over the groups with a positive, their number)."""
    inv, m, _, Z, S = group_sums(F, y, gid)
    term = np.asarray(F, np.float32).astype(np.float64) - m[inv].astype(np.float64) - np.log(Z[inv].astype(np.float64) / TWO32)
    pos = np.asarray(y) == 1
    L = np.zeros(len(Z), np.float64)
    np.add.at(L, inv[pos], term[pos])
    live = S > 0
    return float(np.sum(-L[live] / S[live])), int(live.sum())


def loss(F, y, gid):
    """The metric QuerySoftMax."""
    s, n = loss_sum(F, y, gid)
    return s / n


# ---- trees ------------------------------------------------------------------------------------------------
def grow_tree(bins, qg, qh, is_cat, n_bins, depth, lr, l2, splits=None):
    """gbdt_ref.grow_tree on given gradients: splits None -> the oracle's own argmax per level, else the given
    [(f, b)] are followed. Returns a dict: splits, best (the oracle's best_split per level on the way),
    values, sums, leaf (per row) and per level gap."""
    leaf = np.zeros(bins.shape[1], np.int64)
    out = {"splits": [], "best": [], "gap": []}
    for d in range(depth):
        S = G.scores(G.histogram(bins, leaf, qg, qh, 1 << d), is_cat, n_bins, l2)
        best = G.best_split(S)
        f, b = best if splits is None else (int(splits[d][0]), int(splits[d][1]))
        out["splits"].append((f, b))
        out["best"].append(best)
        u = np.unique(S[np.isfinite(S)])
        out["gap"].append(float((u[-1] - u[-2]) / abs(u[-1])) if len(u) > 1 else np.inf)
        leaf = 2 * leaf + G.go_right(bins, f, b, is_cat)
    out["sums"], out["values"] = G.leaf_values(leaf, qg, qh, 1 << depth, lr, l2)
    out["leaf"] = leaf
    return out


def fit(bins, y, gid, is_cat, n_bins, iterations, lr=0.05, depth=6, l2=3.0):
    """The whole model from F0 = 0: {"splits" int [T, depth, 2], "values" float32 [T, 2^depth], "approx" (the
    float32 approximant after the last tree), "loss" (the learn QuerySoftMax after every tree), "gap"}."""
    F = np.zeros(bins.shape[1], np.float32)
    model = {"splits": [], "values": [], "loss": [], "gap": []}
    for _ in range(iterations):
        qg, qh = grad(F, y, gid)
        t = grow_tree(bins, qg, qh, is_cat, n_bins, depth, lr, l2)
        F = F + t["values"][t["leaf"]]
        model["splits"].append(t["splits"])
        model["values"].append(t["values"])
        model["loss"].append(loss(F, y, gid))
        model["gap"].append(min(t["gap"]))
    model["splits"] = np.asarray(model["splits"], np.int64)
    model["values"] = np.asarray(model["values"], np.float32)
    model["approx"] = F
    return model


def ndcg(F, y, gid, top=10):
    """Mean NDCG@top over the groups with a positive, ties broken by averaging over the tied positions."""
    inv, n = group_index(gid)
    z, y = np.asarray(F, np.float64), np.asarray(y)
    disc = 1.0 / np.log2(np.arange(top) + 2.0)
    total, live = 0.0, 0
    for q in range(n):
        rows = np.flatnonzero(inv == q)
        pos = int((y[rows] == 1).sum())
        if pos == 0:
            continue
        order = rows[np.argsort(-z[rows], kind="stable")]
        dcg, i = 0.0, 0
        while i < len(order):
            j = i
            while j < len(order) and z[order[j]] == z[order[i]]:
                j += 1
            inside = disc[i:min(j, top)].sum() if i < top else 0.0
            dcg += inside * (y[order[i:j]] == 1).sum() / (j - i)
            i = j
        total += dcg / disc[:min(pos, top)].sum()
        live += 1
    return total / live


# ---- the shared group layout --------------------------------------------------------------------------------
SIZES = (1, 2, 6, 63, 64, 65, 6, 6, 257, 6, 1, 1100)


def layout(R, seed):
    """Group ids int64 [R]: the sizes cycle once through SIZES, then 6s, truncated to R; group k has id 3 k + 5;
    the rows are scattered with default_rng(seed).permutation(R)."""
    sizes = list(SIZES)
    while sum(sizes) < R:
        sizes.append(6)
    ids = np.repeat(3 * np.arange(len(sizes), dtype=np.int64) + 5, sizes)[:R]
    gid = np.empty(R, np.int64)
    gid[np.random.default_rng(seed).permutation(R)] = ids
    return gid


def make_sets():
    """((num, cat, y, gid) of the train rows, the same of the validation rows): gbdt_ref.make(4096, 1) with
    layout seed 7 and make(2048, 2) with seed 8."""
    return G.make(4096, 1) + (layout(4096, 7),), G.make(2048, 2) + (layout(2048, 8),)
