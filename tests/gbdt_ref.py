"""Numpy oracle of the oblivious-tree boosting model (a helper, not a test): the specification of
include/recsys_amd.h ("oblivious-tree boosting") restated with int64 histograms and float64 scores, and
the data generator the GBDT tests share.

Model: bins uint8 [F, R]; F0 = log(p / (1 - p)) of the base rate; per tree g = y - sigmoid(F), h =
sigmoid(F)(1 - sigmoid(F)) in float32, quantised to rint(x 2^30) (half to even) as int64; per level the
int64 histogram H[leaf, f, bin, {g, h}], the candidate (f, b) sending bin > b (numeric) or bin == b
(categorical) right, its score the sum over the leaves of G_L^2 / (H_L + l2) + G_R^2 / (H_R + l2) in
float64 with G = sum * 2^-30, the argmax with ties to the lowest f, then the lowest b; leaf = 2 leaf +
right; leaf value float32(lr * (G / (H + l2))); F += value[leaf] in float32."""
import numpy as np

SCALE = float(2 ** 30)
BINS = 256


# ---- borders and bins ---------------------------------------------------------------------------------
def build_borders(x, border_count=254):
    """The float32 borders of the column x: the midpoints a/2 + b/2 (float32) of consecutive distinct
    non-NaN values; when there are more than border_count of them, those at the ranks
    ((2 j + 1) (m - 1)) // (2 border_count), j < border_count, of the m - 1 midpoints."""
    x = np.asarray(x, np.float32)
    v = np.unique(x[~np.isnan(x)])
    m = len(v)
    if m < 2:
        return np.zeros(0, np.float32)
    mids = (v[:-1] * np.float32(0.5) + v[1:] * np.float32(0.5)).astype(np.float32)
    if m - 1 <= border_count:
        return mids
    j = np.arange(border_count, dtype=np.int64)
    return mids[((2 * j + 1) * (m - 1)) // (2 * border_count)]


def bin_column(x, borders):
    """bin = #{borders < x}; NaN -> 0."""
    x = np.asarray(x, np.float32)
    b = np.searchsorted(borders, x, side="left")
    return np.where(np.isnan(x), 0, b).astype(np.uint8)


# ---- one tree -----------------------------------------------------------------------------------------
def sigmoid64(F):
    return 1.0 / (1.0 + np.exp(-np.asarray(F, np.float64)))


def grad(F, y):
    """(qg, qh) int64 of the float32 approximant F and the labels y: the float32 arithmetic of the kernel
    (the sigmoid itself from float64, rounded once)."""
    p = sigmoid64(F).astype(np.float32)
    g = np.asarray(y, np.float32) - p
    h = p * (np.float32(1) - p)
    return quantise(g), quantise(h)


def quantise(x):
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * SCALE).astype(np.int64)


def histogram(bins, leaf, qg, qh, n_leaves):
    """H int64 [n_leaves, F, 256, 2] by np.add.at."""
    F, R = bins.shape
    H = np.zeros((n_leaves, F, BINS, 2), np.int64)
    leaf = np.asarray(leaf, np.int64)
    for f in range(F):
        np.add.at(H[:, f, :, 0], (leaf, bins[f].astype(np.int64)), qg)
        np.add.at(H[:, f, :, 1], (leaf, bins[f].astype(np.int64)), qh)
    return H


def scores(H, is_cat, n_bins, l2):
    """S float64 [F, 256]: the score of every candidate (f, b), -inf for b >= n_bins[f]."""
    G, Hh = H[..., 0], H[..., 1]
    is_cat = np.asarray(is_cat, bool)[None, :, None]
    S = np.zeros(G.shape[1:], np.float64)
    for l in range(H.shape[0]):
        term = 0.0
        sides = []
        for A in (G[l], Hh[l]):
            tot = A.sum(-1, keepdims=True)
            right = np.where(is_cat[0], A, tot - np.cumsum(A, -1))
            sides.append((tot - right, right))
        for side in (0, 1):
            g = sides[0][side].astype(np.float64) / SCALE
            h = sides[1][side].astype(np.float64) / SCALE
            term = term + g * g / (h + l2)
        S += term
    b = np.arange(BINS)[None, :]
    return np.where(b < np.asarray(n_bins)[:, None], S, -np.inf)


def best_split(S):
    """(f, b) of the first maximum of S in (f, b) order."""
    f, b = np.unravel_index(int(np.argmax(S)), S.shape)
    return int(f), int(b)


def go_right(bins, f, b, is_cat):
    return (bins[f] == b) if is_cat[f] else (bins[f] > b)


def leaf_values(leaf, qg, qh, n_leaves, lr, l2):
    """(sums int64 [n_leaves, 2], values float32 [n_leaves]) of the final leaves."""
    sums = np.zeros((n_leaves, 2), np.int64)
    np.add.at(sums[:, 0], leaf, qg)
    np.add.at(sums[:, 1], leaf, qh)
    g, h = sums[:, 0].astype(np.float64) / SCALE, sums[:, 1].astype(np.float64) / SCALE
    return sums, (lr * (g / (h + l2))).astype(np.float32)


def grow_tree(bins, F, y, is_cat, n_bins, depth, lr, l2, splits=None):
    """One tree on the float32 approximant F. splits None: the oracle's own argmax per level; else the
    given [(f, b)] are followed. Returns a dict: splits, values, sums, leaf (per row), and per level
    max_score, chosen_score and gap."""
    qg, qh = grad(F, y)
    leaf = np.zeros(bins.shape[1], np.int64)
    out = {"splits": [], "max_score": [], "chosen_score": [], "gap": []}
    for d in range(depth):
        S = scores(histogram(bins, leaf, qg, qh, 1 << d), is_cat, n_bins, l2)
        f, b = best_split(S) if splits is None else (int(splits[d][0]), int(splits[d][1]))
        out["splits"].append((f, b))
        out["max_score"].append(float(S.max()))
        out["chosen_score"].append(float(S[f, b]))
        u = np.unique(S[np.isfinite(S)])     # gap: how far the best distinct score is above the second
        out["gap"].append(float((u[-1] - u[-2]) / abs(u[-1])) if len(u) > 1 else np.inf)
        leaf = 2 * leaf + go_right(bins, f, b, is_cat)
    out["sums"], out["values"] = leaf_values(leaf, qg, qh, 1 << depth, lr, l2)
    out["leaf"] = leaf
    return out


def base_logit(y):
    p = float(np.mean(np.asarray(y, np.float64)))
    return np.float32(np.log(p / (1.0 - p)))


def fit(bins, y, is_cat, n_bins, iterations, lr=0.05, depth=6, l2=3.0):
    """The whole model: {"f0", "splits" int [T, depth, 2], "values" float32 [T, 2^depth], "approx": the
    float32 training approximant after every tree}."""
    f0 = base_logit(y)
    F = np.full(bins.shape[1], f0, np.float32)
    model = {"f0": f0, "splits": [], "values": [], "approx": [], "gap": []}
    for _ in range(iterations):
        t = grow_tree(bins, F, y, is_cat, n_bins, depth, lr, l2)
        F = F + t["values"][t["leaf"]]
        model["splits"].append(t["splits"])
        model["values"].append(t["values"])
        model["approx"].append(F.copy())
        model["gap"].append(min(t["gap"]))
    model["splits"] = np.asarray(model["splits"], np.int64)
    model["values"] = np.asarray(model["values"], np.float32)
    return model


def tree_leaves(bins, splits, is_cat):
    leaf = np.zeros(bins.shape[1], np.int64)
    for f, b in splits:
        leaf = 2 * leaf + go_right(bins, int(f), int(b), is_cat)
    return leaf


def predict(bins, f0, splits, values, is_cat, ntree_end=None):
    """(float64 sum, float32 sequential sum, bound) of F0 and the first ntree_end trees' leaf values; bound
    = |F0| + sum_t max |leaf_t|."""
    T = len(splits) if ntree_end is None else ntree_end
    s64 = np.full(bins.shape[1], np.float64(f0))
    s32 = np.full(bins.shape[1], np.float32(f0))
    bound = abs(float(f0))
    for t in range(T):
        v = np.asarray(values[t], np.float32)[tree_leaves(bins, splits[t], is_cat)]
        s64 += v.astype(np.float64)
        s32 = s32 + v
        bound += float(np.max(np.abs(values[t])))
    return s64, s32, bound


def logloss(F, y):
    z = np.asarray(F, np.float64)
    y = np.asarray(y, np.float64)
    return float(np.mean(np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))))


def auc(F, y):
    """Tie-aware ROC-AUC in exact integers."""
    z = np.asarray(F, np.float64)
    y = np.asarray(y) > 0.5
    pos, neg = np.sort(z[y]), np.sort(z[~y])
    u2 = int(np.searchsorted(neg, pos, side="left").sum()) + int(np.searchsorted(neg, pos, side="right").sum())
    return u2 / (2 * len(pos) * len(neg))


# ---- shared data --------------------------------------------------------------------------------------
CARDS = (4, 3, 40, 12, 5)
N_NUM = 7
_EFF = (0.8 * np.random.default_rng(91).standard_normal(40)).astype(np.float64)


def make(R, seed):
    """(num float32 [R, 7], cat int64 [R, 5], y float32 [R]): seven standard-normal columns (column 3
    rounded to halves, column 6 a copy of column 0), five categorical columns of cardinality 4, 3, 40, 12,
    5, z = 1.2 x0 - 0.8 [x1 > 0.3] + 0.6 x2 [c0 == 2] + eff[c2] - 1.6, y ~ Bernoulli(sigmoid(z))."""
    rng = np.random.default_rng(seed)
    num = rng.standard_normal((R, N_NUM)).astype(np.float32)
    num[:, 3] = np.round(num[:, 3] * 2) / 2
    num[:, 6] = num[:, 0]
    cat = np.stack([rng.integers(0, c, R) for c in CARDS], axis=1).astype(np.int64)
    z = (1.2 * num[:, 0].astype(np.float64) - 0.8 * (num[:, 1] > 0.3) + 0.6 * num[:, 2] * (cat[:, 0] == 2)
         + _EFF[cat[:, 2]] - 1.6)
    y = (rng.random(R) < sigmoid64(z)).astype(np.float32)
    return num, cat, y


def bin_data(num, cat, borders=None):
    """(bins uint8 [12, R], is_cat, n_bins, borders): numeric columns first, then the categorical codes as
    they are. borders None: built from num (training rows)."""
    if borders is None:
        borders = [build_borders(num[:, j]) for j in range(num.shape[1])]
    rows = [bin_column(num[:, j], borders[j]) for j in range(num.shape[1])]
    rows += [cat[:, j].astype(np.uint8) for j in range(cat.shape[1])]
    is_cat = np.array([0] * num.shape[1] + [1] * cat.shape[1], np.uint8)
    n_bins = np.array([255] * num.shape[1] + [int(c) for c in CARDS[:cat.shape[1]]], np.int32)
    return np.stack(rows), is_cat, n_bins, borders
