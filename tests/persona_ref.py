"""The oracle of the persona tests, all float64; nothing here imports the package.

Features: the reference's staticstics/preprocess_clustering.py restated with the same pandas / scipy calls (groupby,
value_counts, scipy.stats.entropy), with the two stated definitions of the project made explicit: prices are the
log's float32 values held as float64, and the head items of long_tail_ratio are the first max(int(0.2 N), 1) items by
count descending, ties by ascending item index (pandas' value_counts leaves ties in an order that is neither). The
closed forms the device uses (ln n - sum n_c ln n_c / n; repeated / n) are restated beside them.

k-means: Lloyd's algorithm in numpy on the quantised integers q (the data are q 2^-frac_bits exactly), as
include/recsys_amd.h ("k-means") specifies it: the squared distance accumulates over j ascending from 0, subtraction
first, product and sum rounded separately; the label is the first minimum; a centre is float(sum_q) / (count
2^frac_bits) from integer sums; the shift is summed sequentially, k outer, j inner; the fit stops at the first
iteration with no changed label or shift <= tol_abs. The seeding is k-means++ as an exponential race over the
library's hash (tests/dropout_ref.py)."""
import json
import math

import numpy as np
import pandas as pd
from scipy.stats import entropy

from tests import dropout_ref as DR
from tests import tx_features_ref as TR

COLS = ["basket_size", "avg_price", "cat_entropy", "long_tail_ratio", "weekend_ratio", "repurchase_rate",
        "relative_price_pos"]


# ---- features ------------------------------------------------------------------------------------------------------------
def head_items(article_ids):
    """The head set: count descending, ties by ascending item index (= ascending id string)."""
    counts = pd.Series(article_ids).value_counts()
    order = sorted(counts.index, key=lambda a: (-counts[a], a))
    return set(order[:max(int(len(counts) * 0.2), 1)])


def features(df):
    """The seven columns per customer, ascending customer_id, by the reference's pandas calls."""
    d = pd.DataFrame({"customer_id": np.asarray(df["customer_id"]).astype(str),
                      "article_id": np.asarray(df["article_id"]).astype(str),
                      "price": df["price"].to_numpy(dtype=np.float32).astype(np.float64),
                      "t_dat": pd.to_datetime(df["t_dat"])})
    d["category_code"] = d["article_id"].str[:3]
    g = d.groupby("customer_id")
    out = g["article_id"].count().rename("basket_size").astype(np.float64).to_frame()
    out["avg_price"] = g["price"].mean()
    out["cat_entropy"] = g["category_code"].apply(lambda x: entropy(x.value_counts()))
    head = head_items(d["article_id"])
    d["is_tail"] = d["article_id"].apply(lambda x: 1 if x not in head else 0)
    out["long_tail_ratio"] = d.groupby("customer_id")["is_tail"].mean()
    d["is_weekend"] = (d["t_dat"].dt.dayofweek >= 5).astype(int)
    out["weekend_ratio"] = d.groupby("customer_id")["is_weekend"].mean()

    def repurchase(x):
        counts = x.value_counts()
        return counts[counts > 1].sum() / counts.sum()
    out["repurchase_rate"] = g["article_id"].apply(repurchase)
    cat_avg = d.groupby("category_code")["price"].mean().to_dict()
    d["rel"] = d["price"] / d["category_code"].map(cat_avg)
    out["relative_price_pos"] = d.groupby("customer_id")["rel"].mean()
    return out.reset_index()[["customer_id"] + COLS]


def run_lengths(val):
    """The lengths of the runs of equal values of a sorted sequence, in order."""
    val = np.asarray(val)
    if len(val) == 0:
        return np.zeros(0, dtype=np.int64)
    starts = np.flatnonzero(np.concatenate([[True], val[1:] != val[:-1]]))
    return np.diff(np.concatenate([starts, [len(val)]]))


def segment_runs(off, val):
    """(runs, repeated, nlogn) per segment [off[s], off[s + 1]) of val, sorted inside every segment."""
    S = len(off) - 1
    runs, rep, nlogn = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S)
    for s in range(S):
        n = run_lengths(val[off[s]:off[s + 1]])
        runs[s], rep[s] = len(n), n[n > 1].sum()
        nlogn[s] = math.fsum(float(m) * math.log(float(m)) for m in n)
    return runs, rep, nlogn


def entropy_closed_form(n, nlogn, runs):
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.asarray(runs) > 1, np.log(n) - nlogn / n, 0.0)


def segment_sum_f64(off, x, perm=None):
    """(count, exact sum, exact two-pass m2) per segment."""
    x = np.asarray(x, dtype=np.float64)
    S = len(off) - 1
    cnt, tot, m2 = np.zeros(S, np.int64), np.zeros(S), np.zeros(S)
    for s in range(S):
        rows = np.arange(off[s], off[s + 1])
        if perm is not None:
            rows = np.asarray(perm)[rows]
        if len(rows) == 0:
            continue
        v = x[rows]
        cnt[s], tot[s] = len(rows), math.fsum(v)
        m2[s] = math.fsum((v - tot[s] / len(rows)) ** 2)
    return cnt, tot, m2


# ---- standardise / quantise --------------------------------------------------------------------------------------------
def standardize(X):
    """X [d, C] -> ((X - mean) / scale, mean, scale, var): population variance, two passes, exact sums; scale 1 for a
    constant column by scikit-learn's rule var <= C eps var + (C mean eps)^2."""
    X = np.asarray(X, dtype=np.float64)
    C = X.shape[1]
    mean = np.asarray([math.fsum(r) / C for r in X])
    var = np.asarray([math.fsum((r - m) ** 2) / C for r, m in zip(X, mean)])
    eps = np.finfo(np.float64).eps
    constant = var <= C * eps * var + (C * mean * eps) ** 2
    scale = np.where(constant, 1.0, np.sqrt(var))
    return (X - mean[:, None]) / scale[:, None], mean, scale, var


def frac_bits(X):
    m = float(np.abs(X).max())
    return 20 if m == 0.0 else min(20, 30 - math.ceil(math.log2(m)))


def quantize(X, bits):
    """q = rint(X 2^bits) as int64 (ties to even)."""
    return np.rint(np.asarray(X, dtype=np.float64) * 2.0 ** bits).astype(np.int64)


# ---- k-means on the grid -------------------------------------------------------------------------------------------------
def distances(q, bits, centres):
    """D [C, K] for q int [d, C] and centres [K, d]: j ascending, acc = acc + diff * diff."""
    x = q.astype(np.float64) * 2.0 ** -bits
    acc = np.zeros((q.shape[1], len(centres)))
    for j in range(q.shape[0]):
        diff = x[j][:, None] - centres[None, :, j]
        acc = acc + diff * diff
    return acc


def assign(q, bits, centres):
    D = distances(q, bits, centres)
    labels = D.argmin(axis=1)                      # the first minimum
    return labels, D[np.arange(len(labels)), labels]


def lloyd(q, bits, centres, tol_abs=0.0, max_iter=300):
    """-> (centres [K, d], labels [C], dmin [C], n_iter, counts [K] under the final labels)."""
    q = np.asarray(q, dtype=np.int64)
    centres = np.array(centres, dtype=np.float64)
    K, d = centres.shape
    labels = np.full(q.shape[1], -1)
    n_iter = max_iter
    for it in range(1, max_iter + 1):
        new_labels, _ = assign(q, bits, centres)
        changed = int((new_labels != labels).sum())
        labels = new_labels
        new = centres.copy()
        for k in range(K):
            rows = labels == k
            n = int(rows.sum())
            if n:
                new[k] = q[:, rows].sum(axis=1).astype(np.float64) / (float(n) * 2.0 ** bits)
        shift = 0.0
        for v in (new - centres).ravel():          # k outer, j inner
            v = float(v)
            shift = shift + v * v
        centres = new
        if changed == 0 or shift <= tol_abs:
            n_iter = it
            break
    labels, dmin = assign(q, bits, centres)
    return centres, labels, dmin, n_iter, np.bincount(labels, minlength=K)


def seed_round(q, bits, seed, r, prev_row, dmin=None):
    """Round r >= 1 of the seeding after prev_row was chosen in round r - 1: (dmin [C], key [C])."""
    q = np.asarray(q, dtype=np.int64)
    C = q.shape[1]
    x = q.astype(np.float64) * 2.0 ** -bits
    D = distances(q, bits, x[:, prev_row][None, :])[:, 0]
    dmin = D if dmin is None else np.minimum(dmin, D)
    u = (DR.hash_u32(seed + r, np.arange(C)).astype(np.float64) + 0.5) * 2.0 ** -32
    return dmin, dmin / -np.log(u)


def seeds(q, bits, K, seed):
    """The K seed rows: hash_u32(seed, 0) mod C, then the largest key of every round, the lowest row on ties."""
    C = np.asarray(q).shape[1]
    chosen, dmin = [int(DR.hash_u32(seed, [0])[0]) % C], None
    for r in range(1, K):
        dmin, key = seed_round(q, bits, seed, r, chosen[-1], dmin)
        chosen.append(int(np.argmax(key)))
    return np.asarray(chosen)


def blobs(C, K, d, seed, spacing=8.0, sigma=0.5):
    """C points around K distinct centres on a lattice of the given spacing, each centre with at least one point:
    (X [d, C], the planted labels).

    The centres are random points of {0 .. 16 K - 1}^d. k-means++ draws a row in proportion to its squared distance
    to the nearest seed, so with w = 2 d sigma^2 the squared distance inside a blob and s the one between two
    centres, round r of K lands in a blob that already has a seed with probability about r w / ((K - r) s), about
    (w / s) K ln K over a seeding. A lattice as small as K^(1/d) points a side leaves s / w near 100 and one seeding
    in five at K = 20 misses a blob, which no Lloyd iteration repairs; here s / w is above 10^4 even for the
    closest pair of centres, so that the planted partition is what a correct seeding and fit must return."""
    rng = np.random.default_rng(seed)
    side = 16 * K
    cells = np.zeros((0, d), dtype=np.int64)
    while len(cells) < K:                          # distinct lattice points
        cells = np.unique(np.concatenate([cells, rng.integers(0, side, (K, d))]), axis=0)
    centres = cells[rng.permutation(len(cells))[:K]].astype(np.float64) * spacing
    planted = np.concatenate([np.arange(K), rng.integers(0, K, C - K)]) if C >= K else np.arange(C)
    planted = planted[rng.permutation(len(planted))]
    return (centres[planted] + sigma * rng.standard_normal((len(planted), d))).T.copy(), planted


def same_partition(a, b):
    """ARI = 1: the two labelings are the same partition."""
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ---- personas --------------------------------------------------------------------------------------------------------------
def persona_json(user_features, labels):
    """The reference's loop (:141-202), verbatim in its logic, over a features frame and cluster ids."""
    uf = user_features.copy()
    uf["cluster_id"] = np.asarray(labels)
    global_means = uf[COLS].mean()
    out = []
    for cluster_id in sorted(uf["cluster_id"].unique()):
        sub = uf[uf["cluster_id"] == cluster_id]
        stats = {col: round(sub[col].mean(), 2) for col in COLS}
        basket_std = round(sub["basket_size"].std(), 2)
        if pd.isna(basket_std):
            basket_std = 0.0
        desc = []
        if stats["weekend_ratio"] > 0.6:
            desc.append("Weekend_Shopper")
        elif stats["weekend_ratio"] < 0.3:
            desc.append("Weekday_Shopper")
        if stats["repurchase_rate"] > 0.3:
            desc.append("Loyal_Rebuyer")
        if stats["relative_price_pos"] < 0.9:
            desc.append("Discount_Hunter")
        elif stats["relative_price_pos"] > 1.1:
            desc.append("Premium_Picker")
        if stats["cat_entropy"] < 0.5:
            desc.append("Specialist")
        elif stats["cat_entropy"] > 1.5:
            desc.append("Explorer")
        if stats["long_tail_ratio"] > 0.6:
            desc.append("Hipster")
        if not desc:
            desc.append("Standard_Shopper")
        out.append({
            "cluster_id": int(cluster_id),
            "persona_name": f"Cluster {cluster_id}: {' & '.join(desc)}",
            "stats": {
                "basket_size": {"mean": stats["basket_size"], "std": basket_std},
                "category_entropy": stats["cat_entropy"],
                "price_sensitivity": {"avg_price": stats["avg_price"], "relative_pos": stats["relative_price_pos"],
                                      "description": "High Spending" if stats["avg_price"] > global_means["avg_price"] else "Low Spending"},
                "shopping_pattern": {"weekend_ratio": stats["weekend_ratio"], "repurchase_rate": stats["repurchase_rate"],
                                     "long_tail_ratio": stats["long_tail_ratio"]},
            },
            "user_count": int(len(sub)),
        })
    return json.loads(json.dumps(out))             # plain floats, as the JSON file holds them


def persona_log(n_customers=120, n_items=60, n_rows=3000, seed=0):
    """A shuffled log with several items per three-character category (12 categories), skewed item popularity,
    repeat purchases, a customer with many rows, customers of one row and float32 prices that depend on the
    category."""
    rng = np.random.default_rng(seed)
    cust = rng.integers(0, n_customers - 2, n_rows)
    cust[rng.random(n_rows) < 0.15] = 0
    cust = np.concatenate([cust, [n_customers - 2, n_customers - 1]])          # two customers of one row
    item = np.minimum((n_items * rng.random(len(cust)) ** 2.0).astype(np.int64), n_items - 1)
    narrow = cust % 3 == 1                                                     # customers who stay in one category
    item[narrow] = (cust[narrow] % 12) * 5 + item[narrow] % 2
    ids = np.asarray([f"{100 + i // 5}{i % 5:04d}" for i in range(n_items)])   # 5 items per category 100 .. 111
    day = rng.integers(0, 120, len(cust))
    price = (0.01 + 0.004 * (item // 5) + rng.gamma(2.0, 0.01, len(cust))).astype(np.float32)
    df = pd.DataFrame({"t_dat": np.datetime64(TR.BASE_MONDAY, "D") + day.astype("timedelta64[D]"),
                       "customer_id": [f"c{c:05d}" for c in cust], "article_id": ids[item], "price": price,
                       "sales_channel_id": rng.integers(1, 3, len(cust)).astype(np.int8)})
    return df.iloc[rng.permutation(len(df))].reset_index(drop=True)
