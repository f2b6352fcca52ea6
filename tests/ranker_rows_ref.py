"""Host restatement of the ranker's training rows (include/recsys_amd.h, "ranker training rows"): the
sampler of rsx_ranker_rows_sample in integer numpy (hash_u32 of csrc/rsx_common.h restated in 64-bit
integers masked to 32 bits), the seven FeatureEngineer columns of rsx_pair_tabular in float64, and the
reference's importer loop (utils/monitor/log_importer.py:36-87) with the device's draws in place of
Python's random."""
import numpy as np

M32 = 0xFFFFFFFF


def hash_u32(seed, idx):
    """hash_u32(seed, idx) of csrc/rsx_common.h for an int seed in [0, 2^64) and idx an array of indices in
    [0, 2^63): uint32 values as int64."""
    idx = np.asarray(idx, np.uint64)
    seed = int(seed)
    u, m = np.uint64, np.uint64(M32)
    x = (idx & m) ^ (((idx >> u(32)) * u(0x9E3779B1)) & m) ^ u(seed & M32)
    x = x ^ u(((seed >> 32) * 0x85EBCA77) & M32)
    x = x ^ (x >> u(16))
    x = (x * u(0x85EBCA6B)) & m          # x < 2^32: the product fits 64 bits
    x = x ^ (x >> u(13))
    x = (x * u(0xC2B2AE35)) & m
    x = x ^ (x >> u(16))
    return x.astype(np.int64)


def rank_map(s, r):
    """The r-th (0-based) non-negative integer not in the ascending distinct list s: r + #{j : s_j - j <= r}."""
    s = np.asarray(s, np.int64)
    return np.asarray(r, np.int64) + np.searchsorted(s - np.arange(len(s)), r, side="right")


def draw(seed, index, s, n_items):
    """The negatives of the counters `index` (= p K + k) for a customer whose bought items are s."""
    M = n_items - len(s)
    assert M > 0
    r = (hash_u32(seed, index) * M) >> 32
    return rank_map(s, r)


def sample(pos_user, pos_item, bought_off, bought, n_items, K, seed):
    """(row_user, row_item int32, y float32), each [Pv (K + 1)]: the rows of rsx_ranker_rows_sample."""
    Pv = len(pos_user)
    row_user = np.repeat(np.asarray(pos_user, np.int32), K + 1)
    row_item = np.zeros(Pv * (K + 1), np.int32)
    y = np.zeros(Pv * (K + 1), np.float32)
    for p in range(Pv):
        u = int(pos_user[p])
        s = np.asarray(bought[bought_off[u]:bought_off[u + 1]], np.int64)
        row_item[p * (K + 1)] = pos_item[p]
        y[p * (K + 1)] = 1.0
        if K:
            row_item[p * (K + 1) + 1:(p + 1) * (K + 1)] = draw(seed, p * K + np.arange(K), s, n_items)
    return row_user, row_item, y


def columns(row_user, row_item, score, U, V, price, avg):
    """float64 [7, R]: the FeatureEngineer columns of the rows; score None: the float64 dot product. Also
    returns max |u_i v_i| over all rows, the scale of the kernel's rounding error."""
    u, v = np.asarray(U, np.float64)[row_user], np.asarray(V, np.float64)[row_item]
    prod = u * v
    a, p = np.asarray(avg, np.float64)[row_user], np.asarray(price, np.float64)[row_item]
    ratio = np.where(a > 0, (p - a) / np.where(a > 0, a, 1.0), 0.0)
    col0 = prod.sum(-1) if score is None else np.asarray(score, np.float64)
    return np.stack([col0, prod.mean(-1), prod.max(-1), prod.std(-1), p, a, ratio]), float(np.abs(prod).max())


def importer(lines, store_keys, limit, K, seed):
    """The reference's loop over `lines` = [(customer_id, article_id)] in file order: (items, y, groups) with
    an item as its position in store_keys; negative (p, k) is draw(seed, p K + k) over the customer's distinct
    bought items that have a vector."""
    index = {k: i for i, k in enumerate(store_keys)}
    by = {}
    for c, a in lines[:limit]:
        by.setdefault(c, []).append(a)
    items, y, groups, p = [], [], [], 0
    for g, c in enumerate(sorted(by)):
        s = sorted({index[a] for a in by[c] if a in index})
        for a in by[c]:
            if a not in index:
                continue
            items.append(index[a])
            y.append(1.0)
            groups.append(g)
            for neg in draw(seed, p * K + np.arange(K), s, len(store_keys)) if K else []:
                items.append(int(neg))
                y.append(0.0)
                groups.append(g)
            p += 1
    return np.asarray(items, np.int32), np.asarray(y, np.float32), np.asarray(groups, np.int32)
