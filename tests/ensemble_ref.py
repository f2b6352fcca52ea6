"""Numpy restatement of the late-fusion evaluation (csrc/ensemble.hip, tower_code/mined_inference.py):
exact top-k of score rows, the fusion of two retrievers over a candidate pool with its alpha sweep, the
first hit of a list, and the three evaluators built on them. Every float32 expression is formed in the
order include/recsys_amd.h states (numpy float32 arithmetic rounds each operation once, like the
kernel's uncontracted fp32); every sort is stable. dot64 is the float64 yardstick of the scores."""
from __future__ import annotations

import numpy as np

MINMAX, RRF = "minmax", "rrf"


def score_key(x):
    """uint32 sort key of float32 values: larger float <=> larger key, -0.0 and +0.0 equal."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[x == 0.0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_desc(v):
    """Positions of the float32 vector v in the order (key descending, position ascending)."""
    k = score_key(v).astype(np.int64)
    return np.argsort(-k, kind="stable")


def select_topk(S, k):
    """(idx [Q, k] int32, val [Q, k] float32): np.lexsort by (value descending, index ascending)."""
    S = np.asarray(S, dtype=np.float32)
    idx = np.empty((S.shape[0], k), dtype=np.int32)
    for q in range(S.shape[0]):
        key = score_key(S[q]).astype(np.int64)
        idx[q] = np.lexsort((np.arange(S.shape[1]), -key))[:k]
    return idx, np.take_along_axis(S, idx.astype(np.int64), axis=1)


def dot64(u, V):
    """float64 dot products of the row u with the rows of V, and sum |u_i| |v_i| for the error bound."""
    u = np.asarray(u, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    return V @ u, np.abs(V) @ np.abs(u)


def fusion_weights(alphas):
    """(wa, wb) float32: float32(alpha) and float32(1.0 - alpha), the subtraction in double."""
    wa = np.array([np.float32(float(a)) for a in alphas], dtype=np.float32)
    wb = np.array([np.float32(1.0 - float(a)) for a in alphas], dtype=np.float32)
    return wa, wb


def normalise(s, mode, k_rrf):
    s = np.asarray(s, dtype=np.float32)
    if mode == MINMAX:
        mn, mx = s.min(), s.max()
        return ((s - mn) / ((mx - mn) + np.float32(1e-9))).astype(np.float32)
    rank = np.empty(s.shape[0], dtype=np.float32)
    rank[order_desc(s)] = np.arange(s.shape[0], dtype=np.float32)
    return (np.float32(1.0) / ((np.float32(k_rrf) + rank) + np.float32(1.0))).astype(np.float32)


def fused_list(na, nb, wa, wb, cand, cut):
    """One alpha: the ids of the first `cut` entries in the fused order, later repeats dropped."""
    f = (np.float32(wa) * na + np.float32(wb) * nb).astype(np.float32)
    ids = np.asarray(cand)[order_desc(f)[:cut]]
    seen, out = set(), []
    for i in ids.tolist():
        if i not in seen:
            seen.add(i)
            out.append(i)
    return out


def fuse_rank(sa, sb, cand, wa, wb, mode, k_rrf, cut, ks, truth):
    """hits [Q, A] int32 (bit j = hit@ks[j]) and lists [Q, A, ks[-1]] int32 (-1 padded) from the raw
    scores sa / sb [Q, C] of the pool entries cand [Q, C]; truth: one set of item rows per user."""
    Q = len(sa)
    hits = np.zeros((Q, len(wa)), dtype=np.int32)
    lists = np.full((Q, len(wa), ks[-1]), -1, dtype=np.int32)
    for q in range(Q):
        na, nb = normalise(sa[q], mode, k_rrf), normalise(sb[q], mode, k_rrf)
        for a in range(len(wa)):
            lst = fused_list(na, nb, wa[a], wb[a], cand[q], cut)
            head = lst[:ks[-1]]
            lists[q, a, :len(head)] = head
            for j, k in enumerate(ks):
                if not truth[q].isdisjoint(lst[:k]):
                    hits[q, a] |= 1 << j
    return hits, lists


def first_hit(lists, truth):
    out = np.full(len(lists), lists.shape[1], dtype=np.int32)
    for q in range(len(lists)):
        for j, i in enumerate(lists[q].tolist()):
            if i in truth[q]:
                out[q] = j
                break
    return out


def alpha_grid(alpha_step):
    return [float(round(x, 1)) for x in np.arange(1.0, -0.01, -alpha_step)]


def best_alpha(hits, k_list, users):
    """The reference's rule: recall at the first k of k_list, a strict >, alphas in descending order."""
    best, best_score = -1, -1
    for alpha in sorted(hits.keys(), reverse=True):
        score = hits[alpha][k_list[0]] / users if users > 0 else 0
        if score > best_score:
            best_score, best = score, alpha
    return best


def _result(hits, k_list, users):
    recall = {a: {k: (hits[a][k] / users if users > 0 else 0) for k in k_list} for a in hits}
    return {"best_alpha": best_alpha(hits, k_list, users), "hits": hits, "recall": recall, "users": users}


def _ranked(cache, u, seq_u, seq_i, gnn_u, gnn_i):
    """User u's float32 score rows and their full orders (computed once per user when a cache is kept)."""
    if cache is not None and u in cache:
        return cache[u]
    sg = (gnn_i @ gnn_u[u]).astype(np.float32)[None]
    ss = (seq_i @ seq_u[u]).astype(np.float32)[None]
    r = sg, ss, select_topk(sg, sg.shape[1])[0], select_topk(ss, ss.shape[1])[0]
    if cache is not None:
        cache[u] = r
    return r


def evaluate_fused(seq_u, seq_i, gnn_u, gnn_i, ground_truth, k_list, alpha_step, candidate_pool_size, mode,
                   k_rrf=200, cache=None):
    """evaluate_weighted_score_ensemble (mode MINMAX) / evaluate_rrf_ensemble (mode RRF) on the given
    vectors; alpha weighs the GNN retriever, whose pool comes first. cache: a dict kept by the caller
    across evaluations of the same vectors."""
    alphas = alpha_grid(alpha_step)
    wa, wb = fusion_weights(alphas)
    n_items = seq_i.shape[0]
    max_k = max(k_list)
    pool_k = min(max(candidate_pool_size, 2 * max_k), n_items)
    cut = min(2 * pool_k, max_k + 20)
    ks = sorted(min(k, cut) for k in k_list)
    hits = {a: {k: 0 for k in k_list} for a in alphas}
    for u, items in ground_truth.items():
        sg, ss, og, os_ = _ranked(cache, u, seq_u, seq_i, gnn_u, gnn_i)
        cand = np.concatenate([og[:, :pool_k], os_[:, :pool_k]], axis=1)
        bits, _ = fuse_rank(sg[:, cand[0]], ss[:, cand[0]], cand, wa, wb, mode, k_rrf, cut, ks, [set(items)])
        for ai, a in enumerate(alphas):
            for k in k_list:
                hits[a][k] += int(bits[0, ai] >> ks.index(min(k, cut)) & 1)
    return _result(hits, k_list, len(ground_truth))


def evaluate_multi_vector(seq_u, seq_i, gnn_u, gnn_i, ground_truth, k_list, alpha_step, cache=None):
    alphas = alpha_grid(alpha_step)
    max_k = max(k_list)
    hits = {a: {k: 0 for k in k_list} for a in alphas}
    for u, items in ground_truth.items():
        _, _, og, os_ = _ranked(cache, u, seq_u, seq_i, gnn_u, gnn_i)
        lg, ls = og[:, :max_k], os_[:, :max_k]
        pa, pb = first_hit(lg, [set(items)])[0], first_hit(ls, [set(items)])[0]
        for a in alphas:
            for k in k_list:
                n_gnn = int(k * a)
                hits[a][k] += int(pa < n_gnn or pb < k - n_gnn)
    return _result(hits, k_list, len(ground_truth))
