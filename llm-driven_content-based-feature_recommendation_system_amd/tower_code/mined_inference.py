"""Drop-in for the ensemble evaluators of tower_code/mined_inference.py: late fusion of the sequence
retriever and the GNN retriever over an alpha sweep, on the device.

Reference (tower_code/mined_inference.py): evaluate_multi_vector_ensemble :797-993,
evaluate_weighted_score_ensemble :996-1227 (the live entry point of main, :1669-1678),
evaluate_rrf_ensemble :1238-1448.

Departure from the reference signature: the reference took `seq_model, processor, target_df_path` and
the GNN tables, ran the sequence model over a DataLoader and read the targets from a parquet file. These
evaluators work at the vector level: they take the user and item vectors of both retrievers (rows of
one user / one item in the same position in both spaces) and `ground_truth`, a dict from a user row to
the set of its item rows (0-based into the item matrices), as gnn_model.v1_evaluate_lightgcl.
evaluate_recall does. Any tower produces the vectors: SASRecUserTower with the distilled LightGCL tables
(gnn_model.distill_mag_to_cos_l2) today. They return the whole sweep, not only the best alpha:
{"best_alpha", "hits": {alpha: {k: users hit}}, "recall": {alpha: {k: hits / users}}, "users"}.
alpha weighs the GNN retriever, 1 - alpha the sequence retriever.

Compute: per chunk of users the two score matrices come from fp32 torch.matmul, each pool from
ops.select_topk_rows, and the fusion, the alpha sweep and the hit test of the chunk from one
ops.fuse_rank launch (csrc/ensemble.hip); the ratio merge takes two ops.retrieve_topk lists and two
ops.first_hit. Hit counts accumulate on the device and are read once per evaluation. One clamp is ours:
the number of fused entries kept, max_k + 20 in the reference, is min(pool entries, max_k + 20) (torch.topk
would raise there). There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops

SCORE_CHUNK_BYTES = 512 << 20   # bound of one [users, items] fp32 score matrix


def alpha_grid(alpha_step):
    """The reference's sweep (:1058): 1.0 down to 0.0 in steps of alpha_step, rounded to one decimal."""
    return [float(round(x, 1)) for x in np.arange(1.0, -0.01, -alpha_step)]


def fusion_weights(alphas):
    """(wa, wb) float32 arrays: float32(alpha) and float32(1.0 - alpha), the subtraction in double as
    Python does in `alpha * s_gnn + (1.0 - alpha) * s_seq` (:1162); what ops.fuse_rank hands the kernel."""
    wa, wb = ops.fusion_weights(alphas)
    return np.array(wa, dtype=np.float32), np.array(wb, dtype=np.float32)


def ratio_thresholds(alphas, k_list):
    """(n_gnn, n_seq) int arrays [A, K] of the ratio merge (:931-932): n_gnn = int(k * alpha),
    n_seq = k - n_gnn."""
    n_gnn = np.array([[int(k * a) for k in k_list] for a in alphas], dtype=np.int64)
    return n_gnn, np.array([list(k_list)] * len(alphas), dtype=np.int64) - n_gnn


def truth_csr(ground_truth, users, n_items=None):
    """(truth_off int64 [len(users) + 1], truth int32) of the users in order: each user's items
    ascending and distinct. An item outside [0, n_items) raises."""
    off = np.zeros(len(users) + 1, dtype=np.int64)
    parts = []
    for j, u in enumerate(users):
        items = np.unique(np.fromiter((int(i) for i in ground_truth[u]), dtype=np.int64))
        if items.size and (items[0] < 0 or (n_items is not None and items[-1] >= n_items)):
            raise IndexError(f"ground_truth[{u}] holds an item row outside [0, {n_items})")
        parts.append(items)
        off[j + 1] = off[j] + items.size
    truth = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return off, truth.astype(np.int32)


def best_alpha(hits, k_list, users):
    """The reference's choice (:1206-1222): recall at the first k of k_list, alphas in descending order,
    a strict >, so of equal alphas the largest wins; -1 without alphas."""
    best, best_score = -1, -1
    for alpha in sorted(hits.keys(), reverse=True):
        score = hits[alpha][k_list[0]] / users if users > 0 else 0
        if score > best_score:
            best_score, best = score, alpha
    return best


def _result(alphas, k_list, counts, users):
    hits = {a: {k: int(counts[i][j]) for j, k in enumerate(k_list)} for i, a in enumerate(alphas)}
    recall = {a: {k: (hits[a][k] / users if users > 0 else 0) for k in k_list} for a in alphas}
    return {"best_alpha": best_alpha(hits, k_list, users), "hits": hits, "recall": recall, "users": users}


def _prepare(fn, seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth, device, assume_normalized):
    """The four matrices as fp32 on `device`, L2-normalised unless told otherwise, and the users."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{fn}: the ensemble evaluators run on the device only (csrc/ensemble.hip has no CPU "
                           f"path); got device {device}")
    mats = []
    for name, t in (("seq_user_vecs", seq_user_vecs), ("seq_item_vecs", seq_item_vecs),
                    ("gnn_user_vecs", gnn_user_vecs), ("gnn_item_vecs", gnn_item_vecs)):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{fn}: {name} must be a 2-D tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"{fn}: {name} is on {t.device}; the ensemble evaluators run on the device only "
                               "(there is no CPU path)")
        t = t.detach().to(device=device, dtype=torch.float32)
        mats.append(t if assume_normalized else ops.l2_normalize(t))
    su, si, gu, gi = mats
    if su.shape[1] != si.shape[1] or gu.shape[1] != gi.shape[1]:
        raise ValueError(f"{fn}: user and item widths disagree: seq {su.shape[1]} / {si.shape[1]}, "
                         f"gnn {gu.shape[1]} / {gi.shape[1]}")
    if si.shape[0] != gi.shape[0]:
        raise ValueError(f"{fn}: the retrievers must share the corpus: {si.shape[0]} / {gi.shape[0]} item rows")
    users = list(ground_truth.keys())
    n_users = min(su.shape[0], gu.shape[0])
    for u in users:
        if not 0 <= int(u) < n_users:
            raise IndexError(f"{fn}: ground_truth names user row {u}; the user matrices hold {n_users} rows")
    return su, si, gu, gi, users


def _chunk_rows(batch_size, n_items):
    return max(1, min(int(batch_size), SCORE_CHUNK_BYTES // (4 * n_items)))


def _bit_counts(hits, n_bits):
    """[A, n_bits] int64: how many users have bit j set in hits [B, A]."""
    shifts = torch.arange(n_bits, device=hits.device, dtype=torch.int32)
    return ((hits.unsqueeze(-1) >> shifts) & 1).sum(dim=0, dtype=torch.int64)


def _evaluate_fused(fn, mode, seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth, device, k_list,
                    batch_size, alpha_step, candidate_pool_size, assume_normalized, k_rrf):
    k_list = [int(k) for k in k_list]
    with torch.no_grad():
        su, si, gu, gi, users = _prepare(fn, seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth,
                                         device, assume_normalized)
        dev, n_items = su.device, si.shape[0]
        alphas = alpha_grid(alpha_step)
        max_k = max(k_list)
        pool_k = min(max(int(candidate_pool_size), 2 * max_k), n_items)   # :1017
        if 2 * pool_k > ops.FUSE_MAX_POOL:
            raise ValueError(f"{fn}: a pool of {pool_k} per retriever gives {2 * pool_k} fused entries; the fusion "
                             f"kernel takes {ops.FUSE_MAX_POOL} (candidate_pool_size and 2 max(k_list) up to "
                             f"{ops.FUSE_MAX_POOL // 2})")
        cut = min(2 * pool_k, max_k + 20)
        # hit@k for k beyond the cut is hit@cut (the list holds no more); distinct bits, ascending
        ks = sorted({min(k, cut) for k in k_list})
        bit_of = [ks.index(min(k, cut)) for k in k_list]
        off, truth = truth_csr(ground_truth, users, n_items)
        off_d, truth_d = torch.from_numpy(off).to(dev), torch.from_numpy(truth).to(dev)
        users_d = torch.tensor(users, dtype=torch.long, device=dev)
        counts = torch.zeros(len(alphas), len(ks), device=dev, dtype=torch.int64)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        step = _chunk_rows(batch_size, n_items)
        for s in range(0, len(users), step):
            rows = users_d[s:s + step]
            ug, us = gu[rows], su[rows]
            pool_g, _ = ops.select_topk_rows(torch.matmul(ug, gi.T), pool_k)   # :1103-1104
            pool_s, _ = ops.select_topk_rows(torch.matmul(us, si.T), pool_k)   # :1107-1108
            cand = torch.cat([pool_g, pool_s], dim=1)                          # :1115
            out = ops.fuse_rank(ug, gi, us, si, cand, alphas, ks, off_d[s:s + rows.numel() + 1], truth_d, mode=mode,
                                k_rrf=k_rrf, cut=cut, flag=flag)
            counts += _bit_counts(out.hits, len(ks))
        host = torch.cat([counts.flatten(), flag.to(torch.int64)]).cpu().tolist()   # the evaluation's one read
    if host[-1]:
        raise RuntimeError(f"{fn}: a pool entry fell outside the corpus")
    per_bit = np.array(host[:-1], dtype=np.int64).reshape(len(alphas), len(ks))
    return _result(alphas, k_list, per_bit[:, bit_of], len(users))


def evaluate_weighted_score_ensemble(seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth, device,
                                     k_list=[20, 100, 500], batch_size=4096, alpha_step=0.1,
                                     candidate_pool_size=1000, assume_normalized=False):
    """Weighted score fusion (:996-1227): each retriever's top pool_k = max(candidate_pool_size,
    2 max(k_list)) items, both scores of the joined pool min-max normalised per user, and for every
    alpha the order by alpha s_gnn + (1 - alpha) s_seq, its first max_k + 20 entries without repeats,
    hit@k. The vectors are L2-normalised here unless assume_normalized."""
    return _evaluate_fused("evaluate_weighted_score_ensemble", "minmax", seq_user_vecs, seq_item_vecs, gnn_user_vecs,
                           gnn_item_vecs, ground_truth, device, k_list, batch_size, alpha_step, candidate_pool_size,
                           assume_normalized, 0.0)


def evaluate_rrf_ensemble(seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth, device,
                          k_list=[20, 100, 500], batch_size=4096, alpha_step=0.1, candidate_pool_size=1000,
                          k_rrf=200, assume_normalized=False):
    """Weighted reciprocal-rank fusion (:1238-1448): as evaluate_weighted_score_ensemble with each
    score replaced by 1 / (k_rrf + rank + 1), rank the entry's 0-based place in its list of the pool."""
    return _evaluate_fused("evaluate_rrf_ensemble", "rrf", seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs,
                           ground_truth, device, k_list, batch_size, alpha_step, candidate_pool_size,
                           assume_normalized, float(k_rrf))


def _pad128(t):
    # ops.retrieve_topk reads 128 columns; zero columns change no dot product
    return t if t.shape[1] == 128 else F.pad(t, (0, 128 - t.shape[1]))


def evaluate_multi_vector_ensemble(seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth, device,
                                   k_list=[20, 100, 500], batch_size=4096, alpha_step=0.2,
                                   assume_normalized=False):
    """Ratio merge (:797-993): for every alpha and k the union of the GNN retriever's first int(k alpha)
    items and the sequence retriever's first k - int(k alpha); a user hits when the union meets its
    ground truth, i.e. when its first hit in either list lies inside that list's share."""
    fn = "evaluate_multi_vector_ensemble"
    k_list = [int(k) for k in k_list]
    with torch.no_grad():
        su, si, gu, gi, users = _prepare(fn, seq_user_vecs, seq_item_vecs, gnn_user_vecs, gnn_item_vecs, ground_truth,
                                         device, assume_normalized)
        if su.shape[1] > 128 or gu.shape[1] > 128:
            raise ValueError(f"{fn}: ops.retrieve_topk reads 128 columns (got {su.shape[1]} / {gu.shape[1]})")
        dev, n_items = su.device, si.shape[0]
        alphas = alpha_grid(alpha_step)
        max_k = min(max(k_list), n_items)
        n_gnn, n_seq = (torch.from_numpy(t).to(dev) for t in ratio_thresholds(alphas, k_list))
        off, truth = truth_csr(ground_truth, users, n_items)
        off_d, truth_d = torch.from_numpy(off).to(dev), torch.from_numpy(truth).to(dev)
        users_d = torch.tensor(users, dtype=torch.long, device=dev)
        gi, si = _pad128(gi), _pad128(si)
        counts = torch.zeros(len(alphas), len(k_list), device=dev, dtype=torch.int64)
        for s in range(0, len(users), int(batch_size)):
            rows = users_d[s:s + int(batch_size)]
            csr = off_d[s:s + rows.numel() + 1]
            _, idx_g = ops.retrieve_topk(_pad128(gu[rows]), gi, max_k)   # :901-903
            _, idx_s = ops.retrieve_topk(_pad128(su[rows]), si, max_k)   # :907-908
            pg = ops.first_hit(idx_g, csr, truth_d).to(torch.int64)
            ps = ops.first_hit(idx_s, csr, truth_d).to(torch.int64)
            # no hit gives max_k, and n_gnn, n_seq <= k <= max_k unless the corpus is smaller than k: there
            # the lists hold the whole corpus and a miss must stay a miss
            miss_g, miss_s = pg >= max_k, ps >= max_k
            hit = ((pg[:, None, None] < n_gnn) & ~miss_g[:, None, None]) | \
                  ((ps[:, None, None] < n_seq) & ~miss_s[:, None, None])
            counts += hit.sum(dim=0, dtype=torch.int64)
        host = counts.cpu().tolist()   # the evaluation's one read
    return _result(alphas, k_list, host, len(users))
