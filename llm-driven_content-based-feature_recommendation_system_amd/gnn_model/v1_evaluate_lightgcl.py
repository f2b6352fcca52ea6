"""Drop-in for gnn_model/v1_evaluate_lightgcl.py: propagated embeddings and hit-rate@k of a trained
LightGCL.

Reference (gnn_model/v1_evaluate_lightgcl.py): compute_final_embeddings :147-179, evaluate_recall
:275-340. Compute: the propagation is ops.lightgcl_propagate (rsx_spmm_norm per layer), the retrieval
ops.retrieve_topk (exact top-k without the score matrix).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops


def compute_final_embeddings(model, adj, n_layers=2, rows=None):
    """(final_user_emb, final_item_emb): the layer mean of the tables propagated through the graph
    (:147-179). rows (int64 node ids, users first) restricts the last layer to those destinations and
    returns their [len(rows), D] rows instead of the split pair."""
    model.eval()
    with torch.no_grad():
        ego = torch.cat([model.embedding_user.weight, model.embedding_item.weight], dim=0)
        if rows is not None:
            return ops.lightgcl_propagate(ego, adj, n_layers, rows=rows.to(ego.device))
        final = ops.lightgcl_propagate(ego, adj, n_layers)
        return torch.split(final, [model.embedding_user.num_embeddings, model.embedding_item.num_embeddings])


def topk_items(user_emb, all_items, k):
    """Indices [Q, k] of the k largest dot products per user over all_items[1:] (item 0 is the
    padding row and never returned, :315), ties to the lower index."""
    items = all_items[1:]
    if items.shape[1] < 128:   # ops.retrieve_topk reads 128 columns; zero columns change no dot product
        items = F.pad(items, (0, 128 - items.shape[1]))
        user_emb = F.pad(user_emb, (0, 128 - user_emb.shape[1]))
    _, idx = ops.retrieve_topk(user_emb, items, k)
    return idx + 1


def evaluate_recall(model, ground_truth_dict, device, k_list=[20, 100], batch_size=4096):
    """Hit-rate@k by dot product (:275-340): a user counts for k when one of its ground-truth items is
    among its k best items. Returns {"hits": {k: count}, "recall": {k: hits / users}, "users": count}."""
    max_k = max(k_list)
    model.eval()
    users = list(ground_truth_dict.keys())
    hits = {k: 0 for k in k_list}
    with torch.no_grad():
        all_items = model.embedding_item.weight.data.to(device)
        table = model.embedding_user.weight.data
        for s in range(0, len(users), batch_size):
            batch = users[s:s + batch_size]
            u = table[torch.tensor(batch, dtype=torch.long, device=table.device)]
            topk = topk_items(u.to(device), all_items, max_k).cpu().numpy()
            for row, u_idx in zip(topk, batch):
                truth = ground_truth_dict[u_idx]
                for k in k_list:
                    if not truth.isdisjoint(row[:k].tolist()):
                        hits[k] += 1
    total = len(users)
    return {"hits": hits, "recall": {k: (hits[k] / total if total else 0.0) for k in k_list}, "users": total}
