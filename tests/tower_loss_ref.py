"""Float64 restatement of HybridUserTower's two in-batch losses (reference tower_code/mined_inference.py
:738-789), with the [B, B] logit matrix written out and the reference's finite fills (-1e4, -1e9) kept as
they are. Inputs are cast to float64; tensors that require grad keep their graph.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _collisions(pos):
    same = pos.view(-1, 1) == pos.view(1, -1)
    return same & ~torch.eye(pos.numel(), dtype=torch.bool)


def _mean_ce(logits):
    return F.cross_entropy(logits, torch.arange(logits.shape[0]))


def logq_correction(u, v, pos, item_probs, temperature=0.07, lambda_logq=0.0):
    """:738-749: (u v^T - lambda log(item_probs[pos_j] + 1e-4)) / temperature, collisions at -1e4."""
    u, v = u.double(), v.double()
    scores = u @ v.T
    if lambda_logq > 0.0:
        scores = scores - lambda_logq * torch.log(item_probs.double()[pos] + 1e-4)[None, :]
    return _mean_ce((scores / temperature).masked_fill(_collisions(pos), -1e4))


def efficient_corrected_logq(u, v, pos, log_q, temperature=0.1, lambda_logq=0.1):
    """:751-789: u v^T / temperature - lambda log_q[pos_j]; with lambda > 0 the diagonal is put back to
    <u_i, v_i> / temperature; collisions at -1e9."""
    u, v = u.double(), v.double()
    logits = (u @ v.T) / temperature
    if lambda_logq > 0.0:
        logits = logits - lambda_logq * log_q.double()[pos][None, :]
        eye = torch.eye(pos.numel(), dtype=torch.bool)
        logits = torch.where(eye, ((u * v).sum(1) / temperature)[:, None], logits)
    return _mean_ce(logits.masked_fill(_collisions(pos), -1e9))


def make_case(B, seed, n_items=37):
    """Unit rows u, v [B, 128], pos_item_ids [B] with repeats (B > 1), item_probs and log_q [n_items]."""
    g = torch.Generator().manual_seed(seed)
    u = F.normalize(torch.randn(B, 128, generator=g), dim=1)
    v = F.normalize(torch.randn(B, 128, generator=g) + 0.5 * u, dim=1)
    pos = torch.randint(0, n_items, (B,), generator=g)
    if B > 1:
        pos[B - 1] = pos[0]          # at least one collision
    if B > 4:
        pos[3] = pos[1] = n_items - 1   # and a pair on the table's last row
    probs = torch.rand(n_items, generator=g) ** 3 + 1e-6
    probs = probs / probs.sum()
    return u, v, pos, probs, torch.log(probs)
