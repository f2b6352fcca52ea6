"""Float64 reference of LightGCL, written from the model's formulas (dense matrices, torch autograd):
A^ = diag(dinv) B diag(dinv); local = mean_k A^^k E; x_g <- U (S . (V^T x_g)), global = mean of E and
the x_g; BPR with 1e-10 inside the log; InfoNCE of the L2-normalised local rows against the global
rows over the distinct users / items; L2 regulariser; Adam. TEST INFRASTRUCTURE ONLY.

The graph's own fp32 dinv and the fp32 U, S, V are taken as exact inputs. Error bounds use u = 2^-24
(fp32 unit roundoff) and the recursive-summation bound (terms + const) u sum|terms|.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


# ---- graphs ---------------------------------------------------------------------------------
def power_law_edges(num_users=3001, num_items=500, num_edges=20000, seed=0):
    """Seeded bipartite edges [2, E] with Zipf item popularity, unsorted, with duplicates."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, num_items + 1) ** 1.1
    items = rng.choice(num_items, size=num_edges, p=p / p.sum())
    users = rng.integers(0, num_users, num_edges)
    return torch.from_numpy(np.stack([users, items]).astype(np.int64))


def star_edges(num_users):
    """One item joined to every one of num_users users."""
    return torch.stack([torch.arange(num_users), torch.zeros(num_users, dtype=torch.int64)])


def dense_binary(adj):
    """B as a dense float64 matrix from the CSR."""
    n = adj.n
    B = torch.zeros(n, n, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(n), (adj.row_ptr[1:] - adj.row_ptr[:-1]).cpu())
    B[rows, adj.col.cpu().long()] = 1.0
    return B


def dense_norm(adj):
    """A^ in float64 from B and the graph's fp32 dinv (exact input)."""
    d = adj.dinv.cpu().double()
    return d[:, None] * dense_binary(adj) * d[None, :]


# ---- kernels --------------------------------------------------------------------------------
def spmm(A, X, R=None, alpha=1.0, rows=None):
    """(value, bound): alpha (R + A X) and (deg_r + 4) u (|A||X| + |R|)_r |alpha| per element."""
    X = X.double()
    val, mag = A @ X, A.abs() @ X.abs()
    if R is not None:
        val, mag = val + R.double(), mag + R.double().abs()
    deg = (A != 0).sum(1, keepdim=True).double()
    val, bound = alpha * val, (deg + 4) * U24 * mag * abs(alpha)
    if rows is not None:
        val, bound = val[rows], bound[rows]
    return val, bound


def proj(V, X):
    """(V^T X, bound (n + 2) u |V|^T |X|)."""
    V, X = V.double(), X.double()
    return V.t() @ X, (V.shape[0] + 2) * U24 * (V.abs().t() @ X.abs())


def update(Y, V, W):
    """(Y + V W, bound (q + 1 + 2) u (|Y| + |V||W|))."""
    Y, V, W = Y.double(), V.double(), W.double()
    return Y + V @ W, (V.shape[1] + 3) * U24 * (Y.abs() + V.abs() @ W.abs())


# ---- model ----------------------------------------------------------------------------------
def local_view(A, E, n_layers):
    x, acc = E, E
    for _ in range(n_layers):
        x = A @ x
        acc = acc + x
    return acc / (n_layers + 1)


def local_view_bound(A, E, n_layers):
    """Per-element bound of the Horner evaluation T <- alpha_j (E + A T): every step adds its own
    spmm bound to |alpha_j| |A| times the bound carried by T."""
    E = E.double()
    absA = A.abs()
    deg = (A != 0).sum(1, keepdim=True).double()
    T, err = E, torch.zeros_like(E)
    for j in range(n_layers):
        alpha = 1.0 / (n_layers + 1) if j == n_layers - 1 else 1.0
        err = alpha * ((deg + 4) * U24 * (absA @ T.abs() + E.abs()) + absA @ err)
        T = alpha * (E + A @ T)
    return err


def global_view(U, S, V, E, n_layers):
    x, acc = E, E
    for _ in range(n_layers):
        x = U @ (S[:, None] * (V.t() @ x))
        acc = acc + x
    return acc / (n_layers + 1)


def global_view_bound(U, S, V, E, n_layers):
    """Bound of (E + U sum_j C_j) / (L + 1), C_1 = S.(V^T E), C_{j+1} = S.(K C_j), K = V^T U in fp32:
    the projection bounds of P and K, (q + 2) u per small product, one u per scaling or sum, and the
    update's bound, each carried through the terms that follow."""
    U, S, V, E = U.double(), S.double()[:, None], V.double(), E.double()
    n, q = U.shape
    inv = 1.0 / (n_layers + 1)
    if n_layers == 0:
        return torch.zeros_like(E)
    K, eK = V.t() @ U, (n + 2) * U24 * (V.abs().t() @ U.abs())
    P, eP = proj(V, E)
    C = S * P
    eC = S * eP + U24 * C.abs()
    W, eW = C, eC
    for _ in range(n_layers - 1):
        KC = K @ C
        eKC = K.abs() @ eC + eK @ C.abs() + (q + 2) * U24 * (K.abs() @ C.abs())
        C = S * KC
        eC = S * eKC + U24 * C.abs()
        W = W + C
        eW = eW + eC + U24 * W.abs()
    Wi, eWi = W * inv, eW * inv + U24 * (W * inv).abs()
    Y = E * inv
    _, e_upd = update(Y, U, Wi)
    return U24 * Y.abs() + e_upd + U.abs() @ eWi


def losses(Wu, Wi, A, U, S, V, cfg, users, pos, neg):
    """(bpr, ssl, reg, total) in float64 with autograd through Wu, Wi; pos / neg are item ids."""
    nu = Wu.shape[0]
    E = torch.cat([Wu, Wi])
    L = cfg["n_layers"]
    loc, glo = local_view(A, E, L), global_view(U, S, V, E, L)
    ue, pe, ne = loc[users], loc[pos + nu], loc[neg + nu]
    bpr = -torch.mean(torch.log(torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1)) + 1e-10))
    ln, gn = F.normalize(loc, dim=1), F.normalize(glo, dim=1)
    ssl = 0.0
    for idx in (torch.unique(users), torch.unique(pos + nu)):
        logits = ln[idx] @ gn[idx].t() / cfg["temp"]
        ssl = ssl + F.cross_entropy(logits, torch.arange(idx.numel()))
    reg = 0.5 * (Wu[users].pow(2).sum() + Wi[pos].pow(2).sum() + Wi[neg].pow(2).sum())
    return bpr, ssl, reg, bpr + cfg["lambda_ssl"] * ssl + cfg["lambda_reg"] * reg


def train(Wu0, Wi0, A, U, S, V, cfg, batches, lr):
    """Adam steps in float64 from (Wu0, Wi0): per step the losses, both gradients and both tables."""
    Wu = Wu0.double().clone().requires_grad_(True)
    Wi = Wi0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([Wu, Wi], lr=lr)
    out = []
    for users, pos, neg in batches:
        opt.zero_grad()
        bpr, ssl, reg, total = losses(Wu, Wi, A, U, S, V, cfg, users, pos, neg)
        total.backward()
        opt.step()
        out.append({"losses": tuple(float(t.detach()) for t in (bpr, ssl, reg, total)),
                    "grads": (Wu.grad.clone(), Wi.grad.clone()),
                    "params": (Wu.detach().clone(), Wi.detach().clone())})
    return out
