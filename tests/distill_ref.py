"""Float64 reference of the projector's distillation (gnn_model/distill_mag_to_cos_l2.py): the forward,
the MSE against the teacher's dot products, the hand-derived backward and an Adam loop, with the
dropout keep masks passed in (tests/dropout_ref rebuilds them from a step's seed). Helper, not a test.

Stacked rows X = [U[users]; I[items]] ([2B, 64], users first), params = (w1, b1, w2, b2, logit_scale):
  P = X W1^T + b1; A = P > 0 ? P : slope P; H = A keep / (1 - p); Z = H W2^T + b2; n = max(|Z_r|, eps);
  Y = Z / n; s_k = <Y_k, Y_{B+k}> exp(ls); t_k = <X_k, X_{B+k}>; loss = sum_k (s_k - t_k)^2 / div.
"""
from __future__ import annotations

import torch

from tests import dropout_ref as DR

HID = 128


def make_tables(num_users, num_items, seed):
    """Seeded fp32 teacher tables: unit directions times a log-normal length 2 exp(0.5 N(0, 1)); item
    row 0 is the all-zero padding row. Teacher scores span several units."""
    g = torch.Generator().manual_seed(seed)

    def table(n):
        d = torch.randn(n, 64, generator=g, dtype=torch.float64)
        d = d / d.norm(dim=1, keepdim=True)
        return (d * (2.0 * torch.exp(0.5 * torch.randn(n, 1, generator=g, dtype=torch.float64)))).float()

    U, I = table(num_users), table(num_items)
    I[0] = 0.0
    return U, I


def stack(U, I, users, items):
    return torch.cat([U[users], I[items]]).double()


def keep_scale(seed, p, B):
    """keep / (1 - p) of a step, [2B, 128] float64 (None at p = 0): the kernel's mask at index
    r * 128 + c over the stacked row r, times its fp32 scale."""
    if p <= 0:
        return None
    return torch.from_numpy(DR.rows_keep(seed, p, 2 * B, HID)).double() * float(DR.scale32(p))


def forward(X, params, slope=0.2, ks=None, eps=1e-12):
    w1, b1, w2, b2, _ = (t.double() for t in params)
    P = X @ w1.t() + b1
    A = torch.where(P > 0, P, slope * P)
    H = A if ks is None else A * ks
    Z = H @ w2.t() + b2
    nz = Z.norm(dim=1, keepdim=True)
    n = nz.clamp(min=eps)
    return P, H, Z, nz, n, Z / n


def compose(X, params, slope=0.2, ks=None, eps=1e-12, div=None):
    """The loss as a composition of torch ops (for autograd in float64)."""
    w1, b1, w2, b2, ls = params
    B = X.shape[0] // 2
    h = torch.nn.functional.leaky_relu(X @ w1.t() + b1, slope)
    if ks is not None:
        h = h * ks
    y = torch.nn.functional.normalize(h @ w2.t() + b2, p=2, dim=1, eps=eps)
    s = (y[:B] * y[B:]).sum(1) * ls.exp()
    t = (X[:B] * X[B:]).sum(1)
    return ((s - t) ** 2).sum() / (div or B)


def step(X, params, slope=0.2, ks=None, eps=1e-12, div=None):
    """Loss, the five gradients by the hand-derived backward, both score vectors and the unit rows.
    div: the divisor of the mean (default B; the kernel keeps the full batch size when it drops a
    pair with an out-of-range id)."""
    w1, b1, w2, b2, ls = (t.double() for t in params)
    B = X.shape[0] // 2
    div = float(div or B)
    P, H, Z, nz, n, Y = forward(X, params, slope, ks, eps)
    els = ls.exp()
    s = (Y[:B] * Y[B:]).sum(1) * els
    t = (X[:B] * X[B:]).sum(1)
    loss = ((s - t) ** 2).sum() / div
    ds = 2.0 * (s - t) / div
    dls = (ds * s).sum()
    dY = torch.cat([ds[:, None] * els * Y[B:], ds[:, None] * els * Y[:B]])
    dZ = torch.where(nz >= eps, (dY - Y * (Y * dY).sum(1, keepdim=True)) / n, dY / eps)
    dW2, db2 = dZ.t() @ H, dZ.sum(0)
    dH = dZ @ w2
    dP = dH * torch.where(P > 0, torch.ones_like(P), torch.full_like(P, slope))
    if ks is not None:
        dP = dP * ks
    dW1, db1 = dP.t() @ X, dP.sum(0)
    return {"loss": loss, "grads": (dW1, db1, dW2, db2, dls), "student": s, "teacher": t, "rows": Y}


def adam_train(params, batches, slope=0.2, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, eps=1e-12):
    """torch.optim.Adam's steps in float64 over batches of (X, ks, div): per step the loss, the
    gradients and the parameters after the update."""
    ps = [t.double().clone() for t in params]
    m = [torch.zeros_like(t) for t in ps]
    v = [torch.zeros_like(t) for t in ps]
    out = []
    for k, (X, ks, div) in enumerate(batches, start=1):
        r = step(X, ps, slope, ks, eps, div)
        for i, g in enumerate(r["grads"]):
            m[i] = betas[0] * m[i] + (1 - betas[0]) * g
            v[i] = betas[1] * v[i] + (1 - betas[1]) * g * g
            denom = v[i].sqrt() / (1 - betas[1] ** k) ** 0.5 + adam_eps
            ps[i] = ps[i] - lr / (1 - betas[0] ** k) * m[i] / denom
        out.append({"loss": float(r["loss"]), "grads": r["grads"], "params": [t.clone() for t in ps]})
    return out
