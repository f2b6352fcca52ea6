"""float64 reference of HybridUserTower's training pieces: the arithmetic of tests/hybrid_ref.py with the
dropout sites added, their keep masks rebuilt on the host (tests/dropout_ref.py) from the seeds that
ops.next_seed() drew. Everything is differentiable torch float64, so autograd gives the reference gradients.

Dropout sites in the order the training path draws their seeds:
  1. adapter content   2. adapter GNN   (index r * 128 + col over the T token rows)
  3. per encoder layer: attn, oproj, ffn, res
  4. fuse GNN          5. fuse meta     (index token_row * 128 + col)
`wrong=` names a site whose seed is shifted by one: the negative control.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import dropout_ref as DR
from tests import hybrid_ref as R

ADAPTER_KEYS = ("seq_adapter.content_proj.0.weight", "seq_adapter.content_proj.0.bias",
                "seq_adapter.content_proj.1.weight", "seq_adapter.content_proj.1.bias",
                "seq_adapter.gnn_proj.0.weight", "seq_adapter.gnn_proj.0.bias",
                "seq_adapter.gnn_proj.1.weight", "seq_adapter.gnn_proj.1.bias")


def draw_seeds(n, torch_seed):
    """The n seeds that n calls of ops.next_seed() give after torch.manual_seed(torch_seed): one int64 draw
    each from the default CPU generator. Restores the generator's state."""
    state = torch.random.get_rng_state()
    torch.manual_seed(torch_seed)
    from recsys_amd import ops
    seeds = [ops.next_seed() for _ in range(n)]
    torch.random.set_rng_state(state)
    return seeds


def rows_mask(seed, p, T, D=128):
    """[T, D] float64: keep / (1 - p) with the kernels' fp32 scale; ones at p = 0."""
    if p <= 0:
        return torch.ones(T, D, dtype=torch.float64)
    return torch.from_numpy(DR.rows_keep(seed, p, T, D).astype(np.float64) * float(DR.scale32(p)))


def _shift(seeds, wrong, name):
    return seeds[name] + (1 if wrong == name else 0)


def adapter(content, gnn, time_tab, ids, deltas, params, p=0.0, seeds=None, scale=math.sqrt(128.0), wrong=None):
    """seq_in [T, 128] (deltas given) or merged [T, 128]; params = the eight adapter tensors, float64.
    seeds: {"content": s, "gnn": s} when p > 0."""
    wc, bc, lcw, lcb, wg, bg, lgw, lgb = params
    ids = ids.reshape(-1)
    T = ids.numel()
    c, g = content[ids], gnn[ids]
    mc = rows_mask(_shift(seeds, wrong, "content"), p, T) if p > 0 else 1.0
    mg = rows_mask(_shift(seeds, wrong, "gnn"), p, T) if p > 0 else 1.0
    yc = R.gelu(R.layer_norm(c @ wc.T + bc, lcw, lcb)) * mc
    yg = R.gelu(R.layer_norm(g @ wg.T + bg, lgw, lgb)) * mg
    m = (yc + c) + yg
    if deltas is None:
        return m
    return m * scale + time_tab[deltas.reshape(-1).clamp(max=1000)]


def fuse(seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, p=0.0, seeds=None, wrong=None):
    """(out, v, gates [B, L, 2]); seeds: {"gnn": s, "meta": s} when p > 0. Each token row masks its own copy
    of the two projected rows."""
    B, L, D = seq_out.shape
    v = R.normalize(seq_out)
    g = torch.sigmoid(R.gelu(v @ w1.T + b1) @ w2.T + b2)
    a = u_gnn[:, None, :].expand(B, L, D)
    b = u_meta[:, None, :].expand(B, L, D)
    if p > 0:
        a = a * rows_mask(_shift(seeds, wrong, "gnn"), p, B * L).view(B, L, D)
        b = b * rows_mask(_shift(seeds, wrong, "meta"), p, B * L).view(B, L, D)
    fused = v + g[..., 0:1] * a + g[..., 1:2] * b
    return R.normalize(R.layer_norm(fused, ln_w, ln_b)), v, g


# ------------------------------------------------------------------------------------- the module
H, DH, LAYERS = R.HEADS, R.D // R.HEADS, R.LAYERS
P_ADAPTER, P_ENCODER, P_FUSE = 0.3, 0.3, 0.1


def site_names():
    names = ["adapter_content", "adapter_gnn"]
    for i in range(LAYERS):
        names += [f"attn{i}", f"oproj{i}", f"ffn{i}", f"res{i}"]
    return names + ["fuse_gnn", "fuse_meta"]


def module_seeds(torch_seed, training):
    """{site: seed} as the module's training path draws them after torch.manual_seed(torch_seed)."""
    names = site_names()
    if not training:
        return {n: 0 for n in names}
    return dict(zip(names, draw_seeds(len(names), torch_seed)))


def leaves(model):
    return {n: p.detach().cpu().double().requires_grad_() for n, p in model.named_parameters()}


def _mask(seed, p, idx):
    return torch.from_numpy(DR.keep(seed, p, idx).astype(np.float64) * float(DR.scale32(p)))


def encoder(P, x, mask, p, sd):
    """hybrid_ref.encoder with the four dropout sites per layer; x [B, L, 128]. Returns (x, the feed-forward
    pre-activations of every layer [LAYERS, B, L, 512])."""
    B, L, D = x.shape
    T = B * L
    allowed = torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & (mask != 0)[:, None, :]
    ones = p <= 0
    tok = np.arange(T).reshape(B, L)
    zs = []
    for i in range(LAYERS):
        pre = f"seq_encoder.layers.{i}."
        h = R.layer_norm(x, P[pre + "norm1.weight"], P[pre + "norm1.bias"])
        qkv = h @ P[pre + "self_attn.in_proj_weight"].T + P[pre + "self_attn.in_proj_bias"]
        q, k, v = (t.view(B, L, H, DH).transpose(1, 2) for t in qkv.split(D, dim=-1))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(DH)
        s = s.masked_fill(~allowed[:, None], float("-inf"))
        m = s.max(dim=-1, keepdim=True).values
        e = torch.where(allowed[:, None], torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))),
                        torch.zeros_like(s))
        den = e.sum(-1, keepdim=True)
        prob = e / torch.where(den > 0, den, torch.ones_like(den))
        if not ones:   # [B, L, H, L] -> [B, H, L, L]
            prob = prob * _mask(sd[f"attn{i}"], p, DR.attention_index(tok, H, L)).permute(0, 2, 1, 3)
        a = (prob @ v).transpose(1, 2).reshape(B, L, D)
        o = a @ P[pre + "self_attn.out_proj.weight"].T + P[pre + "self_attn.out_proj.bias"]
        x = x + (o if ones else o * _mask(sd[f"oproj{i}"], p, DR.rows_index(T, D)).view(B, L, D))
        h = R.layer_norm(x, P[pre + "norm2.weight"], P[pre + "norm2.bias"])
        z = h @ P[pre + "linear1.weight"].T + P[pre + "linear1.bias"]
        zs.append(z.detach())
        act = torch.relu(z)
        if not ones:
            act = act * _mask(sd[f"ffn{i}"], p, DR.gemm_index(T, 4 * D)).view(B, L, 4 * D)
        f = act @ P[pre + "linear2.weight"].T + P[pre + "linear2.bias"]
        x = x + (f if ones else f * _mask(sd[f"res{i}"], p, DR.rows_index(T, D)).view(B, L, D))
    return x, torch.stack(zs)


def module_forward(P, inp, training, seeds, wrong=None):
    """(output, v_seq, gates [B, L, 2], ffn pre-activations) of the module's training path in float64.
    P: leaves(model)."""
    sd = {n: (s + 1 if n == wrong else s) for n, s in seeds.items()}
    pa, pe, pf = (P_ADAPTER, P_ENCODER, P_FUSE) if training else (0.0, 0.0, 0.0)
    B, L = inp["seq_ids"].shape
    seq_in = adapter(P["item_content_emb.weight"], P["gnn_item_emb.weight"], P["time_emb.weight"], inp["seq_ids"],
                     inp["seq_deltas"], [P[k] for k in ADAPTER_KEYS], pa,
                     {"content": sd["adapter_content"], "gnn": sd["adapter_gnn"]})
    x, zs = encoder(P, seq_in.view(B, L, R.D), inp["seq_mask"], pe, sd)
    u_gnn, u_meta = R.user_side(P, inp["u_dense"], inp["u_cat"])
    out, v, g = fuse(x, u_gnn, u_meta, *R.gate_params(P), p=pf, seeds={"gnn": sd["fuse_gnn"], "meta": sd["fuse_meta"]})
    return out, v, g, zs
