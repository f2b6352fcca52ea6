"""Float64 restatement of SASRecUserTower.forward_packed (tower_code/v1_refine_usertower.py, the
per-op path: static profile, item_proj, embedding stage, norm_first encoder stack, output head)
with every dropout site taking a keep-mask rebuilt on the host (tests/dropout_ref.py). Plain
torch on the CPU; autograd gives the gradients.

Dropout sites, their seeds and index maps (ops._TowerPacked, csrc/tower.hip rsx_tower_fwd; the
per-op path draws the same seeds in the same order through ops.next_seed):

  draw        site                                     index map (rows = packed token rows)
  0           "profile"  static profile output          r * 128 + c over the 2B profile rows
  1           "embed"    seeds[0]: LayerNorm'd embeds   r * 128 + c
  2 + 4i      "attn{i}"  sd[0]: attention probabilities ((tok * 4 + h) * 64 + k), tok = the query's packed
                                                        row, k = the key's position in its segment
  3 + 4i      "oproj{i}" sd[1]: x + drop(out_proj(a))   r * 128 + c
  4 + 4i      "ffn{i}"   sd[2]: drop(gelu(linear1))     r * 256 + n
  5 + 4i      "res{i}"   sd[3]: x + drop(ffn)           r * 128 + c

Tail form (tail_last given; tower.hip:13-16, :354-371): in the LAST layer the attention keeps its
keys (packed query row, so view 2's last query T1 + last[j] draws the all-rows program's mask),
while "oproj", "ffn" and "res" run on the R = T1 + B kept rows and key them by the kept row's own
index r in [0, R): view 1's rows keep r = packed row, view 2's last row of user j is r = T1 + j.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import dropout_ref as R

H, DH, D = 4, 32, 128


def site_names(layers):
    names = ["profile", "embed"]
    for i in range(layers):
        names += [f"attn{i}", f"oproj{i}", f"ffn{i}", f"res{i}"]
    return names


def draw_seeds(torch_seed, layers, p):
    """The seeds the device draws after torch.manual_seed(torch_seed): one per site, in site_names
    order, through the same generator call as ops.next_seed (none are drawn at p = 0)."""
    names = site_names(layers)
    if p <= 0:
        return {n: 0 for n in names}
    torch.manual_seed(torch_seed)
    return {n: int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) for n in names}


def _mask(seed, p, idx):
    """float64 keep-mask * float64(scale32(p)) for an index array."""
    return torch.from_numpy(R.keep(seed, p, idx).astype(np.float64) * float(R.scale32(p)))


def host_index(pk2, tok_ids, pv, static, tail_last=None):
    """CPU copies of the packed index the device run used."""
    c = lambda t: t.detach().cpu()
    return {
        "tok_user": c(pk2.tok_user).long(), "tok_pos": c(pk2.tok_pos).long(), "tok_pad": c(pk2.tok_pad).bool(),
        "seg": c(pk2.seg_off64).long(), "tok_ids": [c(t).long() for t in tok_ids], "pv": c(pv).double(),
        "static_ids": [c(t).long() for t in static[:9]], "cont": c(static[9]).double(),
        "last": None if tail_last is None else c(tail_last).long(),
    }


def leaves(model):
    """The module's parameters as float64 CPU leaves, by name."""
    return {n: p.detach().cpu().double().requires_grad_() for n, p in model.named_parameters()}


def _ln(x, P, name, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), P[name + ".weight"], P[name + ".bias"], eps)


def _profile(P, ix, rows, p, seed):
    u_g = torch.sigmoid(P["static_gate"])
    embs = ["age_emb", "price_emb", "cnt_emb", "recency_emb", "channel_emb", "club_status_emb", "news_freq_emb",
            "fn_emb", "active_emb"]
    parts = [F.embedding(i, P[e + ".weight"], padding_idx=0) * u_g[j]
             for j, (i, e) in enumerate(zip(ix["static_ids"], embs))]
    parts.append(F.relu(F.linear(ix["cont"], P["cont_proj.weight"], P["cont_proj.bias"])) * u_g[9])
    h = F.linear(torch.cat(parts, 1), P["static_mlp.0.weight"], P["static_mlp.0.bias"])
    y = F.gelu(_ln(h, P, "static_mlp.1"))
    B = y.shape[0]
    y = y[torch.arange(rows) % B]                       # output row r reads user r % B (both views)
    return y * _mask(seed, p, R.rows_index(rows, D))


def _attention(qkv, ix, p, seed):
    """Causal + key-padding attention over the packed segments with dropout on the probabilities:
    P = softmax(masked scores), Pd = P * keep * scale, out = Pd @ V. A query without an allowed key
    gets a zero row."""
    seg, user = ix["seg"], ix["tok_user"]
    T = qkv.shape[0]
    U = seg.numel() - 1
    lens = seg[1:] - seg[:-1]
    Lm = int(lens.max())
    pos = torch.arange(T) - seg[user]                   # position inside the segment
    slot = user * Lm + pos
    pad_q = torch.zeros(U * Lm, 3 * D, dtype=qkv.dtype).index_add(0, slot, qkv).view(U, Lm, 3 * D)
    q, k, v = (t.view(U, Lm, H, DH).transpose(1, 2) for t in pad_q.split(D, -1))
    s = q @ k.transpose(-1, -2) / math.sqrt(DH)          # [U, H, Lm, Lm]
    key_ok = torch.zeros(U * Lm, dtype=torch.bool)
    key_ok[slot] = ~ix["tok_pad"]
    key_ok = key_ok.view(U, 1, 1, Lm)
    allowed = key_ok & torch.tril(torch.ones(Lm, Lm, dtype=torch.bool))[None, None]
    s = s.masked_fill(~allowed, float("-inf"))
    dead = ~allowed.any(-1, keepdim=True)
    s = s.masked_fill(dead, 0.0)
    prob = torch.softmax(s, -1) * allowed
    tok = (seg[:-1, None] + torch.arange(Lm)[None, :]).numpy()          # packed row of (u, i)
    m = _mask(seed, p, R.attention_index(tok, H, Lm)).permute(0, 2, 1, 3)  # [U, Lm, H, Lm] -> [U, H, Lm, Lm]
    out = ((prob * m) @ v).transpose(1, 2).reshape(U * Lm, D)
    return out[slot]


def forward(P, ix, layers, p, seeds, wrong=None):
    """Output rows [T, 128] (all packed rows), or [T1 + B, 128] in the tail form (ix["last"] set).
    wrong: a site name whose mask is drawn from seed + 1 instead (the negative controls)."""
    sd = {n: (s + 1 if n == wrong else s) for n, s in seeds.items()}
    T = ix["pv"].shape[0]
    U = ix["seg"].numel() - 1
    prof = _profile(P, ix, U, p, sd["profile"])
    s_g = torch.sigmoid(P["seq_gate"]) * torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    x = F.linear(ix["pv"], P["item_proj.weight"], P["item_proj.bias"])
    tabs = ["item_id_emb", "time_emb", "type_emb", "color_emb", "graphic_emb", "section_emb"]
    for j, (name, ids) in enumerate(zip(tabs, ix["tok_ids"])):
        x = x + F.embedding(ids, P[name + ".weight"], padding_idx=0) * s_g[j]
    x = x + P["pos_emb.weight"][ix["tok_pos"]]
    x = _ln(x, P, "emb_ln") * _mask(sd["embed"], p, R.rows_index(T, D))
    tail = ix["last"] is not None
    rows, user = T, ix["tok_user"]
    h = _ln(x, P, "transformer_encoder.layers.0.norm1")
    for i in range(layers):
        L = f"transformer_encoder.layers.{i}."
        qkv = F.linear(h, P[L + "self_attn.in_proj_weight"], P[L + "self_attn.in_proj_bias"])
        a = _attention(qkv, ix, p, sd[f"attn{i}"])
        if tail and i == layers - 1:                    # the kept rows; per-row masks by their own index
            T1, B = T // 2, U // 2
            keep_rows = torch.cat([torch.arange(T1), T1 + ix["last"]])
            a, x = a[keep_rows], x[keep_rows]
            rows = T1 + B
            user = torch.cat([ix["tok_user"][:T1], B + torch.arange(B)])
        o = F.linear(a, P[L + "self_attn.out_proj.weight"], P[L + "self_attn.out_proj.bias"])
        x = x + o * _mask(sd[f"oproj{i}"], p, R.rows_index(rows, D))
        h2 = _ln(x, P, L + "norm2")
        act = F.gelu(F.linear(h2, P[L + "linear1.weight"], P[L + "linear1.bias"]))
        act = act * _mask(sd[f"ffn{i}"], p, R.gemm_index(rows, 2 * D))
        f = F.linear(act, P[L + "linear2.weight"], P[L + "linear2.bias"])
        x = x + f * _mask(sd[f"res{i}"], p, R.rows_index(rows, D))
        if i + 1 < layers:
            h = _ln(x, P, f"transformer_encoder.layers.{i + 1}.norm1")
    hp = F.linear(torch.cat([x, prof[user]], 1), P["output_proj.0.weight"], P["output_proj.0.bias"])
    g = F.gelu(_ln(hp, P, "output_proj.1"))
    return F.normalize(F.linear(g, P["output_proj.3.weight"], P["output_proj.3.bias"]), dim=1)


def run(model, ix, layers, p, seeds, w, wrong=None):
    """(output, {parameter name: gradient}) of sum(out * w) in float64."""
    P = leaves(model)
    out = forward(P, ix, layers, p, seeds, wrong)
    (out * w.double()).sum().backward()
    return out.detach(), {n: (t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in P.items()}
