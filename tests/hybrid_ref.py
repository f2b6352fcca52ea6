"""float64 restatement of HybridUserTower (tower_code/mined_inference.py of the reference) and the
seeded recipe behind tests/golden/hybrid_b5: the dual-table adapter, the norm-first ReLU encoder under
the causal mask plus the right-padding key mask, the per-user side, the sequence-centric fusion and the
gate means. Everything works on a state_dict, so it restates the arithmetic and shares no code with
the module under test.

One deliberate difference from the reference: a query that sees no key (a user without history) gets
an all-zero attention output instead of NaN, as the device path does.
"""
from __future__ import annotations

import json
import math
import os

import torch
import torch.nn as nn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D, HEADS, LAYERS = 128, 2, 4
LN_EPS, NORM_EPS = 1e-5, 1e-12

# ------------------------------------------------------------------------------------------ recipe
GOLDEN_SEED, N_ITEMS, N_USERS, GOLDEN_L = 20240607, 41, 6, 7
GOLDEN_LENGTHS = (7, 1, 3, 7, 5)


def make_tables(n_items=N_ITEMS, n_users=N_USERS, seed=GOLDEN_SEED):
    """(gnn_user [n_users, 64], gnn_item [n_items, 64], content [n_items, 128]) fp32, seeded."""
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(n_users, 64, generator=g), 0.5 * torch.randn(n_items, 64, generator=g),
            0.5 * torch.randn(n_items, 128, generator=g))


def overwrite_parameters(model, seed=GOLDEN_SEED + 1):
    """Every parameter of `model` redrawn from one torch.Generator, in named_parameters() order, so the
    weights do not depend on any module's own initialisation: LayerNorm weight 1 + 0.1 n and bias 0.1 n,
    embedding tables 0.5 n, matrices n / sqrt(fan_in), other vectors 0.1 n, scalars 2 + 0.1 n. The gate's
    last layer (weight 0, bias -5 after construction) is redrawn like any other Linear."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            owner = model.get_submodule(name.rpartition(".")[0]) if "." in name else model
            n = torch.randn(p.shape, generator=g)
            if isinstance(owner, nn.LayerNorm):
                v = 1.0 + 0.1 * n if name.endswith("weight") else 0.1 * n
            elif isinstance(owner, nn.Embedding):
                v = 0.5 * n
            elif p.dim() == 2:
                v = n / math.sqrt(p.shape[1])
            elif p.dim() == 1:
                v = 0.1 * n
            else:
                v = 2.0 + 0.1 * n
            p.copy_(v)
    return model


def build(cls, n_items=N_ITEMS, n_users=N_USERS, seed=GOLDEN_SEED):
    """cls = a HybridUserTower class (the reference's or this package's): manual_seed, construct,
    overwrite every parameter. eval mode."""
    gu, gi, ct = make_tables(n_items, n_users, seed)
    torch.manual_seed(seed)
    model = cls(n_users, n_items, gu, gi, ct)
    return overwrite_parameters(model, seed + 1).eval()


def make_inputs(B, L, lengths, n_items=N_ITEMS, n_users=N_USERS, seed=0, deltas_head=(0, 1000, 1001)):
    """Right-padded inputs: ids in [1, n_items) at valid positions and 0 after them, deltas in [0, 1200)
    with deltas_head written at the start of row 0, mask = (ids != 0), dense [B, 3], cat in {0, 1}."""
    g = torch.Generator().manual_seed(1000 + seed)
    ids = torch.randint(1, n_items, (B, L), generator=g)
    deltas = torch.randint(0, 1200, (B, L), generator=g)
    for j, d in enumerate(deltas_head[:L]):
        deltas[0, j] = d
    for b, n in enumerate(lengths):
        ids[b, n:] = 0
        deltas[b, n:] = 0
    return {"u_idx": torch.randint(0, n_users, (B,), generator=g), "seq_ids": ids, "seq_deltas": deltas,
            "seq_mask": (ids != 0).long(), "u_dense": torch.randn(B, 3, generator=g),
            "u_cat": torch.randint(0, 2, (B,), generator=g)}


def golden_inputs():
    return make_inputs(len(GOLDEN_LENGTHS), GOLDEN_L, GOLDEN_LENGTHS)


def checksums(state):
    """{name: [shape, sum, sum of |.|]} in float64."""
    return {k: [list(v.shape), float(v.double().sum()), float(v.double().abs().sum())] for k, v in state.items()}


def load_golden():
    from safetensors.torch import load_file
    with open(os.path.join(GOLD, "hybrid_b5.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLD, "hybrid_b5.safetensors")), meta


def check_recipe(state, meta):
    """The recipe still produces the recorded weights (names, shapes, float64 sums)."""
    want = meta["parameters"]
    assert list(state.keys()) == list(want.keys()), "state_dict names differ from the recorded list"
    for name, (shape, s, a) in want.items():
        got = state[name]
        assert list(got.shape) == shape, f"{name}: shape {list(got.shape)}, recorded {shape}"
        gs, ga = float(got.double().sum()), float(got.double().abs().sum())
        assert abs(gs - s) <= 1e-9 * max(1.0, a) and abs(ga - a) <= 1e-9 * max(1.0, a), (
            f"the seeded weight recipe drifted at {name}: sum {gs!r} / {s!r}, |sum| {ga!r} / {a!r}; "
            "tests/golden/hybrid_b5 was recorded with other weights")


# --------------------------------------------------------------------------------------- arithmetic
def f64(state):
    return {k: v.detach().cpu().double() for k, v in state.items()}


def layer_norm(x, w, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def normalize(x, eps=NORM_EPS):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def _branch(sd, prefix, x):
    return gelu(layer_norm(x @ sd[prefix + ".0.weight"].T + sd[prefix + ".0.bias"], sd[prefix + ".1.weight"],
                           sd[prefix + ".1.bias"]))


def adapter(sd, ids):
    """merged [*, 128] of item ids (any shape)."""
    c, g = sd["item_content_emb.weight"][ids], sd["gnn_item_emb.weight"][ids]
    return (_branch(sd, "seq_adapter.content_proj", c) + c) + _branch(sd, "seq_adapter.gnn_proj", g)


def seq_input(sd, ids, deltas):
    return adapter(sd, ids) * math.sqrt(D) + sd["time_emb.weight"][deltas.clamp(max=1000)]


def relu_ffn(x, w1, b1, w2, b2):
    return torch.relu(x @ w1.T + b1) @ w2.T + b2


def encoder(sd, x, mask):
    """Norm-first layers: x += out_proj(attn(norm1 x)); x += linear2(relu(linear1(norm2 x))). Key k is
    visible to query q when k <= q and mask[b, k] != 0; a query without a visible key attends to nothing."""
    B, L, _ = x.shape
    Dh = D // HEADS
    allowed = torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & (mask != 0)[:, None, :]
    for i in range(LAYERS):
        p = f"seq_encoder.layers.{i}."
        h = layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        qkv = h @ sd[p + "self_attn.in_proj_weight"].T + sd[p + "self_attn.in_proj_bias"]
        q, k, v = (t.view(B, L, HEADS, Dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(Dh)
        s = s.masked_fill(~allowed[:, None], float("-inf"))
        m = s.max(dim=-1, keepdim=True).values
        e = torch.where(allowed[:, None], torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))),
                        torch.zeros_like(s))
        den = e.sum(-1, keepdim=True)
        a = (e / torch.where(den > 0, den, torch.ones_like(den))) @ v
        a = a.transpose(1, 2).reshape(B, L, D)
        x = x + a @ sd[p + "self_attn.out_proj.weight"].T + sd[p + "self_attn.out_proj.bias"]
        h = layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
        x = x + relu_ffn(h, sd[p + "linear1.weight"], sd[p + "linear1.bias"], sd[p + "linear2.weight"],
                         sd[p + "linear2.bias"])
    return x


def user_side(sd, u_dense, u_cat):
    """(U_gnn, U_meta) [B, 128]: the fusion's two projections of the per-user vectors. The GNN user
    vector is zero in the reference, so U_gnn = LayerNorm(gnn_proj's bias) for every user."""
    B = u_dense.shape[0]
    x = torch.cat([u_dense.double(), sd["channel_emb.weight"][u_cat]], dim=1)
    h = gelu(x @ sd["meta_mlp.0.weight"].T + sd["meta_mlp.0.bias"])
    v_meta = normalize(layer_norm(h @ sd["meta_mlp.2.weight"].T + sd["meta_mlp.2.bias"], sd["meta_mlp.3.weight"],
                                  sd["meta_mlp.3.bias"]))
    f = "fusion_layer."
    u_meta = layer_norm(v_meta @ sd[f + "meta_proj.0.weight"].T + sd[f + "meta_proj.0.bias"],
                        sd[f + "meta_proj.1.weight"], sd[f + "meta_proj.1.bias"])
    zero = torch.zeros(B, D, dtype=torch.float64)
    u_gnn = layer_norm(zero @ sd[f + "gnn_proj.0.weight"].T + sd[f + "gnn_proj.0.bias"], sd[f + "gnn_proj.1.weight"],
                       sd[f + "gnn_proj.1.bias"])
    return u_gnn, u_meta


def fuse(seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b):
    """seq_out [B, L, 128] -> (out, v, gates [B, L, 2]), everything float64."""
    v = normalize(seq_out)
    g = torch.sigmoid(gelu(v @ w1.T + b1) @ w2.T + b2)
    fused = v + g[..., 0:1] * u_gnn[:, None, :] + g[..., 1:2] * u_meta[:, None, :]
    return normalize(layer_norm(fused, ln_w, ln_b)), v, g


def gate_params(sd):
    f = "fusion_layer."
    return (sd[f + "context_gate.0.weight"], sd[f + "context_gate.0.bias"], sd[f + "context_gate.2.weight"],
            sd[f + "context_gate.2.bias"], sd[f + "final_ln.weight"], sd[f + "final_ln.bias"])


def forward(sd, inp):
    """(output [B, L, 128], v_seq [B, L, 128], [gnn_ratio, meta_ratio]): the ratios are means over all
    B L positions, padded ones included."""
    x = encoder(sd, seq_input(sd, inp["seq_ids"], inp["seq_deltas"]), inp["seq_mask"])
    u_gnn, u_meta = user_side(sd, inp["u_dense"], inp["u_cat"])
    out, v, g = fuse(x, u_gnn, u_meta, *gate_params(sd))
    return out, v, [float(g[..., 0].mean()), float(g[..., 1].mean())]


def valid(mask):
    return mask != 0
