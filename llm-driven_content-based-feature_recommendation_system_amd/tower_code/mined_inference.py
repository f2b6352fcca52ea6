"""Drop-in for tower_code/mined_inference.py: HybridUserTower (the sequence model over content and GNN item
rows with a gated fusion of per-user vectors; defined below, before the evaluators) and the ensemble
evaluators: late fusion of the sequence retriever and the GNN retriever over an alpha sweep, on the device.

Reference (tower_code/mined_inference.py): evaluate_multi_vector_ensemble :797-993,
evaluate_weighted_score_ensemble :996-1227 (the live entry point of main, :1669-1678),
evaluate_rrf_ensemble :1238-1448.

Departure from the reference signature: the reference took `seq_model, processor, target_df_path` and
the GNN tables, ran the sequence model over a DataLoader and read the targets from a parquet file. These
evaluators work at the vector level: they take the user and item vectors of both retrievers (rows of
one user / one item in the same position in both spaces) and `ground_truth`, a dict from a user row to
the set of its item rows (0-based into the item matrices), as gnn_model.v1_evaluate_lightgcl.
evaluate_recall does. Any tower produces the vectors: encode_users / hybrid_item_vectors of
HybridUserTower as in the reference's main, or SASRecUserTower, with the distilled LightGCL tables
(gnn_model.distill_mag_to_cos_l2) on the GNN side. They return the whole sweep, not only the best alpha:
{"best_alpha", "hits": {alpha: {k: users hit}}, "recall": {alpha: {k: hits / users}}, "users"}.
alpha weighs the GNN retriever, 1 - alpha the sequence retriever.

Compute: on corpora of at least FUSED_POOL_MIN_ITEMS items each retriever's pools come from
ops.retrieve_topk (the fused bf16 scan with exact rescoring: no score matrix, chunks of batch_size
users); on smaller ones, per chunk of users the two score matrices come from fp32 torch.matmul and each
pool from ops.select_topk_rows. The fusion, the alpha sweep and the hit test of the chunk from one
ops.fuse_rank launch (csrc/ensemble.hip); the ratio merge takes two ops.retrieve_topk lists and two
ops.first_hit. Hit counts accumulate on the device and are read once per evaluation. One clamp is ours:
the number of fused entries kept, max_k + 20 in the reference, is min(pool entries, max_k + 20) (torch.topk
would raise there). There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pad_sequence

from .. import ops
from .v1_refine_usertower import encoder_stack

SCORE_CHUNK_BYTES = 512 << 20   # bound of one [users, items] fp32 score matrix
# Corpus size from which _evaluate_fused takes its pools from ops.retrieve_topk (the fused bf16 scan
# for pools above 512) and not from a materialised score matrix: the smallest measured size from which
# the fused form's range lies wholly below the materialised form's (profiles/ensemble_pool_switch.json,
# DESIGN.md section 4), and never below the smallest corpus the scan's plan serves at these pools.
FUSED_POOL_MIN_ITEMS = 131_072
DROPOUT = 0.3                   # the reference's module constant (:30)


# ----------------------------------------------------------------------------------------
# HybridUserTower (:607-734) with its ParallelAdapter (:582-602) and SequenceCentricFusion (:514-577):
# the model whose vectors are the sequence side of the evaluators below. In eval mode with gradients
# off on the device it runs on csrc/hybrid.hip, the bf16x3 encoder stack (ReLU feed-forward) and
# ops.linear / layer_norm / l2_normalize; with gradients or in training mode on the device it runs on
# the training forms of the same kernels (ops.hybrid_adapter_train, encoder_stack, ops.hybrid_fuse_train)
# unless native_training is False; in every other case (CPU, other widths, L > 64) the plain PyTorch
# composition of the same modules runs. See DESIGN.md, section 4.
def user_tower_collate_fn(batch):
    """The reference's collate (:180-189): sequences RIGHT-padded with 0 by pad_sequence, seq_mask =
    (seq_ids != 0), last_target = each sample's last target id (0 without targets)."""
    stack = lambda k: torch.stack([b[k] for b in batch])  # noqa: E731
    pad = lambda k: pad_sequence([b[k] for b in batch], batch_first=True, padding_value=0)  # noqa: E731
    seq_ids, seq_deltas, target_ids = pad("seq_ids"), pad("seq_deltas"), pad("target_ids")
    last_target = torch.tensor([b["target_ids"][-1] if len(b["target_ids"]) > 0 else 0 for b in batch],
                               dtype=torch.long)
    return (stack("user_idx"), stack("user_dense"), stack("user_cat"), seq_ids, seq_deltas, (seq_ids != 0).long(),
            target_ids, last_target)


class SequenceCentricFusion(nn.Module):
    """v_seq + g_gnn gnn_proj(v_gnn) + g_meta meta_proj(v_meta) under final_ln: the sequence vector keeps
    weight 1 and gates, by a sigmoid MLP of itself, how much of the two per-user vectors is added
    (:514-577). The gate's last layer starts at weight 0, bias -5 (sigmoid(-5) ~ 0.007)."""

    def __init__(self, dim=128):
        super().__init__()
        self.context_gate = nn.Sequential(nn.Linear(dim, 64), nn.GELU(), nn.Linear(64, 2), nn.Sigmoid())
        self.gnn_proj = nn.Sequential(nn.Linear(dim, dim), nn.LayerNorm(dim), nn.Dropout(0.1))
        self.meta_proj = nn.Sequential(nn.Linear(dim, dim), nn.LayerNorm(dim), nn.Dropout(0.1))
        self.final_ln = nn.LayerNorm(dim)
        nn.init.zeros_(self.context_gate[-2].weight)
        nn.init.constant_(self.context_gate[-2].bias, -5.0)

    def forward(self, v_gnn, v_seq, v_meta):
        gates = self.context_gate(v_seq)
        g_gnn, g_meta = gates[..., 0:1], gates[..., 1:2]
        fused = v_seq + (g_gnn * self.gnn_proj(v_gnn)) + (g_meta * self.meta_proj(v_meta))
        # the means run over every position, padded ones included, as the reference's
        return self.final_ln(fused), [g_gnn.mean().item(), g_meta.mean().item()]


class ParallelAdapter(nn.Module):
    """(content_proj(c) + c) + gnn_proj(g): two Linear -> LayerNorm -> GELU -> Dropout branches over an
    item's content row and its GNN row, the content row kept as a residual (:582-602)."""

    def __init__(self, content_dim=128, gnn_dim=64, out_dim=128, dropout=0.2):
        super().__init__()
        self.content_proj = nn.Sequential(nn.Linear(content_dim, out_dim), nn.LayerNorm(out_dim), nn.GELU(),
                                          nn.Dropout(dropout))
        self.gnn_proj = nn.Sequential(nn.Linear(gnn_dim, out_dim), nn.LayerNorm(out_dim), nn.GELU(),
                                      nn.Dropout(dropout))

    def forward(self, v_content, v_gnn):
        return (self.content_proj(v_content) + v_content) + self.gnn_proj(v_gnn)

    def native_params(self):
        c, g = self.content_proj, self.gnn_proj
        return ops.AdapterParams(c[0].weight, c[0].bias, c[1].weight, c[1].bias, g[0].weight, g[0].bias, g[1].weight,
                                 g[1].bias, c[1].eps)


class HybridUserTower(nn.Module):
    """Reference :607-734; construction order, sub-module names and state_dict as there."""

    native_training = True   # False: calls with gradients / in training mode take the PyTorch composition

    def __init__(self, num_users, num_items, gnn_user_init, gnn_item_init, item_content_init):
        super().__init__()
        self.embed_dim = 128
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.gnn_user_emb = nn.Embedding.from_pretrained(gnn_user_init, freeze=False)
        self.gnn_item_emb = nn.Embedding.from_pretrained(gnn_item_init, freeze=False)
        self.item_content_emb = nn.Embedding.from_pretrained(item_content_init, freeze=False)
        self.gnn_projector = nn.Sequential(
            nn.Linear(gnn_user_init.shape[1], 256), nn.LayerNorm(256), nn.GELU(), nn.Dropout(DROPOUT),
            nn.Linear(256, 128), nn.LayerNorm(128))
        self.seq_adapter = ParallelAdapter(content_dim=128, gnn_dim=64, out_dim=128, dropout=DROPOUT)
        self.time_emb = nn.Embedding(1001, 128)
        # no activation=: the layers' feed-forward is ReLU
        encoder_layer = nn.TransformerEncoderLayer(d_model=128, nhead=2, dim_feedforward=512, dropout=DROPOUT,
                                                   batch_first=True, norm_first=True)
        self.seq_encoder = nn.TransformerEncoder(encoder_layer, num_layers=4, enable_nested_tensor=False)
        self.channel_emb = nn.Embedding(2, 32)
        self.meta_mlp = nn.Sequential(nn.Linear(35, 128), nn.GELU(), nn.Linear(128, 128), nn.LayerNorm(128))
        self.fusion_layer = SequenceCentricFusion(dim=128)

    def get_current_temperature(self, clamp_min):
        """1 / clamp(exp(logit_scale), clamp_min, 100) (:652-664)."""
        return 1.0 / self.logit_scale.exp().clamp(clamp_min, max=100.0)

    def get_meta_feature_importance(self):
        """Shares of the mean |weight| of meta_mlp[0] over the column ranges the reference names
        (:712-734): 0:32, 32:64, 64:96, 96:112 (ranges past the layer's 35 inputs are empty there too)."""
        w = self.meta_mlp[0].weight.abs().detach().cpu()
        imp = {"Price": w[:, 0:32].mean().item(), "Count": w[:, 32:64].mean().item(),
               "Recency": w[:, 64:96].mean().item(), "Channel": w[:, 96:112].mean().item()}
        total = sum(imp.values()) + 1e-9
        return {k: v / total for k, v in imp.items()}

    # -- dispatch ---------------------------------------------------------------------------
    def native_ok(self, seq_ids):
        """The device path: eval mode, gradients off, device tensors, the reference's widths, L <= 64."""
        return not self.training and not torch.is_grad_enabled() and self._native_shapes(seq_ids)

    def native_train_ok(self, seq_ids):
        """The device path with gradients: as native_ok where that is false only because gradients are
        on or the module is in training mode (and native_training is left True)."""
        return (self.native_training and (self.training or torch.is_grad_enabled())
                and self._native_shapes(seq_ids))

    def _native_shapes(self, seq_ids):
        layer = self.seq_encoder.layers[0]
        return (seq_ids.is_cuda
                and self.item_content_emb.weight.is_cuda and seq_ids.dim() == 2
                and 1 <= seq_ids.shape[1] <= ops.HYBRID_MAX_LEN
                and self.item_content_emb.weight.shape[1] == 128 and self.gnn_item_emb.weight.shape[1] == 64
                and self.item_content_emb.weight.dtype == torch.float32
                and layer.self_attn.num_heads == 2 and layer.linear1.out_features == 512
                and layer.self_attn.embed_dim == 128)

    # -- the PyTorch composition (training, gradients, CPU) ------------------------------------
    def _torch_seq_out(self, seq_ids, seq_deltas, seq_mask):
        L = seq_ids.shape[1]
        seq_input = self.seq_adapter(self.item_content_emb(seq_ids), self.gnn_item_emb(seq_ids))
        seq_input = seq_input * math.sqrt(self.embed_dim) + self.time_emb(seq_deltas.clamp(max=1000))
        causal = torch.triu(torch.full((L, L), float("-inf"), device=seq_ids.device), diagonal=1)
        pad = seq_mask == 0
        if bool(pad.all(dim=1).any()):
            # a user without history: the reference's softmax over no key gives NaN; here such a row
            # attends to nothing, as on the device path (csrc/mha.hip: a fully masked query gives zeros)
            return self._torch_encoder_masked(seq_input, pad)
        # the key mask as floats, which is what the encoder makes of the reference's boolean one
        key_mask = torch.zeros_like(pad, dtype=causal.dtype).masked_fill(pad, float("-inf"))
        return self.seq_encoder(seq_input, mask=causal, src_key_padding_mask=key_mask)

    def _torch_encoder_masked(self, x, pad):
        """The norm_first ReLU stack written out, with softmax rows that see no key set to zero."""
        B, L, D = x.shape
        allowed = torch.tril(torch.ones(L, L, dtype=torch.bool, device=x.device))[None] & ~pad[:, None, :]   # [B, q, k]
        for layer in self.seq_encoder.layers:
            sa = layer.self_attn
            H, Dh = sa.num_heads, D // sa.num_heads
            h = layer.norm1(x)
            q, k, v = F.linear(h, sa.in_proj_weight, sa.in_proj_bias).view(B, L, 3, H, Dh).permute(2, 0, 3, 1, 4)
            s = (q @ k.transpose(-1, -2)) / math.sqrt(Dh)
            has_key = allowed[:, None].any(-1, keepdim=True)
            s = torch.where(has_key, s.masked_fill(~allowed[:, None], float("-inf")), torch.zeros_like(s))
            p = F.dropout(torch.softmax(s, dim=-1) * has_key, sa.dropout, self.training)
            a = (p @ v).permute(0, 2, 1, 3).reshape(B, L, D)
            x = x + layer.dropout1(sa.out_proj(a))
            x = x + layer.dropout2(layer.linear2(layer.dropout(F.relu(layer.linear1(layer.norm2(x))))))
        return x

    def _torch_user_side(self, u_idx, u_dense, u_cat):
        v_gnn = F.normalize(self.gnn_projector(self.gnn_user_emb(u_idx)), p=2, dim=1)
        v_gnn = torch.zeros_like(v_gnn)   # reference :672: the GNN user vector is replaced by zeros
        if self.training:                 # :673-681 (a scaled mask over zeros: still zeros)
            keep = torch.bernoulli(torch.full((v_gnn.shape[0], 1), 0.6, device=v_gnn.device))
            v_gnn = (v_gnn * keep) / 0.6
        v_meta = self.meta_mlp(torch.cat([u_dense, self.channel_emb(u_cat)], dim=1))
        return v_gnn, F.normalize(v_meta, p=2, dim=1)

    def _torch_forward(self, u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat):
        L = seq_ids.shape[1]
        v_gnn, v_meta = self._torch_user_side(u_idx, u_dense, u_cat)
        v_seq = F.normalize(self._torch_seq_out(seq_ids, seq_deltas, seq_mask), p=2, dim=2)
        output, gates = self.fusion_layer(v_gnn.unsqueeze(1).expand(-1, L, -1), v_seq,
                                          v_meta.unsqueeze(1).expand(-1, L, -1))
        return F.normalize(output, p=2, dim=2), v_seq, gates

    # -- the device path ------------------------------------------------------------------------
    def _native_seq_out(self, seq_ids, seq_deltas, seq_mask, merged=None):
        B, L = seq_ids.shape
        scale = math.sqrt(self.embed_dim)
        if merged is None:
            _, _, seq_in = ops.hybrid_adapter(self.item_content_emb.weight, self.gnn_item_emb.weight,
                                              self.seq_adapter.native_params(), ids=seq_ids, deltas=seq_deltas,
                                              time_tab=self.time_emb.weight, scale=scale, want_merged=False)
        else:
            first_row = self.item_content_emb.weight.shape[0] - merged.shape[0]
            if first_row < 0:
                raise ValueError(f"merged has {merged.shape[0]} rows, the item table {merged.shape[0] + first_row}")
            seq_in = ops.hybrid_seq_gather(merged, seq_ids, seq_deltas, self.time_emb.weight, scale=scale,
                                           first_row=first_row)
        return encoder_stack(self.seq_encoder.layers, seq_in.view(B, L, self.embed_dim), seq_mask == 0, 0.0, False,
                             causal=True, act="relu")

    def _native_user_side(self, u_idx, u_dense, u_cat):
        """(U_gnn, U_meta) [B, 128]: gnn_proj / meta_proj of the fusion applied to the per-user vectors.
        The GNN vector is zero (:672), so its row is LayerNorm(gnn_proj's bias) for every user."""
        B = u_idx.shape[0]
        fl = self.fusion_layer
        gp, mp = fl.gnn_proj, fl.meta_proj
        u_gnn = ops.layer_norm(gp[0].bias.detach().view(1, -1), gp[1].weight, gp[1].bias, gp[1].eps).expand(B, -1)
        m0, m2, mln = self.meta_mlp[0], self.meta_mlp[2], self.meta_mlp[3]
        x = torch.cat([u_dense.to(torch.float32), self.channel_emb(u_cat)], dim=1)
        k_pad = (-x.shape[1]) % 4                   # ops.linear reads K in multiples of 4: zero columns
        h = ops.linear(F.pad(x, (0, k_pad)), F.pad(m0.weight.detach(), (0, k_pad)), m0.bias, ops.ACT_GELU)
        v_meta = ops.l2_normalize(ops.layer_norm(ops.linear(h, m2.weight, m2.bias), mln.weight, mln.bias, mln.eps))
        u_meta = ops.layer_norm(ops.linear(v_meta, mp[0].weight, mp[0].bias), mp[1].weight, mp[1].bias, mp[1].eps)
        return u_gnn.contiguous(), u_meta

    def _native_fuse(self, seq_out, u_gnn, u_meta, rows=None, want_v=True, want_gate=True):
        fl = self.fusion_layer
        g0, g2 = fl.context_gate[0], fl.context_gate[2]
        return ops.hybrid_fuse(seq_out, u_gnn, u_meta, g0.weight, g0.bias, g2.weight, g2.bias, fl.final_ln.weight,
                               fl.final_ln.bias, rows=rows, ln_eps=fl.final_ln.eps, want_v=want_v, want_gate=want_gate)

    # -- the device path with gradients -----------------------------------------------------------
    def _train_user_side(self, u_dense, u_cat):
        """(U_gnn, U_meta) [B, 128] on the PyTorch modules (B rows; their gradient arrives through the
        fusion's d u_gnn / d u_meta). The GNN user vector is zero (:672), so gnn_projector and gnn_user_emb
        are not evaluated and get no gradient, and the Bernoulli user mask over zeros (:673-681) is not
        drawn; U_gnn = LayerNorm(gnn_proj's bias) expanded, gnn_proj.0.weight sees a zero input."""
        fl = self.fusion_layer
        gp, mp = fl.gnn_proj, fl.meta_proj
        B = u_dense.shape[0]
        zero = torch.zeros(B, self.embed_dim, device=u_dense.device, dtype=torch.float32)
        u_gnn = gp[1](gp[0](zero))
        v_meta = F.normalize(self.meta_mlp(torch.cat([u_dense.to(torch.float32), self.channel_emb(u_cat)], dim=1)),
                             p=2, dim=1)
        return u_gnn, mp[1](mp[0](v_meta))

    def _native_train_forward(self, u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat):
        B, L = seq_ids.shape
        ad, fl = self.seq_adapter, self.fusion_layer
        c, g = ad.content_proj, ad.gnn_proj
        params = (c[0].weight, c[0].bias, c[1].weight, c[1].bias, g[0].weight, g[0].bias, g[1].weight, g[1].bias)
        seq_in = ops.hybrid_adapter_train(self.item_content_emb.weight, self.gnn_item_emb.weight, self.time_emb.weight,
                                          seq_ids, seq_deltas, params, ln_eps=c[1].eps,
                                          scale=math.sqrt(self.embed_dim), p_drop=c[3].p, training=self.training)
        seq_out = encoder_stack(self.seq_encoder.layers, seq_in.view(B, L, self.embed_dim), seq_mask == 0,
                                DROPOUT if self.training else 0.0, self.training, causal=True, act="relu")
        u_gnn, u_meta = self._train_user_side(u_dense, u_cat)
        g0, g2 = fl.context_gate[0], fl.context_gate[2]
        out, v, gate = ops.hybrid_fuse_train(seq_out, u_gnn, u_meta, g0.weight, g0.bias, g2.weight, g2.bias,
                                             fl.final_ln.weight, fl.final_ln.bias, ln_eps=fl.final_ln.eps,
                                             p_drop=fl.gnn_proj[2].p, training=self.training)
        ratios = gate.tolist()        # the forward's one host read
        ops._HYBRID_IDS.check()
        return out, v, ratios

    def forward(self, u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat):
        """(output [B, L, 128], v_seq [B, L, 128], [gnn_ratio, meta_ratio]); right-padded sequences."""
        if not self.native_ok(seq_ids):
            if self.native_train_ok(seq_ids):
                return self._native_train_forward(u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat)
            return self._torch_forward(u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat)
        B, L = seq_ids.shape
        seq_out = self._native_seq_out(seq_ids, seq_deltas, seq_mask)
        u_gnn, u_meta = self._native_user_side(u_idx, u_dense, u_cat)
        out, v, gate = self._native_fuse(seq_out, u_gnn, u_meta)
        ratios = gate.tolist()        # Python floats, as .item() in the reference: the forward's one host read
        ops._HYBRID_IDS.check()       # an id outside the tables raises here (encode_users: at a later call)
        return out.view(B, L, -1), v.view(B, L, -1), ratios


def hybrid_item_vectors(model, first_row=1):
    """(merged [N, 128], unit [N, 128]) of item rows first_row .. of the model's tables: the adapter
    over the whole table in one launch. unit = normalize(seq_adapter(content, gnn)) is the item side of
    the reference's evaluators (:1038-1050, ids from 1); merged feeds encode_users."""
    content, gnn = model.item_content_emb.weight, model.gnn_item_emb.weight
    with torch.no_grad():
        if not model.training and content.is_cuda and content.shape[1] == 128 and gnn.shape[1] == 64:
            merged, unit, _ = ops.hybrid_adapter(content, gnn, model.seq_adapter.native_params(), first_row=first_row,
                                                 want_unit=True)
            return merged, unit
        n = min(content.shape[0], gnn.shape[0])
        merged = model.seq_adapter(content[first_row:n], gnn[first_row:n])
        return merged, F.normalize(merged, p=2, dim=1)


def encode_users(model, u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat, merged=None):
    """[B, 128]: the model's unit output at each user's last valid position, (len - 1).clamp(0) with
    len = seq_mask.sum(1) (:1087-1095). No host read, no gate ratios. On the device path the fusion runs
    on those B rows only and, with merged = hybrid_item_vectors(model)[0], the sequence input is a
    gather from it (in eval mode the adapter's result depends on the item id alone)."""
    B, L = seq_ids.shape
    last = (seq_mask.sum(dim=1) - 1).clamp(min=0).to(torch.int64)
    with torch.no_grad():
        if not model.native_ok(seq_ids):
            out, _, _ = model._torch_forward(u_idx, seq_ids, seq_deltas, seq_mask, u_dense, u_cat)
            return out[torch.arange(B, device=out.device), last]
        seq_out = model._native_seq_out(seq_ids, seq_deltas, seq_mask, merged)
        u_gnn, u_meta = model._native_user_side(u_idx, u_dense, u_cat)
        rows = torch.arange(B, device=last.device, dtype=torch.int64) * L + last
        out, _, _ = model._native_fuse(seq_out, u_gnn, u_meta, rows=rows, want_v=False, want_gate=False)
        return out


# ----------------------------------------------------------------------------------------
# The tower's two in-batch losses (:738-789). On 128-wide fp32 device rows they run on the fused
# contrastive kernels (ops.nce_sum: no B x B logit matrix); anything else takes the PyTorch formula.
def _nce_loss_ok(user_emb, item_emb, pos_item_ids, temperature):
    return (user_emb.is_cuda and item_emb.is_cuda and pos_item_ids.is_cuda and user_emb.dim() == 2
            and item_emb.dim() == 2 and user_emb.shape[1] == 128 and item_emb.shape == user_emb.shape
            and user_emb.shape[0] > 0 and pos_item_ids.shape == (user_emb.shape[0],)
            and user_emb.dtype == torch.float32 and item_emb.dtype == torch.float32
            and not (torch.is_tensor(temperature) and temperature.requires_grad))


def _collisions(pos_item_ids):
    """[B, B] bool: another row with the same positive item (the diagonal is never a collision)."""
    return (pos_item_ids.unsqueeze(1) == pos_item_ids.unsqueeze(0)).fill_diagonal_(False)


def logq_correction_loss(user_emb, item_emb, pos_item_ids, item_probs, temperature=0.07, lambda_logq=0.0):
    """Reference :738-749: cross-entropy over (U I^T - lambda log(item_probs[pos] + 1e-4)) / temperature with
    the label on the diagonal and the other rows of the same positive item filled with -1e4. On the device:
    ops.nce_sum flags 2 with bias_j = lambda log(item_probs[pos_j] + 1e-4) / temperature; the fill is
    exclusion there (exp(-1e4 - max) is 0 in fp32 beside the diagonal). An id outside item_probs is
    reported through ops._LOGQ_IDS (IndexError at the next call or at its check()), the read clamped."""
    if not _nce_loss_ok(user_emb, item_emb, pos_item_ids, temperature):
        scores = torch.matmul(user_emb, item_emb.T)
        if lambda_logq > 0.0:
            scores = scores - lambda_logq * torch.log(item_probs[pos_item_ids] + 1e-4).view(1, -1)
        logits = (scores / temperature).masked_fill(_collisions(pos_item_ids), -1e4)
        return F.cross_entropy(logits, torch.arange(logits.size(0), device=logits.device))
    tau = float(temperature)
    bias = None
    if lambda_logq > 0.0:
        ids = ops._LOGQ_IDS(pos_item_ids, item_probs.shape[0])
        probs = item_probs.detach().to(device=user_emb.device, dtype=torch.float32)
        bias = torch.log(probs[ids] + 1e-4) * (float(lambda_logq) / tau)
    return ops.nce_loss(user_emb, item_emb, bias, k1a=pos_item_ids, k1b=pos_item_ids, tau=tau,
                        flags=ops.NCE_MASK_ITEM, tag="logq_correction")


def efficient_corrected_logq_loss(user_emb, item_emb, pos_item_ids, precomputed_log_q, temperature=0.1,
                                  lambda_logq=0.1):
    """Reference :751-789: cross-entropy over U I^T / temperature - lambda log_q[pos_j], the diagonal
    restored to its uncorrected logit when lambda > 0, same-item rows off the diagonal filled with -1e9. On
    the device: ops.nce_sum flags 18 (NCE_MASK_ITEM_POS) with bias_j = lambda log_q[pos_j], flags 2 without a
    bias at lambda = 0. The reference's host assert on the ids is the device check of ops._LOGQ_IDS
    (IndexError at the next call or at its check(); the read clamped); the PyTorch formula raises at once."""
    n_q = precomputed_log_q.size(0)
    if not _nce_loss_ok(user_emb, item_emb, pos_item_ids, temperature):
        if pos_item_ids.numel() and not 0 <= int(pos_item_ids.min()) <= int(pos_item_ids.max()) < n_q:
            raise IndexError(f"efficient_corrected_logq_loss: pos_item_ids outside [0, {n_q})")
        logits = torch.matmul(user_emb, item_emb.T) / temperature
        if lambda_logq > 0.0:
            logits = logits - precomputed_log_q[pos_item_ids].view(1, -1) * lambda_logq
            pos = torch.einsum("bd,bd->b", user_emb, item_emb) / temperature
            eye = torch.eye(logits.size(0), dtype=torch.bool, device=logits.device)
            logits = torch.where(eye, pos.view(-1, 1), logits)
        mask_value = -30000.0 if logits.dtype == torch.float16 else -1e9
        logits = logits.masked_fill(_collisions(pos_item_ids), mask_value)
        return F.cross_entropy(logits, torch.arange(logits.size(0), device=logits.device))
    ids = ops._LOGQ_IDS(pos_item_ids, n_q)
    bias, flags = None, ops.NCE_MASK_ITEM
    if lambda_logq > 0.0:
        log_q = precomputed_log_q.detach().to(device=user_emb.device, dtype=torch.float32)
        bias, flags = log_q[ids] * float(lambda_logq), ops.NCE_MASK_ITEM_POS
    return ops.nce_loss(user_emb, item_emb, bias, k1a=pos_item_ids, k1b=pos_item_ids, tau=float(temperature),
                        flags=flags, tag="efficient_logq")


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
        fused = n_items >= FUSED_POOL_MIN_ITEMS and len(users) > 0
        if fused:
            # no score matrix bounds the chunk; one retriever's pools for every chunk first, then the
            # other's, so that the two corpora do not evict each other's cached bf16 image per chunk
            step = max(1, int(batch_size))
            pools_g, pools_s = (
                torch.cat([ops.retrieve_topk(_pad128(uv[users_d[s:s + step]]), iv, pool_k)[1].to(torch.int32)
                           for s in range(0, len(users), step)])
                for uv, iv in ((gu, _pad128(gi)), (su, _pad128(si))))
        else:
            step = _chunk_rows(batch_size, n_items)
        for s in range(0, len(users), step):
            rows = users_d[s:s + step]
            ug, us = gu[rows], su[rows]
            if fused:
                pool_g, pool_s = pools_g[s:s + step], pools_s[s:s + step]
            else:
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
