"""Autograd-aware wrappers over the C-ABI kernels (include/recsys_amd.h).

Every function here launches HIP kernels from librecsys_amd.so on the current torch stream.
There is no CPU path: a non-ROCm tensor raises.
"""
from __future__ import annotations

import ctypes
import math
import os
import weakref

import torch

from . import _native as N

NCE_PLAIN = 0
NCE_MASK_ITEM = 2
NCE_MASK_ITEM_USER = 6
NCE_SUPCON = 9
NCE_MASK_ITEM_POS = 18  # NCE_MASK_ITEM with the label logit left without its bias (plain kernels only)

_NSPLIT_FWD = 8
# partial slots of the grouped forward; the fused forward (rsx_nce_grouped_fwd_grad) accepts 1/2/4/8. With 1 or
# 2 the library lays its grid out itself from the row count and the device's CU count: whole-row workgroups
# on the row blocks that fill whole rounds of the chip, up to 8 splits on the rest (csrc/nce_common.h,
# fwdg_schedule); 4 runs 4 splits everywhere, 8 runs 4 on the leading row blocks and 8 on the tail
_NSPLIT_FWD_GROUPED = int(os.environ.get("RSX_NCE_NSPLIT_FWD", "2"))
if _NSPLIT_FWD_GROUPED not in (1, 2, 4, 8):
    raise ValueError("RSX_NCE_NSPLIT_FWD must be 1, 2, 4 or 8 (the fused forward's supported partial-slot counts)")
_NSPLIT_BWD = 8

# Logit precision of the grouped (live LogQ) loss kernels, include/recsys_amd.h RSX_NCE_*:
# "bf16x3" = hi/lo bf16 split on the bf16 MFMA (max |dot error| ~3e-6 on unit vectors; the
# reference computes these logits in fp16 under AMP), "fp32" = fp32-input MFMA, "f16" = the fused
# forward and the column pass on the fp16 MFMA: logits from an fp16 hi/lo split (tighter than
# bf16x3), gradient products as one fp16 MFMA (the reference's autocast-fp16 arithmetic for them).
NCE_PRECISIONS = {"fp32": 0, "bf16x3": 1, "f16": 2}
_nce_precision = os.environ.get("RSX_NCE_PRECISION", "f16")
if _nce_precision not in NCE_PRECISIONS:
    raise ValueError(f"RSX_NCE_PRECISION must be one of {sorted(NCE_PRECISIONS)}")


def set_nce_precision(mode: str) -> str:
    """Set the grouped-loss precision ("fp32" | "bf16x3" | "f16"); returns the previous mode."""
    global _nce_precision
    if mode not in NCE_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(NCE_PRECISIONS)}")
    prev, _nce_precision = _nce_precision, mode
    return prev


def nce_precision() -> str:
    return _nce_precision


def next_seed() -> int:
    """Dropout seed from torch's CPU generator (reproducible under torch.manual_seed)."""
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def _c(t):
    return t if t is None or t.is_contiguous() else t.contiguous()


# Host-side argument checks of the raw-pointer wrappers: attribute comparisons only (no tensor
# op, no synchronisation), run before ensure_device so that a bad call never reaches a kernel.
# TypeError: wrong dtype; ValueError: wrong shape / length; RuntimeError: wrong device.
_INT_DTYPES = (torch.int32, torch.int16, torch.int8, torch.uint8)


def _f32(fn, name, t, ref=None):
    """t is an fp32 tensor (on ref's device)."""
    if t.dtype != torch.float32:
        raise TypeError(f"{fn}: {name} must be float32, got {t.dtype}")
    if ref is not None and t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")


def _f32_vec(fn, name, t, n, ref):
    """t (None allowed) is an fp32 tensor of n elements on ref's device."""
    if t is None:
        return
    _f32(fn, name, t, ref)
    if t.numel() != n:
        raise ValueError(f"{fn}: {name} has {t.numel()} elements, expected {n}")


def _index(fn, name, t, ref=None, n=None):
    """t as the int64 index tensor the kernels read (another integer dtype is converted;
    anything else refused), on ref's device, of n elements."""
    if t.dtype != torch.int64:
        if t.dtype not in _INT_DTYPES:
            raise TypeError(f"{fn}: {name} must be an integer tensor, got {t.dtype}")
        t = t.long()
    if ref is not None and t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")
    if n is not None and t.numel() != n:
        raise ValueError(f"{fn}: {name} has {t.numel()} elements, expected {n}")
    return t


def _rows2(fn, name, t):
    """t is an fp32 [rows, D] matrix; returns D."""
    _f32(fn, name, t)
    if t.dim() != 2:
        raise ValueError(f"{fn}: {name} must be 2-D, got shape {tuple(t.shape)}")
    return t.shape[1]


def _ln_args(fn, x, res, weight, bias):
    """LayerNorm family: x (and res, same shape / dtype / device) fp32 rows of D = last dim,
    weight / bias of D elements on x's device."""
    _f32(fn, "x", x)
    if x.dim() < 1:
        raise ValueError(f"{fn}: x must have a last dimension")
    if res is not None:
        _f32(fn, "res", res, x)
        if res.shape != x.shape:
            raise ValueError(f"{fn}: res has shape {tuple(res.shape)}, x {tuple(x.shape)}")
    D = x.shape[-1]
    _f32_vec(fn, "weight", weight, D, x)
    _f32_vec(fn, "bias", bias, D, x)


def _tensor_key(ts):
    """Cache key of derived device images: the tensor OBJECTS (held, so their storage cannot be
    recycled under a stale key), their storage pointers and in-place version counters."""
    return tuple((t, t.data_ptr(), t._version) for t in ts)


def _key_eq(a, b) -> bool:
    """Key equality with identity for tensors (== on tensors is elementwise)."""
    if a is None or len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            if x[0] is not y[0] or x[1:] != y[1:]:
                return False
        elif x != y:
            return False
    return True


# ----------------------------------------------------------------------------------------
# A2: fused sequence embedding (v1_refine_usertower.py:447-459)
def _zeros_group(likes):
    """Zero gradient buffers shaped like each tensor in likes (None -> None), carved out of ONE
    zero-filled allocation (one fill launch instead of one per table); 16-B aligned slices."""
    shapes = [None if t is None else t.shape for t in likes]
    sizes = [0 if t is None else (t.numel() + 3) // 4 * 4 for t in likes]
    total = sum(sizes)
    if total == 0:
        return [None] * len(likes)
    ref = next(t for t in likes if t is not None)
    flat = torch.zeros(total, device=ref.device, dtype=torch.float32)
    out, o = [], 0
    for shp, n, t in zip(shapes, sizes, likes):
        out.append(None if t is None else flat[o:o + t.numel()].view(shp))
        o += n
    return out


class ItemRows:
    """The pretrained rows of a packed token list kept once per distinct item: token t's row is
    rows[idx[t]] (rows [Uq, D] fp32 = the lookup's rows of the step index's uniq_items, idx [T]
    int64 = each token's slot in them; both dropout views share the slots). item_proj, the
    embedding stage and item_proj's weight gradient then run over the Uq rows
    (SASRecUserTower.forward_packed), and the [T, D] per-token matrix is never written.

    The fields to use are rows, idx and materialize() (a fresh rows[idx] gather, [T, D]). The object
    stands where the step index used to carry that [T, D] tensor (StepIndex.packed[3]), so it also
    answers shape / dtype / device / len / indexing like it, and any other tensor attribute or torch
    function is served by a materialised copy -- never cached (the index does not end up holding the
    matrix it exists to avoid) and counted in ItemRows.materialized, so a path that falls back to the
    per-token matrix by accident shows up (tests/test_gpu_item_proj_unique.py holds the step at 0)."""

    requires_grad = False
    materialized = 0  # materialize() calls so far, process-wide

    def __init__(self, rows, idx):
        self.rows, self.idx = rows, idx

    shape = property(lambda self: torch.Size((self.idx.numel(), self.rows.shape[1])))
    dtype = property(lambda self: self.rows.dtype)
    device = property(lambda self: self.rows.device)
    is_cuda = property(lambda self: self.rows.is_cuda)

    def materialize(self):
        ItemRows.materialized += 1
        return gather_rows(self.rows, self.idx)

    def __len__(self):
        return self.idx.numel()

    def __getitem__(self, key):
        return self.materialize()[key]

    def __getattr__(self, name):  # only reached for attributes not defined above
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        def tok(a):
            return a.materialize() if isinstance(a, ItemRows) else a
        return func(*[tok(a) for a in args], **{k: tok(v) for k, v in (kwargs or {}).items()})


class _SeqEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base, gate, pos, ln_w, ln_b, ids, cfg, tok_pos, *tables):
        eps, p_drop, seed, padding_idx, L, tab0_seg, base_idx = cfg
        N.ensure_device(base)
        D = base.shape[-1]
        base = _c(base)
        ids = [_c(t) for t in ids]
        tables = [_c(t) for t in tables]
        if base_idx is None:
            T = base.numel() // D
            out = torch.empty_like(base)
        else:  # token t reads base[base_idx[t]]
            T = base_idx.numel()
            out = torch.empty(T, D, device=base.device, dtype=torch.float32)
        mean = torch.empty(T, device=base.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        gate = _c(gate)
        with timed("seq_embed_fwd"):
            rc = N.lib().rsx_seq_embed_fwd(
                N.ptr(base), N.ptr(base_idx), N.ptr_array(ids), N.ptr_array(tables), len(tables), N.ptr(gate),
                N.ptr(pos), N.ptr(tok_pos), N.ptr(ln_w), N.ptr(ln_b), eps, T, L, D, p_drop, seed, N.ptr(out),
                N.ptr(mean), N.ptr(rstd), N.stream())
        N.check(rc, "seq_embed_fwd")
        ctx.save_for_backward(base, gate, pos, ln_w, mean, rstd, tok_pos, *ids, *tables)
        ctx.cfg = (eps, p_drop, seed, padding_idx, len(tables), T, L, D)
        ctx.tab0_seg = tab0_seg
        ctx.base_idx = base_idx
        return out

    @staticmethod
    def backward(ctx, dout):
        eps, p_drop, seed, padding_idx, nt, T, L, D = ctx.cfg
        saved = ctx.saved_tensors
        base, gate, pos, ln_w, mean, rstd, tok_pos = saved[:7]
        ids = list(saved[7:7 + nt])
        tables = list(saved[7 + nt:7 + 2 * nt])
        dout = _c(dout)
        need = ctx.needs_input_grad
        base_idx = ctx.base_idx
        dbase = torch.empty_like(dout) if need[0] else None  # per token, also with base_idx
        dgate, dpos, dlnw, dlnb, *dtabs = _zeros_group(
            [gate if need[1] else None, pos if need[2] else None, ln_w if need[3] else None,
             ln_w if need[4] else None] + [t if need[8 + j] else None for j, t in enumerate(tables)])
        rows = N.i64_array([t.shape[0] for t in tables])
        # table 0 with a prepared sort by id: segmented sums of dx (= dbase) instead of atomics
        seg0 = ctx.tab0_seg if (nt > 0 and dtabs[0] is not None) else None
        seg_b = ctx.tab0_seg if (base_idx is not None and need[0]) else None  # per-row sums of an indexed base
        if seg0 is not None and dbase is None:
            dbase = torch.empty_like(dout)
        kern_tabs = ([None] + dtabs[1:]) if seg0 is not None else dtabs
        nws = N.lib().rsx_seq_embed_bwd_workspace_floats(T, L, D)
        ws = torch.empty(nws, device=base.device, dtype=torch.float32)
        with timed("seq_embed_bwd"):
            rc = N.lib().rsx_seq_embed_bwd(
                N.ptr(base), N.ptr(base_idx), N.ptr_array(ids), N.ptr_array(tables), rows,
                N.i64_array(padding_idx), nt, N.ptr(gate), N.ptr(pos), N.ptr(tok_pos), N.ptr(ln_w), N.ptr(mean),
                N.ptr(rstd), eps, T, L, D, p_drop, seed, N.ptr(dout), N.ptr(dbase), N.ptr_array(kern_tabs),
                N.ptr(dgate), N.ptr(dpos), N.ptr(dlnw), N.ptr(dlnb), N.ptr(ws), nws, N.stream())
        N.check(rc, "seq_embed_bwd")
        if seg0 is not None or seg_b is not None:  # chunk partials, then per-id sums of its chunks (both deterministic)
            perm, cb, chunk_ids, ch_off, uniq = ctx.tab0_seg
            part = torch.empty(chunk_ids.numel(), D, device=base.device, dtype=torch.float32)
            rc = N.lib().rsx_segment_sum_rows(N.ptr(dbase), D, N.ptr(perm), N.ptr(cb), N.ptr(chunk_ids),
                                              chunk_ids.numel(), D, None, -1, N.ptr(part), D, 0, N.stream())
            N.check(rc, "segment_sum_rows(chunks)")
            if seg_b is not None:  # the per-id sums ungated, in segment order: the gradient of base's rows
                dbase = torch.empty_like(base)
            if seg0 is not None and seg_b is not None:  # one pass: gated into table 0, raw into dbase
                rc = N.lib().rsx_segment_sum_rows2(N.ptr(part), D, N.ptr(chunk_ids), N.ptr(ch_off), N.ptr(uniq),
                                                   uniq.numel(), D, N.ptr(gate), padding_idx[0], N.ptr(dtabs[0]),
                                                   dtabs[0].stride(0), 1, N.ptr(dbase), D, N.stream())
                N.check(rc, "segment_sum_rows2(ids)")
            elif seg0 is not None:
                rc = N.lib().rsx_segment_sum_rows(N.ptr(part), D, N.ptr(chunk_ids), N.ptr(ch_off), N.ptr(uniq),
                                                  uniq.numel(), D, N.ptr(gate), padding_idx[0], N.ptr(dtabs[0]),
                                                  dtabs[0].stride(0), 1, N.stream())
                N.check(rc, "segment_sum_rows(ids)")
            else:
                rc = N.lib().rsx_segment_sum_rows(N.ptr(part), D, N.ptr(chunk_ids), N.ptr(ch_off), None,
                                                  uniq.numel(), D, None, -1, N.ptr(dbase), D, 0, N.stream())
                N.check(rc, "segment_sum_rows(base)")
        if not need[0]:
            dbase = None
        return (dbase, dgate, dpos, dlnw, dlnb, None, None, None, *dtabs)


_SEG_CHUNK = 64


def sort_segments(ids):
    """Two-level plan for the sorted segmented sums of table 0's gradient (seq_embed tab0_seg):
    ids[perm] sorted (stable); the sorted tokens are cut into chunks of <= 64 tokens that never
    straddle two ids (chunk c = [cb[c], cb[c+1])), so a Zipf-hot id's thousands of tokens are
    summed by many chunks in parallel; segment u (id uniq[u]) owns chunks [ch_off[u],
    ch_off[u+1]). Its size queries synchronise the host (build it ahead, e.g. in
    dist.prepare_step_index_async). Returns (perm, cb, chunk_ids, ch_off, uniq)."""
    ids = ids.reshape(-1)
    dev = ids.device
    srt, perm = torch.sort(ids, stable=True)
    uniq, cnt = torch.unique_consecutive(srt, return_counts=True)
    seg_off = torch.zeros(uniq.numel() + 1, device=dev, dtype=torch.int64)
    seg_off[1:] = torch.cumsum(cnt, 0)
    nch = (cnt + _SEG_CHUNK - 1) // _SEG_CHUNK
    ch_off = torch.zeros(uniq.numel() + 1, device=dev, dtype=torch.int64)
    ch_off[1:] = torch.cumsum(nch, 0)
    total = int(ch_off[-1])
    ch_seg = torch.repeat_interleave(torch.arange(uniq.numel(), device=dev), nch, output_size=total)
    k = torch.arange(total, device=dev)
    cb = torch.empty(total + 1, device=dev, dtype=torch.int64)
    cb[:-1] = seg_off[ch_seg] + _SEG_CHUNK * (k - ch_off[ch_seg])
    cb[-1] = ids.numel()
    return perm, cb, k, ch_off, uniq


def seq_embed(base, ids, tables, gate, pos, ln_w, ln_b, eps=1e-5, p_drop=0.0, padding_idx=None, tok_pos=None,
              tab0_seg=None, base_idx=None):
    """x = base + sum_j tables[j][ids[j]] * gate[j] + pos[l] ; LayerNorm ; dropout.

    Dense: base [B, L, D], ids [B, L], pos [>= L, D] (position = token % L).
    Packed: base [T, D], ids [T], tok_pos [T] int64 positions, pos [L, D].
    gate [ntab]; ln_w/ln_b [D]. padding_idx: per-table row excluded from the table gradient
    (nn.Embedding semantics). tab0_seg: sort_segments(ids[0]) — table 0's gradient then comes
    from rsx_segment_sum_rows (deterministic, no atomics) instead of the kernel's scatter-add.
    base_idx (packed form with tab0_seg): base holds one row per distinct ids[0] value, in
    tab0_seg's uniq order, and token t reads base[base_idx[t]] (base_idx[t] = the slot of
    ids[0][t] in uniq); base's gradient is then the per-slot sum of the per-token one, from the
    same sorted segment sums.
    """
    if padding_idx is None:
        padding_idx = [-1] * len(tables)
    padding_idx = [(-1 if p is None else int(p)) for p in padding_idx]
    seed = next_seed() if p_drop > 0 else 0
    if tok_pos is None:
        L = base.shape[1]
        pos = pos[:L]
    else:
        L = pos.shape[0]
        tok_pos = _c(tok_pos)
    if base_idx is not None:
        if tok_pos is None or tab0_seg is None or base.dim() != 2 or base.shape[0] != tab0_seg[4].numel():
            raise RuntimeError("seq_embed: base_idx needs the packed form, tab0_seg and one base row per "
                               "distinct ids[0] value")
        base_idx = _c(_index("seq_embed", "base_idx", base_idx, base, ids[0].numel()))
    cfg = (float(eps), float(p_drop), seed, padding_idx, int(L), tab0_seg, base_idx)
    return _SeqEmbed.apply(base, gate, pos, ln_w, ln_b, list(ids), cfg, tok_pos, *tables)


# ----------------------------------------------------------------------------------------
# A3 / A9: masked MHA core
# "bf16x3" (default): head dim 32 runs rsx_mha_fwd_x3 / rsx_mha_bwd_x3 (split-bf16 MFMA, ~2^-17
# relative error per product); other head dims and "fp32" run the fp32 kernels.
MHA_PRECISIONS = ("fp32", "bf16x3")
_mha_precision = os.environ.get("RSX_MHA_PRECISION", "bf16x3")
assert _mha_precision in MHA_PRECISIONS, _mha_precision


def set_mha_precision(p: str) -> None:
    global _mha_precision
    assert p in MHA_PRECISIONS, p
    _mha_precision = p


def mha_precision() -> str:
    return _mha_precision


def _mha_x3(Dh):
    return _mha_precision == "bf16x3" and Dh == 32


def _mha_x3_fwd(Dh):  # the bf16x3 forward also covers head dim 64 (BERT inference; no x3 backward)
    return _mha_precision == "bf16x3" and Dh in (32, 64)


class _MHA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, key_pad, seg_off, H, causal, p_drop, seed, max_len=None):
        N.ensure_device(qkv)
        qkv = _c(qkv)
        D3 = qkv.shape[-1]
        T = qkv.numel() // D3
        D = D3 // 3
        Dh = D // H
        if seg_off is None:
            B, L = qkv.shape[0], qkv.shape[1]
        else:  # packed: L bounds the segment lengths (the head-dim-64 backward sizes its LDS by it)
            B, L = seg_off.numel() - 1, int(max_len) if max_len else 64
        out = torch.empty(qkv.shape[:-1] + (D,), device=qkv.device, dtype=torch.float32)
        lse = torch.empty(T, H, device=qkv.device, dtype=torch.float32)
        kp = None
        if key_pad is not None:
            kp = _c(key_pad.to(torch.uint8)) if key_pad.dtype != torch.uint8 else _c(key_pad)
        fn = N.lib().rsx_mha_fwd_x3 if _mha_x3_fwd(Dh) else N.lib().rsx_mha_fwd
        rc = fn(N.ptr(qkv), N.ptr(kp), N.ptr(seg_off), B, L, H, Dh, int(causal), p_drop, seed, N.ptr(out), N.ptr(lse),
                N.stream())
        N.check(rc, "mha_fwd")
        ctx.save_for_backward(qkv, kp, seg_off, out, lse)
        ctx.cfg = (B, L, H, Dh, int(causal), p_drop, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, L, H, Dh, causal, p_drop, seed = ctx.cfg
        qkv, kp, seg_off, out, lse = ctx.saved_tensors
        dout = _c(dout)
        dqkv = torch.empty_like(qkv)
        fn = N.lib().rsx_mha_bwd_x3 if _mha_x3(Dh) else N.lib().rsx_mha_bwd
        rc = fn(N.ptr(qkv), N.ptr(kp), N.ptr(seg_off), N.ptr(out), N.ptr(lse), N.ptr(dout), B, L, H, Dh, causal,
                p_drop, seed, N.ptr(dqkv), N.stream())
        N.check(rc, "mha_bwd")
        return dqkv, None, None, None, None, None, None, None


class _QKVMHA(torch.autograd.Function):
    """mha(F.linear(x, w, b)) with the projection fused into the attention forward
    (rsx_mha_qkv_fwd_x3: head dim 32, D = 128, bf16x3). The kernel still writes qkv, which the
    backward uses exactly as _MHA + _TokLinear do: dqkv from rsx_mha_bwd_x3, then dx on the
    bf16x3 GEMM and (dw, db) from the split-K weight-gradient kernel."""

    @staticmethod
    def forward(ctx, x, w, b, key_pad, seg_off, H, causal, p_drop, seed):
        N.ensure_device(x)
        x = _c(x)
        w = _c(w)
        D = x.shape[-1]
        T = x.numel() // D
        if seg_off is None:
            B, L = x.shape[0], x.shape[1]
        else:
            B, L = seg_off.numel() - 1, 64
        qkv = torch.empty(x.shape[:-1] + (3 * D,), device=x.device, dtype=torch.float32)
        out = torch.empty_like(x)
        lse = torch.empty(T, H, device=x.device, dtype=torch.float32)
        kp = None
        if key_pad is not None:
            kp = _c(key_pad.to(torch.uint8)) if key_pad.dtype != torch.uint8 else _c(key_pad)
        with timed("qkv_mha_fwd"):
            rc = N.lib().rsx_mha_qkv_fwd_x3(N.ptr(x), N.ptr(w), N.ptr(None if b is None else _c(b)), N.ptr(kp),
                                            N.ptr(seg_off), B, L, H, int(causal), p_drop, seed, N.ptr(qkv),
                                            N.ptr(out), N.ptr(lse), N.stream())
        N.check(rc, "mha_qkv_fwd_x3")
        ctx.save_for_backward(x, w, qkv, kp, seg_off, out, lse)
        ctx.cfg = (B, L, H, int(causal), p_drop, seed, b is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, L, H, causal, p_drop, seed, has_bias = ctx.cfg
        x, w, qkv, kp, seg_off, out, lse = ctx.saved_tensors
        dout = _c(dout)
        dqkv = torch.empty_like(qkv)
        rc = N.lib().rsx_mha_bwd_x3(N.ptr(qkv), N.ptr(kp), N.ptr(seg_off), N.ptr(out), N.ptr(lse), N.ptr(dout), B, L,
                                    H, 32, causal, p_drop, seed, N.ptr(dqkv), N.stream())
        N.check(rc, "mha_bwd")
        D = x.shape[-1]
        dq2 = dqkv.reshape(-1, 3 * D)
        dx = _dx(dq2, w).reshape(x.shape) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_wgrad(dq2, x.reshape(-1, D), w.shape, has_bias and ctx.needs_input_grad[2])
        return dx, dw, db, None, None, None, None, None, None


# RSX_QKV_FUSED=1 opts into the fused projection + attention kernel. Off by default:
# measured 0.879 ms vs 0.358 ms for linear_tok + mha at the step shape (the fused
# kernel recomputes the K/V projection per query block and runs at 272 VGPRs).
_QKV_FUSED = os.environ.get("RSX_QKV_FUSED", "0") == "1"


def qkv_mha(x, w, b, key_pad, num_heads, causal, p_drop=0.0, seg_off=None):
    """mha(linear(x, w, b), ...): the fused projection + attention kernel when it applies
    (bf16x3 mode, 4 heads of 32, dense or packed), otherwise linear_tok then mha."""
    D = x.shape[-1]
    if (_QKV_FUSED and _mha_precision == "bf16x3" and _gemm_precision == "bf16x3" and D == 128
            and int(num_heads) == 4 and tuple(w.shape) == (3 * D, D) and x.is_cuda):
        seed = next_seed() if p_drop > 0 else 0
        if seg_off is not None:
            seg_off = _c(seg_off.to(torch.int32))
        return _QKVMHA.apply(x, w, b, key_pad, seg_off, 4, bool(causal), float(p_drop), seed)
    return mha(linear_tok(x, w, b), key_pad, num_heads, causal, p_drop, seg_off)


def mha(qkv, key_pad, num_heads, causal, p_drop=0.0, seg_off=None, max_len=None):
    """Dense: qkv [B, L, 3D], key_pad [B, L]. Packed: qkv [T, 3D], key_pad [T], seg_off [B+1] int32;
    max_len (packed, optional) = an upper bound of the segment lengths (<= 64)."""
    seed = next_seed() if p_drop > 0 else 0
    if seg_off is not None:
        seg_off = _c(seg_off.to(torch.int32))
    return _MHA.apply(qkv, key_pad, seg_off, int(num_heads), bool(causal), float(p_drop), seed, max_len)


# ----------------------------------------------------------------------------------------
# Row gather (+ optional F.normalize) with scatter backward
class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, idx, normalize, eps, unique, skip_idx):
        N.ensure_device(src)
        D = src.shape[-1]
        src2 = src.reshape(-1, D)
        if src2.stride(1) != 1 or src2.stride(0) % 4 != 0 or src2.data_ptr() % 16 != 0:
            src2 = src2.contiguous()
        n = idx.numel() if idx is not None else src2.shape[0]
        idx_c = _c(idx) if idx is not None else None
        out = torch.empty(n, D, device=src.device, dtype=torch.float32)
        nrm = torch.empty(n, device=src.device, dtype=torch.float32) if normalize else None
        rc = N.lib().rsx_gather_rows(N.ptr(src2), src2.stride(0), N.ptr(idx_c), n, D, int(normalize), eps,
                                     N.ptr(out), N.ptr(nrm), N.stream())
        N.check(rc, "gather_rows")
        ctx.src_shape = src.shape
        ctx.cfg = (normalize, eps, unique, skip_idx, n, D)
        saved = [t for t in (idx_c, out if normalize else None, nrm) if t is not None]
        ctx.has_idx = idx_c is not None
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dy):
        normalize, eps, unique, skip_idx, n, D = ctx.cfg
        saved = list(ctx.saved_tensors)
        idx = saved.pop(0) if ctx.has_idx else None
        y = nrm = None
        if normalize:
            y, nrm = saved
        dy = _c(dy)
        rows = 1
        for s in ctx.src_shape[:-1]:
            rows *= s
        if idx is None:
            # plain store of every row but skip_idx, which the kernel leaves untouched: zero it
            alloc = torch.zeros if 0 <= skip_idx < rows else torch.empty
            dsrc = alloc(rows, D, device=dy.device, dtype=torch.float32)
            mode = 0
        else:
            dsrc = torch.zeros(rows, D, device=dy.device, dtype=torch.float32)
            mode = 1 if unique else 2
        rc = N.lib().rsx_scatter_rows(N.ptr(dy), N.ptr(y), N.ptr(nrm), N.ptr(idx), n, D, int(normalize), eps, mode,
                                      skip_idx, N.ptr(dsrc), D, N.stream())
        N.check(rc, "scatter_rows")
        return dsrc.view(ctx.src_shape), None, None, None, None, None


def gather_rows(src, idx=None, normalize=False, eps=1e-12, unique=False, skip_idx=-1):
    """out[r] = src.view(-1, D)[idx[r]] (idx None => all rows), optionally L2-normalised. The kernel
    reads fp32 rows: another floating dtype is cast first (autograd-aware), anything else refused;
    idx: int64 on src's device (another integer dtype is converted, anything else refused)."""
    if src.dtype != torch.float32:
        if not src.is_floating_point():
            raise TypeError(f"gather_rows: floating-point rows expected, got {src.dtype}")
        src = src.float()
    if idx is not None:
        idx = _index("gather_rows", "idx", idx, src)
    return _GatherRows.apply(src, idx, bool(normalize), float(eps), bool(unique), int(skip_idx))


class _GatherRowsMulti(torch.autograd.Function):
    """Several row gathers of one source (each index list duplicate-free), with ONE zero-filled
    source gradient that every gather's backward accumulates into in turn (non-atomic
    read-add-write, scatter mode 1): the autograd form of k gathers of slices of one tensor
    costs k zero-filled gradients, the slice gradients and their sums."""

    @staticmethod
    def forward(ctx, src, norms, eps, *idxs):
        N.ensure_device(src)
        src2 = _c(src)
        D = src2.shape[-1]
        outs, saved = [], []
        for idx, nz in zip(idxs, norms):
            idx = _c(idx)
            n = idx.numel()
            out = torch.empty(n, D, device=src.device, dtype=torch.float32)
            nrm = torch.empty(n, device=src.device, dtype=torch.float32) if nz else None
            rc = N.lib().rsx_gather_rows(N.ptr(src2), src2.stride(0), N.ptr(idx), n, D, int(nz), eps, N.ptr(out),
                                         N.ptr(nrm), N.stream())
            N.check(rc, "gather_rows")
            outs.append(out)
            saved += [idx, out if nz else idx, nrm if nz else idx]
        ctx.cfg = (tuple(norms), eps, src2.shape)
        ctx.save_for_backward(*saved)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        norms, eps, shape = ctx.cfg
        saved = ctx.saved_tensors
        D = shape[-1]
        dsrc = torch.zeros(shape, device=saved[0].device, dtype=torch.float32)
        for k, (dy, nz) in enumerate(zip(dys, norms)):
            if dy is None:
                continue
            idx, y, nrm = saved[3 * k], saved[3 * k + 1], saved[3 * k + 2]
            dy = _c(dy)
            rc = N.lib().rsx_scatter_rows(N.ptr(dy), N.ptr(y if nz else None), N.ptr(nrm if nz else None), N.ptr(idx),
                                          idx.numel(), D, int(nz), eps, 1, -1, N.ptr(dsrc), D, N.stream())
            N.check(rc, "scatter_rows")
        return (dsrc, None, None) + (None,) * len(dys)


def gather_rows_multi(src, specs, eps=1e-12):
    """[gather_rows(src, idx, normalize=nz, unique=True) for idx, nz in specs] as one autograd
    node (one source gradient buffer; each idx must be duplicate-free)."""
    _rows2("gather_rows_multi", "src", src)
    idxs = [_index("gather_rows_multi", f"idx[{k}]", i, src) for k, (i, _) in enumerate(specs)]
    norms = [bool(nz) for _, nz in specs]
    return list(_GatherRowsMulti.apply(src, norms, float(eps), *idxs))


def l2_normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=-1) on the last dim."""
    shape = x.shape
    return gather_rows(x, None, normalize=True, eps=eps).view(shape)


# ----------------------------------------------------------------------------------------
# A6 / A7 / A12: fused contrastive cross-entropy
class _NCE(torch.autograd.Function):
    """Returns (sum of row losses over valid rows, number of valid rows). bf16x3 precision
    (default) runs rsx_nce_fwd_x3 / rsx_nce_bwd_x3 (split counts chosen by the library), fp32
    the fp32-MFMA rsx_nce_fwd / rsx_nce_bwd."""

    @staticmethod
    def forward(ctx, A, B, bias, k1a, k1b, k2a, k2b, tau, flags, diag_offset, tag):
        N.ensure_device(A)
        A = _c(A)
        B = _c(B)
        n, m = A.shape[0], B.shape[0]
        x3 = _nce_precision != "fp32"  # "f16" only changes the grouped kernels
        nws = (N.lib().rsx_nce_x3_workspace_floats(n, m) if x3
               else N.lib().rsx_nce_workspace_floats(n, m, _NSPLIT_FWD, _NSPLIT_BWD))
        ws = torch.empty(nws, device=A.device, dtype=torch.float32)
        out2 = torch.empty(2, device=A.device, dtype=torch.float32)
        keys = [_c(k) for k in (k1a, k1b, k2a, k2b)]
        with timed(f"{tag}/nce_fwd"):
            if x3:
                rc = N.lib().rsx_nce_fwd_x3(N.ptr(A), N.ptr(B), N.ptr(bias), *[N.ptr(k) for k in keys], n, m,
                                            A.stride(0), B.stride(0), diag_offset, tau, flags, N.ptr(ws), N.ptr(out2),
                                            N.stream())
            else:
                rc = N.lib().rsx_nce_fwd(N.ptr(A), N.ptr(B), N.ptr(bias), *[N.ptr(k) for k in keys], n, m,
                                         A.stride(0), B.stride(0), diag_offset, tau, flags, _NSPLIT_FWD, N.ptr(ws),
                                         N.ptr(out2), N.stream())
        N.check(rc, "nce_fwd")
        ctx.save_for_backward(A, B, bias, *keys, ws)
        ctx.cfg = (n, m, tau, flags, diag_offset, tag, x3)
        cnt = out2[1]
        ctx.mark_non_differentiable(cnt)
        return out2[0], cnt

    @staticmethod
    def backward(ctx, g, _gcnt):
        A, B, bias, k1a, k1b, k2a, k2b, ws = ctx.saved_tensors
        n, m, tau, flags, off, tag, x3 = ctx.cfg
        g = _c(g.reshape(1).to(torch.float32))
        head = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1a), N.ptr(k1b), N.ptr(k2a), N.ptr(k2b), n, m, A.stride(0),
                B.stride(0), off, tau, flags)
        if x3:
            fn, args = N.lib().rsx_nce_bwd_x3, head + (N.ptr(g), N.ptr(ws))
        else:
            fn, args = N.lib().rsx_nce_bwd, head + (_NSPLIT_FWD, _NSPLIT_BWD, N.ptr(g), N.ptr(ws))
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = torch.empty_like(A)
            with timed(f"{tag}/nce_bwd_rows"):
                rc = fn(*args, N.ptr(dA), None, 0, N.stream())
            N.check(rc, "nce_bwd(rows)")
        if ctx.needs_input_grad[1]:
            dB = torch.empty_like(B)
            with timed(f"{tag}/nce_bwd_cols"):
                rc = fn(*args, None, N.ptr(dB), 0, N.stream())
            N.check(rc, "nce_bwd(cols)")
        return dA, dB, None, None, None, None, None, None, None, None, None


def _i32(t):
    return None if t is None else t.to(torch.int32)


# The plain view's index arrays (rsx_nce_view_fill) depend on (N, M, diag_offset) only: filled once per
# size and device and kept (a training run has one batch size; the cache holds a few evaluation sizes too).
_nce_views: dict = {}


def _nce_view(n, m, off, device):
    key = (n, m, off, device)
    view = _nce_views.get(key)
    if view is None:
        if len(_nce_views) >= 16:
            _nce_views.clear()
        view = torch.empty(max(1, N.lib().rsx_nce_view_ints(n, m)), device=device, dtype=torch.int32)
        N.check(N.lib().rsx_nce_view_fill(n, m, off, N.ptr(view), N.stream()), "nce_view_fill")
        _nce_views[key] = view
    return view


class _NCEFused(torch.autograd.Function):
    """_NCE for flags 0 and 9 (no bias) on the fused grouped kernels (rsx_nce_fwd_grad /
    rsx_nce_bwd_cols, bf16x3 products): the forward also produces the row gradient, the backward is the
    column pass."""

    @staticmethod
    def forward(ctx, A, B, bias, k1a, k1b, tau, flags, diag_offset, tag):
        N.ensure_device(A)
        A = _c(A)
        B = _c(B)
        n, m = A.shape[0], B.shape[0]
        view = _nce_view(n, m, diag_offset, A.device)
        ws = torch.empty(N.lib().rsx_nce_fused_workspace_floats(n, m), device=A.device, dtype=torch.float32)
        out2 = torch.empty(2, device=A.device, dtype=torch.float32)
        ga = torch.empty(n, 128, device=A.device, dtype=torch.float32)
        k1a, k1b = _c(k1a), _c(k1b)
        with timed(f"{tag}/nce_fwd"):
            rc = N.lib().rsx_nce_fwd_grad(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1a), N.ptr(k1b), n, m, A.stride(0),
                                          B.stride(0), diag_offset, tau, flags, N.ptr(view), N.ptr(ws),
                                          N.ptr(out2), N.ptr(ga), N.stream())
        N.check(rc, "nce_fwd_grad")
        ctx.save_for_backward(A, B, bias, k1a, k1b, view, ws, ga)
        ctx.cfg = (n, m, tau, flags, diag_offset, tag)
        cnt = out2[1]
        ctx.mark_non_differentiable(cnt)
        return out2[0], cnt

    @staticmethod
    def backward(ctx, g, _gcnt):
        A, B, bias, k1a, k1b, view, ws, ga = ctx.saved_tensors
        n, m, tau, flags, off, tag = ctx.cfg
        g = _c(g.reshape(1).to(torch.float32))
        dA = ga * g  # the forward's row gradient, per unit upstream gradient
        dB = None
        if ctx.needs_input_grad[1]:
            dB = torch.empty(m, 128, device=B.device, dtype=torch.float32)
            with timed(f"{tag}/nce_bwd_cols"):
                rc = N.lib().rsx_nce_bwd_cols(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1a), N.ptr(k1b), n, m,
                                              A.stride(0), B.stride(0), off, tau, flags, N.ptr(view), N.ptr(g),
                                              N.ptr(ws), N.ptr(dB), N.stream())
            N.check(rc, "nce_bwd_cols")
        return dA, dB, None, None, None, None, None, None, None


def nce_sum(A, B, bias=None, k1a=None, k1b=None, k2a=None, k2b=None, tau=0.1, flags=NCE_PLAIN, diag_offset=0,
            tag="nce", precision=None):
    """(sum of row losses, valid-row count) of S = A B^T / tau - bias; row i's label column
    is i + diag_offset (see include/recsys_amd.h).
    flags: NCE_PLAIN, NCE_MASK_ITEM, NCE_MASK_ITEM_USER, NCE_SUPCON, or NCE_MASK_ITEM_POS (18: NCE_MASK_ITEM
    with the label logit S_ii left without its bias; plain kernels).
    precision: None = the plain kernels (bf16x3, or fp32 under set_nce_precision("fp32")), bit for bit
    what they always gave. "bf16x3" | "f16" (the grouped loss's modes, as ops.nce_precision() names them)
    = the fused grouped kernels where they apply (flags 0, and flags 9 without a bias, when A needs a
    gradient), with bf16x3 products in both modes: the f16 mode's one-MFMA gradient products do not hold
    1e-3 of the gradient's scale for these terms near convergence. "fp32" and every other case fall back
    to the plain kernels."""
    if precision is not None and precision not in NCE_PRECISIONS:
        raise ValueError(f"precision must be None or one of {sorted(NCE_PRECISIONS)}")
    if bias is not None:
        bias = _c(bias.to(torch.float32))
    flags = int(flags)
    fused = (precision in ("bf16x3", "f16") and A.requires_grad
             and torch.is_grad_enabled() and A.shape[1] == 128 and B.shape[1] == 128 and A.shape[0] > 0
             and (flags == NCE_PLAIN or (flags == NCE_SUPCON and bias is None and k1a is not None
                                         and k1b is not None)))
    if fused:
        return _NCEFused.apply(A, B, bias, _i32(k1a), _i32(k1b), float(tau), flags, int(diag_offset), str(tag))
    return _NCE.apply(A, B, bias, _i32(k1a), _i32(k1b), _i32(k2a), _i32(k2b), float(tau), flags,
                      int(diag_offset), str(tag))


def nce_loss(A, B, bias=None, k1a=None, k1b=None, k2a=None, k2b=None, tau=0.1, flags=NCE_PLAIN, tag="nce",
             precision=None):
    """Mean InfoNCE over valid rows (0 if none), the reference's F.cross_entropy mean."""
    total, cnt = nce_sum(A, B, bias, k1a, k1b, k2a, k2b, tau, flags, tag=tag, precision=precision)
    return total / cnt.clamp(min=1.0)


class _NCEEmphasis(torch.autograd.Function):
    """(sum of row losses, N) of full_batch_hard_emphasis_loss's cross-entropy (v1_refine_usertower.py
    :762-822): S = A B^T / tau - bias, same-key columns off the diagonal excluded (flags MASK_K1), and
    +margin on each row's mined columns top [N, K] -- the dense flags-2 InfoNCE pass plus the O(N K)
    rsx_nce_emphasis_fwd / _bwd correction; no N x N tensor."""

    @staticmethod
    def forward(ctx, A, B, bias, k1, top, tau, margin, tag):
        N.ensure_device(A)
        A = _c(A)
        B = _c(B)
        n, m = A.shape[0], B.shape[0]
        K = top.shape[1] if top.dim() == 2 else 0
        top = _c(top.to(torch.int64))
        x3 = _nce_precision != "fp32"
        prec = 1 if x3 else 0
        nws = (N.lib().rsx_nce_x3_workspace_floats(n, m) if x3
               else N.lib().rsx_nce_workspace_floats(n, m, _NSPLIT_FWD, _NSPLIT_BWD))
        ws = torch.empty(nws, device=A.device, dtype=torch.float32)
        out2 = torch.empty(2, device=A.device, dtype=torch.float32)
        flags = NCE_MASK_ITEM
        with timed(f"{tag}/nce_fwd"):
            if x3:
                rc = N.lib().rsx_nce_fwd_x3(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1), None, None, n, m,
                                            A.stride(0), B.stride(0), 0, tau, flags, N.ptr(ws), N.ptr(out2), N.stream())
            else:
                rc = N.lib().rsx_nce_fwd(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1), None, None, n, m,
                                         A.stride(0), B.stride(0), 0, tau, flags, _NSPLIT_FWD, N.ptr(ws), N.ptr(out2),
                                         N.stream())
            N.check(rc, "nce_fwd")
            rc = N.lib().rsx_nce_emphasis_fwd(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1), N.ptr(top), n, m,
                                              K, A.stride(0), B.stride(0), 0, tau, margin, prec, _NSPLIT_FWD,
                                              N.ptr(ws), N.ptr(out2), N.stream())
            N.check(rc, "nce_emphasis_fwd")
        # the mined entries in column order (stable: a fixed summation order per column) for the
        # backward's atomic-free dB pass
        flat = top.reshape(-1)
        key = torch.where((flat >= 0) & (flat < m), flat, torch.full_like(flat, m))
        sk, col_ent = torch.sort(key, stable=True)
        col_ptr = torch.searchsorted(sk, torch.arange(m + 1, device=A.device, dtype=sk.dtype))
        ctx.save_for_backward(A, B, bias, k1, top, ws, _c(col_ptr), _c(col_ent))
        ctx.cfg = (n, m, K, tau, margin, tag, x3)
        cnt = out2[1]
        ctx.mark_non_differentiable(cnt)
        return out2[0], cnt

    @staticmethod
    def backward(ctx, g, _gcnt):
        A, B, bias, k1, top, ws, col_ptr, col_ent = ctx.saved_tensors
        n, m, K, tau, margin, tag, x3 = ctx.cfg
        g = _c(g.reshape(1).to(torch.float32))
        head = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1), None, None, n, m, A.stride(0), B.stride(0), 0,
                tau, NCE_MASK_ITEM)
        if x3:
            fn, args = N.lib().rsx_nce_bwd_x3, head + (N.ptr(g), N.ptr(ws))
        else:
            fn, args = N.lib().rsx_nce_bwd, head + (_NSPLIT_FWD, _NSPLIT_BWD, N.ptr(g), N.ptr(ws))
        dA = torch.empty_like(A) if ctx.needs_input_grad[0] else None
        dB = torch.empty_like(B) if ctx.needs_input_grad[1] else None
        with timed(f"{tag}/nce_bwd"):
            if dA is not None:
                N.check(fn(*args, N.ptr(dA), None, 0, N.stream()), "nce_bwd(rows)")
            if dB is not None:
                N.check(fn(*args, None, N.ptr(dB), 0, N.stream()), "nce_bwd(cols)")
            if dA is not None or dB is not None:
                cbuf = torch.empty(n * K, device=A.device, dtype=torch.float32) if dB is not None else None
                rc = N.lib().rsx_nce_emphasis_bwd_csr(N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1),
                                                      N.ptr(top), n, m, K, A.stride(0), B.stride(0), 0, tau, margin,
                                                      1 if x3 else 0, _NSPLIT_FWD, N.ptr(col_ptr), N.ptr(col_ent),
                                                      N.ptr(cbuf), N.ptr(g), N.ptr(ws), N.ptr(dA), N.ptr(dB),
                                                      N.stream())
                N.check(rc, "nce_emphasis_bwd")
        return dA, dB, None, None, None, None, None, None


def nce_emphasis_loss(A, B, keys, top, margin, bias=None, tau=0.1, tag="hard_emphasis"):
    """Mean over the N rows of CE(A B^T / tau - bias + margin on each row's mined columns top [N, K],
    same-key columns off the diagonal at -inf; label = diagonal) -- full_batch_hard_emphasis_loss's
    objective (v1_refine_usertower.py:546-554) without its N x N tensors. margin is in logit units
    (the reference's hard_margin / temperature). A [N, 128], B [N, 128], keys [N] int. The mined ids of
    one row must be distinct (a repeated id is counted twice where the reference's scatter_ sets it once)."""
    if A.shape[0] != B.shape[0]:
        raise ValueError("nce_emphasis_loss: A and B must have the same number of rows (label = diagonal)")
    if bias is not None:
        bias = _c(bias.to(torch.float32))
    total, cnt = _NCEEmphasis.apply(A, B, bias, _c(keys.to(torch.int32)), top, float(tau), float(margin), str(tag))
    return total / cnt.clamp(min=1.0)


# ----------------------------------------------------------------------------------------
# Grouped form of the live LogQ loss (distinct targets as columns, exact multiplicities)
class TargetGroups:
    """Index structures for rsx_nce_grouped_*: built on the GPU with a few sorts.

    t_rows/u_rows: this process's rows (flat order; rows of one user are contiguous and user
    ids are non-decreasing). t_cols: every column's target (all ranks' rows; defaults to
    t_rows). The distinct targets of t_cols are the grouped columns."""

    def __init__(self, t_rows, u_rows, t_cols=None):
        t_cols = t_rows if t_cols is None else t_cols
        dev = t_rows.device
        self.uniq, col_cnt = torch.unique(t_cols, sorted=True, return_counts=True)
        D = self.uniq.numel()
        self.colcnt = col_cnt.to(torch.float32)
        inv = torch.searchsorted(self.uniq, t_rows)
        self.row_col = inv.to(torch.int32)
        n = t_rows.numel()
        # rows of each user: [start, end) in flat order
        users, ucnt = torch.unique_consecutive(u_rows, return_counts=True)
        ends = torch.cumsum(ucnt, 0)
        starts = ends - ucnt
        self.row_beg = torch.repeat_interleave(starts, ucnt).to(torch.int32)
        self.row_end = torch.repeat_interleave(ends, ucnt).to(torch.int32)
        # per-row exception list = the user's own targets, sorted within each user segment
        seg = torch.repeat_interleave(torch.arange(users.numel(), device=dev), ucnt)
        key = seg * D + inv
        self.exc_cols = (torch.sort(key).values % D).to(torch.int32)
        # per-column list of (user row range, multiplicity), sorted by column then user
        key2 = inv * users.numel() + seg
        k2, kn = torch.unique_consecutive(torch.sort(key2).values, return_counts=True)
        pd = torch.div(k2, users.numel(), rounding_mode="floor")
        pseg = k2 % users.numel()
        self.exc_s = starts[pseg].to(torch.int32)
        self.exc_e = ends[pseg].to(torch.int32)
        self.exc_n = kn.to(torch.int32)
        ar = torch.arange(D, device=dev)
        self.col_beg = torch.searchsorted(pd, ar).to(torch.int32)
        self.col_end = torch.searchsorted(pd, ar, right=True).to(torch.int32)
        self.n_rows = n
        self.n_cols = D

    @classmethod
    def from_arrays(cls, uniq, colcnt, row_col, row_beg, row_end, exc_cols, exc_s, exc_e, exc_n, col_beg, col_end,
                    n_rows):
        """The same structure from prepared arrays (rsx_step_index_fill, dist.py)."""
        g = cls.__new__(cls)
        g.uniq, g.colcnt, g.row_col, g.row_beg, g.row_end, g.exc_cols = uniq, colcnt, row_col, row_beg, row_end, exc_cols
        g.exc_s, g.exc_e, g.exc_n, g.col_beg, g.col_end = exc_s, exc_e, exc_n, col_beg, col_end
        g.n_rows, g.n_cols = int(n_rows), uniq.numel()
        return g


# bf16x3 + the rows need a gradient: the forward also produces the row gradient (one sweep of
# S instead of two; rsx_nce_grouped_fwd_grad). RSX_NCE_FUSED_ROWGRAD=0 restores the separate
# backward row pass.
_NCE_FUSED_ROWGRAD = os.environ.get("RSX_NCE_FUSED_ROWGRAD", "1") != "0"


class _NCEGrouped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, bias, grp, tau, tag, prec):
        N.ensure_device(A)
        A = _c(A)
        B = _c(B)
        n, d = A.shape[0], B.shape[0]
        nws = N.lib().rsx_nce_grouped_workspace_floats(n, d, _NSPLIT_FWD_GROUPED, _NSPLIT_BWD, prec)
        ws = torch.empty(nws, device=A.device, dtype=torch.float32)
        out2 = torch.empty(2, device=A.device, dtype=torch.float32)
        fused = _NCE_FUSED_ROWGRAD and prec != NCE_PRECISIONS["fp32"] and ctx.needs_input_grad[0]
        ga = None
        with timed(f"{tag}/nce_fwd"):
            if fused:
                ga = torch.empty(n, 128, device=A.device, dtype=torch.float32)
                rc = N.lib().rsx_nce_grouped_fwd_grad(
                    N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(grp.colcnt), N.ptr(grp.row_col), N.ptr(grp.row_beg),
                    N.ptr(grp.row_end), N.ptr(grp.exc_cols), n, d, A.stride(0), B.stride(0), tau, prec,
                    _NSPLIT_FWD_GROUPED, N.ptr(ws), N.ptr(out2), N.ptr(ga), N.stream())
            else:
                rc = N.lib().rsx_nce_grouped_fwd(
                    N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(grp.colcnt), N.ptr(grp.row_col), N.ptr(grp.row_beg),
                    N.ptr(grp.row_end), N.ptr(grp.exc_cols), n, d, A.stride(0), B.stride(0), tau, prec,
                    _NSPLIT_FWD_GROUPED, N.ptr(ws), N.ptr(out2), N.stream())
        N.check(rc, "nce_grouped_fwd")
        ctx.save_for_backward(A, B, bias, ws, ga)
        ctx.grp = grp
        ctx.cfg = (n, d, tau, tag, prec)
        cnt = out2[1]
        ctx.mark_non_differentiable(cnt)
        return out2[0], cnt

    @staticmethod
    def backward(ctx, g, _gcnt):
        A, B, bias, ws, ga = ctx.saved_tensors
        grp = ctx.grp
        n, d, tau, tag, prec = ctx.cfg
        g = _c(g.reshape(1).to(torch.float32))
        args = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(grp.colcnt), N.ptr(grp.row_col), N.ptr(grp.row_beg),
                N.ptr(grp.row_end), N.ptr(grp.exc_cols), N.ptr(grp.col_beg), N.ptr(grp.col_end), N.ptr(grp.exc_s),
                N.ptr(grp.exc_e), N.ptr(grp.exc_n), n, d, A.stride(0), B.stride(0), tau, prec, _NSPLIT_FWD_GROUPED,
                _NSPLIT_BWD,
                N.ptr(g), N.ptr(ws))
        dA = dB = None
        if ctx.needs_input_grad[0]:
            if ga is not None:  # the forward's row gradient, per unit upstream gradient
                dA = ga * g
            else:
                dA = torch.empty_like(A)
                with timed(f"{tag}/nce_bwd_rows"):
                    rc = N.lib().rsx_nce_grouped_bwd(*args, N.ptr(dA), None, 0, N.stream())
                N.check(rc, "nce_grouped_bwd(rows)")
        if ctx.needs_input_grad[1]:
            dB = torch.empty_like(B)
            with timed(f"{tag}/nce_bwd_cols"):
                rc = N.lib().rsx_nce_grouped_bwd(*args, None, N.ptr(dB), 0, N.stream())
            N.check(rc, "nce_grouped_bwd(cols)")
        return dA, dB, None, None, None, None, None


def nce_grouped_sum(A, B_distinct, bias, groups: TargetGroups, tau=0.1, tag="nce", precision=None):
    """(sum of row losses, N) of the live LogQ loss with same-item / same-user masking, with
    the columns given as the distinct targets (B_distinct[d] = normalised item groups.uniq[d]).
    precision: "fp32" | "bf16x3" | "f16" | None (= set_nce_precision / RSX_NCE_PRECISION).
    "f16" scales the operands by 2^8 into fp16: every component of A and B_distinct must have
    |x| < 256 (the callers pass unit-norm rows)."""
    if bias is not None:
        bias = _c(bias.to(torch.float32))
    prec = NCE_PRECISIONS[precision or _nce_precision]
    return _NCEGrouped.apply(A, B_distinct, bias, groups, float(tau), str(tag), prec)


class _LossCombine(torch.autograd.Function):
    """total = s_main / n + lambda_cl * (s_un / b + lambda_sup * s_sup / max(cnt, 1)) on the device
    (rsx_loss_combine), with (total, main, cl) also returned detached for logging."""

    @staticmethod
    def forward(ctx, s_main, s_un, s_sup, cnt, consts):
        inv_n, inv_b, lsup, lcl = consts
        total = torch.empty((), device=s_un.device, dtype=torch.float32)
        logs = torch.empty(3, device=s_un.device, dtype=torch.float32)
        rc = N.lib().rsx_loss_combine(N.ptr(s_main), N.ptr(s_un), N.ptr(s_sup), N.ptr(cnt), inv_n, inv_b, lsup, lcl,
                                      N.ptr(total), N.ptr(logs), N.stream())
        N.check(rc, "loss_combine")
        ctx.consts = consts
        ctx.has = (s_main is not None, s_sup is not None)
        ctx.save_for_backward(cnt)
        ctx.mark_non_differentiable(logs)
        return total, logs

    @staticmethod
    def backward(ctx, g, _glogs):
        (cnt,) = ctx.saved_tensors
        inv_n, inv_b, lsup, lcl = ctx.consts
        g3 = torch.empty(3, device=g.device, dtype=torch.float32)
        rc = N.lib().rsx_loss_combine_bwd(N.ptr(_c(g.reshape(1))), N.ptr(cnt), inv_n, inv_b, lsup, lcl, N.ptr(g3),
                                          N.stream())
        N.check(rc, "loss_combine_bwd")
        has_main, has_sup = ctx.has
        return (g3[0] if has_main else None), g3[1], (g3[2] if has_sup else None), None, None


def loss_combine(s_main, s_un, s_sup, cnt, n, b, lambda_sup, lambda_cl):
    """(objective, detached [total, main, cl]) of the contrastive step from device scalars:
    s_main / n + lambda_cl * (s_un / b + lambda_sup * s_sup / max(cnt, 1)); s_main / s_sup may be
    None (no valid step / lambda_sup = 0), cnt is not differentiated."""
    if s_un is None:
        raise ValueError("loss_combine: s_un is required")
    _f32_vec("loss_combine", "s_un", s_un, 1, None)
    _f32_vec("loss_combine", "s_main", s_main, 1, s_un)
    _f32_vec("loss_combine", "s_sup", s_sup, 1, s_un)
    _f32_vec("loss_combine", "cnt", cnt, 1, s_un)
    N.ensure_device(s_un)
    consts = (1.0 / float(n) if n else 0.0, 1.0 / float(b), float(lambda_sup), float(lambda_cl))
    cnt = None if cnt is None else _c(cnt.detach().reshape(1))
    return _LossCombine.apply(s_main, s_un, s_sup, cnt, consts)


# ----------------------------------------------------------------------------------------
# The step's tail: clip_grad_norm_ + AdamW.step (v1_usertower_train.py:852-853), rsx_clip_adamw
_CLIP_ADAMW = os.environ.get("RSX_CLIP_ADAMW", "1") != "0"


def _adamw_native_ok(opt) -> bool:
    """torch.optim.AdamW configurations rsx_clip_adamw reproduces: no amsgrad / maximize /
    capturable / differentiable, float hyper-parameters, no step hooks."""
    if type(opt) is not torch.optim.AdamW or opt._optimizer_step_pre_hooks or opt._optimizer_step_post_hooks:
        return False
    from torch.optim import optimizer as _om
    if _om._global_optimizer_pre_hooks or _om._global_optimizer_post_hooks:
        return False
    if torch.get_default_dtype() != torch.float32:
        return False
    for g in opt.param_groups:
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            return False
        if not g.get("decoupled_weight_decay", True):
            return False
        if any(isinstance(v, torch.Tensor) for v in (g["lr"], g["eps"], g["weight_decay"], *g["betas"])):
            return False
    return True


# per-optimizer pointer / size arrays of rsx_clip_adamw, reused while the parameter list, the
# clip set and the state tensors are the same objects (rebuilt otherwise; gradients every step)
_ADAMW_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def module_params(model):
    """The set of model.parameters() (same members: every registered, non-None parameter of the
    module tree, each once) by a plain walk of _modules / _parameters: the clip set of the step,
    where only membership matters, without named_parameters()' prefix strings (~0.2 ms per step)."""
    out, seen, stack = [], set(), [model]
    while stack:
        m = stack.pop()
        for p in m._parameters.values():
            if p is not None and id(p) not in seen:
                seen.add(id(p))
                out.append(p)
        stack.extend(c for c in m._modules.values() if c is not None)
    return out


def clip_adamw_step(optimizer, clip_params, max_norm: float):
    """torch.nn.utils.clip_grad_norm_(clip_params, max_norm) followed by optimizer.step() for a
    torch.optim.AdamW, as two launches (rsx_clip_adamw) instead of torch's ~10 (per-tensor norms,
    stack, norm, clamp, foreach multiply, the AdamW kernels) and their ~1 ms of host time.
    Same state (optimizer.state[p]: step / exp_avg / exp_avg_sq, created as torch does), same
    in-place gradient scaling; the update follows torch's fused AdamW arithmetic. Returns the
    total norm (device scalar), or None when the optimizer or a tensor is one this does not
    handle (sparse / non-fp32 / non-contiguous / CPU, a clipped parameter the optimizer does not
    own): then nothing was changed and the caller runs torch's pair."""
    if not _CLIP_ADAMW or not _adamw_native_ok(optimizer):
        return None
    clip_ids = {id(p) for p in clip_params if p.grad is not None}
    items = []
    for g in optimizer.param_groups:
        for p in g["params"]:
            gr = p.grad
            if gr is None:
                continue
            if (gr.is_sparse or p.dtype != torch.float32 or gr.dtype != torch.float32 or p.device.type != "cuda"
                    or not p.is_contiguous() or not gr.is_contiguous() or gr.shape != p.shape):
                return None
            items.append((p, gr, g))
    if not items:
        return None
    if sum(1 for p, _, _ in items if id(p) in clip_ids) != len(clip_ids):
        return None
    N.ensure_device(items[0][0])
    state = optimizer.state
    for p, gr, g in items:
        st = state[p]
        if len(st) == 0:   # torch.optim.Adam._init_group
            st["step"] = (torch.zeros((), dtype=torch.float32, device=p.device) if g["fused"]
                          else torch.tensor(0.0, dtype=torch.float32))
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    sts = [state[p] for p, _, _ in items]
    sig = (tuple(id(p) for p, _, _ in items), frozenset(clip_ids),
           tuple((id(st["exp_avg"]), id(st["exp_avg_sq"]), id(st["step"])) for st in sts))
    c = _ADAMW_CACHE.get(optimizer)
    if c is None or c["sig"] != sig:
        m_l, v_l, dev_steps, cpu_steps = [], [], [], []
        for st in sts:
            m, v, s = st["exp_avg"], st["exp_avg_sq"], st["step"]
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == torch.float32 and v.dtype == torch.float32):
                return None
            m_l.append(m)
            v_l.append(v)
            (dev_steps if s.device.type == "cuda" else cpu_steps).append(s)
        n = len(items)
        numel = N.i64_array([p.numel() for p, _, _ in items])
        clip = (ctypes.c_int * n)(*[1 if id(p) in clip_ids else 0 for p, _, _ in items])
        steps_t = [st["step"] for st in sts]
        c = {"sig": sig, "n": n, "dev_steps": dev_steps, "cpu_steps": cpu_steps, "steps_t": steps_t,
             # the tensors are held so that the ids in sig cannot be reused by other objects
             "hold": (m_l, v_l, [p for p, _, _ in items]),
             "ps": N.ptr_array([p for p, _, _ in items]), "ms": N.ptr_array(m_l), "vs": N.ptr_array(v_l),
             "numel": numel, "clip": clip,
             "step_d": N.ptr_array([s if s.device.type == "cuda" else None for s in steps_t]) if dev_steps else None,
             "nbytes": N.lib().rsx_clip_adamw_workspace_bytes(n, numel, clip)}
        _ADAMW_CACHE[optimizer] = c
    n = c["n"]
    # the step counts first, as torch's AdamW does (one multi-tensor launch for device counts)
    if c["dev_steps"]:
        torch._foreach_add_(c["dev_steps"], 1.0)
    if c["cpu_steps"]:
        torch._foreach_add_(c["cpu_steps"], 1.0)
    gs = N.ptr_array([gr for _, gr, _ in items])
    step_h = (ctypes.c_float * n)(*[0.0 if s.device.type == "cuda" else float(s) for s in c["steps_t"]])
    lr = (ctypes.c_double * n)(*[g["lr"] for _, _, g in items])   # doubles, as torch's kernels take them
    wd = (ctypes.c_double * n)(*[g["weight_decay"] for _, _, g in items])
    b1 = (ctypes.c_double * n)(*[g["betas"][0] for _, _, g in items])
    b2 = (ctypes.c_double * n)(*[g["betas"][1] for _, _, g in items])
    eps = (ctypes.c_double * n)(*[g["eps"] for _, _, g in items])
    dev = items[0][0].device
    nbytes = c["nbytes"]
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    norm = torch.empty((), device=dev, dtype=torch.float32)
    rc = N.lib().rsx_clip_adamw(n, c["ps"], gs, c["ms"], c["vs"], c["numel"], c["clip"], step_h, c["step_d"], lr, wd,
                                b1, b2, eps, float(max_norm), N.ptr(ws), nbytes, N.ptr(norm), N.stream())
    N.check(rc, "clip_adamw")
    optimizer._opt_called = True   # what torch's step wrapper records (LR schedulers check it)
    return norm


def zero_grad_(optimizer) -> None:
    """optimizer.zero_grad(set_to_none=True) without the profiler record_function around it."""
    for g in optimizer.param_groups:
        for p in g["params"]:
            p.grad = None


# ----------------------------------------------------------------------------------------
# Static-profile embeddings (several tiny gated tables, concatenated): rsx_static_embed_*
class _StaticEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, ids, padding_idx, *tables):
        N.ensure_device(gate)
        ids = [_c(t) for t in ids]
        tables = [_c(t) for t in tables]
        B = ids[0].shape[0]
        dims = [t.shape[1] for t in tables]
        out = torch.empty(B, sum(dims), device=gate.device, dtype=torch.float32)
        gate = _c(gate)
        rc = N.lib().rsx_static_embed_fwd(N.ptr_array(ids), N.ptr_array(tables),
                                          N.i64_array([t.shape[0] for t in tables]), N.i64_array(dims), len(tables),
                                          N.ptr(gate), B, N.ptr(out), out.stride(0), N.stream())
        N.check(rc, "static_embed_fwd")
        ctx.save_for_backward(gate, *ids, *tables)
        ctx.cfg = (len(tables), list(padding_idx))
        return out

    @staticmethod
    def backward(ctx, dout):
        nt, pad = ctx.cfg
        saved = ctx.saved_tensors
        gate, ids, tables = saved[0], list(saved[1:1 + nt]), list(saved[1 + nt:1 + 2 * nt])
        need = ctx.needs_input_grad
        dgate, *dtabs = _empty_group([gate if need[0] else None] +
                                     [t if need[3 + j] else None for j, t in enumerate(tables)])
        dout = _c(dout)
        B = ids[0].shape[0]
        rows = N.i64_array([t.shape[0] for t in tables])
        dims = N.i64_array([t.shape[1] for t in tables])
        nws = N.lib().rsx_static_embed_bwd_workspace_floats(B, nt, rows, dims)
        ws = torch.empty(nws, device=dout.device, dtype=torch.float32)
        rc = N.lib().rsx_static_embed_bwd(N.ptr_array(ids), N.ptr_array(tables), rows, dims, N.i64_array(pad), nt,
                                          N.ptr(gate), N.ptr(dout), dout.stride(0), B, B, N.ptr_array(dtabs),
                                          N.ptr(dgate), 0, N.ptr(ws), nws, N.stream())  # written
        N.check(rc, "static_embed_bwd")
        return (dgate, None, None, *dtabs)


def static_embed(ids, tables, gate, padding_idx=None):
    """cat_j(tables[j][ids[j]] * gate[j]) -> [B, sum_j dim_j] (nn.Embedding padding_idx
    semantics for the gradient)."""
    if padding_idx is None:
        padding_idx = [-1] * len(tables)
    padding_idx = [(-1 if p is None else int(p)) for p in padding_idx]
    return _StaticEmbed.apply(gate, list(ids), padding_idx, *tables)


# ----------------------------------------------------------------------------------------
# A4: the static profile as one native call per direction (rsx_static_profile_*)
_SP_IDS, _SP_TABLES, _SP_GATE, _SP_N = 0, 16, 32, 40


class _StaticProfile(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, static_gate, cont, wc, bc, wm, bm, ln_w, ln_b, *tables):
        ids, pads, eps, p_drop, seed, U = cfg
        N.ensure_device(static_gate)
        ids = [_c(t) for t in ids]
        tables = [_c(t) for t in tables]
        params = [_c(t) for t in (static_gate, cont, wc, bc, wm, bm, ln_w, ln_b)]
        src = ids[0].shape[0]
        nt = len(tables)
        ptrs = [None] * _SP_N
        ptrs[_SP_IDS:_SP_IDS + nt] = ids
        ptrs[_SP_TABLES:_SP_TABLES + nt] = tables
        ptrs[_SP_GATE:_SP_N] = params
        p_arr = N.ptr_array(ptrs)
        dims = N.i64_array([U, nt, cont.shape[1], wc.shape[0], wm.shape[1], src] + [t.shape[0] for t in tables]
                           + [t.shape[1] for t in tables] + list(pads))
        lib = N.lib()
        arena = torch.empty(lib.rsx_static_profile_arena_bytes(U), device=static_gate.device, dtype=torch.uint8)
        out = torch.empty(U, wm.shape[0], device=static_gate.device, dtype=torch.float32)
        rc = lib.rsx_static_profile_fwd(p_arr, dims, eps, p_drop, seed, N.ptr(arena), arena.numel(), N.ptr(out),
                                        N.stream())
        N.check(rc, "static_profile_fwd")
        # the kernel range-checks the nine ids (an out-of-range id reads and scatters row 0 and sets
        # the flag in the arena's first int32): raised as IndexError at the next poll / check
        _STATIC_IDS.watch(arena[:4].view(torch.int32))
        # the parameters and tables through autograd's saved tensors, so an in-place change between
        # forward and backward raises instead of the backward reading the new values
        ctx.save_for_backward(*params, *tables)
        ctx.keep = (p_arr, dims, ptrs, arena, p_drop, seed, U)
        return out

    @staticmethod
    def backward(ctx, dout):
        ctx.saved_tensors  # noqa: B018 -- the version check of the saved parameters and tables
        p_arr, dims, ptrs, arena, p_drop, seed, U = ctx.keep
        nt = len(ctx.needs_input_grad) - 9
        likes = [ptrs[_SP_GATE]] + [None] + ptrs[_SP_GATE + 2:_SP_N] + ptrs[_SP_TABLES:_SP_TABLES + nt]
        if U == 0:
            grads = [None if t is None else torch.zeros_like(t) for t in likes]
        else:
            grads = _empty_group(likes)
            g_ptrs = [None] * _SP_N
            g_ptrs[_SP_GATE:_SP_N] = grads[:8]
            g_ptrs[_SP_TABLES:_SP_TABLES + nt] = grads[8:]
            lib = N.lib()
            nws = lib.rsx_static_profile_bwd_workspace_bytes(U)
            ws = torch.empty(nws, device=dout.device, dtype=torch.uint8)
            rc = lib.rsx_static_profile_bwd(p_arr, dims, p_drop, seed, N.ptr(arena), N.ptr(_c(dout)),
                                            N.ptr_array(g_ptrs), N.ptr(ws), nws, N.stream())
            N.check(rc, "static_profile_bwd")
        return (None, *grads)


def static_profile(model, ids, cont_feats, p_drop, rows=None):
    """SASRecUserTower phase 2 (v1_refine_usertower.py:472-494): sigmoid(static_gate), the nine
    gated lookups, relu(cont_proj(cont)) * u_g[9], static_mlp (Linear + LayerNorm + GELU +
    Dropout) -> [rows, 128], as rsx_static_profile_fwd / _bwd (dropout: counter-hash mask).
    ids (nine int64 [B]) / cont_feats [B, 4] hold B users; rows (default B, a multiple of B):
    output row r is user r % B (the two dropout views of the contrastive step: rows = 2B)."""
    B = ids[0].shape[0]
    rows = B if rows is None else int(rows)
    if B == 0 or rows % B:
        raise ValueError(f"static_profile: rows ({rows}) must be a positive multiple of the users ({B})")
    embs = [model.age_emb, model.price_emb, model.cnt_emb, model.recency_emb, model.channel_emb,
            model.club_status_emb, model.news_freq_emb, model.fn_emb, model.active_emb]
    lin, ln = model.static_mlp[0], model.static_mlp[1]
    seed = next_seed() if p_drop > 0 else 0
    pads = [(-1 if e.padding_idx is None else int(e.padding_idx)) for e in embs]
    cfg = ([t.to(torch.int64) for t in ids], pads, float(ln.eps), float(p_drop), seed, rows)
    return _StaticProfile.apply(cfg, model.static_gate, cont_feats.to(torch.float32), model.cont_proj.weight,
                                model.cont_proj.bias,
                                lin.weight, lin.bias, ln.weight, ln.bias, *[e.weight for e in embs])


# ----------------------------------------------------------------------------------------
# LayerNorm (+ residual add + dropout before it, + GELU after it): rsx_ln_fwd / rsx_ln_bwd
ACT_GELU_ERF = 2


def _ln_bwd(s, mean, rstd, w, b, act, dy, ds_in, p_drop, seed, want_dx, want_dres, want_w, want_b):
    T, D = s.shape
    dx = torch.empty_like(s) if want_dx or want_dres else None
    dres = torch.empty_like(s) if want_dres else None
    dw = torch.empty(D, device=s.device, dtype=torch.float32) if want_w else None
    db = torch.empty(D, device=s.device, dtype=torch.float32) if want_b else None
    nws = N.lib().rsx_ln_bwd_workspace_floats(T, D)
    ws = torch.empty(nws, device=s.device, dtype=torch.float32) if (want_w or want_b) else None
    with timed("ln_bwd"):
        rc = N.lib().rsx_ln_bwd(N.ptr(s), N.ptr(mean), N.ptr(rstd), N.ptr(w), N.ptr(b), act, N.ptr(_c(dy)),
                                N.ptr(None if ds_in is None else _c(ds_in)), p_drop, seed, T, D, N.ptr(dx),
                                N.ptr(dres), N.ptr(dw), N.ptr(db), N.ptr(ws), nws if ws is not None else 0,
                                N.stream())
    N.check(rc, "ln_bwd")
    return dx, dres, dw, db


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps, act):
        N.ensure_device(x)
        x = _c(x)
        T, D = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(T, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        with timed("ln_fwd"):
            rc = N.lib().rsx_ln_fwd(N.ptr(x), None, 0.0, 0, N.ptr(w), N.ptr(b), eps, act, T, D, None, N.ptr(y),
                                    N.ptr(mean), N.ptr(rstd), N.stream())
        N.check(rc, "ln_fwd")
        ctx.save_for_backward(x, mean, rstd, w, b)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, _, dw, db = _ln_bwd(x, mean, rstd, w, b, ctx.act, dy, None, 0.0, 0, need[0], False, need[1], need[2])
        return dx, dw, db, None, None


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, w, b, eps, p_drop, seed):
        N.ensure_device(x)
        x = _c(x)
        res = _c(res)
        T, D = x.shape
        s = torch.empty_like(x)
        y = torch.empty_like(x)
        mean = torch.empty(T, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        with timed("ln_fwd"):
            rc = N.lib().rsx_ln_fwd(N.ptr(x), N.ptr(res), p_drop, seed, N.ptr(w), N.ptr(b), eps, 0, T, D, N.ptr(s),
                                    N.ptr(y), N.ptr(mean), N.ptr(rstd), N.stream())
        N.check(rc, "ln_fwd")
        ctx.save_for_backward(s, mean, rstd, w, b)
        ctx.cfg = (p_drop, seed)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, mean, rstd, w, b = ctx.saved_tensors
        p_drop, seed = ctx.cfg
        need = ctx.needs_input_grad
        if dy is None:
            dy = torch.zeros_like(s)
        dx, dres, dw, db = _ln_bwd(s, mean, rstd, w, b, 0, dy, ds, p_drop, seed, need[0], need[1], need[2], need[3])
        return dx, dres, dw, db, None, None, None


class _LayerNormPass(torch.autograd.Function):
    """(x, LayerNorm(x)): the first norm1 of a norm_first encoder, whose input also feeds the
    residual. The backward adds the residual-path gradient inside the LayerNorm backward
    (ds_in) instead of autograd's separate add of two [T, D] gradients."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        N.ensure_device(x)
        T, D = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(T, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        with timed("ln_fwd"):
            rc = N.lib().rsx_ln_fwd(N.ptr(x), None, 0.0, 0, N.ptr(w), N.ptr(b), eps, 0, T, D, None, N.ptr(y),
                                    N.ptr(mean), N.ptr(rstd), N.stream())
        N.check(rc, "ln_fwd")
        ctx.save_for_backward(x, mean, rstd, w, b)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dx_pass, dy):
        x, mean, rstd, w, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dy is None:
            return dx_pass, None, None, None
        dx, _, dw, db = _ln_bwd(x, mean, rstd, w, b, 0, dy, dx_pass, 0.0, 0, need[0], False, need[1], need[2])
        return dx, dw, db, None


def layer_norm_pass(x, weight, bias, eps=1e-5):
    """(x, LayerNorm(x)) with the residual gradient of x folded into the LayerNorm backward."""
    _ln_args("layer_norm_pass", x, None, weight, bias)
    shp = x.shape
    x2, y = _LayerNormPass.apply(_c(x.reshape(-1, shp[-1])), weight, bias, float(eps))
    return x2.reshape(shp), y.reshape(shp)


class _AddDropout(torch.autograd.Function):
    """s = x + dropout_p(res) in one pass (rsx_ln_fwd's add-only form); backward dx = ds,
    dres = mask(ds) (rsx_dropout_bwd, the same counter hash)."""

    @staticmethod
    def forward(ctx, x, res, p_drop, seed):
        N.ensure_device(x)
        T, D = x.shape
        s = torch.empty_like(x)
        rc = N.lib().rsx_ln_fwd(N.ptr(x), N.ptr(res), p_drop, seed, None, None, 0.0, 0, T, D, N.ptr(s), None,
                                None, None, N.stream())
        N.check(rc, "ln_fwd(add)")
        ctx.cfg = (p_drop, seed, T, D)
        return s

    @staticmethod
    def backward(ctx, ds):
        p_drop, seed, T, D = ctx.cfg
        ds = _c(ds)
        dres = None
        if ctx.needs_input_grad[1]:
            dres = torch.empty_like(ds)
            rc = N.lib().rsx_dropout_bwd(N.ptr(ds), T, D, p_drop, seed, N.ptr(dres), N.stream())
            N.check(rc, "dropout_bwd")
        return ds, dres, None, None


def add_dropout(x, res, p_drop=0.0, training=True):
    """x + F.dropout(res, p_drop, training) as one kernel (counter-hash mask; p = 0 in eval)."""
    _ln_args("add_dropout", x, res, None, None)
    p = float(p_drop) if training else 0.0
    shp = x.shape
    seed = next_seed() if p > 0 else 0
    s = _AddDropout.apply(_c(x.reshape(-1, shp[-1])), _c(res.reshape(-1, shp[-1])), p, seed)
    return s.reshape(shp)


def layer_norm(x, weight, bias, eps=1e-5, act=0):
    """act(LayerNorm(x)) over the last dim (act 0 none / ACT_GELU_ERF)."""
    _ln_args("layer_norm", x, None, weight, bias)
    shp = x.shape
    y = _LayerNorm.apply(x.reshape(-1, shp[-1]), weight, bias, float(eps), int(act))
    return y.reshape(shp)


@torch.no_grad()
def add_layer_norm_infer(x, res, weight, bias, eps=1e-5):
    """LayerNorm(x + res) forward only (no statistics saved, the sum not written): inference,
    e.g. BERT's post-norm residuals in item_tower.bert_cls_packed. Hidden up to 1024."""
    _ln_args("add_layer_norm_infer", x, res, weight, bias)
    if x.dim() != 2:
        raise ValueError(f"add_layer_norm_infer: x must be [T, D], got shape {tuple(x.shape)}")
    N.ensure_device(x)
    x = _c(x)
    res = _c(res)
    T, D = x.shape
    y = torch.empty_like(x)
    rc = N.lib().rsx_ln_fwd(N.ptr(x), N.ptr(res), 0.0, 0, N.ptr(weight), N.ptr(bias), float(eps), 0, T, D, None,
                            N.ptr(y), None, None, N.stream())
    N.check(rc, "ln_fwd(add, inference)")
    return y


def add_layer_norm(x, res, weight, bias, eps=1e-5, p_drop=0.0):
    """(s, LayerNorm(s)) with s = x + dropout(res): the residual add of a norm_first encoder
    layer fused with the next LayerNorm."""
    _ln_args("add_layer_norm", x, res, weight, bias)
    shp = x.shape
    seed = next_seed() if p_drop > 0 else 0
    s, y = _AddLayerNorm.apply(x.reshape(-1, shp[-1]), res.reshape(-1, shp[-1]), weight, bias, float(eps),
                               float(p_drop), seed)
    return s.reshape(shp), y.reshape(shp)


# ----------------------------------------------------------------------------------------
# Token-level linear layers: forward / dX on rsx_gemm_x3, dW / db on rsx_linear_wgrad(_x3)
# Token-linear GEMM precision: "bf16x3" = rsx_gemm_x3 / rsx_linear_wgrad_x3 (hi/lo bf16 split
# on the bf16 MFMA, ~2^-17 relative error per product), "fp32" = the library fp32 GEMM for the
# forward / input gradient and the fp32-MFMA rsx_linear_wgrad. RSX_GEMM_PRECISION selects.
GEMM_PRECISIONS = ("fp32", "bf16x3")
_gemm_precision = os.environ.get("RSX_GEMM_PRECISION", "bf16x3")
EPI_BIAS, EPI_GELU_DROP, EPI_DGELU_DROP = 0, 1, 2
EPI_RELU = 3   # C = max(acc + bias, 0): inference only (no aux, p_drop 0)


def set_gemm_precision(p: str) -> str:
    """Set the token-linear GEMM precision ("fp32" | "bf16x3"); returns the previous mode."""
    global _gemm_precision
    if p not in GEMM_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(GEMM_PRECISIONS)}")
    prev, _gemm_precision = _gemm_precision, p
    return prev


def _x3_ok(m_out: int, k_in: int) -> bool:
    return _gemm_precision == "bf16x3" and m_out % 128 == 0 and k_in % 32 == 0


def gemm_x3(a, b, bias=None, epi=EPI_BIAS, aux=None, p_drop=0.0, seed=0, tag=None):
    """epi(a [M, K] @ b [N, K]^T + bias) on rsx_gemm_x3 (N % 128 == 0, K % 32 == 0).
    EPI_GELU_DROP returns dropout(gelu(pre)) and writes gelu'(pre) into aux;
    EPI_DGELU_DROP returns (a @ b^T) * keep / (1 - p) * aux."""
    a = _c(a)
    b = _c(b)
    M, K = a.shape
    n = b.shape[0]
    out = torch.empty(M, n, device=a.device, dtype=torch.float32)
    if M == 0:
        return out
    nws = N.lib().rsx_gemm_x3_split_floats(M, n, K)  # > 0: split-K for a shape with fewer tiles than CUs
    ws = torch.empty(nws, device=a.device, dtype=torch.float32) if nws > 0 else None
    with timed(tag or "gemm_x3"):
        rc = N.lib().rsx_gemm_x3_ws(N.ptr(a), a.stride(0), N.ptr(b), b.stride(0),
                                    N.ptr(None if bias is None else _c(bias)), M, n, K, epi, N.ptr(aux),
                                    0 if aux is None else aux.stride(0), float(p_drop), int(seed), N.ptr(out),
                                    out.stride(0), N.ptr(ws), nws, N.stream())
    N.check(rc, "gemm_x3")
    return out


def _tn_ok(w) -> bool:
    """rsx_gemm_x3_tn takes W [out, in] as stored for dX = dY W (weight-stationary path)."""
    return (_gemm_precision == "bf16x3" and w.shape[0] in (128, 256, 384) and w.shape[1] % 128 == 0
            and w.stride(1) == 1 and w.stride(0) % 4 == 0)


def gemm_x3_tn(a, w, epi=EPI_BIAS, aux=None, p_drop=0.0, seed=0, tag=None):
    """epi(a [M, K] @ w [K, N]) on rsx_gemm_x3_tn: the input gradient dY W of a token linear with W
    as stored ([out, in], K = out in {128, 256, 384}, N = in % 128 == 0), no transposed copy;
    EPI_DGELU_DROP as gemm_x3."""
    a = _c(a)
    M, K = a.shape
    n = w.shape[1]
    out = torch.empty(M, n, device=a.device, dtype=torch.float32)
    if M == 0:
        return out
    with timed(tag or "gemm_x3"):
        rc = N.lib().rsx_gemm_x3_tn(N.ptr(a), a.stride(0), N.ptr(w), w.stride(0), None, M, n, K, epi, N.ptr(aux),
                                    0 if aux is None else aux.stride(0), float(p_drop), int(seed), N.ptr(out),
                                    out.stride(0), N.stream())
    N.check(rc, "gemm_x3_tn")
    return out


def _dx(dy, w, tag="tok_linear_dx"):
    """dX = dY W of a token linear (rsx_gemm_x3_tn when the shape allows, else a transposed copy)."""
    if _tn_ok(w):
        return gemm_x3_tn(dy, w, tag=tag)
    return gemm_x3(dy, w.t(), tag=tag)


def linear_wgrad(dy, x, weight_shape, need_bias, tag="linear_wgrad", precision=None):
    """(dW, db) of y = x W^T + b over the token axis: split-K over tokens, deterministic.
    precision: "fp32" | "bf16x3" (default: the module's GEMM precision)."""
    N.ensure_device(dy)
    dy = _c(dy)
    x = _c(x)
    t, n = dy.shape
    k = x.shape[1]
    assert (n, k) == tuple(weight_shape)
    nws = N.lib().rsx_linear_wgrad_workspace_floats(t, n, k)
    ws = torch.empty(nws, device=dy.device, dtype=torch.float32)
    dw = torch.empty(n, k, device=dy.device, dtype=torch.float32)
    db = torch.empty(n, device=dy.device, dtype=torch.float32) if need_bias else None
    fn = N.lib().rsx_linear_wgrad_x3 if (precision or _gemm_precision) == "bf16x3" else N.lib().rsx_linear_wgrad
    with timed(tag):
        rc = fn(N.ptr(dy), dy.stride(0), N.ptr(x), x.stride(0), t, n, k, N.ptr(dw), dw.stride(0), N.ptr(db), 0,
                N.ptr(ws), nws, N.stream())
    N.check(rc, "linear_wgrad")
    return dw, db


class _TokLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if _x3_ok(weight.shape[0], weight.shape[1]):
            return gemm_x3(x, weight, bias, tag="tok_linear_fwd")
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            if _x3_ok(weight.shape[1], weight.shape[0]):
                dx = _dx(dy, weight)
            else:
                dx = dy @ weight
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_wgrad(dy, x, weight.shape, ctx.has_bias and ctx.needs_input_grad[2])
        return dx, dw, db


class _LinearAddLayerNorm(torch.autograd.Function):
    """(s, LayerNorm(s)), s = x + dropout(a W^T + b): rsx_gemm_x3_addln (the add and the
    LayerNorm in the GEMM's epilogue; the projection itself is never written). Backward: the
    add + LayerNorm backward (rsx_ln_bwd, whose dres is the projection's gradient), then dA on
    rsx_gemm_x3 and dW / db on the split-K weight-gradient kernel, as _TokLinear."""

    @staticmethod
    def forward(ctx, x, a, weight, bias, w, b, eps, p_drop, seed):
        T, D = x.shape
        s = torch.empty_like(x)
        y = torch.empty_like(x)
        mean = torch.empty(T, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        with timed("tok_linear_addln"):
            rc = N.lib().rsx_gemm_x3_addln(N.ptr(a), a.stride(0), N.ptr(weight), weight.stride(0), N.ptr(bias), T, D,
                                           a.shape[1], N.ptr(x), x.stride(0), p_drop, seed, N.ptr(w), N.ptr(b), eps,
                                           N.ptr(s), s.stride(0), N.ptr(y), y.stride(0), N.ptr(mean), N.ptr(rstd),
                                           N.stream())
        N.check(rc, "gemm_x3_addln")
        ctx.save_for_backward(a, weight, s, mean, rstd, w, b)
        ctx.cfg = (p_drop, seed, bias is not None)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        a, weight, s, mean, rstd, w, b = ctx.saved_tensors
        p_drop, seed, has_bias = ctx.cfg
        need = ctx.needs_input_grad
        if dy is None:
            dy = torch.zeros_like(s)
        dx, dres, dw, db = _ln_bwd(s, mean, rstd, w, b, 0, dy, ds, p_drop, seed, need[0], True, need[4], need[5])
        da = _dx(dres, weight) if need[1] else None
        dwt = dbt = None
        if need[2] or (has_bias and need[3]):
            dwt, dbt = linear_wgrad(dres, a, weight.shape, has_bias and need[3])
        return dx, da, dwt, dbt, dw, db, None, None, None


def linear_add_layer_norm(x, a, weight, bias, ln_weight, ln_bias, eps=1e-5, p_drop=0.0):
    """(s, LayerNorm(s)) with s = x + dropout(linear(a, weight, bias)): a norm_first encoder
    layer's attention out-projection, residual add and the LayerNorm after it in one kernel
    (bf16x3 mode, D = 128, K 128 or 256); otherwise linear_tok + add_layer_norm."""
    shp = x.shape
    D = shp[-1]
    if not (_x3_ok(weight.shape[0], weight.shape[1]) and D == 128 and weight.shape[0] == 128
            and weight.shape[1] in (128, 256) and x.numel() > 0):
        return add_layer_norm(x, linear_tok(a, weight, bias), ln_weight, ln_bias, eps, p_drop)
    N.ensure_device(x)
    seed = next_seed() if p_drop > 0 else 0
    s, y = _LinearAddLayerNorm.apply(_c(x.reshape(-1, D)), _c(a.reshape(-1, a.shape[-1])), _c(weight), bias,
                                     ln_weight, ln_bias, float(eps), float(p_drop), seed)
    return s.reshape(shp), y.reshape(shp)


def linear_tok(x, weight, bias=None):
    """F.linear over a token axis (x [..., K]) whose weight/bias gradients come from the
    split-K rsx_linear_wgrad kernel instead of the library GEMM (T >> N, K); forward and
    input gradient on rsx_gemm_x3 when the shapes allow (bf16x3 mode). GPU tensors only."""
    N.ensure_device(x)
    shp = x.shape
    x2 = _c(x.reshape(-1, shp[-1]))
    if x2.shape[0] == 0 or shp[-1] % 16 or weight.shape[0] % 16:
        return torch.nn.functional.linear(x, weight, bias)
    y = _TokLinear.apply(x2, weight, bias)
    return y.reshape(*shp[:-1], weight.shape[0])


class _ProfileLinear(torch.autograd.Function):
    """h[t] = x[t] W[:, :D]^T + (profile W[:, D:]^T + b)[user(t)]: nn.Linear(2D -> N) applied
    to cat(x_tok, profile[user]) without materialising the concatenation or the broadcast
    (v1_refine_usertower.py:498-505, output_proj[0] on the packed tokens). Forward: the small
    per-user GEMM, then the token GEMM with the per-user rows added in its epilogue
    (rsx_gemm_x3_rowadd). Backward: dX on rsx_gemm_x3; the per-user gradient is a segmented
    sum over each user's contiguous tokens (rsx_segment_sum_rows, no atomics); both weight
    halves and the bias from the split-K weight-gradient kernel, written into one [N, 2D]
    gradient (no slice / concatenation kernels)."""

    @staticmethod
    def forward(ctx, x, profile, weight, bias, tok_user, seg):
        D = x.shape[1]
        n = weight.shape[0]
        wp = weight[:, D:]
        prof = gemm_x3(profile, wp, bias, tag="tok_linear_fwd") if _x3_ok(n, D) else \
            torch.addmm(bias, profile, wp.t())
        h = torch.empty(x.shape[0], n, device=x.device, dtype=torch.float32)
        with timed("tok_linear_fwd"):
            rc = N.lib().rsx_gemm_x3_rowadd(N.ptr(x), x.stride(0), N.ptr(weight), weight.stride(0), None,
                                            x.shape[0], n, D, N.ptr(prof), prof.stride(0), N.ptr(tok_user),
                                            N.ptr(h), h.stride(0), N.stream())
        N.check(rc, "gemm_x3_rowadd")
        ctx.save_for_backward(x, profile, weight, seg)
        return h

    @staticmethod
    def backward(ctx, dh):
        x, profile, weight, seg = ctx.saved_tensors
        dh = _c(dh)
        D = x.shape[1]
        n = weight.shape[0]
        U = profile.shape[0]
        dprof = torch.empty(U, n, device=dh.device, dtype=torch.float32)
        rc = N.lib().rsx_segment_sum_rows(N.ptr(dh), dh.stride(0), None, N.ptr(seg), None, U, n, None, -1,
                                          N.ptr(dprof), dprof.stride(0), 0, N.stream())
        N.check(rc, "segment_sum_rows(profile)")
        dx = dprofile = None
        if ctx.needs_input_grad[0]:
            dx = _dx(dh, weight[:, :D])
        if ctx.needs_input_grad[1]:
            dprofile = _dx(dprof, weight[:, D:]) if _x3_ok(D, n) else \
                dprof @ weight[:, D:]
        dw = torch.empty_like(weight)
        db = torch.empty(n, device=dh.device, dtype=torch.float32)
        _wgrad_into(dh, x, dw[:, :D], None)
        _wgrad_into(dprof, profile, dw[:, D:], db)
        return dx, dprofile, dw, db, None, None


def _wgrad_into(dy, x, dw_view, db):
    """dW (+ db) of y = x W^T + b written into a (row-strided) view: rsx_linear_wgrad(_x3)."""
    t, n = dy.shape
    k = x.shape[1]
    nws = N.lib().rsx_linear_wgrad_workspace_floats(t, n, k)
    ws = torch.empty(nws, device=dy.device, dtype=torch.float32)
    fn = N.lib().rsx_linear_wgrad_x3 if _gemm_precision == "bf16x3" else N.lib().rsx_linear_wgrad
    with timed("linear_wgrad"):
        rc = fn(N.ptr(dy), dy.stride(0), N.ptr(_c(x)), x.stride(0), t, n, k, N.ptr(dw_view), dw_view.stride(0),
                N.ptr(db), 0, N.ptr(ws), nws, N.stream())
    N.check(rc, "linear_wgrad")


def profile_linear(x, profile, weight, bias, tok_user, seg):
    """x [T, D] packed tokens, profile [U, D] per user, weight [N, 2D], bias [N], tok_user [T]
    int64 (user of each token, non-decreasing), seg [U + 1] int64 token offsets of the users.
    Returns [T, N] = F.linear(cat(x, profile[tok_user]), weight, bias)."""
    N.ensure_device(x)
    D = x.shape[1]
    n = weight.shape[0]
    if (x.shape[0] == 0 or weight.shape[1] != 2 * D or D not in (128, 256) or n % 128 or weight.stride(1) != 1
            or weight.stride(0) % 4 or _gemm_precision != "bf16x3"):
        return linear_tok(x, weight[:, :D]) + torch.nn.functional.linear(profile, weight[:, D:], bias)[tok_user]
    return _ProfileLinear.apply(_c(x), _c(profile), weight, bias, _c(tok_user), _c(seg))


def gemm_x3_relu_train(a, b, bias, aux, p_drop=0.0, seed=0, tag=None):
    """dropout_p(relu(a [M, K] @ b [N, K]^T + bias)) on rsx_gemm_x3_relu_train; writes the 0/1 mask
    z > 0 into aux [M, N], the multiplier EPI_DGELU_DROP takes in the backward (same p_drop, seed)."""
    a = _c(a)
    b = _c(b)
    M, K = a.shape
    n = b.shape[0]
    if tuple(aux.shape) != (M, n) or aux.dtype != torch.float32 or aux.stride(1) != 1:
        raise ValueError(f"gemm_x3_relu_train: aux must be a float32 [{M}, {n}] tensor with unit column stride")
    out = torch.empty(M, n, device=a.device, dtype=torch.float32)
    if M == 0:
        return out
    nws = N.lib().rsx_gemm_x3_split_floats(M, n, K)
    ws = torch.empty(nws, device=a.device, dtype=torch.float32) if nws > 0 else None
    with timed(tag or "gemm_x3"):
        rc = N.lib().rsx_gemm_x3_relu_train(N.ptr(a), a.stride(0), N.ptr(b), b.stride(0),
                                            N.ptr(None if bias is None else _c(bias)), M, n, K, N.ptr(aux),
                                            aux.stride(0), float(p_drop), int(seed), N.ptr(out), out.stride(0),
                                            N.ptr(ws), nws, N.stream())
    N.check(rc, "gemm_x3_relu_train")
    return out


class _FFN(torch.autograd.Function):
    """linear2(dropout(act(linear1(h)))) with the activation and the dropout in the GEMM epilogues:
    act "gelu": rsx_gemm_x3 EPI_GELU_DROP forward (aux = gelu'(pre)); act "relu":
    rsx_gemm_x3_relu_train (aux = pre > 0). EPI_DGELU_DROP is the backward through either."""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, p_drop, seed, act_name="gelu"):
        h = _c(h)
        ggrad = torch.empty(h.shape[0], w1.shape[0], device=h.device, dtype=torch.float32)  # act'(pre)
        if act_name == "relu":
            act = gemm_x3_relu_train(h, w1, b1, ggrad, p_drop, seed, tag="ffn_relu_fwd1")
        else:
            act = gemm_x3(h, w1, b1, EPI_GELU_DROP, ggrad, p_drop, seed, tag="ffn_fwd1")
        f = gemm_x3(act, w2, b2, tag="ffn_fwd2")
        ctx.save_for_backward(h, w1, w2, ggrad, act)
        ctx.cfg = (p_drop, seed, b1 is not None, b2 is not None)
        return f

    @staticmethod
    def backward(ctx, df):
        h, w1, w2, ggrad, act = ctx.saved_tensors
        p_drop, seed, has_b1, has_b2 = ctx.cfg
        df = _c(df)
        need = ctx.needs_input_grad
        if _tn_ok(w2):
            dpre = gemm_x3_tn(df, w2, EPI_DGELU_DROP, ggrad, p_drop, seed, tag="ffn_dpre")
        else:
            dpre = gemm_x3(df, w2.t(), None, EPI_DGELU_DROP, ggrad, p_drop, seed, tag="ffn_dpre")
        dw2 = db2 = dw1 = db1 = None
        if need[3] or need[4]:
            dw2, db2 = linear_wgrad(df, act, w2.shape, has_b2 and need[4])
        if need[1] or need[2]:
            dw1, db1 = linear_wgrad(dpre, h, w1.shape, has_b1 and need[2])
        dh = _dx(dpre, w1, tag="ffn_dh") if need[0] else None
        return dh, dw1, db1, dw2, db2, None, None, None


def ffn(h, w1, b1, w2, b2, p_drop=0.0, training=True, act="gelu"):
    """linear2(dropout(act(linear1(h)))) over a token axis (nn.TransformerEncoderLayer's
    feed-forward block). act="gelu": bf16x3 mode with GEMM-shaped widths: two fused GEMM launches
    forward, three plus two weight gradients backward; otherwise the unfused ops. act="relu" (the
    layer's default activation): the same fused pair on rsx_gemm_x3_relu_train, with or without gradients;
    with gradients off and no dropout rsx_gemm_x3's EPI_RELU, which saves nothing; shapes outside the
    GEMMs take the unfused PyTorch form."""
    if act not in ("gelu", "relu"):
        raise ValueError(f"ffn: act must be 'gelu' or 'relu', got {act!r}")
    p = float(p_drop) if training else 0.0
    shp = h.shape
    h2 = h.reshape(-1, shp[-1])
    shaped = (h2.is_cuda and h2.shape[0] > 0 and _x3_ok(w1.shape[0], w1.shape[1]) and _x3_ok(w2.shape[0], w2.shape[1])
              and _x3_ok(w2.shape[1], w2.shape[0]) and _x3_ok(w1.shape[1], w1.shape[0]))
    if act == "relu":
        if shaped and p == 0.0 and not torch.is_grad_enabled():
            a = gemm_x3(h2, w1, b1, EPI_RELU, tag="ffn_relu_fwd1")
            return gemm_x3(a, w2, b2, tag="ffn_fwd2").reshape(*shp[:-1], w2.shape[0])
        if shaped:
            seed = next_seed() if p > 0 else 0
            return _FFN.apply(h2, w1, b1, w2, b2, p, seed, "relu").reshape(*shp[:-1], w2.shape[0])
        F = torch.nn.functional
        return F.linear(F.dropout(F.relu(F.linear(h, w1, b1)), p, training), w2, b2)
    if shaped:
        seed = next_seed() if p > 0 else 0
        f = _FFN.apply(h2, w1, b1, w2, b2, p, seed, "gelu")
        return f.reshape(*shp[:-1], w2.shape[0])
    return linear_tok(torch.nn.functional.dropout(torch.nn.functional.gelu(linear_tok(h, w1, b1)), p, training),
                      w2, b2)


# ----------------------------------------------------------------------------------------
# A2 + A3 + A4: the user tower's packed-token training program as one native call per direction
# (rsx_tower_fwd / rsx_tower_bwd, csrc/tower.hip). RSX_TOWER_NATIVE=0 keeps the per-op path.
_TOWER_NATIVE = os.environ.get("RSX_TOWER_NATIVE", "1") != "0"


def tower_params(model):
    """SASRecUserTower parameters in rsx_tower_* order (include/recsys_amd.h RSX_TW_ITEM_PROJ ..)."""
    ps = [model.item_proj.weight, model.item_proj.bias, model.item_id_emb.weight, model.time_emb.weight,
          model.type_emb.weight, model.color_emb.weight, model.graphic_emb.weight, model.section_emb.weight,
          model.pos_emb.weight, model.emb_ln.weight, model.emb_ln.bias]
    for layer in model.transformer_encoder.layers:
        sa = layer.self_attn
        ps += [layer.norm1.weight, layer.norm1.bias, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight,
               sa.out_proj.bias, layer.norm2.weight, layer.norm2.bias, layer.linear1.weight, layer.linear1.bias,
               layer.linear2.weight, layer.linear2.bias]
    op = model.output_proj
    ps += [op[0].weight, op[0].bias, op[1].weight, op[1].bias, op[3].weight, op[3].bias]
    return ps


def tower_native_ok(model, packed, pv):
    """Whether rsx_tower_* runs exactly what forward_packed's per-op path runs: bf16x3 token linears
    and attention, d_model 128 with 4 heads and a 256-wide feed-forward, every parameter trained,
    fp32 contiguous rows, the item-id gradient plan present. Returns the parameter list in
    rsx_tower_* order (truthy; tower_packed takes it) or None."""
    if not (_TOWER_NATIVE and _gemm_precision == "bf16x3" and _mha_precision == "bf16x3" and _ADDLN_ON):
        return None
    if getattr(packed, "item_seg", None) is None or not pv.is_cuda:
        return None
    layers = model.transformer_encoder.layers
    if model.d_model != 128 or not (1 <= len(layers) <= 8) or model.pos_emb.weight.shape[0] > 64:
        return None
    for layer in layers:
        if (layer.self_attn.num_heads != 4 or layer.linear1.out_features != 256 or not layer.norm_first
                or layer.activation_relu_or_gelu != 2):
            return None
    ps = tower_params(model)
    ok = all(p.requires_grad and p.dtype == torch.float32 and p.is_contiguous() for p in ps)
    return ps if ok else None


_ADDLN_ON = os.environ.get("RSX_LINEAR_ADDLN", "1") != "0"


class _TowerPacked(torch.autograd.Function):
    """out = normalize(output_proj(...encoder(seq_embed(item_proj(pv)))...)) over packed tokens; see
    rsx_tower_fwd. Inputs with gradients: pv (optional), gate, profile and the tower parameters."""

    @staticmethod
    def forward(ctx, pv, gate, profile, cfg, *params):
        packed, tok_ids, p_drop, eps, nl, tail_last, tok_uidx = cfg
        T, D = tok_ids[0].numel(), pv.shape[1]
        U = packed.seg_off.numel() - 1
        dev = pv.device
        pv = _c(pv)
        gate = _c(gate)
        profile = _c(profile)
        perm, cb, chunk_ids, ch_off, uniq = packed.item_seg
        # tok_uidx: pv holds one row per distinct item (uniq's order), token t reads row tok_uidx[t]
        assert pv.shape[0] == (T if tok_uidx is None else uniq.numel())
        inputs = ([pv] + list(tok_ids) + [packed.tok_pos, packed.tok_pad, packed.seg_off, packed.seg_off64,
                                            packed.tok_user, gate, profile, perm, cb, chunk_ids, ch_off, uniq,
                                            tok_uidx])
        tail_last = None if tail_last is None else _c(tail_last)
        ptrs = N.ptr_array(inputs + list(params) + [tail_last])
        tabs = params[2:8]
        tB = 0 if tail_last is None else tail_last.numel()
        R = T // 2 + tB if tB else T
        dims = N.i64_array([T, U, params[8].shape[0], nl, chunk_ids.numel(), uniq.numel()]
                           + [t.shape[0] for t in tabs] + [tB, T // 2])
        fargs = (ctypes.c_float * (len(eps) + 1))(p_drop, *eps)
        seeds = [next_seed() if p_drop > 0 else 0 for _ in range(1 + 4 * nl)]
        seeds_arr = (ctypes.c_uint64 * len(seeds))(*seeds)
        nbytes = N.lib().rsx_tower_arena_bytes(T, U, nl, pv.shape[0])
        arena = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        out = torch.empty(R, D, device=dev, dtype=torch.float32)
        with timed("tower_fwd"):
            rc = N.lib().rsx_tower_fwd(ptrs, dims, fargs, seeds_arr, N.ptr(arena), nbytes, N.ptr(out), N.stream())
        N.check(rc, "tower_fwd")
        ctx.save_for_backward(pv, gate, profile, out, *params)
        ctx.keep = (inputs + [tail_last], arena, ptrs, dims, fargs, seeds_arr)
        ctx.shape = (T, U, params[8].shape[0], nl, chunk_ids.numel())
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.keep is None:  # the arena (the forward's activations) is released by the first backward
            raise RuntimeError("tower_packed: a second backward through the same forward (retain_graph=True) "
                               "is not supported; run the forward again")
        pv, gate, profile, out, *params = ctx.saved_tensors
        inputs, arena, ptrs, dims, fargs, seeds_arr = ctx.keep
        T, U, L, nl, C = ctx.shape
        dev = dout.device
        dout = _c(dout)
        # accumulated: the six tables, pos_emb, emb_ln w / b, the gate (one zero-filled allocation);
        # written: every other parameter's gradient and the profile's
        acc_like = [gate] + [params[i] for i in range(2, 11)]
        dgate, *acc = _zeros_group(acc_like)
        written = _empty_group([params[0], params[1]] + list(params[11:]) + [profile])
        dprofile = written[-1]
        dparams = [written[0], written[1]] + acc + written[2:-1]
        dpv = torch.empty_like(pv) if ctx.needs_input_grad[0] else None
        grads = [dpv] + [None] * 11 + [dgate, dprofile] + [None] * 6 + dparams + [None]
        nws = N.lib().rsx_tower_bwd_workspace_bytes(T, U, L, nl, C)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        with timed("tower_bwd"):
            rc = N.lib().rsx_tower_bwd(ptrs, dims, fargs, seeds_arr, N.ptr(arena), N.ptr(out), N.ptr(dout),
                                       N.ptr_array(grads), N.ptr(ws), nws, N.stream())
        N.check(rc, "tower_bwd")
        ctx.keep = None
        return (dpv, dgate, dprofile, None) + tuple(dparams)


def _empty_group(likes):
    """Uninitialised fp32 buffers shaped like each tensor (None -> None), carved out of ONE
    allocation (16-B aligned slices)."""
    sizes = [0 if t is None else (t.numel() + 3) // 4 * 4 for t in likes]
    if sum(sizes) == 0:
        return [None] * len(likes)
    ref = next(t for t in likes if t is not None)
    flat = torch.empty(sum(sizes), device=ref.device, dtype=torch.float32)
    out, o = [], 0
    for t, n in zip(likes, sizes):
        out.append(None if t is None else flat[o:o + t.numel()].view(t.shape))
        o += n
    return out


def tower_packed(model, packed, pv_tok, tok_ids, s_g, profile, p_drop, params=None, tail_last=None):
    """The native form of SASRecUserTower.forward_packed after the static profile: [T, 128], or with
    tail_last (view 1's "last" token per user, [B]) the [T/2 + B, 128] tail rows (see
    rsx_tower_fwd). params: tower_native_ok's list (else rebuilt). pv_tok: the [T, 128] rows, or
    ItemRows: item_proj and its weight gradient then run once per distinct item."""
    layers = model.transformer_encoder.layers
    eps = [model.emb_ln.eps]
    for layer in layers:
        eps += [layer.norm1.eps, layer.norm2.eps]
    eps.append(model.output_proj[1].eps)
    tok_uidx = None
    if isinstance(pv_tok, ItemRows):
        pv_tok, tok_uidx = pv_tok.rows, _c(pv_tok.idx)
    cfg = (packed, [_c(t) for t in tok_ids], float(p_drop), [float(e) for e in eps], len(layers), tail_last, tok_uidx)
    return _TowerPacked.apply(pv_tok, s_g, profile, cfg, *(params if params is not None else tower_params(model)))


# ----------------------------------------------------------------------------------------
# A9: item-tower RE fields over packed (valid) tokens
@torch.no_grad()
def bert_embed_packed(embeddings, ids, tok_pos):
    """BertEmbeddings(input_ids) rows for a packed token list (ids [T], positions tok_pos [T],
    token type 0) via rsx_embed3_ln; dropout as the module's (active only in training)."""
    word = embeddings.word_embeddings.weight
    ids = _index("bert_embed_packed", "ids", ids, word)
    tok_pos = _index("bert_embed_packed", "tok_pos", tok_pos, word, ids.numel())
    N.ensure_device(ids)
    D = word.shape[1]
    T = ids.numel()
    out = torch.empty(T, D, device=ids.device, dtype=torch.float32)
    ln = embeddings.LayerNorm
    rc = N.lib().rsx_embed3_ln(N.ptr(word), word.stride(0), N.ptr(_c(embeddings.position_embeddings.weight)),
                               N.ptr(_c(embeddings.token_type_embeddings.weight[0])), N.ptr(ln.weight),
                               N.ptr(ln.bias), float(ln.eps), N.ptr(_c(ids)), N.ptr(_c(tok_pos)), T, D, N.ptr(out),
                               N.stream())
    N.check(rc, "embed3_ln")
    if embeddings.training and embeddings.dropout.p > 0:
        out = torch.nn.functional.dropout(out, embeddings.dropout.p, True)
    return out


class _SegmentMean(torch.autograd.Function):
    """vec[u] = sum_{t in [seg[u], seg[u+1])} x[t] / max(cnt[u], 1e-9): the masked mean of the
    reference's (feats * m).sum(1) / clamp(m.sum(1), 1e-9) over packed valid tokens."""

    @staticmethod
    def forward(ctx, x, seg, tok_seg, inv):
        U = inv.numel()
        D = x.shape[1]
        s = torch.empty(U, D, device=x.device, dtype=torch.float32)
        rc = N.lib().rsx_segment_sum_rows(N.ptr(x), x.stride(0), None, N.ptr(seg), None, U, D, None, -1, N.ptr(s),
                                          s.stride(0), 0, N.stream())
        N.check(rc, "segment_sum_rows(mean)")
        ctx.save_for_backward(tok_seg, inv)
        return s * inv.unsqueeze(1)

    @staticmethod
    def backward(ctx, dv):
        tok_seg, inv = ctx.saved_tensors
        return gather_rows(_c(dv * inv.unsqueeze(1)), tok_seg), None, None, None


def segment_mean(x, seg, tok_seg, counts):
    """x [T, D] packed rows (segments contiguous), seg [U+1] int64 offsets, tok_seg [T] int64,
    counts [U] float -> [U, D] means (a zero-count segment gives 0, as the clamp does)."""
    _rows2("segment_mean", "x", x)
    if counts.device != x.device:
        raise RuntimeError(f"segment_mean: counts is on {counts.device}, expected {x.device}")
    seg = _index("segment_mean", "seg", seg, x, counts.numel() + 1)
    tok_seg = _index("segment_mean", "tok_seg", tok_seg, x, x.shape[0])
    N.ensure_device(x)
    inv = 1.0 / torch.clamp(counts, min=1e-9)
    return _SegmentMean.apply(_c(x), _c(seg), _c(tok_seg), inv.float())


# ----------------------------------------------------------------------------------------
# DCN-V2 reranker: cross network + the cross half of the final head
def crossnet(x, kernels, biases, w_head=None, want_x=False):
    """rsx_crossnet: x [B, D] -> (x_L [B, D] or None, head_part [B] = x_L . w_head or None)."""
    D = _rows2("crossnet", "x", x)
    if len(kernels) != len(biases):
        raise ValueError(f"crossnet: {len(kernels)} kernels but {len(biases)} biases")
    for l, (k, b) in enumerate(zip(kernels, biases)):
        _f32_vec("crossnet", f"kernels[{l}]", k, D, x)
        _f32_vec("crossnet", f"biases[{l}]", b, D, x)
    _f32_vec("crossnet", "w_head", w_head, D, x)
    N.ensure_device(x)
    x = _c(x)
    B, D = x.shape
    x_out = torch.empty(B, D, device=x.device, dtype=torch.float32) if want_x else None
    part = torch.empty(B, device=x.device, dtype=torch.float32) if w_head is not None else None
    rc = N.lib().rsx_crossnet(N.ptr(x), x.stride(0), B, D, len(kernels),
                              N.ptr_array([_c(k.reshape(-1)) for k in kernels]),
                              N.ptr_array([_c(b.reshape(-1)) for b in biases]),
                              N.ptr(None if w_head is None else _c(w_head.reshape(-1))), N.ptr(x_out), N.ptr(part),
                              N.stream())
    N.check(rc, "crossnet")
    return x_out, part


def _cross_params(fn, x, kernels, biases, w_head):
    """Shared checks of crossnet_bwd / dcn_train_step: x fp32 [B, >= D], L kernels / biases of D
    elements, w_head (None allowed) of D elements, all on x's device. Returns D = the kernels' length
    (x's width when there is no layer)."""
    width = _rows2(fn, "x", x)
    if len(kernels) != len(biases):
        raise ValueError(f"{fn}: {len(kernels)} kernels but {len(biases)} biases")
    D = kernels[0].numel() if len(kernels) else width
    for l, (k, b) in enumerate(zip(kernels, biases)):
        _f32_vec(fn, f"kernels[{l}]", k, D, x)
        _f32_vec(fn, f"biases[{l}]", b, D, x)
    _f32_vec(fn, "w_head", w_head, D, x)
    return D


def _row_view(x):
    """x [B, W] as the kernels read rows: unit column stride, row stride a multiple of 4."""
    return x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= x.shape[1] else x.contiguous()


def crossnet_bwd(x, kernels, biases, w_head=None, dhead=None, dx_out=None, want_dx=False, dw_head_out=None,
                 max_blocks=0):
    """rsx_crossnet_bwd: the gradients of ops.crossnet's sweep over x [B, D] (a [B, D] view of a
    wider buffer is read in place) for the upstream dhead [B] (gradient of head_part; needs w_head)
    and / or dx_out [B, D] (gradient of x_L); both mean their sum. Returns (dk: L tensors shaped as
    the kernels, db: L tensors [D], dw_head [D] or None, dx [B, D] or None (want_dx)). dw_head_out:
    a contiguous [D] buffer to receive dw_head (a slice of final_head.weight's gradient).
    max_blocks: a smaller grid cap than the kernel's 1024 workgroups (tests). Deterministic."""
    fn = "crossnet_bwd"
    D = _cross_params(fn, x, kernels, biases, w_head)
    if x.shape[1] != D:
        raise ValueError(f"{fn}: x has {x.shape[1]} columns, the layers {D}")
    B = x.shape[0]
    if (w_head is None) != (dhead is None):
        raise ValueError(f"{fn}: w_head and dhead go together")
    if dhead is None and dx_out is None:
        raise ValueError(f"{fn}: no upstream gradient (give w_head and dhead, and / or dx_out)")
    _f32_vec(fn, "dhead", dhead, B, x)
    if dx_out is not None:
        _f32(fn, "dx_out", dx_out, x)
        if tuple(dx_out.shape) != (B, D):
            raise ValueError(f"{fn}: dx_out has shape {tuple(dx_out.shape)}, expected {(B, D)}")
    if dw_head_out is not None:
        _f32_vec(fn, "dw_head_out", dw_head_out, D, x)
        if w_head is None or not dw_head_out.is_contiguous():
            raise ValueError(f"{fn}: dw_head_out must be contiguous and needs w_head")
    N.ensure_device(x)
    x = _row_view(x)
    L, dev, lib = len(kernels), x.device, N.lib()
    ks = [_c(k.reshape(-1)) for k in kernels]
    bs = [_c(b.reshape(-1)) for b in biases]
    # rows: dk_0.., db_0.., dw_head (an empty batch launches nothing: its sums are zero)
    flat = (torch.empty if B else torch.zeros)(2 * L + 1, D, device=dev, dtype=torch.float32)
    if B == 0 and dw_head_out is not None:
        dw_head_out.zero_()
    dk, db = [flat[l] for l in range(L)], [flat[L + l] for l in range(L)]
    dwh = None if w_head is None else (dw_head_out if dw_head_out is not None else flat[2 * L])
    dx = torch.empty(B, D, device=dev, dtype=torch.float32) if want_dx else None
    nws = lib.rsx_crossnet_bwd_workspace_bytes(B, D, L, int(max_blocks))
    ws = torch.empty(max(nws, 0), device=dev, dtype=torch.uint8)
    with timed("crossnet_bwd"):
        rc = lib.rsx_crossnet_bwd(N.ptr(x), x.stride(0), B, D, L, N.ptr_array(ks), N.ptr_array(bs),
                                  N.ptr(None if w_head is None else _c(w_head.reshape(-1))),
                                  N.ptr(None if dhead is None else _c(dhead.reshape(-1))), N.ptr(_c(dx_out)),
                                  N.ptr_array(dk), N.ptr_array(db), N.ptr(dwh), N.ptr(dx), N.ptr(ws), max(nws, 0),
                                  int(max_blocks), N.stream())
    N.check(rc, "crossnet_bwd")
    return [g.view(k.shape) for g, k in zip(dk, kernels)], db, dwh, dx


# ----------------------------------------------------------------------------------------
# DCN-V2 reranker training: one step of the RankingModel (csrc/dcn.hip, csrc/dcn_train.hip)
def dcn_train_supported(D, hidden):
    """None when the training kernels cover the shape, else the text naming the limit."""
    if tuple(hidden) != (256, 128):
        return f"RankingModel training needs the deep net's widths (256, 128) (got {tuple(hidden)})"
    if D % 4 or not 4 <= D <= 512:
        return f"RankingModel training needs an input width that is a multiple of 4 in [4, 512] (got {D})"
    return None


class DCNStep:
    """What dcn_train_step returns: loss (0-d float64 device tensor), logit [B], grads (in the order
    of its parameters: the L kernels, the L biases, W1, b1, LN1 weight / bias, W2, b2, LN2 weight /
    bias, final_head.weight [1, D + 128], final_head.bias [1]) and, with return_acts, h1 (after the
    dropout) and x_L."""

    def __init__(self, loss, logit, grads, h1=None, x_L=None):
        self.loss, self.logit, self.grads, self.h1, self.x_L = loss, logit, grads, h1, x_L


def dcn_train_step(x, y, kernels, biases, w1, b1, ln1_w, ln1_b, w2, b2, ln2_w, ln2_b, w_head, head_bias,
                   eps1=1e-5, eps2=1e-5, p_drop=0.0, seed=0, reduction="mean", return_acts=False):
    """Forward, Logloss and backward of the DCN-V2 RankingModel over raw tensors, no host
    synchronisation: x [B, D] fp32 (or the list of its column blocks: user, item[, context]), y [B];
    cross network (kernels / biases, L of [D(, 1)]) and deep net Linear(D, 256) + LayerNorm + GELU +
    dropout(p_drop, seed) + Linear(256, 128) + LayerNorm + GELU, final_head weight w_head [1, D + 128]
    and bias head_bias [1] (read on the device). Binary cross-entropy on the logit, reduction "mean"
    | "sum". The step's input lives in a [B, Dp] buffer, Dp = D rounded up to 16 with zero pad
    columns: row stride Dp for the cross network and the first linear, K = Dp for its weight gradient
    (rsx_linear_wgrad needs K % 16 == 0). Returns a DCNStep; the caller applies the update."""
    fn = "dcn_train_step"
    parts = list(x) if isinstance(x, (list, tuple)) else [x]
    for i, t in enumerate(parts):
        _rows2(fn, f"x[{i}]" if len(parts) > 1 else "x", t)
        if t.shape[0] != parts[0].shape[0]:
            raise ValueError(f"{fn}: x[{i}] has {t.shape[0]} rows, x[0] {parts[0].shape[0]}")
        if t.device != parts[0].device:
            raise RuntimeError(f"{fn}: x[{i}] is on {t.device}, expected {parts[0].device}")
    x0 = parts[0]
    B, D = x0.shape[0], sum(t.shape[1] for t in parts)
    if reduction not in ("mean", "sum"):
        raise ValueError('reduction must be "mean" or "sum"')
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError(f"{fn}: p_drop must be in [0, 1) (got {p_drop})")
    if B < 1:
        raise ValueError(f"{fn} needs at least one row")
    if len(kernels) != len(biases):
        raise ValueError(f"{fn}: {len(kernels)} kernels but {len(biases)} biases")
    for l, (k, b) in enumerate(zip(kernels, biases)):
        _f32_vec(fn, f"kernels[{l}]", k, D, x0)
        _f32_vec(fn, f"biases[{l}]", b, D, x0)
    for name, t, shape in (("w1", w1, (256, D)), ("w2", w2, (128, 256))):
        _f32(fn, name, t, x0)
        if tuple(t.shape) != shape:
            raise ValueError(f"{fn}: {name} has shape {tuple(t.shape)}, expected {shape}")
    for name, t, n in (("b1", b1, 256), ("ln1_w", ln1_w, 256), ("ln1_b", ln1_b, 256), ("b2", b2, 128),
                       ("ln2_w", ln2_w, 128), ("ln2_b", ln2_b, 128), ("w_head", w_head, D + 128),
                       ("head_bias", head_bias, 1)):
        if t is None:
            raise ValueError(f"{fn}: {name} is missing")
        _f32_vec(fn, name, t, n, x0)
    if not torch.is_tensor(y):
        raise TypeError(f"{fn}: y must be a tensor")
    if y.numel() != B:
        raise ValueError(f"{fn}: {y.numel()} labels for {B} rows")
    if y.device != x0.device:
        raise RuntimeError(f"{fn}: y is on {y.device}, expected {x0.device}")
    why = dcn_train_supported(D, (w1.shape[0], w2.shape[0]))
    if why:
        raise NotImplementedError(why)
    N.ensure_device(x0)
    dev, lib, st = x0.device, N.lib(), N.stream()
    L = len(kernels)
    y = _c(y.to(torch.float32).reshape(-1))
    Dp = (D + 15) // 16 * 16
    if len(parts) == 1 and Dp == D:
        xp = _row_view(x0)
    else:
        xp = torch.empty(B, Dp, device=dev, dtype=torch.float32)
        o = 0
        for t in parts:
            xp[:, o:o + t.shape[1]].copy_(t)
            o += t.shape[1]
        if Dp > D:
            xp[:, D:].zero_()
    ldx = xp.stride(0)
    ks, bs = [_c(k.reshape(-1)) for k in kernels], [_c(b.reshape(-1)) for b in biases]
    kp, bp = N.ptr_array(ks), N.ptr_array(bs)
    w1, w2, wh = _c(w1), _c(w2), _c(w_head.reshape(-1))
    f32 = dict(device=dev, dtype=torch.float32)

    def ln_gelu(z, w, b, eps):
        h = torch.empty_like(z)
        mean, rstd = torch.empty(B, **f32), torch.empty(B, **f32)
        N.check(lib.rsx_ln_fwd(N.ptr(z), None, 0.0, 0, N.ptr(w), N.ptr(b), float(eps), ACT_GELU_ERF, B, z.shape[1],
                               None, N.ptr(h), N.ptr(mean), N.ptr(rstd), st), "ln_fwd")
        return h, mean, rstd

    def mask(t):
        """dropout's keep-mask / (1 - p) of (seed, row * 256 + col) applied to t [B, 256]; t itself at p = 0."""
        if p_drop == 0.0:
            return t
        out = torch.empty_like(t)
        N.check(lib.rsx_dropout_bwd(N.ptr(t), B, 256, float(p_drop), int(seed), N.ptr(out), st), "dropout")
        return out

    # forward, keeping the LayerNorm inputs and statistics
    with timed("dcn_train/forward"):
        head_part = torch.empty(B, **f32)
        x_L = torch.empty(B, D, **f32) if return_acts else None
        N.check(lib.rsx_crossnet(N.ptr(xp), ldx, B, D, L, kp, bp, N.ptr(wh), N.ptr(x_L), N.ptr(head_part), st),
                "crossnet")
        z1 = torch.empty(B, 256, **f32)
        N.check(lib.rsx_linear_fwd(N.ptr(xp), ldx, N.ptr(w1), N.ptr(_c(b1)), B, 256, D, ACT_NONE, N.ptr(z1), st),
                "linear_fwd")
        a1, mean1, rstd1 = ln_gelu(z1, ln1_w, ln1_b, eps1)
        h1 = mask(a1)
        z2 = linear(h1, w2, b2)
        h2, mean2, rstd2 = ln_gelu(z2, ln2_w, ln2_b, eps2)
        logit, g, dh2 = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, 128, **f32)
        loss = torch.empty((), device=dev, dtype=torch.float64)
        gwh = torch.empty(1, D + 128, **f32)     # final_head.weight's gradient: [cross | deep] slices
        gbias = torch.empty(1, **f32)
        nws = lib.rsx_dcn_train_head_workspace_bytes(B)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        N.check(lib.rsx_dcn_train_head(N.ptr(h2), 128, N.ptr(wh) + 4 * D, N.ptr(head_part), N.ptr(_c(head_bias)),
                                       N.ptr(y), B, 1 if reduction == "mean" else 0, N.ptr(logit), N.ptr(g),
                                       N.ptr(dh2), N.ptr(ws), nws, N.ptr(loss), N.ptr(gbias), N.ptr(gwh) + 4 * D, st),
                "dcn_train_head")

    # deep half backward: exact fp32 products for the weight gradients, as the DeepFM step
    with timed("dcn_train/deep_bwd"):
        dz2, _, dln2w, dln2b = _ln_bwd(z2, mean2, rstd2, ln2_w, ln2_b, ACT_GELU_ERF, dh2, None, 0.0, 0, True, False,
                                       True, True)
        dw2, db2 = linear_wgrad(dz2, h1, (128, 256), True, tag="dcn_train/dw2", precision="fp32")
        dh1 = mask(gemm_x3_tn(dz2, w2, tag="dcn_train/dh1"))
        dz1, _, dln1w, dln1b = _ln_bwd(z1, mean1, rstd1, ln1_w, ln1_b, ACT_GELU_ERF, dh1, None, 0.0, 0, True, False,
                                       True, True)
        dw1, db1 = linear_wgrad(dz1, xp, (256, Dp), True, tag="dcn_train/dw1", precision="fp32")
        if Dp > D:
            dw1 = dw1[:, :D].contiguous()

    # cross network backward from g (dx is not needed to train the ranker alone)
    dk, dbs, _, _ = crossnet_bwd(xp[:, :D], ks, bs, w_head=wh[:D], dhead=g, dw_head_out=gwh[0, :D])
    grads = ([t.view(k.shape) for t, k in zip(dk, kernels)] + [t.view(b.shape) for t, b in zip(dbs, biases)]
             + [dw1, db1, dln1w, dln1b, dw2, db2, dln2w, dln2b, gwh, gbias])
    return DCNStep(loss, logit, grads, h1 if return_acts else None, x_L)


# ----------------------------------------------------------------------------------------
# A16: DeepFM forward (inference)
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def linear(x, weight, bias=None, act=ACT_NONE):
    """act(x @ weight.T + bias) on the fp32 MFMA (forward only). x [M, K], weight [N<=256, K]."""
    K = _rows2("linear", "x", x)
    _f32("linear", "weight", weight, x)
    if weight.dim() != 2 or weight.shape[1] != K:
        raise ValueError(f"linear: weight has shape {tuple(weight.shape)}, expected [N, {K}]")
    _f32_vec("linear", "bias", bias, weight.shape[0], x)
    N.ensure_device(x)
    x = _c(x)
    M, K = x.shape
    n = weight.shape[0]
    y = torch.empty(M, n, device=x.device, dtype=torch.float32)
    with timed("linear"):
        rc = N.lib().rsx_linear_fwd(N.ptr(x), x.stride(0), N.ptr(_c(weight)), N.ptr(bias), M, n, K, act, N.ptr(y),
                                    N.stream())
    N.check(rc, "linear_fwd")
    return y


# RSX_DEEPFM_FUSED=0 selects the three-kernel path (gather+FM, fp32-MFMA linears) for A/B runs
_DEEPFM_FUSED = os.environ.get("RSX_DEEPFM_FUSED", "1") != "0"
# packed inference tables for the persistent DeepFM kernel (RSX_DEEPFM_PACK=0: read V / W directly)
_DEEPFM_PACK = os.environ.get("RSX_DEEPFM_PACK", "1") != "0"


class _FastKey:
    """Validity key of derived device state over a list of tensors: identities (the tensors are
    held, so an id cannot be recycled), storage pointers and in-place version counters, compared
    as three flat lists (≈ 0.25 µs per tensor; the per-tensor tuple key cost ≈ 0.75 µs)."""
    __slots__ = ("held", "ids", "ptrs", "vers")

    def __init__(self, ts):
        self.held = list(ts)
        self.ids = [id(t) for t in ts]
        self.ptrs = [t.data_ptr() for t in ts]
        self.vers = [t._version for t in ts]

    def matches(self, ts) -> bool:
        return ([id(t) for t in ts] == self.ids and [t._version for t in ts] == self.vers
                and [t.data_ptr() for t in ts] == self.ptrs)


def _deepfm_state(F, dev, emb_tables, lin_tables, dnn_weights, dnn_biases, w_out, cache):
    """Device state of the fused DeepFM kernel: the bf16 DNN weight images, the packed tables (when
    the kernel form takes them) and the pointer arrays, rebuilt when any input tensor changes
    (storage or in-place version). Kept in the caller's cache dict (the DeepFM module) between
    calls; without one it is built per call."""
    ts = list(emb_tables) + list(lin_tables) + list(dnn_weights) + list(dnn_biases) + [w_out]
    if cache is not None:
        st = cache.get("fused_state")
        if st is not None and st["dev"] == dev and st["key"].matches(ts):
            return st
    emb = [_c(t) for t in emb_tables]
    lin = [_c(t) for t in lin_tables]
    w1, w2 = _c(dnn_weights[0]), _c(dnn_weights[1])
    b1, b2 = _c(dnn_biases[0]), _c(dnn_biases[1])
    wo = _c(w_out.reshape(-1))
    ws = torch.empty(N.lib().rsx_deepfm_fused_workspace_bytes(F), device=dev, dtype=torch.uint8)
    N.check(N.lib().rsx_deepfm_fused_prep(F, N.ptr(w1), N.ptr(w2), N.ptr(ws), N.stream()), "deepfm_prep")
    packed = None
    if cache is not None and _DEEPFM_PACK and N.lib().rsx_deepfm_fused_uses_packed(F):
        # inference images of the tables: [vocab][32] per field (V row, W, pad); one 128-B line
        # per (row, field) instead of two
        packed = [torch.empty(v.shape[0], 32, device=dev, dtype=torch.float32) for v in emb]
        for v, w, p in zip(emb, lin, packed):
            N.check(N.lib().rsx_deepfm_pack(N.ptr(v), N.ptr(w), v.shape[0], N.ptr(p), N.stream()), "deepfm_pack")
    st = {"dev": dev, "key": _FastKey(ts), "hold": (emb, lin, w1, w2, b1, b2, wo, packed), "ws": N.ptr(ws),
          "ws_t": ws, "V": N.ptr_array(emb), "W": N.ptr_array(lin),
          "P": N.ptr_array(packed) if packed is not None else None,
          "b1": N.ptr(b1), "b2": N.ptr(b2), "wo": N.ptr(wo)}
    if cache is not None:
        cache["fused_state"] = st
    return st


def deepfm_forward(x, emb_tables, lin_tables, out_bias, dnn_weights, dnn_biases, w_out, cache=None):
    """DeepFM logits/probabilities for x [R, F] int64 (see csrc/deepfm.hip).

    emb_tables: F tensors [vocab_f, 16]; lin_tables: F tensors [vocab_f] (or [vocab_f, 1]);
    dnn_weights/dnn_biases: torch Linear layout, ReLU between layers; w_out [H_last].
    Config-3 shapes (E 16, DNN (256, 128)) run the single fused kernel (rsx_deepfm_fused, bf16x3
    DNN products); other shapes the gather + fp32-MFMA linear kernels. cache: a dict owned by the
    caller (the DeepFM module) that keeps the fused kernel's bf16 weight images between calls,
    rebuilt when either DNN weight changes (storage or in-place version). Returns (logit [R], prob [R])."""
    N.ensure_device(x)
    x = _c(x)
    R, F = x.shape
    E = emb_tables[0].shape[1]
    dev = x.device
    if (_DEEPFM_FUSED and E == 16 and F <= 64 and len(dnn_weights) == 2 and tuple(dnn_weights[0].shape) == (256, F * 16)
            and tuple(dnn_weights[1].shape) == (128, 256)):
        if len(emb_tables) != F or len(lin_tables) != F:
            raise ValueError(f"deepfm: {len(emb_tables)} embedding / {len(lin_tables)} linear tables for {F} fields")
        logit = torch.empty(R, device=dev, dtype=torch.float32)
        prob = torch.empty(R, device=dev, dtype=torch.float32)
        with timed("deepfm/fused"):
            st = _deepfm_state(F, dev, emb_tables, lin_tables, dnn_weights, dnn_biases, w_out, cache)
            rc = N.lib().rsx_deepfm_fused_run(N.ptr(x), R, F, st["V"], st["W"], st["P"], float(out_bias), st["b1"],
                                              st["b2"], st["wo"], st["ws"], N.ptr(logit), N.ptr(prob), N.stream())
        N.check(rc, "deepfm_fused")
        return logit, prob
    emb = torch.empty(R, F * E, device=dev, dtype=torch.float32)
    lin = torch.empty(R, device=dev, dtype=torch.float32)
    with timed("deepfm/embed"):
        rc = N.lib().rsx_deepfm_embed(N.ptr(x), R, F, E, N.ptr_array([_c(t) for t in emb_tables]),
                                      N.ptr_array([_c(t) for t in lin_tables]), float(out_bias), N.ptr(emb),
                                      N.ptr(lin), N.stream())
    N.check(rc, "deepfm_embed")
    h = emb
    for w, b in zip(dnn_weights[:-1], dnn_biases[:-1]):
        with timed("deepfm/linear"):
            y = torch.empty(R, w.shape[0], device=dev, dtype=torch.float32)
            rc = N.lib().rsx_linear_fwd(N.ptr(h), h.stride(0), N.ptr(_c(w)), N.ptr(b), R, w.shape[0], h.shape[1],
                                        ACT_RELU, N.ptr(y), N.stream())
        N.check(rc, "linear_fwd")
        h = y
    logit = torch.empty(R, device=dev, dtype=torch.float32)
    prob = torch.empty(R, device=dev, dtype=torch.float32)
    w, b = dnn_weights[-1], dnn_biases[-1]
    with timed("deepfm/linear_dot"):
        rc = N.lib().rsx_linear_dot_fwd(N.ptr(h), h.stride(0), N.ptr(_c(w)), N.ptr(b), R, w.shape[0], h.shape[1],
                                        ACT_RELU, N.ptr(_c(w_out.reshape(-1))), N.ptr(lin), N.ptr(logit),
                                        N.ptr(prob), N.stream())
    N.check(rc, "linear_dot_fwd")
    return logit, prob


# ----------------------------------------------------------------------------------------
# A16 training: one DeepFM step (csrc/deepfm_train.hip)
_DEEPFM_ID_BITS = 40
_DEEPFM_DROPPED = (1 << _DEEPFM_ID_BITS) - 1


def deepfm_train_supported(F, embed_dim, hidden):
    """None when the training kernels cover the shape, else the text naming the limit."""
    if embed_dim != 16:
        return f"DeepFM training needs embed_dim 16 (got {embed_dim})"
    if tuple(hidden) != (256, 128):
        return f"DeepFM training needs dnn_hidden_units (256, 128) (got {tuple(hidden)})"
    if not 1 <= F <= 64:
        return f"DeepFM training needs 1 <= F <= 64 fields (got {F})"
    return None


class DeepFMStep:
    """What deepfm_train_step returns: loss (0-d float64 device tensor), logit [R], dense (the
    gradients of W1, b1, W2, b2, w_out [128], out.bias [1]) and, with return_grads, sparse_grads()."""

    def __init__(self, loss, logit, dense, sparse):
        self.loss, self.logit, self.dense, self._sparse = loss, logit, dense, sparse

    def sparse_grads(self):
        """Per field (distinct ids [U_f], dV [U_f, 16], dW [U_f], U_f as a device scalar): the summed
        rows the sparse update consumed (one host read: the number of distinct (field, id))."""
        if self._sparse is None:
            raise RuntimeError("deepfm_train_step was called without return_grads=True")
        keys_sorted, seg_start, nseg, oV, oW, F = self._sparse[:6]
        U = int(nseg.item())
        keys = keys_sorted[seg_start[:U].long()]
        fld, ids = keys >> _DEEPFM_ID_BITS, keys & _DEEPFM_DROPPED
        out = []
        for f in range(F):
            sel = (fld == f) & (ids != _DEEPFM_DROPPED)
            out.append((ids[sel], oV[:U][sel], oW[:U][sel], sel.sum()))
        return out

    def contributions(self):
        """(keys [R*F] sorted, field << 40 | id, gV [R*F, 16], gW [R*F]): the per-(row, field) gradient
        rows in the order the coalescing pass summed them (id 2^40 - 1: a dropped contribution)."""
        if self._sparse is None:
            raise RuntimeError("deepfm_train_step was called without return_grads=True")
        return self._sparse[0], self._sparse[6], self._sparse[7]


def deepfm_train_step(x, y, emb_tables, lin_tables, emb_m, emb_v, lin_m, lin_v, out_bias, dnn_weights, dnn_biases,
                      w_out, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, reduction="mean", return_grads=False,
                      id_flag=None, cache=None):
    """One DeepFM training step over raw tensors, no host synchronisation: forward keeping the
    activations, Logloss (binary cross-entropy on the logit, reduction "mean" | "sum"), backward, and
    the torch.optim.SparseAdam update of the rows of emb_tables [vocab_f, 16] / lin_tables [vocab_f]
    that occur in x [R, F] (moments emb_m / emb_v / lin_m / lin_v, same shapes; `step` = the shared
    step count after this step's increment, >= 1), applied in place. The dense gradients are returned
    for the caller's Adam (DeepFMStep.dense: W1, b1, W2, b2, w_out, out.bias). out_bias: the [1]
    device tensor. id_flag: device int32 [1] set to 1 when an id lies outside its field's vocab (such
    an id reads row 0 and its contribution is dropped). cache: a dict the caller keeps for the
    zero-padded image of W1's columns (refreshed here every step)."""
    N.ensure_device(x)
    if reduction not in ("mean", "sum"):
        raise ValueError('reduction must be "mean" or "sum"')
    x = _c(x.to(torch.int64))
    R, F = x.shape
    why = deepfm_train_supported(F, emb_tables[0].shape[1], [w.shape[0] for w in dnn_weights])
    if why:
        raise NotImplementedError(why)
    if len(emb_tables) != F or len(lin_tables) != F or tuple(dnn_weights[0].shape) != (256, F * 16):
        raise ValueError(f"deepfm: {len(emb_tables)} embedding / {len(lin_tables)} linear tables for {F} fields")
    if R < 1:
        raise ValueError("deepfm_train_step needs at least one row")
    groups = (emb_tables, lin_tables, emb_m, emb_v, lin_m, lin_v)
    for grp in groups:
        for t, e in zip(grp, emb_tables):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != e.shape[0] or t.device != x.device:
                raise ValueError("deepfm_train_step: tables and moments must be contiguous fp32 of their field's vocab")
    dev, lib, st = x.device, N.lib(), N.stream()
    n = R * F
    y = _c(y.to(device=dev, dtype=torch.float32).reshape(-1))
    if y.numel() != R:
        raise ValueError(f"deepfm_train_step: {y.numel()} labels for {R} rows")
    w1, w2 = _c(dnn_weights[0]), _c(dnn_weights[1])
    b1, b2 = _c(dnn_biases[0]), _c(dnn_biases[1])
    wo = _c(w_out.reshape(-1))
    vocab = N.i64_array([t.shape[0] for t in emb_tables])
    flag = id_flag if id_flag is not None else torch.zeros(1, device=dev, dtype=torch.int32)

    # 1. keys, checked ids, the sorted index (segment heads and counts stay on the device)
    keys = torch.empty(n, device=dev, dtype=torch.int64)
    xs = torch.empty(n, device=dev, dtype=torch.int64)
    with timed("deepfm_train/index"):
        N.check(lib.rsx_deepfm_train_keys(N.ptr(x), R, F, vocab, N.ptr(keys), N.ptr(xs), N.ptr(flag), st),
                "deepfm_train_keys")
        keys_sorted, perm = torch.sort(keys, stable=True)
        head = torch.empty(n, device=dev, dtype=torch.int32)
        inv = torch.empty(n, device=dev, dtype=torch.int32)
        N.check(lib.rsx_deepfm_train_segments(N.ptr(keys_sorted), N.ptr(perm), n, N.ptr(head), N.ptr(inv), st),
                "deepfm_train_segments")
        cum = torch.cumsum(head, 0, dtype=torch.int32)
        seg_start = torch.empty(n + 1, device=dev, dtype=torch.int32)
        nseg = torch.empty(1, device=dev, dtype=torch.int32)
        N.check(lib.rsx_deepfm_train_starts(N.ptr(cum), n, N.ptr(seg_start), N.ptr(nseg), st), "deepfm_train_starts")

    # 2. forward keeping emb, h1, h2; the head
    V, W = N.ptr_array(emb_tables), N.ptr_array(lin_tables)
    emb = torch.empty(R, F * 16, device=dev, dtype=torch.float32)
    lin = torch.empty(R, device=dev, dtype=torch.float32)
    with timed("deepfm_train/forward"):
        N.check(lib.rsx_deepfm_embed(N.ptr(xs), R, F, 16, V, W, 0.0, N.ptr(emb), N.ptr(lin), st), "deepfm_embed")
        h1 = linear(emb, w1, b1, ACT_RELU)
        h2 = linear(h1, w2, b2, ACT_RELU)
        logit = torch.empty(R, device=dev, dtype=torch.float32)
        g = torch.empty(R, device=dev, dtype=torch.float32)
        dh2 = torch.empty(R, 128, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float64)
        dbias = torch.empty(1, device=dev, dtype=torch.float32)
        dwo = torch.empty(128, device=dev, dtype=torch.float32)
        nws = lib.rsx_deepfm_train_head_workspace_bytes(R)
        ws = torch.empty(nws, device=dev, dtype=torch.uint8)
        N.check(lib.rsx_deepfm_train_head(N.ptr(h2), 128, N.ptr(wo), N.ptr(lin), N.ptr(_c(out_bias)), N.ptr(y), R,
                                          1 if reduction == "mean" else 0, N.ptr(logit), N.ptr(g), N.ptr(dh2),
                                          N.ptr(ws), nws, N.ptr(loss), N.ptr(dbias), N.ptr(dwo), st),
                "deepfm_train_head")

    # 3. dense backward on the existing GEMMs
    with timed("deepfm_train/dense_bwd"):
        # exact fp32 products for the dense weight gradients
        dw2, db2 = linear_wgrad(dh2, h1, w2.shape, True, tag="deepfm_train/dw2", precision="fp32")
        dh1 = gemm_x3_tn(dh2, w2, tag="deepfm_train/dh1")
        N.check(lib.rsx_relu_bwd(N.ptr(dh1), N.ptr(h1), dh1.numel(), st), "relu_bwd")
        dw1, db1 = linear_wgrad(dh1, emb, w1.shape, True, tag="deepfm_train/dw1", precision="fp32")
        K = F * 16
        if K % 128 == 0:
            w1p = w1
        else:
            Kp = (K + 127) // 128 * 128
            w1p = cache.get("w1_padded") if cache is not None else None
            if w1p is None or w1p.shape != (256, Kp) or w1p.device != dev:
                w1p = torch.zeros(256, Kp, device=dev, dtype=torch.float32)
                if cache is not None:
                    cache["w1_padded"] = w1p
            w1p[:, :K].copy_(w1)
        dE = gemm_x3_tn(dh1, w1p, tag="deepfm_train/dE")

    # 4./5. contribution rows at their sorted positions, then coalesce + SparseAdam per distinct id
    gV = torch.empty(n, 16, device=dev, dtype=torch.float32)
    gW = torch.empty(n, device=dev, dtype=torch.float32)
    oV = torch.empty(n, 16, device=dev, dtype=torch.float32) if return_grads else None
    oW = torch.empty(n, device=dev, dtype=torch.float32) if return_grads else None
    nws = lib.rsx_deepfm_train_sparse_workspace_bytes(n)
    ws2 = torch.empty(nws, device=dev, dtype=torch.uint8)
    with timed("deepfm_train/sparse"):
        N.check(lib.rsx_deepfm_train_contrib(N.ptr(emb), N.ptr(g), N.ptr(dE), dE.stride(0), N.ptr(inv), R, F, 16,
                                             N.ptr(gV), N.ptr(gW), st), "deepfm_train_contrib")
        N.check(lib.rsx_deepfm_train_sparse_adam(
            N.ptr(keys_sorted), N.ptr(cum), N.ptr(seg_start), N.ptr(nseg), n, F, 16, vocab, N.ptr(gV), N.ptr(gW), V, W,
            N.ptr_array(emb_m), N.ptr_array(emb_v), N.ptr_array(lin_m), N.ptr_array(lin_v), float(lr), float(betas[0]),
            float(betas[1]), float(eps), int(step), N.ptr(ws2), nws, N.ptr(oV), N.ptr(oW), st), "deepfm_train_sparse_adam")
    # the kernels wrote through raw pointers: advance the version counters the inference caches key on
    for grp in groups:
        for t in grp:
            torch.autograd.graph.increment_version(t)
    sparse = (keys_sorted, seg_start, nseg, oV, oW, F, gV, gW) if return_grads else None
    return DeepFMStep(loss, logit, [dw1, db1, dw2, db2, dwo, dbias], sparse)


# ----------------------------------------------------------------------------------------
# A16 validation: exact AUC and Logloss of a binary ranker (csrc/binary_eval.hip)
_BINARY_EVAL_WS = {}   # R -> workspace bytes (a host-side size computation, the same for every call)


class BinaryEval:
    """What binary_eval returns. The outputs stay on the device until result(): counts (int64 [3]:
    positives P, negatives N, U2 = twice the tie-aware Mann-Whitney U), loss_sum (float64 [1]) and
    flag (int32 [1]) are views of one 40-byte allocation, fetched by one copy."""

    def __init__(self, buf, rows):
        self._buf, self.rows = buf, rows
        self.counts, self.loss_sum, self.flag = buf[:3], buf[3:4].view(torch.float64), buf[4:5].view(torch.int32)[:1]

    def result(self, also=None):
        """The one host read: {"auc", "logloss", "positives", "negatives"}. auc = U2 / (2 P N) in
        double (NaN when one class is absent), logloss = loss_sum / R. ValueError for a non-finite
        logit or a label that is neither 0 nor 1. also: a float64 device tensor fetched by the same
        copy (its bits untouched); the return value is then (the dict, its values as a list)."""
        if also is None:
            host = self._buf.cpu()
        else:
            host = torch.cat([self._buf, also.detach().reshape(-1).view(torch.int64)]).cpu()
        out = self._result(host)
        return out if also is None else (out, host[5:].view(torch.float64).tolist())

    def _result(self, host):
        flag = int(host[4:5].view(torch.int32)[0])
        if flag:
            why = [w for b, w in ((1, "a logit is NaN or infinite"), (2, "a label is neither 0 nor 1")) if flag & b]
            raise ValueError("binary_eval: " + " and ".join(why))
        p, n, u2 = (int(v) for v in host[:3])
        loss = float(host[3:4].view(torch.float64)[0])
        return {"auc": u2 / (2 * p * n) if p and n else float("nan"), "logloss": loss / self.rows,
                "positives": p, "negatives": n}


def binary_eval(logit, y):
    """Exact tie-aware ROC-AUC and Logloss of the scores logit [R] (fp32, device) against the labels
    y [R] (any dtype, values 0 / 1), without a host synchronisation: rsx_binary_eval on the current
    stream. Returns a BinaryEval; its result() does the one host read."""
    N.ensure_device(logit)
    if logit.dtype != torch.float32:
        raise ValueError(f"binary_eval: logits must be float32 (got {logit.dtype})")
    z = _c(logit.detach().reshape(-1))
    R = z.numel()
    if R < 1:
        raise ValueError("binary_eval needs at least one row")
    y = _c(torch.as_tensor(y).detach().to(device=z.device, dtype=torch.float32).reshape(-1))
    if y.numel() != R:
        raise ValueError(f"binary_eval: {y.numel()} labels for {R} scores")
    lib = N.lib()
    nws = _BINARY_EVAL_WS.get(R)
    if nws is None:
        nws = _BINARY_EVAL_WS[R] = int(lib.rsx_binary_eval_workspace_bytes(R))
        if nws < 0:
            N.check(1, "binary_eval_workspace_bytes")
    ws = torch.empty(nws, device=z.device, dtype=torch.uint8)
    out = BinaryEval(torch.empty(5, device=z.device, dtype=torch.int64), R)
    with timed("binary_eval"):
        N.check(lib.rsx_binary_eval(N.ptr(z), N.ptr(y), R, N.ptr(ws), nws, N.ptr(out.counts), N.ptr(out.loss_sum),
                                    N.ptr(out.flag), N.stream()), "binary_eval")
    return out


# ----------------------------------------------------------------------------------------
# A16 grouped validation: per-query NDCG@top and QueryAUC (csrc/group_eval.hip)
NDCG_MAX_TOP = 65536
_GROUP_EVAL_WS = {}     # R -> workspace bytes
_NDCG_DISCOUNTS = {}    # (top, device) -> the table D[0..top]; device None = the host tensor


def _check_top(top, what):
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= NDCG_MAX_TOP:
        raise ValueError(f"{what}: top must be an integer in [1, {NDCG_MAX_TOP}] (got {top!r})")


def ndcg_discounts(top, device=None):
    """D [top + 1] float64 with D[i] = sum_{p<i} 1 / log2(p + 2): the cumulated DCG discounts of the
    0-based positions below i, a sequential float64 sum on the host (D[0] = 0, D[1] = 1). Cached per
    (top, device); device None -> the CPU tensor. The device never takes a logarithm: rsx_group_eval
    and the tests' reference index the same table."""
    _check_top(top, "ndcg_discounts")
    host = _NDCG_DISCOUNTS.get((top, None))
    if host is None:
        acc, vals = 0.0, [0.0]
        for p in range(top):
            acc += 1.0 / math.log2(p + 2)
            vals.append(acc)
        host = _NDCG_DISCOUNTS[(top, None)] = torch.tensor(vals, dtype=torch.float64)
    if device is None:
        return host
    device = torch.device(device)
    dev = _NDCG_DISCOUNTS.get((top, device))
    if dev is None:
        dev = _NDCG_DISCOUNTS[(top, device)] = host.to(device)
    return dev


class GroupEval:
    """What group_eval returns. The outputs stay on the device until result(): the summary (int64
    [3]: groups G, ndcg_groups, auc_groups; float64 [2]: ndcg_sum, auc_sum) and the flag (int32) are
    views of one 48-byte allocation, fetched by one copy; the per-group arrays (sized R, their first
    G entries written) are sliced by per_group() once result() has made G known."""

    def __init__(self, buf, rows, top, per_group):
        self._buf, self.rows, self.top, self._per_group = buf, rows, top, per_group
        self.summary, self.flag = buf[:5], buf[5:6].view(torch.int32)[:1]
        self.groups = None

    def result(self, also=None):
        """The one host read: {"ndcg", "query_auc", "groups", "ndcg_groups", "auc_groups"}. ndcg =
        the mean of NDCG_g over the ndcg_groups groups with a positive, query_auc = the mean of
        AUC_g over the auc_groups groups with both classes (NaN when there is none), formed in
        double. ValueError for a non-finite logit, a label that is neither 0 nor 1 or a group id
        out of range. also: as BinaryEval.result."""
        if also is None:
            host = self._buf.cpu()
        else:
            host = torch.cat([self._buf, also.detach().reshape(-1).view(torch.int64)]).cpu()
        out = self._result(host)
        return out if also is None else (out, host[6:].view(torch.float64).tolist())

    def _result(self, host):
        flag = int(host[5:6].view(torch.int32)[0])
        if flag:
            why = [w for b, w in ((1, "a logit is NaN or infinite"), (2, "a label is neither 0 nor 1"),
                                  (4, "a group id is outside [0, 2^31) or above max_group_id")) if flag & b]
            raise ValueError("group_eval: " + " and ".join(why))
        g, ng, na = (int(v) for v in host[:3])
        s_ndcg, s_auc = host[3:5].view(torch.float64).tolist()
        self.groups = g
        return {"ndcg": s_ndcg / ng if ng else float("nan"), "query_auc": s_auc / na if na else float("nan"),
                "groups": g, "ndcg_groups": ng, "auc_groups": na}

    def per_group(self):
        """(gid int32, P, N, U2 int64, dcg float64), device tensors [G], the groups ascending by id."""
        if self.groups is None:
            raise RuntimeError("GroupEval.per_group: call result() first (it reads the number of groups)")
        return tuple(t[:self.groups] for t in self._per_group)


def _fetch_evals(binary, group, also=None):
    """A BinaryEval's and a GroupEval's result() by one copy: (binary dict, group dict[, the values of
    the float64 device tensor `also` as a list])."""
    parts = [binary._buf, group._buf]
    if also is not None:
        parts.append(also.detach().reshape(-1).view(torch.int64))
    host = torch.cat(parts).cpu()
    out = (binary._result(host[:5]), group._result(host[5:11]))
    return out if also is None else out + (host[11:].view(torch.float64).tolist(),)


def group_ids_int32(group_id, device):
    """group_id (an integer tensor or array-like) as the contiguous int32 device tensor rsx_group_eval
    reads, without a host read: an id outside [0, 2^31) becomes -1, which the kernel flags."""
    g = torch.as_tensor(group_id)
    if g.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"group_eval: group_id must have an integer dtype (got {g.dtype})")
    g = g.detach().to(device).reshape(-1)
    if g.dtype == torch.int64:
        g = torch.where((g >= 0) & (g < 2 ** 31), g, torch.full_like(g, -1))
    return _c(g.to(torch.int32))


def group_eval(logit, y, group_id, top=10, max_group_id=None):
    """Per-query evaluation of the scores logit [R] (fp32, device) against the labels y [R] (any
    dtype, values 0 / 1) within the groups group_id [R] (integer dtype, ids in [0, 2^31), the rows of
    a group anywhere): every group's P, N, U2 and tie-averaged DCG@top, and the sums behind NDCG and
    QueryAUC (definitions: include/recsys_amd.h), without a host synchronisation: rsx_group_eval on
    the current stream. max_group_id: an upper bound of the ids, if the host knows one (fewer sort
    passes). Returns a GroupEval; its result() does the one host read."""
    N.ensure_device(logit)
    if logit.dtype != torch.float32:
        raise ValueError(f"group_eval: logits must be float32 (got {logit.dtype})")
    z = _c(logit.detach().reshape(-1))
    R = z.numel()
    if R < 1:
        raise ValueError("group_eval needs at least one row")
    y = _c(torch.as_tensor(y).detach().to(device=z.device, dtype=torch.float32).reshape(-1))
    if y.numel() != R:
        raise ValueError(f"group_eval: {y.numel()} labels for {R} scores")
    g = group_ids_int32(group_id, z.device)
    if g.numel() != R:
        raise ValueError(f"group_eval: {g.numel()} group ids for {R} scores")
    _check_top(top, "group_eval")
    if max_group_id is None:
        max_group_id = -1
    elif not 0 <= int(max_group_id) < 2 ** 31:
        raise ValueError(f"group_eval: max_group_id must be in [0, 2^31) (got {max_group_id!r})")
    lib = N.lib()
    nws = _GROUP_EVAL_WS.get(R)
    if nws is None:
        nws = _GROUP_EVAL_WS[R] = int(lib.rsx_group_eval_workspace_bytes(R))
        if nws < 0:
            N.check(1, "group_eval_workspace_bytes")
    D = ndcg_discounts(top, z.device)
    ws = torch.empty(nws, device=z.device, dtype=torch.uint8)
    gid = torch.empty(R, device=z.device, dtype=torch.int32)
    cnt = torch.empty(3, R, device=z.device, dtype=torch.int64)
    dcg = torch.empty(R, device=z.device, dtype=torch.float64)
    out = GroupEval(torch.empty(6, device=z.device, dtype=torch.int64), R, top, (gid, cnt[0], cnt[1], cnt[2], dcg))
    with timed("group_eval"):
        N.check(lib.rsx_group_eval(N.ptr(z), N.ptr(y), N.ptr(g), R, top, N.ptr(D), int(max_group_id), N.ptr(ws), nws,
                                   N.ptr(out.summary), N.ptr(gid), N.ptr(cnt[0]), N.ptr(cnt[1]), N.ptr(cnt[2]),
                                   N.ptr(dcg), N.ptr(out.flag), N.stream()), "group_eval")
    return out


# ----------------------------------------------------------------------------------------
# §8f #3: GDCN reranker batch (utils/data_preprocessing/feature_processor.py:144-195)
def reranker_batch(uidx, iidx, tables, max_len=50):
    """(dense [B,12] f32, cat [B], seq_ids [B,L], seq_mask [B,L], target [B]) of the batch rows
    uidx / iidx (int64 device row indices) from device tables (a dict: u_scaled [U,3] f32,
    u_raw [U,2] f64, u_cat [U], i_scaled [I,6] f32, i_raw [I,3] f64, i_num [I], seq_off [U+1],
    seq_ids [nnz]) on rsx_reranker_batch. L = the batch's longest min(len, max_len) (one host
    read of the per-row lengths: pad_sequence pads to the batch maximum)."""
    N.ensure_device(uidx)
    uidx, iidx = _c(uidx), _c(iidx)
    B = uidx.numel()
    dev = uidx.device
    t = tables
    lens = torch.empty(B, device=dev, dtype=torch.int64)
    N.check(N.lib().rsx_reranker_seq_lens(N.ptr(uidx), N.ptr(t["seq_off"]), B, int(max_len), N.ptr(lens), N.stream()),
            "reranker_seq_lens")
    L = int(lens.max().item()) if B > 0 else 0
    dense = torch.empty(B, 12, device=dev, dtype=torch.float32)
    cat = torch.empty(B, device=dev, dtype=torch.int64)
    target = torch.empty(B, device=dev, dtype=torch.int64)
    seq = torch.empty(B, L, device=dev, dtype=torch.int64)
    mask = torch.empty(B, L, device=dev, dtype=torch.int64)
    rc = N.lib().rsx_reranker_batch(
        N.ptr(uidx), N.ptr(iidx), B, N.ptr(t["u_scaled"]), N.ptr(t["u_raw"]), N.ptr(t["u_cat"]), N.ptr(t["i_scaled"]),
        N.ptr(t["i_raw"]), N.ptr(t["i_num"]), N.ptr(t["seq_off"]), N.ptr(t["seq_ids"]), int(max_len), L, N.ptr(dense),
        N.ptr(cat), N.ptr(target), N.ptr(seq), N.ptr(mask), N.stream())
    N.check(rc, "reranker_batch")
    return dense, cat, seq, mask, target


# ----------------------------------------------------------------------------------------
# A14: retrieval top-k
class IdRangeGuard:
    """Range check of embedding ids on the device without a host sync (rsx_ids_check): the call
    returns the ids with every out-of-range id replaced by 0 (the following gather stays in
    bounds) and copies a device flag into pinned host memory behind an event. The error is
    raised as IndexError by the next call whose flag is visible (a non-blocking event query) or
    by check(), which the callers run at their own synchronisation points -- like the
    asynchronous device-side assert an out-of-range nn.Embedding index raises on the
    reference's CUDA path."""

    def __init__(self, what):
        self.what = what
        self.pending = []

    def __call__(self, ids, n):
        self.poll()
        N.ensure_device(ids)
        ids = _c(ids.to(torch.int64))
        out = torch.empty_like(ids)
        flag = torch.zeros(1, device=ids.device, dtype=torch.int32)
        N.check(N.lib().rsx_ids_check(N.ptr(ids), ids.numel(), 0, int(n), N.ptr(out), N.ptr(flag), N.stream()),
                "ids_check")
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, host, flag, int(n)))
        return out

    def watch(self, flag, n=None):
        """Track a device int32 flag that a kernel sets for an out-of-range id (rsx_static_profile_fwd)
        in the same asynchronous way."""
        self.poll()
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, host, flag, n))

    def poll(self, wait=False):
        while self.pending and (wait or self.pending[0][0].query()):
            ev, host, _, n = self.pending.pop(0)
            ev.synchronize()
            if int(host[0]):
                self.pending.clear()
                rng = "its table's range" if n is None else f"[0, {n})"
                raise IndexError(f"{self.what}: id out of range {rng}")

    def check(self):
        """Raise for any call so far whose ids were out of range (waits for their checks)."""
        self.poll(wait=True)


# the static profile's nine lookups (v1_refine_usertower.py:472-481), checked inside prof_in_k
_STATIC_IDS = IdRangeGuard("static profile ids (SASRecUserTower's nine nn.Embedding lookups)")


_TOPK_PATHS = {0: "list", 1: "fast", 2: "bf16"}
_TOPK_CORPUS = {}


def _topk_corpus(it):
    """The bf16 corpus image of `it` for the single-scan path (rsx_topk_prepare_corpus), cached
    for the most recent corpus and rebuilt when it changes (identity, storage or in-place
    version, as DeepFM's images): retrieval corpora are static between calls (the serving
    index, evaluate_model's normalised item table), so the conversion pass runs once, not per
    call. A call on another stream waits for the image's build."""
    dev = it.device
    st = _TOPK_CORPUS.get(dev)
    if st is not None and st["key"].matches([it]):
        cur = torch.cuda.current_stream(dev)
        if cur != st["stream"]:
            cur.wait_event(st["event"])
            # the image is read on this stream too: its block must not return to the building
            # stream's pool (when the cache entry is replaced) before this stream's reads finish
            st["buf"].record_stream(cur)
        return st["buf"]
    NI = it.shape[0]
    buf = torch.empty(N.lib().rsx_topk_corpus_bytes(NI), device=dev, dtype=torch.uint8)
    with timed("retrieve_topk/prepare"):
        rc = N.lib().rsx_topk_prepare_corpus(N.ptr(it), it.stride(0), NI, N.ptr(buf), N.stream())
    N.check(rc, "topk_prepare_corpus")
    ev = torch.cuda.Event()
    ev.record()
    _TOPK_CORPUS[dev] = {"key": _FastKey([it]), "buf": buf, "event": ev,
                         "stream": torch.cuda.current_stream(dev)}
    return buf


def clear_retrieval_cache(device=None) -> None:
    """Drop the cached bf16 corpus image(s) (and the references to their corpora): about
    0.75 GB at 1M items. The next retrieval over a corpus rebuilds its image."""
    if device is None:
        _TOPK_CORPUS.clear()
    else:
        _TOPK_CORPUS.pop(torch.device(device), None)


RETRIEVE_TOPK_MAX = 2048  # rsx_topk_max_k(): largest k of retrieve_topk
_TOPK_NOT_NATIVE = 3      # rsx_topk_path: 512 < k <= 2048 on a corpus the bf16 plan does not serve


def _retrieve_topk_materialised(q, it, k):
    """retrieve_topk's composition where the fused scan does not apply: fp32 score chunks of at most
    the evaluators' SCORE_CHUNK_BYTES by torch.matmul, each selected by select_topk_rows."""
    from .tower_code.mined_inference import SCORE_CHUNK_BYTES
    Q, NI = q.shape[0], it.shape[0]
    sc = torch.empty(Q, k, device=q.device, dtype=torch.float32)
    ix = torch.empty(Q, k, device=q.device, dtype=torch.int64)
    w = it[:, :q.shape[1]].to(torch.float32)
    step = max(1, SCORE_CHUNK_BYTES // (4 * NI))
    for s in range(0, Q, step):
        idx, val = select_topk_rows(torch.matmul(q[s:s + step], w.T), k)
        sc[s:s + step], ix[s:s + step] = val, idx
    return sc, ix


def retrieve_topk(queries, items, k, diag=None):
    """(scores [Q, k] desc, indices [Q, k] int64) of queries @ items.T. Ties resolve to the lower
    item index. D = 128. Exact for 1 <= k <= min(NI, RETRIEVE_TOPK_MAX = 2048); a k outside that
    range raises ValueError before any device work (k <= 512 may exceed NI: the missing places hold
    index -1). Three behaviours:
      * k <= 512: the score matrix is never formed. Large corpora take the bf16 single scan + exact
        fp32 rescoring (path "bf16"), whose corpus image is cached across calls (_topk_corpus);
        small ones the fp32 paths ("list" / "fast").
      * 512 < k <= 2048 where the bf16 scan's plan applies (rsx_topk_path == 2: NI >= 131,072 for
        k <= 1024, NI >= 262,144 beyond): the same scan with a larger margin set; a query that fails
        its exactness check is served from fp32 score rows in a bounded scratch.
      * 512 < k <= 2048 on smaller corpora: fp32 score chunks by torch.matmul (at most
        SCORE_CHUNK_BYTES each) selected by select_topk_rows (path "materialised").
    diag: optional dict; receives "path" ("list" / "fast" / "bf16" / "materialised"), "fallback"
    (bool) and "fallback_queries" (int): how many queries the path's exactness check sent to the
    exact kernels (the "fast" path re-runs the whole batch; one host sync, for tests /
    diagnostics)."""
    k = int(k)
    NI = items.shape[0]
    if not 1 <= k <= RETRIEVE_TOPK_MAX or (k > 512 and k > NI):
        raise ValueError(f"retrieve_topk: k={k} out of range for {NI} items "
                         f"(1 <= k <= min(items, {RETRIEVE_TOPK_MAX}); k <= 512 may exceed the item count)")
    N.ensure_device(queries)
    q = _c(queries.to(torch.float32))
    it = items if (items.stride(-1) == 1 and items.stride(0) % 4 == 0) else items.contiguous()
    Q = q.shape[0]
    path = N.lib().rsx_topk_path(Q, NI, k)
    if path == _TOPK_NOT_NATIVE:
        sc, ix = _retrieve_topk_materialised(q, it, k)
        if diag is not None:
            diag["path"], diag["fallback"], diag["fallback_queries"] = "materialised", False, 0
        return sc, ix
    corpus = _topk_corpus(it) if path == 2 and Q > 0 else None
    nws = (N.lib().rsx_topk_workspace_bytes_corpus(Q, NI, k) if corpus is not None
           else N.lib().rsx_topk_workspace_bytes(Q, NI, k))
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8)
    sc = torch.empty(Q, k, device=q.device, dtype=torch.float32)
    ix = torch.empty(Q, k, device=q.device, dtype=torch.int64)
    with timed("retrieve_topk"):
        if corpus is not None:
            rc = N.lib().rsx_retrieve_topk_corpus(N.ptr(q), q.stride(0), N.ptr(it), it.stride(0), N.ptr(corpus), Q,
                                                  NI, k, N.ptr(ws), N.ptr(sc), N.ptr(ix), N.stream())
        else:
            rc = N.lib().rsx_retrieve_topk(N.ptr(q), q.stride(0), N.ptr(it), it.stride(0), Q, NI, k, N.ptr(ws),
                                           N.ptr(sc), N.ptr(ix), N.stream())
    N.check(rc, "retrieve_topk")
    if diag is not None:
        h = ws[:16].view(torch.int32).cpu().tolist()
        assert h[1] == path, (h, path)
        n = h[0] if path == 2 else (Q if (path == 1 and h[2]) else 0)
        diag["path"] = _TOPK_PATHS[path]
        diag["fallback"], diag["fallback_queries"] = n > 0, n
    return sc, ix


def hnm_mine(u_norm, i_norm, target_ids, k, hnm_threshold=0.90, temperature=1.0, ignored_at=None):
    """Hard-negative mining (v1_refine_usertower.py:641-669, 705-728, 776-790) in one kernel:
    per row the k largest of (u_norm @ i_norm.T) / temperature with same-target columns and
    columns whose item-item cosine exceeds hnm_threshold (off the diagonal) set to -inf.
    Returns (top_idx [N, k] int64, value desc then column asc; top_cos [N, k] raw cosines;
    avail [N] int32 = columns not ignored). No autograd (the reference mines under no_grad).
    ignored_at: optional [N, M] int64 column indices; then a 4th output [N, M] bool tells
    whether column ignored_at[i, m] is ignored for row i, read from the kernel's own masked
    workspace (the same item-item products and threshold test the mining used)."""
    N.ensure_device(u_norm)
    u = _c(u_norm.detach().to(torch.float32))
    it = _c(i_norm.detach().to(torch.float32))
    tg = _c(target_ids.to(torch.int64))
    n, d = u.shape
    if it.shape != u.shape or tg.shape != (n,):
        raise ValueError(f"hnm_mine: shapes {tuple(u.shape)} / {tuple(it.shape)} / {tuple(tg.shape)} disagree")
    if not 1 <= k <= n:
        raise ValueError(f"hnm_mine: k={k} out of range for N={n} (torch.topk would fail too)")
    if n > N.lib().rsx_hnm_max_rows():
        raise ValueError(f"hnm_mine: N={n} exceeds the LDS-resident row limit {N.lib().rsx_hnm_max_rows()}")
    idx = torch.empty(n, k, device=u.device, dtype=torch.int64)
    cos = torch.empty(n, k, device=u.device, dtype=torch.float32)
    avail = torch.empty(n, device=u.device, dtype=torch.int32)
    nws = N.lib().rsx_hnm_workspace_bytes(n)
    ws = torch.empty(nws, device=u.device, dtype=torch.uint8)
    with timed("hnm_mine"):
        rc = N.lib().rsx_hnm_mine(N.ptr(u), N.ptr(it), N.ptr(tg), n, d, k, float(hnm_threshold), float(temperature),
                                  N.ptr(ws), nws, N.ptr(idx), N.ptr(cos), N.ptr(avail), N.stream())
    N.check(rc, "hnm_mine")
    if ignored_at is None:
        return idx, cos, avail
    ldw = nws // (4 * n)
    masked = ws.view(torch.float32)[: n * ldw].view(n, ldw)
    return idx, cos, avail, torch.gather(masked, 1, ignored_at) == float("-inf")


# ----------------------------------------------------------------------------------------
# LightGCL (gnn_model/v1_lightgcl.py:163-186): normalised SpMM, low-rank view (csrc/lightgcl.hip)
# The kernels' shape constants, for the graph's chunk plan (built without the library) and the tests:
SPMM_CHUNK = 512          # rsx_spmm_norm_chunk_len(): neighbours per chunk of a long row
SPMM_ROWS_PER_WG = 64     # rsx_spmm_norm_rows_per_workgroup()
LOWRANK_ROWS_PER_WG = 256  # rsx_lowrank_rows_per_workgroup(): rows per tile of rsx_lowrank_proj
LOWRANK_MAX_SLOTS = 512   # its partial slots: min(tiles, 512)


def _rows16(fn, name, t):
    """t as fp32 [n, D] rows the lightgcl kernels read: unit column stride, row stride a multiple of
    4 floats, 16-B aligned (anything else is copied)."""
    D = _rows2(fn, name, t)
    if D not in (64, 128):
        raise ValueError(f"{fn}: {name} must have 64 or 128 columns, got {D}")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < D or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t


def spmm_norm(adj, X, R=None, alpha=1.0, rows=None, out=None):
    """alpha (R + A^ X) for the graph adj (gnn_model.v1_lightgcl.NormAdjacency: row_ptr, col, dinv and
    the long-row chunk plan), A^ = diag(dinv) B diag(dinv) never stored. rows None: every row, [n, D]
    (into out when given); rows int64 [m]: those destination rows only, dense [m, D]. No autograd
    (lightgcl_propagate is the differentiable form); deterministic."""
    fn = "spmm_norm"
    X = _rows16(fn, "X", X)
    N.ensure_device(X)
    n, D = adj.n, X.shape[1]
    if X.shape[0] != n or adj.row_ptr.device != X.device:
        raise ValueError(f"{fn}: X must be [{n}, D] on the graph's device {adj.row_ptr.device}")
    if R is not None:
        R = _rows16(fn, "R", R)
        if R.shape != X.shape or R.device != X.device:
            raise ValueError(f"{fn}: R must match X")
    if rows is not None:
        rows = _c(_index(fn, "rows", rows, X))
        m = rows.numel()
    else:
        m = n
    if out is None:
        out = torch.empty(m, D, device=X.device, dtype=torch.float32)
    elif out.shape != (m, D) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != X.device:
        raise ValueError(f"{fn}: out must be a contiguous fp32 [{m}, {D}] tensor on X's device")
    if m == 0:   # an empty rows list has no storage: its null pointer would read as "every row"
        return out
    if out.data_ptr() == X.data_ptr():
        raise ValueError(f"{fn}: out must not alias X")
    ws = adj.workspace(D) if rows is None else None
    with timed("lightgcl/spmm_norm"):
        rc = N.lib().rsx_spmm_norm(N.ptr(adj.row_ptr), N.ptr(adj.col), N.ptr(adj.dinv), n, N.ptr(X), X.stride(0),
                                   N.ptr(R), R.stride(0) if R is not None else 0, D, float(alpha), N.ptr(rows),
                                   m if rows is not None else 0, N.ptr(adj.long_rows), N.ptr(adj.part_off),
                                   N.ptr(adj.chunk_beg), N.ptr(adj.chunk_end), adj.long_rows.numel(),
                                   adj.chunk_beg.numel(), N.ptr(ws), ws.numel() if ws is not None else 0,
                                   N.ptr(out), D, N.stream())
    N.check(rc, fn)
    return out


def lowrank_proj(V, X):
    """V^T X [q, D] for V [n, q] (q <= 8) and X [n, D] in one streaming pass; deterministic."""
    fn = "lowrank_proj"
    X = _rows16(fn, "X", X)
    N.ensure_device(X)
    _f32(fn, "V", V, X)
    if V.dim() != 2 or V.shape[0] != X.shape[0] or not 1 <= V.shape[1] <= 8:
        raise ValueError(f"{fn}: V must be [{X.shape[0]}, q <= 8], got {tuple(V.shape)}")
    V = _c(V)
    n, q, D = X.shape[0], V.shape[1], X.shape[1]
    nws = N.lib().rsx_lowrank_proj_workspace_bytes(n, q, D)
    ws = torch.empty(nws, device=X.device, dtype=torch.uint8)
    P = torch.empty(q, D, device=X.device, dtype=torch.float32)
    with timed("lightgcl/lowrank_proj"):
        rc = N.lib().rsx_lowrank_proj(N.ptr(V), q, N.ptr(X), X.stride(0), n, q, D, N.ptr(ws), nws, N.ptr(P),
                                      N.stream())
    N.check(rc, fn)
    return P


def lowrank_update_(Y, V, W):
    """Y += V W in place, Y [n, D] contiguous, V [n, q], W [q, D]; deterministic."""
    fn = "lowrank_update_"
    D = _rows2(fn, "Y", Y)
    N.ensure_device(Y)
    _f32(fn, "V", V, Y)
    _f32(fn, "W", W, Y)
    if D not in (64, 128) or not Y.is_contiguous():
        raise ValueError(f"{fn}: Y must be contiguous with 64 or 128 columns")
    if V.dim() != 2 or V.shape[0] != Y.shape[0] or not 1 <= V.shape[1] <= 8 or W.shape != (V.shape[1], D):
        raise ValueError(f"{fn}: V must be [{Y.shape[0]}, q <= 8] and W [q, {D}]")
    V, W = _c(V), _c(W)
    with timed("lightgcl/lowrank_update"):
        rc = N.lib().rsx_lowrank_update(N.ptr(V), V.shape[1], N.ptr(W), Y.shape[0], V.shape[1], D, N.ptr(Y), D,
                                        N.stream())
    N.check(rc, fn)
    return Y


def _propagate(E, adj, n_layers, rows=None):
    """(1/(L+1)) sum_{k<=L} A^^k E by Horner, T <- E + A^ T: one rsx_spmm_norm per layer with R = E, the
    last one scaled (and restricted to `rows` when given); the output and one scratch [n, D] alternate
    as T."""
    if n_layers == 0:
        return E.clone() if rows is None else E[rows]
    bufs = [None, None]
    T = E
    for j in range(n_layers):
        if j == n_layers - 1:
            return spmm_norm(adj, T, R=E, alpha=1.0 / (n_layers + 1), rows=rows,
                             out=bufs[0] if rows is None else None)
        k = (n_layers - 1 - j) % 2
        if bufs[k] is None:
            bufs[k] = torch.empty(E.shape[0], E.shape[1], device=E.device, dtype=torch.float32)
        T = spmm_norm(adj, T, R=E, out=bufs[k])


class _LightGCLPropagate(torch.autograd.Function):
    """A^ is symmetric, so the backward is the forward on the gradient; nothing is saved."""

    @staticmethod
    def forward(ctx, E, adj, n_layers):
        ctx.adj, ctx.n_layers = adj, n_layers
        return _propagate(E, adj, n_layers)

    @staticmethod
    def backward(ctx, g):
        return _propagate(_rows16("lightgcl_propagate", "grad", g), ctx.adj, ctx.n_layers), None, None


def lightgcl_propagate(E, adj, n_layers, rows=None):
    """LightGCL's local view (gnn_model/v1_lightgcl.py:166-173): the mean of E, A^ E, ..., A^^L E.
    rows (in-range int64, no autograd): only those rows of it, the last layer computed for them alone."""
    if int(n_layers) < 0:
        raise ValueError("lightgcl_propagate: n_layers must be >= 0")
    E = _rows16("lightgcl_propagate", "E", E)
    N.ensure_device(E)
    if rows is not None:
        with torch.no_grad():
            return _propagate(E, adj, int(n_layers), _c(_index("lightgcl_propagate", "rows", rows, E)))
    return _LightGCLPropagate.apply(E, adj, int(n_layers))


def _scatter_add_sorted(dst, src, idx):
    """dst[idx[k]] += src[k] with repeated indices summed in a fixed order (ops.sort_segments' two-level
    plan and rsx_segment_sum_rows: no atomics). dst [rows, D] contiguous, src [m, D] contiguous."""
    if idx.numel() == 0:
        return
    _scatter_add_plan(dst, src, sort_segments(idx))


def _scatter_add_plan(dst, src, plan):
    """_scatter_add_sorted with the plan of ops.sort_segments(idx) given: one sort serves every table that is
    indexed by the same ids."""
    D = dst.shape[1]
    perm, cb, chunk_ids, ch_off, uniq = plan
    part = torch.empty(chunk_ids.numel(), D, device=dst.device, dtype=torch.float32)
    rc = N.lib().rsx_segment_sum_rows(N.ptr(src), D, N.ptr(perm), N.ptr(cb), N.ptr(chunk_ids), chunk_ids.numel(), D,
                                      None, -1, N.ptr(part), D, 0, N.stream())
    N.check(rc, "segment_sum_rows(chunks)")
    rc = N.lib().rsx_segment_sum_rows(N.ptr(part), D, N.ptr(chunk_ids), N.ptr(ch_off), N.ptr(uniq), uniq.numel(), D,
                                      None, -1, N.ptr(dst), D, 1, N.stream())
    N.check(rc, "segment_sum_rows(rows)")


class _GatherRowsSorted(torch.autograd.Function):
    """src[idx] whose backward sums repeated indices through the sorted segment sums (deterministic),
    where _GatherRows scatters them with float atomics."""

    @staticmethod
    def forward(ctx, src, idx):
        n, D = idx.numel(), src.shape[1]
        out = torch.empty(n, D, device=src.device, dtype=torch.float32)
        rc = N.lib().rsx_gather_rows(N.ptr(src), src.stride(0), N.ptr(idx), n, D, 0, 0.0, N.ptr(out), None, N.stream())
        N.check(rc, "gather_rows")
        ctx.rows = src.shape[0]
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dsrc = torch.zeros(ctx.rows, dy.shape[1], device=dy.device, dtype=torch.float32)
        _scatter_add_sorted(dsrc, _c(dy), idx)
        return dsrc, None


def gather_rows_sorted(src, idx):
    """src[idx] for fp32 rows of 64 / 128 columns and in-range int64 idx; the gradient of src is summed
    per row in a fixed order (a host synchronisation in the backward: ops.sort_segments)."""
    src = _rows16("gather_rows_sorted", "src", src)
    N.ensure_device(src)
    return _GatherRowsSorted.apply(src, _c(_index("gather_rows_sorted", "idx", idx, src)))


def _small_matmul(K, C):
    """K [q, q] @ C [q, D] as a broadcast product and a sum (fixed order; q <= 8)."""
    return (K.unsqueeze(2) * C.unsqueeze(0)).sum(1)


class _LightGCLGlobalRows(torch.autograd.Function):
    """global_final[rows] of gnn_model/v1_lightgcl.py:175-185 reassociated: with P = V^T E, C_1 = S.P,
    C_{j+1} = S.(K C_j), K = V^T U, it is (E[rows] + U[rows] sum_j C_j) / (L + 1). Nothing of the
    graph's size is saved or formed but the gradient of E. rows None: every row (the full view)."""

    @staticmethod
    def forward(ctx, E, view, rows, n_layers):
        inv = 1.0 / (n_layers + 1)
        S = view.S.unsqueeze(1)
        n, D = (rows.numel() if rows is not None else E.shape[0]), E.shape[1]
        out = torch.empty(n, D, device=E.device, dtype=torch.float32)
        rc = N.lib().rsx_gather_rows(N.ptr(E), E.stride(0), N.ptr(rows), n, D, 0, 0.0, N.ptr(out), None, N.stream())
        N.check(rc, "gather_rows")
        out *= inv
        Ur = view.U[rows] if rows is not None else view.U
        if n_layers > 0:
            C = S * lowrank_proj(view.V, E)
            W = C
            for _ in range(n_layers - 1):
                C = S * _small_matmul(view.K, C)
                W = W + C
            lowrank_update_(out, Ur, W * inv)
        ctx.view, ctx.n_layers, ctx.shape = view, n_layers, E.shape
        ctx.rows = rows
        ctx.save_for_backward(Ur)
        return out

    @staticmethod
    def backward(ctx, g):
        (Ur,) = ctx.saved_tensors
        view, L, rows = ctx.view, ctx.n_layers, ctx.rows
        g = _c(g) * (1.0 / (L + 1))
        if rows is None:
            dE = g
        else:
            dE = torch.zeros(ctx.shape, device=g.device, dtype=torch.float32)
            _scatter_add_sorted(dE, g, rows)
        if L > 0 and g.shape[0] > 0:
            S = view.S.unsqueeze(1)
            dW = lowrank_proj(Ur, g)          # d(sum_j C_j) = U[rows]^T g
            dC = dW
            Kt = view.K.t()
            for _ in range(L - 1):            # dC_j = dW + K^T (S . dC_{j+1})
                dC = dW + _small_matmul(Kt, S * dC)
            lowrank_update_(dE, view.V, S * dC)
        return dE, None, None, None


def lightgcl_global_rows(E, view, rows, n_layers):
    """The low-rank (SVD) view's rows of LightGCL without forming the [n, D] view. view: U [n, q],
    S [q], V [n, q] and K = V^T U [q, q] (gnn_model.v1_lightgcl.LowRankView); rows: in-range int64
    (repeats allowed), or None for the whole [n, D] view."""
    fn = "lightgcl_global_rows"
    if int(n_layers) < 0:
        raise ValueError(f"{fn}: n_layers must be >= 0")
    E = _rows16(fn, "E", E)
    N.ensure_device(E)
    if view.U.shape[0] != E.shape[0] or view.U.device != E.device:
        raise ValueError(f"{fn}: the view's factors must have E's {E.shape[0]} rows on its device")
    if rows is not None:
        rows = _c(_index(fn, "rows", rows, E))
    return _LightGCLGlobalRows.apply(E, view, rows, int(n_layers))


# ----------------------------------------------------------------------------------------
# Distillation of dot-product scores into unit vectors (gnn_model/distill_mag_to_cos_l2.py,
# csrc/distill.hip): MagnitudeEncoder's forward and one fused training step
DISTILL_WIDTHS = (64, 128, 64)      # input, hidden, output width of the kernels
DISTILL_PARAMS = 128 * 64 + 128 + 64 * 128 + 64 + 1   # w1, b1, w2, b2, logit_scale: 16,577


def distill_supported(input_dim, hidden_dim, output_dim):
    """None when the distillation kernels cover the widths, else the text naming the limit."""
    if (int(input_dim), int(hidden_dim), int(output_dim)) != DISTILL_WIDTHS:
        return (f"the MagnitudeEncoder kernels need the widths (input, hidden, output) = {DISTILL_WIDTHS} "
                f"(got {(int(input_dim), int(hidden_dim), int(output_dim))})")
    return None


def _distill_weights(fn, w1, b1, w2, b2, ref):
    """The encoder's four tensors: fp32 on ref's device, Linear shapes, the kernels' widths."""
    for name, t in (("w1", w1), ("w2", w2)):
        _rows2(fn, name, t)
        _f32(fn, name, t, ref)
    if w2.shape[1] != w1.shape[0]:
        raise ValueError(f"{fn}: w2 {tuple(w2.shape)} does not follow w1 {tuple(w1.shape)}")
    _f32_vec(fn, "b1", b1, w1.shape[0], ref)
    _f32_vec(fn, "b2", b2, w2.shape[0], ref)
    why = distill_supported(w1.shape[1], w1.shape[0], w2.shape[0])
    if why:
        raise NotImplementedError(f"{fn}: {why}")


def _rows64(fn, name, t):
    """t as fp32 [n, 64] rows the distillation kernels read (unit column stride, row stride a multiple
    of 4 floats, 16-B aligned; anything else is copied)."""
    D = _rows2(fn, name, t)
    if D != DISTILL_WIDTHS[0]:
        raise ValueError(f"{fn}: {name} must have {DISTILL_WIDTHS[0]} columns, got {D}")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < D or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t


def magnitude_encode(x, w1, b1, w2, b2, slope=0.2, eps=1e-12):
    """F.normalize(Linear(w2, b2)(leaky_relu(Linear(w1, b1)(x), slope)), eps=eps) over the rows of x
    [N, 64] in one kernel (MagnitudeEncoder's eval forward): [N, 64]. No autograd; deterministic; the
    arithmetic of distill_step's forward at p = 0, bit for bit."""
    fn = "magnitude_encode"
    x = _rows64(fn, "x", x)
    _distill_weights(fn, w1, b1, w2, b2, x)
    if not float(eps) > 0.0:
        raise ValueError(f"{fn}: eps must be positive (got {eps})")
    N.ensure_device(x)
    w1, b1, w2, b2 = (_c(t.detach()) for t in (w1, b1, w2, b2))
    y = torch.empty(x.shape[0], DISTILL_WIDTHS[2], device=x.device, dtype=torch.float32)
    with timed("distill/encode"):
        rc = N.lib().rsx_magnitude_encode(N.ptr(x), x.stride(0), x.shape[0], N.ptr(w1), N.ptr(b1), N.ptr(w2),
                                          N.ptr(b2), float(slope), float(eps), N.ptr(y), y.stride(0), N.stream())
    N.check(rc, fn)
    return y


class DistillStep:
    """What distill_step returns: loss (0-d float64 device tensor) and, on request, grads (w1, b1, w2,
    b2, logit_scale, views of one flat buffer), student_scores [B] (cos exp(logit_scale)),
    teacher_scores [B] (<u, i>) and rows [2B, 64] (the normalised student rows, users first); flag is the
    int32 [1] device flag the kernel sets for an id outside its table."""

    def __init__(self, loss, flag, grads=None, student_scores=None, teacher_scores=None, rows=None):
        self.loss, self.flag, self.grads = loss, flag, grads
        self.student_scores, self.teacher_scores, self.rows = student_scores, teacher_scores, rows


def distill_step(user_table, item_table, users, items, w1, b1, w2, b2, logit_scale, slope=0.2, p_drop=0.0, seed=0,
                 eps=1e-12, update=True, exp_avg=None, exp_avg_sq=None, step=1, lr=1e-3, betas=(0.9, 0.999),
                 adam_eps=1e-8, return_grads=False, return_scores=False, return_rows=False, flag=None):
    """One step of the projector's distillation over raw tensors in two launches, no host
    synchronisation: the rows user_table[users] / item_table[items] ([n, 64] fp32 tables, B int64 ids
    each) through the encoder (w1 [128, 64], b1, w2 [64, 128], b2, dropout (p_drop, seed) on the hidden
    layer), loss = mean_k (cos_k exp(logit_scale) - <u_k, i_k>)^2 and its gradients (none to the tables).
    update=True applies torch.optim.Adam's step number `step` (>= 1) in place to the five parameters and
    the flat moments exp_avg / exp_avg_sq [16,577] (parameter order); update=False computes the loss and
    the gradients only. A pair with an id outside its table sets flag (int32 [1], created zeroed when
    not given) and contributes nothing; the mean still divides by B. Returns a DistillStep."""
    fn = "distill_step"
    user_table = _rows64(fn, "user_table", user_table)
    item_table = _rows64(fn, "item_table", item_table)
    if item_table.device != user_table.device:
        raise RuntimeError(f"{fn}: item_table is on {item_table.device}, expected {user_table.device}")
    users = _index(fn, "users", users, user_table)
    items = _index(fn, "items", items, user_table, users.numel())
    B = users.numel()
    if B < 1:
        raise ValueError(f"{fn} needs at least one pair")
    _distill_weights(fn, w1, b1, w2, b2, user_table)
    _f32_vec(fn, "logit_scale", logit_scale, 1, user_table)
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError(f"{fn}: p_drop must be in [0, 1) (got {p_drop})")
    if not float(eps) > 0.0:
        raise ValueError(f"{fn}: eps must be positive (got {eps})")
    if update:
        if exp_avg is None or exp_avg_sq is None:
            raise ValueError(f"{fn}: update=True needs exp_avg and exp_avg_sq")
        _f32_vec(fn, "exp_avg", exp_avg, DISTILL_PARAMS, user_table)
        _f32_vec(fn, "exp_avg_sq", exp_avg_sq, DISTILL_PARAMS, user_table)
        if int(step) < 1:
            raise ValueError(f"{fn}: step counts from 1 (got {step})")
        for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("logit_scale", logit_scale),
                        ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if not t.is_contiguous():
                raise ValueError(f"{fn}: {name} is updated in place and must be contiguous")
    if flag is not None and (flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != user_table.device):
        raise ValueError(f"{fn}: flag must be an int32 tensor of one element on the tables' device")
    N.ensure_device(user_table)
    dev, lib, st = user_table.device, N.lib(), N.stream()
    users, items = _c(users), _c(items)
    w1, b1, w2, b2, ls = (_c(t.detach()) for t in (w1, b1, w2, b2, logit_scale))
    if flag is None:
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
    nws = lib.rsx_distill_workspace_bytes(B)
    ws = torch.empty(nws // 8, device=dev, dtype=torch.float64)
    loss = torch.empty((), device=dev, dtype=torch.float64)
    f32 = dict(device=dev, dtype=torch.float32)
    flat = torch.empty(DISTILL_PARAMS, **f32) if return_grads else None
    s_out = torch.empty(B, **f32) if return_scores else None
    t_out = torch.empty(B, **f32) if return_scores else None
    rows = torch.empty(2 * B, DISTILL_WIDTHS[2], **f32) if return_rows else None
    with timed("distill/grads"):
        rc = lib.rsx_distill_grads(N.ptr(user_table), user_table.stride(0), user_table.shape[0], N.ptr(item_table),
                                   item_table.stride(0), item_table.shape[0], N.ptr(users), N.ptr(items), B,
                                   N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(ls), float(slope),
                                   float(p_drop), int(seed), float(eps), N.ptr(ws), nws, N.ptr(s_out), N.ptr(t_out),
                                   N.ptr(rows), N.ptr(flag), st)
    N.check(rc, "distill_grads")
    with timed("distill/apply"):
        rc = lib.rsx_distill_apply(N.ptr(ws), nws, B, N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(ls),
                                   N.ptr(exp_avg) if update else None, N.ptr(exp_avg_sq) if update else None,
                                   N.ptr(flat), N.ptr(loss), 1 if update else 0, float(lr), float(betas[0]),
                                   float(betas[1]), float(adam_eps), int(step) if update else 0, st)
    N.check(rc, "distill_apply")
    grads = None
    if flat is not None:
        grads, o = [], 0
        for t in (w1, b1, w2, b2, ls):
            grads.append(flat[o:o + t.numel()].view(t.shape))
            o += t.numel()
    return DistillStep(loss, flag, grads, s_out, t_out, rows)


# ----------------------------------------------------------------------------------------
# Late fusion of two retrievers (tower_code/mined_inference.py): pool, fuse, hits (csrc/ensemble.hip)
SELECT_TOPK_MAX = 2048    # rsx_select_topk_rows: largest k
FUSE_MAX_POOL = 2048      # rsx_fuse_rank: largest candidate pool C
FUSE_MAX_ALPHAS = 32
FUSE_MAX_KS = 16
FUSE_MINMAX, FUSE_RRF = 0, 1
_FUSE_MODES = {"minmax": FUSE_MINMAX, "rrf": FUSE_RRF}


def select_topk_rows(S, k):
    """(idx [Q, k] int32, val [Q, k]) of the k largest entries of each row of the fp32 score matrix S
    [Q, N], in the order (value descending, index ascending); -0.0 and +0.0 tie. Exact for
    1 <= k <= min(N, 2048); the scores must be finite. Rows may be strided (unit column stride)."""
    fn = "select_topk_rows"
    _rows2(fn, "S", S)
    Q, n = S.shape
    k = int(k)
    if not 1 <= k <= min(n, SELECT_TOPK_MAX):
        raise ValueError(f"{fn}: k={k} out of range for N={n} (1 <= k <= min(N, {SELECT_TOPK_MAX}))")
    N.ensure_device(S)
    if S.stride(1) != 1 or S.stride(0) < n:
        S = S.contiguous()
    idx = torch.empty(Q, k, device=S.device, dtype=torch.int32)
    val = torch.empty(Q, k, device=S.device, dtype=torch.float32)
    with timed("select_topk_rows"):
        rc = N.lib().rsx_select_topk_rows(N.ptr(S), S.stride(0), Q, n, k, N.ptr(idx), N.ptr(val), N.stream())
    N.check(rc, fn)
    return idx, val


def _rows_vec(fn, name, t, ref=None):
    """t as fp32 [rows, D] rows read 16 bytes at a time, D in {64, 128} (unit column stride, row stride a
    multiple of 4 floats, 16-B aligned; anything else is copied)."""
    D = _rows2(fn, name, t)
    if D not in (64, 128):
        raise ValueError(f"{fn}: {name} must have 64 or 128 columns, got {D}")
    if ref is not None and t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < D or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t


def _truth_csr(fn, truth_off, truth, Q, ref):
    if truth_off.dtype != torch.int64 or truth.dtype != torch.int32:
        raise TypeError(f"{fn}: truth_off must be int64 and truth int32, got {truth_off.dtype} / {truth.dtype}")
    if truth_off.device != ref.device or truth.device != ref.device:
        raise RuntimeError(f"{fn}: the truth is on {truth_off.device} / {truth.device}, expected {ref.device}")
    if truth_off.dim() != 1 or truth_off.numel() != Q + 1 or truth.dim() != 1:
        raise ValueError(f"{fn}: truth_off must hold Q + 1 = {Q + 1} offsets (got {tuple(truth_off.shape)}) "
                         "and truth must be 1-D")
    return _c(truth_off), _c(truth)


class FuseRank:
    """What fuse_rank returns: hits [Q, A] int32 (bit j = hit@ks[j]), the flag and, on request, lists
    [Q, A, ks[-1]] int32 (each alpha's fused list without repeats, -1 padded) and the raw scores sa / sb
    [Q, C] of the pool entries."""

    def __init__(self, hits, flag, lists=None, sa=None, sb=None):
        self.hits, self.flag, self.lists, self.sa, self.sb = hits, flag, lists, sa, sb


def fusion_weights(alphas):
    """(wa, wb) as Python floats that are exact in fp32: float32(alpha) and float32(1.0 - alpha), the
    subtraction in double as Python does in `alpha * s_gnn + (1.0 - alpha) * s_seq`
    (tower_code/mined_inference.py:1162)."""
    wa = [ctypes.c_float(float(a)).value for a in alphas]
    wb = [ctypes.c_float(1.0 - float(a)).value for a in alphas]
    return wa, wb


def fuse_rank(ua, Ia, ub, Ib, cand, alphas, ks, truth_off, truth, mode="minmax", k_rrf=200.0, cut=None,
              return_lists=False, return_scores=False, flag=None):
    """Late fusion of retrievers a and b over each user's candidate pool, for every alpha, in one launch
    (include/recsys_amd.h, rsx_fuse_rank): ua [Q, Da], Ia [NI, Da], ub [Q, Db], Ib [NI, Db] (Da, Db in
    {64, 128}); cand [Q, C] int32 corpus rows, C <= 2048, duplicates kept; alphas: the weights of a
    (fusion_weights); ks ascending; cut defaults to min(C, ks[-1] + 20); the truth in CSR (truth_off int64
    [Q + 1], truth int32, each user's items ascending and distinct). mode "minmax" or "rrf".
    flag (int32 [1], created zeroed when not given) is set by a pool entry outside the corpus, which
    scores 0. Returns a FuseRank."""
    fn = "fuse_rank"
    ua = _rows_vec(fn, "ua", ua)
    Ia = _rows_vec(fn, "Ia", Ia, ua)
    ub = _rows_vec(fn, "ub", ub, ua)
    Ib = _rows_vec(fn, "Ib", Ib, ua)
    if ua.shape[1] != Ia.shape[1] or ub.shape[1] != Ib.shape[1]:
        raise ValueError(f"{fn}: widths disagree: ua {tuple(ua.shape)} / Ia {tuple(Ia.shape)}, "
                         f"ub {tuple(ub.shape)} / Ib {tuple(Ib.shape)}")
    Q, NI = ua.shape[0], Ia.shape[0]
    if ub.shape[0] != Q or Ib.shape[0] != NI:
        raise ValueError(f"{fn}: the two retrievers must share users and corpus: {Q} / {ub.shape[0]} users, "
                         f"{NI} / {Ib.shape[0]} items")
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != Q or cand.device != ua.device:
        raise ValueError(f"{fn}: cand must be an int32 [Q, C] tensor on the vectors' device")
    C = cand.shape[1]
    if not 1 <= C <= FUSE_MAX_POOL:
        raise ValueError(f"{fn}: the pool holds {C} entries; the kernel takes 1 to {FUSE_MAX_POOL}")
    if mode not in _FUSE_MODES:
        raise ValueError(f"{fn}: mode must be one of {sorted(_FUSE_MODES)}")
    wa, wb = fusion_weights(alphas)
    A = len(wa)
    if not 1 <= A <= FUSE_MAX_ALPHAS:
        raise ValueError(f"{fn}: need 1 to {FUSE_MAX_ALPHAS} alphas (got {A})")
    ks = [int(x) for x in ks]
    if not 1 <= len(ks) <= FUSE_MAX_KS or ks[0] < 1 or any(b < a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"{fn}: ks must be 1 to {FUSE_MAX_KS} ascending positive integers (got {ks})")
    cut = min(C, ks[-1] + 20) if cut is None else int(cut)
    if not (1 <= cut <= C and ks[-1] <= cut):
        raise ValueError(f"{fn}: need ks[-1] <= cut <= C (ks[-1]={ks[-1]}, cut={cut}, C={C})")
    truth_off, truth = _truth_csr(fn, truth_off, truth, Q, ua)
    own_flag = flag is None
    if not own_flag and (flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != ua.device):
        raise ValueError(f"{fn}: flag must be an int32 tensor of one element on the vectors' device")
    N.ensure_device(ua)
    dev = ua.device
    cand = _c(cand)
    if own_flag:
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
    hits = torch.empty(Q, A, device=dev, dtype=torch.int32)
    lists = torch.empty(Q, A, ks[-1], device=dev, dtype=torch.int32) if return_lists else None
    sa = torch.empty(Q, C, device=dev, dtype=torch.float32) if return_scores else None
    sb = torch.empty(Q, C, device=dev, dtype=torch.float32) if return_scores else None
    wa_c, wb_c = (ctypes.c_float * A)(*wa), (ctypes.c_float * A)(*wb)
    ks_c = (ctypes.c_int32 * len(ks))(*ks)
    with timed("fuse_rank"):
        rc = N.lib().rsx_fuse_rank(N.ptr(ua), ua.stride(0), N.ptr(Ia), Ia.stride(0), ua.shape[1], N.ptr(ub),
                                   ub.stride(0), N.ptr(Ib), Ib.stride(0), ub.shape[1], Q, NI, N.ptr(cand), C, wa_c,
                                   wb_c, A, _FUSE_MODES[mode], float(k_rrf), cut, ks_c, len(ks), N.ptr(truth_off),
                                   N.ptr(truth), truth.numel(), N.ptr(hits), N.ptr(lists), N.ptr(sa), N.ptr(sb),
                                   N.ptr(flag), N.stream())
    N.check(rc, fn)
    return FuseRank(hits, flag, lists, sa, sb)


def first_hit(lists, truth_off, truth):
    """[Q] int32: the smallest j with lists[q, j] in user q's truth (CSR: truth_off int64 [Q + 1], truth
    int32, each user's items ascending and distinct), or K = lists.shape[1] when there is none.
    lists [Q, K] is an integer tensor (int32 is read as it is, other integer types are converted)."""
    fn = "first_hit"
    if lists.dim() != 2 or lists.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{fn}: lists must be an int32 or int64 [Q, K] tensor")
    Q, K = lists.shape
    if K < 1:
        raise ValueError(f"{fn}: lists must have at least one column")
    truth_off, truth = _truth_csr(fn, truth_off, truth, Q, lists)
    N.ensure_device(lists)
    if lists.dtype != torch.int32:
        lists = lists.to(torch.int32)
    if lists.stride(1) != 1 or lists.stride(0) < K:
        lists = lists.contiguous()
    out = torch.empty(Q, device=lists.device, dtype=torch.int32)
    with timed("first_hit"):
        rc = N.lib().rsx_first_hit(N.ptr(lists), lists.stride(0), Q, K, N.ptr(truth_off), N.ptr(truth), truth.numel(),
                                   N.ptr(out), N.stream())
    N.check(rc, fn)
    return out


# ----------------------------------------------------------------------------------------
# HybridUserTower inference (tower_code/mined_inference.py, csrc/hybrid.hip): the dual-table adapter,
# the sequence input and the sequence-centric fusion
HYBRID_WIDTHS = (128, 64, 128)   # content row, GNN row, model width of the kernels
HYBRID_GATE_HIDDEN = 64
HYBRID_MAX_LEN = 64
HYBRID_TIME_ROWS = 1001
_HYBRID_IDS = IdRangeGuard("HybridUserTower ids (item ids, time deltas or token rows)")
_LOGQ_IDS = IdRangeGuard("pos_item_ids of the tower's logQ losses (rows of item_probs / precomputed_log_q)")


class AdapterParams:
    """The eight tensors of a ParallelAdapter and its LayerNorm eps, as the kernels read them."""

    def __init__(self, wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b, ln_eps=1e-5):
        self.tensors = tuple(_c(t.detach()) for t in (wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b))
        self.ln_eps = float(ln_eps)

    def check(self, fn, ref):
        Dc, Dg, D = HYBRID_WIDTHS
        shapes = ((D, Dc), (D,), (D,), (D,), (D, Dg), (D,), (D,), (D,))
        for name, t, shp in zip(("wc", "bc", "lnc_w", "lnc_b", "wg", "bg", "lng_w", "lng_b"), self.tensors, shapes):
            _f32(fn, name, t, ref)
            if tuple(t.shape) != shp:
                raise ValueError(f"{fn}: {name} has shape {tuple(t.shape)}, the adapter kernel takes {shp}")


def _hybrid_table(fn, name, t, width):
    D = _rows2(fn, name, t)
    if D != width:
        raise ValueError(f"{fn}: {name} must have {width} columns, got {D}")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < D or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t.detach()


def _time_table(fn, time_tab, ref):
    _f32(fn, "time_tab", time_tab, ref)
    if tuple(time_tab.shape) != (HYBRID_TIME_ROWS, HYBRID_WIDTHS[2]):
        raise ValueError(f"{fn}: time_tab has shape {tuple(time_tab.shape)}, expected "
                         f"{(HYBRID_TIME_ROWS, HYBRID_WIDTHS[2])}")
    return _c(time_tab.detach())


def hybrid_adapter(content, gnn, params, ids=None, first_row=0, rows=None, deltas=None, time_tab=None, scale=1.0,
                   want_merged=True, want_unit=False, eps=1e-12):
    """ParallelAdapter's eval forward over gathered rows in one launch (rsx_hybrid_adapter_fwd):
    m = gelu(LN(Wc c + bc)) + c + gelu(LN(Wg g + bg)) with c = content[id] [*, 128], g = gnn[id] [*, 64]
    and id = ids.flatten()[r] (any shape, repeats allowed) or, without ids, first_row + r for r < rows
    (default: to the end of the shorter table). Returns (merged, unit, seq_in), each [R, 128] or None:
    merged = m, unit = m / max(|m|, eps), seq_in = m scale + time_tab[min(deltas, 1000)] when deltas is
    given. No autograd; deterministic; a row's bits depend on its id (and delta) alone. An id outside
    the tables raises IndexError asynchronously (IdRangeGuard)."""
    fn = "hybrid_adapter"
    Dc, Dg, D = HYBRID_WIDTHS
    content = _hybrid_table(fn, "content", content, Dc)
    gnn = _hybrid_table(fn, "gnn", gnn, Dg)
    _f32(fn, "gnn", gnn, content)
    params.check(fn, content)
    n_tab = min(content.shape[0], gnn.shape[0])
    if ids is not None:
        ids = _c(_index(fn, "ids", ids, content))
        R = ids.numel()
    else:
        first_row = int(first_row)
        R = n_tab - first_row if rows is None else int(rows)
        if first_row < 0 or R < 0 or first_row + R > n_tab:
            raise ValueError(f"{fn}: rows [{first_row}, {first_row + R}) exceed the tables ({n_tab} rows)")
    want_seq = deltas is not None
    if want_seq:
        if time_tab is None:
            raise ValueError(f"{fn}: deltas need time_tab")
        deltas = _c(_index(fn, "deltas", deltas, content, R))
        time_tab = _time_table(fn, time_tab, content)
    if not (want_merged or want_unit or want_seq):
        raise ValueError(f"{fn}: no output requested")
    N.ensure_device(content)
    dev = content.device
    new = lambda on: torch.empty(R, D, device=dev, dtype=torch.float32) if on else None  # noqa: E731
    merged, unit, seq_in = new(want_merged), new(want_unit), new(want_seq)
    if R == 0:
        return merged, unit, seq_in
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("hybrid/adapter"):
        rc = N.lib().rsx_hybrid_adapter_fwd(
            N.ptr(content), content.stride(0), content.shape[0], Dc, N.ptr(gnn), gnn.stride(0), gnn.shape[0], Dg,
            N.ptr(ids), first_row if ids is None else 0, R, *(N.ptr(t) for t in params.tensors), params.ln_eps,
            float(eps), N.ptr(deltas), N.ptr(time_tab), float(scale), N.ptr(merged), N.ptr(unit), N.ptr(seq_in),
            N.ptr(flag), N.stream())
    N.check(rc, fn)
    _HYBRID_IDS.watch(flag)
    return merged, unit, seq_in


def hybrid_seq_gather(merged, ids, deltas, time_tab, scale=1.0, first_row=0):
    """seq_in [T, 128] = merged[ids - first_row] scale + time_tab[min(deltas, 1000)] from the merged
    table of hybrid_adapter(first_row=first_row): the adapter once per item instead of once per token,
    the same bits as its seq_in. An id below first_row (the padding id) reads a zero row."""
    fn = "hybrid_seq_gather"
    D = HYBRID_WIDTHS[2]
    if _rows2(fn, "merged", merged) != D:
        raise ValueError(f"{fn}: merged must have {D} columns, got {merged.shape[1]}")
    merged = _c(merged.detach())
    ids = _c(_index(fn, "ids", ids, merged))
    T = ids.numel()
    deltas = _c(_index(fn, "deltas", deltas, merged, T))
    time_tab = _time_table(fn, time_tab, merged)
    N.ensure_device(merged)
    seq_in = torch.empty(T, D, device=merged.device, dtype=torch.float32)
    if T == 0:
        return seq_in
    flag = torch.zeros(1, device=merged.device, dtype=torch.int32)
    with timed("hybrid/seq_gather"):
        rc = N.lib().rsx_hybrid_seq_gather(N.ptr(merged), merged.shape[0], D, int(first_row), N.ptr(ids), N.ptr(deltas),
                                           T, N.ptr(time_tab), float(scale), N.ptr(seq_in), N.ptr(flag), N.stream())
    N.check(rc, fn)
    _HYBRID_IDS.watch(flag)
    return seq_in


def hybrid_fuse(seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, rows=None, ln_eps=1e-5, eps=1e-12,
                want_v=True, want_gate=True):
    """SequenceCentricFusion with the normalisations around it, per token row (rsx_hybrid_fuse_fwd):
    v = normalize(seq_out), g = sigmoid(W2 gelu(W1 v + b1) + b2), out = normalize(LN(v + g0 u_gnn[u] +
    g1 u_meta[u])). seq_out [B, L, 128] (L <= 64); u_gnn / u_meta [B, 128], the outputs of gnn_proj /
    meta_proj; rows: int64 token rows b L + l to fuse (None: all, in order). Returns (out [n, 128],
    v [n, 128] or None, gate_mean [2] device floats (the means of g0, g1 over the n rows) or None).
    No autograd; bit-reproducible."""
    fn = "hybrid_fuse"
    D = HYBRID_WIDTHS[2]
    _f32(fn, "seq_out", seq_out)
    if seq_out.dim() != 3 or seq_out.shape[2] != D:
        raise ValueError(f"{fn}: seq_out must be [B, L, {D}], got shape {tuple(seq_out.shape)}")
    B, L = seq_out.shape[:2]
    if not 1 <= L <= HYBRID_MAX_LEN:
        raise ValueError(f"{fn}: L must be in [1, {HYBRID_MAX_LEN}], got {L}")
    for name, t, shp in (("u_gnn", u_gnn, (B, D)), ("u_meta", u_meta, (B, D)), ("w1", w1, (HYBRID_GATE_HIDDEN, D)),
                         ("b1", b1, (HYBRID_GATE_HIDDEN,)), ("w2", w2, (2, HYBRID_GATE_HIDDEN)), ("b2", b2, (2,)),
                         ("ln_w", ln_w, (D,)), ("ln_b", ln_b, (D,))):
        _f32(fn, name, t, seq_out)
        if tuple(t.shape) != shp:
            raise ValueError(f"{fn}: {name} has shape {tuple(t.shape)}, expected {shp}")
    if rows is not None:
        rows = _c(_index(fn, "rows", rows, seq_out))
    n = B * L if rows is None else rows.numel()
    N.ensure_device(seq_out)
    dev = seq_out.device
    seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b = (_c(t.detach()) for t in (seq_out, u_gnn, u_meta, w1, b1, w2,
                                                                                  b2, ln_w, ln_b))
    out = torch.empty(n, D, device=dev, dtype=torch.float32)
    v = torch.empty(n, D, device=dev, dtype=torch.float32) if want_v else None
    gate = torch.zeros(2, device=dev, dtype=torch.float32) if want_gate else None
    if n == 0:
        return out, v, gate
    slots = N.lib().rsx_hybrid_fuse_slots(n)
    ws = torch.empty(2 * slots, device=dev, dtype=torch.float64) if want_gate else None
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("hybrid/fuse"):
        rc = N.lib().rsx_hybrid_fuse_fwd(N.ptr(seq_out), B, L, D, N.ptr(rows), n if rows is not None else 0,
                                         N.ptr(u_gnn), N.ptr(u_meta), N.ptr(w1), N.ptr(b1), HYBRID_GATE_HIDDEN,
                                         N.ptr(w2), N.ptr(b2), N.ptr(ln_w), N.ptr(ln_b), float(ln_eps), float(eps),
                                         N.ptr(out), N.ptr(v), N.ptr(gate), N.ptr(ws), 16 * slots if want_gate else 0,
                                         N.ptr(flag), N.stream())
    N.check(rc, fn)
    _HYBRID_IDS.watch(flag)
    return out, v, gate


class _HybridAdapterTrain(torch.autograd.Function):
    """The adapter with gradients (rsx_hybrid_adapter_train_fwd / rsx_hybrid_adapter_bwd). Saved for the
    backward: the gathered rows (768 bytes per token) and the two pre-LayerNorm products (1,024): the
    LayerNorm statistics, the GELUs and the keep masks are recomputed."""

    @staticmethod
    def forward(ctx, content, gnn, time_tab, ids, deltas, wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b, ln_eps, scale,
                p_drop, seed_c, seed_g):
        Dc, Dg, D = HYBRID_WIDTHS
        dev, R = content.device, ids.numel()
        new = lambda w: torch.empty(R, w, device=dev, dtype=torch.float32)  # noqa: E731
        out, xc, xg, zc, zg = new(D), new(Dc), new(Dg), new(D), new(D)
        seq = deltas is not None
        params = tuple(_c(t.detach()) for t in (wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b))
        if R > 0:
            flag = torch.zeros(1, device=dev, dtype=torch.int32)
            tab_c, tab_g = _hybrid_table("hybrid_adapter_train", "content", content, Dc), \
                _hybrid_table("hybrid_adapter_train", "gnn", gnn, Dg)
            with timed("hybrid/adapter_train"):
                rc = N.lib().rsx_hybrid_adapter_train_fwd(
                    N.ptr(tab_c), tab_c.stride(0), tab_c.shape[0], Dc, N.ptr(tab_g), tab_g.stride(0), tab_g.shape[0],
                    Dg, N.ptr(ids), R, *(N.ptr(t) for t in params), float(ln_eps), N.ptr(deltas),
                    N.ptr(None if time_tab is None else _c(time_tab.detach())), float(scale), float(p_drop),
                    int(seed_c), int(seed_g), None if seq else N.ptr(out), N.ptr(out) if seq else None, N.ptr(xc),
                    N.ptr(xg), N.ptr(zc), N.ptr(zg), N.ptr(flag), N.stream())
            N.check(rc, "hybrid_adapter_train")
            _HYBRID_IDS.watch(flag)
        ctx.save_for_backward(ids, deltas, xc, xg, zc, zg, *params)
        ctx.cfg = (float(ln_eps), float(scale) if seq else 1.0, float(p_drop), int(seed_c), int(seed_g),
                   content.shape[0], gnn.shape[0], None if time_tab is None else time_tab.shape[0])
        return out

    @staticmethod
    def backward(ctx, dy):
        ids, deltas, xc, xg, zc, zg, wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b = ctx.saved_tensors
        ln_eps, gscale, p_drop, seed_c, seed_g, n_c, n_g, n_t = ctx.cfg
        Dc, Dg, D = HYBRID_WIDTHS
        dev, R = dy.device, ids.numel()
        need = ctx.needs_input_grad
        dy = _c(dy.to(torch.float32))
        new = lambda w: torch.empty(R, w, device=dev, dtype=torch.float32)  # noqa: E731
        dzc, dzg, dc, dg = new(D), new(D), new(Dc), new(Dg)
        dln = torch.empty(4, D, device=dev, dtype=torch.float32)
        nws = N.lib().rsx_hybrid_adapter_bwd_workspace_floats(R)
        ws = torch.empty(max(nws, 1), device=dev, dtype=torch.float32)
        with timed("hybrid/adapter_bwd"):
            rc = N.lib().rsx_hybrid_adapter_bwd(N.ptr(dy), gscale, R, N.ptr(zc), N.ptr(zg), N.ptr(wc), N.ptr(wg),
                                                N.ptr(lnc_w), N.ptr(lnc_b), N.ptr(lng_w), N.ptr(lng_b), ln_eps, p_drop,
                                                seed_c, seed_g, N.ptr(dzc), N.ptr(dzg), N.ptr(dc), N.ptr(dg),
                                                N.ptr(dln), N.ptr(ws), nws, N.stream())
        N.check(rc, "hybrid_adapter_bwd")
        dwc = dbc = dwg = dbg = None
        if need[5] or need[6]:
            dwc, dbc = linear_wgrad(dzc, xc, (D, Dc), True, tag="hybrid/adapter_wgrad", precision="fp32")
        if need[9] or need[10]:
            dwg, dbg = linear_wgrad(dzg, xg, (D, Dg), True, tag="hybrid/adapter_wgrad", precision="fp32")
        dcontent = dgnn = dtime = None
        if (need[0] or need[1]) and R > 0:
            plan = sort_segments(ids)   # one sort for both item tables
            if need[0]:
                dcontent = torch.zeros(n_c, Dc, device=dev, dtype=torch.float32)
                _scatter_add_plan(dcontent, dc, plan)
            if need[1]:
                dgnn = torch.zeros(n_g, Dg, device=dev, dtype=torch.float32)
                _scatter_add_plan(dgnn, dg, plan)
        if need[2] and deltas is not None:
            dtime = torch.zeros(n_t, D, device=dev, dtype=torch.float32)
            _scatter_add_sorted(dtime, dy, deltas.clamp(0, HYBRID_TIME_ROWS - 1))   # the second sort
        return (dcontent, dgnn, dtime, None, None, dwc, dbc, dln[0], dln[1], dwg, dbg, dln[2], dln[3], None, None,
                None, None, None)


def hybrid_adapter_train(content, gnn, time_tab, ids, deltas, params, ln_eps=1e-5, scale=1.0, p_drop=0.0,
                         training=True):
    """ParallelAdapter with gradients over gathered rows: m = (drop(gelu(LN(Wc c + bc))) + c) +
    drop(gelu(LN(Wg g + bg))), c = content[ids], g = gnn[ids]. With deltas: seq_in = m scale +
    time_tab[min(deltas, 1000)] [T, 128]; with deltas None (time_tab may be None): merged = m, the item side of
    a loss. params: the eight adapter tensors (wc, bc, lnc_w, lnc_b, wg, bg, lng_w, lng_b) as they take
    gradients. In training mode with p_drop > 0 the two dropout sites draw ops.next_seed(), content first;
    otherwise no seed is drawn. Table gradients are dense; repeated ids are summed in a fixed order
    (ops.sort_segments: a host synchronisation in the backward). Deterministic. An id outside the tables is
    replaced by 0 before the forward (IdRangeGuard: IndexError at the next call or at
    ops._HYBRID_IDS.check()); the forward and the backward both use the replaced ids, and the time rows are
    min(max(delta, 0), 1000), so no gather or scatter leaves its table even if backward() runs before the
    error is raised."""
    fn = "hybrid_adapter_train"
    Dc, Dg, D = HYBRID_WIDTHS
    _f32(fn, "content", content)
    _f32(fn, "gnn", gnn, content)
    if _rows2(fn, "content", content) != Dc or _rows2(fn, "gnn", gnn) != Dg:
        raise ValueError(f"{fn}: content must have {Dc} columns and gnn {Dg}")
    if len(params) != 8:
        raise ValueError(f"{fn}: params must be the adapter's eight tensors")
    AdapterParams(*params, ln_eps=ln_eps).check(fn, content)
    ids = _index(fn, "ids", ids, content).reshape(-1)
    if deltas is not None:
        if time_tab is None:
            raise ValueError(f"{fn}: deltas need time_tab")
        _time_table(fn, time_tab, content)
        deltas = _c(_index(fn, "deltas", deltas, content, ids.numel())).reshape(-1)
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError(f"{fn}: p_drop must be in [0, 1)")
    N.ensure_device(content)
    # the ids as the kernels and the backward's scatter read them: an id outside the tables becomes 0 here
    # (rsx_ids_check) and is reported by _HYBRID_IDS, so the table gradients' segment sums stay in bounds
    if ids.numel() > 0:
        ids = _HYBRID_IDS(ids, min(content.shape[0], gnn.shape[0]))
    p = float(p_drop) if training else 0.0
    seed_c = next_seed() if p > 0 else 0
    seed_g = next_seed() if p > 0 else 0
    return _HybridAdapterTrain.apply(content, gnn, time_tab if deltas is not None else None, ids, deltas, *params,
                                     float(ln_eps), float(scale), p, seed_c, seed_g)


class _HybridFuseTrain(torch.autograd.Function):
    """The fusion with gradients (rsx_hybrid_fuse_train_fwd / rsx_hybrid_fuse_bwd). Nothing but the inputs
    and v_seq (an output) is saved: the backward recomputes the forward per tile."""

    @staticmethod
    def forward(ctx, seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, ln_eps, eps, p_drop, seed_a, seed_b):
        B, L, D = seq_out.shape
        dev, n = seq_out.device, B * L
        ts = tuple(_c(t.detach()) for t in (seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b))
        out = torch.empty(B, L, D, device=dev, dtype=torch.float32)
        v = torch.empty(B, L, D, device=dev, dtype=torch.float32)
        gate = torch.zeros(2, device=dev, dtype=torch.float32)
        if n > 0:
            slots = N.lib().rsx_hybrid_fuse_slots(n)
            ws = torch.empty(2 * slots, device=dev, dtype=torch.float64)
            flag = torch.zeros(1, device=dev, dtype=torch.int32)
            with timed("hybrid/fuse_train"):
                rc = N.lib().rsx_hybrid_fuse_train_fwd(*(N.ptr(t) for t in ts[:1]), B, L, *(N.ptr(t) for t in ts[1:]),
                                                       float(ln_eps), float(eps), float(p_drop), int(seed_a),
                                                       int(seed_b), N.ptr(out), N.ptr(v), N.ptr(gate), N.ptr(ws),
                                                       16 * slots, N.ptr(flag), N.stream())
            N.check(rc, "hybrid_fuse_train")
        ctx.save_for_backward(*ts, v)
        ctx.cfg = (float(ln_eps), float(eps), float(p_drop), int(seed_a), int(seed_b))
        ctx.mark_non_differentiable(gate)
        return out, v, gate

    @staticmethod
    def backward(ctx, dout, dv, _dgate):
        seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, v = ctx.saved_tensors
        ln_eps, eps, p_drop, seed_a, seed_b = ctx.cfg
        B, L, D = seq_out.shape
        H = HYBRID_GATE_HIDDEN
        dev, n = seq_out.device, B * L
        need = ctx.needs_input_grad
        dout = torch.zeros_like(seq_out) if dout is None else _c(dout.to(torch.float32))
        dv = None if dv is None else _c(dv.to(torch.float32))
        dx = torch.empty(B, L, D, device=dev, dtype=torch.float32)
        dpre = torch.empty(n, H, device=dev, dtype=torch.float32)
        dug = torch.zeros(B, D, device=dev, dtype=torch.float32)
        dum = torch.zeros(B, D, device=dev, dtype=torch.float32)
        dsmall = torch.empty(2 * D + 2 * H + 2, device=dev, dtype=torch.float32)
        nws = N.lib().rsx_hybrid_fuse_bwd_workspace_floats(B, L)
        ws = torch.empty(max(nws, 4), device=dev, dtype=torch.float32)
        with timed("hybrid/fuse_bwd"):
            rc = N.lib().rsx_hybrid_fuse_bwd(N.ptr(seq_out), B, L, N.ptr(u_gnn), N.ptr(u_meta), N.ptr(w1), N.ptr(b1),
                                             N.ptr(w2), N.ptr(b2), N.ptr(ln_w), N.ptr(ln_b), ln_eps, eps, p_drop,
                                             seed_a, seed_b, N.ptr(dout), N.ptr(dv), N.ptr(dx), N.ptr(dpre),
                                             N.ptr(dug), N.ptr(dum), N.ptr(dsmall), N.ptr(ws), nws, N.stream())
        N.check(rc, "hybrid_fuse_bwd")
        dw1 = db1 = None
        if need[3] or need[4]:
            dw1, db1 = linear_wgrad(dpre, v.view(n, D), (H, D), True, tag="hybrid/fuse_wgrad", precision="fp32")
        return (dx, dug, dum, dw1, db1, dsmall[2 * D:2 * D + 2 * H].view(2, H), dsmall[2 * D + 2 * H:], dsmall[:D],
                dsmall[D:2 * D], None, None, None, None, None)


def hybrid_fuse_train(seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, ln_eps=1e-5, eps=1e-12, p_drop=0.0,
                      training=True):
    """SequenceCentricFusion with gradients over all token rows (hybrid_fuse's arithmetic): returns (out
    [B, L, 128], v_seq [B, L, 128], gate_mean [2]); out and v_seq are differentiable in seq_out, u_gnn, u_meta
    and the six parameters, gate_mean (the means of the gates before dropout) is not. In training mode with
    p_drop > 0 each token draws its own keep masks over its copies of u_gnn[u] and u_meta[u] (two
    ops.next_seed() draws, the GNN row's first); otherwise no seed is drawn. Deterministic."""
    fn = "hybrid_fuse_train"
    D = HYBRID_WIDTHS[2]
    _f32(fn, "seq_out", seq_out)
    if seq_out.dim() != 3 or seq_out.shape[2] != D:
        raise ValueError(f"{fn}: seq_out must be [B, L, {D}], got shape {tuple(seq_out.shape)}")
    B, L = seq_out.shape[:2]
    if not 1 <= L <= HYBRID_MAX_LEN:
        raise ValueError(f"{fn}: L must be in [1, {HYBRID_MAX_LEN}], got {L}")
    for name, t, shp in (("u_gnn", u_gnn, (B, D)), ("u_meta", u_meta, (B, D)), ("w1", w1, (HYBRID_GATE_HIDDEN, D)),
                         ("b1", b1, (HYBRID_GATE_HIDDEN,)), ("w2", w2, (2, HYBRID_GATE_HIDDEN)), ("b2", b2, (2,)),
                         ("ln_w", ln_w, (D,)), ("ln_b", ln_b, (D,))):
        _f32(fn, name, t, seq_out)
        if tuple(t.shape) != shp:
            raise ValueError(f"{fn}: {name} has shape {tuple(t.shape)}, expected {shp}")
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError(f"{fn}: p_drop must be in [0, 1)")
    N.ensure_device(seq_out)
    p = float(p_drop) if training else 0.0
    seed_a = next_seed() if p > 0 else 0
    seed_b = next_seed() if p > 0 else 0
    return _HybridFuseTrain.apply(seq_out, u_gnn, u_meta, w1, b1, w2, b2, ln_w, ln_b, float(ln_eps), float(eps), p,
                                  seed_a, seed_b)


# ----------------------------------------------------------------------------------------
# A17 oblivious-tree boosting, the rerank stage's classifier (csrc/gbdt.hip; the model:
# include/recsys_amd.h, "oblivious-tree boosting")
GBDT_MAX_FEATURES = 32
GBDT_BINS = 256
GBDT_MAX_BORDERS = 254
GBDT_MAX_DEPTH = 6
GBDT_LEAF_STRIDE = 64
GBDT_SCALE = float(2 ** 30)     # qg = llrint(g * GBDT_SCALE)
RERANK_TABULAR_COLUMNS = ("two_tower_score", "vec_prod_mean", "vec_prod_max", "vec_prod_std", "item_price",
                          "user_avg_price", "price_diff_ratio")


class GBDTModel:
    """The trees gbdt_predict reads, all on one device: splits int32 [T, 6, 2] = (feature, bin) per level
    (the first `depth` levels used), leaf_values fp32 [T, 64], is_cat uint8 [F], f0 (host float, exactly
    an fp32 value) and n_trees <= T, the trees in use."""

    def __init__(self, splits, leaf_values, is_cat, depth, f0, n_trees):
        self.splits, self.leaf_values, self.is_cat = splits, leaf_values, is_cat
        self.depth, self.f0, self.n_trees = int(depth), float(f0), int(n_trees)


def _gbdt_rows(fn, name, t, dtype, R, ref):
    """t is a contiguous dtype vector of R elements on ref's device."""
    if t.dtype != dtype:
        raise TypeError(f"{fn}: {name} must be {dtype}, got {t.dtype}")
    if t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")
    if t.dim() != 1 or t.numel() != R or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous vector of {R} elements, got shape {tuple(t.shape)}")


def _gbdt_bins(fn, bins):
    """bins is a contiguous uint8 [F, R] device matrix, F <= 32, 1 <= R < 2^31; returns (F, R)."""
    N.ensure_device(bins)
    if bins.dtype != torch.uint8:
        raise TypeError(f"{fn}: bins must be uint8, got {bins.dtype}")
    if bins.dim() != 2 or not bins.is_contiguous():
        raise ValueError(f"{fn}: bins must be a contiguous [F, R] matrix, got shape {tuple(bins.shape)}")
    F, R = bins.shape
    if not (1 <= F <= GBDT_MAX_FEATURES and 1 <= R < 2 ** 31):
        raise ValueError(f"{fn}: need 1 <= F <= {GBDT_MAX_FEATURES} and 1 <= R < 2^31 (got F {F}, R {R})")
    return F, R


def _gbdt_leaves(fn, n_leaves):
    if n_leaves not in (1, 2, 4, 8, 16, 32):
        raise ValueError(f"{fn}: n_leaves must be 1, 2, 4, 8, 16 or 32 (got {n_leaves!r})")


_GBDT_GUARD = IdRangeGuard("gbdt: a leaf index or a split feature")
_RERANK_GUARD = IdRangeGuard("rerank_tabular candidate ids")


def gbdt_bin(x, borders, n_borders, out=None):
    """Numeric columns x [Fn, R] (fp32, device) -> their bins uint8 [Fn, R]: bin = #{borders < x}, NaN -> 0
    (rsx_gbdt_bin). borders [Fn, 256] fp32 ascending, the first n_borders[j] <= 254 (int32 [Fn], device) of
    row j valid. out: a contiguous uint8 [F >= Fn, R] matrix whose first Fn rows are written instead."""
    N.ensure_device(x)
    _f32("gbdt_bin", "x", x)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"gbdt_bin: x must be a contiguous [Fn, R] matrix, got shape {tuple(x.shape)}")
    Fn, R = x.shape
    if not (1 <= Fn <= GBDT_MAX_FEATURES and 1 <= R < 2 ** 31):
        raise ValueError(f"gbdt_bin: need 1 <= Fn <= {GBDT_MAX_FEATURES} and 1 <= R < 2^31 (got {Fn}, {R})")
    _f32("gbdt_bin", "borders", borders, x)
    if tuple(borders.shape) != (Fn, GBDT_BINS) or not borders.is_contiguous():
        raise ValueError(f"gbdt_bin: borders must be a contiguous [{Fn}, {GBDT_BINS}] matrix, got {tuple(borders.shape)}")
    _gbdt_rows("gbdt_bin", "n_borders", n_borders, torch.int32, Fn, x)
    if out is None:
        out = torch.empty(Fn, R, device=x.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < Fn or out.shape[1] != R or not out.is_contiguous() \
            or out.device != x.device:
        raise ValueError(f"gbdt_bin: out must be a contiguous uint8 [>= {Fn}, {R}] matrix on {x.device}")
    with timed("gbdt/bin"):
        N.check(N.lib().rsx_gbdt_bin(N.ptr(x), N.ptr(borders), N.ptr(n_borders), R, Fn, N.ptr(out), N.stream()), "gbdt_bin")
    return out


def gbdt_grad(F, y, out=None):
    """(qg, qh) int32 [R] of the approximant F [R] and the labels y [R] (both fp32, device): g = y -
    sigmoid(F) and h = sigmoid(F)(1 - sigmoid(F)) in fp32, each quantised to llrint(x 2^30) (rsx_gbdt_grad).
    out: a (qg, qh) pair to write."""
    N.ensure_device(F)
    _f32("gbdt_grad", "F", F)
    R = F.numel()
    if R < 1 or R >= 2 ** 31:
        raise ValueError(f"gbdt_grad: need 1 <= R < 2^31 rows (got {R})")
    _gbdt_rows("gbdt_grad", "F", F, torch.float32, R, F)
    _gbdt_rows("gbdt_grad", "y", y, torch.float32, R, F)
    qg, qh = out if out is not None else (torch.empty(R, device=F.device, dtype=torch.int32) for _ in range(2))
    _gbdt_rows("gbdt_grad", "qg", qg, torch.int32, R, F)
    _gbdt_rows("gbdt_grad", "qh", qh, torch.int32, R, F)
    with timed("gbdt/grad"):
        N.check(N.lib().rsx_gbdt_grad(N.ptr(F), N.ptr(y), R, N.ptr(qg), N.ptr(qh), N.stream()), "gbdt_grad")
    return qg, qh


def gbdt_histogram(bins, leaf, qg, qh, n_leaves, out=None):
    """hist int64 [n_leaves, F, 256, 2]: the exact sums of (qg, qh) (int32 [R]) over the rows of every
    (leaf, feature, bin); bins uint8 [F, R], leaf uint8 [R] < n_leaves in {1, 2, 4, 8, 16, 32}
    (rsx_gbdt_histogram: LDS and global integer atomics, the same bits every run). A leaf index out of
    range is skipped and raises IndexError at a later call."""
    F, R = _gbdt_bins("gbdt_histogram", bins)
    _gbdt_leaves("gbdt_histogram", n_leaves)
    _gbdt_rows("gbdt_histogram", "leaf", leaf, torch.uint8, R, bins)
    _gbdt_rows("gbdt_histogram", "qg", qg, torch.int32, R, bins)
    _gbdt_rows("gbdt_histogram", "qh", qh, torch.int32, R, bins)
    shape = (n_leaves, F, GBDT_BINS, 2)
    if out is None:
        out = torch.empty(shape, device=bins.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != bins.device:
        raise ValueError(f"gbdt_histogram: out must be a contiguous int64 {shape} tensor on {bins.device}")
    flag = torch.zeros(1, device=bins.device, dtype=torch.int32)
    with timed("gbdt/histogram"):
        N.check(N.lib().rsx_gbdt_histogram(N.ptr(bins), N.ptr(leaf), N.ptr(qg), N.ptr(qh), R, F, n_leaves, N.ptr(out),
                                           N.ptr(flag), N.stream()), "gbdt_histogram")
    _GBDT_GUARD.watch(flag)
    return out


def _gbdt_features(fn, is_cat, n_bins, F, ref):
    _gbdt_rows(fn, "is_cat", is_cat, torch.uint8, F, ref)
    if n_bins is not None:
        _gbdt_rows(fn, "n_bins", n_bins, torch.int32, F, ref)


def _gbdt_l2(fn, l2):
    if not float(l2) > 0.0:
        raise ValueError(f"{fn}: l2 must be positive (got {l2!r})")


def gbdt_best_split(hist, is_cat, n_bins, l2, out=None):
    """The best candidate of a level: (split int32 [2] = (f, b), score float64 [1]), on the device. hist
    int64 [n_leaves, F, 256, 2]; is_cat uint8 [F]; n_bins int32 [F]: the candidates of feature f are b <
    n_bins[f]; a numeric one sends bin > b right, a categorical one bin == b; the score is the sum over the
    leaves of G_L^2 / (H_L + l2) + G_R^2 / (H_R + l2) in fp64; ties go to the lowest f, then the lowest b
    (rsx_gbdt_best_split). out: the int32 [2] tensor to write the split to."""
    N.ensure_device(hist)
    if hist.dtype != torch.int64 or hist.dim() != 4 or tuple(hist.shape[2:]) != (GBDT_BINS, 2) or not hist.is_contiguous():
        raise ValueError(f"gbdt_best_split: hist must be a contiguous int64 [n_leaves, F, {GBDT_BINS}, 2] tensor")
    n_leaves, F = hist.shape[:2]
    _gbdt_leaves("gbdt_best_split", n_leaves)
    if not 1 <= F <= GBDT_MAX_FEATURES:
        raise ValueError(f"gbdt_best_split: need 1 <= F <= {GBDT_MAX_FEATURES} (got {F})")
    _gbdt_features("gbdt_best_split", is_cat, n_bins, F, hist)
    _gbdt_l2("gbdt_best_split", l2)
    split = out if out is not None else torch.empty(2, device=hist.device, dtype=torch.int32)
    _gbdt_rows("gbdt_best_split", "out", split, torch.int32, 2, hist)
    score = torch.empty(1, device=hist.device, dtype=torch.float64)
    ws = torch.empty(16 * F, device=hist.device, dtype=torch.uint8)
    with timed("gbdt/best_split"):
        N.check(N.lib().rsx_gbdt_best_split(N.ptr(hist), N.ptr(is_cat), N.ptr(n_bins), F, n_leaves, float(l2), N.ptr(ws),
                                            N.ptr(split), N.ptr(score), N.stream()), "gbdt_best_split")
    return split, score


def gbdt_apply_split(bins, leaf, split, is_cat, n_leaves, hist=None, F=None, lr=None, l2=None):
    """leaf = 2 leaf + right in place for the device split (f, b) (int32 [2]) of a level with n_leaves leaves
    (rsx_gbdt_apply_split). With hist (that level's histogram) the level is the tree's last: returns
    (leaf_sums int64 [2 n_leaves, 2], leaf_values fp32 [2 n_leaves]) with value = (float)(lr (G / (H +
    l2))) from the children's exact sums (an empty leaf: 0) and adds value[leaf] to the approximant F [R] in
    place; else returns None. A split feature or leaf index out of range raises IndexError at a later call."""
    nF, R = _gbdt_bins("gbdt_apply_split", bins)
    _gbdt_leaves("gbdt_apply_split", n_leaves)
    _gbdt_rows("gbdt_apply_split", "leaf", leaf, torch.uint8, R, bins)
    _gbdt_rows("gbdt_apply_split", "split", split, torch.int32, 2, bins)
    _gbdt_features("gbdt_apply_split", is_cat, None, nF, bins)
    sums = values = None
    if hist is not None:
        shape = (n_leaves, nF, GBDT_BINS, 2)
        if hist.dtype != torch.int64 or tuple(hist.shape) != shape or not hist.is_contiguous() or hist.device != bins.device:
            raise ValueError(f"gbdt_apply_split: hist must be a contiguous int64 {shape} tensor on {bins.device}")
        if F is None or lr is None or l2 is None:
            raise ValueError("gbdt_apply_split: the last level (hist given) needs F, lr and l2")
        _gbdt_rows("gbdt_apply_split", "F", F, torch.float32, R, bins)
        _gbdt_l2("gbdt_apply_split", l2)
        sums = torch.empty(2 * n_leaves, 2, device=bins.device, dtype=torch.int64)
        values = torch.empty(2 * n_leaves, device=bins.device, dtype=torch.float32)
    flag = torch.zeros(1, device=bins.device, dtype=torch.int32)
    with timed("gbdt/apply_split"):
        N.check(N.lib().rsx_gbdt_apply_split(N.ptr(bins), R, nF, N.ptr(split), N.ptr(is_cat), n_leaves, N.ptr(leaf),
                                             N.ptr(hist), float(lr or 0.0), float(l2 or 0.0), N.ptr(sums), N.ptr(values),
                                             N.ptr(F) if hist is not None else None, N.ptr(flag), N.stream()),
                "gbdt_apply_split")
    _GBDT_GUARD.watch(flag)
    return None if hist is None else (sums, values)


class GBDTScratch:
    """The buffers gbdt_tree reuses from tree to tree (R rows, F features, one device)."""

    def __init__(self, R, F, depth, device):
        self.qg = torch.empty(R, device=device, dtype=torch.int32)
        self.qh = torch.empty(R, device=device, dtype=torch.int32)
        self.leaf = torch.empty(R, device=device, dtype=torch.uint8)
        self.hist = torch.empty(1 << (depth - 1), F, GBDT_BINS, 2, device=device, dtype=torch.int64)
        self.ws = torch.empty(16 * F, device=device, dtype=torch.uint8)
        self.sums = torch.empty(GBDT_LEAF_STRIDE, 2, device=device, dtype=torch.int64)
        self.flag = torch.zeros(1, device=device, dtype=torch.int32)
        self.key = (R, F, depth, torch.device(device))


class GBDTGroupPlan:
    """The group layout the QuerySoftMax kernels read, built once per set of rows from group_id [R] (int32 /
    int64 ids >= 0, the rows of a group anywhere) with torch on the device and one host read (the number of
    groups, with the smallest id in the same copy; ValueError for a negative id): order int64 [R] = the
    stable sort of the rows by id (rows in group order = rows[order]), row_group int32 [R] = the dense
    group index of each row in that order, goff int32 [G + 1] = the groups' offsets, G, R, ws = the
    kernels' workspace."""

    def __init__(self, group_id, device=None):
        g = torch.as_tensor(group_id)
        if g.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"GBDTGroupPlan: group_id must be int32 or int64 (got {g.dtype})")
        if device is None:
            device = g.device if g.is_cuda else torch.device("cuda", torch.cuda.current_device())
        g = g.detach().to(device).reshape(-1).to(torch.int64)
        N.ensure_device(g)
        R = g.numel()
        if not 1 <= R < 2 ** 31:
            raise ValueError(f"GBDTGroupPlan: need 1 <= R < 2^31 rows (got {R})")
        ids, order = torch.sort(g, stable=True)
        head = torch.ones(R, device=g.device, dtype=torch.bool)
        head[1:] = ids[1:] != ids[:-1]
        dense = torch.cumsum(head, 0) - 1
        G, lowest = (int(v) for v in torch.stack([dense[-1] + 1, ids[0]]).tolist())     # the one host read
        if lowest < 0:
            raise ValueError(f"GBDTGroupPlan: group ids must be >= 0 (got {lowest})")
        sizes = torch.zeros(G + 1, device=g.device, dtype=torch.int64)
        sizes.scatter_add_(0, dense + 1, torch.ones_like(dense))      # an integer sum: the same bits every run
        self.order, self.row_group = order, _c(dense.to(torch.int32))
        self.goff = _c(torch.cumsum(sizes, 0).to(torch.int32))
        self.G, self.R, self.device = G, R, g.device
        nws = int(N.lib().rsx_gbdt_grad_query_softmax_workspace_bytes(R, G))
        if nws < 0:
            N.check(1, "gbdt_grad_query_softmax_workspace_bytes")
        self.ws = torch.empty(nws, device=g.device, dtype=torch.uint8)


def _gbdt_plan(fn, plan, R, ref):
    if not isinstance(plan, GBDTGroupPlan):
        raise TypeError(f"{fn}: groups must be a GBDTGroupPlan, got {type(plan).__name__}")
    if plan.R != R or plan.device != ref.device:
        raise ValueError(f"{fn}: the plan was built for {plan.R} rows on {plan.device}, not {R} on {ref.device}")


def gbdt_grad_query_softmax(F, y, plan, out=None):
    """(qg, qh) int32 [R] of the approximant F [R] and the labels y [R] (fp32, device, both in the group
    order of plan: rows[plan.order]) under the QuerySoftMax objective (include/recsys_amd.h): per group the
    exact maximum, Z = the int64 sum of llrint(exp(a - m) 2^32) and S = the positives, then g = t - p, h =
    p (1 - p) in fp32, quantised as gbdt_grad's (rsx_gbdt_grad_query_softmax). The rows of a group without
    a positive get 0. The result does not depend on the order of the rows. out: (qg, qh) to write into."""
    N.ensure_device(F)
    _f32("gbdt_grad_query_softmax", "F", F)
    R = F.numel()
    _gbdt_plan("gbdt_grad_query_softmax", plan, R, F)
    _gbdt_rows("gbdt_grad_query_softmax", "F", F, torch.float32, R, F)
    _gbdt_rows("gbdt_grad_query_softmax", "y", y, torch.float32, R, F)
    qg, qh = out if out is not None else (torch.empty(R, device=F.device, dtype=torch.int32) for _ in range(2))
    _gbdt_rows("gbdt_grad_query_softmax", "qg", qg, torch.int32, R, F)
    _gbdt_rows("gbdt_grad_query_softmax", "qh", qh, torch.int32, R, F)
    with timed("gbdt/grad_query_softmax"):
        N.check(N.lib().rsx_gbdt_grad_query_softmax(N.ptr(F), N.ptr(y), N.ptr(plan.row_group), N.ptr(plan.goff), R, plan.G,
                                                    N.ptr(plan.ws), plan.ws.numel(), N.ptr(qg), N.ptr(qh), N.stream()),
                "gbdt_grad_query_softmax")
    return qg, qh


class QuerySoftMaxEval:
    """What query_softmax_eval returns. The outputs stay on the device until result(): loss_sum (float64)
    and live_groups (int64) are views of one 16-byte allocation, fetched by one copy."""

    def __init__(self, buf):
        self._buf = buf
        self.loss_sum, self.live_groups = buf[:1].view(torch.float64), buf[1:2]

    def result(self):
        """The one host read: {"loss": loss_sum / live_groups (NaN when no group holds a positive),
        "live_groups"}."""
        return self._result(self._buf.cpu())

    @staticmethod
    def _result(host):
        live = int(host[1])
        loss = float(host[:1].view(torch.float64)[0])
        return {"loss": loss / live if live else float("nan"), "live_groups": live}


def query_softmax_eval(F, y, plan):
    """The QuerySoftMax metric of the scores F [R] against the labels y [R] (fp32, device, in the group order
    of plan): the mean over the groups with a positive of L_q = -(1 / S_q) sum_{y_i = 1} log softmax(a)_i, its
    sum formed in fp64 in a fixed order (rsx_query_softmax_eval: the same bits every run), without a host
    synchronisation. Returns a QuerySoftMaxEval; its result() does the one host read."""
    N.ensure_device(F)
    _f32("query_softmax_eval", "F", F)
    R = F.numel()
    _gbdt_plan("query_softmax_eval", plan, R, F)
    _gbdt_rows("query_softmax_eval", "F", F, torch.float32, R, F)
    _gbdt_rows("query_softmax_eval", "y", y, torch.float32, R, F)
    out = QuerySoftMaxEval(torch.empty(2, device=F.device, dtype=torch.int64))
    with timed("query_softmax_eval"):
        N.check(N.lib().rsx_query_softmax_eval(N.ptr(F), N.ptr(y), N.ptr(plan.row_group), N.ptr(plan.goff), R, plan.G,
                                               N.ptr(plan.ws), plan.ws.numel(), N.ptr(out._buf), N.stream()),
                "query_softmax_eval")
    return out


def gbdt_tree(bins, y, Fx, is_cat, n_bins, depth, lr, l2, splits, leaf_values, scratch, groups=None):
    """One whole tree on the approximant Fx [R] (updated in place), enqueued by one native call
    (rsx_gbdt_tree: gradients, then per level histogram, split search and leaf update, the last level with the
    leaf values and the update of Fx; 2 + 4 depth kernels and 1 + depth fills, no host synchronisation).
    Writes splits int32 [>= depth, 2] and leaf_values fp32 [>= 2^depth] (a tree's rows of a GBDTModel).
    scratch: a GBDTScratch(R, F, depth, device); its flag collects range errors (the caller watches it).
    groups: a GBDTGroupPlan of the rows (given in its group order) selects the QuerySoftMax gradients
    (rsx_gbdt_tree_grouped: three kernels and a fill in place of the Logloss gradient kernel)."""
    F, R = _gbdt_bins("gbdt_tree", bins)
    if not 1 <= depth <= GBDT_MAX_DEPTH:
        raise ValueError(f"gbdt_tree: need 1 <= depth <= {GBDT_MAX_DEPTH} (got {depth})")
    _gbdt_rows("gbdt_tree", "y", y, torch.float32, R, bins)
    _gbdt_rows("gbdt_tree", "F", Fx, torch.float32, R, bins)
    _gbdt_features("gbdt_tree", is_cat, n_bins, F, bins)
    _gbdt_l2("gbdt_tree", l2)
    if scratch.key != (R, F, depth, bins.device):
        raise ValueError(f"gbdt_tree: the scratch was sized for {scratch.key}, not {(R, F, depth, bins.device)}")
    if splits.dtype != torch.int32 or splits.numel() < 2 * depth or not splits.is_contiguous() or splits.device != bins.device:
        raise ValueError(f"gbdt_tree: splits must be a contiguous int32 [>= {depth}, 2] tensor on {bins.device}")
    if (leaf_values.dtype != torch.float32 or leaf_values.numel() < (1 << depth) or not leaf_values.is_contiguous()
            or leaf_values.device != bins.device):
        raise ValueError(f"gbdt_tree: leaf_values must be a contiguous fp32 [>= {1 << depth}] tensor on {bins.device}")
    s = scratch
    if groups is not None:
        _gbdt_plan("gbdt_tree", groups, R, bins)
        g = groups
        with timed("gbdt/tree_grouped"):
            N.check(N.lib().rsx_gbdt_tree_grouped(N.ptr(bins), N.ptr(y), N.ptr(g.row_group), N.ptr(g.goff), R, g.G, F,
                                                  N.ptr(is_cat), N.ptr(n_bins), int(depth), float(lr), float(l2), N.ptr(Fx),
                                                  N.ptr(s.qg), N.ptr(s.qh), N.ptr(s.leaf), N.ptr(s.hist), N.ptr(s.ws),
                                                  N.ptr(g.ws), g.ws.numel(), N.ptr(splits), N.ptr(s.sums),
                                                  N.ptr(leaf_values), N.ptr(s.flag), N.stream()), "gbdt_tree_grouped")
        return
    with timed("gbdt/tree"):
        N.check(N.lib().rsx_gbdt_tree(N.ptr(bins), N.ptr(y), R, F, N.ptr(is_cat), N.ptr(n_bins), int(depth), float(lr),
                                      float(l2), N.ptr(Fx), N.ptr(s.qg), N.ptr(s.qh), N.ptr(s.leaf), N.ptr(s.hist),
                                      N.ptr(s.ws), N.ptr(splits), N.ptr(s.sums), N.ptr(leaf_values), N.ptr(s.flag),
                                      N.stream()), "gbdt_tree")


def gbdt_predict(bins, model, ntree_end=None, ntree_begin=0, init=None, out=None):
    """The raw scores [R] (fp32) of the binned rows bins uint8 [F, R] under a GBDTModel: f0 (or init [R], for
    a running sum) plus the leaf values of the trees [ntree_begin, ntree_end) in tree order, added in fp32
    one row per lane (rsx_gbdt_predict), so the result equals the training approximant after the same
    trees bit for bit. ntree_end None: model.n_trees. out may be init."""
    F, R = _gbdt_bins("gbdt_predict", bins)
    end = model.n_trees if ntree_end is None else int(ntree_end)
    begin = int(ntree_begin)
    T = model.splits.shape[0]
    if not 0 <= begin <= end <= T:
        raise ValueError(f"gbdt_predict: need 0 <= ntree_begin <= ntree_end <= {T} (got {begin}, {end})")
    if not 1 <= model.depth <= GBDT_MAX_DEPTH:
        raise ValueError(f"gbdt_predict: need 1 <= depth <= {GBDT_MAX_DEPTH} (got {model.depth})")
    sp, lv = model.splits, model.leaf_values
    if sp.dtype != torch.int32 or tuple(sp.shape[1:]) != (GBDT_MAX_DEPTH, 2) or not sp.is_contiguous() or sp.device != bins.device:
        raise ValueError(f"gbdt_predict: model.splits must be a contiguous int32 [T, {GBDT_MAX_DEPTH}, 2] tensor on {bins.device}")
    if lv.dtype != torch.float32 or tuple(lv.shape) != (T, GBDT_LEAF_STRIDE) or not lv.is_contiguous() or lv.device != bins.device:
        raise ValueError(f"gbdt_predict: model.leaf_values must be a contiguous fp32 [{T}, {GBDT_LEAF_STRIDE}] tensor on "
                         f"{bins.device}")
    _gbdt_features("gbdt_predict", model.is_cat, None, F, bins)
    if init is not None:
        _gbdt_rows("gbdt_predict", "init", init, torch.float32, R, bins)
    if out is None:
        out = torch.empty(R, device=bins.device, dtype=torch.float32)
    else:
        _gbdt_rows("gbdt_predict", "out", out, torch.float32, R, bins)
    with timed("gbdt/predict"):
        N.check(N.lib().rsx_gbdt_predict(N.ptr(bins), R, F, N.ptr(sp), N.ptr(lv), N.ptr(model.is_cat), model.depth, begin,
                                         end, N.ptr(init), model.f0, N.ptr(out), N.stream()), "gbdt_predict")
    return out


def rerank_tabular(cand_ids, cand_scores, user_vectors, item_vectors, item_price, user_avg_price):
    """The FeatureEngineer numeric columns of the candidates cand_ids [Q, K] (item ids) with their retrieval
    scores cand_scores [Q, K]: (feats fp32 [7, Q K] in the order RERANK_TABULAR_COLUMNS, ids int64 [Q K]) on
    rsx_rerank_tabular, one wave per candidate. user_vectors [Q, d], item_vectors [N, d], item_price [N],
    user_avg_price [Q], all fp32 on the device. vec_prod_std is the population standard deviation (np.std);
    price_diff_ratio is 0 where user_avg_price is not positive. An id outside [0, N) reads item 0 (ids holds
    the ids used) and raises IndexError at a later call."""
    N.ensure_device(cand_ids)
    if cand_ids.dim() != 2:
        raise ValueError(f"rerank_tabular: cand_ids must be [Q, K], got shape {tuple(cand_ids.shape)}")
    Q, K = cand_ids.shape
    if Q < 1 or K < 1 or Q * K >= 2 ** 31:
        raise ValueError(f"rerank_tabular: need Q, K >= 1 and Q K < 2^31 (got {Q}, {K})")
    cand = _c(_index("rerank_tabular", "cand_ids", cand_ids))
    _f32("rerank_tabular", "cand_scores", cand_scores, cand)
    if cand_scores.shape != cand_ids.shape:
        raise ValueError(f"rerank_tabular: cand_scores has shape {tuple(cand_scores.shape)}, cand_ids {tuple(cand_ids.shape)}")
    d = _rows2("rerank_tabular", "user_vectors", user_vectors)
    if _rows2("rerank_tabular", "item_vectors", item_vectors) != d or user_vectors.shape[0] != Q:
        raise ValueError(f"rerank_tabular: need user_vectors [{Q}, d] and item_vectors [N, d] (got "
                         f"{tuple(user_vectors.shape)} and {tuple(item_vectors.shape)})")
    n_items = item_vectors.shape[0]
    if n_items < 1 or d < 1:
        raise ValueError("rerank_tabular: item_vectors is empty")
    for name, t in (("user_vectors", user_vectors), ("item_vectors", item_vectors)):
        if t.device != cand.device:
            raise RuntimeError(f"rerank_tabular: {name} is on {t.device}, expected {cand.device}")
    _f32_vec("rerank_tabular", "item_price", item_price, n_items, cand)
    _f32_vec("rerank_tabular", "user_avg_price", user_avg_price, Q, cand)
    R = Q * K
    feats = torch.empty(len(RERANK_TABULAR_COLUMNS), R, device=cand.device, dtype=torch.float32)
    ids = torch.empty(R, device=cand.device, dtype=torch.int64)
    flag = torch.zeros(1, device=cand.device, dtype=torch.int32)
    with timed("gbdt/rerank_tabular"):
        N.check(N.lib().rsx_rerank_tabular(N.ptr(cand), N.ptr(_c(cand_scores)), N.ptr(_c(user_vectors)),
                                           N.ptr(_c(item_vectors)), N.ptr(_c(item_price)), N.ptr(_c(user_avg_price)), Q, K,
                                           n_items, d, N.ptr(feats), N.ptr(ids), N.ptr(flag), N.stream()), "rerank_tabular")
    _RERANK_GUARD.watch(flag, n_items)
    return feats, ids


# ----------------------------------------------------------------------------------------
# A19 ordered target statistics of wide categorical columns (csrc/gbdt_ts.hip; include/recsys_amd.h, "ordered
# target statistics")
GBDT_TS_MAX_CODES = 1 << 22
_GBDT_TS_TILE = 256
_GBDT_TS_GUARD = IdRangeGuard("gbdt_ordered_ts: a code outside [0, V] or an order entry outside [0, R)")


def _gbdt_ts_codes(fn, codes):
    """codes is a contiguous int32 [Fts, R] device matrix, Fts <= 32, 1 <= R < 2^31; returns (Fts, R)."""
    N.ensure_device(codes)
    if codes.dtype != torch.int32:
        raise TypeError(f"{fn}: codes must be int32, got {codes.dtype}")
    if codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError(f"{fn}: codes must be a contiguous [Fts, R] matrix, got shape {tuple(codes.shape)}")
    Fts, R = codes.shape
    if not (1 <= Fts <= GBDT_MAX_FEATURES and 1 <= R < 2 ** 31):
        raise ValueError(f"{fn}: need 1 <= Fts <= {GBDT_MAX_FEATURES} and 1 <= R < 2^31 (got Fts {Fts}, R {R})")
    return Fts, R


def gbdt_ts_plan(codes, seed=0):
    """The order the ordered target statistics of codes int32 [Fts, R] run along: order int64 [Fts, R], per
    column the rows by code and inside a code by (hash_u32(seed + column, row), row). rsx_gbdt_ts_keys writes the
    keys code << 32 | hash and a stable torch.sort gives the order (ties fall to the row index). No host read."""
    Fts, R = _gbdt_ts_codes("gbdt_ts_plan", codes)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64 - GBDT_MAX_FEATURES:
        raise ValueError(f"gbdt_ts_plan: seed must be in [0, 2^64 - {GBDT_MAX_FEATURES}) (got {seed})")
    keys = torch.empty(Fts, R, device=codes.device, dtype=torch.int64)
    with timed("gbdt/ts_keys"):
        N.check(N.lib().rsx_gbdt_ts_keys(N.ptr(codes), R, Fts, seed, N.ptr(keys), N.stream()), "gbdt_ts_keys")
    return torch.sort(keys, dim=1, stable=True).indices


def gbdt_ordered_ts(codes, order, y, V, prior=(0.5, 1.0)):
    """Ordered target statistics (rsx_gbdt_ordered_ts) of the TS columns codes int32 [Fts, R] with the labels y
    fp32 [R] in {0, 1} along order int64 [Fts, R] (gbdt_ts_plan): (ts fp32 [Fts, R] in the caller's row order,
    totals int32 [Fts, Vmax + 1, 2] = (N_c, S_c), table fp32 [Fts, Vmax + 1]), Vmax = max(V). V: the largest
    code of each column (host ints, <= GBDT_TS_MAX_CODES); prior = (p, a): ts_i = (s_i + a p) / (n_i + a) over
    the rows of the same code that precede row i, table[c] = (S_c + a p) / (N_c + a). Integer sums: the same
    bits every call. A code outside [0, V] or an order entry outside [0, R) gives the prior value, no access
    leaves its array, and IndexError is raised at a later call (_GBDT_TS_GUARD.check())."""
    fn = "gbdt_ordered_ts"
    Fts, R = _gbdt_ts_codes(fn, codes)
    if order.dtype != torch.int64 or tuple(order.shape) != (Fts, R) or not order.is_contiguous() or order.device != codes.device:
        raise ValueError(f"{fn}: order must be a contiguous int64 [{Fts}, {R}] matrix on {codes.device}")
    _gbdt_rows(fn, "y", y, torch.float32, R, codes)
    V = [int(v) for v in V]
    if len(V) != Fts or min(V) < 0:
        raise ValueError(f"{fn}: V must hold {Fts} largest codes >= 0 (got {V})")
    Vmax = max(V)
    if Vmax > GBDT_TS_MAX_CODES:
        raise ValueError(f"{fn}: a target-statistic column has at most {GBDT_TS_MAX_CODES} known values (got {Vmax})")
    p, a = float(prior[0]), float(prior[1])
    if not (a > 0 and math.isfinite(a) and 0.0 <= p <= 1.0):
        raise ValueError(f"{fn}: prior must be (p in [0, 1], a > 0) (got {prior})")
    dev = codes.device
    Vd = torch.tensor(V, dtype=torch.int32, device=dev)
    ts = torch.empty(Fts, R, device=dev, dtype=torch.float32)
    totals = torch.empty(Fts, Vmax + 1, 2, device=dev, dtype=torch.int32)
    table = torch.empty(Fts, Vmax + 1, device=dev, dtype=torch.float32)
    ws = torch.empty(16 * Fts * ((R + _GBDT_TS_TILE - 1) // _GBDT_TS_TILE), device=dev, dtype=torch.uint8)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("gbdt/ordered_ts"):
        N.check(N.lib().rsx_gbdt_ordered_ts(N.ptr(codes), N.ptr(order), N.ptr(y), N.ptr(Vd), R, Fts, Vmax, a * p, a,
                                            N.ptr(ws), ws.numel(), N.ptr(ts), N.ptr(totals), N.ptr(table), N.ptr(flag),
                                            N.stream()), fn)
    _GBDT_TS_GUARD.watch(flag)
    return ts, totals, table


# ----------------------------------------------------------------------------------------
# A22 explaining the boosted ranker (csrc/gbdt_explain.hip; include/recsys_amd.h, "explaining the boosted ranker")
GBDT_TABLE_STRIDE = 729     # 3^6 states {0, 1, *} per level of a tree


class GBDTExplainPlan:
    """What gbdt_explain_plan returns, on the model's device: table float64 [T, 729] (a tree's conditional values
    E(s), the first 3^depth entries used), pvc float64 [T, 6] (PredictionValuesChange per level), depth and
    n_trees, the trees it covers."""

    def __init__(self, table, pvc, depth, n_trees):
        self.table, self.pvc, self.depth, self.n_trees = table, pvc, int(depth), int(n_trees)


def _gbdt_trees(fn, model, ntree_end, dev):
    """The checks of a GBDTModel that gbdt_predict makes (splits, leaf_values, depth, the tree count); returns
    (T, end)."""
    T = model.splits.shape[0]
    end = model.n_trees if ntree_end is None else int(ntree_end)
    if not 0 <= end <= T:
        raise ValueError(f"{fn}: need 0 <= ntree_end <= {T} (got {end})")
    if not 1 <= model.depth <= GBDT_MAX_DEPTH:
        raise ValueError(f"{fn}: need 1 <= depth <= {GBDT_MAX_DEPTH} (got {model.depth})")
    sp, lv = model.splits, model.leaf_values
    if sp.dtype != torch.int32 or tuple(sp.shape[1:]) != (GBDT_MAX_DEPTH, 2) or not sp.is_contiguous() or sp.device != dev:
        raise ValueError(f"{fn}: model.splits must be a contiguous int32 [T, {GBDT_MAX_DEPTH}, 2] tensor on {dev}")
    if lv.dtype != torch.float32 or tuple(lv.shape) != (T, GBDT_LEAF_STRIDE) or not lv.is_contiguous() or lv.device != dev:
        raise ValueError(f"{fn}: model.leaf_values must be a contiguous fp32 [{T}, {GBDT_LEAF_STRIDE}] tensor on {dev}")
    return T, end


def _gbdt_weights(fn, weights, end, dev):
    """weights is a contiguous int64 [>= end, 64] tensor on dev: a row per tree in use."""
    if weights.dtype != torch.int64:
        raise TypeError(f"{fn}: weights must be int64, got {weights.dtype}")
    if (weights.dim() != 2 or weights.shape[0] < end or weights.shape[1] != GBDT_LEAF_STRIDE or not weights.is_contiguous()
            or weights.device != dev):
        raise ValueError(f"{fn}: weights must be a contiguous int64 [>= {end}, {GBDT_LEAF_STRIDE}] tensor on {dev}, got "
                         f"{tuple(weights.shape)} on {weights.device}")


def gbdt_leaf_weights(bins, model, ntree_end=None, out=None):
    """The leaf weights int64 [T, 64] of a GBDTModel over the binned rows bins uint8 [F, R]: out[t][l] = the number
    of rows that reach leaf l of tree t (rsx_gbdt_leaf_weights: LDS and global integer atomics, the same bits every
    run and in any row order), for the first ntree_end trees (default: model.n_trees); the other rows of a fresh
    out are 0, those of a given out (int64 [>= ntree_end, 64]) are left as they are. No host read."""
    F, R = _gbdt_bins("gbdt_leaf_weights", bins)
    T, end = _gbdt_trees("gbdt_leaf_weights", model, ntree_end, bins.device)
    _gbdt_features("gbdt_leaf_weights", model.is_cat, None, F, bins)
    if out is None:
        out = torch.zeros(T, GBDT_LEAF_STRIDE, device=bins.device, dtype=torch.int64)
    else:
        _gbdt_weights("gbdt_leaf_weights", out, end, bins.device)
    with timed("gbdt/leaf_weights"):
        N.check(N.lib().rsx_gbdt_leaf_weights(N.ptr(bins), R, F, N.ptr(model.splits), N.ptr(model.is_cat), model.depth, 0,
                                              end, N.ptr(out), N.stream()), "gbdt_leaf_weights")
    return out


def gbdt_explain_plan(model, weights, ntree_end=None):
    """The GBDTExplainPlan of the first ntree_end trees (default: model.n_trees) of a GBDTModel under the leaf
    weights int64 [>= ntree_end, 64] (gbdt_leaf_weights): per tree the table of the conditional values E(s) and the
    PredictionValuesChange of every level (rsx_gbdt_explain_plan, one workgroup per tree). The rows of the other
    trees are 0. No host read."""
    N.ensure_device(weights)
    dev = weights.device
    T, end = _gbdt_trees("gbdt_explain_plan", model, ntree_end, dev)
    _gbdt_weights("gbdt_explain_plan", weights, end, dev)
    table = torch.zeros(T, GBDT_TABLE_STRIDE, device=dev, dtype=torch.float64)
    pvc = torch.zeros(T, GBDT_MAX_DEPTH, device=dev, dtype=torch.float64)
    with timed("gbdt/explain_plan"):
        N.check(N.lib().rsx_gbdt_explain_plan(N.ptr(model.splits), N.ptr(model.leaf_values), N.ptr(weights), model.depth, 0,
                                              end, N.ptr(table), N.ptr(pvc), N.stream()), "gbdt_explain_plan")
    return GBDTExplainPlan(table, pvc, model.depth, end)


def gbdt_shap(bins, model, plan, ntree_end=None, out=None):
    """The exact path-dependent Shapley values float64 [F + 1, R] of the binned rows bins uint8 [F, R] under the
    first ntree_end trees (default: plan.n_trees; at most that) of a GBDTModel: row j < F is feature j's, row F
    the expected value f0 + sum_t E_t(*, ..., *), and a row's F + 1 entries sum to its raw score
    (rsx_gbdt_shap: one row per lane, every sum in tree order, so the bits depend neither on R nor on the grid).
    plan: the model's GBDTExplainPlan. No host read."""
    F, R = _gbdt_bins("gbdt_shap", bins)
    if not isinstance(plan, GBDTExplainPlan):
        raise TypeError(f"gbdt_shap: plan must be a GBDTExplainPlan, got {type(plan).__name__}")
    T, end = _gbdt_trees("gbdt_shap", model, plan.n_trees if ntree_end is None else ntree_end, bins.device)
    if end > plan.n_trees or plan.depth != model.depth:
        raise ValueError(f"gbdt_shap: the plan covers {plan.n_trees} trees of depth {plan.depth}, asked for {end} of depth "
                         f"{model.depth}")
    tb = plan.table
    if tb.dtype != torch.float64 or tuple(tb.shape) != (T, GBDT_TABLE_STRIDE) or not tb.is_contiguous() or tb.device != bins.device:
        raise ValueError(f"gbdt_shap: plan.table must be a contiguous float64 [{T}, {GBDT_TABLE_STRIDE}] tensor on {bins.device}")
    _gbdt_features("gbdt_shap", model.is_cat, None, F, bins)
    if out is None:
        out = torch.empty(F + 1, R, device=bins.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (F + 1, R) or not out.is_contiguous() or out.device != bins.device:
        raise ValueError(f"gbdt_shap: out must be a contiguous float64 [{F + 1}, {R}] tensor on {bins.device}")
    with timed("gbdt/shap"):
        N.check(N.lib().rsx_gbdt_shap(N.ptr(bins), R, F, N.ptr(model.splits), N.ptr(model.is_cat), model.depth, 0, end,
                                      N.ptr(tb), model.f0, N.ptr(out), N.stream()), "gbdt_shap")
    return out


# ----------------------------------------------------------------------------------------
# A18 the ranker's training rows (csrc/ranker_rows.hip; include/recsys_amd.h, "ranker training rows")
_RANKER_ROWS_GUARD = IdRangeGuard("ranker_sample_rows: a positive's user or item, a bought list, or a customer who "
                                  "bought every item (nothing to draw a negative from)")
_PAIR_GUARD = IdRangeGuard("pair_tabular row users or items")


def _i32_rows(fn, name, t, ref=None, n=None):
    """t is a 1-D int32 tensor (on ref's device, of n elements); returned contiguous."""
    if t.dtype != torch.int32:
        raise TypeError(f"{fn}: {name} must be int32, got {t.dtype}")
    if ref is not None and t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")
    if t.dim() != 1 or (n is not None and t.numel() != n):
        want = "" if n is None else f" of {n} elements"
        raise ValueError(f"{fn}: {name} must be a vector{want}, got shape {tuple(t.shape)}")
    return _c(t)


def ranker_sample_rows(pos_user, pos_item, bought_off, bought, n_items, negative_ratio, seed):
    """HMLogImporter's rows (utils/monitor/log_importer.py:59-84) on rsx_ranker_rows_sample: for the valid
    positives pos_user, pos_item int32 [Pv] in order, (row_user int32, row_item int32, y fp32), each
    [Pv (K + 1)] with K = negative_ratio >= 0: positive p with y = 1, then its K negatives with y = 0, each
    drawn uniformly (bias <= M / 2^32) among the M = n_items - D items customer pos_user[p] has not bought.
    The customers' distinct bought items are the CSR of first_hit: bought_off int64 [C + 1], bought int32
    ascending and distinct per customer. Negative (p, k) is a function of (seed, p K + k) alone (no rejection
    loop: the specification is in include/recsys_amd.h). A customer with M <= 0, a positive outside [0, C) x
    [0, n_items) or a malformed bought list raises IndexError at a later call (_RANKER_ROWS_GUARD.check())."""
    fn = "ranker_sample_rows"
    N.ensure_device(pos_user)
    pos_user = _i32_rows(fn, "pos_user", pos_user)
    Pv = pos_user.numel()
    pos_item = _i32_rows(fn, "pos_item", pos_item, pos_user, Pv)
    K, n_items, seed = int(negative_ratio), int(n_items), int(seed)
    if K < 0:
        raise ValueError(f"{fn}: negative_ratio must be >= 0 (got {K})")
    if not 1 <= n_items < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= n_items < 2^31 (got {n_items})")
    if Pv < 1 or Pv * (K + 1) >= 2 ** 31:
        raise ValueError(f"{fn}: need Pv >= 1 and Pv (negative_ratio + 1) < 2^31 (got {Pv}, {K})")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{fn}: seed must be in [0, 2^64) (got {seed})")
    if bought_off.dim() != 1 or bought_off.numel() < 2:
        raise ValueError(f"{fn}: bought_off must hold C + 1 >= 2 offsets, got shape {tuple(bought_off.shape)}")
    C = bought_off.numel() - 1
    bought_off, bought = _truth_csr(fn, bought_off, bought, C, pos_user)
    if bought.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: bought holds {bought.numel()} >= 2^31 entries")
    R = Pv * (K + 1)
    dev = pos_user.device
    row_user = torch.empty(R, device=dev, dtype=torch.int32)
    row_item = torch.empty(R, device=dev, dtype=torch.int32)
    y = torch.empty(R, device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("gbdt/ranker_sample_rows"):
        N.check(N.lib().rsx_ranker_rows_sample(N.ptr(pos_user), N.ptr(pos_item), Pv, N.ptr(bought_off), N.ptr(bought),
                                               bought.numel(), C, n_items, K, seed, N.ptr(row_user), N.ptr(row_item),
                                               N.ptr(y), N.ptr(flag), N.stream()), fn)
    _RANKER_ROWS_GUARD.watch(flag)
    return row_user, row_item, y


def pair_tabular(row_user, row_item, score, user_vectors, item_vectors, item_price, user_avg_price, truth_off=None,
                 truth=None):
    """The FeatureEngineer numeric columns of the rows (row_user[r], row_item[r]), int32 [R]: feats fp32 [7, R]
    in the order RERANK_TABULAR_COLUMNS on rsx_pair_tabular, one wave per row. user_vectors [C, d],
    item_vectors [N, d], item_price [N], user_avg_price [C], all fp32 on the device. Columns 1..6 have the bits
    rerank_tabular gives the same pair (one device function); column 0 is score [R] fp32, or with score None
    the fp32 dot product of the pair's vectors. With truth_off int64 [C + 1] and truth int32 (the CSR of
    first_hit) the result is (feats, y): y fp32 [R] = 1 where the row's item is in its user's truth set. A
    user outside [0, C) or an item outside [0, N) reads row 0 and raises IndexError at a later call."""
    fn = "pair_tabular"
    N.ensure_device(row_user)
    row_user = _i32_rows(fn, "row_user", row_user)
    R = row_user.numel()
    row_item = _i32_rows(fn, "row_item", row_item, row_user, R)
    if not 1 <= R < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= R < 2^31 rows (got {R})")
    if score is not None:
        _f32(fn, "score", score, row_user)
        if score.dim() != 1 or score.numel() != R:
            raise ValueError(f"{fn}: score must be a vector of {R} elements, got shape {tuple(score.shape)}")
    d = _rows2(fn, "user_vectors", user_vectors)
    if _rows2(fn, "item_vectors", item_vectors) != d:
        raise ValueError(f"{fn}: need user_vectors [C, d] and item_vectors [N, d] (got {tuple(user_vectors.shape)} and "
                         f"{tuple(item_vectors.shape)})")
    C, n_items = user_vectors.shape[0], item_vectors.shape[0]
    if C < 1 or n_items < 1 or not 1 <= d <= 65536:
        raise ValueError(f"{fn}: need C, N >= 1 and 1 <= d <= 65536 (got {C}, {n_items}, {d})")
    for name, t in (("user_vectors", user_vectors), ("item_vectors", item_vectors)):
        if t.device != row_user.device:
            raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {row_user.device}")
    if item_price is None or user_avg_price is None:
        raise ValueError(f"{fn}: item_price and user_avg_price are needed")
    _f32_vec(fn, "item_price", item_price, n_items, row_user)
    _f32_vec(fn, "user_avg_price", user_avg_price, C, row_user)
    if (truth_off is None) != (truth is None):
        raise ValueError(f"{fn}: truth_off and truth come together")
    y = None
    if truth is not None:
        truth_off, truth = _truth_csr(fn, truth_off, truth, C, row_user)
        if truth.numel() >= 2 ** 31:
            raise ValueError(f"{fn}: truth holds {truth.numel()} >= 2^31 entries")
        y = torch.empty(R, device=row_user.device, dtype=torch.float32)
    feats = torch.empty(len(RERANK_TABULAR_COLUMNS), R, device=row_user.device, dtype=torch.float32)
    flag = torch.zeros(1, device=row_user.device, dtype=torch.int32)
    with timed("gbdt/pair_tabular"):
        N.check(N.lib().rsx_pair_tabular(N.ptr(row_user), N.ptr(row_item), N.ptr(_c(score)), N.ptr(_c(user_vectors)),
                                         N.ptr(_c(item_vectors)), N.ptr(_c(item_price)), N.ptr(_c(user_avg_price)), R, C,
                                         n_items, d, N.ptr(truth_off), N.ptr(truth), 0 if truth is None else truth.numel(),
                                         N.ptr(feats), N.ptr(y), N.ptr(flag), N.stream()), fn)
    _PAIR_GUARD.watch(flag)
    return feats if y is None else (feats, y)


# ----------------------------------------------------------------------------------------
# A20 the towers' feature frames from the transaction log (csrc/tx_features.hip; include/recsys_amd.h, "transaction
# features"). The table is sorted by (customer, day): item, day int32 [T], price fp32 [T], channel uint8 [T].
TX_ITEM_COLUMNS = ("raw_probability", "pop_1w_log", "pop_1m_log", "velocity_1w", "velocity_1m", "steady_score_log",
                   "avg_item_price_log", "days_since_release_log")
TX_USER_COLUMNS = ("price_std", "last_price_diff", "repurchase_ratio", "weekend_ratio", "price_std_scaled",
                   "last_price_diff_scaled", "repurchase_ratio_scaled", "weekend_ratio_scaled", "user_avg_price_log",
                   "total_cnt_log", "recency_log")
TX_USER_F64 = ("user_avg_price", "total_cnt", "recency_days")
TX_COLD_DAYS = 14
TX_MAX_QUANTILES = 126
_TX_CALENDAR_GUARD = IdRangeGuard("tx_calendar: a negative day")
_TX_ROWS_GUARD = IdRangeGuard("tx_segment_rows: offsets that do not run from 0 to T without decreasing")
_TX_STATS_GUARD = IdRangeGuard("tx_segment_stats: a row_seg that decreases or has an entry >= S, or a perm entry outside "
                               "[0, T)")
_TX_DISTINCT_GUARD = IdRangeGuard("tx_segment_distinct: a value column that decreases inside a segment, or a row_seg "
                                  "that decreases or has an entry >= S")
_TX_WEEKLY_GUARD = IdRangeGuard("tx_weekly_sales: an item outside [0, N) or a week that is not a column")
_TX_SEQ_GUARD = IdRangeGuard("tx_sequences: an item outside [0, N), or a row_seg that decreases or has an entry >= C")


def _tx_rows(fn, t, name="row_seg"):
    """t is a contiguous int32 device vector of 1 <= T < 2^31 rows; returns T."""
    N.ensure_device(t)
    T = t.numel()
    if not 1 <= T < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= T < 2^31 rows (got {T})")
    _gbdt_rows(fn, name, t, torch.int32, T, t)
    return T


def _tx_count(fn, name, n):
    n = int(n)
    if not 1 <= n < 2 ** 31 - 1:
        raise ValueError(f"{fn}: need 1 <= {name} < 2^31 - 1 (got {n})")
    return n


def _tx_ws(T, dev):
    return torch.empty(N.lib().rsx_tx_workspace_bytes(T), device=dev, dtype=torch.uint8)


def tx_calendar(day):
    """day int32 [T], days since 1970-01-01 -> (weekend uint8, month int32 = 12 year + month - 1, week int32 =
    floor((day + 3) / 7), Monday-start weeks). A negative day counts as 0 and raises IndexError at a later call
    (_TX_CALENDAR_GUARD.check())."""
    fn = "tx_calendar"
    T = _tx_rows(fn, day, "day")
    dev = day.device
    weekend = torch.empty(T, device=dev, dtype=torch.uint8)
    month = torch.empty(T, device=dev, dtype=torch.int32)
    week = torch.empty(T, device=dev, dtype=torch.int32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/calendar"):
        N.check(N.lib().rsx_tx_calendar(N.ptr(day), T, N.ptr(weekend), N.ptr(month), N.ptr(week), N.ptr(flag),
                                        N.stream()), fn)
    _TX_CALENDAR_GUARD.watch(flag)
    return weekend, month, week


def tx_segment_rows(seg_off, T):
    """seg_off int64 [S + 1] (device) over T rows -> row_seg int32 [T], the segment of every row (-1: none). Offsets
    are clamped to [0, T]; malformed ones raise IndexError at a later call (_TX_ROWS_GUARD.check())."""
    fn = "tx_segment_rows"
    N.ensure_device(seg_off)
    T = int(T)
    if not 1 <= T < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= T < 2^31 rows (got {T})")
    if seg_off.dim() != 1 or seg_off.numel() < 2:
        raise ValueError(f"{fn}: seg_off must hold S + 1 >= 2 offsets, got shape {tuple(seg_off.shape)}")
    S = _tx_count(fn, "S", seg_off.numel() - 1)
    _gbdt_rows(fn, "seg_off", seg_off, torch.int64, S + 1, seg_off)
    dev = seg_off.device
    row_seg = torch.empty(T, device=dev, dtype=torch.int32)
    ws = _tx_ws(T, dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/segment_rows"):
        N.check(N.lib().rsx_tx_segment_rows(N.ptr(seg_off), S, T, N.ptr(ws), ws.numel(), N.ptr(row_seg), N.ptr(flag),
                                            N.stream()), fn)
    _TX_ROWS_GUARD.watch(flag)
    return row_seg


def tx_segment_stats(row_seg, S, price, day, channel, weekend, perm=None):
    """Per segment of row_seg int32 [T] (tx_segment_rows, or a sorted column) over the table columns price fp32,
    day int32, channel uint8, weekend uint8 [T] (read through perm int64 [T] when given: sorted position -> table
    row): a dict of count int32, sum fp64, m2 fp64 = sum (price - sum / count)^2, last fp32, dmin, dmax int32, chan
    int64, wkend int32, each [S]. Fixed combination order: the same bits every call."""
    fn = "tx_segment_stats"
    T = _tx_rows(fn, row_seg)
    S = _tx_count(fn, "S", S)
    _gbdt_rows(fn, "price", price, torch.float32, T, row_seg)
    _gbdt_rows(fn, "day", day, torch.int32, T, row_seg)
    _gbdt_rows(fn, "channel", channel, torch.uint8, T, row_seg)
    _gbdt_rows(fn, "weekend", weekend, torch.uint8, T, row_seg)
    if perm is not None:
        _gbdt_rows(fn, "perm", perm, torch.int64, T, row_seg)
    dev = row_seg.device
    out = {"count": torch.empty(S, device=dev, dtype=torch.int32), "sum": torch.empty(S, device=dev, dtype=torch.float64),
           "m2": torch.empty(S, device=dev, dtype=torch.float64), "last": torch.empty(S, device=dev, dtype=torch.float32),
           "dmin": torch.empty(S, device=dev, dtype=torch.int32), "dmax": torch.empty(S, device=dev, dtype=torch.int32),
           "chan": torch.empty(S, device=dev, dtype=torch.int64), "wkend": torch.empty(S, device=dev, dtype=torch.int32)}
    ws = _tx_ws(T, dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/segment_stats"):
        N.check(N.lib().rsx_tx_segment_stats(N.ptr(row_seg), S, T, N.ptr(perm), N.ptr(price), N.ptr(day), N.ptr(channel),
                                             N.ptr(weekend), N.ptr(ws), ws.numel(), N.ptr(out["count"]), N.ptr(out["sum"]),
                                             N.ptr(out["m2"]), N.ptr(out["last"]), N.ptr(out["dmin"]), N.ptr(out["dmax"]),
                                             N.ptr(out["chan"]), N.ptr(out["wkend"]), N.ptr(flag), N.stream()), fn)
    _TX_STATS_GUARD.watch(flag)
    return out


def tx_segment_distinct(row_seg, S, val):
    """The number of distinct values of val int32 [T] per segment of row_seg, int32 [S]; val is non-decreasing
    inside every segment (a decreasing pair raises IndexError at a later call, _TX_DISTINCT_GUARD.check())."""
    fn = "tx_segment_distinct"
    T = _tx_rows(fn, row_seg)
    S = _tx_count(fn, "S", S)
    _gbdt_rows(fn, "val", val, torch.int32, T, row_seg)
    dev = row_seg.device
    out = torch.empty(S, device=dev, dtype=torch.int32)
    ws = _tx_ws(T, dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/segment_distinct"):
        N.check(N.lib().rsx_tx_segment_distinct(N.ptr(row_seg), S, T, N.ptr(val), N.ptr(ws), ws.numel(), N.ptr(out),
                                                N.ptr(flag), N.stream()), fn)
    _TX_DISTINCT_GUARD.watch(flag)
    return out


def _tx_grid(fn, n_items, W):
    n_items, W = int(n_items), int(W)
    if not (1 <= W <= 65536 and n_items >= 1 and n_items * W < 2 ** 31):
        raise ValueError(f"{fn}: need 1 <= W <= 65536 weeks, N >= 1 items and N W < 2^31 (got N {n_items}, W {W})")
    return n_items, W


def tx_weekly_sales(item, week, n_items, weeks=None):
    """(weekly int32 [N, W], weeks int32 [W]): weekly[i, j] = the rows of item i in week weeks[j]; weeks = the
    distinct values of week ascending (torch.unique: one host read for W) unless given. The reference's
    groupby([article_id, week_start]).size().unstack(fill_value=0).sort_index(axis=1)."""
    fn = "tx_weekly_sales"
    T = _tx_rows(fn, item, "item")
    _gbdt_rows(fn, "week", week, torch.int32, T, item)
    if weeks is None:
        weeks = torch.unique(week)
    n_items, W = _tx_grid(fn, n_items, weeks.numel())
    _gbdt_rows(fn, "weeks", weeks, torch.int32, W, item)
    weekly = torch.empty(n_items, W, device=item.device, dtype=torch.int32)
    flag = torch.zeros(1, device=item.device, dtype=torch.int32)
    with timed("tx/weekly_sales"):
        N.check(N.lib().rsx_tx_weekly_sales(N.ptr(item), N.ptr(week), T, N.ptr(weeks), W, n_items, N.ptr(weekly),
                                            N.ptr(flag), N.stream()), fn)
    _TX_WEEKLY_GUARD.watch(flag, n_items)
    return weekly, weeks


def tx_item_features(weekly, count, price_sum, dmin, n_rows, max_day, cold_days=TX_COLD_DAYS):
    """The eight item columns TX_ITEM_COLUMNS, fp32 [8, N], from weekly int32 [N, W] and the per-item count int32,
    price_sum fp64 and dmin int32 [N] (tx_segment_stats over a by-item order), the number of rows T and the
    largest day; the cold-start imputation included. Evaluated in fp64, rounded once."""
    fn = "tx_item_features"
    N.ensure_device(weekly)
    if weekly.dtype != torch.int32 or weekly.dim() != 2 or not weekly.is_contiguous():
        raise ValueError(f"{fn}: weekly must be a contiguous int32 [N, W] matrix")
    n_items, W = _tx_grid(fn, *weekly.shape)
    _gbdt_rows(fn, "count", count, torch.int32, n_items, weekly)
    _gbdt_rows(fn, "price_sum", price_sum, torch.float64, n_items, weekly)
    _gbdt_rows(fn, "dmin", dmin, torch.int32, n_items, weekly)
    n_rows, max_day, cold_days = int(n_rows), int(max_day), int(cold_days)
    if not 1 <= n_rows < 2 ** 31 or not 0 <= max_day < 2 ** 31 or cold_days < 0:
        raise ValueError(f"{fn}: need 1 <= T < 2^31, 0 <= max_day < 2^31 and cold_days >= 0")
    out = torch.empty(len(TX_ITEM_COLUMNS), n_items, device=weekly.device, dtype=torch.float32)
    col_sum = torch.empty(4 + 4 * ((n_items + 4095) // 4096), device=weekly.device, dtype=torch.float64)
    with timed("tx/item_features"):
        N.check(N.lib().rsx_tx_item_features(N.ptr(weekly), n_items, W, N.ptr(count), N.ptr(price_sum), N.ptr(dmin), n_rows,
                                             max_day, cold_days, N.ptr(col_sum), col_sum.numel(), N.ptr(out), N.stream()), fn)
    return out


def tx_user_features(stats, uniq, months, max_day):
    """The user columns from the per-customer stats (tx_segment_stats), uniq and months int32 [C] (the distinct items
    and months, tx_segment_distinct) and the largest day: (f64 fp64 [3, C] in the order TX_USER_F64, cols fp32
    [11, C] in the order TX_USER_COLUMNS, preferred_channel int8 [C], active_months int16 [C])."""
    fn = "tx_user_features"
    count = stats["count"]
    N.ensure_device(count)
    C = _tx_count(fn, "C", count.numel())
    for name, dt in (("count", torch.int32), ("sum", torch.float64), ("m2", torch.float64), ("last", torch.float32),
                     ("dmax", torch.int32), ("chan", torch.int64), ("wkend", torch.int32)):
        _gbdt_rows(fn, name, stats[name], dt, C, count)
    _gbdt_rows(fn, "uniq", uniq, torch.int32, C, count)
    _gbdt_rows(fn, "months", months, torch.int32, C, count)
    max_day = int(max_day)
    if not 0 <= max_day < 2 ** 31:
        raise ValueError(f"{fn}: need 0 <= max_day < 2^31 (got {max_day})")
    dev = count.device
    f64 = torch.empty(len(TX_USER_F64), C, device=dev, dtype=torch.float64)
    cols = torch.empty(len(TX_USER_COLUMNS), C, device=dev, dtype=torch.float32)
    channel = torch.empty(C, device=dev, dtype=torch.int8)
    active = torch.empty(C, device=dev, dtype=torch.int16)
    ws = torch.empty(4 * C + 8 + 4 * ((C + 4095) // 4096), device=dev, dtype=torch.float64)
    with timed("tx/user_features"):
        N.check(N.lib().rsx_tx_user_features(N.ptr(count), N.ptr(stats["sum"]), N.ptr(stats["m2"]), N.ptr(stats["last"]),
                                             N.ptr(stats["dmax"]), N.ptr(stats["chan"]), N.ptr(stats["wkend"]), N.ptr(uniq),
                                             N.ptr(months), C, max_day, N.ptr(ws), ws.numel() * 8, N.ptr(f64), N.ptr(cols),
                                             N.ptr(channel), N.ptr(active), N.stream()), fn)
    return f64, cols, channel, active


def quantile_bucket(x, q=10, return_edges=False):
    """pd.qcut(x, q, labels=False, duplicates='drop') + 1 of x fp64 [n] on the device, int8 [n]: the edges are the
    linear interpolations at (n - 1) k / q of the sorted copy (torch.sort, plumbing) in the float64 steps pandas
    takes (include/recsys_amd.h: the same bits as pd.Series.quantile), equal edges dropped, bucket =
    #{edges < x}, the lowest edge in bucket 1; a constant column is 1 everywhere. No host read. With return_edges
    also (edges fp64 [q + 1], n_edges int32 [1])."""
    fn = "quantile_bucket"
    N.ensure_device(x)
    n, q = x.numel(), int(q)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= n < 2^31 values (got {n})")
    _gbdt_rows(fn, "x", x, torch.float64, n, x)
    if not 1 <= q <= TX_MAX_QUANTILES:
        raise ValueError(f"{fn}: need 1 <= q <= {TX_MAX_QUANTILES} (got {q})")
    s = torch.sort(x).values
    edges = torch.zeros(q + 1, device=x.device, dtype=torch.float64)
    n_edges = torch.zeros(1, device=x.device, dtype=torch.int32)
    bucket = torch.empty(n, device=x.device, dtype=torch.int8)
    with timed("tx/quantile_bucket"):
        N.check(N.lib().rsx_quantile_bucket(N.ptr(x), N.ptr(s), n, q, N.ptr(edges), N.ptr(n_edges), N.ptr(bucket),
                                            N.stream()), fn)
    return (bucket, edges, n_edges) if return_edges else bucket


def tx_sequences(row_seg, C, item, day, valid, max_len=50):
    """Per customer of row_seg int32 [T] the last max_len rows whose item is marked in valid uint8 [N]: the CSR
    (seq_off int64 [C + 1], seq_item int32, seq_delta int32 = the day of the customer's last kept row - day), in
    table order. A customer without a valid row has an empty range. One host read (the number of kept rows)."""
    fn = "tx_sequences"
    T = _tx_rows(fn, row_seg)
    C, max_len = _tx_count(fn, "C", C), int(max_len)
    _gbdt_rows(fn, "item", item, torch.int32, T, row_seg)
    _gbdt_rows(fn, "day", day, torch.int32, T, row_seg)
    if valid.dtype != torch.uint8 or valid.dim() != 1 or not 1 <= valid.numel() < 2 ** 31 or not valid.is_contiguous():
        raise ValueError(f"{fn}: valid must be a contiguous uint8 vector over the items")
    if valid.device != row_seg.device:
        raise RuntimeError(f"{fn}: valid is on {valid.device}, expected {row_seg.device}")
    if max_len < 1:
        raise ValueError(f"{fn}: max_len must be >= 1 (got {max_len})")
    dev = row_seg.device
    rank = torch.empty(T, device=dev, dtype=torch.int32)
    n_valid = torch.empty(C, device=dev, dtype=torch.int32)
    last_day = torch.empty(C, device=dev, dtype=torch.int32)
    ws = _tx_ws(T, dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/sequence_ranks"):
        N.check(N.lib().rsx_tx_sequence_ranks(N.ptr(row_seg), C, T, N.ptr(item), N.ptr(day), N.ptr(valid), valid.numel(),
                                              N.ptr(ws), ws.numel(), N.ptr(rank), N.ptr(n_valid), N.ptr(last_day),
                                              N.ptr(flag), N.stream()), fn)
    seq_off = torch.zeros(C + 1, device=dev, dtype=torch.int64)
    torch.cumsum(n_valid.clamp(max=max_len), 0, out=seq_off[1:])
    n_out = int(seq_off[-1])
    seq_item = torch.empty(n_out, device=dev, dtype=torch.int32)
    seq_delta = torch.empty(n_out, device=dev, dtype=torch.int32)
    with timed("tx/sequences"):
        N.check(N.lib().rsx_tx_sequences(N.ptr(row_seg), C, T, N.ptr(item), N.ptr(day), N.ptr(rank), N.ptr(last_day),
                                         N.ptr(seq_off), max_len, n_out, N.ptr(seq_item), N.ptr(seq_delta), N.ptr(flag),
                                         N.stream()), fn)
    _TX_SEQ_GUARD.watch(flag)
    return seq_off, seq_item, seq_delta


# the persona columns' passes (reference staticstics/preprocess_clustering.py)
PERSONA_COLUMNS = ("basket_size", "avg_price", "cat_entropy", "long_tail_ratio", "weekend_ratio", "repurchase_rate",
                   "relative_price_pos")
_TX_RUNS_GUARD = IdRangeGuard("tx_segment_runs: a value column that decreases inside a segment, or a row_seg that "
                              "decreases or has an entry >= S")
_TX_SUM_GUARD = IdRangeGuard("tx_segment_sum_f64: a row_seg that decreases or has an entry >= S, or a perm entry outside "
                             "[0, T)")
_TX_RATIO_GUARD = IdRangeGuard("tx_price_ratio: an item outside [0, N) or a category outside [0, n_cat)")


def tx_segment_runs(row_seg, S, val):
    """The runs of val int32 [T] (non-decreasing inside every segment of row_seg) per segment: (runs int32 [S] = the
    number of runs = tx_segment_distinct, repeated int32 [S] = the rows in runs longer than one, nlogn fp64 [S] =
    sum n ln n over the runs). ln n - nlogn / n is the entropy of the value counts, repeated / n the share of rows
    whose value occurs more than once. A decreasing pair raises IndexError at a later call (_TX_RUNS_GUARD)."""
    fn = "tx_segment_runs"
    T = _tx_rows(fn, row_seg)
    S = _tx_count(fn, "S", S)
    _gbdt_rows(fn, "val", val, torch.int32, T, row_seg)
    dev = row_seg.device
    runs = torch.empty(S, device=dev, dtype=torch.int32)
    repeated = torch.empty(S, device=dev, dtype=torch.int32)
    nlogn = torch.empty(S, device=dev, dtype=torch.float64)
    ws = torch.empty(N.lib().rsx_tx_workspace_bytes(T) + 4 * T, device=dev, dtype=torch.uint8)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/segment_runs"):
        N.check(N.lib().rsx_tx_segment_runs(N.ptr(row_seg), S, T, N.ptr(val), N.ptr(ws), ws.numel(), N.ptr(runs),
                                            N.ptr(repeated), N.ptr(nlogn), N.ptr(flag), N.stream()), fn)
    _TX_RUNS_GUARD.watch(flag)
    return runs, repeated, nlogn


def tx_segment_sum_f64(row_seg, S, x, perm=None, m2=True):
    """(count int32, sum fp64, m2 fp64 or None), each [S]: per segment of row_seg int32 [T] the rows, the fp64 sum of
    x fp64 [T] (read through perm int64 [T] when given) and, with m2, sum (x - sum / count)^2 from a second pass.
    Fixed combination order: the same bits every call; a 0.0 / 1.0 column is counted exactly."""
    fn = "tx_segment_sum_f64"
    T = _tx_rows(fn, row_seg)
    S = _tx_count(fn, "S", S)
    _gbdt_rows(fn, "x", x, torch.float64, T, row_seg)
    if perm is not None:
        _gbdt_rows(fn, "perm", perm, torch.int64, T, row_seg)
    dev = row_seg.device
    count = torch.empty(S, device=dev, dtype=torch.int32)
    total = torch.empty(S, device=dev, dtype=torch.float64)
    second = torch.empty(S, device=dev, dtype=torch.float64) if m2 else None
    ws = _tx_ws(T, dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("tx/segment_sum_f64"):
        N.check(N.lib().rsx_tx_segment_sum_f64(N.ptr(row_seg), S, T, N.ptr(perm), N.ptr(x), N.ptr(ws), ws.numel(),
                                               N.ptr(count), N.ptr(total), N.ptr(second), N.ptr(flag), N.stream()), fn)
    _TX_SUM_GUARD.watch(flag)
    return count, total, second


def tx_price_ratio(item, price, item_cat, cat_mean):
    """ratio fp64 [T] = price / cat_mean[item_cat[item]] in fp64: item int32 [T], price fp32 [T], item_cat int32 [N],
    cat_mean fp64 [n_cat]. An item or category out of range gives 0 and raises IndexError at a later call
    (_TX_RATIO_GUARD.check())."""
    fn = "tx_price_ratio"
    T = _tx_rows(fn, item, "item")
    _gbdt_rows(fn, "price", price, torch.float32, T, item)
    n_items, n_cat = item_cat.numel(), cat_mean.numel()
    if not 1 <= n_cat <= n_items < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= n_cat <= N < 2^31 (got n_cat {n_cat}, N {n_items})")
    _gbdt_rows(fn, "item_cat", item_cat, torch.int32, n_items, item)
    _gbdt_rows(fn, "cat_mean", cat_mean, torch.float64, n_cat, item)
    ratio = torch.empty(T, device=item.device, dtype=torch.float64)
    flag = torch.zeros(1, device=item.device, dtype=torch.int32)
    with timed("tx/price_ratio"):
        N.check(N.lib().rsx_tx_price_ratio(N.ptr(item), N.ptr(price), T, N.ptr(item_cat), N.ptr(cat_mean), n_items, n_cat,
                                           N.ptr(ratio), N.ptr(flag), N.stream()), fn)
    _TX_RATIO_GUARD.watch(flag)
    return ratio


# ----------------------------------------------------------------------------------------
# A21 k-means on a fixed-point grid (csrc/kmeans.hip; include/recsys_amd.h, "k-means"). The data are feature-major:
# X fp64 [d, C], q int32 [d, C] standing for q 2^-frac_bits; centres fp64 [K, d].
KMEANS_MAX_D = 32
KMEANS_MAX_K = 256
KMEANS_MAX_KD = 4096
KMEANS_MAX_FRAC_BITS = 20
KMEANS_POLL = 8           # iterations enqueued between two looks at the done flag
_CUS = {}


def num_cus(device=None) -> int:
    """The compute units of a device (grid sizing, speed only)."""
    idx = torch.device("cuda" if device is None else device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _CUS:
        _CUS[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return _CUS[idx]


def _km_matrix(fn, name, t, dtype, ref=None):
    """t is a contiguous dtype [d, C] device matrix; returns (d, C)."""
    N.ensure_device(t)
    if t.dtype != dtype:
        raise TypeError(f"{fn}: {name} must be {dtype}, got {t.dtype}")
    if ref is not None and t.device != ref.device:
        raise RuntimeError(f"{fn}: {name} is on {t.device}, expected {ref.device}")
    if t.dim() != 2 or t.numel() == 0 or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous non-empty matrix, got shape {tuple(t.shape)}")
    return t.shape[0], t.shape[1]


def _km_shape(fn, d, C, K):
    if not (1 <= d <= KMEANS_MAX_D and 1 <= K <= KMEANS_MAX_K and K * d <= KMEANS_MAX_KD and 1 <= C < 2 ** 31):
        raise ValueError(f"{fn}: need 1 <= d <= {KMEANS_MAX_D}, 1 <= K <= {KMEANS_MAX_K}, K d <= {KMEANS_MAX_KD} and "
                         f"1 <= C < 2^31 rows (got d {d}, K {K}, C {C})")


def _km_grid(max_workgroups, dev):
    g = 4 * num_cus(dev) if max_workgroups is None else int(max_workgroups)
    if g < 1:
        raise ValueError(f"kmeans: max_workgroups must be >= 1 (got {g})")
    return g


def _km_centres(fn, centres, d, ref):
    if centres.dtype != torch.float64 or centres.dim() != 2 or centres.shape[1] != d or not centres.is_contiguous():
        raise ValueError(f"{fn}: centres must be a contiguous fp64 [K, {d}] matrix, got {centres.dtype} "
                         f"{tuple(centres.shape)}")
    if centres.device != ref.device:
        raise RuntimeError(f"{fn}: centres is on {centres.device}, expected {ref.device}")
    return centres.shape[0]


def standardize_columns(X, out=True):
    """X fp64 [d, C], feature-major -> ((X - mean) / scale fp64 [d, C], mean, scale, var), each of the last three fp64
    [d]: sklearn's StandardScaler (population variance, scale 1 for a constant column) from two-pass fixed-order
    sums: the same bits every call. out=False: the moments only (the first entry is None)."""
    fn = "standardize_columns"
    d, C = _km_matrix(fn, "X", X, torch.float64)
    if d > 65535 or C >= 2 ** 31:
        raise ValueError(f"{fn}: need d <= 65535 columns of C < 2^31 values (got {d}, {C})")
    dev = X.device
    Z = torch.empty_like(X) if out else None
    mean, var, scale = (torch.empty(d, device=dev, dtype=torch.float64) for _ in range(3))
    ws = torch.empty((2 + (C + 4095) // 4096) * d, device=dev, dtype=torch.float64)
    with timed("kmeans/standardize"):
        N.check(N.lib().rsx_standardize_columns(N.ptr(X), d, C, N.ptr(ws), ws.numel(), N.ptr(Z), N.ptr(mean), N.ptr(var),
                                                N.ptr(scale), N.stream()), fn)
    return Z, mean, scale, var


def kmeans_frac_bits(X) -> int:
    """min(20, 30 - ceil(log2(max |X|))): the grid on which every value of X fits an int32 with a bit to spare. One
    host read (the maximum)."""
    m = float(X.abs().max())
    if not math.isfinite(m):
        raise ValueError("kmeans: the data hold a NaN or an infinity")
    bits = KMEANS_MAX_FRAC_BITS if m == 0.0 else min(KMEANS_MAX_FRAC_BITS, 30 - math.ceil(math.log2(m)))
    if bits < 0:
        raise ValueError(f"kmeans: max |x| = {m} does not fit the fixed-point grid (|x| <= 2^30)")
    return bits


def kmeans_quantize(X, frac_bits=None):
    """X fp64 [d, C] -> (q int32 [d, C] = rint(X 2^frac_bits), frac_bits). Raises ValueError when a value does not
    fit or is a NaN (one host read of the flag)."""
    fn = "kmeans_quantize"
    d, C = _km_matrix(fn, "X", X, torch.float64)
    frac_bits = kmeans_frac_bits(X) if frac_bits is None else int(frac_bits)
    if not 0 <= frac_bits <= 30:
        raise ValueError(f"{fn}: need 0 <= frac_bits <= 30 (got {frac_bits})")
    q = torch.empty(d, C, device=X.device, dtype=torch.int32)
    flag = torch.zeros(1, device=X.device, dtype=torch.int32)
    with timed("kmeans/quantize"):
        N.check(N.lib().rsx_kmeans_quantize(N.ptr(X), d, C, frac_bits, N.ptr(q), N.ptr(flag), N.stream()), fn)
    if int(flag):
        raise ValueError(f"{fn}: a value does not fit frac_bits = {frac_bits} (|x| 2^frac_bits < 2^31), or is a NaN")
    return q, frac_bits


def kmeans_seed(q, frac_bits, K, seed, max_workgroups=None):
    """k-means++ seeds of q int32 [d, C] as an exponential race (include/recsys_amd.h): (seeds int32 [K], the rows
    drawn, centres fp64 [K, d] = those rows). No host read; the same bits every call."""
    fn = "kmeans_seed"
    d, C = _km_matrix(fn, "q", q, torch.int32)
    K = int(K)
    _km_shape(fn, d, C, K)
    dev = q.device
    grid = _km_grid(max_workgroups, dev)
    seeds = torch.empty(K, device=dev, dtype=torch.int32)
    centres = torch.empty(K, d, device=dev, dtype=torch.float64)
    ws = torch.empty(N.lib().rsx_kmeans_seed_workspace_bytes(C, grid), device=dev, dtype=torch.uint8)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    with timed("kmeans/seed"):
        N.check(N.lib().rsx_kmeans_seed(N.ptr(q), d, C, int(frac_bits), K, int(seed) & (2 ** 64 - 1), grid, N.ptr(ws),
                                        ws.numel(), N.ptr(seeds), N.ptr(centres), N.ptr(flag), N.stream()), fn)
    return seeds, centres


def kmeans_assign(q, frac_bits, centres, max_workgroups=None, inertia=True):
    """The nearest centre of every row of q int32 [d, C] (the smallest index among equals): (labels int32 [C], dmin
    fp64 [C] = the squared distance to it, inertia fp64 [1] = their fixed-order sum, or None)."""
    fn = "kmeans_assign"
    d, C = _km_matrix(fn, "q", q, torch.int32)
    K = _km_centres(fn, centres, d, q)
    _km_shape(fn, d, C, K)
    dev = q.device
    labels = torch.empty(C, device=dev, dtype=torch.int32)
    dmin = torch.empty(C, device=dev, dtype=torch.float64)
    total = torch.empty(1, device=dev, dtype=torch.float64) if inertia else None
    ws = torch.empty((C + 4095) // 4096, device=dev, dtype=torch.float64)
    with timed("kmeans/assign"):
        N.check(N.lib().rsx_kmeans_assign(N.ptr(q), d, C, int(frac_bits), K, N.ptr(centres), _km_grid(max_workgroups, dev),
                                          N.ptr(ws), ws.numel(), N.ptr(labels), N.ptr(dmin), N.ptr(total), N.stream()), fn)
    return labels, dmin, total


class KMeansFit:
    """centres fp64 [K, d], labels int32 [C], dmin fp64 [C], inertia fp64 [1] (all on the device), n_iter (int) and
    counts int32 [K]: the rows of every cluster under the final labels."""

    def __init__(self, centres, labels, dmin, inertia, n_iter, frac_bits):
        self.centres, self.labels, self.dmin, self.inertia = centres, labels, dmin, inertia
        self.n_iter, self.frac_bits = n_iter, frac_bits

    @property
    def counts(self):
        return torch.bincount(self.labels, minlength=self.centres.shape[0]).to(torch.int32)


def kmeans_fit(q, frac_bits, centres, tol_abs=0.0, max_iter=300, max_workgroups=None, poll=KMEANS_POLL):
    """Lloyd's iterations on q int32 [d, C] from the centres fp64 [K, d] (not modified): an iteration assigns every
    row, sums the clusters in integers and moves the centres; the fit ends with the first iteration after which no
    label changed or the centres' squared shift is <= tol_abs, or after max_iter. The device decides that; the host
    looks every `poll` iterations, which changes no result. Then one assignment against the final centres, as
    sklearn does. Returns a KMeansFit."""
    fn = "kmeans_fit"
    d, C = _km_matrix(fn, "q", q, torch.int32)
    K = _km_centres(fn, centres, d, q)
    _km_shape(fn, d, C, K)
    max_iter, poll, frac_bits, tol_abs = int(max_iter), int(poll), int(frac_bits), float(tol_abs)
    if max_iter < 1 or poll < 1 or not tol_abs >= 0.0:
        raise ValueError(f"{fn}: need max_iter >= 1, poll >= 1 and tol_abs >= 0")
    dev = q.device
    grid = _km_grid(max_workgroups, dev)
    centres = centres.clone()
    labels = torch.full((C,), -1, device=dev, dtype=torch.int32)
    sum_q = torch.zeros(K, d, device=dev, dtype=torch.int64)
    count = torch.zeros(K, device=dev, dtype=torch.int32)
    ctl = torch.zeros(4, device=dev, dtype=torch.int32)
    shift = torch.zeros(1, device=dev, dtype=torch.float64)
    it, done = 0, 0
    with timed("kmeans/iterate"):
        while it < max_iter and not done:
            n = min(poll, max_iter - it)
            N.check(N.lib().rsx_kmeans_iterate(N.ptr(q), d, C, frac_bits, K, N.ptr(centres), N.ptr(labels), N.ptr(sum_q),
                                               N.ptr(count), N.ptr(ctl), N.ptr(shift), tol_abs, it + 1, n, grid,
                                               N.stream()), fn)
            it += n
            done = int(ctl[1])
    labels, dmin, inertia = kmeans_assign(q, frac_bits, centres, grid)
    return KMeansFit(centres, labels, dmin, inertia, done if done else max_iter, frac_bits)


# ----------------------------------------------------------------------------------------
# Optional per-op device timing (bench.py): HIP events on the launching (current) stream.
_TIMING = {"on": False, "events": {}}


class timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _TIMING["on"]:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _TIMING["on"]:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMING["events"].setdefault(self.name, []).append((self.e0, e1))
        return False


def timing_start():
    _TIMING["on"] = True
    _TIMING["events"] = {}


def timing_stop():
    """-> {name: (launches, total_ms)} (synchronises)."""
    _TIMING["on"] = False
    torch.cuda.synchronize()
    out = {}
    for k, evs in _TIMING["events"].items():
        out[k] = (len(evs), sum(a.elapsed_time(b) for a, b in evs))
    return out
