"""The library's dropout keep-mask rebuilt on the host (numpy only, no GPU use).

The mask is a pure function of (seed, flat element index): murmur3's fmix32 finaliser over the
index mixed with the 64-bit seed (csrc/rsx_common.h:18-27, hash_u32), kept iff hash >= thresh
(rsx_common.h:31-37), with thresh and the keep scale as make_dropout computes them
(rsx_common.h:40-54). Seeds come from torch's CPU generator (ops.next_seed), so a test that
replays the generator can rebuild every mask of a run and hand it to a float64 reference.

Index maps, one helper per kernel family. Each cites the function that forms the index (`bi`,
`base_idx`, `rowidx` or `idx` there) and, as a hint that may drift, the line at the time of writing:
  rows_index       r * D + c         ln.hip: ln_fwd_k (:63), ln_fwd_wide_k (:111), their backward kernels and
                                     dropout_bwd_k (:358-367, rsx_dropout_bwd, flat over T x D);
                                     seq_embed.hip: ln_drop_store (:152) and its backward (:372); the static
                                     profile's row * 128 + col (profile.hip rsx_static_profile_fwd / _bwd:
                                     rsx_dropout_bwd over the U output rows, :303 / :325); DCN's row * 256 +
                                     col (ops.py dcn_train_step, rsx_dropout_bwd over [B, 256])
  gemm_index       m * N + n         gemm_x3.hip: the header comment (:17), keep() (:73-83) as called in
                                     epilogue() (:171-173), gemm_splitk_reduce_k (:349-351) and gemm_ws_k's
                                     epilogues (:513, :580) for EPI_GELU_DROP / EPI_DGELU_DROP and for
                                     rsx_gemm_x3_addln's out-projection dropout
  attention_index  ((tok * H + h) * 64 + k)
                                     mha.hip: mha_fwd_k (:106), mha_bwd_k (:222), mha_bwd64_k (:353),
                                     mha_bwd_mfma_k (:521), the bf16x3 forward bodies behind mha_fwd_x3b_k /
                                     mha_fwd_x3b64_k (:757 / :860), mha_bwd_x3p_k (:1006), mha_bwd_x3s_k (:1200),
                                     mha_qkv_fwd_x3_k's body (:1527); tower.hip: tw_lastq_fwd_k (:185),
                                     tw_lastq_bwd_k (:237). tok = the query's packed (or flat b * L + i) token
                                     row, k = the key's position inside its sequence / segment
"""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def _fmix32(x):
    """murmur3 fmix32 on uint64 lanes holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def hash_u32(seed, idx):
    """rsx::hash_u32(seed, idx) (rsx_common.h:18-27): 64-bit seed, 64-bit index, both high words
    mixed in. Returns uint32 of idx's shape."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = _u64(idx)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    x = (idx & _M32) ^ (((idx >> np.uint64(32)) * np.uint64(0x9E3779B1)) & _M32) ^ s_lo
    x = x ^ ((s_hi * np.uint64(0x85EBCA77)) & _M32)
    return _fmix32(x).astype(np.uint32)


def hash_u32_low(seed, idx32):
    """The 32-bit shortcut of gemm_x3.hip:73-83 (keep(): index < 2^32, no index-high-word term)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = _u64(idx32) & _M32
    x = idx ^ np.uint64(seed & 0xFFFFFFFF)
    x = x ^ ((np.uint64(seed >> 32) * np.uint64(0x85EBCA77)) & _M32)
    return _fmix32(x).astype(np.uint32)


def threshold(p) -> int:
    """make_dropout's thresh (rsx_common.h:43-51): p as float32, floor(double(p) * 2^32) capped at
    2^32 - 1, at least 1 when p > 0; 0 (= dropout off) when p <= 0."""
    p32 = np.float32(p)
    if p32 <= np.float32(0.0):
        return 0
    t = float(p32) * 4294967296.0
    if t >= 4294967295.0:
        t = 4294967295.0
    return max(int(t), 1)


def scale32(p) -> np.float32:
    """make_dropout's keep scale: float32(1) / (float32(1) - float32(p)); 1 when p <= 0."""
    p32 = np.float32(p)
    if p32 <= np.float32(0.0):
        return np.float32(1.0)
    return np.float32(1.0) / (np.float32(1.0) - p32)


def keep(seed, p, idx):
    """Boolean keep-mask: hash >= thresh (all True at p <= 0, where thresh = 0)."""
    return hash_u32(seed, idx) >= np.uint32(threshold(p))


def rows_index(T, D, row0=0):
    """[T, D] indices r * D + c for rows row0 .. row0 + T - 1."""
    r = np.arange(row0, row0 + T, dtype=np.uint64)[:, None]
    return r * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]


def gemm_index(M, N):
    """[M, N] indices m * N + n of the GEMM epilogues."""
    return rows_index(M, N)


def attention_index(tok, H, n_keys):
    """[..., H, n_keys] indices ((tok * H + h) * 64 + k) for query token rows tok (any shape)."""
    tok = _u64(tok)[..., None, None]
    h = np.arange(H, dtype=np.uint64)[:, None]
    k = np.arange(n_keys, dtype=np.uint64)[None, :]
    return (tok * np.uint64(H) + h) * np.uint64(64) + k


def rows_keep(seed, p, T, D, row0=0):
    return keep(seed, p, rows_index(T, D, row0))


def attention_keep(seed, p, tok, H, n_keys):
    return keep(seed, p, attention_index(tok, H, n_keys))
