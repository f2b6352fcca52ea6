"""Every dropout path at p > 0 against float64 with the keep-mask rebuilt on the host.

The mask is hash(seed, flat index) >= thresh (csrc/rsx_common.h), restated in tests/dropout_ref.py
with one index map per kernel family; seeds are either passed explicitly or replayed from torch's
CPU generator (ops.next_seed). Four groups:

  a. host mask == device mask exactly, for the elementwise ops (the set of zeroed elements);
  b. attention (every kernel of mha.hip) against P = softmax(masked scores), Pd = P * keep *
     float64(scale32(p)), out = Pd @ V in float64, gradients from float64 autograd;
  c. ops._FFN and ops.seq_embed at p = 0.2, value and every gradient;
  d. the user tower at p = 0.2 (per-op path, native program, native tail form) against
     tests/tower_dropout_ref.py, output and every parameter gradient.
  e. negative controls inside (b)-(d): the reference recomputed with ONE site's mask drawn from
     seed + 1 must miss the same comparison by at least 100x its tolerance (host work only).

Each comparison is reduced to one figure, max |device - ref| / (atol + rtol |ref|) ("excess"; the
assertion is excess <= 1, a control needs excess >= 100), printed before it is asserted.

Attention: which kernel a configuration reaches (the entry points rsx_mha_fwd / rsx_mha_bwd /
rsx_mha_fwd_x3 / rsx_mha_bwd_x3 at the end of mha.hip; ops._MHA picks the _x3 forward for bf16x3 at head dim 32 and
64, the _x3 backward for bf16x3 at head dim 32 only). L is the dense length or the packed max_len:

  precision  head dim  forward            backward
  fp32       16        mha_fwd_k<16>      mha_bwd_k<16>
  fp32       32        mha_fwd_k<32>      mha_bwd_mfma_k
  fp32       64        mha_fwd_k<64>      mha_bwd64_k<32> (L <= 32), mha_bwd64_k<64> (L > 32)
  bf16x3     32        mha_fwd_x3b_k      mha_bwd_x3s_k (causal), mha_bwd_x3p_k (non-causal)
  bf16x3     64        mha_fwd_x3b64_k    the fp32 mha_bwd64_k<32> / <64> (must regenerate the x3 mask)
  fused      32 (H=4)  mha_qkv_fwd_x3_k   mha_bwd_x3s_k / mha_bwd_x3p_k
  tower tail 32        tw_lastq_fwd_k     tw_lastq_bwd_k      (group d, the tail form)

_MHA_CASES below runs every row dense and packed, causal and non-causal, at p = 0.2 and 0.5.

Attention tolerances: tests/test_gpu_kernels.py's _MHA_TOL (output atol, gradient atol) = fp32
(2e-5, 5e-5), bf16x3 (6e-5, 2e-4), output atol x2 at head dim 64 (test_mha_head_dim_64_forward: twice
the score terms; the gradient keeps the 1x that test_mha_forward_backward holds head dim 64 to), rtol
1e-5 / 1e-4, and every atol multiplied by 1 / (1 - p): each kept probability is P * 1 / (1 - p), so the
output, dP and with them every error term of the p = 0 analysis carry that factor. That gives, (out,
grad) atol: fp32 (2.5e-5, 6.25e-5) at p = 0.2 and (4e-5, 1e-4) at p = 0.5; bf16x3 (7.5e-5, 2.5e-4) and
(1.2e-4, 4e-4); head dim 64 doubles the first of each pair. The fused path's output is held to the same
bf16x3 bound as every other row, and its dx / dw / db, which the pair does not cover, to the suite's
token-linear rule (2e-4 + 2e-5 max|ref|) / (1 - p) (test_linear_tok_autograd_matches_linear).
Measured maxima on an MI355X over all cases, (out, dqkv) at p = 0.2 / p = 0.5: fp32 head dim 16
(7.9e-7, 2.7e-6) / (1.1e-6, 3.5e-6), 32 (8.4e-7, 4.3e-6) / (9.9e-7, 5.3e-6), 64 (1.1e-6, 6.8e-6) / (1.5e-6,
4.4e-6); bf16x3 head dim 32 (4.2e-5, 6.2e-5) / (4.9e-5, 7.6e-5), 64 (3.3e-5, 8.9e-5) / (6.1e-5, 1.2e-4); the
fused path's out errs by at most 4.7e-5 / 7.8e-5 (0.50 of 7.5e-5 / 1.2e-4 with the rtol term), and its
dx, dw, db use at most 0.25, 0.34, 0.15 of their bounds. The weakest
seed + 1 control of groups (b) and (c) misses its bound 9000-fold, of the tower 2700-fold.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops, synth
from recsys_amd.tower_code import v1_refine_usertower as T
from tests import dropout_ref as R
from tests import tower_dropout_ref as TR
from tests.helpers import small_cfg, small_universe, to_dev

pytestmark = pytest.mark.gpu

SEED_HI = 0x123456789AD0          # non-zero high word
SEED_HI2 = 2 ** 61 + 12345
_MHA_TOL = {"fp32": (2e-5, 5e-5), "bf16x3": (6e-5, 2e-4)}   # tests/test_gpu_kernels.py


def _excess(a, r, atol, rtol):
    """max |a - r| / (atol + rtol |r|): <= 1 is assert_close(atol, rtol) passing."""
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    if a.numel() == 0:
        return 0.0
    return float(((a - r).abs() / (atol + rtol * r.abs())).max())


def _t(mask):
    return torch.from_numpy(np.ascontiguousarray(mask))


def _replayed_seed(s):
    """The seed the next ops.next_seed() call draws after torch.manual_seed(s); the generator is
    left re-seeded, ready for the device call that draws it."""
    torch.manual_seed(s)
    seed = ops.next_seed()
    torch.manual_seed(s)
    return seed


# ------------------------------------------------------------------ a. host mask == device mask
@pytest.mark.parametrize("D", [64, 2048])
@pytest.mark.parametrize("seed", [SEED_HI, 5])
def test_add_dropout_mask_is_host_mask(gpu, D, seed):
    """_AddDropout (rsx_ln_fwd's add-only form, ln_fwd_k<64> / ln_fwd_wide_k<8>; rsx_dropout_bwd):
    s == x exactly where the host mask drops, s = x + res * scale where it keeps; dres = ds * scale
    on the kept set and exactly 0 elsewhere. T = 37 rows (a partly filled last row group)."""
    g = torch.Generator().manual_seed(D)
    Tn, p = 37, 0.2
    x = torch.randn(Tn, D, generator=g)
    res = torch.randn(Tn, D, generator=g) + 3.0          # no zeros
    ds = torch.randn(Tn, D, generator=g)
    keep = _t(R.rows_keep(seed, p, Tn, D))
    sc = float(R.scale32(p))
    rd = res.to(gpu).requires_grad_()
    s = ops._AddDropout.apply(x.to(gpu), rd, p, seed)
    s.backward(ds.to(gpu))
    s = s.detach().cpu()
    assert torch.equal(s == x, ~keep)
    torch.testing.assert_close(s.double(), x.double() + res.double() * keep * sc, atol=1e-6, rtol=1e-6)
    assert torch.equal(rd.grad.cpu(), torch.where(keep, ds * torch.tensor(R.scale32(p)), torch.zeros(())))
    # with x = 0 the output is the dropped residual itself, bit for bit
    s0 = ops._AddDropout.apply(torch.zeros(Tn, D, device=gpu), res.to(gpu), p, seed).cpu()
    assert torch.equal(s0, torch.where(keep, res * torch.tensor(R.scale32(p)), torch.zeros(())))


def test_seq_embed_mask_is_host_mask(gpu):
    """ops.seq_embed (D = 128, B = 5, L = 7, dense): the output is the p = 0 output times the host
    mask (index (b * L + l) * 128 + c) and the float32 scale; seed replayed from the generator."""
    g = torch.Generator().manual_seed(3)
    B, L, D = 5, 7, 128
    rows = (31, 12, 9, 9, 9, 9)
    base = torch.randn(B, L, D, generator=g)
    tables = [torch.randn(r, D, generator=g) * 0.02 for r in rows]
    ids = [torch.randint(0, r, (B, L), generator=g) for r in rows]
    gate = torch.sigmoid(torch.randn(6, generator=g))
    pos = torch.randn(L, D, generator=g) * 0.02
    lw = 1 + 0.1 * torch.randn(D, generator=g)
    lb = 0.1 * torch.randn(D, generator=g)
    d = lambda t: t.to(gpu)
    args = (d(base), [d(i) for i in ids], [d(t) for t in tables], d(gate), d(pos), d(lw), d(lb))
    y0 = ops.seq_embed(*args, p_drop=0.0).cpu()
    assert (y0 != 0).all()
    p = 0.2
    seed = _replayed_seed(77)
    assert seed >> 32 != 0
    y = ops.seq_embed(*args, p_drop=p).cpu()
    keep = _t(R.rows_keep(seed, p, B * L, D)).view(B, L, D)
    assert torch.equal(y == 0, ~keep)
    torch.testing.assert_close(y, torch.where(keep, y0 * torch.tensor(R.scale32(p)), torch.zeros(())),
                               atol=0, rtol=3e-7)


@pytest.mark.parametrize("K", [128, 1024])
def test_gemm_gelu_drop_mask_is_host_mask(gpu, K):
    """rsx_gemm_x3 EPI_GELU_DROP / EPI_DGELU_DROP at (M, N, K) = (131, 256, K); K = 1024 takes the
    split-K path (epilogue in the reduction pass). Zeroed set == host mask over m * 256 + n."""
    g = torch.Generator().manual_seed(K)
    M, Nn, p, seed = 131, 256, 0.2, SEED_HI2
    if K == 1024:
        assert N.lib().rsx_gemm_x3_split_floats(M, Nn, K) > 0
    x = torch.randn(M, K, generator=g).to(gpu)
    w1 = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).to(gpu)
    b1 = torch.randn(Nn, generator=g).to(gpu)
    aux0 = torch.empty(M, Nn, device=gpu)
    aux = torch.empty(M, Nn, device=gpu)
    g0 = ops.gemm_x3(x, w1, b1, ops.EPI_GELU_DROP, aux0, 0.0, 0).cpu()
    act = ops.gemm_x3(x, w1, b1, ops.EPI_GELU_DROP, aux, p, seed).cpu()
    keep = _t(R.keep(seed, p, R.gemm_index(M, Nn)))
    assert np.array_equal(R.hash_u32(seed, R.gemm_index(M, Nn)), R.hash_u32_low(seed, R.gemm_index(M, Nn)))
    live = g0 != 0
    assert live.float().mean() > 0.99
    assert torch.equal((act == 0)[live], (~keep)[live])
    torch.testing.assert_close(act, torch.where(keep, g0 * torch.tensor(R.scale32(p)), torch.zeros(())),
                               atol=0, rtol=3e-7)
    assert torch.equal(aux, aux0)
    dy = torch.randn(M, K, generator=g).to(gpu)
    w2 = (torch.randn(K, Nn, generator=g) / math.sqrt(Nn)).to(gpu)
    d0 = ops.gemm_x3(dy, w2.t(), None, ops.EPI_DGELU_DROP, aux, 0.0, 0).cpu()
    dp = ops.gemm_x3(dy, w2.t(), None, ops.EPI_DGELU_DROP, aux, p, seed).cpu()
    live = d0 != 0
    assert torch.equal((dp == 0)[live], (~keep)[live])
    torch.testing.assert_close(dp, torch.where(keep, d0 * torch.tensor(R.scale32(p)), torch.zeros(())),
                               atol=1e-7, rtol=1e-6)


def test_static_profile_mask_is_host_mask(gpu):
    """ops.static_profile, U = 257 users and rows = 514 (both views share the users, output row r
    reads user r % 257): the mask is keyed by the OUTPUT row, r * 128 + c over all 514 rows, so the
    two views of a user draw different masks."""
    from tests.test_gpu_static_profile import _inputs, _model
    m = _model()
    U, p = 257, 0.2
    ids, cont = _inputs(U)
    with torch.no_grad():
        y0 = ops.static_profile(m, ids, cont, 0.0, rows=2 * U).cpu()
        assert torch.equal(y0[:U], y0[U:])
        seed = _replayed_seed(4242)
        y = ops.static_profile(m, ids, cont, p, rows=2 * U).cpu()
    keep = _t(R.rows_keep(seed, p, 2 * U, 128))
    live = y0 != 0
    assert live.float().mean() > 0.99
    assert torch.equal((y == 0)[live], (~keep)[live])
    assert not torch.equal(keep[:U], keep[U:])
    torch.testing.assert_close(y, torch.where(keep, y0 * torch.tensor(R.scale32(p)), torch.zeros(())),
                               atol=0, rtol=3e-7)


# ------------------------------------------------------------------ b. attention
def _attn_ref(qkv, pad, H, causal, keep_scaled):
    """One dense batch [B, L, 3D] in float64 with dropout on the probabilities; keep_scaled
    [B, H, L, L] = keep * scale. Queries without an allowed key give zero rows."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (t.view(B, L, H, dh).transpose(1, 2) for t in qkv.split(D, -1))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    allowed = torch.ones(B, 1, L, L, dtype=torch.bool)
    if causal:
        allowed = allowed & torch.tril(torch.ones(L, L, dtype=torch.bool))
    if pad is not None:
        allowed = allowed & ~pad[:, None, None, :]
    s = s.masked_fill(~allowed, float("-inf"))
    s = s.masked_fill(~allowed.any(-1, keepdim=True), 0.0)
    prob = torch.softmax(s, -1) * allowed
    return ((prob * keep_scaled) @ v).transpose(1, 2).reshape(B, L, D)


def _attn_case(dense, L, width, seed_rng):
    """(rows, pad, seg) of one configuration; rows are N(0, 1) of the given width (qkv for _MHA, x
    for the fused path). Dense: B = 7 sequences of L with left padding (B * H is no multiple of 4
    for H in {1, 2}: a partly filled last workgroup of the 256-thread kernels). Packed: segments
    whose lengths include 1, 33 and 64 (capped at L), some ending on a padded key."""
    g = torch.Generator().manual_seed(seed_rng)
    if dense:
        B = 7
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = L
        lens[1] = 1
        pad = torch.arange(L)[None, :] < (L - lens)[:, None]
        return torch.randn(B, L, width, generator=g), pad, None
    lens = torch.randint(1, L + 1, (7,), generator=g)
    lens[:4] = torch.tensor([1, min(33, L), L, min(17, L)])
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0)])
    rows = torch.randn(int(seg[-1]), width, generator=g)
    pad = torch.zeros(rows.shape[0], dtype=torch.bool)
    pad[seg[1:] - 1] = torch.tensor([True, False, True, False, True, False, True])
    return rows, pad, seg


def _attn_reference(qkv64, pad, seg, H, causal, p, seed):
    sc = float(R.scale32(p))
    if seg is None:
        B, L = qkv64.shape[:2]
        tok = np.arange(B * L).reshape(B, L)
        m = _t(R.attention_keep(seed, p, tok, H, L).astype(np.float64) * sc).permute(0, 2, 1, 3)
        return _attn_ref(qkv64, pad, H, causal, m)
    outs = []
    for b in range(seg.numel() - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        tok = np.arange(s0, s1)[None, :]
        m = _t(R.attention_keep(seed, p, tok, H, s1 - s0).astype(np.float64) * sc).permute(0, 2, 1, 3)
        outs.append(_attn_ref(qkv64[s0:s1][None], pad[s0:s1][None], H, causal, m)[0])
    return torch.cat(outs)


# (precision, head dim, H, form, L = dense length / packed max_len); see the table in the docstring
_MHA_CASES = (
    [(prec, dh, H, "dense", L) for prec, dh, H in [("fp32", 16, 2), ("fp32", 32, 2), ("fp32", 64, 1),
                                                   ("bf16x3", 32, 2), ("bf16x3", 64, 1)]
     for L in (1, 17, 50, 64)]
    + [("fp32", 16, 2, "packed", 64), ("fp32", 32, 2, "packed", 64), ("fp32", 64, 1, "packed", 64),
       ("fp32", 64, 2, "packed", 32), ("bf16x3", 32, 2, "packed", 64), ("bf16x3", 32, 1, "packed", 64),
       ("bf16x3", 64, 1, "packed", 64), ("bf16x3", 64, 2, "packed", 32)])


@pytest.mark.parametrize("prec,dh,H,form,L", _MHA_CASES)
def test_mha_dropout_against_float64(gpu, prec, dh, H, form, L):
    """ops._MHA with an explicit seed against the float64 reference with the host mask: output,
    dqkv, exact zeros on fully masked rows, and the seed + 1 control; causal and non-causal, p = 0.2
    and 0.5. Tolerances: the module docstring."""
    prev = ops.mha_precision()
    ops.set_mha_precision(prec)
    try:
        for causal in (True, False):
            for p, seed in ((0.2, SEED_HI), (0.5, 777)):
                qkv, pad, seg = _attn_case(form == "dense", L, 3 * H * dh, 1000 * dh + 10 * L + H)
                g = torch.Generator().manual_seed(L + dh)
                dout = torch.randn(qkv.shape[:-1] + (H * dh,), generator=g, dtype=torch.float64)
                q64 = qkv.double().requires_grad_()
                ref = _attn_reference(q64, pad, seg, H, causal, p, seed)
                (ref * dout).sum().backward()
                qd = qkv.to(gpu).requires_grad_()
                seg_d = None if seg is None else seg.to(torch.int32).to(gpu)
                out = ops._MHA.apply(qd, pad.to(gpu), seg_d, H, causal, p, seed, None if seg is None else L)
                (out * dout.float().to(gpu)).sum().backward()
                s = 1.0 / (1.0 - p)
                a_out = _MHA_TOL[prec][0] * (2 if dh == 64 else 1) * s
                a_grad = _MHA_TOL[prec][1] * s
                e_out = _excess(out, ref, a_out, 1e-5)
                e_grad = _excess(qd.grad, q64.grad, a_grad, 1e-4)
                print(f"mha {prec} dh={dh} H={H} {form} L={L} causal={causal} p={p}: "
                      f"out max err {(out.cpu().double() - ref).abs().max().item():.3e} (atol {a_out:.2e}, "
                      f"excess {e_out:.3f}); dqkv max err {(qd.grad.cpu().double() - q64.grad).abs().max().item():.3e}"
                      f" (atol {a_grad:.2e}, excess {e_grad:.3f})")
                assert e_out <= 1.0 and e_grad <= 1.0, (causal, p, e_out, e_grad)
                if causal and seg is None:   # left-padded queries see no key: exactly zero, forward and backward
                    assert (out[pad.to(gpu)] == 0).all() and (qd.grad[pad.to(gpu)] == 0).all()
                    assert pad.any() or L == 1
                # control: the same comparison against the reference with the mask of seed + 1
                q64b = qkv.double().requires_grad_()
                bad = _attn_reference(q64b, pad, seg, H, causal, p, seed + 1)
                (bad * dout).sum().backward()
                c = max(_excess(out, bad, a_out, 1e-5), _excess(qd.grad, q64b.grad, a_grad, 1e-4))
                print(f"    control (seed + 1): excess {c:.1f}")
                assert c >= 100.0, c
    finally:
        ops.set_mha_precision(prev)


@pytest.mark.parametrize("form,L", [("dense", 1), ("dense", 17), ("dense", 50), ("dense", 64), ("packed", 64)])
def test_qkv_mha_fused_dropout_against_float64(gpu, form, L):
    """ops._QKVMHA (mha_qkv_fwd_x3_k; backward mha_bwd_x3s_k causal / mha_bwd_x3p_k non-causal, then
    the in-projection's dx, dw, db) against float64 with the host mask. out is held to the attention
    group's bf16x3 bound, 6e-5 / (1 - p) with rtol 1e-5; dx, dw, db to (2e-4 + 2e-5 max|ref|) / (1 - p).
    Fully masked query rows (dense, causal, left padding): out and dx rows exactly zero (their dqkv
    rows are zero and dx = dqkv @ w)."""
    H, dh, D = 4, 32, 128
    for causal in (True, False):
        for p, seed in ((0.2, SEED_HI2), (0.5, 4242)):
            x, pad, seg = _attn_case(form == "dense", L, D, 7 * L + 1)
            g = torch.Generator().manual_seed(L)
            w = torch.randn(3 * D, D, generator=g) * D ** -0.5
            b = torch.randn(3 * D, generator=g) * 0.1
            dout = torch.randn(x.shape, generator=g, dtype=torch.float64)

            def reference(sd):
                lv = [t.double().requires_grad_() for t in (x, w, b)]
                qkv = F.linear(*lv)
                ref = _attn_reference(qkv, pad, seg, H, causal, p, sd)
                (ref * dout).sum().backward()
                return [ref.detach()] + [t.grad for t in lv]

            refs = reference(seed)
            dv = [t.to(gpu).requires_grad_() for t in (x, w, b)]
            seg_d = None if seg is None else seg.to(torch.int32).to(gpu)
            out = ops._QKVMHA.apply(dv[0], dv[1], dv[2], pad.to(gpu), seg_d, H, causal, p, seed)
            (out * dout.float().to(gpu)).sum().backward()
            s = 1.0 / (1.0 - p)
            got = [out] + [t.grad for t in dv]
            tols = [(_MHA_TOL["bf16x3"][0] * s, 1e-5)] + \
                   [((2e-4 + 2e-5 * float(r.abs().max())) * s, 0.0) for r in refs[1:]]
            bad = reference(seed + 1)
            worst = 0.0
            for name, a, r, rb, (atol, rtol) in zip(["out", "dx", "dw", "db"], got, refs, bad, tols):
                e = _excess(a, r, atol, rtol)
                worst = max(worst, _excess(a, rb, atol, rtol))
                print(f"qkv_mha {form} L={L} causal={causal} p={p} {name}: max err "
                      f"{(a.detach().cpu().double() - r).abs().max().item():.3e} (atol {atol:.2e}, excess {e:.3f})")
                assert e <= 1.0, (name, causal, p, e)
            print(f"    control (seed + 1): excess {worst:.1f}")
            assert worst >= 100.0, worst
            if causal and seg is None:
                assert (out[pad.to(gpu)] == 0).all() and (dv[0].grad[pad.to(gpu)] == 0).all()


# ------------------------------------------------------------------ c. FFN and seq_embed at p = 0.2
def test_ffn_dropout_against_float64(gpu):
    """ops._FFN at p = 0.2 (shapes of test_ffn_matches_torch: 1998 tokens, 128 -> 256 -> 128): value
    and the h, w1, b1, w2, b2 gradients against float64 with the host mask over m * 256 + n;
    |err| <= (2e-4 + 2e-5 max|ref|) / (1 - p), test_ffn_matches_torch's rule times the keep scale."""
    g = torch.Generator().manual_seed(5)
    h = torch.randn(1998, 128, generator=g)
    w1 = torch.randn(256, 128, generator=g) / 11
    b1 = torch.randn(256, generator=g)
    w2 = torch.randn(128, 256, generator=g) / 16
    b2 = torch.randn(128, generator=g)
    gy = torch.randn(1998, 128, generator=g)
    p, seed = 0.2, SEED_HI

    def reference(sd):
        lv = [t.double().requires_grad_() for t in (h, w1, b1, w2, b2)]
        m = _t(R.keep(sd, p, R.gemm_index(1998, 256)).astype(np.float64) * float(R.scale32(p)))
        y = F.linear(F.gelu(F.linear(lv[0], lv[1], lv[2])) * m, lv[3], lv[4])
        (y * gy.double()).sum().backward()
        return [y.detach()] + [t.grad for t in lv]

    dv = [t.to(gpu).requires_grad_() for t in (h, w1, b1, w2, b2)]
    y = ops._FFN.apply(*dv, p, seed)
    (y * gy.to(gpu)).sum().backward()
    got = [y] + [t.grad for t in dv]
    refs, bad = reference(seed), reference(seed + 1)
    worst = 0.0
    for name, a, r, rb in zip(["y", "dh", "dw1", "db1", "dw2", "db2"], got, refs, bad):
        atol = (2e-4 + 2e-5 * float(r.abs().max())) / (1 - p)
        e = _excess(a, r, atol, 0.0)
        worst = max(worst, _excess(a, rb, atol, 0.0))
        print(f"ffn p={p} {name}: max err {(a.detach().cpu().double() - r).abs().max().item():.3e} "
              f"(bound {atol:.3e}, excess {e:.3f})")
        assert e <= 1.0, (name, e)
    print(f"    control (seed + 1): excess {worst:.1f}")
    assert worst >= 100.0, worst


@pytest.mark.parametrize("seg", [False, True])
def test_seq_embed_dropout_against_float64(gpu, seg):
    """ops.seq_embed at p = 0.2 (shapes of test_seq_embed_layernorm_and_backward: B = 37, L = 50,
    D = 128), seed replayed from the generator: forward atol 2e-6 / (1 - p), every gradient (base, the
    six tables, gate, pos, LN weight and bias) atol 2e-5 / (1 - p), rtol 1e-4, against float64 with the
    host mask over (b * L + l) * 128 + c."""
    from tests.test_gpu_kernels import _embed_inputs
    base, tables, ids, gate, pos, lw, lb = _embed_inputs(seed=1)
    B, L, D = base.shape
    p = 0.2
    g = torch.Generator().manual_seed(8)
    dout = torch.randn(B, L, D, generator=g, dtype=torch.float64)
    seed = _replayed_seed(31 + int(seg))

    def reference(sd):
        lv = [t.clone().double().requires_grad_() for t in [base, *tables, gate, pos, lw, lb]]
        x = lv[0].clone()
        for j in range(6):
            x = x + lv[1 + j][ids[j]] * lv[7][j]
        x = x + lv[8].unsqueeze(0)
        m = _t(R.rows_keep(sd, p, B * L, D).astype(np.float64) * float(R.scale32(p))).view(B, L, D)
        ref = F.layer_norm(x, (D,), lv[9], lv[10], 1e-5) * m
        (ref * dout).sum().backward()
        grads = []
        for name, t in zip(names, lv):
            gr = t.grad.clone()
            if name.startswith("table"):
                gr[0] = 0.0                              # padding_idx 0
                if gate[int(name[-1])] == 0:
                    gr.zero_()                           # zero gate (s_mask) => zero table gradient
            if name == "gate":
                gr = gr * (gate != 0)
            grads.append(gr)
        return [ref.detach()] + grads

    names = ["base"] + [f"table{j}" for j in range(6)] + ["gate", "pos", "ln_w", "ln_b"]
    dev = [t.clone().to(gpu).requires_grad_() for t in [base, *tables, gate, pos, lw, lb]]
    out = ops.seq_embed(dev[0], [i.to(gpu) for i in ids], dev[1:7], dev[7], dev[8], dev[9], dev[10], eps=1e-5,
                        p_drop=p, padding_idx=[0] * 6,
                        tab0_seg=ops.sort_segments(ids[0].to(gpu)) if seg else None)
    (out * dout.float().to(gpu)).sum().backward()
    got = [out] + [t.grad for t in dev]
    refs, bad = reference(seed), reference(seed + 1)
    s = 1.0 / (1.0 - p)
    worst = 0.0
    for name, a, r, rb in zip(["out"] + names, got, refs, bad):
        atol, rtol = (2e-6 * s, 0.0) if name == "out" else (2e-5 * s, 1e-4)
        e = _excess(a, r, atol, rtol)
        worst = max(worst, _excess(a, rb, atol, rtol))
        print(f"seq_embed seg={seg} p={p} {name}: max err {(a.detach().cpu().double() - r).abs().max().item():.3e} "
              f"(atol {atol:.2e}, excess {e:.3f})")
        assert e <= 1.0, (name, e)
    print(f"    control (seed + 1): excess {worst:.1f}")
    assert worst >= 100.0, worst


# ------------------------------------------------------------------ d. the user tower
_TOWER_TORCH_SEED = 9
_FORMS = ("per_op", "native", "tail")


def _tower_tols(p):
    """test_tower_forward_parity's output bound (atol 2e-5, rtol 1e-4) and test_step_losses_and_grads_parity's
    gradient bound (2e-3 * scale + 1e-6), each times (1 / (1 - p))^2: at most two keep scales multiply
    along a branch before the next LayerNorm renormalises (attention then out-projection, or the
    feed-forward's dropout then the residual's)."""
    s2 = (1.0 / (1.0 - p)) ** 2
    return 2e-5 * s2, 1e-4 * s2, 2e-3 * s2, 1e-6 * s2


class _TowerRuns:
    """The device runs (per-op path, native program, native tail form) and the float64 references
    (all rows / tail form) of one dropout rate, computed once per module."""

    def __init__(self, gpu, p):
        self.p = p
        cfg = small_cfg(num_items=500, dropout=p)
        items = small_universe(500)
        batch = to_dev(synth.make_batch(items, 96, seed=21), gpu)
        lookup = items.pretrained.to(gpu)
        from recsys_amd import dist as D
        ix = D.prepare_step_index(batch, pretrained_lookup=lookup)
        pk, pk2, tok_ids, pv, static = ix.packed
        self.layers = cfg.num_layers
        self.T1, self.B = pk.flat.numel(), pk.last_tok.numel()
        self.dev = {}
        for form in _FORMS:
            torch.manual_seed(5)
            model = T.SASRecUserTower(cfg).to(gpu).train()
            prev = ops._TOWER_NATIVE
            ops._TOWER_NATIVE = form != "per_op"
            try:
                assert (ops.tower_native_ok(model, pk2, pv) is not None) == (form != "per_op")
                torch.manual_seed(_TOWER_TORCH_SEED)
                out = model.forward_packed(pk2, pv, tok_ids, *static,
                                           tail_last=pk.last_tok if form == "tail" else None)
                w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
                (out * w.to(gpu)).sum().backward()
            finally:
                ops._TOWER_NATIVE = prev
            torch.cuda.synchronize()
            grads = {n: (q.grad.detach().cpu().double() if q.grad is not None else None)
                     for n, q in model.named_parameters()}
            self.dev[form] = (out.detach().cpu().double(), grads, w)
        self.model = model
        self.seeds = TR.draw_seeds(_TOWER_TORCH_SEED, self.layers, p)
        self.ix = {"all": TR.host_index(pk2, tok_ids, pv, static),
                   "tail": TR.host_index(pk2, tok_ids, pv, static, pk.last_tok)}
        self.ref = {k: TR.run(self.model, self.ix[k], self.layers, p, self.seeds, self.dev["native" if k == "all"
                                                                                          else "tail"][2])
                    for k in ("all", "tail")}

    def excess(self, form, ref):
        """(output excess, worst gradient excess, its name, max output error, max scaled gradient error)."""
        out, grads, _ = self.dev[form]
        r_out, r_grads = ref
        a_o, r_o, g_rel, g_abs = _tower_tols(self.p)
        e_out = _excess(out, r_out, a_o, r_o)
        worst, name, rel = 0.0, None, 0.0
        for n, gr in r_grads.items():
            gd = grads[n] if grads[n] is not None else torch.zeros_like(gr)
            scale = gr.abs().max().item() + 1e-12
            err = (gd - gr).abs().max().item()
            e = err / (g_rel * scale + g_abs)
            rel = max(rel, err / scale)
            if e > worst:
                worst, name = e, n
        return e_out, worst, name, (out - r_out).abs().max().item(), rel


@pytest.fixture(scope="module")
def tower_p0(gpu):
    return _TowerRuns(gpu, 0.0)


@pytest.fixture(scope="module")
def tower_p02(gpu):
    return _TowerRuns(gpu, 0.2)


@pytest.mark.parametrize("form", _FORMS)
def test_tower_p0_against_float64(tower_p0, form):
    """The comparison of test_tower_dropout_against_float64 at p = 0 (all-ones masks), the baseline
    its figures are read against; the p = 0 bounds: output atol 2e-5 / rtol 1e-4, gradients
    2e-3 * scale + 1e-6."""
    r = tower_p0
    e_out, e_grad, name, err, rel = r.excess(form, r.ref["tail" if form == "tail" else "all"])
    print(f"tower p=0 {form}: output max err {err:.3e} (excess {e_out:.3f}); "
          f"worst gradient {name}: err / scale {rel:.3e} (excess {e_grad:.3f})")
    assert e_out <= 1.0 and e_grad <= 1.0, (e_out, e_grad, name)


@pytest.mark.parametrize("form", _FORMS)
def test_tower_dropout_against_float64(tower_p02, form):
    """SASRecUserTower.forward_packed at p = 0.2 (small_cfg(500, dropout=0.2), small_universe(500), 96
    users, both views packed: the setup of test_native_tower_program_equals_per_op_path) against
    tests/tower_dropout_ref.py with every mask rebuilt on the host, output and every parameter
    gradient of sum(out * w): the per-op path and the native program on all rows, and the native tail
    form (tail_last), whose reference keys view 2's kept rows as tower.hip documents (attention by the
    packed query row T1 + last[j]; out-projection dropout, FFN dropout and the closing add by the
    tail index T1 + j). The tail form runs tw_lastq_fwd_k / tw_lastq_bwd_k.

    Seeds: torch.manual_seed(9), then one ops.next_seed() per site in this order: static profile;
    embedding stage (seeds[0]); per layer attention, out-projection, FFN, residual (sd[0..3]); the
    site-to-index-map table is in tests/tower_dropout_ref.py.

    Bounds: the p = 0 bounds times (1 / (1 - p))^2 = 1.5625 (_tower_tols): output atol 3.125e-5 / rtol
    1.5625e-4, gradients 3.125e-3 * scale + 1.5625e-6.
    Measured (MI355X): max output error | worst gradient error / that gradient's scale
      form             p = 0 (bounds 2e-5 + 1e-4|ref| | 2e-3)   p = 0.2 (bounds 3.125e-5 + 1.5625e-4|ref| | 3.125e-3)
      per-op path      5.03e-6 | 2.38e-5                         5.92e-6 | 5.52e-5
      native program   5.03e-6 | 2.38e-5                         5.92e-6 | 5.52e-5
      native tail      5.03e-6 | 5.77e-5                         5.38e-6 | 3.48e-5
    (the worst gradient is static_gate's every time; view 2's kept rows of the tail form alone use
    0.11 of their bound). p = 0.2 needs no more than p = 0 does.
    """
    r = tower_p02
    e_out, e_grad, name, err, rel = r.excess(form, r.ref["tail" if form == "tail" else "all"])
    print(f"tower p=0.2 {form}: output max err {err:.3e} (excess {e_out:.3f}); "
          f"worst gradient {name}: err / scale {rel:.3e} (excess {e_grad:.3f})")
    assert e_out <= 1.0 and e_grad <= 1.0, (e_out, e_grad, name)
    if form == "tail":   # view 2's kept rows alone (the rows no other test compares)
        out, _, _ = r.dev["tail"]
        a_o, r_o, _, _ = _tower_tols(r.p)
        e2 = _excess(out[r.T1:], r.ref["tail"][0][r.T1:], a_o, r_o)
        print(f"    view 2's kept rows: excess {e2:.3f}")
        assert e2 <= 1.0


@pytest.mark.parametrize("form", ["native", "tail"])
@pytest.mark.parametrize("site", TR.site_names(2))
def test_tower_dropout_control(tower_p02, site, form):
    """Negative control per dropout site: the reference with that one site's mask drawn from
    seed + 1 misses the comparison above by at least 100x (host work only: the device results are
    the fixture's)."""
    r = tower_p02
    assert r.layers == 2
    w = r.dev[form][2]
    bad = TR.run(r.model, r.ix["tail" if form == "tail" else "all"], r.layers, r.p, r.seeds, w, wrong=site)
    e_out, e_grad, name, _, _ = r.excess(form, bad)
    print(f"tower control {form} {site}: output excess {e_out:.1f}, gradient excess {e_grad:.1f} ({name})")
    assert max(e_out, e_grad) >= 100.0
