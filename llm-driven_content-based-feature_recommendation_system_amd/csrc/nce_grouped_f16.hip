#include "nce_common.h"
#include "nce_mfma.h"
#include <stdlib.h>

using namespace rsx::nce;

namespace {

// =====================================================================================
// fp16 form of the fused forward and the column pass (precision RSX_NCE_F16).
// Logits: every operand is split into fp16 hi + lo of x * 2^8 (unit-vector components scaled into
// fp16's normal range; lo carries the next 11 bits), S = hi*hi' + hi*lo' + lo*hi' on
// v_mfma_f32_32x32x16_f16 (the GP = 1 column pass: v_mfma_f32_16x16x32_f16) with fp32 accumulation:
// |dot error| ~2^-22 relative per term, tighter than bf16x3 (2^-16) at the same MFMA count; the 2^16
// product scale is folded into 1/tau.
// Gradient products (the softmax weights G against the streamed rows): G rounded to fp16 once and
// multiplied by the rows' fp16 hi image (GP = 1: one MFMA per k-step instead of three) or by hi and
// lo (GP = 2: only G's rounding, 2^-11 relative per weight). This is the reference's own GPU
// arithmetic for these products (autocast(float16), v1_usertower_train.py:787) with fp32
// accumulation; the gradient scales (the 2^8 row scale, the column pass's per-owner factor and
// its 2^14 weight scale) are applied to the fp32 accumulators after the sweep.
// The images keep the bf16x3 layout and LDS tiles (16-bit containers: bf16x8 vectors carry fp16
// bits and are bit-cast at the MFMA); the 16x16x32 column pass has an LDS image of its own.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
constexpr float kHUnscale = 1.0f / 256.0f;
constexpr float kHS2 = 1.0f / 65536.0f;   // S product scale 2^-16
constexpr float kHGS = 14.0f;             // column pass: G weights scaled by 2^14 (<= 16384)
constexpr float kHGSv = 16384.0f;

__device__ __forceinline__ f32x16 mfma_h(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                0);
}

__device__ __forceinline__ uint32_t pack_h(float a, float b) {
  const f16x2 v = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ void load_owner_h(bf16x8 (&uh)[8], bf16x8 (&ul)[8], const float* base, int64_t row,
                                             int64_t ld, bool ok, int h) {
  // all 16 loads issued back to back from a clamped row, then zeroed past the rows (a branch
  // around each pair made hipcc wait for every pair before issuing the next)
  const float4* src = reinterpret_cast<const float4*>(base + (ok ? row : 0) * ld + h * 64);
  float4 v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) v[t] = src[t];
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int s = 0; s < 8; ++s) split8_h(ok ? v[2 * s] : z, ok ? v[2 * s + 1] : z, uh[s], ul[s]);
}

// S tile (dots_x3 on the fp16 MFMA): acc[r] = 2^16 <streamed row tile_row(r,h), owner row c>
__device__ __forceinline__ f32x16 dots_h3(const X3Tile& t, int c, int h, const bf16x8 (&uh)[8],
                                          const bf16x8 (&ul)[8]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int base = img_off(c, 64 * h);
  bf16x8 ah = *reinterpret_cast<const bf16x8*>(&t.hi[base]);
  bf16x8 al = *reinterpret_cast<const bf16x8*>(&t.lo[base]);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    bf16x8 nh = ah, nl = al;
    if (s < 7) {
      nh = *reinterpret_cast<const bf16x8*>(&t.hi[base + 8 * (s + 1)]);
      nl = *reinterpret_cast<const bf16x8*>(&t.lo[base + 8 * (s + 1)]);
    }
    acc = mfma_h(al, uh[s], acc);
    acc = mfma_h(ah, ul[s], acc);
    acc = mfma_h(ah, uh[s], acc);
    __builtin_amdgcn_sched_barrier(0);
    ah = nh;
    al = nl;
  }
  return acc;
}

// g = 2^(x - m) for a pair, summed into sum (fp32, before rounding) and packed as two fp16
__device__ __forceinline__ void exp_h_pair(float a, float b, float m, uint32_t& og, f32x2& sum) {
  f32x2 v = {a, b};
  const f32x2 mm = {m, m};
  v = v - mm;
  v.x = __builtin_amdgcn_exp2f(v.x);
  v.y = __builtin_amdgcn_exp2f(v.y);
  sum = sum + v;
  og = pack_h(v.x, v.y);
}

// grad_half_x3 in fp16: gacc[nb] += G_ks^T X over tile t (nb = 0..3, ks fixed), G one fp16
// fragment; X the streamed rows' hi image (GP = 2: + lo). WORK: the exp / pack of G pair nb of
// half xh of the next operand placed under step nb's MFMAs.
template <bool WORK, int GP>
__device__ __forceinline__ void grad_half_h(f32x16 (&gacc)[4], const bf16x8& g, const X3Tile& t, int base, int ks,
                                            const f32x16& x, int xh, float m, uint32_t (&og)[4], f32x2& sum) {
  bf16x8 bh, bl;
  bh = img_read_tr(t.hi, base, ks, 0);
  if (GP == 2) bl = img_read_tr(t.lo, base, ks, 0);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      nh = img_read_tr(t.hi, base, ks, nb + 1);
      if (GP == 2) nl = img_read_tr(t.lo, base, ks, nb + 1);
    }
    if (GP == 2) gacc[nb] = mfma_h(g, bl, gacc[nb]);
    gacc[nb] = mfma_h(g, bh, gacc[nb]);
    if (WORK) {
      exp_h_pair(x[8 * xh + 2 * nb], x[8 * xh + 2 * nb + 1], m, og[nb], sum);
      asm volatile("" : "+v"(og[nb]));  // pins the work to this step (no sinking)
      __builtin_amdgcn_sched_group_barrier(0x100, 2 * GP, 0);  // next step's transposed reads
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      if (GP == 2) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

// The fused forward (nce_grouped_fwdg_x3p_k's pipeline: 3-slot LDS ring, k-step 1 of each tile's
// gradient product deferred to the next iteration, lazy running max) on the fp16 products.
template <int GP>
__global__ __launch_bounds__(256, 2) void nce_grouped_fwdg_h_k(GArgs a) {
  constexpr int NW = 4, kRows = 32 * NW;
  __shared__ __attribute__((aligned(16))) X3Tile sT[3];
  __shared__ __attribute__((aligned(16))) float sB2[3][kTile];
  __shared__ __attribute__((aligned(16))) float sCnt[3][kTile];
  __shared__ __attribute__((aligned(16))) float sAlpha[NW][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split;
  int64_t rb, j_begin, j_end;
  fwdg_geometry(a, split, rb, j_begin, j_end);
  const int64_t i = rb * kRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  bf16x8 uh[8], ul[8];
  load_owner_h(uh, ul, a.A, i, a.lda, row_ok, h);
  constexpr int kNone = 0x7fffffff;
  int di = -1, p = 0, e = 0, next = kNone;
  if (row_ok) {
    di = a.row_col[i];
    p = a.row_beg[i];
    e = a.row_end[i];
    p = lower_bound_i(a.exc_cols, p, e, j_begin);
    next = (p < e) ? a.exc_cols[p] : kNone;
  }
  const float it2 = a.inv_tau * kLog2e * kHS2;
  float m = -INFINITY, l = 0.0f, lab_x = -INFINITY;
  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;
  X3Stage stg;
  float stg_b = 0.0f, stg_c = 0.0f;
  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + ((tid >> 3) & 31);
    stg.load(a.bhi, a.blo, j, j < j_end, tid);
    stage_bias_count_load(a, j0, j_end, tid, stg_b, stg_c);
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    stage_bias_count_store(sB2[buf], sCnt[buf], tid, stg_b, stg_c);
  };
  if (j_begin < j_end) {
    gload(j_begin);
    lstore(0);
    __syncthreads();
    int cur = 0, prev = 0;
    bf16x8 pg;
#pragma unroll
    for (int k = 0; k < 8; ++k) pg[k] = (__bf16)0.0f;  // zero bits = fp16 zero
    const int gbase = img_tr_base(lane);
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kTile) {
      const bool has_next = j0 + kTile < j_end;
      const bool exc = (int64_t)next < j0 + kTile;
      if (has_next) gload(j0 + kTile);
      f32x16 acc = dots_h3(sT[cur], c, h, uh, ul);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 nb = *reinterpret_cast<const float4*>(&sB2[cur][8 * g + 4 * h]);
        acc[4 * g + 0] = fmaf(acc[4 * g + 0], it2, nb.x);
        acc[4 * g + 1] = fmaf(acc[4 * g + 1], it2, nb.y);
        acc[4 * g + 2] = fmaf(acc[4 * g + 2], it2, nb.z);
        acc[4 * g + 3] = fmaf(acc[4 * g + 3], it2, nb.w);
      }
      if (exc) {
        int q = p;
        while (q < e && (int64_t)a.exc_cols[q] < j0 + kTile) ++q;
        float n[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) n[r] = 0.0f;
        for (int k = p; k < q; ++k) {
          const int tk = (int)(a.exc_cols[k] - j0);
#pragma unroll
          for (int r = 0; r < 16; ++r) n[r] += (tk == tile_row(r, h)) ? 1.0f : 0.0f;
        }
        const int tl = ((int64_t)di < j_end) ? (int)(di - j0) : -1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 cw = *reinterpret_cast<const float4*>(&sCnt[cur][8 * g + 4 * h]);
          const float cv[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int r = 4 * g + t;
            const float wn = (tile_row(r, h) == tl) ? 1.0f : cv[t] - n[r];
            if (wn != cv[t]) acc[r] = (wn > 0.0f) ? acc[r] + __log2f(wn / cv[t]) : -INFINITY;
            if (tile_row(r, h) == tl) lab_x = acc[r];  // the label's logit (weight 1), see below
          }
        }
        p = q;
        next = (p < e) ? a.exc_cols[p] : kNone;
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, acc[r]);
      {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      if (!row_ok) tmax = -INFINITY;
      const bool raise = tmax > m + kLazyLog2;
      if (__any(raise)) {
        {
          uint32_t dg[4];
          f32x2 ds = {0.0f, 0.0f};
          grad_half_h<false, GP>(gacc, pg, sT[prev], gbase, 1, acc, 0, 0.0f, dg, ds);
#pragma unroll
          for (int k = 0; k < 8; ++k) pg[k] = (__bf16)0.0f;
        }
        const float alpha = raise ? ((m == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(m - tmax)) : 1.0f;
        if (raise) {
          l *= alpha;
          m = tmax;
        }
        if (h == 0) sAlpha[wave][c] = alpha;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float al = sAlpha[wave][tile_row(r, h)];
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) gacc[kb][r] *= al;
        }
        __builtin_amdgcn_wave_barrier();
      }
      const float ms = (m == -INFINITY) ? 0.0f : m;
      if (lab_x != -INFINITY) {
        // the label column enters the sum l here and is left out of the gradient product: the merge
        // adds its term as (p_pos - 1) B_d(i) in fp32 (near convergence p_pos B_d(i) and the label's
        // -B_d(i) cancel, and an fp16-rounded p_pos B_d(i) would leave a 2^-12 |B| residue)
        l += __builtin_amdgcn_exp2f(lab_x - ms);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (tile_row(r, h) == (int)(di - j0)) acc[r] = -INFINITY;
        lab_x = -INFINITY;
      }
      uint32_t g0[4], g1[4];
      f32x2 sum = {0.0f, 0.0f};
      grad_half_h<true, GP>(gacc, pg, sT[prev], gbase, 1, acc, 0, ms, g0, sum);
      const u32x4 g0v = {g0[0], g0[1], g0[2], g0[3]};
      grad_half_h<true, GP>(gacc, __builtin_bit_cast(bf16x8, g0v), sT[cur], gbase, 0, acc, 1, ms, g1, sum);
      l += sum.x + sum.y;
      const u32x4 g1v = {g1[0], g1[1], g1[2], g1[3]};
      pg = __builtin_bit_cast(bf16x8, g1v);
      prev = cur;
      const int nxt = (cur == 2) ? 0 : cur + 1;
      if (has_next) lstore(nxt);
      __builtin_amdgcn_s_waitcnt(kVmcnt0);
      __syncthreads();
      cur = nxt;
    }
    {
      uint32_t dg[4];
      f32x2 ds = {0.0f, 0.0f};
      f32x16 z;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.0f;
      grad_half_h<false, GP>(gacc, pg, sT[prev], gbase, 1, z, 0, 0.0f, dg, ds);
    }
  }
  const float lt = l + __shfl_xor(l, 32, 64);
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)a.nslots * a.N;
    const int64_t o = (int64_t)split * a.N + i;
    a.part[o] = (m == -INFINITY) ? -INFINITY : m * kLn2;
    a.part[stride + o] = lt;
    a.part[2 * stride + o] = 0.0f;
    a.part[3 * stride + o] = 0.0f;
  }
  // not on store_d_own: with it hipcc allocates this kernel's registers differently (GP = 1)
  const int64_t own_base = rb * kRows + wave * 32;
  float* dst = a.dout + (int64_t)split * a.N * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < a.N) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r] * kHUnscale;
    }
  }
}

// k-step ks of the column pass's gradient product in fp16, gacc[nb] += G'_ks^T X, with (WORK) the
// next k-step's G' pair nb: G' = 2^14 min(c_o p1, 1), c_o p1 = 2^(S it2 - m0 - bias_o) c_o = 2^(S it2 -
// (m0 + o_m2s)) / 2^14: row i's softmax mass on target o when (i, o) is not an exception pair (<= 1: lse_i
// sums every column with its multiplicity); on exception pairs (same user / label, where the true weight
// is below c_o) the clamp keeps the term finite and within 1, and the exception product replaces it.
// The uniform factor gout / tau and the 2^-14 scale are applied after the sweep
template <bool WORK, int GP>
__device__ __forceinline__ void grad_half_gh(f32x16 (&gacc)[4], const bf16x8& g, const X3Tile& t, int base, int ks,
                                             const f32x16& S, int h, const float* m0, float o_m2s, float it2,
                                             uint32_t (&og)[4]) {
  bf16x8 bh, bl;
  bh = img_read_tr(t.hi, base, ks, 0);
  if (GP == 2) bl = img_read_tr(t.lo, base, ks, 0);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      nh = img_read_tr(t.hi, base, ks, nb + 1);
      if (GP == 2) nl = img_read_tr(t.lo, base, ks, nb + 1);
    }
    if (GP == 2) gacc[nb] = mfma_h(g, bl, gacc[nb]);
    gacc[nb] = mfma_h(g, bh, gacc[nb]);
    if (WORK) {
      const int pp = 4 + nb;  // rows 2pp, 2pp+1
      const f32x4 q0 = *reinterpret_cast<const f32x4*>(m0 + 8 * (pp >> 1) + 4 * h);
      float gp[2];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int r = 2 * pp + rr, e = r & 3;
        gp[rr] = fminf(__builtin_amdgcn_exp2f(fmaf(S[r], it2, -(q0[e] + o_m2s))), kHGSv);
      }
      og[nb] = pack_h(gp[0], gp[1]);
      asm volatile("" : "+v"(og[nb]));
    }
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

// Column pass of the grouped backward on the fp16 products: owner = distinct target column o (its fp16
// hi/lo fragments in registers), streamed = user rows (A's fp16 images). Every (row, column) pair is
// first taken with the common weight G' = 2^14 min(c_o p1_io, 1) (p1 = one column instance's softmax
// probability; the clamp only acts on exception pairs); on the rare tiles where the owner's same-user
// rows or label rows appear (the user-range lists exc_s / exc_e / exc_n), a second product adds
// dG' = G'_exact - G'_common for those pairs, formed from the same S tile in fp32 before its one
// rounding (v1_refine_usertower.py:846-858: same-user mask, label column). The correction runs after
// the common product, when its G fragments are dead: folded into the common product, the exception
// bookkeeping needs ~60 more VGPRs than the 256 a two-wave-per-SIMD kernel has (and with the owner
// fragments moved to LDS instead the pass is LDS-bound).
// This 32x32x16 form serves RSX_NCE_F16_GP = 2 (three S products, gradient products on the rows' hi and
// lo images); the shipped GP = 1 pass is nce_grouped_bwd_cols_h16_k below.
template <int GP>
__global__ __launch_bounds__(256, 2) void nce_grouped_bwd_cols_h_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) X3Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // lse_i * log2e (+inf past the split)
  __shared__ __attribute__((aligned(16))) int sM2[2][kTile];    // d(i) (-2 past the split)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, ob;
  const int64_t n_own = a.M, n_str = a.N;
  if (a.split_major) {
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    const int nob = (int)((n_own + kOwnRows - 1) / kOwnRows);
    split = xcd + 8 * (q / nob);
    ob = q % nob;
  } else {
    remap_block(a.nsplit, split, ob);
  }
  const float gs = a.gout[0] * a.inv_tau;
  const float it2 = a.inv_tau * kLog2e * kHS2;
  const int64_t o = (int64_t)ob * kOwnRows + wave * 32 + c;
  const bool own_ok = o < n_own;
  bf16x8 uh[8], ul[8];
  load_owner_h(uh, ul, a.B, o, a.ldb, own_ok, h);
  const int64_t s_begin = (int64_t)split * a.span;
  int64_t s_end = s_begin + a.span;
  if (s_end > n_str) s_end = n_str;
  constexpr int kNone = 0x7fffffff;
  // exponent offset of G' = 2^14 c_o 2^(x): bias_o log2e - log2 c_o - 14 (no owner: +inf -> G' = 0)
  float o_m2s = INFINITY, o_cnt = 0.0f;
  int p = 0, e = 0;
  if (own_ok) {
    o_cnt = a.colcnt[o];
    o_m2s = (a.bias ? a.bias[o] * kLog2e : 0.0f) - __log2f(o_cnt) - kHGS;
    p = a.col_beg[o];
    e = a.col_end[o];
    p = lower_bound_i(a.exc_e, p, e, s_begin + 1);  // first user range ending after s_begin
  }
  int q = p, e_first = 0, s_next = kNone;
  if (own_ok && q < e) s_next = a.exc_s[q];

  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;

  X3Stage stg;
  float stg0 = 0.0f;
  int stg2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load(a.ahi, a.alo, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      stg0 = ok ? a.lse[ss] : INFINITY;
      stg2 = ok ? a.row_col[ss] : -2;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sM0[buf][tid] = stg0 * kLog2e;
      sM2[buf][tid] = stg2;
    }
  };
  // user row ranges [p, q) of the owner's column intersecting tile s0 (before the prefetch: may load)
  auto exc_flag = [&](int64_t s0) -> bool {
    while (p < q && (int64_t)e_first <= s0) {
      ++p;
      if (p < q) e_first = a.exc_e[p];
    }
    while ((int64_t)s_next < s0 + kTile) {
      if (p == q) e_first = a.exc_e[q];
      ++q;
      s_next = (q < e) ? a.exc_s[q] : kNone;
    }
    return q != p;
  };

  if (s_begin < s_end) {
    const int ntile = (int)((s_end - s_begin + kTile - 1) / kTile);
    gload(s_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    const int gbase = img_tr_base(lane);
    for (int t = 0; t < ntile; ++t) {
      const int64_t s0 = s_begin + (int64_t)t * kTile;
      const bool has_next = t + 1 < ntile;
      const bool exc = exc_flag(s0);
      if (has_next) gload(s0 + kTile);
      f32x16 acc = dots_h3(sT[cur], c, h, uh, ul);
      // G' rows of k-step 0, then k-step 0's product with k-step 1's rows under its MFMAs
      u32x4 g0;
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(&sM0[cur][8 * (pp >> 1) + 4 * h]);
        float gp[2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int r = 2 * pp + rr, ee = r & 3;
          gp[rr] = fminf(__builtin_amdgcn_exp2f(fmaf(acc[r], it2, -(q0[ee] + o_m2s))), kHGSv);
        }
        g0[pp] = pack_h(gp[0], gp[1]);
      }
      uint32_t g1[4];
      grad_half_gh<true, GP>(gacc, __builtin_bit_cast(bf16x8, g0), sT[cur], gbase, 0, acc, h, sM0[cur], o_m2s, it2,
                             g1);
      const u32x4 g1v = {g1[0], g1[1], g1[2], g1[3]};
      grad_half_gh<false, GP>(gacc, __builtin_bit_cast(bf16x8, g1v), sT[cur], gbase, 1, acc, h, sM0[cur], o_m2s, it2,
                              g1);
      if (__any(exc)) {
        // dG' = 2^14 (w p1 - lab) - 2^14 min(c_o p1, 1) on the owner's exception rows (0 elsewhere):
        // w = c_o - n (the user's own rows of target o) or 1 (label), from the same S as the common term
        float n[16];  // multiplicity n of the user range holding streamed row tr (0: none)
#pragma unroll
        for (int r = 0; r < 16; ++r) n[r] = 0.0f;
        if (exc) {
          for (int k = p; k < q; ++k) {  // each range's bounds loaded once
            const int ks = (int)(a.exc_s[k] - s0), ke = (int)(a.exc_e[k] - s0);
            const float nk = (float)a.exc_n[k];
#pragma unroll
            for (int r = 0; r < 16; ++r) n[r] += (tile_row(r, h) >= ks && tile_row(r, h) < ke) ? nk : 0.0f;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tr = tile_row(r, h);
          const float nr = n[r];
          const bool lab = exc && sM2[cur][tr] == (int)o;
          float dg = 0.0f;
          if (exc && (nr > 0.0f || lab)) {
            const float ex = __builtin_amdgcn_exp2f(fmaf(acc[r], it2, -(sM0[cur][tr] + o_m2s)));  // 2^14 c_o p1
            const float rc = __builtin_amdgcn_rcpf(o_cnt);
            const float w = lab ? 1.0f : fmaxf(o_cnt - nr, 0.0f);
            dg = (w * rc) * ex - (lab ? kHGSv : 0.0f) - fminf(ex, kHGSv);
          }
          acc[r] = dg;
        }
        u32x4 d0, d1;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          d0[qq] = pack_h(acc[2 * qq], acc[2 * qq + 1]);
          d1[qq] = pack_h(acc[8 + 2 * qq], acc[8 + 2 * qq + 1]);
        }
        grad_half_gh<false, GP>(gacc, __builtin_bit_cast(bf16x8, d0), sT[cur], gbase, 0, acc, h, sM0[cur], o_m2s, it2,
                                g1);
        grad_half_gh<false, GP>(gacc, __builtin_bit_cast(bf16x8, d1), sT[cur], gbase, 1, acc, h, sM0[cur], o_m2s, it2,
                                g1);
      }
      if (has_next) lstore(cur ^ 1);
      __builtin_amdgcn_s_waitcnt(kVmcnt0);
      __syncthreads();
      cur ^= 1;
    }
  }
  // scale: gout / tau, the 2^-8 row scale and the 2^-14 weight scale
  store_d_own<true>((int64_t)ob * kOwnRows + wave * 32, a.dout + (int64_t)split * n_own * kD, n_own, h, c, gacc,
                    gs * (kHUnscale / kHGSv));
}

// =====================================================================================
// The GP = 1 column pass (the shipped one) on v_mfma_f32_16x16x32_f16: nce_grouped_bwd_cols_h_k's
// pass in 16x16 accumulator blocks, with two S products, hi*hi' + hi*lo' (streamed hi against the
// owner's hi and lo): with one gradient product on the hi image as well, the streamed rows' lo image is
// neither staged nor read. |dot error| = |<lo, owner>| ~ 2^-11 |x| per component with random signs, ~2e-5
// on unit vectors (the pass outputs gradients only, 1e-3 of scale; the logits of the loss keep three
// products in the forward); grad_b's deviation from fp32 is that of three products (4.897e-4 vs
// 4.899e-4 of scale, tools/nce_micro.py --compare). A wave owns 32 columns and streams 32-row tiles;
// a lane (i = lane & 15, g = lane >> 4) serves owner columns i and 16 + i, and everything per owner
// (exponent offset, count, exception cursor) is held twice.
// Exception pairs (the owner's same-user rows and label rows) do not take a second product here: on
// the rare tiles that hold some, their exact weight 2^14 (w p1 - lab), formed in fp32 from the same S,
// replaces the common weight in the G' fragment before the one gradient product, so it is rounded to
// fp16 once at its own magnitude; a label pair's p - 1 comes from the forward's row loss lse_i - s_ii. (Common weight plus a correction product, as in the 32x32 form,
// rounds two values of magnitude 2^14 whose sum on a label pair is 2^14 (p - 1): an absolute floor of
// ~3e-4 per label row, 1e-2 of a near-converged batch's column gradient.)
//   S block (sh, b): streamed rows 16sh .. 16sh+15 x owner columns 16b .. 16b+15, 4 k-steps of 32
//             dims, 2 products each. Operands: lane (i, g) holds dims 32ks + 8g + j of streamed row
//             16sh + i (A) and of owner column 16b + i (B); accumulator register r is streamed row
//             16sh + 4g + r, owner column 16b + i.
//   gradient: K = the tile's 32 streamed rows, one k-step: for owner half b the A fragment is the
//             lane's own G' of blocks (0, b) and (1, b), i.e. k element j = streamed row
//             16(j>>2) + 4g + (j&3), and the B fragment of dims 16nb .. 16nb+15 is read transposed
//             in the same k order (two 4-row blocks 16 rows apart). gacc[b][nb] register r is owner
//             column 16b + 4g + r, dim 16nb + i.
// The S of streamed half 0 is complete after half of the tile's S MFMAs, and its G' work is issued
// under the S MFMAs of half 1.
// LDS image of the hi tile (the lo image is not staged): plain 288-B rows, no skew; conflict-free
// for the 16-row fragment reads (ds_read_b128: row i, 16-B chunk 4ks + g), the transposed reads
// and the staging stores (tools/lds_banks.py, "16x16x32 column pass").
constexpr int kImg16Row = 144;  // fp16 elements per image row
__device__ __forceinline__ int img16_off(int row, int col) { return row * kImg16Row + col; }
struct H16Tile {
  __bf16 hi[kTile * kImg16Row];
};

__device__ __forceinline__ f32x4 mfma_h16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                0);
}

// transposed fragment of dims 16nb .. 16nb+15: rows 4g .. 4g+3 and 16 + 4g .. 16 + 4g+3 from the
// lane's base offset img16_off(4g + q, 4p) (lane = 16g + 4q + p)
__device__ __forceinline__ bf16x8 img16_read_tr(const __bf16* img, int base, int nb) {
  const int o0 = base + img16_off(0, 16 * nb), o1 = base + img16_off(16, 16 * nb);
  const rsx::bf16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((rsx::lds_bf16x4*)(&img[o0]));
  const rsx::bf16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((rsx::lds_bf16x4*)(&img[o1]));
  return __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// owner columns row0 + 16b + i (b = 0, 1): fragment [b][ks] = dims 32ks + 8g .. 32ks + 8g+7
__device__ __forceinline__ void load_owner_h16(bf16x8 (&uh)[2][4], bf16x8 (&ul)[2][4], const float* base,
                                               const int64_t (&row)[2], int64_t ld, const bool (&ok)[2], int g) {
  float4 v[16];  // all loads issued from clamped rows, then zeroed past the rows (load_owner_h)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const float* src = base + (ok[b] ? row[b] : 0) * ld + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      v[8 * b + 2 * ks] = *reinterpret_cast<const float4*>(src + 32 * ks);
      v[8 * b + 2 * ks + 1] = *reinterpret_cast<const float4*>(src + 32 * ks + 4);
    }
  }
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      split8_h(ok[b] ? v[8 * b + 2 * ks] : z, ok[b] ? v[8 * b + 2 * ks + 1] : z, uh[b][ks], ul[b][ks]);
}

// G' pair of one lane: 2^14 min(c_o p1, 1) of two logits, packed as fp16 (grad_half_gh's arithmetic)
__device__ __forceinline__ uint32_t gprime_pair(float s0, float s1, float q0, float q1, float o_m2s, float it2) {
  const float a = fminf(__builtin_amdgcn_exp2f(fmaf(s0, it2, -(q0 + o_m2s))), kHGSv);
  const float b = fminf(__builtin_amdgcn_exp2f(fmaf(s1, it2, -(q1 + o_m2s))), kHGSv);
  return pack_h(a, b);
}

// S blocks (sh, 0) and (sh, 1) from two fp16 products, hi*lo' then hi*hi' per k-step.
// WORK: the G' pairs of the previous half's blocks prev[0], prev[1] (its row offsets pm), one pair
// under each k-step's four MFMAs: og[2b + t] = rows 2t, 2t+1 of block b, pair 2b + t at step 2b + t
template <bool WORK>
__device__ __forceinline__ void dots_h16(f32x4 (&acc)[2], const H16Tile& t, int fbase, int sh,
                                         const bf16x8 (&uh)[2][4], const bf16x8 (&ul)[2][4], const f32x4 (&prev)[2],
                                         const f32x4& pm, const float (&o_m2s)[2], float it2, uint32_t (&og)[4]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[b][r] = 0.0f;
  const int base = fbase + img16_off(16 * sh, 0);
  bf16x8 a = *reinterpret_cast<const bf16x8*>(&t.hi[base]);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    bf16x8 n = a;
    if (ks < 3) n = *reinterpret_cast<const bf16x8*>(&t.hi[base + 32 * (ks + 1)]);
    acc[0] = mfma_h16(a, ul[0][ks], acc[0]);
    acc[1] = mfma_h16(a, ul[1][ks], acc[1]);
    acc[0] = mfma_h16(a, uh[0][ks], acc[0]);
    acc[1] = mfma_h16(a, uh[1][ks], acc[1]);
    if (WORK) {
      const int b = ks >> 1, r = 2 * (ks & 1);
      og[ks] = gprime_pair(prev[b][r], prev[b][r + 1], pm[r], pm[r + 1], o_m2s[b], it2);
      asm volatile("" : "+v"(og[ks]));  // pins the work to this step (no sinking)
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // next step's fragment read
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    a = n;
  }
}

// gacc[b][nb] += G'_b^T X over the tile's 32 rows (one k-step), nb = 0..7
__device__ __forceinline__ void grad_h16(f32x4 (&gacc)[2][8], const bf16x8 (&g)[2], const H16Tile& t, int tbase) {
  bf16x8 x = img16_read_tr(t.hi, tbase, 0);
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
    bf16x8 n = x;
    if (nb < 7) n = img16_read_tr(t.hi, tbase, nb + 1);
    gacc[0][nb] = mfma_h16(g[0], x, gacc[0][nb]);
    gacc[1][nb] = mfma_h16(g[1], x, gacc[1][nb]);
    __builtin_amdgcn_sched_barrier(0);
    x = n;
  }
}

__global__ __launch_bounds__(256, 2) void nce_grouped_bwd_cols_h16_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) H16Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // lse_i * log2e (+inf past the split)
  __shared__ __attribute__((aligned(16))) int sM2[2][kTile];    // d(i) (-2 past the split)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  int split, ob;
  const int64_t n_own = a.M, n_str = a.N;
  if (a.split_major) {
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    const int nob = (int)((n_own + kOwnRows - 1) / kOwnRows);
    split = xcd + 8 * (q / nob);
    ob = q % nob;
  } else {
    remap_block(a.nsplit, split, ob);
  }
  const float gs = a.gout[0] * a.inv_tau;
  const float it2 = a.inv_tau * kLog2e * kHS2;
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  const int64_t o[2] = {own_base + i, own_base + 16 + i};
  const bool own_ok[2] = {o[0] < n_own, o[1] < n_own};
  bf16x8 uh[2][4], ul[2][4];
  load_owner_h16(uh, ul, a.B, o, a.ldb, own_ok, g);
  const int64_t s_begin = (int64_t)split * a.span;
  int64_t s_end = s_begin + a.span;
  if (s_end > n_str) s_end = n_str;
  constexpr int kNone = 0x7fffffff;
  // exponent offset of G' = 2^14 c_o 2^(x): bias_o log2e - log2 c_o - 14 (no owner: +inf -> G' = 0)
  float o_m2s[2] = {INFINITY, INFINITY}, o_cnt[2] = {0.0f, 0.0f};
  int p[2] = {0, 0}, e[2] = {0, 0}, q[2], e_first[2] = {0, 0}, s_next[2] = {kNone, kNone};
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    if (own_ok[b]) {
      o_cnt[b] = a.colcnt[o[b]];
      o_m2s[b] = (a.bias ? a.bias[o[b]] * kLog2e : 0.0f) - __log2f(o_cnt[b]) - kHGS;
      p[b] = a.col_beg[o[b]];
      e[b] = a.col_end[o[b]];
      p[b] = lower_bound_i(a.exc_e, p[b], e[b], s_begin + 1);  // first user range ending after s_begin
    }
    q[b] = p[b];
    if (own_ok[b] && q[b] < e[b]) s_next[b] = a.exc_s[q[b]];
  }

  f32x4 gacc[2][8];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) gacc[b][nb][r] = 0.0f;

  X3Stage stg;
  float stg0 = 0.0f;
  int stg2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load_hi(a.ahi, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      stg0 = ok ? a.lse[ss] : INFINITY;
      stg2 = ok ? a.row_col[ss] : -2;
    }
  };
  auto lstore = [&](int buf) {
    const int row = tid >> 3, ch = tid & 7;
    *reinterpret_cast<u32x4*>(&sT[buf].hi[img16_off(row, 8 * ch)]) = stg.v[0];
    *reinterpret_cast<u32x4*>(&sT[buf].hi[img16_off(row, 64 + 8 * ch)]) = stg.v[1];
    if (tid < kTile) {
      sM0[buf][tid] = stg0 * kLog2e;
      sM2[buf][tid] = stg2;
    }
  };
  // user row ranges [p, q) of owner column b intersecting tile s0 (before the prefetch: may load)
  auto exc_flag = [&](int b, int64_t s0) -> bool {
    while (p[b] < q[b] && (int64_t)e_first[b] <= s0) {
      ++p[b];
      if (p[b] < q[b]) e_first[b] = a.exc_e[p[b]];
    }
    while ((int64_t)s_next[b] < s0 + kTile) {
      if (p[b] == q[b]) e_first[b] = a.exc_e[q[b]];
      ++q[b];
      s_next[b] = (q[b] < e[b]) ? a.exc_s[q[b]] : kNone;
    }
    return q[b] != p[b];
  };

  if (s_begin < s_end) {
    const int ntile = (int)((s_end - s_begin + kTile - 1) / kTile);
    gload(s_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    const int fbase = img16_off(i, 8 * g);
    const int tbase = img16_off(4 * g + (i >> 2), 4 * (i & 3));
    for (int t = 0; t < ntile; ++t) {
      const int64_t s0 = s_begin + (int64_t)t * kTile;
      const bool has_next = t + 1 < ntile;
      const bool exc[2] = {exc_flag(0, s0), exc_flag(1, s0)};
      if (has_next) gload(s0 + kTile);
      // lse offsets of the lane's streamed rows 4g .. 4g+3 and 16 + 4g .. 16 + 4g+3
      const f32x4 m0 = *reinterpret_cast<const f32x4*>(&sM0[cur][4 * g]);
      const f32x4 m1 = *reinterpret_cast<const f32x4*>(&sM0[cur][16 + 4 * g]);
      f32x4 S0[2], S1[2];
      uint32_t g0[4], g1[4];
      dots_h16<false>(S0, sT[cur], fbase, 0, uh, ul, S0, m0, o_m2s, it2, g0);
      dots_h16<true>(S1, sT[cur], fbase, 1, uh, ul, S0, m0, o_m2s, it2, g0);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
          g1[2 * b + tt] = gprime_pair(S1[b][2 * tt], S1[b][2 * tt + 1], m1[2 * tt], m1[2 * tt + 1], o_m2s[b], it2);
      // A fragments of the gradient product: element j of gf[b] = G' of streamed row 16(j>>2) + 4g + (j&3)
      const u32x4 f0 = {g0[0], g0[1], g1[0], g1[1]}, f1 = {g0[2], g0[3], g1[2], g1[3]};
      f16x8 gf[2] = {__builtin_bit_cast(f16x8, f0), __builtin_bit_cast(f16x8, f1)};
      if (__any(exc[0] || exc[1])) {
        // the owners' exception rows take their exact weight 2^14 (w p1 - lab) in place of the common one:
        // w = c_o - n (the user's own rows of target o) or 1 (label), from the same S, rounded to fp16 once
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          float n[8];  // multiplicity n of the user range holding streamed row 16(k>>2) + 4g + (k&3) (0: none)
#pragma unroll
          for (int k = 0; k < 8; ++k) n[k] = 0.0f;
          if (exc[b]) {
            for (int k = p[b]; k < q[b]; ++k) {  // each range's bounds loaded once
              const int ks = (int)(a.exc_s[k] - s0), ke = (int)(a.exc_e[k] - s0);
              const float nk = (float)a.exc_n[k];
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const int tr = 16 * (r >> 2) + 4 * g + (r & 3);
                n[r] += (tr >= ks && tr < ke) ? nk : 0.0f;
              }
            }
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int tr = 16 * (r >> 2) + 4 * g + (r & 3);
            const float s = (r < 4) ? S0[b][r & 3] : S1[b][r & 3];
            const bool lab = exc[b] && sM2[cur][tr] == (int)o[b];
            if (exc[b] && (n[r] > 0.0f || lab)) {
              const float ex = __builtin_amdgcn_exp2f(fmaf(s, it2, -(sM0[cur][tr] + o_m2s[b])));  // 2^14 c_o p1
              const float rc = __builtin_amdgcn_rcpf(o_cnt[b]);
              const float w = lab ? 1.0f : fmaxf(o_cnt[b] - n[r], 0.0f);
              // (c_o - n) p1 <= 1: lse_i holds the column's other c_o - n instances; no instance left: 0
              // label pair: p - 1 = expm1(-(lse_i - s_ii)) from the forward's fp32 label logit (this pass's
              // two-product S leaves ~2e-4 on the logit, which is all of p - 1's error once p is near 1)
              const float ge = lab ? kHGSv * expm1f(-a.row_loss[s0 + tr])
                                   : ((w > 0.0f) ? fminf((w * rc) * ex, kHGSv) : 0.0f);
              gf[b][r] = (_Float16)ge;
            }
          }
        }
      }
      {
        const bf16x8 ga[2] = {__builtin_bit_cast(bf16x8, gf[0]), __builtin_bit_cast(bf16x8, gf[1])};
        grad_h16(gacc, ga, sT[cur], tbase);
      }
      if (has_next) lstore(cur ^ 1);
      __builtin_amdgcn_s_waitcnt(kVmcnt0);
      __syncthreads();
      cur ^= 1;
    }
  }
  // scale: gout / tau, the 2^-8 row scale and the 2^-14 weight scale
  const float scale = gs * (kHUnscale / kHGSv);
  float* dst = a.dout + (int64_t)split * n_own * kD;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t orow = own_base + 16 * b + 4 * g + r;
      if (orow < n_own) {
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) dst[orow * kD + 16 * nb + i] = gacc[b][nb][r] * scale;
      }
    }
}

// RSX_NCE_F16_GP = 1 | 2: MFMAs per gradient-product k-step in the fp16 kernels (default 1)
int f16_gp() {
  static const int v = [] {
    const char* e = getenv("RSX_NCE_F16_GP");
    return (e && e[0] == '2') ? 2 : 1;
  }();
  return v;
}

}  // namespace

void rsx::nce::launch_grouped_fwdg_h(const GArgs& g, int blocks, hipStream_t st) {
  if (f16_gp() == 2) hipLaunchKernelGGL(nce_grouped_fwdg_h_k<2>, dim3(blocks), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(nce_grouped_fwdg_h_k<1>, dim3(blocks), dim3(256), 0, st, g);
}

void rsx::nce::launch_grouped_bwd_cols_h(const GArgs& g, int blocks, hipStream_t st) {
  if (f16_gp() == 2) hipLaunchKernelGGL(nce_grouped_bwd_cols_h_k<2>, dim3(blocks), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(nce_grouped_bwd_cols_h16_k, dim3(blocks), dim3(256), 0, st, g);
}
