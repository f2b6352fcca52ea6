// Grouped form of the live LogQ loss (GArgs in nce_common.h), fp32 and bf16x3; fp16: nce_grouped_f16.hip.
#include "nce_common.h"
#include "nce_mfma.h"
#include <mutex>
#include <utility>
#include <vector>

using namespace rsx::nce;

namespace {

// Row-side weights for the tile [d0, d0+32): w[r] = multiplicity of column d0 + tile_row(r,h)
// for row i (0 => excluded). p/next walk the row's sorted exception list.
__device__ __forceinline__ void row_weights(float (&w)[16], const float* s_cnt, int64_t d0, int64_t d_end, int h,
                                            int di, const int* exc, int& p, int e, int& next) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t d = d0 + tile_row(r, h);
    float cw = s_cnt[tile_row(r, h)];
    if (d == di) cw = 1.0f;
    w[r] = (d < d_end) ? cw : 0.0f;
  }
  if ((int64_t)next < d0 + kTile) {  // rare: some of the user's own targets fall in this tile
    int q = p;
    while (q < e && (int64_t)exc[q] < d0 + kTile) ++q;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (int)(d0 + tile_row(r, h));
      int c = 0;
      for (int k = p; k < q; ++k) c += (exc[k] == d);
      if (d != di) w[r] -= (float)c;
    }
    p = q;
    next = (p < e) ? exc[p] : 0x7fffffff;
  }
}

__global__ __launch_bounds__(256, 2) void nce_grouped_fwd_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) F32Prod::Tile sB[2];
  __shared__ __attribute__((aligned(16))) float sBias[2][kTile];
  __shared__ __attribute__((aligned(16))) float sCnt[2][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  F32Prod::Owner own;
  F32Prod::load_owner(own, {}, a.A, i, a.lda, row_ok, h);
  const int64_t j_begin = (int64_t)split * a.span;
  int64_t j_end = j_begin + a.span;
  if (j_end > a.M) j_end = a.M;
  int di = -1, p = 0, e = 0, next = 0x7fffffff;
  if (row_ok) {
    di = a.row_col[i];
    p = a.row_beg[i];
    e = a.row_end[i];
    p = lower_bound_i(a.exc_cols, p, e, j_begin);
    next = (p < e) ? a.exc_cols[p] : 0x7fffffff;
  }
  float m = -INFINITY, l = 0.0f;
  F32Prod::Stage stg = F32Prod::stage(tid);
  float stg_b = 0.0f, stg_c = 0.0f;
  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + (tid >> 3);
    stg.load({a.B, a.ldb}, j, j < j_end, tid);
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_b = (ok && a.bias) ? a.bias[jj] : 0.0f;
      stg_c = ok ? a.colcnt[jj] : 0.0f;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sB[buf], tid);
    if (tid < kTile) {
      sBias[buf][tid] = stg_b;
      sCnt[buf][tid] = stg_c;
    }
  };
  if (j_begin < j_end) {
    gload(j_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kTile) {
      const bool has_next = j0 + kTile < j_end;
      if (has_next) gload(j0 + kTile);
      const f32x16 acc = F32Prod::dots(sB[cur], own, {}, c, h);
      float w[16];
      row_weights(w, sCnt[cur], j0, j_end, h, di, a.exc_cols, p, e, next);
      float v[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        v[r] = acc[r] * a.inv_tau - sBias[cur][tile_row(r, h)];
        if (w[r] > 0.0f) tmax = fmaxf(tmax, v[r]);
      }
      if (!row_ok) tmax = -INFINITY;
      if (tmax > m) {
        l = (m == -INFINITY) ? 0.0f : l * __expf(m - tmax);
        m = tmax;
      }
      if (m != -INFINITY) {
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += (w[r] > 0.0f) ? w[r] * __expf(v[r] - m) : 0.0f;
        l += t;
      }
      __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  fold_store_partials<false>(a.part, a.nsplit, split, a.N, i, row_ok, h, m, l, 0.0f, 0.0f);
}

// merge for the grouped form: S_ii = <A_i, B_{d(i)}>/tau - bias_{d(i)}
__global__ __launch_bounds__(256) void nce_grouped_merge_k(const float* A, const float* B, const float* bias,
                                                           const int* row_col, int64_t N, int64_t lda,
                                                           int64_t ldb, float inv_tau, int nsplit,
                                                           const float* part, float* lse_out, float* row_loss,
                                                           float* row_valid) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int64_t stride = (int64_t)nsplit * N;
  float m = -INFINITY, l = 0.0f;
  if (lane < nsplit) {
    m = part[(int64_t)lane * N + i];
    l = part[stride + (int64_t)lane * N + i];
  }
  float mm = m;
  for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
  float t = (m == -INFINITY) ? 0.0f : l * __expf(m - mm);
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  const float lse = (mm == -INFINITY) ? -INFINITY : mm + logf(t);
  const int d = row_col[i];
  const float2 x = reinterpret_cast<const float2*>(A + i * lda)[lane];
  const float2 y = reinterpret_cast<const float2*>(B + (int64_t)d * ldb)[lane];
  float dd = x.x * y.x + x.y * y.y;
  for (int o = 32; o > 0; o >>= 1) dd += __shfl_xor(dd, o, 64);
  const float sii = dd * inv_tau - (bias ? bias[d] : 0.0f);
  if (lane == 0) {
    lse_out[i] = lse;
    row_loss[i] = lse - sii;
    row_valid[i] = 1.0f;
  }
}

template <bool ROW_OWNED>
__global__ __launch_bounds__(256, 2) void nce_grouped_bwd_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) F32Prod::Tile sX[2];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // rows: lse_i  | cols: bias_d
  __shared__ __attribute__((aligned(16))) float sM1[2][kTile];  // cols: c_d
  __shared__ __attribute__((aligned(16))) int sM2[2][kTile];    // rows: d(i)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, ob;
  remap_block(a.nsplit, split, ob);
  const int64_t n_own = ROW_OWNED ? a.N : a.M;
  const int64_t n_str = ROW_OWNED ? a.M : a.N;
  const float* own = ROW_OWNED ? a.A : a.B;
  const float* str = ROW_OWNED ? a.B : a.A;
  const int64_t ld_own = ROW_OWNED ? a.lda : a.ldb;
  const int64_t ld_str = ROW_OWNED ? a.ldb : a.lda;
  const float gs = a.gout[0] * a.inv_tau;
  const int64_t o = (int64_t)ob * kOwnRows + wave * 32 + c;
  const bool own_ok = o < n_own;
  F32Prod::Owner u;
  F32Prod::load_owner(u, {}, own, o, ld_own, own_ok, h);
  const int64_t s_begin = (int64_t)split * a.span;
  int64_t s_end = s_begin + a.span;
  if (s_end > n_str) s_end = n_str;

  // owner metadata + exception walker
  float o_lse = 0.0f, o_bias = 0.0f, o_cnt = 0.0f;
  int o_d = -1, p = 0, e = 0, next = 0x7fffffff;
  if (own_ok) {
    if (ROW_OWNED) {
      o_lse = a.lse[o];
      o_d = a.row_col[o];
      p = a.row_beg[o];
      e = a.row_end[o];
      p = lower_bound_i(a.exc_cols, p, e, s_begin);
      next = (p < e) ? a.exc_cols[p] : 0x7fffffff;
    } else {
      o_bias = a.bias ? a.bias[o] : 0.0f;
      o_cnt = a.colcnt[o];
      p = a.col_beg[o];
      e = a.col_end[o];
      p = lower_bound_i(a.exc_e, p, e, s_begin + 1);  // first user range ending after s_begin
    }
  }

  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;

  F32Prod::Stage stg = F32Prod::stage(tid);
  float stg0 = 0.0f, stg1 = 0.0f;
  int stg2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load({str, ld_str}, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      if (ROW_OWNED) {
        stg0 = (ok && a.bias) ? a.bias[ss] : 0.0f;
        stg1 = ok ? a.colcnt[ss] : 0.0f;
      } else {
        stg0 = ok ? a.lse[ss] : 0.0f;
        stg2 = ok ? a.row_col[ss] : -2;
      }
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sX[buf], tid);
    if (tid < kTile) {
      sM0[buf][tid] = stg0;
      sM1[buf][tid] = stg1;
      sM2[buf][tid] = stg2;
    }
  };

  if (s_begin < s_end) {
    gload(s_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int64_t s0 = s_begin; s0 < s_end; s0 += kTile) {
      const bool has_next = s0 + kTile < s_end;
      if (has_next) gload(s0 + kTile);
      f32x16 acc = F32Prod::dots(sX[cur], u, {}, c, h);
      if (ROW_OWNED) {
        // exceptions of this row inside the tile: exc_cols[p, q)
        int q = p;
        if ((int64_t)next < s0 + kTile) {
          while (q < e && (int64_t)a.exc_cols[q] < s0 + kTile) ++q;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tr = tile_row(r, h);
          const int64_t d = s0 + tr;
          float wr = (d < s_end) ? ((d == o_d) ? 1.0f : sM1[cur][tr]) : 0.0f;
          if (q > p && d != o_d) {
            for (int k = p; k < q; ++k) wr -= (a.exc_cols[k] == (int)d) ? 1.0f : 0.0f;
          }
          const float x = acc[r] * a.inv_tau - sM0[cur][tr];
          const float pr = (wr > 0.0f && own_ok) ? wr * __expf(x - o_lse) : 0.0f;
          acc[r] = own_ok ? gs * (pr - (d == o_d ? 1.0f : 0.0f)) : 0.0f;
        }
        if (q > p) {
          p = q;
          next = (p < e) ? a.exc_cols[p] : 0x7fffffff;
        }
      } else {
        // owner column d = o; streamed rows i = s0 + tile_row(r,h); user ranges of column o
        // intersecting this row tile are exc[p, q)
        while (p < e && (int64_t)a.exc_e[p] <= s0) ++p;
        int q = p;
        while (q < e && (int64_t)a.exc_s[q] < s0 + kTile) ++q;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tr = tile_row(r, h);
          const int64_t ii = s0 + tr;
          const int di = sM2[cur][tr];
          float wr = (ii < s_end) ? ((di == (int)o) ? 1.0f : o_cnt) : 0.0f;
          if (q > p && di != (int)o) {
            for (int k = p; k < q; ++k)
              if (ii >= a.exc_s[k] && ii < a.exc_e[k]) wr -= (float)a.exc_n[k];
          }
          const float x = acc[r] * a.inv_tau - o_bias;
          const float pr = (wr > 0.0f && own_ok) ? wr * __expf(x - sM0[cur][tr]) : 0.0f;
          acc[r] = own_ok ? gs * (pr - (di == (int)o ? 1.0f : 0.0f)) : 0.0f;
        }
      }
      F32Prod::grad(gacc, acc, sX[cur], lane, c, h);
      __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  store_d_own((int64_t)ob * kOwnRows + wave * 32, a.dout + (int64_t)split * n_own * kD, n_own, h, c, gacc);
}

// g = 2^(x - m) per element of the tile, summed into ls and split to hi/lo fragments, two elements
// per step on packed fp32 ops: one v_pk_add for the exponent arguments, one for the running sum,
// and a truncation split (hi = top 16 bits: one v_perm packs the pair, two masks give hi as fp32,
// one v_pk_add the exact residuals x - hi, one pair conversion rounds them to bf16). Truncation
// leaves |lo| < 2^-7 |x| and an error below 2^-16 |x| after rounding lo (RNE hi: 2^-17), well
// inside the bf16x3 product's own 2^-16 (the dropped lo*lo' term).
__device__ __forceinline__ void exp_split_pair(float a, float b, float m, uint32_t& hi, uint32_t& lo, f32x2& sum) {
  f32x2 v = {a, b};
  const f32x2 mm = {m, m};
  v = v - mm;
  v.x = __builtin_amdgcn_exp2f(v.x);
  v.y = __builtin_amdgcn_exp2f(v.y);
  sum = sum + v;
  const uint32_t ua = __float_as_uint(v.x), ub = __float_as_uint(v.y);
  hi = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
  const f32x2 hv = {__uint_as_float(ua & 0xffff0000u), __uint_as_float(ub & 0xffff0000u)};
  const f32x2 r = v - hv;  // exact
  const bf16x2 lq = {(__bf16)r.x, (__bf16)r.y};
  lo = __builtin_bit_cast(uint32_t, lq);
}

// One k-step half of the gradient product, gacc[nb] += G_ks^T X (steps nb = 0..3 over tile t,
// ks fixed), with WORK: the exp/split of pair q of half xh of the next G operand placed under
// step q's three MFMAs (sched_group_barrier: the VALU fills the MFMA issue gaps of the same wave
// instead of running as its own phase).
template <bool WORK>
__device__ __forceinline__ void grad_half_x3(f32x16 (&gacc)[4], const bf16x8& gh, const bf16x8& gl, const X3Tile& t,
                                             int base, int ks, const f32x16& x, int xh, float m, uint32_t (&oh)[4],
                                             uint32_t (&ol)[4], f32x2& sum) {
  bf16x8 bh, bl;
  bh = img_read_tr(t.hi, base, ks, 0);
  bl = img_read_tr(t.lo, base, ks, 0);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      nh = img_read_tr(t.hi, base, ks, nb + 1);
      nl = img_read_tr(t.lo, base, ks, nb + 1);
    }
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl, bh, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, bl, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, bh, gacc[nb], 0, 0, 0);
    if (WORK) {
      exp_split_pair(x[8 * xh + 2 * nb], x[8 * xh + 2 * nb + 1], m, oh[nb], ol[nb], sum);
      asm volatile("" : "+v"(oh[nb]), "+v"(ol[nb]));  // pins the work to this step (no sinking)
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // next step's transposed reads
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

// The common-form gradient tile from its S tile:
//   g_r = f_r * 2^(S_r * it2 - (m0[tr] + o_m2)),  f_r = ROW ? fo * m1[tr] : fo,  tr = tile_row(r, h)
// split to hi/lo fragments, two rows of G per k-step. The tile's metadata comes in as b128
// reads two k-steps ahead of use.
template <bool ROW>
__device__ __forceinline__ void g_tile_x3(int h, const f32x16& S, const float* m0, const float* m1, float o_m2,
                                          float it2, float fo, bf16x8 (&gh)[2], bf16x8 (&gl)[2]) {
  f32x4 q0 = *reinterpret_cast<const f32x4*>(m0 + 4 * h), q1 = q0, n0 = q0, n1 = q0;
  if (ROW) q1 = *reinterpret_cast<const f32x4*>(m1 + 4 * h);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if ((s & 1) == 0 && s < 6) {  // rows of k-steps s+2, s+3
      n0 = *reinterpret_cast<const f32x4*>(m0 + 8 * ((s >> 1) + 1) + 4 * h);
      if (ROW) n1 = *reinterpret_cast<const f32x4*>(m1 + 8 * ((s >> 1) + 1) + 4 * h);
    }
    float gp[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * s + rr, e = r & 3;
      const float f = ROW ? fo * q1[e] : fo;
      gp[rr] = f * __builtin_amdgcn_exp2f(fmaf(S[r], it2, -(q0[e] + o_m2)));
    }
    {  // rows 2s, 2s+1 = dword s & 3 of fragment s >> 2
      uint32_t hp, lp;
      split_pair(gp[0], gp[1], hp, lp);
      u32x4 hv = __builtin_bit_cast(u32x4, gh[s >> 2]), lv = __builtin_bit_cast(u32x4, gl[s >> 2]);
      hv[s & 3] = hp;
      lv[s & 3] = lp;
      gh[s >> 2] = __builtin_bit_cast(bf16x8, hv);
      gl[s >> 2] = __builtin_bit_cast(bf16x8, lv);
    }
    if (s & 1) {
      q0 = n0;
      q1 = n1;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One G pair (rows 2p, 2p+1 of the tile, the g_tile_x3 formula) as hi/lo bf16 words.
template <bool ROW>
__device__ __forceinline__ void g_pair(const f32x16& S, int p, int h, const float* m0, const float* m1, float o_m2,
                                       float it2, float fo, uint32_t& hp, uint32_t& lp) {
  const f32x4 q0 = *reinterpret_cast<const f32x4*>(m0 + 8 * (p >> 1) + 4 * h);
  f32x4 q1 = q0;
  if (ROW) q1 = *reinterpret_cast<const f32x4*>(m1 + 8 * (p >> 1) + 4 * h);
  float gp[2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int r = 2 * p + rr, e = r & 3;
    const float f = ROW ? fo * q1[e] : fo;
    gp[rr] = f * __builtin_amdgcn_exp2f(fmaf(S[r], it2, -(q0[e] + o_m2)));
  }
  split_pair(gp[0], gp[1], hp, lp);
}

// k-step ks of the backward's gradient product, gacc[nb] += G_ks^T X; WORK: G pair 4 + nb (the
// next k-step's rows) computed under step nb's three MFMAs, so half of the tile's G work runs
// in the MFMA issue gaps of the same wave (grad_half_x3's pattern for the fused forward). Same
// MFMA order as grad_x3s, same G arithmetic as g_tile_x3: bit-identical results.
template <bool ROW, bool WORK>
__device__ __forceinline__ void grad_half_g_x3(f32x16 (&gacc)[4], const bf16x8& gh, const bf16x8& gl, const X3Tile& t,
                                               int base, int ks, const f32x16& S, int h, const float* m0,
                                               const float* m1, float o_m2, float it2, float fo, uint32_t (&oh)[4],
                                               uint32_t (&ol)[4]) {
  bf16x8 bh, bl;
  bh = img_read_tr(t.hi, base, ks, 0);
  bl = img_read_tr(t.lo, base, ks, 0);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      nh = img_read_tr(t.hi, base, ks, nb + 1);
      nl = img_read_tr(t.lo, base, ks, nb + 1);
    }
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl, bh, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, bl, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, bh, gacc[nb], 0, 0, 0);
    if (WORK) {
      g_pair<ROW>(S, 4 + nb, h, m0, m1, o_m2, it2, fo, oh[nb], ol[nb]);
      asm volatile("" : "+v"(oh[nb]), "+v"(ol[nb]));  // pins the work to this step (no sinking)
    }
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

__global__ __launch_bounds__(256, 2) void nce_grouped_fwd_x3_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) X3Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sB2[2][kTile];   // bias_d * log2e (0 past the split)
  __shared__ __attribute__((aligned(16))) float sCnt[2][kTile];  // c_d (0 past the split)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  bf16x8 uh[8], ul[8];
  load_owner_x3(uh, ul, a.A, i, a.lda, row_ok, h);
  const int64_t j_begin = (int64_t)split * a.span;
  int64_t j_end = j_begin + a.span;
  if (j_end > a.M) j_end = a.M;
  int di = -1, p = 0, e = 0, next = 0x7fffffff;
  if (row_ok) {
    di = a.row_col[i];
    p = a.row_beg[i];
    e = a.row_end[i];
    p = lower_bound_i(a.exc_cols, p, e, j_begin);
    next = (p < e) ? a.exc_cols[p] : 0x7fffffff;
  }
  const float it2 = a.inv_tau * kLog2e;
  float m = -INFINITY, l = 0.0f;  // base 2
  X3Stage stg;
  float stg_b = 0.0f, stg_c = 0.0f;
  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + (tid >> 3);
    stg.load(a.bhi, a.blo, j, j < j_end, tid);
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      // raw values only (math on a load in flight would wait for it here); columns past the
      // split get bias +inf, i.e. logit -inf, so the common path needs no mask
      stg_b = ok ? (a.bias ? a.bias[jj] : 0.0f) : INFINITY;
      stg_c = ok ? a.colcnt[jj] : 0.0f;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sB2[buf][tid] = stg_b * kLog2e;
      sCnt[buf][tid] = stg_c;
    }
  };
  if (j_begin < j_end) {
    gload(j_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kTile) {
      const bool has_next = j0 + kTile < j_end;
      if (has_next) gload(j0 + kTile);
      const f32x16 acc = dots_x3(sT[cur], c, h, uh, ul);
      float w[16], v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tr = tile_row(r, h);
        w[r] = sCnt[cur][tr];
        v[r] = fmaf(acc[r], it2, -sB2[cur][tr]);
      }
      if ((int64_t)next < j0 + kTile) {
        // rare: some of the user's own targets (d(i) among them) fall in this tile; a column
        // whose multiplicity drops to 0 is masked
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
        for (int r = 0; r < 16; ++r) {
          const int tr = tile_row(r, h);
          w[r] = (tr == tl) ? 1.0f : w[r] - n[r];
          if (!(w[r] > 0.0f)) v[r] = -INFINITY;
        }
        p = q;
        next = (p < e) ? a.exc_cols[p] : 0x7fffffff;
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, v[r]);
      if (!row_ok) tmax = -INFINITY;
      if (tmax > m) {
        l = (m == -INFINITY) ? 0.0f : l * __builtin_amdgcn_exp2f(m - tmax);
        m = tmax;
      }
      if (m != -INFINITY) {
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t = fmaf(w[r], __builtin_amdgcn_exp2f(v[r] - m), t);  // w >= 0
        l += t;
      }
      // buffer cur^1 was last read in the previous tile, which every wave finished before the
      // barrier that ended it: one barrier per tile
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  const float m2 = __shfl_xor(m, 32, 64);
  const float l2 = __shfl_xor(l, 32, 64);
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (mm != -INFINITY) {
    if (m != -INFINITY) ll += l * __builtin_amdgcn_exp2f(m - mm);
    if (m2 != -INFINITY) ll += l2 * __builtin_amdgcn_exp2f(m2 - mm);
  }
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)a.nsplit * a.N;
    const int64_t o = (int64_t)split * a.N + i;
    a.part[o] = (mm == -INFINITY) ? -INFINITY : mm * kLn2;  // natural-log max, same sum
    a.part[stride + o] = ll;
    a.part[2 * stride + o] = 0.0f;
    a.part[3 * stride + o] = 0.0f;
  }
}

// Backward of the grouped loss (bf16x3). Per streamed tile: S = owner x streamed rows, then
// G = w * 2^(S log2e / tau - ...) (- 1 on the label), then G^T X into the owner's gradient.
// Ordering rules that keep the staging loads in flight (vmcnt counts in order, so a wait on
// any later load drains the prefetch): the per-tile exception flag (and the column pass's
// window update, which may load) runs BEFORE the prefetch is issued, and an explicit
// vmcnt(0) before each barrier leaves no load pending at the loop head on any path, so the
// common path never waits on memory before its LDS store. Only the rare exception tiles
// load after the prefetch.
template <bool ROW_OWNED, bool HALFG = true>
__global__ __launch_bounds__(256, 2) void nce_grouped_bwd_x3_k(GArgs a) {
  __shared__ __attribute__((aligned(16))) X3Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // rows: bias_d*log2e | cols: lse_i*log2e (+inf past the split)
  __shared__ __attribute__((aligned(16))) float sM1[2][kTile];  // rows: c_d (0 past the split) | cols: unused
  __shared__ __attribute__((aligned(16))) int sM2[2][kTile];    // cols: d(i)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, ob;
  const int64_t n_own = ROW_OWNED ? a.N : a.M;
  const int64_t n_str = ROW_OWNED ? a.M : a.N;
  if (a.split_major) {
    // split-major XCD order: an XCD group (b % 8) runs all owner blocks of one split before the
    // next, so its L2 holds one split's streamed images at a time (speed only)
    const int b = blockIdx.x, xcd = b & 7, q = b >> 3;
    const int nob = (int)((n_own + kOwnRows - 1) / kOwnRows);
    split = xcd + 8 * (q / nob);
    ob = q % nob;
  } else {
    remap_block(a.nsplit, split, ob);
  }
  const float* own = ROW_OWNED ? a.A : a.B;
  const int64_t ld_own = ROW_OWNED ? a.lda : a.ldb;
  const float gs = a.gout[0] * a.inv_tau;
  const float it2 = a.inv_tau * kLog2e;
  const int64_t o = (int64_t)ob * kOwnRows + wave * 32 + c;
  const bool own_ok = o < n_own;
  bf16x8 uh[8], ul[8];
  load_owner_x3(uh, ul, own, o, ld_own, own_ok, h);
  const int64_t s_begin = (int64_t)split * a.span;
  int64_t s_end = s_begin + a.span;
  if (s_end > n_str) s_end = n_str;
  constexpr int kNone = 0x7fffffff;

  float o_m2 = 0.0f, o_cnt = 0.0f;  // rows: lse_o*log2e | cols: bias_o*log2e, c_o
  int o_d = -1, p = 0, e = 0, next = kNone;
  if (own_ok) {
    if (ROW_OWNED) {
      o_m2 = a.lse[o] * kLog2e;
      o_d = a.row_col[o];
      p = a.row_beg[o];
      e = a.row_end[o];
      p = lower_bound_i(a.exc_cols, p, e, s_begin);
      next = (p < e) ? a.exc_cols[p] : kNone;
    } else {
      o_m2 = a.bias ? a.bias[o] * kLog2e : 0.0f;
      o_cnt = a.colcnt[o];
      p = a.col_beg[o];
      e = a.col_end[o];
      p = lower_bound_i(a.exc_e, p, e, s_begin + 1);  // first user range ending after s_begin
    }
  }
  const float gso = own_ok ? gs : 0.0f;  // the owner's factor of every G entry
  const float fo = ROW_OWNED ? gso : gso * o_cnt;
  // cols: ranges [p, q) intersect the current tile; e_first = end of range p (if p < q),
  // s_next = start of range q: the per-tile window update is register compares only
  int q = p, e_first = 0, s_next = kNone;
  if (!ROW_OWNED && own_ok && q < e) s_next = a.exc_s[q];

  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;

  X3Stage stg;
  float stg0 = 0.0f, stg1 = 0.0f;
  int stg2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load(ROW_OWNED ? a.bhi : a.ahi, ROW_OWNED ? a.blo : a.alo, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      // raw loads only (math on a value in flight would wait for the whole tile load here)
      if (ROW_OWNED) {
        stg0 = (ok && a.bias) ? a.bias[ss] : 0.0f;
        stg1 = ok ? a.colcnt[ss] : 0.0f;
      } else {
        stg0 = ok ? a.lse[ss] : INFINITY;  // past the split: 2^(x - inf) = 0
        stg1 = 0.0f;
        stg2 = ok ? a.row_col[ss] : -2;
      }
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sM0[buf][tid] = stg0 * kLog2e;
      sM1[buf][tid] = stg1;
      sM2[buf][tid] = stg2;
    }
  };
  // exception flag of tile s0 (before the tile prefetch is issued: the column pass's window
  // update may load, and a wait on it must not drain the prefetch): rows: the user's own
  // target columns; cols: user row ranges [p, q) holding target o that intersect the tile
  auto exc_flag = [&](int64_t s0) -> bool {
    if (ROW_OWNED) return (int64_t)next < s0 + kTile;
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
  // per-lane multiplicities n[r] of the owner's exceptions among the tile's streamed rows
  // and the row label column tl (rare: called when some lane of the wave has exceptions)
  auto exc_counts = [&](int64_t s0, bool exc, float (&n)[16], int& tl) {
#pragma unroll
    for (int r = 0; r < 16; ++r) n[r] = 0.0f;
    tl = -1;
    if (!exc) return;
    if (ROW_OWNED) {
      int k = p;
      for (; k < e && (int64_t)a.exc_cols[k] < s0 + kTile; ++k) {  // sorted, with repeats
        const int tk = (int)(a.exc_cols[k] - s0);
#pragma unroll
        for (int r = 0; r < 16; ++r) n[r] += (tk == tile_row(r, h)) ? 1.0f : 0.0f;
      }
      p = k;
      next = (p < e) ? a.exc_cols[p] : kNone;
      tl = ((int64_t)o_d < s_end) ? (int)(o_d - s0) : -1;  // label column, if this split owns it
    } else {
      for (int k = p; k < q; ++k) {
        const int ks = (int)(a.exc_s[k] - s0), ke = (int)(a.exc_e[k] - s0);
        const float nk = (float)a.exc_n[k];
#pragma unroll
        for (int r = 0; r < 16; ++r) n[r] += (tile_row(r, h) >= ks && tile_row(r, h) < ke) ? nk : 0.0f;
      }
    }
  };
  // G of tile buffer cb from its S tile (in place), exception form: per-lane multiplicities
  // and labels; lanes without exceptions take the common form
  auto g_exc = [&](f32x16& acc, int cb, bool exc, const float (&n)[16], int tl) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = tile_row(r, h);
      const float x = fmaf(acc[r], it2, -(sM0[cb][tr] + o_m2));
      bool lab;
      float wr;
      if (ROW_OWNED) {
        lab = exc && tr == tl;
        wr = lab ? 1.0f : sM1[cb][tr] - n[r];
      } else {
        lab = exc && sM2[cb][tr] == (int)o;
        wr = lab ? 1.0f : o_cnt - n[r];
      }
      const float g = (wr > 0.0f ? wr * __builtin_amdgcn_exp2f(x) : 0.0f) - (lab ? 1.0f : 0.0f);
      acc[r] = gso * g;
    }
  };

  if (s_begin < s_end) {
    const int ntile = (int)((s_end - s_begin + kTile - 1) / kTile);
    gload(s_begin);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < ntile; ++t) {
      const int64_t s0 = s_begin + (int64_t)t * kTile;
      const bool has_next = t + 1 < ntile;
      const bool exc = exc_flag(s0);
      if (has_next) gload(s0 + kTile);
      f32x16 acc = dots_x3(sT[cur], c, h, uh, ul);
      bf16x8 gh[2], gl[2];
      const bool any_exc = __any(exc);
      if (any_exc) {
        float n[16];
        int tl;
        exc_counts(s0, exc, n, tl);
        g_exc(acc, cur, exc, n, tl);
        split_tile(acc, gh, gl);
      } else if (HALFG) {
        // G rows of k-step 0, then k-step 0's product with k-step 1's G rows under its MFMAs
        u32x4 h0, l0;
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
          uint32_t hp, lp;
          g_pair<ROW_OWNED>(acc, pp, h, sM0[cur], sM1[cur], o_m2, it2, fo, hp, lp);
          h0[pp] = hp;
          l0[pp] = lp;
        }
        gh[0] = __builtin_bit_cast(bf16x8, h0);
        gl[0] = __builtin_bit_cast(bf16x8, l0);
        uint32_t oh[4], ol[4];
        const int gbase = img_tr_base(lane);
        grad_half_g_x3<ROW_OWNED, true>(gacc, gh[0], gl[0], sT[cur], gbase, 0, acc, h, sM0[cur], sM1[cur], o_m2, it2,
                                        fo, oh, ol);
        gh[1] = __builtin_bit_cast(bf16x8, u32x4{oh[0], oh[1], oh[2], oh[3]});
        gl[1] = __builtin_bit_cast(bf16x8, u32x4{ol[0], ol[1], ol[2], ol[3]});
        grad_half_g_x3<ROW_OWNED, false>(gacc, gh[1], gl[1], sT[cur], gbase, 1, acc, h, sM0[cur], sM1[cur], o_m2,
                                         it2, fo, oh, ol);
      } else {
        g_tile_x3<ROW_OWNED>(h, acc, sM0[cur], sM1[cur], o_m2, it2, fo, gh, gl);
      }
      if (!HALFG || any_exc) grad_x3s(gacc, gh, gl, sT[cur], lane);
      if (has_next) lstore(cur ^ 1);  // cur^1: read in the previous tile, fenced by its barrier
      __builtin_amdgcn_s_waitcnt(kVmcnt0);  // nothing pending at the loop head on any path
      __syncthreads();
      cur ^= 1;
    }
  }
  store_d_own((int64_t)ob * kOwnRows + wave * 32, a.dout + (int64_t)split * n_own * kD, n_own, h, c, gacc);
}

// Forward of the grouped loss fused with the row-side gradient (bf16x3). The row gradient
//   dA_i = gout/tau * (sum_j p_ij B_j - B_d(i)),  p_ij = w_ij 2^(x_ij) / sum_j w_ij 2^(x_ij)
// is a softmax-weighted sum of the streamed rows, i.e. an attention output with V = B: it is
// accumulated during the forward sweep, unnormalised, against a lazily raised running max
// (rescaled only when a tile max exceeds it by more than 2^8, so almost never after the first
// tiles), and normalised in the merge. This replaces the forward plus the backward's row pass
// (two sweeps of S) with one sweep; the backward keeps only the column pass.
// Per split: part = (m ln2, l) per row as the plain forward, dpart[split][row][128] = O.
__global__ __launch_bounds__(256, 2) void nce_grouped_fwdg_x3p_k(GArgs a) {
  constexpr int NW = kWaves, kRows = kOwnRows;
  __shared__ __attribute__((aligned(16))) X3Tile sT[3];  // ring: t-1 (deferred k-step), t, t+1
  __shared__ __attribute__((aligned(16))) float sB2[3][kTile];   // -bias_d * log2e (-inf past the split)
  __shared__ __attribute__((aligned(16))) float sCnt[3][kTile];  // c_d (0 past the split)
  __shared__ __attribute__((aligned(16))) float sAlpha[NW][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split;
  int64_t rb, j_begin, j_end;
  fwdg_geometry(a, split, rb, j_begin, j_end);
  const int64_t i = rb * kRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  bf16x8 uh[8], ul[8];
  load_owner_x3(uh, ul, a.A, i, a.lda, row_ok, h);
  constexpr int kNone = 0x7fffffff;
  int di = -1, p = 0, e = 0, next = kNone;
  if (row_ok) {
    di = a.row_col[i];
    p = a.row_beg[i];
    e = a.row_end[i];
    p = lower_bound_i(a.exc_cols, p, e, j_begin);
    next = (p < e) ? a.exc_cols[p] : kNone;
  }
  const float it2 = a.inv_tau * kLog2e;
  float m = -INFINITY, l = 0.0f;  // base 2; m is the same on both lane halves
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
    // k-step 1 of the previous tile's gradient product runs in the next iteration (its G
    // fragments pgh/pgl); zero fragments (first tile, after a flush) add exactly zero
    int cur = 0, prev = 0;
    bf16x8 pgh, pgl;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pgh[k] = (__bf16)0.0f;
      pgl[k] = (__bf16)0.0f;
    }
    const int gbase = img_tr_base(lane);
    for (int64_t j0 = j_begin; j0 < j_end; j0 += kTile) {
      const bool has_next = j0 + kTile < j_end;
      const bool exc = (int64_t)next < j0 + kTile;  // before the prefetch (see the backward)
      if (has_next) gload(j0 + kTile);
      f32x16 acc = dots_x3(sT[cur], c, h, uh, ul);
      // registers 4g..4g+3 hold tile rows 8g + 4h + 0..3: one b128 read per group and array
      // (an immediate offset from a per-lane base) instead of 16 scalar reads with 32 address ops
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 nb = *reinterpret_cast<const float4*>(&sB2[cur][8 * g + 4 * h]);
        acc[4 * g + 0] = fmaf(acc[4 * g + 0], it2, nb.x);  // x = S/tau - bias + log2 c, base 2
        acc[4 * g + 1] = fmaf(acc[4 * g + 1], it2, nb.y);
        acc[4 * g + 2] = fmaf(acc[4 * g + 2], it2, nb.z);
        acc[4 * g + 3] = fmaf(acc[4 * g + 3], it2, nb.w);
      }
      if (exc) {  // the row's own targets: multiplicity c_d - n_{u,d}, or 1 for d(i)
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
          }
        }
        p = q;
        next = (p < e) ? a.exc_cols[p] : kNone;
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, acc[r]);
      {  // max with the partner lane c ^ 32: v_permlane32_swap (VALU) instead of an LDS permute
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      if (!row_ok) tmax = -INFINITY;
      const bool raise = tmax > m + kLazyLog2;  // m = -inf: the first finite tile
      if (__any(raise)) {
        {  // the deferred product was formed against the old max: add it before rescaling
          uint32_t dh[4], dl[4];
          f32x2 ds = {0.0f, 0.0f};
          grad_half_x3<false>(gacc, pgh, pgl, sT[prev], gbase, 1, acc, 0, 0.0f, dh, dl, ds);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            pgh[k] = (__bf16)0.0f;
            pgl[k] = (__bf16)0.0f;
          }
        }
        // rescale this lane's l and, through LDS, the accumulator rows of every raised owner
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
      // G half 0 of this tile under the previous tile's deferred k-step 1, then G half 1 under
      // this tile's k-step 0; this tile's k-step 1 is deferred to the next iteration
      uint32_t h0[4], l0[4], h1[4], l1[4];
      f32x2 sum = {0.0f, 0.0f};
      grad_half_x3<true>(gacc, pgh, pgl, sT[prev], gbase, 1, acc, 0, ms, h0, l0, sum);
      const u32x4 h0v = {h0[0], h0[1], h0[2], h0[3]}, l0v = {l0[0], l0[1], l0[2], l0[3]};
      grad_half_x3<true>(gacc, __builtin_bit_cast(bf16x8, h0v), __builtin_bit_cast(bf16x8, l0v), sT[cur], gbase, 0,
                         acc, 1, ms, h1, l1, sum);
      l += sum.x + sum.y;
      const u32x4 h1v = {h1[0], h1[1], h1[2], h1[3]}, l1v = {l1[0], l1[1], l1[2], l1[3]};
      pgh = __builtin_bit_cast(bf16x8, h1v);
      pgl = __builtin_bit_cast(bf16x8, l1v);
      prev = cur;
      const int nxt = (cur == 2) ? 0 : cur + 1;
      if (has_next) lstore(nxt);  // nxt held tile t-2, whose deferred step ran before the last barrier
      __builtin_amdgcn_s_waitcnt(kVmcnt0);  // nothing pending at the loop head on any path
      __syncthreads();
      cur = nxt;
    }
    {
      uint32_t dh[4], dl[4];
      f32x2 ds = {0.0f, 0.0f};
      f32x16 z;
#pragma unroll
      for (int r = 0; r < 16; ++r) z[r] = 0.0f;
      grad_half_x3<false>(gacc, pgh, pgl, sT[prev], gbase, 1, z, 0, 0.0f, dh, dl, ds);
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
  store_d_own(rb * kRows + wave * 32, a.dout + (int64_t)split * a.N * kD, a.N, h, c, gacc);
}


// merge of the fused forward: lse / row loss as nce_grouped_merge_k, plus the row gradient
// per unit upstream gradient  ga_i = (sum_s O_s e^(m_s - M) / sum_s l_s e^(m_s - M) - B_d(i)) / tau
// POS (the plain view's flags 9, SupCon): the row has no label column; its positive set enters through
// pos_cnt / pos_ps / pos_P (nce_pos_rows_k) as loss_i = lse_i - ps_i / cnt_i and ga_i -= P_i / (tau cnt_i).
// A row without positives is invalid: zero loss and gradient, and lse = +inf for the column pass
// (every column weight of the row exactly 0). row_col is not read.
template <bool POS>
__global__ __launch_bounds__(256) void nce_grouped_merge_g_k(const float* A, const float* B, const float* bias,
                                                             const int* row_col, int64_t N, int64_t lda,
                                                             int64_t ldb, float inv_tau, int nsplit,
                                                             const float* part, const float* opart,
                                                             float* lse_out, float* row_loss, float* row_valid,
                                                             float* ga, int64_t rows1, int nsplit2, int nslots,
                                                             int lab_out, const float* pos_cnt, const float* pos_ps,
                                                             const float* pos_P) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int64_t stride = (int64_t)nslots * N;
  if (i >= rows1) nsplit = nsplit2;  // this row's workgroups ran the tail split count
  float m = -INFINITY, l = 0.0f;
  if (lane < nsplit) {
    m = part[(int64_t)lane * N + i];
    l = part[stride + (int64_t)lane * N + i];
  }
  float mm = m;
  for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
  const float f = (m == -INFINITY) ? 0.0f : __expf(m - mm);
  float t = l * f;
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  const float lse = (mm == -INFINITY) ? -INFINITY : mm + logf(t);
  float2 y;
  float sii = 0.0f, pcnt = 0.0f;
  if (POS) {
    pcnt = pos_cnt[i];
    y = reinterpret_cast<const float2*>(pos_P + i * kD)[lane];
  } else {
    const int d = row_col[i];
    const float2 x = reinterpret_cast<const float2*>(A + i * lda)[lane];
    y = reinterpret_cast<const float2*>(B + (int64_t)d * ldb)[lane];
    float dd = x.x * y.x + x.y * y.y;
    for (int o = 32; o > 0; o >>= 1) dd += __shfl_xor(dd, o, 64);
    sii = dd * inv_tau - (bias ? bias[d] : 0.0f);
  }
  const float inv_t = (t > 0.0f) ? 1.0f / t : 0.0f;
  // every split's partial row is loaded unconditionally (all in flight at once) and a split
  // with no columns (f = 0: its slot was never written) is dropped by a select, not a branch
  float2 acc = make_float2(0.0f, 0.0f);
  for (int s0 = 0; s0 < nsplit; s0 += 8) {
    float2 v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (s0 + s < nsplit) v[s] = reinterpret_cast<const float2*>(opart + ((int64_t)(s0 + s) * N + i) * kD)[lane];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s0 + s >= nsplit) break;
      const float fs = __shfl(f, s0 + s, 64) * inv_t;
      acc.x = fs != 0.0f ? fmaf(fs, v[s].x, acc.x) : acc.x;
      acc.y = fs != 0.0f ? fmaf(fs, v[s].y, acc.y) : acc.y;
    }
  }
  // lab_out: the kernel left the label column out of its partial rows (nce_grouped_fwdg_h_k): its term
  // p_pos B_d(i) and the label's -B_d(i) enter together as (p_pos - 1) B_d(i), p_pos = e^(s_ii - lse)
  if (POS) {
    const bool valid = pcnt > 0.0f;
    const float ic = valid ? 1.0f / pcnt : 0.0f;
    const float2 g = make_float2(fmaf(-ic, y.x, acc.x) * inv_tau, fmaf(-ic, y.y, acc.y) * inv_tau);
    reinterpret_cast<float2*>(ga + i * kD)[lane] = valid ? g : make_float2(0.0f, 0.0f);
    if (lane == 0) {
      lse_out[i] = valid ? lse : INFINITY;
      row_loss[i] = valid ? lse - pos_ps[i] * ic : 0.0f;
      row_valid[i] = valid ? 1.0f : 0.0f;
    }
    return;
  }
  const float cy = lab_out ? ((lse == -INFINITY) ? -1.0f : __expf(sii - lse) - 1.0f) : -1.0f;
  reinterpret_cast<float2*>(ga + i * kD)[lane] = make_float2(fmaf(cy, y.x, acc.x) * inv_tau, fmaf(cy, y.y, acc.y) * inv_tau);
  if (lane == 0) {
    lse_out[i] = lse;
    row_loss[i] = lse - sii;
    row_valid[i] = 1.0f;
  }
}

// ---- plain-family view (rsx_nce_fwd_grad / rsx_nce_bwd_cols) ------------------------------
__global__ __launch_bounds__(256) void nce_view_fill_k(int* view, int64_t N, int64_t M, int64_t off, int64_t total) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < total) view[k] = view_entry(k, N, M, off);
}

// SupCon's positive term, row side (flags 9): pos(i) = {j : k1b[j] == k1a[i] != 0, j != i + off}.
// One wave per row scans the M keys and adds the matching rows of B in ascending j (fp32, a fixed
// order): cnt_i = |pos(i)|, P_i = sum B_j, ps_i = <A_i, P_i> / tau.
// Two chains of dependent loads are broken up. The key scan loads kPosScan x 64 keys per step. The
// matches are first collected, in order, in a per-wave LDS list and then added kPosBatch rows at a
// time with all of a batch's row loads in flight: on a Zipf batch a popular target has hundreds of
// members spread over the whole batch, and one row load per match, each waited for, made these two
// kernels take 78 and 93 us at batch 8192, as long as the MFMA sweeps beside them.
constexpr int kPosScan = 16;
constexpr int kPosList = 512;  // list entries per wave (flushed when 64 more may not fit)
constexpr int kPosBatch = 8;

// the matches of one 64-key block appended to the wave's list (ascending: lane order)
__device__ __forceinline__ void pos_append(int* list, int& nl, unsigned long long mask, bool hit, int idx, int lane) {
  if (hit) list[nl + __popcll(mask & ((1ull << lane) - 1))] = idx;
  nl += __popcll(mask);
}

// acc += sum over the list of w_k X[list[k]] (W: w_k = 1 / cnt[list[k]], else 1), kPosBatch rows in flight
template <bool W>
__device__ __forceinline__ void pos_flush(const int* list, int& nl, const float* X, int64_t ld, const float* cnt,
                                          int lane, float2& acc) {
  __builtin_amdgcn_wave_barrier();  // the list's writes (this wave's lanes) before its reads
  for (int t0 = 0; t0 < nl; t0 += kPosBatch) {
    float2 v[kPosBatch];
    float w[kPosBatch];
#pragma unroll
    for (int t = 0; t < kPosBatch; ++t) {
      const int k = t0 + t < nl ? t0 + t : nl - 1;  // past the list: a valid row, not added
      const int r = list[k];
      v[t] = reinterpret_cast<const float2*>(X + (int64_t)r * ld)[lane];
      w[t] = W ? cnt[r] : 1.0f;
    }
#pragma unroll
    for (int t = 0; t < kPosBatch; ++t) {
      if (t0 + t < nl) {
        const float f = W ? 1.0f / w[t] : 1.0f;
        acc.x = fmaf(f, v[t].x, acc.x);
        acc.y = fmaf(f, v[t].y, acc.y);
      }
    }
  }
  nl = 0;
  __builtin_amdgcn_wave_barrier();  // the reads before the next block's writes
}

__global__ __launch_bounds__(256) void nce_pos_rows_k(const float* A, const float* B, const int* k1a, const int* k1b,
                                                      int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t off,
                                                      float inv_tau, float* cnt, float* ps, float* P) {
  __shared__ int sList[4][kPosList];
  const int lane = threadIdx.x & 63;
  int* list = sList[threadIdx.x >> 6];
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int key = k1a[i];
  float2 acc = make_float2(0.0f, 0.0f);
  int n = 0, nl = 0;
  if (key != 0) {
    for (int64_t j0 = 0; j0 < M; j0 += 64 * kPosScan) {
      int kv[kPosScan];  // independent loads, all in flight at once; past the end: key 0, never a match
#pragma unroll
      for (int u = 0; u < kPosScan; ++u) {
        const int64_t j = j0 + 64 * u + lane;
        kv[u] = j < M ? k1b[j] : 0;
      }
#pragma unroll
      for (int u = 0; u < kPosScan; ++u) {
        const int64_t j = j0 + 64 * u + lane;
        const bool hit = kv[u] == key && j != i + off;
        const unsigned long long mask = __ballot(hit);
        if (mask == 0) continue;
        n += __popcll(mask);
        pos_append(list, nl, mask, hit, (int)j, lane);
        if (nl + 64 > kPosList) pos_flush<false>(list, nl, B, ldb, nullptr, lane, acc);
      }
    }
    if (nl > 0) pos_flush<false>(list, nl, B, ldb, nullptr, lane, acc);
  }
  const float2 x = reinterpret_cast<const float2*>(A + i * lda)[lane];
  float d = x.x * acc.x + x.y * acc.y;
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  reinterpret_cast<float2*>(P + i * kD)[lane] = acc;
  if (lane == 0) {
    cnt[i] = (float)n;
    ps[i] = d * inv_tau;
  }
}

// Column side, after the column pass's split sum: dB_j -= gout / tau * sum_{i : j in pos(i)} A_i / cnt_i,
// one wave per column, rows in ascending i (j in pos(i) makes row i valid: cnt_i >= 1).
__global__ __launch_bounds__(256) void nce_pos_cols_k(const float* A, const int* k1a, const int* k1b, int64_t N,
                                                      int64_t M, int64_t lda, int64_t off, float inv_tau,
                                                      const float* cnt, const float* gout, float* dB) {
  __shared__ int sList[4][kPosList];
  const int lane = threadIdx.x & 63;
  int* list = sList[threadIdx.x >> 6];
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= M) return;
  const int key = k1b[j];
  if (key == 0) return;
  float2 acc = make_float2(0.0f, 0.0f);
  bool any = false;
  int nl = 0;
  for (int64_t i0 = 0; i0 < N; i0 += 64 * kPosScan) {
    int kv[kPosScan];
#pragma unroll
    for (int u = 0; u < kPosScan; ++u) {
      const int64_t i = i0 + 64 * u + lane;
      kv[u] = i < N ? k1a[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < kPosScan; ++u) {
      const int64_t i = i0 + 64 * u + lane;
      const bool hit = kv[u] == key && i + off != j;
      const unsigned long long mask = __ballot(hit);
      if (mask == 0) continue;
      any = true;
      pos_append(list, nl, mask, hit, (int)i, lane);
      if (nl + 64 > kPosList) pos_flush<true>(list, nl, A, lda, cnt, lane, acc);
    }
  }
  if (!any) return;
  if (nl > 0) pos_flush<true>(list, nl, A, lda, cnt, lane, acc);
  const float f = -gout[0] * inv_tau;
  float2* dst = reinterpret_cast<float2*>(dB + j * kD) + lane;
  float2 o = *dst;
  o.x = fmaf(f, acc.x, o.x);
  o.y = fmaf(f, acc.y, o.y);
  *dst = o;
}

// ---- host side ------------------------------------------------------------------------
// SupCon's positive term of the plain view, handed to the fused forward's merge
struct PosTerm {
  const int* k1a;
  const int* k1b;
  int64_t off;
  float *cnt, *ps, *P;
};

// The fields every grouped entry point fills the same way; splits, spans and the workspace
// pointers are set by the caller.
GArgs grouped_args(const float* A, const float* B, const float* bias, const float* colcnt, const int* row_col,
                   const int* row_beg, const int* row_end, const int* exc_cols, int64_t N, int64_t D, int64_t lda,
                   int64_t ldb, float tau) {
  GArgs g = {};
  g.A = A; g.B = B; g.bias = bias; g.colcnt = colcnt;
  g.row_col = row_col; g.row_beg = row_beg; g.row_end = row_end; g.exc_cols = exc_cols;
  g.N = N; g.M = D; g.lda = lda; g.ldb = ldb;
  g.inv_tau = 1.0f / tau;
  return g;
}

// Measurement hooks (include/recsys_amd.h): event pairs around the fused forward kernel's launch.
struct KernelEvents {
  std::mutex mu;
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  void clear() {
    for (auto& e : ev) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    ev.clear();
  }
};
KernelEvents& kernel_events() {
  static KernelEvents k;
  return k;
}

// The two grouped forwards after their argument checks. ga == nullptr: the loss alone over nsplit
// column splits; else fused with the row gradient ga, nsplit partial slots per row.
// pos: the plain view's SupCon term (no label column; ga required); events: whether the fused kernel's
// launch is bracketed for rsx_kernel_events (the main loss's launches only).
int grouped_forward(const float* A, const float* B, const float* bias, const float* colcnt, const int* row_col,
                    const int* row_beg, const int* row_end, const int* exc_cols, int64_t N, int64_t D, int64_t lda,
                    int64_t ldb, float tau, int precision, int nsplit, float* ws, float* out2, float* ga,
                    hipStream_t st, const PosTerm* pos = nullptr, bool events = true) {
  if (N == 0) return zero_sums(out2, st);
  const GroupedLayout L(N, D, nsplit, precision);
  const bool h16 = precision == RSX_NCE_F16;
  const int64_t rbs = (N + kOwnRows - 1) / kOwnRows;
  GArgs g = grouped_args(A, B, bias, colcnt, row_col, row_beg, row_end, exc_cols, N, D, lda, ldb, tau);
  g.part = ws + L.part;
  if (precision != RSX_NCE_FP32) {  // B's images, kept in ws for the backward's row pass
    const Images im = images_at(ws, L.img, N, D);
    g.bhi = im.bhi;
    g.blo = im.blo;
    launch_split(B, ldb, D, im.bhi, im.blo, h16, st);
    RSX_LAUNCHED();
  }
  if (!ga) {
    g.nsplit = nsplit;
    g.span = split_span(D, nsplit);
    const int blocks = (int)(rbs * nsplit);
    if (precision == RSX_NCE_BF16X3) hipLaunchKernelGGL(nce_grouped_fwd_x3_k, dim3(blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(nce_grouped_fwd_k, dim3(blocks), dim3(256), 0, st, g);
    RSX_LAUNCHED();
    hipLaunchKernelGGL(nce_grouped_merge_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, A, B, bias, row_col, N,
                       lda, ldb, g.inv_tau, nsplit, g.part, ws + L.lse, ws + L.row_loss, ws + L.row_valid);
  } else {
    // the grid (fwdg_schedule): whole rounds of equal workgroups on the leading row blocks, the
    // remaining row blocks on more, shorter splits dispatched last, so the grid's final round is
    // short and full. nsplit 1 and 2 (the grouped loss): whole-row workgroups, then up to 8 splits
    // (batch 8192: 1,024 row blocks x 1 = 2 rounds of 512, then 173 x 8 eighth-length workgroups);
    // 8 (the plain view): 4 splits, then 8. The rows' partial slots follow their region's count.
    const FwdgSchedule sc = fwdg_schedule(N, D, nsplit, 2 * (int64_t)rsx::cu_count());
    const int ns1 = sc.ns1;
    const int64_t rb1 = sc.rb1;
    // the per-slot row gradients [nslots][N][128] go into the backward's split-partial region
    RSX_ARG((int64_t)sc.nslots * N * kD <= L.dpart_cap, "fused forward partials exceed the split-partial region");
    RSX_ARG(sc.blocks < (1ll << 31), "too many workgroups");
    g.nsplit = ns1;
    g.span = sc.span1;
    g.rb1 = rb1;
    g.nsplit2 = sc.ns2;
    g.span2 = sc.span2;
    g.nslots = sc.nslots;
    g.part = ws + L.fwd_part(nsplit);
    g.dout = ws + L.dpart;
    const int blocks = (int)sc.blocks;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (events) {
      KernelEvents& k = kernel_events();
      std::lock_guard<std::mutex> lk(k.mu);
      if (k.on && hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess) {
        (void)hipEventRecord(ev0, st);
        k.ev.emplace_back(ev0, ev1);
      }
    }
    if (h16) launch_grouped_fwdg_h(g, blocks, st);
    else hipLaunchKernelGGL(nce_grouped_fwdg_x3p_k, dim3(blocks), dim3(256), 0, st, g);
    RSX_LAUNCHED();
    if (ev1) (void)hipEventRecord(ev1, st);
    const dim3 mgrid((unsigned)((N + 3) / 4));
    if (pos) {
      hipLaunchKernelGGL(nce_pos_rows_k, mgrid, dim3(256), 0, st, A, B, pos->k1a, pos->k1b, N, D, lda, ldb, pos->off,
                         g.inv_tau, pos->cnt, pos->ps, pos->P);
      RSX_LAUNCHED();
      hipLaunchKernelGGL(nce_grouped_merge_g_k<true>, mgrid, dim3(256), 0, st, A, B, bias, row_col, N, lda, ldb,
                         g.inv_tau, ns1, g.part, g.dout, ws + L.lse, ws + L.row_loss, ws + L.row_valid, ga,
                         rb1 * kOwnRows, sc.ns2, sc.nslots, 0, pos->cnt, pos->ps, pos->P);
    } else {
      hipLaunchKernelGGL(nce_grouped_merge_g_k<false>, mgrid, dim3(256), 0, st, A, B, bias, row_col, N, lda, ldb,
                         g.inv_tau, ns1, g.part, g.dout, ws + L.lse, ws + L.row_loss, ws + L.row_valid, ga,
                         rb1 * kOwnRows, sc.ns2, sc.nslots, h16 ? 1 : 0, nullptr, nullptr, nullptr);
    }
  }
  RSX_LAUNCHED();
  launch_reduce(ws + L.row_loss, ws + L.row_valid, N, out2, st);
  RSX_LAUNCHED();
  return 0;
}

// the fused forward writes up to 8 partial slots per row into the backward's partial region
static_assert(kNsplitBwdGrouped >= 8, "fused forward slots must fit the backward's split-partial region");

}  // namespace

RSX_API int64_t rsx_nce_grouped_workspace_floats(int64_t N, int64_t D, int nsplit_fwd, int nsplit_bwd,
                                                 int precision) {
  return GroupedLayout(N, D, nsplit_fwd, precision, nsplit_bwd).total;
}

RSX_API int rsx_nce_grouped_fwd(const float* A, const float* B, const float* bias, const float* colcnt,
                                const int* row_col, const int* row_beg, const int* row_end, const int* exc_cols,
                                int64_t N, int64_t D, int64_t lda, int64_t ldb, float tau, int precision, int nsplit,
                                float* ws, float* out2, void* stream) {
  RSX_ARG(A && B && colcnt && row_col && row_beg && row_end && exc_cols && ws && out2, "null tensor");
  RSX_ARG(precision == RSX_NCE_FP32 || precision == RSX_NCE_BF16X3 || precision == RSX_NCE_F16,
          "precision must be 0 (fp32), 1 (bf16x3) or 2 (f16)");
  // the loss alone has no gradient product: RSX_NCE_F16 runs the bf16x3 logits here (its B
  // images are bf16, which is what a following row pass of rsx_nce_grouped_bwd reads)
  if (precision == RSX_NCE_F16) precision = RSX_NCE_BF16X3;
  RSX_ARG(nsplit == 1 || nsplit == 2 || nsplit == 4 || (nsplit >= 8 && nsplit <= 64 && nsplit % 8 == 0),
          "nsplit must be 1, 2, 4 or a multiple of 8 in [8,64]");
  NCE_REQUIRE(operand_error(A, B, lda, ldb));
  return grouped_forward(A, B, bias, colcnt, row_col, row_beg, row_end, exc_cols, N, D, lda, ldb, tau, precision,
                         nsplit, ws, out2, nullptr, (hipStream_t)stream);
}

RSX_API int rsx_nce_fwdg_schedule(int64_t N, int64_t D, int nsplit, int cus, int64_t* sched, int64_t* block_map,
                                  int64_t max_blocks) {
  RSX_ARG(sched != nullptr, "null sched");
  RSX_ARG(N >= 0 && D >= 0, "N and D must be >= 0");
  RSX_ARG(nsplit == 1 || nsplit == 2 || nsplit == 4 || nsplit == 8, "nsplit must be 1, 2, 4 or 8");
  const FwdgSchedule sc = fwdg_schedule(N, D, nsplit, 2 * (int64_t)(cus > 0 ? cus : rsx::cu_count()));
  const int64_t v[7] = {sc.rb1, sc.ns1, sc.span1, sc.ns2, sc.span2, sc.nslots, sc.blocks};
  for (int k = 0; k < 7; ++k) sched[k] = v[k];
  if (block_map) {
    for (int64_t b = 0; b < sc.blocks && b < max_blocks; ++b) {
      int split;
      int64_t rb, j0, j1;
      fwdg_block(b, sc.ns1, sc.span1, sc.rb1, sc.ns2, sc.span2, D, split, rb, j0, j1);
      block_map[4 * b] = rb; block_map[4 * b + 1] = split; block_map[4 * b + 2] = j0; block_map[4 * b + 3] = j1;
    }
  }
  return 0;
}

RSX_API int rsx_kernel_events(int on) {
  KernelEvents& k = kernel_events();
  std::lock_guard<std::mutex> g(k.mu);
  k.clear();
  k.on = on != 0;
  return 0;
}

RSX_API int rsx_kernel_events_read(float* ms, int max_n) {
  RSX_ARG(ms != nullptr || max_n == 0, "null output");
  KernelEvents& k = kernel_events();
  std::lock_guard<std::mutex> g(k.mu);
  int n = 0;
  for (auto& e : k.ev) {
    if (n >= max_n) break;
    float t = 0.0f;
    hipError_t err = hipEventSynchronize(e.second);
    if (err == hipSuccess) err = hipEventElapsedTime(&t, e.first, e.second);
    if (err != hipSuccess) {
      rsx::set_error("%s: %s", __func__, hipGetErrorString(err));
      return -1;
    }
    ms[n++] = t;
  }
  return n;
}

RSX_API int rsx_nce_grouped_fwd_grad(const float* A, const float* B, const float* bias, const float* colcnt,
                                     const int* row_col, const int* row_beg, const int* row_end,
                                     const int* exc_cols, int64_t N, int64_t D, int64_t lda, int64_t ldb, float tau,
                                     int precision, int nsplit, float* ws, float* out2, float* ga, void* stream) {
  RSX_ARG(A && B && colcnt && row_col && row_beg && row_end && exc_cols && ws && out2 && ga, "null tensor");
  RSX_ARG(precision == RSX_NCE_BF16X3 || precision == RSX_NCE_F16, "precision must be 1 (bf16x3) or 2 (f16)");
  RSX_ARG(nsplit == 1 || nsplit == 2 || nsplit == 4 || nsplit == 8, "nsplit must be 1, 2, 4 or 8");
  NCE_REQUIRE(operand_error(A, B, lda, ldb));
  return grouped_forward(A, B, bias, colcnt, row_col, row_beg, row_end, exc_cols, N, D, lda, ldb, tau, precision,
                         nsplit, ws, out2, ga, (hipStream_t)stream);
}

RSX_API int rsx_nce_grouped_bwd(const float* A, const float* B, const float* bias, const float* colcnt,
                                const int* row_col, const int* row_beg, const int* row_end, const int* exc_cols,
                                const int* col_beg, const int* col_end, const int* exc_s, const int* exc_e,
                                const int* exc_n, int64_t N, int64_t D, int64_t lda, int64_t ldb, float tau,
                                int precision, int nsplit_fwd, int nsplit, const float* gout, float* ws, float* dA, float* dB,
                                int accumulate, void* stream) {
  RSX_ARG(gout != nullptr && ws != nullptr, "gout/ws required");
  RSX_ARG(nsplit == kNsplitBwdGrouped, "grouped backward nsplit must be 8");
  RSX_ARG(precision == RSX_NCE_FP32 || precision == RSX_NCE_BF16X3 || precision == RSX_NCE_F16,
          "precision must be 0 (fp32), 1 (bf16x3) or 2 (f16)");
  RSX_ARG(!dB || (col_beg && col_end && exc_s && exc_e && exc_n), "column exception lists required for dB");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return 0;
  const GroupedLayout L(N, D, nsplit_fwd, precision);
  const bool h16 = precision == RSX_NCE_F16;
  const bool x3 = precision != RSX_NCE_FP32;
  const Images im = x3 ? images_at(ws, L.img, N, D) : Images{};
  GArgs g = grouped_args(A, B, bias, colcnt, row_col, row_beg, row_end, exc_cols, N, D, lda, ldb, tau);
  g.col_beg = col_beg; g.col_end = col_end; g.exc_s = exc_s; g.exc_e = exc_e; g.exc_n = exc_n;
  g.lse = ws + L.lse;
  g.row_loss = ws + L.row_loss;
  g.gout = gout;
  g.dout = ws + L.dpart;
  g.ahi = im.ahi; g.alo = im.alo; g.bhi = im.bhi; g.blo = im.blo;
  for (int pass = 0; pass < 2; ++pass) {
    const bool row_owned = pass == 0;
    float* target = row_owned ? dA : dB;
    if (!target) continue;
    const int64_t n_own = row_owned ? N : D;
    const int64_t n_str = row_owned ? D : N;
    if (n_own == 0) continue;
    // split count of this pass: fewer splits when the owner side alone fills the chip (>= 1024
    // workgroups), which halves the partial-gradient traffic of the row pass
    const int64_t own_blocks = (n_own + kOwnRows - 1) / kOwnRows;
    int ps = (own_blocks * 4 >= 1024) ? 4 : nsplit;
    g.split_major = 0;
    if (!row_owned && x3) {
      // column pass: 32 (else 16) splits in a split-major block order, so each XCD's L2 holds the
      // one split of A's images it streams (the 8-split span, N/8 rows = 9.8 MB at batch 8192, does
      // not fit a 4-MB L2): 5.5 -> 5.0-5.1 ms at batch 8192 (profiles/r02_nce_colsplit_ab.json).
      // Bounded by the partial region.
      for (int want : {32, 16}) {
        if ((int64_t)want * n_own * kD <= L.dpart_cap && N >= (int64_t)want * 2 * kTile) {
          ps = want;
          g.split_major = 1;
          break;
        }
      }
    }
    RSX_ARG((int64_t)ps * n_own * kD <= L.dpart_cap, "split partials exceed their workspace region");
    g.nsplit = ps;
    g.span = split_span(n_str, ps);
    const int blocks = (int)(own_blocks * ps);
    if (x3 && !row_owned) {  // B's images come from the forward; A's are made here, for the col pass
      launch_split(A, lda, N, im.ahi, im.alo, h16, st);
      RSX_LAUNCHED();
    } else if (h16 && row_owned) {  // the row pass streams bf16 images of B (a fused f16 forward left fp16 ones)
      launch_split(B, ldb, D, im.bhi, im.blo, false, st);
      RSX_LAUNCHED();
    }
    if (!row_owned && h16) launch_grouped_bwd_cols_h(g, blocks, st);
    else if (row_owned && x3) hipLaunchKernelGGL((nce_grouped_bwd_x3_k<true, false>), dim3(blocks), dim3(256), 0, st, g);
    else if (x3) hipLaunchKernelGGL((nce_grouped_bwd_x3_k<false, true>), dim3(blocks), dim3(256), 0, st, g);
    else if (row_owned) hipLaunchKernelGGL(nce_grouped_bwd_k<true>, dim3(blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(nce_grouped_bwd_k<false>, dim3(blocks), dim3(256), 0, st, g);
    RSX_LAUNCHED();
    launch_sum_splits(g.dout, ps, n_own, target, accumulate, st);
    RSX_LAUNCHED();
  }
  return 0;
}

// ---- plain-family view of the fused kernels (include/recsys_amd.h) --------------------------
namespace {

// the view's arguments checked, and the grouped arguments over its arrays
const char* fused_error(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, int64_t N,
                        int64_t M, int64_t lda, int64_t ldb, int64_t off, int flags) {
  if (!(flags == 0 || (flags == (F_EXCL_DIAG | F_POS) && bias == nullptr)))
    return "fused plain view: flags must be 0, or 9 without a bias";
  if (flags != 0 && !(k1a && k1b)) return "flags 9 needs k1a and k1b";
  if (!(N >= 0 && M >= 0 && N < (1ll << 30) && M < (1ll << 30))) return "N and M must be in [0, 2^30)";
  if (const char* e = operand_error(A, B, lda, ldb)) return e;
  return diag_error(N, M, off);
}

GArgs view_args(const float* A, const float* B, const float* bias, const int* view, int64_t N, int64_t M, int64_t lda,
                int64_t ldb, float tau, int flags) {
  const ViewLayout V(N, M);
  GArgs g = grouped_args(A, B, bias, reinterpret_cast<const float*>(view + V.colcnt),
                         view + (flags == 0 ? V.lab : V.none), view + V.beg, view + V.end, view + V.lab, N, M, lda,
                         ldb, tau);
  g.col_beg = view + V.col_beg;
  g.col_end = view + V.col_end;
  g.exc_s = view + V.beg;
  g.exc_e = view + V.end;
  g.exc_n = view + V.one;
  return g;
}

}  // namespace

RSX_API int64_t rsx_nce_fused_workspace_floats(int64_t N, int64_t M) {
  return FusedLayout(N, M).total;
}

RSX_API int64_t rsx_nce_view_ints(int64_t N, int64_t M) { return ViewLayout(N, M).total; }

RSX_API int rsx_nce_view_fill_host(int64_t N, int64_t M, int64_t diag_offset, int* view) {
  RSX_ARG(view != nullptr || ViewLayout(N, M).total == 0, "null view");
  NCE_REQUIRE(diag_error(N, M, diag_offset));
  const int64_t total = ViewLayout(N, M).total;
  for (int64_t k = 0; k < total; ++k) view[k] = view_entry(k, N, M, diag_offset);
  return 0;
}

RSX_API int rsx_nce_view_fill(int64_t N, int64_t M, int64_t diag_offset, int* view, void* stream) {
  RSX_ARG(view != nullptr, "null view");
  RSX_ARG(N >= 0 && M >= 0 && N < (1ll << 30) && M < (1ll << 30), "N and M must be in [0, 2^30)");
  NCE_REQUIRE(diag_error(N, M, diag_offset));
  const int64_t total = ViewLayout(N, M).total;
  if (total == 0) return 0;
  hipLaunchKernelGGL(nce_view_fill_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, view,
                     N, M, diag_offset, total);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_nce_fwd_grad(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                             int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau, int flags,
                             const int* view, float* ws, float* out2, float* ga, void* stream) {
  RSX_ARG(A && B && view && ws && out2 && ga, "null tensor");
  NCE_REQUIRE(fused_error(A, B, bias, k1a, k1b, N, M, lda, ldb, diag_offset, flags));
  const FusedLayout L(N, M);
  const GArgs g = view_args(A, B, bias, view, N, M, lda, ldb, tau, flags);
  const PosTerm pos = {k1a, k1b, diag_offset, ws + L.pos_cnt, ws + L.pos_ps, ws + L.pos_P};
  return grouped_forward(A, B, bias, g.colcnt, g.row_col, g.row_beg, g.row_end, g.exc_cols, N, M, lda, ldb, tau,
                         RSX_NCE_BF16X3, kNsplitFused, ws, out2, ga, (hipStream_t)stream, flags == 0 ? nullptr : &pos,
                         false);
}

RSX_API int rsx_nce_bwd_cols(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                             int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau, int flags,
                             const int* view, const float* gout, float* ws, float* dB, void* stream) {
  RSX_ARG(A && B && view && ws && gout && dB, "null tensor");
  NCE_REQUIRE(fused_error(A, B, bias, k1a, k1b, N, M, lda, ldb, diag_offset, flags));
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return 0;
  if (N == 0) {
    (void)hipMemsetAsync(dB, 0, (size_t)M * kD * sizeof(float), st);
    RSX_LAUNCHED();
    return 0;
  }
  const FusedLayout L(N, M);
  const Images im = images_at(ws, L.img, N, M);
  GArgs g = view_args(A, B, bias, view, N, M, lda, ldb, tau, flags);
  g.lse = ws + L.lse;
  g.gout = gout;
  g.dout = ws + L.dpart;
  g.ahi = im.ahi; g.alo = im.alo; g.bhi = im.bhi; g.blo = im.blo;
  // 8 row splits: at batch 8192 the 64 owner blocks x 8 fill one round of two workgroups per CU
  g.nsplit = kNsplitFused;
  g.span = split_span(N, kNsplitFused);
  g.split_major = 0;
  const int64_t own_blocks = (M + kOwnRows - 1) / kOwnRows;
  RSX_ARG(own_blocks * kNsplitFused < (1ll << 31), "too many workgroups");
  const int blocks = (int)(own_blocks * kNsplitFused);
  launch_split(A, lda, N, im.ahi, im.alo, false, st);
  RSX_LAUNCHED();
  hipLaunchKernelGGL((nce_grouped_bwd_x3_k<false, true>), dim3(blocks), dim3(256), 0, st, g);
  RSX_LAUNCHED();
  launch_sum_splits(g.dout, kNsplitFused, M, dB, 0, st);
  RSX_LAUNCHED();
  if (flags != 0) {
    hipLaunchKernelGGL(nce_pos_cols_k, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, A, k1a, k1b, N, M, lda,
                       diag_offset, g.inv_tau, ws + L.pos_cnt, gout, dB);
    RSX_LAUNCHED();
  }
  return 0;
}
