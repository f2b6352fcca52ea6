// Fused in-batch contrastive cross-entropy (InfoNCE) over an implicit N x M logit
// matrix that is never materialised:
//
//   S_ij = <A_i, B_j> * (1/tau) - bias_j
//   S_ij = -inf   if excluded(i,j)
//   row loss_i = LSE_j S_ij - label term
//
// Reference semantics covered (file:line in /root/reference):
//   * inbatch_corrected_logq_loss  tower_code/v1_refine_usertower.py:826-861 (live def):
//       bias_j = logQ[t_j]*lambda, excluded = (t_i==t_j || user_i==user_j) && i!=j, label = diag
//   * inbatch_corrected_logq_loss  v1_refine_usertower.py:520-573 (shadowed def): same, no user key
//   * duorec_loss_refined unsup    v1_refine_usertower.py:588-590: no bias/masks, label = diag
//   * duorec_loss_refined sup      v1_refine_usertower.py:595-625: excluded = (i==j),
//       positives M_ij = (t_i==t_j) && t_i!=0 && i!=j, loss_i = LSE_i - sum_j M_ij S_ij / sum_j M_ij
//   * item-tower SimCSE loss       item_tower.py:1075-1082 (both directions = two calls)
//
// Dot products run on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact f32 FMA chain,
// no reduced-precision path on gfx950). Each wave keeps 32 rows of its "owner" operand
// in registers (64 VGPRs, k permuted as k = 64*h + s so each lane holds a contiguous
// half row) and streams 32-row tiles of the other operand through LDS. The accumulator
// tile is computed transposed (streamed rows in registers, owner row on the lane), so
// the online log-sum-exp is lane-local and the tile doubles as the A operand of the
// gradient MFMA in the backward (no LDS round trip for dS).
#include "rsx_common.h"
#include <math.h>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 128;        // embedding width (fixed by the reference: d_model=128)
constexpr int kTile = 32;      // streamed rows per tile
constexpr int kWaves = 4;      // waves per workgroup
constexpr int kOwnRows = 32 * kWaves;  // owner rows per workgroup
constexpr int kLdsStride = kD + 4;     // padded row (conflict-free ds_read_b128 columns)

enum : int { F_EXCL_DIAG = 1, F_MASK_K1 = 2, F_MASK_K2 = 4, F_POS = 8 };
enum : int { RSX_NCE_FP32 = 0, RSX_NCE_BF16X3 = 1, RSX_NCE_F16 = 2 };
constexpr int kNsplitBwdGrouped = 8;  // fixed: the image region's offset in ws depends on it  // logit/gradient precision of the grouped kernels

struct FwdArgs {
  const float* A;     // [N, lda] owner rows (queries)
  const float* B;     // [M, ldb] streamed rows (columns)
  const float* bias;  // [M] or nullptr
  const int* k1a;     // [N] or nullptr
  const int* k1b;     // [M]
  const int* k2a;
  const int* k2b;
  int64_t N, M, lda, ldb;
  int64_t diag_off;  // row i's label / diagonal column is i + diag_off (data-parallel shards)
  float inv_tau;
  int nsplit;
  int64_t cols_per_split;
  float* part;  // [4][nsplit][N] : running max, sum-exp, positive-logit sum, positive count
};

__device__ __forceinline__ int tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Block-id remap: all workgroups of one column split share an XCD group (b % 8), so the
// split's streamed operand is re-read from that XCD's L2. Speed only, never correctness.
__device__ __forceinline__ void remap_block(int nsplit, int& split, int& rb) {
  const int b = blockIdx.x;
  const int xcd = b & 7, q = b >> 3;
  if (nsplit >= 8) {  // multiple of 8: each split on one XCD group
    const int nsub = nsplit >> 3;
    split = xcd + 8 * (q % nsub);
    rb = q / nsub;
  } else {  // nsplit in {1, 2, 4}: 8 / nsplit XCD groups per split
    split = xcd % nsplit;
    rb = (8 / nsplit) * q + xcd / nsplit;
  }
}

template <int FL>
__global__ __launch_bounds__(256, 2) void nce_fwd_k(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sB[2][kTile][kLdsStride];
  __shared__ __attribute__((aligned(16))) float sBias[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK1[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK2[2][kTile];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;

  float u[64];
  if (row_ok) {
    const float4* src = reinterpret_cast<const float4*>(a.A + i * a.lda + h * 64);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float4 v = src[t];
      u[4 * t + 0] = v.x; u[4 * t + 1] = v.y; u[4 * t + 2] = v.z; u[4 * t + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 64; ++t) u[t] = 0.0f;
  }
  int k1i = 0, k2i = 0;
  if (row_ok) {
    if ((FL & (F_MASK_K1 | F_POS)) && a.k1a) k1i = a.k1a[i];
    if ((FL & F_MASK_K2) && a.k2a) k2i = a.k2a[i];
  }

  const int64_t j_begin = (int64_t)split * a.cols_per_split;
  int64_t j_end = j_begin + a.cols_per_split;
  if (j_end > a.M) j_end = a.M;

  float m = -INFINITY, l = 0.0f, ps = 0.0f, pc = 0.0f;

  const int srow = tid >> 3, scol = (tid & 7) * 16;
  float4 stg[4];
  float stg_bias = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;

  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + srow;
    if (j < j_end) {
      const float4* src = reinterpret_cast<const float4*>(a.B + j * a.ldb + scol);
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = src[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_bias = (ok && a.bias) ? a.bias[jj] : 0.0f;
      stg_k1 = (ok && a.k1b) ? a.k1b[jj] : 0;
      stg_k2 = (ok && a.k2b) ? a.k2b[jj] : 0;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<float4*>(&sB[buf][srow][scol + 4 * t]) = stg[t];
    if (tid < kTile) {
      sBias[buf][tid] = stg_bias;
      sK1[buf][tid] = stg_k1;
      sK2[buf][tid] = stg_k2;
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

      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      const float* brow = &sB[cur][c][h * 64];
#pragma unroll
      for (int s = 0; s < 64; s += 4) {
        const float4 bv = *reinterpret_cast<const float4*>(brow + s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, u[s + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, u[s + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.z, u[s + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.w, u[s + 3], acc, 0, 0, 0);
      }

      float v[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int rbase = 8 * q4 + 4 * h;
        const float4 bi4 = *reinterpret_cast<const float4*>(&sBias[cur][rbase]);
        const int4 k14 = *reinterpret_cast<const int4*>(&sK1[cur][rbase]);
        const int4 k24 = *reinterpret_cast<const int4*>(&sK2[cur][rbase]);
        const float bia[4] = {bi4.x, bi4.y, bi4.z, bi4.w};
        const int kk1[4] = {k14.x, k14.y, k14.z, k14.w};
        const int kk2[4] = {k24.x, k24.y, k24.z, k24.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          const int64_t j = j0 + rbase + e;
          const float s = acc[r] * a.inv_tau - bia[e];
          bool excl = (j >= j_end) || !row_ok;
          const bool offdiag = (j != i + a.diag_off);
          if (FL & F_EXCL_DIAG) excl = excl || !offdiag;
          if (FL & F_MASK_K1) excl = excl || (offdiag && kk1[e] == k1i);
          if (FL & F_MASK_K2) excl = excl || (offdiag && kk2[e] == k2i);
          if (FL & F_POS) {
            if (!excl && offdiag && kk1[e] == k1i && k1i != 0) {
              ps += s;
              pc += 1.0f;
            }
          }
          v[r] = excl ? -INFINITY : s;
          tmax = fmaxf(tmax, v[r]);
        }
      }
      if (tmax > m) {
        l = (m == -INFINITY) ? 0.0f : l * __expf(m - tmax);
        m = tmax;
      }
      if (m != -INFINITY) {
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += __expf(v[r] - m);
        l += t;
      }
      __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  // fold the two lane halves (same row i, complementary column sets)
  const float m2 = __shfl_xor(m, 32, 64);
  const float l2 = __shfl_xor(l, 32, 64);
  const float ps2 = __shfl_xor(ps, 32, 64);
  const float pc2 = __shfl_xor(pc, 32, 64);
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (mm != -INFINITY) {
    if (m != -INFINITY) ll += l * __expf(m - mm);
    if (m2 != -INFINITY) ll += l2 * __expf(m2 - mm);
  }
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)a.nsplit * a.N;
    const int64_t o = (int64_t)split * a.N + i;
    a.part[o] = mm;
    a.part[stride + o] = ll;
    a.part[2 * stride + o] = ps + ps2;
    a.part[3 * stride + o] = pc + pc2;
  }
}

// ---------------------------------------------------------------------------------
// Merge the column splits: LSE, label term, per-row loss/valid/1-over-count.
struct MergeArgs {
  const float* A;
  const float* B;
  const float* bias;
  int64_t N, lda, ldb;
  int64_t diag_off;
  float inv_tau;
  int nsplit;
  const float* part;
  int pos_mode;      // 0: label = diagonal, 1: label = positive set
  float* lse;        // [N]
  float* row_loss;   // [N]
  float* row_valid;  // [N] 0/1
  float* inv_cnt;    // [N] (pos mode) or nullptr
};

__global__ __launch_bounds__(256) void nce_merge_k(MergeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const int64_t stride = (int64_t)a.nsplit * a.N;
  // every lane reads a split (nsplit <= 64 asserted on host)
  float m = -INFINITY, l = 0.0f, ps = 0.0f, pc = 0.0f;
  if (lane < a.nsplit) {
    const int64_t o = (int64_t)lane * a.N + i;
    m = a.part[o];
    l = a.part[stride + o];
    ps = a.part[2 * stride + o];
    pc = a.part[3 * stride + o];
  }
  float mm = m;
  for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
  float t = (m == -INFINITY) ? 0.0f : l * __expf(m - mm);
  for (int o = 32; o > 0; o >>= 1) {
    t += __shfl_xor(t, o, 64);
    ps += __shfl_xor(ps, o, 64);
    pc += __shfl_xor(pc, o, 64);
  }
  const float lse = (mm == -INFINITY) ? -INFINITY : mm + logf(t);
  float loss, valid, icnt = 0.0f;
  if (!a.pos_mode) {
    // diagonal logit S_ii (same expression as the fused kernel)
    const float2 x = reinterpret_cast<const float2*>(a.A + i * a.lda)[lane];
    const float2 y = reinterpret_cast<const float2*>(a.B + (i + a.diag_off) * a.ldb)[lane];
    float d = x.x * y.x + x.y * y.y;
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    const float sii = d * a.inv_tau - (a.bias ? a.bias[i + a.diag_off] : 0.0f);
    loss = lse - sii;
    valid = 1.0f;
  } else {
    valid = pc > 0.0f ? 1.0f : 0.0f;
    icnt = pc > 0.0f ? 1.0f / pc : 0.0f;
    loss = pc > 0.0f ? lse - ps / pc : 0.0f;
  }
  if (lane == 0) {
    a.lse[i] = lse;
    a.row_loss[i] = loss;
    a.row_valid[i] = valid;
    if (a.inv_cnt) a.inv_cnt[i] = icnt;
  }
}

// Deterministic single-workgroup sums over rows. out[0] = sum of row losses, out[1] = n_valid.
__global__ __launch_bounds__(1024) void nce_reduce_k(const float* row_loss, const float* row_valid, int64_t N,
                                                      float* out) {
  __shared__ float s_l[1024], s_v[1024];
  float l = 0.0f, v = 0.0f;
  for (int64_t i = threadIdx.x; i < N; i += 1024) {
    l += row_loss[i];
    v += row_valid[i];
  }
  s_l[threadIdx.x] = l;
  s_v[threadIdx.x] = v;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_l[threadIdx.x] += s_l[threadIdx.x + o];
      s_v[threadIdx.x] += s_v[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = s_l[0];
    out[1] = s_v[0];
  }
}

// ---------------------------------------------------------------------------------
// Backward. G_ij = w_i * (P_ij - Y_ij) / tau, P_ij = exp(S_ij - LSE_i) (0 if excluded),
// Y = diagonal (pos_mode 0) or M_ij / cnt_i (pos_mode 1), w_i = g * valid_i where g is the
// upstream gradient of the row-loss SUM (device scalar).
// ROW_OWNED: dA_i = sum_j G_ij B_j ; else dB_j = sum_i G_ij A_i.
struct BwdArgs {
  const float* A;
  const float* B;
  const float* bias;
  const int* k1a;
  const int* k1b;
  const int* k2a;
  const int* k2b;
  int64_t N, M, lda, ldb;
  int64_t diag_off;
  float inv_tau;
  const float* lse;
  const float* row_valid;
  const float* inv_cnt;
  const float* gout;   // upstream gradient of the row-loss sum (device scalar)
  int nsplit;
  int64_t span_per_split;  // streamed rows per split
  float* dout;             // [nsplit][owner_rows][128] (split partials) or final when nsplit==1
};

template <int FL, bool ROW_OWNED>
__global__ __launch_bounds__(256, 2) void nce_bwd_k(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float sX[2][kTile][kLdsStride];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // row side: lse_i | col side: bias_j
  __shared__ __attribute__((aligned(16))) float sM1[2][kTile];  // row side: w_i
  __shared__ __attribute__((aligned(16))) float sM2[2][kTile];  // row side: inv_cnt_i
  __shared__ __attribute__((aligned(16))) int sK1[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK2[2][kTile];

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
  const float g_scale = a.gout[0] * a.inv_tau;

  const int64_t o = (int64_t)ob * kOwnRows + wave * 32 + c;  // this lane's owner index
  const bool own_ok = o < n_own;
  float u[64];
  if (own_ok) {
    const float4* src = reinterpret_cast<const float4*>(own + o * ld_own + h * 64);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float4 v = src[t];
      u[4 * t + 0] = v.x; u[4 * t + 1] = v.y; u[4 * t + 2] = v.z; u[4 * t + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 64; ++t) u[t] = 0.0f;
  }
  // owner-side metadata
  float o_lse = 0.0f, o_w = 0.0f, o_icnt = 0.0f, o_bias = 0.0f;
  int o_k1 = 0, o_k2 = 0;
  if (own_ok) {
    if (ROW_OWNED) {
      o_lse = a.lse[o];
      o_w = a.row_valid[o] * g_scale;
      if ((FL & F_POS) && a.inv_cnt) o_icnt = a.inv_cnt[o];
      if ((FL & (F_MASK_K1 | F_POS)) && a.k1a) o_k1 = a.k1a[o];
      if ((FL & F_MASK_K2) && a.k2a) o_k2 = a.k2a[o];
    } else {
      o_bias = a.bias ? a.bias[o] : 0.0f;
      if ((FL & (F_MASK_K1 | F_POS)) && a.k1b) o_k1 = a.k1b[o];
      if ((FL & F_MASK_K2) && a.k2b) o_k2 = a.k2b[o];
    }
  }

  const int64_t s_begin = (int64_t)split * a.span_per_split;
  int64_t s_end = s_begin + a.span_per_split;
  if (s_end > n_str) s_end = n_str;

  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;

  const int srow = tid >> 3, scol = (tid & 7) * 16;
  float4 stg[4];
  float stg0 = 0.0f, stg1 = 0.0f, stg2 = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;

  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + srow;
    if (sidx < s_end) {
      const float4* src = reinterpret_cast<const float4*>(str + sidx * ld_str + scol);
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = src[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      if (ROW_OWNED) {  // streamed = columns j
        stg0 = (ok && a.bias) ? a.bias[ss] : 0.0f;
        stg_k1 = (ok && a.k1b) ? a.k1b[ss] : 0;
        stg_k2 = (ok && a.k2b) ? a.k2b[ss] : 0;
      } else {  // streamed = rows i
        stg0 = ok ? a.lse[ss] : 0.0f;
        stg1 = ok ? a.row_valid[ss] * g_scale : 0.0f;
        stg2 = (ok && a.inv_cnt) ? a.inv_cnt[ss] : 0.0f;
        stg_k1 = (ok && a.k1a) ? a.k1a[ss] : 0;
        stg_k2 = (ok && a.k2a) ? a.k2a[ss] : 0;
      }
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<float4*>(&sX[buf][srow][scol + 4 * t]) = stg[t];
    if (tid < kTile) {
      sM0[buf][tid] = stg0;
      sM1[buf][tid] = stg1;
      sM2[buf][tid] = stg2;
      sK1[buf][tid] = stg_k1;
      sK2[buf][tid] = stg_k2;
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

      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      const float* xrow = &sX[cur][c][h * 64];
#pragma unroll
      for (int s = 0; s < 64; s += 4) {
        const float4 bv = *reinterpret_cast<const float4*>(xrow + s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, u[s + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, u[s + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.z, u[s + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.w, u[s + 3], acc, 0, 0, 0);
      }

      // acc[r] = <own_o, str_s>, s = s0 + tile_row(r,h). Turn it into G (in place).
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int rbase = 8 * q4 + 4 * h;
        const float4 m04 = *reinterpret_cast<const float4*>(&sM0[cur][rbase]);
        const float4 m14 = *reinterpret_cast<const float4*>(&sM1[cur][rbase]);
        const float4 m24 = *reinterpret_cast<const float4*>(&sM2[cur][rbase]);
        const int4 k14 = *reinterpret_cast<const int4*>(&sK1[cur][rbase]);
        const int4 k24 = *reinterpret_cast<const int4*>(&sK2[cur][rbase]);
        const float mm0[4] = {m04.x, m04.y, m04.z, m04.w};
        const float mm1[4] = {m14.x, m14.y, m14.z, m14.w};
        const float mm2[4] = {m24.x, m24.y, m24.z, m24.w};
        const int kk1[4] = {k14.x, k14.y, k14.z, k14.w};
        const int kk2[4] = {k24.x, k24.y, k24.z, k24.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          const int64_t sidx = s0 + rbase + e;
          // resolve (i, j) and their metadata
          int64_t ii, jj;
          float lse_i, w_i, icnt_i, bias_j;
          int k1_i, k1_j, k2_i, k2_j;
          if (ROW_OWNED) {
            ii = o; jj = sidx;
            lse_i = o_lse; w_i = o_w; icnt_i = o_icnt; bias_j = mm0[e];
            k1_i = o_k1; k1_j = kk1[e]; k2_i = o_k2; k2_j = kk2[e];
          } else {
            ii = sidx; jj = o;
            lse_i = mm0[e]; w_i = mm1[e]; icnt_i = mm2[e]; bias_j = o_bias;
            k1_i = kk1[e]; k1_j = o_k1; k2_i = kk2[e]; k2_j = o_k2;
          }
          const float sv = acc[r] * a.inv_tau - bias_j;
          bool excl = (sidx >= s_end) || !own_ok;
          const bool offdiag = (jj != ii + a.diag_off);
          if (FL & F_EXCL_DIAG) excl = excl || !offdiag;
          if (FL & F_MASK_K1) excl = excl || (offdiag && k1_i == k1_j);
          if (FL & F_MASK_K2) excl = excl || (offdiag && k2_i == k2_j);
          float y = 0.0f;
          if (FL & F_POS) {
            if (!excl && offdiag && k1_i == k1_j && k1_i != 0) y = icnt_i;
          } else {
            y = offdiag ? 0.0f : 1.0f;
          }
          const float p = (excl || lse_i == -INFINITY) ? 0.0f : __expf(sv - lse_i);
          acc[r] = excl ? 0.0f : w_i * (p - y);
        }
      }

      // gradient MFMA: d_own[o][kb*32 + n] += sum_s G[o][s] * str[s][kb*32 + n]
      // A operand (lane c,h, step t) = G[own=c][str=tile_row(t,h)] = acc[t]
      // B operand = str[tile_row(t,h)][kb*32 + c]
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float* srow_p = &sX[cur][tile_row(t, h)][c];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          gacc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[t], srow_p[kb * 32], gacc[kb], 0, 0, 0);
      }

      __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  // write d_own rows: D[row = own-local tile_row(r,h)][col = kb*32 + c]
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  float* dst = a.dout + (int64_t)split * n_own * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r];
    }
  }
}

// Sum split partials: out[i][k] (+)= sum_s part[s][i][k]
__global__ __launch_bounds__(256) void nce_sum_splits_k(const float* part, int nsplit, int64_t n, float* out,
                                                         int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
  const int64_t total4 = n * kD / 4;
  if (idx >= total4) return;
  float4 s = reinterpret_cast<const float4*>(part)[idx];
#pragma unroll 8
  for (int k = 1; k < nsplit; ++k) {
    const float4 v = reinterpret_cast<const float4*>(part + (int64_t)k * n * kD)[idx];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (accumulate) {
    const float4 v = reinterpret_cast<const float4*>(out)[idx];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  reinterpret_cast<float4*>(out)[idx] = s;
}

template <int FL>
void launch_fwd_t(const FwdArgs& a, int blocks, hipStream_t st) {
  hipLaunchKernelGGL(nce_fwd_k<FL>, dim3(blocks), dim3(256), 0, st, a);
}

template <int FL>
void launch_bwd_t(const BwdArgs& a, bool row_owned, int blocks, hipStream_t st) {
  if (row_owned) hipLaunchKernelGGL((nce_bwd_k<FL, true>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((nce_bwd_k<FL, false>), dim3(blocks), dim3(256), 0, st, a);
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

bool valid_flags(int f) {
  // supported combinations (see header)
  return f == 0 || f == F_MASK_K1 || f == (F_MASK_K1 | F_MASK_K2) || f == (F_EXCL_DIAG | F_POS);
}

// fn(std::integral_constant<int, FL>) for the kernel instantiation FL of a valid flag combination
template <typename Fn>
void with_flags(int flags, Fn&& fn) {
  switch (flags) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case F_MASK_K1: fn(std::integral_constant<int, F_MASK_K1>{}); break;
    case F_MASK_K1 | F_MASK_K2: fn(std::integral_constant<int, F_MASK_K1 | F_MASK_K2>{}); break;
    default: fn(std::integral_constant<int, F_EXCL_DIAG | F_POS>{}); break;
  }
}

// Arguments of the plain forward over nsplit column splits; ws = part [4][nsplit][N], then the
// lse / row_loss / row_valid / inv_cnt rows that plain_fwd_finish fills.
FwdArgs plain_fwd_args(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                       const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                       int64_t diag_offset, float tau, int nsplit, float* ws) {
  FwdArgs fa;
  fa.A = A; fa.B = B; fa.bias = bias;
  fa.k1a = k1a; fa.k1b = k1b; fa.k2a = k2a; fa.k2b = k2b;
  fa.N = N; fa.M = M; fa.lda = lda; fa.ldb = ldb;
  fa.diag_off = diag_offset;
  fa.inv_tau = 1.0f / tau;
  fa.nsplit = nsplit;
  fa.cols_per_split = round_up((M + nsplit - 1) / nsplit, kTile);
  if (fa.cols_per_split < kTile) fa.cols_per_split = kTile;
  fa.part = ws;
  return fa;
}

// Merges the forward's split partials into the per-row statistics and reduces them to out2.
int plain_fwd_finish(const FwdArgs& fa, int flags, float* out2, hipStream_t st) {
  float* lse = fa.part + 4 * (int64_t)fa.nsplit * fa.N;
  float* row_loss = lse + fa.N;
  float* row_valid = row_loss + fa.N;
  MergeArgs ma;
  ma.A = fa.A; ma.B = fa.B; ma.bias = fa.bias;
  ma.N = fa.N; ma.lda = fa.lda; ma.ldb = fa.ldb;
  ma.diag_off = fa.diag_off;
  ma.inv_tau = fa.inv_tau;
  ma.nsplit = fa.nsplit;
  ma.part = fa.part;
  ma.pos_mode = (flags & F_POS) ? 1 : 0;
  ma.lse = lse; ma.row_loss = row_loss; ma.row_valid = row_valid; ma.inv_cnt = row_valid + fa.N;
  hipLaunchKernelGGL(nce_merge_k, dim3((unsigned)((fa.N + 3) / 4)), dim3(256), 0, st, ma);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(nce_reduce_k, dim3(1), dim3(1024), 0, st, row_loss, row_valid, fa.N, out2);
  RSX_LAUNCHED();
  return 0;
}


// =====================================================================================
// Grouped form of the live LogQ loss (v1_refine_usertower.py:826-861).
// The logit S_ij depends on column j only through its target t_j, so the N x N problem is
// evaluated over the D distinct targets of the batch with exact integer multiplicities:
//   w_{i,d} = 1                         if d == d(i) (the row's own target: only j == i survives
//                                       the same-item mask)
//           = c_d - n_{u_i,d}           otherwise (c_d: columns with target d, n_{u,d}: those
//                                       belonging to row i's user, removed by the same-user mask)
//   LSE_i = log sum_d w_{i,d} exp(x_{i,d}),  x_{i,d} = <A_i,B_d>/tau - bias_d
// This is the same sum as the reference's (only the summation order differs); FLOPs drop by
// N / D (4.7x on Zipf(1.0) H&M-shaped batches). The user's own targets are the sparse
// exceptions, walked with a monotone pointer per lane.
struct GArgs {
  const float* A;        // [N, lda] rows (normalised user steps)
  const float* B;        // [D, ldb] distinct target rows (normalised item vectors)
  const float* bias;     // [D] logQ * lambda (nullable)
  const float* colcnt;   // [D] c_d
  const int* row_col;    // [N] d(i)
  const int* row_beg;    // [N] row exception list range [row_beg, row_end) in exc_cols
  const int* row_end;
  const int* exc_cols;   // sorted d values of the row's user's targets (with repeats)
  const int* col_beg;    // [D] column exception list range into exc_s/exc_e/exc_n
  const int* col_end;
  const int* exc_s;      // user row range [s, e) and multiplicity n_{u,d}, sorted by s
  const int* exc_e;
  const int* exc_n;
  int64_t N, M, lda, ldb;
  float inv_tau;
  int nsplit;
  int64_t span;          // streamed rows per split
  float* part;           // fwd: [4][nsplit][N]
  const float* lse;      // bwd
  const float* gout;     // bwd: gradient of the row-loss sum
  float* dout;           // bwd: [nsplit][owner][128]
  const __bf16* ahi;     // bf16x3: hi/lo images of A [N][128] and B [M][128]
  const __bf16* alo;
  const __bf16* bhi;
  const __bf16* blo;
  // fused forward, tail-split geometry (fwdg_geometry): row blocks [0, rb1) run nsplit splits of
  // span columns, the rest nsplit2 splits of span2; partial slots per row: nslots
  int64_t rb1, span2;
  int nsplit2, nslots;
  int split_major;       // grouped backward: split-major block order (nce_grouped_bwd_x3_k)
};

__device__ __forceinline__ int lower_bound_i(const int* a, int lo, int hi, int64_t key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Block geometry of the fused forward (nce_grouped_fwdg_x3p_k). Row blocks [0, rb1)
// run a.nsplit column splits, the rest a.nsplit2 (finer: their workgroups are shorter and are
// dispatched last, so the final round of the grid is filled by short workgroups instead of a
// third of the chip running long ones). Each region keeps the XCD-aware remap of remap_block.
__device__ __forceinline__ void fwdg_geometry(const GArgs& a, int& split, int64_t& rb, int64_t& j_begin,
                                              int64_t& j_end) {
  const int64_t b = blockIdx.x, n1 = a.rb1 * a.nsplit;
  int64_t span;
  if (b < n1) {
    const int xcd = (int)(b & 7);
    const int64_t q = b >> 3;
    if (a.nsplit >= 8) {
      const int nsub = a.nsplit >> 3;
      split = xcd + 8 * (int)(q % nsub);
      rb = q / nsub;
    } else {
      split = xcd % a.nsplit;
      rb = (8 / a.nsplit) * q + xcd / a.nsplit;
    }
    span = a.span;
  } else {  // n1 is a multiple of 8 (host), so b & 7 still names the XCD group
    const int64_t b2 = b - n1;
    const int xcd = (int)(b2 & 7);
    const int64_t q = b2 >> 3;
    const int nsub = a.nsplit2 >> 3;  // nsplit2 in {8, 16, ...}
    split = xcd + 8 * (int)(q % nsub);
    rb = a.rb1 + q / nsub;
    span = a.span2;
  }
  j_begin = (int64_t)split * span;
  j_end = j_begin + span;
  if (j_end > a.M) j_end = a.M;
}

__device__ __forceinline__ void load_owner(float (&u)[64], const float* base, int64_t row, int64_t ld, bool ok,
                                           int h) {
  if (ok) {
    const float4* src = reinterpret_cast<const float4*>(base + row * ld + h * 64);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float4 v = src[t];
      u[4 * t + 0] = v.x; u[4 * t + 1] = v.y; u[4 * t + 2] = v.z; u[4 * t + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 64; ++t) u[t] = 0.0f;
  }
}

__device__ __forceinline__ f32x16 tile_dots(const float* xrow, const float (&u)[64]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int s = 0; s < 64; s += 4) {
    const float4 bv = *reinterpret_cast<const float4*>(xrow + s);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, u[s + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, u[s + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.z, u[s + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.w, u[s + 3], acc, 0, 0, 0);
  }
  return acc;
}

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
  __shared__ __attribute__((aligned(16))) float sB[2][kTile][kLdsStride];
  __shared__ __attribute__((aligned(16))) float sBias[2][kTile];
  __shared__ __attribute__((aligned(16))) float sCnt[2][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  float u[64];
  load_owner(u, a.A, i, a.lda, row_ok, h);
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
  const int srow = tid >> 3, scol = (tid & 7) * 16;
  float4 stg[4];
  float stg_b = 0.0f, stg_c = 0.0f;
  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + srow;
    if (j < j_end) {
      const float4* src = reinterpret_cast<const float4*>(a.B + j * a.ldb + scol);
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = src[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_b = (ok && a.bias) ? a.bias[jj] : 0.0f;
      stg_c = ok ? a.colcnt[jj] : 0.0f;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<float4*>(&sB[buf][srow][scol + 4 * t]) = stg[t];
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
      const f32x16 acc = tile_dots(&sB[cur][c][h * 64], u);
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
  const float m2 = __shfl_xor(m, 32, 64);
  const float l2 = __shfl_xor(l, 32, 64);
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (mm != -INFINITY) {
    if (m != -INFINITY) ll += l * __expf(m - mm);
    if (m2 != -INFINITY) ll += l2 * __expf(m2 - mm);
  }
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)a.nsplit * a.N;
    const int64_t o = (int64_t)split * a.N + i;
    a.part[o] = mm;
    a.part[stride + o] = ll;
    a.part[2 * stride + o] = 0.0f;
    a.part[3 * stride + o] = 0.0f;
  }
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
  __shared__ __attribute__((aligned(16))) float sX[2][kTile][kLdsStride];
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
  float u[64];
  load_owner(u, own, o, ld_own, own_ok, h);
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

  const int srow = tid >> 3, scol = (tid & 7) * 16;
  float4 stg[4];
  float stg0 = 0.0f, stg1 = 0.0f;
  int stg2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + srow;
    if (sidx < s_end) {
      const float4* src = reinterpret_cast<const float4*>(str + sidx * ld_str + scol);
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = src[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) stg[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
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
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<float4*>(&sX[buf][srow][scol + 4 * t]) = stg[t];
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
      f32x16 acc = tile_dots(&sX[cur][c][h * 64], u);
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
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float* srow_p = &sX[cur][tile_row(t, h)][c];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          gacc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[t], srow_p[kb * 32], gacc[kb], 0, 0, 0);
      }
      __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  float* dst = a.dout + (int64_t)split * n_own * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r];
    }
  }
}


// =====================================================================================
// bf16x3 form of the grouped kernels (precision RSX_NCE_BF16X3).
// Every fp32 operand x is split x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (x - hi is exact
// in fp32), and a product is hi*hi' + hi*lo' + lo*hi' on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation (bf16 products are exact; the dropped lo*lo' and the rounding of lo leave
// ~2^-17 relative error per term: max |dot error| 2.7e-6 on unit vectors against 5e-7 for
// the fp32 MFMA and 1.2e-3 for plain bf16). Both products of the backward use it:
//   S tile  : streamed rows (A, ds_read_b128 row reads) x owner rows (B, registers)
//   gradient: G^T (A, straight from the S accumulator: its rows are the k index) x streamed
//             rows (B, ds_read_b64_tr_b16 transposed reads of the same LDS image)
// 3 x 32 cycles per 16 k per 32x32 tile instead of 8 x 64 for the fp32 MFMA (5.3x fewer
// MFMA cycles). The log-sum-exp runs in base 2 (v_exp_f32 without the log2e multiply).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
// s_waitcnt vmcnt(0) (expcnt, lgkmcnt left at their maxima): gfx9 encoding
constexpr int kVmcnt0 = 0x0F70;

// [32][128] bf16 image: 320-B rows plus a 16-B skew per 8-row group, i.e. byte offset
// 320*row + 16*(row>>3) + 2*col. Conflict-free for the row reads (ds_read_b128, lane (c,h)
// -> row c, chunk 8h+s), the transposed reads (ds_read_b64_tr_b16) and the staging stores
// (ds_write_b128), and every read address is a per-lane base + an immediate (no per-step
// address registers); checked with tools/lds_banks.py.
constexpr int kImgRow = 160;  // bf16 elements per image row
constexpr int kImgElems = 5120;
__device__ __forceinline__ int img_off(int row, int col) { return row * kImgRow + 8 * (row >> 3) + col; }

struct X3Tile {
  __bf16 hi[kImgElems];
  __bf16 lo[kImgElems];
};

__device__ __forceinline__ void split8(const float4& a, const float4& b, bf16x8& h, bf16x8& l) {
  const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const __bf16 hk = (__bf16)f[k];
    h[k] = hk;
    l[k] = (__bf16)(f[k] - (float)hk);
  }
}

// owner row (dims 64h .. 64h+63 on lane half h) -> hi/lo fragments of k-steps s = 0..7
// (fragment s, element j = dim 64h + 8s + j: the chunk 8h + s of the streamed row reads)
__device__ __forceinline__ void load_owner_x3(bf16x8 (&uh)[8], bf16x8 (&ul)[8], const float* base, int64_t row,
                                              int64_t ld, bool ok, int h) {
  // all 16 loads issued back to back from a clamped row, then zeroed past the rows (a branch
  // around each pair made hipcc wait for every pair before issuing the next)
  const float4* src = reinterpret_cast<const float4*>(base + (ok ? row : 0) * ld + h * 64);
  float4 v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) v[t] = src[t];
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int s = 0; s < 8; ++s) split8(ok ? v[2 * s] : z, ok ? v[2 * s + 1] : z, uh[s], ul[s]);
}

// Streamed operands are split once per call into global hi/lo bf16 images ([rows][128] each,
// nce_split_k), so staging a tile is a plain copy: thread tid moves row tid>>3, 16-B chunks
// tid&7 and 8+(tid&7) of both images (4 x 16-B loads, 4 ds_write_b128).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct X3Stage {
  u32x4 v[4];  // hi chunk0, hi chunk1, lo chunk0, lo chunk1
  __device__ __forceinline__ void load(const __bf16* hi, const __bf16* lo, int64_t row, bool ok, int tid) {
    if (ok) {
      const int64_t o = row * kD + (tid & 7) * 8;
      v[0] = *reinterpret_cast<const u32x4*>(hi + o);
      v[1] = *reinterpret_cast<const u32x4*>(hi + o + 64);
      v[2] = *reinterpret_cast<const u32x4*>(lo + o);
      v[3] = *reinterpret_cast<const u32x4*>(lo + o + 64);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void store(X3Tile& t, int tid) const {
    const int row = tid >> 3, ch = tid & 7;
    const int o0 = img_off(row, 8 * ch), o1 = img_off(row, 64 + 8 * ch);
    *reinterpret_cast<u32x4*>(&t.hi[o0]) = v[0];
    *reinterpret_cast<u32x4*>(&t.hi[o1]) = v[1];
    *reinterpret_cast<u32x4*>(&t.lo[o0]) = v[2];
    *reinterpret_cast<u32x4*>(&t.lo[o1]) = v[3];
  }
  // the hi image alone (a pass whose products never read the streamed rows' lo image)
  __device__ __forceinline__ void load_hi(const __bf16* hi, int64_t row, bool ok, int tid) {
    if (ok) {
      const int64_t o = row * kD + (tid & 7) * 8;
      v[0] = *reinterpret_cast<const u32x4*>(hi + o);
      v[1] = *reinterpret_cast<const u32x4*>(hi + o + 64);
    } else {
      v[0] = v[1] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void store_hi(X3Tile& t, int tid) const {
    const int row = tid >> 3, ch = tid & 7;
    *reinterpret_cast<u32x4*>(&t.hi[img_off(row, 8 * ch)]) = v[0];
    *reinterpret_cast<u32x4*>(&t.hi[img_off(row, 64 + 8 * ch)]) = v[1];
  }
};

// rows x 128 fp32 (row stride ld) -> hi/lo bf16 images [rows][128]; one thread per 8 floats
__global__ __launch_bounds__(256) void nce_split_k(const float* src, int64_t ld, int64_t rows, __bf16* hi,
                                                   __bf16* lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 8-float chunk index
  if (i >= rows * (kD / 8)) return;
  const int64_t r = i / (kD / 8), c8 = i % (kD / 8);
  const float4* p = reinterpret_cast<const float4*>(src + r * ld + c8 * 8);
  bf16x8 h, l;
  split8(p[0], p[1], h, l);
  *reinterpret_cast<bf16x8*>(hi + r * kD + c8 * 8) = h;
  *reinterpret_cast<bf16x8*>(lo + r * kD + c8 * 8) = l;
}

// S tile: acc[r] = <streamed row tile_row(r,h), owner row c> (owner on the lane).
// The next k-step's fragments are read before this step's MFMAs (LDS latency under MFMA);
// the scheduling barrier keeps the compiler from hoisting more reads (VGPR budget).
__device__ __forceinline__ f32x16 dots_x3(const X3Tile& t, int c, int h, const bf16x8 (&uh)[8],
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
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, uh[s], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ul[s], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, uh[s], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    ah = nh;
    al = nl;
  }
  return acc;
}

// gacc[nb] += G^T X over the tile, G given as its hi/lo bf16 fragments (acc layout: streamed
// row tile_row(r,h) in register r, owner on the lane; k-step ks takes registers 8ks..8ks+7,
// i.e. streamed rows 16ks + 8(j>>2) + 4h + (j&3)). The B fragment is those rows of dims
// 32nb + c, two transposed 4-row reads per image. Steps (ks, nb) are software-pipelined by one.
__device__ __forceinline__ void grad_x3s(f32x16 (&gacc)[4], const bf16x8 (&gh)[2], const bf16x8 (&gl)[2],
                                         const X3Tile& t, int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3, h = lane >> 5, cb = (lane >> 4) & 1;
  const int base = img_off(4 * h + q, 16 * cb + 4 * p);  // + img_off(16ks + 8half, 32nb) - img_off(0,0)
  auto rd = [&](const __bf16* img, int step, bf16x8& out) {
    const int ks = step >> 2, nb = step & 3;
    const int o0 = base + img_off(16 * ks, 32 * nb), o1 = base + img_off(16 * ks + 8, 32 * nb);
    const bf16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o0]));
    const bf16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o1]));
    out = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  bf16x8 bh, bl;
  rd(t.hi, 0, bh);
  rd(t.lo, 0, bl);
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    bf16x8 nh = bh, nl = bl;
    if (step < 7) {
      rd(t.hi, step + 1, nh);
      rd(t.lo, step + 1, nl);
    }
    const int ks = step >> 2, nb = step & 3;
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[ks], bh, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[ks], bl, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[ks], bh, gacc[nb], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

// (a, b) -> packed bf16 hi pair and lo pair (x = hi + lo, hi = RNE bf16(x), lo = bf16(x - hi)):
// one pair conversion for hi, its two halves unpacked as fp32 by a shift and a mask, two
// subtractions and one pair conversion for lo (the per-element form converted every element
// twice and re-packed).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  const bf16x2 h = {(__bf16)a, (__bf16)b};
  hi = __builtin_bit_cast(uint32_t, h);
  const float ha = __uint_as_float(hi << 16), hb = __uint_as_float(hi & 0xffff0000u);
  const bf16x2 l = {(__bf16)(a - ha), (__bf16)(b - hb)};
  lo = __builtin_bit_cast(uint32_t, l);
}

__device__ __forceinline__ void split_tile(const f32x16& g, bf16x8 (&gh)[2], bf16x8 (&gl)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4 h, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t hq, lq;
      split_pair(g[8 * ks + 2 * q], g[8 * ks + 2 * q + 1], hq, lq);
      h[q] = hq;
      l[q] = lq;
    }
    gh[ks] = __builtin_bit_cast(bf16x8, h);
    gl[ks] = __builtin_bit_cast(bf16x8, l);
  }
}

// g = 2^(x - m) per element of the tile, summed into ls and split to hi/lo fragments, two elements
// per step on packed fp32 ops: one v_pk_add for the exponent arguments, one for the running sum,
// and a truncation split (hi = top 16 bits: one v_perm packs the pair, two masks give hi as fp32,
// one v_pk_add the exact residuals x - hi, one pair conversion rounds them to bf16). Truncation
// leaves |lo| < 2^-7 |x| and an error below 2^-16 |x| after rounding lo (RNE hi: 2^-17), well
// inside the bf16x3 product's own 2^-16 (the dropped lo*lo' term).
typedef float f32x2 __attribute__((ext_vector_type(2)));
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
__device__ __forceinline__ int grad_lane_base(int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3, h = lane >> 5, cb = (lane >> 4) & 1;
  return img_off(4 * h + q, 16 * cb + 4 * p);
}

__device__ __forceinline__ void grad_rd(const __bf16* img, int base, int ks, int nb, bf16x8& out) {
  const int o0 = base + img_off(16 * ks, 32 * nb), o1 = base + img_off(16 * ks + 8, 32 * nb);
  const bf16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o0]));
  const bf16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o1]));
  out = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <bool WORK>
__device__ __forceinline__ void grad_half_x3(f32x16 (&gacc)[4], const bf16x8& gh, const bf16x8& gl, const X3Tile& t,
                                             int base, int ks, const f32x16& x, int xh, float m, uint32_t (&oh)[4],
                                             uint32_t (&ol)[4], f32x2& sum) {
  bf16x8 bh, bl;
  grad_rd(t.hi, base, ks, 0, bh);
  grad_rd(t.lo, base, ks, 0, bl);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      grad_rd(t.hi, base, ks, nb + 1, nh);
      grad_rd(t.lo, base, ks, nb + 1, nl);
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
typedef float f32x4 __attribute__((ext_vector_type(4)));
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
  grad_rd(t.hi, base, ks, 0, bh);
  grad_rd(t.lo, base, ks, 0, bl);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      grad_rd(t.hi, base, ks, nb + 1, nh);
      grad_rd(t.lo, base, ks, nb + 1, nl);
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
        const int gbase = grad_lane_base(lane);
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
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  float* dst = a.dout + (int64_t)split * n_own * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r];
    }
  }
}

// ---- plain (ungrouped) InfoNCE in bf16x3: DuoRec unsup/sup, SimCSE -------------------
// The objective, flags and partial layout of nce_fwd_k / nce_bwd_k; the products as in the
// grouped bf16x3 kernels (streamed hi/lo images copied from ws into LDS, owner fragments in
// registers, S tile on dots_x3, gradient tile split and fed to grad_x3s), one barrier per tile.
struct X3Args {
  const __bf16* shi;  // streamed operand's hi/lo images [rows][128]
  const __bf16* slo;
};

template <int FL>
__global__ __launch_bounds__(256, 2) void nce_fwd_x3_k(FwdArgs a, X3Args x) {
  __shared__ __attribute__((aligned(16))) X3Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sBias[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK1[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK2[2][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;
  bf16x8 uh[8], ul[8];
  load_owner_x3(uh, ul, a.A, i, a.lda, row_ok, h);
  int k1i = 0, k2i = 0;
  if (row_ok) {
    if ((FL & (F_MASK_K1 | F_POS)) && a.k1a) k1i = a.k1a[i];
    if ((FL & F_MASK_K2) && a.k2a) k2i = a.k2a[i];
  }
  const int64_t j_begin = (int64_t)split * a.cols_per_split;
  int64_t j_end = j_begin + a.cols_per_split;
  if (j_end > a.M) j_end = a.M;
  float m = -INFINITY, l = 0.0f, ps = 0.0f, pc = 0.0f;
  X3Stage stg;
  float stg_bias = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;
  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + (tid >> 3);
    stg.load(x.shi, x.slo, j, j < j_end, tid);
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_bias = (ok && a.bias) ? a.bias[jj] : 0.0f;
      stg_k1 = (ok && a.k1b) ? a.k1b[jj] : 0;
      stg_k2 = (ok && a.k2b) ? a.k2b[jj] : 0;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sBias[buf][tid] = stg_bias;
      sK1[buf][tid] = stg_k1;
      sK2[buf][tid] = stg_k2;
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
      float v[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int rbase = 8 * q4 + 4 * h;
        const float4 bi4 = *reinterpret_cast<const float4*>(&sBias[cur][rbase]);
        const int4 k14 = *reinterpret_cast<const int4*>(&sK1[cur][rbase]);
        const int4 k24 = *reinterpret_cast<const int4*>(&sK2[cur][rbase]);
        const float bia[4] = {bi4.x, bi4.y, bi4.z, bi4.w};
        const int kk1[4] = {k14.x, k14.y, k14.z, k14.w};
        const int kk2[4] = {k24.x, k24.y, k24.z, k24.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          const int64_t j = j0 + rbase + e;
          const float sv = acc[r] * a.inv_tau - bia[e];
          bool excl = (j >= j_end) || !row_ok;
          const bool offdiag = (j != i + a.diag_off);
          if (FL & F_EXCL_DIAG) excl = excl || !offdiag;
          if (FL & F_MASK_K1) excl = excl || (offdiag && kk1[e] == k1i);
          if (FL & F_MASK_K2) excl = excl || (offdiag && kk2[e] == k2i);
          if (FL & F_POS) {
            if (!excl && offdiag && kk1[e] == k1i && k1i != 0) {
              ps += sv;
              pc += 1.0f;
            }
          }
          v[r] = excl ? -INFINITY : sv;
          tmax = fmaxf(tmax, v[r]);
        }
      }
      if (tmax > m) {
        l = (m == -INFINITY) ? 0.0f : l * __expf(m - tmax);
        m = tmax;
      }
      if (m != -INFINITY) {
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += __expf(v[r] - m);
        l += t;
      }
      if (has_next) lstore(cur ^ 1);  // cur^1: read in the previous tile, fenced by its barrier
      __syncthreads();
      cur ^= 1;
    }
  }
  const float m2 = __shfl_xor(m, 32, 64);
  const float l2 = __shfl_xor(l, 32, 64);
  const float ps2 = __shfl_xor(ps, 32, 64);
  const float pc2 = __shfl_xor(pc, 32, 64);
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (mm != -INFINITY) {
    if (m != -INFINITY) ll += l * __expf(m - mm);
    if (m2 != -INFINITY) ll += l2 * __expf(m2 - mm);
  }
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)a.nsplit * a.N;
    const int64_t o = (int64_t)split * a.N + i;
    a.part[o] = mm;
    a.part[stride + o] = ll;
    a.part[2 * stride + o] = ps + ps2;
    a.part[3 * stride + o] = pc + pc2;
  }
}

template <int FL, bool ROW_OWNED>
__global__ __launch_bounds__(256, 2) void nce_bwd_x3_k(BwdArgs a, X3Args x) {
  __shared__ __attribute__((aligned(16))) X3Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sM0[2][kTile];  // row side: lse_i | col side: bias_j
  __shared__ __attribute__((aligned(16))) float sM1[2][kTile];  // row side: w_i
  __shared__ __attribute__((aligned(16))) float sM2[2][kTile];  // row side: inv_cnt_i
  __shared__ __attribute__((aligned(16))) int sK1[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK2[2][kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, ob;
  remap_block(a.nsplit, split, ob);
  const int64_t n_own = ROW_OWNED ? a.N : a.M;
  const int64_t n_str = ROW_OWNED ? a.M : a.N;
  const float* own = ROW_OWNED ? a.A : a.B;
  const int64_t ld_own = ROW_OWNED ? a.lda : a.ldb;
  const float g_scale = a.gout[0] * a.inv_tau;
  const int64_t o = (int64_t)ob * kOwnRows + wave * 32 + c;
  const bool own_ok = o < n_own;
  bf16x8 uh[8], ul[8];
  load_owner_x3(uh, ul, own, o, ld_own, own_ok, h);
  float o_lse = 0.0f, o_w = 0.0f, o_icnt = 0.0f, o_bias = 0.0f;
  int o_k1 = 0, o_k2 = 0;
  if (own_ok) {
    if (ROW_OWNED) {
      o_lse = a.lse[o];
      o_w = a.row_valid[o] * g_scale;
      if ((FL & F_POS) && a.inv_cnt) o_icnt = a.inv_cnt[o];
      if ((FL & (F_MASK_K1 | F_POS)) && a.k1a) o_k1 = a.k1a[o];
      if ((FL & F_MASK_K2) && a.k2a) o_k2 = a.k2a[o];
    } else {
      o_bias = a.bias ? a.bias[o] : 0.0f;
      if ((FL & (F_MASK_K1 | F_POS)) && a.k1b) o_k1 = a.k1b[o];
      if ((FL & F_MASK_K2) && a.k2b) o_k2 = a.k2b[o];
    }
  }
  const int64_t s_begin = (int64_t)split * a.span_per_split;
  int64_t s_end = s_begin + a.span_per_split;
  if (s_end > n_str) s_end = n_str;
  f32x16 gacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[kb][r] = 0.0f;
  X3Stage stg;
  float stg0 = 0.0f, stg1 = 0.0f, stg2 = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;
  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load(x.shi, x.slo, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      if (ROW_OWNED) {
        stg0 = (ok && a.bias) ? a.bias[ss] : 0.0f;
        stg_k1 = (ok && a.k1b) ? a.k1b[ss] : 0;
        stg_k2 = (ok && a.k2b) ? a.k2b[ss] : 0;
      } else {
        stg0 = ok ? a.lse[ss] : 0.0f;
        stg1 = ok ? a.row_valid[ss] * g_scale : 0.0f;
        stg2 = (ok && a.inv_cnt) ? a.inv_cnt[ss] : 0.0f;
        stg_k1 = (ok && a.k1a) ? a.k1a[ss] : 0;
        stg_k2 = (ok && a.k2a) ? a.k2a[ss] : 0;
      }
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sM0[buf][tid] = stg0;
      sM1[buf][tid] = stg1;
      sM2[buf][tid] = stg2;
      sK1[buf][tid] = stg_k1;
      sK2[buf][tid] = stg_k2;
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
      f32x16 acc = dots_x3(sT[cur], c, h, uh, ul);
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int rbase = 8 * q4 + 4 * h;
        const float4 m04 = *reinterpret_cast<const float4*>(&sM0[cur][rbase]);
        const float4 m14 = *reinterpret_cast<const float4*>(&sM1[cur][rbase]);
        const float4 m24 = *reinterpret_cast<const float4*>(&sM2[cur][rbase]);
        const int4 k14 = *reinterpret_cast<const int4*>(&sK1[cur][rbase]);
        const int4 k24 = *reinterpret_cast<const int4*>(&sK2[cur][rbase]);
        const float mm0[4] = {m04.x, m04.y, m04.z, m04.w};
        const float mm1[4] = {m14.x, m14.y, m14.z, m14.w};
        const float mm2[4] = {m24.x, m24.y, m24.z, m24.w};
        const int kk1[4] = {k14.x, k14.y, k14.z, k14.w};
        const int kk2[4] = {k24.x, k24.y, k24.z, k24.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          const int64_t sidx = s0 + rbase + e;
          int64_t ii, jj;
          float lse_i, w_i, icnt_i, bias_j;
          int k1_i, k1_j, k2_i, k2_j;
          if (ROW_OWNED) {
            ii = o; jj = sidx;
            lse_i = o_lse; w_i = o_w; icnt_i = o_icnt; bias_j = mm0[e];
            k1_i = o_k1; k1_j = kk1[e]; k2_i = o_k2; k2_j = kk2[e];
          } else {
            ii = sidx; jj = o;
            lse_i = mm0[e]; w_i = mm1[e]; icnt_i = mm2[e]; bias_j = o_bias;
            k1_i = kk1[e]; k1_j = o_k1; k2_i = kk2[e]; k2_j = o_k2;
          }
          const float sv = acc[r] * a.inv_tau - bias_j;
          bool excl = (sidx >= s_end) || !own_ok;
          const bool offdiag = (jj != ii + a.diag_off);
          if (FL & F_EXCL_DIAG) excl = excl || !offdiag;
          if (FL & F_MASK_K1) excl = excl || (offdiag && k1_i == k1_j);
          if (FL & F_MASK_K2) excl = excl || (offdiag && k2_i == k2_j);
          float y = 0.0f;
          if (FL & F_POS) {
            if (!excl && offdiag && k1_i == k1_j && k1_i != 0) y = icnt_i;
          } else {
            y = offdiag ? 0.0f : 1.0f;
          }
          const float p = (excl || lse_i == -INFINITY) ? 0.0f : __expf(sv - lse_i);
          acc[r] = excl ? 0.0f : w_i * (p - y);
        }
      }
      bf16x8 gh[2], gl[2];
      split_tile(acc, gh, gl);
      grad_x3s(gacc, gh, gl, sT[cur], lane);
      if (has_next) lstore(cur ^ 1);  // cur^1: read in the previous tile, fenced by its barrier
      __syncthreads();
      cur ^= 1;
    }
  }
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  float* dst = a.dout + (int64_t)split * n_own * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r];
    }
  }
}

// Forward of the grouped loss fused with the row-side gradient (bf16x3). The row gradient
//   dA_i = gout/tau * (sum_j p_ij B_j - B_d(i)),  p_ij = w_ij 2^(x_ij) / sum_j w_ij 2^(x_ij)
// is a softmax-weighted sum of the streamed rows, i.e. an attention output with V = B: it is
// accumulated during the forward sweep, unnormalised, against a lazily raised running max
// (rescaled only when a tile max exceeds it by more than 2^8, so almost never after the first
// tiles), and normalised in the merge. This replaces the forward plus the backward's row pass
// (two sweeps of S) with one sweep; the backward keeps only the column pass.
// Per split: part = (m ln2, l) per row as the plain forward, dpart[split][row][128] = O.
constexpr float kLazyLog2 = 8.0f;
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
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_b = ok ? (a.bias ? a.bias[jj] : 0.0f) : INFINITY;
      stg_c = ok ? a.colcnt[jj] : 0.0f;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      // -bias log2e + log2 c_d: the multiplicity rides in the exponent (one fma per logit, no
      // multiply); -inf past the split (c = 0, bias = inf)
      sB2[buf][tid] = -(stg_b * kLog2e) + __log2f(stg_c);
      sCnt[buf][tid] = stg_c;
    }
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
    const int gbase = grad_lane_base(lane);
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
  const int64_t own_base = rb * kRows + wave * 32;
  float* dst = a.dout + (int64_t)split * a.N * kD;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < a.N) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r];
    }
  }
}

// =====================================================================================
// fp16 form of the fused forward and the column pass (precision RSX_NCE_F16).
// Logits: every operand is split into fp16 hi + lo of x * 2^8 (unit-vector components scaled into
// fp16's normal range; lo carries the next 11 bits), S = hi*hi' + hi*lo' + lo*hi' on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation: |dot error| ~2^-22 relative per term, tighter
// than bf16x3 (2^-16) at the same MFMA count; the 2^16 product scale is folded into 1/tau.
// Gradient products (the softmax weights G against the streamed rows): G rounded to fp16 once and
// multiplied by the rows' fp16 hi image (GP = 1: one MFMA per k-step instead of three) or by hi and
// lo (GP = 2: only G's rounding, 2^-11 relative per weight). This is the reference's own GPU
// arithmetic for these products (autocast(float16), v1_usertower_train.py:787) with fp32
// accumulation; the gradient scales (the 2^8 row scale, the column pass's per-owner factor and
// its 2^14 weight scale) are applied to the fp32 accumulators after the sweep.
// The images keep the bf16x3 layout and LDS tiles (16-bit containers: bf16x8 vectors carry fp16
// bits and are bit-cast at the MFMA).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
constexpr float kHScale = 256.0f;         // operand scale 2^8
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

__device__ __forceinline__ void split8_h(const float4& a, const float4& b, bf16x8& h, bf16x8& l) {
  const float f[8] = {a.x * kHScale, a.y * kHScale, a.z * kHScale, a.w * kHScale,
                      b.x * kHScale, b.y * kHScale, b.z * kHScale, b.w * kHScale};
  f16x8 hv, lv;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const _Float16 hk = (_Float16)f[k];
    hv[k] = hk;
    lv[k] = (_Float16)(f[k] - (float)hk);
  }
  h = __builtin_bit_cast(bf16x8, hv);
  l = __builtin_bit_cast(bf16x8, lv);
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

// rows x 128 fp32 -> fp16 hi/lo images of x * 2^8 (nce_split_k's layout)
__global__ __launch_bounds__(256) void nce_split_h_k(const float* src, int64_t ld, int64_t rows, __bf16* hi,
                                                     __bf16* lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * (kD / 8)) return;
  const int64_t r = i / (kD / 8), c8 = i % (kD / 8);
  const float4* p = reinterpret_cast<const float4*>(src + r * ld + c8 * 8);
  bf16x8 h, l;
  split8_h(p[0], p[1], h, l);
  *reinterpret_cast<bf16x8*>(hi + r * kD + c8 * 8) = h;
  *reinterpret_cast<bf16x8*>(lo + r * kD + c8 * 8) = l;
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

// S tile from two fp16 products, hi*hi' + hi*lo' (streamed hi against the owner's hi and lo): the
// streamed rows' lo image is never read. |dot error| = |<lo, owner>| ~ 2^-11 |x| per component with
// random signs, ~2e-5 on unit vectors (the column pass's weights only; the logits of the loss keep
// three products in the forward)
__device__ __forceinline__ f32x16 dots_h2(const X3Tile& t, int c, int h, const bf16x8 (&uh)[8],
                                          const bf16x8 (&ul)[8]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int base = img_off(c, 64 * h);
  bf16x8 ah = *reinterpret_cast<const bf16x8*>(&t.hi[base]);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    bf16x8 nh = ah;
    if (s < 7) nh = *reinterpret_cast<const bf16x8*>(&t.hi[base + 8 * (s + 1)]);
    acc = mfma_h(ah, ul[s], acc);
    acc = mfma_h(ah, uh[s], acc);
    __builtin_amdgcn_sched_barrier(0);
    ah = nh;
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
  grad_rd(t.hi, base, ks, 0, bh);
  if (GP == 2) grad_rd(t.lo, base, ks, 0, bl);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      grad_rd(t.hi, base, ks, nb + 1, nh);
      if (GP == 2) grad_rd(t.lo, base, ks, nb + 1, nl);
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
    if (tid < kTile) {
      const int64_t jj = j0 + tid;
      const bool ok = jj < j_end;
      stg_b = ok ? (a.bias ? a.bias[jj] : 0.0f) : INFINITY;
      stg_c = ok ? a.colcnt[jj] : 0.0f;
    }
  };
  auto lstore = [&](int buf) {
    stg.store(sT[buf], tid);
    if (tid < kTile) {
      sB2[buf][tid] = -(stg_b * kLog2e) + __log2f(stg_c);
      sCnt[buf][tid] = stg_c;
    }
  };
  if (j_begin < j_end) {
    gload(j_begin);
    lstore(0);
    __syncthreads();
    int cur = 0, prev = 0;
    bf16x8 pg;
#pragma unroll
    for (int k = 0; k < 8; ++k) pg[k] = (__bf16)0.0f;  // zero bits = fp16 zero
    const int gbase = grad_lane_base(lane);
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
  grad_rd(t.hi, base, ks, 0, bh);
  if (GP == 2) grad_rd(t.lo, base, ks, 0, bl);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    bf16x8 nh = bh, nl = bl;
    if (nb < 3) {
      grad_rd(t.hi, base, ks, nb + 1, nh);
      if (GP == 2) grad_rd(t.lo, base, ks, nb + 1, nl);
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
// SPN = products of the S tile: 3 (dots_h3) or 2 (dots_h2, GP = 1 only: with one gradient product on the
// hi image as well, the streamed rows' lo image is neither staged nor read). GP = 1 runs with two: the
// column weights' logits to ~2e-5 on unit vectors (the pass outputs gradients only, 1e-3 of scale); at
// batch 8192 the pass takes 3.33 instead of 4.03 ms with grad_b's deviation from fp32 unchanged
// (4.897e-4 vs 4.899e-4 of scale, tools/nce_micro.py --compare).
template <int GP, int SPN = 3>
__global__ __launch_bounds__(256, 2) void nce_grouped_bwd_cols_h_k(GArgs a) {
  static_assert(SPN == 3 || (SPN == 2 && GP == 1), "two S products only with one gradient product");
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
    if constexpr (SPN == 2) stg.load_hi(a.ahi, sidx, sidx < s_end, tid);
    else stg.load(a.ahi, a.alo, sidx, sidx < s_end, tid);
    if (tid < kTile) {
      const int64_t ss = s0 + tid;
      const bool ok = ss < s_end;
      stg0 = ok ? a.lse[ss] : INFINITY;
      stg2 = ok ? a.row_col[ss] : -2;
    }
  };
  auto lstore = [&](int buf) {
    if constexpr (SPN == 2) stg.store_hi(sT[buf], tid);
    else stg.store(sT[buf], tid);
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
    const int gbase = grad_lane_base(lane);
    for (int t = 0; t < ntile; ++t) {
      const int64_t s0 = s_begin + (int64_t)t * kTile;
      const bool has_next = t + 1 < ntile;
      const bool exc = exc_flag(s0);
      if (has_next) gload(s0 + kTile);
      f32x16 acc = SPN == 2 ? dots_h2(sT[cur], c, h, uh, ul) : dots_h3(sT[cur], c, h, uh, ul);
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
  const int64_t own_base = (int64_t)ob * kOwnRows + wave * 32;
  float* dst = a.dout + (int64_t)split * n_own * kD;
  const float f = gs * (kHUnscale / kHGSv);  // gout / tau, the 2^-8 row scale and the 2^-14 weight scale
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = gacc[kb][r] * f;
    }
  }
}

// merge of the fused forward: lse / row loss as nce_grouped_merge_k, plus the row gradient
// per unit upstream gradient  ga_i = (sum_s O_s e^(m_s - M) / sum_s l_s e^(m_s - M) - B_d(i)) / tau
__global__ __launch_bounds__(256) void nce_grouped_merge_g_k(const float* A, const float* B, const float* bias,
                                                             const int* row_col, int64_t N, int64_t lda,
                                                             int64_t ldb, float inv_tau, int nsplit,
                                                             const float* part, const float* opart,
                                                             float* lse_out, float* row_loss, float* row_valid,
                                                             float* ga, int64_t rows1, int nsplit2, int nslots,
                                                             int lab_out) {
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
  const int d = row_col[i];
  const float2 x = reinterpret_cast<const float2*>(A + i * lda)[lane];
  const float2 y = reinterpret_cast<const float2*>(B + (int64_t)d * ldb)[lane];
  float dd = x.x * y.x + x.y * y.y;
  for (int o = 32; o > 0; o >>= 1) dd += __shfl_xor(dd, o, 64);
  const float sii = dd * inv_tau - (bias ? bias[d] : 0.0f);
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
  const float cy = lab_out ? ((lse == -INFINITY) ? -1.0f : __expf(sii - lse) - 1.0f) : -1.0f;
  reinterpret_cast<float2*>(ga + i * kD)[lane] = make_float2(fmaf(cy, y.x, acc.x) * inv_tau, fmaf(cy, y.y, acc.y) * inv_tau);
  if (lane == 0) {
    lse_out[i] = lse;
    row_loss[i] = lse - sii;
    row_valid[i] = 1.0f;
  }
}

}  // namespace

RSX_API int64_t rsx_nce_workspace_floats(int64_t N, int64_t M, int nsplit_fwd, int nsplit_bwd) {
  const int64_t mx = N > M ? N : M;
  return 4 * (int64_t)nsplit_fwd * N      // fwd partials
         + 4 * N                          // lse, row_loss, row_valid, inv_cnt
         + (int64_t)nsplit_bwd * mx * kD  // bwd split partials
         + 16;
}

// Grouped kernels: the plain layout, then (bf16x3) the hi/lo images of A [N][128] and B [D][128].
RSX_API int64_t rsx_nce_grouped_workspace_floats(int64_t N, int64_t D, int nsplit_fwd, int nsplit_bwd,
                                                 int precision) {
  const int64_t base = (rsx_nce_workspace_floats(N, D, nsplit_fwd, nsplit_bwd) + 63) / 64 * 64;
  return base + (precision != RSX_NCE_FP32 ? (N + D) * kD + 64 : 0);
}

namespace {
struct Images {
  __bf16 *ahi, *alo, *bhi, *blo;
};
Images grouped_images(float* ws, int64_t N, int64_t D, int nsplit_fwd, int nsplit_bwd) {
  const int64_t base = (rsx_nce_workspace_floats(N, D, nsplit_fwd, nsplit_bwd) + 63) / 64 * 64;
  __bf16* p = reinterpret_cast<__bf16*>(ws + base);
  Images im;
  im.ahi = p;
  im.alo = p + N * kD;
  im.bhi = p + 2 * N * kD;
  im.blo = p + 2 * N * kD + D * kD;
  return im;
}
void launch_split(const float* src, int64_t ld, int64_t rows, __bf16* hi, __bf16* lo, hipStream_t st) {
  const int64_t n = rows * (kD / 8);
  if (n > 0) hipLaunchKernelGGL(nce_split_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, ld, rows, hi, lo);
}
// the fp16 images of RSX_NCE_F16 (x * 2^8, hi + lo)
void launch_split_h(const float* src, int64_t ld, int64_t rows, __bf16* hi, __bf16* lo, hipStream_t st) {
  const int64_t n = rows * (kD / 8);
  if (n > 0)
    hipLaunchKernelGGL(nce_split_h_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, ld, rows, hi, lo);
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

// Forward: writes lse/row_loss/row_valid/inv_cnt (ws) and out2 = {sum of row losses, n_valid}.
RSX_API int rsx_nce_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                        const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                        int64_t diag_offset, float tau, int flags, int nsplit, float* ws, float* out2,
                        void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(nsplit >= 8 && nsplit <= 64 && nsplit % 8 == 0, "nsplit must be a multiple of 8 in [8,64]");
  RSX_ARG(N >= 0 && M >= 0, "negative size");
  RSX_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= kD && ldb >= kD, "row strides must be >=128 and multiples of 4");
  RSX_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "A/B must be 16-byte aligned");
  RSX_ARG(diag_offset >= 0 && diag_offset + N <= M, "need 0 <= diag_offset and diag_offset + N <= M");
  RSX_ARG(!(flags & (F_MASK_K1 | F_POS)) || (k1a && k1b), "k1 keys required");
  RSX_ARG(!(flags & F_MASK_K2) || (k2a && k2b), "k2 keys required");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    (void)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
    RSX_LAUNCHED();
    return 0;
  }
  const FwdArgs fa = plain_fwd_args(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, nsplit, ws);
  const int blocks = (int)(((N + kOwnRows - 1) / kOwnRows) * nsplit);
  with_flags(flags, [&](auto fl) { launch_fwd_t<decltype(fl)::value>(fa, blocks, st); });
  RSX_LAUNCHED();
  return plain_fwd_finish(fa, flags, out2, st);
}

// Backward: dA (N x 128) and/or dB (M x 128); accumulate != 0 adds into them.
RSX_API int rsx_nce_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                        const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                        int64_t diag_offset, float tau, int flags, int nsplit_fwd, int nsplit, const float* gout,
                        float* ws, float* dA, float* dB, int accumulate, void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(nsplit >= 8 && nsplit <= 64 && nsplit % 8 == 0, "nsplit must be a multiple of 8 in [8,64]");
  RSX_ARG(gout != nullptr, "gout required");
  RSX_ARG(diag_offset >= 0 && diag_offset + N <= M, "need 0 <= diag_offset and diag_offset + N <= M");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return 0;
  float* part = ws;
  float* lse = part + 4 * (int64_t)nsplit_fwd * N;
  float* row_valid = lse + 2 * N;
  float* inv_cnt = row_valid + N;
  float* dpart = inv_cnt + N;
  BwdArgs ba;
  ba.A = A; ba.B = B; ba.bias = bias;
  ba.k1a = k1a; ba.k1b = k1b; ba.k2a = k2a; ba.k2b = k2b;
  ba.N = N; ba.M = M; ba.lda = lda; ba.ldb = ldb;
  ba.diag_off = diag_offset;
  ba.inv_tau = 1.0f / tau;
  ba.lse = lse; ba.row_valid = row_valid; ba.inv_cnt = inv_cnt;
  ba.gout = gout;
  ba.nsplit = nsplit;
  for (int pass = 0; pass < 2; ++pass) {
    const bool row_owned = pass == 0;
    float* target = row_owned ? dA : dB;
    if (!target) continue;
    const int64_t n_own = row_owned ? N : M;
    const int64_t n_str = row_owned ? M : N;
    if (n_own == 0) continue;
    ba.span_per_split = round_up((n_str + nsplit - 1) / nsplit, kTile);
    if (ba.span_per_split < kTile) ba.span_per_split = kTile;
    ba.dout = dpart;
    const int blocks = (int)(((n_own + kOwnRows - 1) / kOwnRows) * nsplit);
    with_flags(flags, [&](auto fl) { launch_bwd_t<decltype(fl)::value>(ba, row_owned, blocks, st); });
    RSX_LAUNCHED();
    const int64_t total4 = n_own * kD / 4;
    hipLaunchKernelGGL(nce_sum_splits_k, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dpart, nsplit,
                       n_own, target, accumulate);
    RSX_LAUNCHED();
  }
  return 0;
}


// ---- plain InfoNCE, bf16x3 ------------------------------------------------------------
namespace {
// split count of one pass: the smallest power of two (<= 64) that gives the owner side >= 1024
// workgroups while every split keeps >= 2 streamed tiles
int plain_split(int64_t n_own, int64_t n_str) {
  const int64_t ob = (n_own + kOwnRows - 1) / kOwnRows;
  // workgroup target: one round of two workgroups per CU (512 on MI355X) measured 8 % faster than
  // 1024 over the DuoRec + SupCon passes at B = 8192 (tools/nce_plain_micro.py: 0.763 vs 0.830 ms;
  // 256: 1.05, 2048: 0.93).
  const int64_t target = 2 * rsx::cu_count();
  int ps = 1;
  while (ps < 64 && ob * ps < target && n_str >= (int64_t)ps * 4 * kTile) ps *= 2;
  return ps;
}
struct X3Plan {
  int nf, pr, pc;            // forward / row-pass / column-pass splits
  int64_t img, dpart, total;  // float offsets of the images and the split partials; total size
};
X3Plan plain_plan(int64_t N, int64_t M) {
  X3Plan p;
  p.nf = plain_split(N, M);
  p.pr = plain_split(N, M);
  p.pc = plain_split(M, N);
  p.img = (4 * (int64_t)p.nf * N + 4 * N + 63) / 64 * 64;  // after part [4][nf][N] and lse/loss/valid/icnt
  p.dpart = p.img + (N + M) * kD;                          // hi+lo bf16 of A and B = 1 float per element
  const int64_t a = (int64_t)p.pr * N, b = (int64_t)p.pc * M;
  p.total = p.dpart + (a > b ? a : b) * kD + 16;
  return p;
}
Images plain_images(float* ws, const X3Plan& p, int64_t N, int64_t M) {
  __bf16* q = reinterpret_cast<__bf16*>(ws + p.img);
  Images im;
  im.ahi = q;
  im.alo = q + N * kD;
  im.bhi = q + 2 * N * kD;
  im.blo = q + 2 * N * kD + M * kD;
  return im;
}
template <int FL>
void launch_fwd_x3_t(const FwdArgs& a, const X3Args& x, int blocks, hipStream_t st) {
  hipLaunchKernelGGL(nce_fwd_x3_k<FL>, dim3(blocks), dim3(256), 0, st, a, x);
}
template <int FL>
void launch_bwd_x3_t(const BwdArgs& a, const X3Args& x, bool row_owned, int blocks, hipStream_t st) {
  if (row_owned) hipLaunchKernelGGL((nce_bwd_x3_k<FL, true>), dim3(blocks), dim3(256), 0, st, a, x);
  else hipLaunchKernelGGL((nce_bwd_x3_k<FL, false>), dim3(blocks), dim3(256), 0, st, a, x);
}
}  // namespace

RSX_API int64_t rsx_nce_x3_workspace_floats(int64_t N, int64_t M) { return plain_plan(N, M).total; }

RSX_API int rsx_nce_fwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                           const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                           int64_t diag_offset, float tau, int flags, float* ws, float* out2, void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(N >= 0 && M >= 0, "negative size");
  RSX_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= kD && ldb >= kD, "row strides must be >=128 and multiples of 4");
  RSX_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "A/B must be 16-byte aligned");
  RSX_ARG(diag_offset >= 0 && diag_offset + N <= M, "need 0 <= diag_offset and diag_offset + N <= M");
  RSX_ARG(!(flags & (F_MASK_K1 | F_POS)) || (k1a && k1b), "k1 keys required");
  RSX_ARG(!(flags & F_MASK_K2) || (k2a && k2b), "k2 keys required");
  RSX_ARG(ws && out2, "null workspace / output");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    (void)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
    RSX_LAUNCHED();
    return 0;
  }
  const X3Plan pl = plain_plan(N, M);
  const Images im = plain_images(ws, pl, N, M);
  launch_split(B, ldb, M, im.bhi, im.blo, st);  // kept in ws for the backward's row pass
  RSX_LAUNCHED();
  const FwdArgs fa = plain_fwd_args(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, pl.nf, ws);
  const X3Args x = {im.bhi, im.blo};
  const int blocks = (int)(((N + kOwnRows - 1) / kOwnRows) * pl.nf);
  with_flags(flags, [&](auto fl) { launch_fwd_x3_t<decltype(fl)::value>(fa, x, blocks, st); });
  RSX_LAUNCHED();
  return plain_fwd_finish(fa, flags, out2, st);
}

RSX_API int rsx_nce_bwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                           const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                           int64_t diag_offset, float tau, int flags, const float* gout, float* ws, float* dA,
                           float* dB, int accumulate, void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(gout != nullptr && ws != nullptr, "gout/ws required");
  RSX_ARG(diag_offset >= 0 && diag_offset + N <= M, "need 0 <= diag_offset and diag_offset + N <= M");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return 0;
  const X3Plan pl = plain_plan(N, M);
  float* part = ws;
  float* lse = part + 4 * (int64_t)pl.nf * N;
  float* row_valid = lse + 2 * N;
  float* inv_cnt = row_valid + N;
  float* dpart = ws + pl.dpart;
  const Images im = plain_images(ws, pl, N, M);
  BwdArgs ba;
  ba.A = A; ba.B = B; ba.bias = bias;
  ba.k1a = k1a; ba.k1b = k1b; ba.k2a = k2a; ba.k2b = k2b;
  ba.N = N; ba.M = M; ba.lda = lda; ba.ldb = ldb;
  ba.diag_off = diag_offset;
  ba.inv_tau = 1.0f / tau;
  ba.lse = lse; ba.row_valid = row_valid; ba.inv_cnt = inv_cnt;
  ba.gout = gout;
  for (int pass = 0; pass < 2; ++pass) {
    const bool row_owned = pass == 0;
    float* target = row_owned ? dA : dB;
    if (!target) continue;
    const int64_t n_own = row_owned ? N : M;
    const int64_t n_str = row_owned ? M : N;
    if (n_own == 0) continue;
    const int ps = row_owned ? pl.pr : pl.pc;
    ba.nsplit = ps;
    ba.span_per_split = round_up((n_str + ps - 1) / ps, kTile);
    if (ba.span_per_split < kTile) ba.span_per_split = kTile;
    ba.dout = dpart;
    if (!row_owned) {  // B's images come from the forward; A's are made here, for the column pass
      launch_split(A, lda, N, im.ahi, im.alo, st);
      RSX_LAUNCHED();
    }
    const X3Args x = row_owned ? X3Args{im.bhi, im.blo} : X3Args{im.ahi, im.alo};
    const int blocks = (int)(((n_own + kOwnRows - 1) / kOwnRows) * ps);
    with_flags(flags, [&](auto fl) { launch_bwd_x3_t<decltype(fl)::value>(ba, x, row_owned, blocks, st); });
    RSX_LAUNCHED();
    const int64_t total4 = n_own * kD / 4;
    hipLaunchKernelGGL(nce_sum_splits_k, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dpart, ps,
                       n_own, target, accumulate);
    RSX_LAUNCHED();
  }
  return 0;
}

// ---- hard-emphasis term (full_batch_hard_emphasis_loss, v1_refine_usertower.py:762-822) ----------------
// The reference adds +margin to each row's K mined logits (torch.zeros_like(logits).scatter_) before the
// same-item mask and the cross-entropy, over an N x N logit tensor. Here the dense part is the flags-2
// InfoNCE above (never materialised) and the K entries per row are a sparse correction on its row
// statistics: with E_i = sum over allowed mined j of exp(S_ij - lse_i),
//   lse'_i = lse_i + log1p((e^margin - 1) E_i),   loss'_i = loss_i + (lse'_i - lse_i) - margin [i's own column mined],
// and, once lse'_i replaces lse_i in the workspace, the dense backward's exp(S_ij - lse'_i) - [j = label] is
// exactly the emphasised softmax gradient off the mined entries; rsx_nce_emphasis_bwd adds the mined
// entries' remaining (e^margin - 1) exp(S_ij - lse'_i). One wave per row, fp32 dot products (lane = two
// of the 128 dims), K mined columns walked in order.
namespace {
struct EmphArgs {
  const float* A; const float* B; const float* bias;
  const int* k1a; const int* k1b;
  const int64_t* top;
  int64_t N, M, K, lda, ldb, diag_off;
  float inv_tau, margin, em1;  // em1 = e^margin - 1
  float* lse; float* row_loss;
  const float* gout; float* dA; float* dB;
  float* cbuf;              // [N*K] per mined entry c_ij (0 where skipped) instead of dB atomics, or null
  const int64_t* col_ptr;   // [M+1] CSR over the mined entries sorted by column (with cbuf)
  const int64_t* col_ent;   // [N*K] entry ids i*K + r in column order
};

__device__ __forceinline__ float emph_dot(const float2 x, const float* brow, int lane) {
  const float2 y = reinterpret_cast<const float2*>(brow)[lane];
  float d = x.x * y.x + x.y * y.y;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  return d;
}

__global__ __launch_bounds__(256) void nce_emph_fwd_k(EmphArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const float lse = a.lse[i];
  if (lse == -INFINITY) return;
  const float2 x = reinterpret_cast<const float2*>(a.A + i * a.lda)[lane];
  const int64_t lab = i + a.diag_off;
  const int ki = a.k1a ? a.k1a[i] : 0;
  float e = 0.0f;
  bool self = false;
  for (int64_t r = 0; r < a.K; ++r) {
    const int64_t j = a.top[i * a.K + r];
    if (j < 0 || j >= a.M) continue;                       // host-checked; never read out of bounds
    if (j != lab && a.k1b && a.k1b[j] == ki) continue;      // same item off the label: -inf in the reference
    const float s = emph_dot(x, a.B + j * a.ldb, lane) * a.inv_tau - (a.bias ? a.bias[j] : 0.0f);
    e += __expf(s - lse);
    self |= j == lab;
  }
  if (lane == 0) {
    const float dl = log1pf(a.em1 * e);
    a.lse[i] = lse + dl;
    a.row_loss[i] += dl - (self ? a.margin : 0.0f);
  }
}

__global__ __launch_bounds__(256) void nce_emph_bwd_k(EmphArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const float lse = a.lse[i];
  if (lse == -INFINITY) return;
  const float2 x = reinterpret_cast<const float2*>(a.A + i * a.lda)[lane];
  const int64_t lab = i + a.diag_off;
  const int ki = a.k1a ? a.k1a[i] : 0;
  const float c0 = a.gout[0] * a.em1 * a.inv_tau;
  float2 acc = make_float2(0.0f, 0.0f);
  for (int64_t r = 0; r < a.K; ++r) {
    const int64_t j = a.top[i * a.K + r];
    if (j < 0 || j >= a.M) continue;
    if (j != lab && a.k1b && a.k1b[j] == ki) continue;
    const float* brow = a.B + j * a.ldb;
    const float s = emph_dot(x, brow, lane) * a.inv_tau - (a.bias ? a.bias[j] : 0.0f);
    const float c = c0 * __expf(s - lse);
    const float2 y = reinterpret_cast<const float2*>(brow)[lane];
    acc.x = fmaf(c, y.x, acc.x);
    acc.y = fmaf(c, y.y, acc.y);
    if (a.cbuf) {
      if (lane == 0) a.cbuf[i * a.K + r] = c;
    } else if (a.dB) {  // mined columns are shared between rows: vector atomics (order not deterministic)
      atomicAdd(a.dB + j * kD + 2 * lane, c * x.x);
      atomicAdd(a.dB + j * kD + 2 * lane + 1, c * x.y);
    }
  }
  if (a.dA) {  // row i belongs to this wave alone
    float2* d = reinterpret_cast<float2*>(a.dA + i * kD) + lane;
    float2 v = *d;
    v.x += acc.x;
    v.y += acc.y;
    *d = v;
  }
}

// dB from the per-entry weights: one wave per column j walks the entries mined into it (CSR, entry order
// fixed by the host's stable sort) and adds c_ij A_i; each dB row belongs to one wave (deterministic)
__global__ __launch_bounds__(256) void nce_emph_cols_k(EmphArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= a.M) return;
  const int64_t e0 = a.col_ptr[j], e1 = a.col_ptr[j + 1];
  if (e0 == e1) return;
  float2 acc = make_float2(0.0f, 0.0f);
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t ent = a.col_ent[e];
    const float c = a.cbuf[ent];
    if (c == 0.0f) continue;  // wave-uniform
    const float2 x = reinterpret_cast<const float2*>(a.A + (ent / a.K) * a.lda)[lane];
    acc.x = fmaf(c, x.x, acc.x);
    acc.y = fmaf(c, x.y, acc.y);
  }
  float2* d = reinterpret_cast<float2*>(a.dB + j * kD) + lane;
  float2 v = *d;
  v.x += acc.x;
  v.y += acc.y;
  *d = v;
}

int emph_setup(EmphArgs& e, const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
               const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb, int64_t diag_offset,
               float tau, float margin, int precision, int nsplit_fwd, float* ws) {
  RSX_ARG(A && B && top && ws, "null tensor");
  RSX_ARG(precision == RSX_NCE_FP32 || precision == RSX_NCE_BF16X3, "precision must be 0 (fp32) or 1 (bf16x3)");
  RSX_ARG(N >= 0 && M >= 0 && K >= 0, "negative size");
  RSX_ARG(diag_offset >= 0 && diag_offset + N <= M, "need 0 <= diag_offset and diag_offset + N <= M");
  RSX_ARG(lda % 2 == 0 && ldb % 2 == 0 && lda >= kD && ldb >= kD, "row strides must be >= 128 and even");
  RSX_ARG((k1a == nullptr) == (k1b == nullptr), "k1 keys: both or neither");
  RSX_ARG(tau > 0.0f, "tau must be > 0");
  const int nf = precision == RSX_NCE_FP32 ? nsplit_fwd : plain_plan(N, M).nf;
  RSX_ARG(nf >= 1, "nsplit_fwd must be >= 1");
  e.A = A; e.B = B; e.bias = bias; e.k1a = k1a; e.k1b = k1b; e.top = top;
  e.N = N; e.M = M; e.K = K; e.lda = lda; e.ldb = ldb; e.diag_off = diag_offset;
  e.inv_tau = 1.0f / tau;
  e.margin = margin;
  e.em1 = expm1f(margin);
  e.lse = ws + 4 * (int64_t)nf * N;
  e.row_loss = e.lse + N;
  e.gout = nullptr; e.dA = nullptr; e.dB = nullptr;
  e.cbuf = nullptr; e.col_ptr = nullptr; e.col_ent = nullptr;
  return 0;
}
}  // namespace

RSX_API int rsx_nce_emphasis_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                                 const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb,
                                 int64_t diag_offset, float tau, float margin, int precision, int nsplit_fwd,
                                 float* ws, float* out2, void* stream) {
  EmphArgs e;
  const int rc = emph_setup(e, A, B, bias, k1a, k1b, top, N, M, K, lda, ldb, diag_offset, tau, margin, precision,
                            nsplit_fwd, ws);
  if (rc) return rc;
  RSX_ARG(out2 != nullptr, "null output");
  if (N == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (K > 0) {
    hipLaunchKernelGGL(nce_emph_fwd_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, e);
    RSX_LAUNCHED();
  }
  hipLaunchKernelGGL(nce_reduce_k, dim3(1), dim3(1024), 0, st, e.row_loss, e.row_loss + N, N, out2);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_nce_emphasis_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                                 const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb,
                                 int64_t diag_offset, float tau, float margin, int precision, int nsplit_fwd,
                                 const float* gout, float* ws, float* dA, float* dB, void* stream) {
  EmphArgs e;
  const int rc = emph_setup(e, A, B, bias, k1a, k1b, top, N, M, K, lda, ldb, diag_offset, tau, margin, precision,
                            nsplit_fwd, ws);
  if (rc) return rc;
  RSX_ARG(gout != nullptr, "gout required");
  if (N == 0 || K == 0 || (!dA && !dB)) return 0;
  e.gout = gout; e.dA = dA; e.dB = dB;
  hipLaunchKernelGGL(nce_emph_bwd_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, e);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_nce_emphasis_bwd_csr(const float* A, const float* B, const float* bias, const int* k1a,
                                     const int* k1b, const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda,
                                     int64_t ldb, int64_t diag_offset, float tau, float margin, int precision,
                                     int nsplit_fwd, const int64_t* col_ptr, const int64_t* col_ent, float* cbuf,
                                     const float* gout, float* ws, float* dA, float* dB, void* stream) {
  EmphArgs e;
  const int rc = emph_setup(e, A, B, bias, k1a, k1b, top, N, M, K, lda, ldb, diag_offset, tau, margin, precision,
                            nsplit_fwd, ws);
  if (rc) return rc;
  RSX_ARG(gout != nullptr, "gout required");
  RSX_ARG(!dB || (col_ptr && col_ent && cbuf), "dB needs the column CSR and the entry buffer");
  if (N == 0 || K == 0 || (!dA && !dB)) return 0;
  hipStream_t st = (hipStream_t)stream;
  e.gout = gout; e.dA = dA; e.dB = dB;
  if (dB) {
    e.cbuf = cbuf; e.col_ptr = col_ptr; e.col_ent = col_ent;
    (void)hipMemsetAsync(cbuf, 0, (size_t)(N * K) * sizeof(float), st);  // skipped entries keep 0
  }
  hipLaunchKernelGGL(nce_emph_bwd_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, e);
  RSX_LAUNCHED();
  if (dB) {
    hipLaunchKernelGGL(nce_emph_cols_k, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, e);
    RSX_LAUNCHED();
  }
  return 0;
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
  RSX_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= kD && ldb >= kD, "row strides must be >=128 and multiples of 4");
  RSX_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "A/B must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    (void)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
    RSX_LAUNCHED();
    return 0;
  }
  float* part = ws;
  float* lse = part + 4 * (int64_t)nsplit * N;
  float* row_loss = lse + N;
  float* row_valid = row_loss + N;
  GArgs g = {};
  g.A = A; g.B = B; g.bias = bias; g.colcnt = colcnt;
  g.row_col = row_col; g.row_beg = row_beg; g.row_end = row_end; g.exc_cols = exc_cols;
  g.N = N; g.M = D; g.lda = lda; g.ldb = ldb;
  g.inv_tau = 1.0f / tau;
  g.nsplit = nsplit;
  g.span = round_up((D + nsplit - 1) / nsplit, kTile);
  if (g.span < kTile) g.span = kTile;
  g.part = part;
  const int blocks = (int)(((N + kOwnRows - 1) / kOwnRows) * nsplit);
  if (precision == RSX_NCE_BF16X3) {
    const Images im = grouped_images(ws, N, D, nsplit, kNsplitBwdGrouped);
    g.bhi = im.bhi;
    g.blo = im.blo;
    launch_split(B, ldb, D, im.bhi, im.blo, st);  // kept in ws for the backward's row pass
    RSX_LAUNCHED();
    hipLaunchKernelGGL(nce_grouped_fwd_x3_k, dim3(blocks), dim3(256), 0, st, g);
  } else {
    hipLaunchKernelGGL(nce_grouped_fwd_k, dim3(blocks), dim3(256), 0, st, g);
  }
  RSX_LAUNCHED();
  hipLaunchKernelGGL(nce_grouped_merge_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, A, B, bias, row_col, N,
                     lda, ldb, g.inv_tau, nsplit, part, lse, row_loss, row_valid);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(nce_reduce_k, dim3(1), dim3(1024), 0, st, row_loss, row_valid, N, out2);
  RSX_LAUNCHED();
  return 0;
}

// Measurement hooks (include/recsys_amd.h): event pairs around the fused forward kernel's launch.
namespace {
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
}  // namespace

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
  RSX_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= kD && ldb >= kD, "row strides must be >=128 and multiples of 4");
  RSX_ARG(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "A/B must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    (void)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
    RSX_LAUNCHED();
    return 0;
  }
  float* part = ws;
  float* lse = part + 4 * (int64_t)nsplit * N;
  float* row_loss = lse + N;
  float* row_valid = row_loss + N;
  float* opart = lse + 4 * N;  // the backward's split-partial region (>= nsplit x N x 128)
  // nsplit = 8 (the partial slots per row): the leading row blocks run 4 column splits, as many
  // as fill whole rounds of the grid at two workgroups per CU; the remaining row blocks run 8
  // half-length splits, dispatched last, so the grid's final round is short and full
  // (batch 8192: 1,152 row blocks x 4 = 9 rounds of 512, then 45 x 8 half-length workgroups)
  const bool h16 = precision == RSX_NCE_F16;
  const int64_t rbs = (N + kOwnRows - 1) / kOwnRows;
  const int ns1 = nsplit == 8 ? 4 : nsplit;
  int64_t rb1 = rbs;
  if (nsplit == 8) {
    const int64_t slots = 2 * (int64_t)rsx::cu_count();
    rb1 = (ns1 * rbs / slots) * slots / ns1;  // whole rounds of the 4-split blocks
  }
  GArgs g = {};
  g.A = A; g.B = B; g.bias = bias; g.colcnt = colcnt;
  g.row_col = row_col; g.row_beg = row_beg; g.row_end = row_end; g.exc_cols = exc_cols;
  g.N = N; g.M = D; g.lda = lda; g.ldb = ldb;
  g.inv_tau = 1.0f / tau;
  g.nsplit = ns1;
  g.span = round_up((D + ns1 - 1) / ns1, kTile);
  if (g.span < kTile) g.span = kTile;
  g.rb1 = rb1;
  g.nsplit2 = 8;
  g.span2 = round_up((D + 7) / 8, kTile);
  if (g.span2 < kTile) g.span2 = kTile;
  g.nslots = nsplit;
  g.part = part;
  g.dout = opart;
  const Images im = grouped_images(ws, N, D, nsplit, kNsplitBwdGrouped);
  g.bhi = im.bhi;
  g.blo = im.blo;
  if (h16) launch_split_h(B, ldb, D, im.bhi, im.blo, st);
  else launch_split(B, ldb, D, im.bhi, im.blo, st);
  RSX_LAUNCHED();
  const int blocks = (int)(rb1 * ns1 + (rbs - rb1) * (nsplit == 8 ? 8 : 0));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  {
    KernelEvents& k = kernel_events();
    std::lock_guard<std::mutex> lk(k.mu);
    if (k.on && hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess) {
      (void)hipEventRecord(ev0, st);
      k.ev.emplace_back(ev0, ev1);
    }
  }
  if (h16 && f16_gp() == 2)
    hipLaunchKernelGGL(nce_grouped_fwdg_h_k<2>, dim3(blocks), dim3(256), 0, st, g);
  else if (h16)
    hipLaunchKernelGGL(nce_grouped_fwdg_h_k<1>, dim3(blocks), dim3(256), 0, st, g);
  else
    hipLaunchKernelGGL(nce_grouped_fwdg_x3p_k, dim3(blocks), dim3(256), 0, st, g);
  RSX_LAUNCHED();
  if (ev1) (void)hipEventRecord(ev1, st);
  hipLaunchKernelGGL(nce_grouped_merge_g_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, A, B, bias, row_col,
                     N, lda, ldb, g.inv_tau, ns1, part, opart, lse, row_loss, row_valid, ga, rb1 * kOwnRows, 8,
                     nsplit, h16 ? 1 : 0);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(nce_reduce_k, dim3(1), dim3(1024), 0, st, row_loss, row_valid, N, out2);
  RSX_LAUNCHED();
  return 0;
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
  float* part = ws;
  float* lse = part + 4 * (int64_t)nsplit_fwd * N;
  float* dpart = lse + 4 * N;
  GArgs g = {};
  g.A = A; g.B = B; g.bias = bias; g.colcnt = colcnt;
  g.row_col = row_col; g.row_beg = row_beg; g.row_end = row_end; g.exc_cols = exc_cols;
  g.col_beg = col_beg; g.col_end = col_end; g.exc_s = exc_s; g.exc_e = exc_e; g.exc_n = exc_n;
  g.N = N; g.M = D; g.lda = lda; g.ldb = ldb;
  g.inv_tau = 1.0f / tau;
  g.nsplit = nsplit;
  g.lse = lse;
  g.gout = gout;
  g.dout = dpart;
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
    if (!row_owned && precision != RSX_NCE_FP32) {
      // column pass: 32 (else 16) splits in a split-major block order, so each XCD's L2 holds the
      // one split of A's images it streams (the 8-split span, N/8 rows = 9.8 MB at batch 8192, does
      // not fit a 4-MB L2): 5.5 -> 5.0-5.1 ms at batch 8192 (profiles/r02_nce_colsplit_ab.json).
      // Bounded by the partial region (nsplit x max(N, D) rows).
      const int64_t cap = (int64_t)nsplit * (N > D ? N : D);
      for (int want : {32, 16}) {
        if ((int64_t)want * n_own <= cap && N >= (int64_t)want * 2 * kTile) {
          ps = want;
          g.split_major = 1;
          break;
        }
      }
    }
    g.nsplit = ps;
    g.span = round_up((n_str + ps - 1) / ps, kTile);
    if (g.span < kTile) g.span = kTile;
    const int blocks = (int)(own_blocks * ps);
    const bool h16 = precision == RSX_NCE_F16;
    const bool x3 = precision != RSX_NCE_FP32;
    if (x3) {
      const Images im = grouped_images(ws, N, D, nsplit_fwd, kNsplitBwdGrouped);
      g.ahi = im.ahi; g.alo = im.alo; g.bhi = im.bhi; g.blo = im.blo;
      if (!row_owned) {  // B's images come from the forward; A's are made here, for the col pass
        if (h16) launch_split_h(A, lda, N, im.ahi, im.alo, st);
        else launch_split(A, lda, N, im.ahi, im.alo, st);
        RSX_LAUNCHED();
      } else if (h16) {  // the row pass streams bf16 images of B (a fused f16 forward left fp16 ones)
        launch_split(B, ldb, D, im.bhi, im.blo, st);
        RSX_LAUNCHED();
      }
    }
    if (!row_owned && h16 && f16_gp() == 2)
      hipLaunchKernelGGL(nce_grouped_bwd_cols_h_k<2>, dim3(blocks), dim3(256), 0, st, g);
    else if (!row_owned && h16)
      hipLaunchKernelGGL((nce_grouped_bwd_cols_h_k<1, 2>), dim3(blocks), dim3(256), 0, st, g);
    else if (row_owned && x3) hipLaunchKernelGGL((nce_grouped_bwd_x3_k<true, false>), dim3(blocks), dim3(256), 0, st, g);
    else if (x3) hipLaunchKernelGGL((nce_grouped_bwd_x3_k<false, true>), dim3(blocks), dim3(256), 0, st, g);
    else if (row_owned) hipLaunchKernelGGL(nce_grouped_bwd_k<true>, dim3(blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(nce_grouped_bwd_k<false>, dim3(blocks), dim3(256), 0, st, g);
    RSX_LAUNCHED();
    const int64_t total4 = n_own * kD / 4;
    hipLaunchKernelGGL(nce_sum_splits_k, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dpart, ps,
                       n_own, target, accumulate);
    RSX_LAUNCHED();
  }
  return 0;
}
