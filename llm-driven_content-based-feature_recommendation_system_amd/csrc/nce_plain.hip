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
//   * logq_correction_loss         tower_code/mined_inference.py:738-749: flags 2, bias_j = lambda log(p_j + 1e-4) / tau
//   * efficient_corrected_logq_loss  mined_inference.py:751-789: the same with the label logit restored to
//       <A_i, B_i> / tau (F_DIAG_NOBIAS: the bias applies off the diagonal only)
//
// This file: the plain (ungrouped) kernels and the small kernels every family launches, behind
// nce_common.h's launchers. Grouped form: nce_grouped*.hip; emphasis: nce_emphasis.hip.
//
// One forward body nce_fwd_k<FL, P> and one backward body nce_bwd_k<FL, ROW_OWNED, P> over a product
// type P (nce_mfma.h): F32Prod, the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact f32 FMA chain, no
// reduced-precision path on gfx950), or X3Prod, bf16x3 products on hi/lo images that the drivers
// split into ws. The objective lives in the bodies, once per direction: the per-pair rule (excl,
// offdiag, the same-key masks, SupCon's positives, the label y) and the online log-sum-exp; P only
// says how rows are held, staged and multiplied. The pair rule is kept as plain text in both bodies,
// not in a helper: hipcc compiles the short-circuit form and a call differently, and at 256 VGPRs
// that moved the backward's spills.
//
// Each wave keeps 32 rows of its "owner" operand in registers and streams 32-row tiles of the other
// operand through LDS. The accumulator tile is computed transposed (streamed rows in registers,
// owner row on the lane), so the online log-sum-exp is lane-local and the tile doubles as the A
// operand of the gradient MFMA in the backward (no LDS round trip for dS).
#include "nce_common.h"
#include "nce_mfma.h"

using namespace rsx::nce;

namespace {

template <int FL, typename P>
__global__ __launch_bounds__(256, 2) void nce_fwd_k(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) typename P::Tile sT[2];
  __shared__ __attribute__((aligned(16))) float sBias[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK1[2][kTile];
  __shared__ __attribute__((aligned(16))) int sK2[2][kTile];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  int split, rb;
  remap_block(a.nsplit, split, rb);
  const int64_t i = (int64_t)rb * kOwnRows + wave * 32 + c;
  const bool row_ok = i < a.N;

  typename P::Owner u;
  typename P::OwnerLo ul;
  P::load_owner(u, ul, a.A, i, a.lda, row_ok, h);
  int k1i = 0, k2i = 0;
  if (row_ok) {
    if ((FL & (F_MASK_K1 | F_POS)) && a.k1a) k1i = a.k1a[i];
    if ((FL & F_MASK_K2) && a.k2a) k2i = a.k2a[i];
  }

  const int64_t j_begin = (int64_t)split * a.cols_per_split;
  int64_t j_end = j_begin + a.cols_per_split;
  if (j_end > a.M) j_end = a.M;

  float m = -INFINITY, l = 0.0f, ps = 0.0f, pc = 0.0f;

  typename P::Stage stg = P::stage(tid);
  float stg_bias = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;

  auto gload = [&](int64_t j0) {
    const int64_t j = j0 + (tid >> 3);
    stg.load(P::src(a.B, a.ldb, a.shi, a.slo), j, j < j_end, tid);
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

      const f32x16 acc = P::dots(sT[cur], u, ul, c, h);

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
          const bool offdiag = (j != i + a.diag_off);
          const float s = acc[r] * a.inv_tau - (((FL & F_DIAG_NOBIAS) && !offdiag) ? 0.0f : bia[e]);
          bool excl = (j >= j_end) || !row_ok;
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
      if (P::kStoreAfterBarrier) __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  fold_store_partials<true>(a.part, a.nsplit, split, a.N, i, row_ok, h, m, l, ps, pc);
}

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
    const float sii = d * a.inv_tau - ((a.bias && !a.diag_nobias) ? a.bias[i + a.diag_off] : 0.0f);
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

template <int FL, bool ROW_OWNED, typename P>
__global__ __launch_bounds__(256, 2) void nce_bwd_k(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) typename P::Tile sT[2];
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
  typename P::Owner u;
  typename P::OwnerLo ul;
  P::load_owner(u, ul, own, o, ld_own, own_ok, h);
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

  typename P::Stage stg = P::stage(tid);
  float stg0 = 0.0f, stg1 = 0.0f, stg2 = 0.0f;
  int stg_k1 = 0, stg_k2 = 0;

  auto gload = [&](int64_t s0) {
    const int64_t sidx = s0 + (tid >> 3);
    stg.load(P::src(str, ld_str, a.shi, a.slo), sidx, sidx < s_end, tid);
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

      // acc[r] = <own_o, str_s>, s = s0 + tile_row(r,h). Turn it into G (in place).
      f32x16 acc = P::dots(sT[cur], u, ul, c, h);
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
          const bool offdiag = (jj != ii + a.diag_off);
          const float sv = acc[r] * a.inv_tau - (((FL & F_DIAG_NOBIAS) && !offdiag) ? 0.0f : bias_j);
          bool excl = (sidx >= s_end) || !own_ok;
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

      // d_own[o][kb*32 + n] += sum_s G[o][s] * str[s][kb*32 + n]
      P::grad(gacc, acc, sT[cur], lane, c, h);

      if (P::kStoreAfterBarrier) __syncthreads();
      if (has_next) lstore(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  store_d_own((int64_t)ob * kOwnRows + wave * 32, a.dout + (int64_t)split * n_own * kD, n_own, h, c, gacc);
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

// rows x 128 fp32 (row stride ld) -> hi/lo images [rows][128], one thread per 8 floats: bf16, or
// (HALF) the fp16 images of x * 2^8 in the same containers
template <bool HALF>
__global__ __launch_bounds__(256) void nce_split_k(const float* src, int64_t ld, int64_t rows, __bf16* hi,
                                                   __bf16* lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 8-float chunk index
  if (i >= rows * (kD / 8)) return;
  const int64_t r = i / (kD / 8), c8 = i % (kD / 8);
  const float4* p = reinterpret_cast<const float4*>(src + r * ld + c8 * 8);
  bf16x8 h, l;
  if (HALF) split8_h(p[0], p[1], h, l);
  else split8(p[0], p[1], h, l);
  *reinterpret_cast<bf16x8*>(hi + r * kD + c8 * 8) = h;
  *reinterpret_cast<bf16x8*>(lo + r * kD + c8 * 8) = l;
}

// ---- host side: the forward entry points' checks on their operands
const char* fwd_error(const float* A, const float* B, const int* k1a, const int* k1b, const int* k2a, const int* k2b,
                      int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, int flags) {
  if (!valid_flags(flags)) return "unsupported flag combination";
  if (N < 0 || M < 0) return "negative size";
  if (const char* m = operand_error(A, B, lda, ldb)) return m;
  if (const char* m = diag_error(N, M, diag_offset)) return m;
  if ((flags & (F_MASK_K1 | F_POS)) && !(k1a && k1b)) return "k1 keys required";
  if ((flags & F_MASK_K2) && !(k2a && k2b)) return "k2 keys required";
  return nullptr;
}

// Forward over L.nf column splits, then the merge into the per-row statistics and their sums
// out2. im (bf16x3): B's images are split here and kept in ws for the backward's row pass.
int plain_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, const int* k2a,
              const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau,
              int flags, const StatsLayout& L, const Images* im, float* ws, float* out2, hipStream_t st) {
  if (N == 0) return zero_sums(out2, st);
  if (im) {
    launch_split(B, ldb, M, im->bhi, im->blo, false, st);
    RSX_LAUNCHED();
  }
  FwdArgs fa;
  fa.A = A; fa.B = B; fa.bias = bias;
  fa.k1a = k1a; fa.k1b = k1b; fa.k2a = k2a; fa.k2b = k2b;
  fa.N = N; fa.M = M; fa.lda = lda; fa.ldb = ldb;
  fa.diag_off = diag_offset;
  fa.inv_tau = 1.0f / tau;
  fa.nsplit = L.nf;
  fa.cols_per_split = split_span(M, L.nf);
  fa.part = ws + L.part;
  fa.shi = im ? im->bhi : nullptr;
  fa.slo = im ? im->blo : nullptr;
  const int blocks = (int)(((N + kOwnRows - 1) / kOwnRows) * L.nf);
  with_flags(flags, [&](auto fl) {
    constexpr int FL = decltype(fl)::value;
    if (im) hipLaunchKernelGGL((nce_fwd_k<FL, X3Prod>), dim3(blocks), dim3(256), 0, st, fa);
    else hipLaunchKernelGGL((nce_fwd_k<FL, F32Prod>), dim3(blocks), dim3(256), 0, st, fa);
  });
  RSX_LAUNCHED();
  MergeArgs ma;
  ma.A = A; ma.B = B; ma.bias = bias;
  ma.N = N; ma.lda = lda; ma.ldb = ldb;
  ma.diag_off = diag_offset;
  ma.inv_tau = fa.inv_tau;
  ma.nsplit = L.nf;
  ma.part = fa.part;
  ma.pos_mode = (flags & F_POS) ? 1 : 0;
  ma.diag_nobias = (flags & F_DIAG_NOBIAS) ? 1 : 0;
  ma.lse = ws + L.lse; ma.row_loss = ws + L.row_loss; ma.row_valid = ws + L.row_valid; ma.inv_cnt = ws + L.inv_cnt;
  hipLaunchKernelGGL(nce_merge_k, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, ma);
  RSX_LAUNCHED();
  launch_reduce(ma.row_loss, ma.row_valid, N, out2, st);
  RSX_LAUNCHED();
  return 0;
}

// Backward: the row pass (dA, pr splits) and the column pass (dB, pc splits), each into the
// split partials at ws + dpart (room for dpart_cap floats) and summed into its target.
// im (bf16x3): B's images come from the forward; A's are made here, for the column pass.
int plain_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, const int* k2a,
              const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau,
              int flags, const StatsLayout& L, int pr, int pc, int64_t dpart, int64_t dpart_cap, const Images* im,
              const float* gout, float* ws, float* dA, float* dB, int accumulate, hipStream_t st) {
  if (N == 0) return 0;
  BwdArgs ba;
  ba.A = A; ba.B = B; ba.bias = bias;
  ba.k1a = k1a; ba.k1b = k1b; ba.k2a = k2a; ba.k2b = k2b;
  ba.N = N; ba.M = M; ba.lda = lda; ba.ldb = ldb;
  ba.diag_off = diag_offset;
  ba.inv_tau = 1.0f / tau;
  ba.lse = ws + L.lse; ba.row_valid = ws + L.row_valid; ba.inv_cnt = ws + L.inv_cnt;
  ba.gout = gout;
  ba.dout = ws + dpart;
  for (int pass = 0; pass < 2; ++pass) {
    const bool row_owned = pass == 0;
    float* target = row_owned ? dA : dB;
    if (!target) continue;
    const int64_t n_own = row_owned ? N : M;
    const int64_t n_str = row_owned ? M : N;
    if (n_own == 0) continue;
    const int ps = row_owned ? pr : pc;
    RSX_ARG((int64_t)ps * n_own * kD <= dpart_cap, "split partials exceed their workspace region");
    ba.nsplit = ps;
    ba.span_per_split = split_span(n_str, ps);
    ba.shi = !im ? nullptr : row_owned ? im->bhi : im->ahi;
    ba.slo = !im ? nullptr : row_owned ? im->blo : im->alo;
    if (im && !row_owned) {
      launch_split(A, lda, N, im->ahi, im->alo, false, st);
      RSX_LAUNCHED();
    }
    const int blocks = (int)(((n_own + kOwnRows - 1) / kOwnRows) * ps);
    with_flags(flags, [&](auto fl) {
      constexpr int FL = decltype(fl)::value;
      if (im && row_owned) hipLaunchKernelGGL((nce_bwd_k<FL, true, X3Prod>), dim3(blocks), dim3(256), 0, st, ba);
      else if (im) hipLaunchKernelGGL((nce_bwd_k<FL, false, X3Prod>), dim3(blocks), dim3(256), 0, st, ba);
      else if (row_owned) hipLaunchKernelGGL((nce_bwd_k<FL, true, F32Prod>), dim3(blocks), dim3(256), 0, st, ba);
      else hipLaunchKernelGGL((nce_bwd_k<FL, false, F32Prod>), dim3(blocks), dim3(256), 0, st, ba);
    });
    RSX_LAUNCHED();
    launch_sum_splits(ba.dout, ps, n_own, target, accumulate, st);
    RSX_LAUNCHED();
  }
  return 0;
}

}  // namespace

void rsx::nce::launch_reduce(const float* row_loss, const float* row_valid, int64_t N, float* out2, hipStream_t st) {
  hipLaunchKernelGGL(nce_reduce_k, dim3(1), dim3(1024), 0, st, row_loss, row_valid, N, out2);
}

void rsx::nce::launch_sum_splits(const float* part, int nsplit, int64_t n_own, float* out, int accumulate,
                                 hipStream_t st) {
  const int64_t total4 = n_own * kD / 4;
  hipLaunchKernelGGL(nce_sum_splits_k, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, part, nsplit, n_own,
                     out, accumulate);
}

void rsx::nce::launch_split(const float* src, int64_t ld, int64_t rows, __bf16* hi, __bf16* lo, bool half,
                            hipStream_t st) {
  const int64_t n = rows * (kD / 8);
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (half) hipLaunchKernelGGL(nce_split_k<true>, grid, dim3(256), 0, st, src, ld, rows, hi, lo);
  else hipLaunchKernelGGL(nce_split_k<false>, grid, dim3(256), 0, st, src, ld, rows, hi, lo);
}

RSX_API int64_t rsx_nce_workspace_floats(int64_t N, int64_t M, int nsplit_fwd, int nsplit_bwd) {
  return PlainLayout(N, M, nsplit_fwd, nsplit_bwd).total;
}

RSX_API int64_t rsx_nce_x3_workspace_floats(int64_t N, int64_t M) { return PlainX3Layout(N, M).total; }

// Forward: writes lse/row_loss/row_valid/inv_cnt (ws) and out2 = {sum of row losses, n_valid}.
RSX_API int rsx_nce_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                        const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                        int64_t diag_offset, float tau, int flags, int nsplit, float* ws, float* out2,
                        void* stream) {
  RSX_ARG(nsplit >= 8 && nsplit <= 64 && nsplit % 8 == 0, "nsplit must be a multiple of 8 in [8,64]");
  NCE_REQUIRE(fwd_error(A, B, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, flags));
  return plain_fwd(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, flags, StatsLayout(N, nsplit),
                   nullptr, ws, out2, (hipStream_t)stream);
}

// Backward: dA (N x 128) and/or dB (M x 128); accumulate != 0 adds into them.
RSX_API int rsx_nce_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                        const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                        int64_t diag_offset, float tau, int flags, int nsplit_fwd, int nsplit, const float* gout,
                        float* ws, float* dA, float* dB, int accumulate, void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(nsplit >= 8 && nsplit <= 64 && nsplit % 8 == 0, "nsplit must be a multiple of 8 in [8,64]");
  RSX_ARG(gout != nullptr, "gout required");
  NCE_REQUIRE(diag_error(N, M, diag_offset));
  const PlainLayout L(N, M, nsplit_fwd, nsplit);
  return plain_bwd(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, flags, L, nsplit, nsplit, L.dpart,
                   L.dpart_cap, nullptr, gout, ws, dA, dB, accumulate, (hipStream_t)stream);
}

RSX_API int rsx_nce_fwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                           const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                           int64_t diag_offset, float tau, int flags, float* ws, float* out2, void* stream) {
  NCE_REQUIRE(fwd_error(A, B, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, flags));
  RSX_ARG(ws && out2, "null workspace / output");
  const PlainX3Layout L(N, M);
  const Images im = images_at(ws, L.img, N, M);
  return plain_fwd(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, flags, L, &im, ws, out2,
                   (hipStream_t)stream);
}

RSX_API int rsx_nce_bwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                           const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                           int64_t diag_offset, float tau, int flags, const float* gout, float* ws, float* dA,
                           float* dB, int accumulate, void* stream) {
  RSX_ARG(valid_flags(flags), "unsupported flag combination");
  RSX_ARG(gout != nullptr && ws != nullptr, "gout/ws required");
  NCE_REQUIRE(diag_error(N, M, diag_offset));
  const PlainX3Layout L(N, M);
  const Images im = images_at(ws, L.img, N, M);
  return plain_bwd(A, B, bias, k1a, k1b, k2a, k2b, N, M, lda, ldb, diag_offset, tau, flags, L, L.pr, L.pc, L.dpart,
                   L.dpart_cap, &im, gout, ws, dA, dB, accumulate, (hipStream_t)stream);
}
