// Evaluation of a binary ranker on the device: exact tie-aware ROC-AUC (as the integer 2 U) and
// the Logloss sum of R scored rows, for one host read.
// Reference: the validation half of RecommendationRanker.train (temp_model/ranker_skelet.py:98-108
// eval_metric='AUC', early_stopping_rounds; :123-135 eval_set / use_best_model), which CatBoost
// computes on the host.
//
//   P = #{y == 1}, N = #{y == 0},
//   U2 = sum over positive rows i of #{negative j : z_j < z_i} + #{negative j : z_j <= z_i}
// (twice the Mann-Whitney U with ties at one half; AUC = U2 / (2 P N) on the host, in double).
// Scores compare as reals (-0.0 == +0.0). In the rows sorted by score, with cn = the inclusive count
// of negatives, a positive of the tie group [s, e] contributes cn[s] - neg[s] (the negatives
// before its group) + cn[e] (those up to its group's end).
//
//   be_key_k    z -> order-preserving uint32 key (-0.0 canonicalised, sign-flip transform), y -> a
//               uint8 label, the input flags, and the per-workgroup Logloss partials (double)
//   rocprim::radix_sort_pairs over the (key, label) pairs (what hipCUB's SortPairs calls)
//   be_tile_k<false>  per 2048-row tile of the sorted rows: its negatives, the tile-local exclusive
//               count at its last group head and the inclusive count at its first group tail
//   be_carry_k  one workgroup over the tiles: exclusive sum of the negatives (which gives N, and
//               P = R - N), a forward max-scan of the heads' values and a backward min-scan of the
//               tails' (cn is non-decreasing, so the latest head at or before a row is a max, the
//               first tail at or after it a min); the Logloss partials added in a fixed order
//   be_tile_k<true>   the same tile-local scans with the carries: every positive adds its two
//               counts; one 64-bit integer atomic per workgroup
// No step walks a tie group: one group over all R rows costs what distinct scores cost. The sums
// are integers (any order gives the same bits); the only floating-point sum is the Logloss, whose
// order is fixed.
#include "rsx_block.h"
#include "rsx_common.h"
#include "rsx_x3.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <limits.h>

namespace {

using rsx::at, rsx::block_scan_excl, rsx::score_key, rsx::Sum;

constexpr int kThreads = 256, kPer = 8, kTile = kThreads * kPer;
constexpr int kLossSlots = 1024;  // workgroups of the key pass (each one Logloss partial)
constexpr int kNone = -1;         // "no head in range" (every real count is >= 0)

// The library's radix sort with its own tuning, except the size up to which it merge-sorts instead of
// running the onesweep radix passes: its default is 2^20 rows, but measured on an MI355X with these
// 5-byte pairs (whole evaluation, merge sort / onesweep): 65,536 rows 0.076 / 0.120 ms, 262,144 rows
// 0.127 / 0.129 ms, 1,048,576 rows 0.204 / 0.157 ms (profiles/deepfm_eval_sort_ab.json).
#ifndef RSX_BE_MERGE_LIMIT
#define RSX_BE_MERGE_LIMIT (256 * 1024)
#endif
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                              rocprim::default_config, RSX_BE_MERGE_LIMIT>;

hipError_t sort_pairs(void* tmp, size_t& bytes, const unsigned* kin, unsigned* kout, const uint8_t* vin, uint8_t* vout,
                      int64_t R, hipStream_t st) {
  return rocprim::radix_sort_pairs<SortConfig>(tmp, bytes, kin, kout, vin, vout, (size_t)R, 0u, 32u, st);
}

struct Max {
  __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; }
};
struct Min {
  __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void be_key_k(const float* __restrict__ logit, const float* __restrict__ y,
                                                      int64_t R, int64_t tiles, unsigned* __restrict__ keys,
                                                      uint8_t* __restrict__ lab, double* __restrict__ lpart,
                                                      int* __restrict__ flag) {
  __shared__ double sW[kThreads / 64];
  __shared__ int sBad;
  if (threadIdx.x == 0) sBad = 0;
  __syncthreads();
  double acc = 0.0;
  int bad = 0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i0 = t * kTile + (int64_t)threadIdx.x * kPer;
    float z[kPer], yy[kPer];
    const bool full = i0 + kPer <= R;
    if (VEC && full) {
#pragma unroll
      for (int q = 0; q < kPer / 4; ++q) {
        const float4 a = reinterpret_cast<const float4*>(logit + i0)[q];
        const float4 b = reinterpret_cast<const float4*>(y + i0)[q];
        z[4 * q] = a.x, z[4 * q + 1] = a.y, z[4 * q + 2] = a.z, z[4 * q + 3] = a.w;
        yy[4 * q] = b.x, yy[4 * q + 1] = b.y, yy[4 * q + 2] = b.z, yy[4 * q + 3] = b.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const bool in = i0 + j < R;
        z[j] = in ? logit[i0 + j] : 0.0f;
        yy[j] = in ? y[i0 + j] : 0.0f;
      }
    }
    unsigned k[kPer];
    uint8_t l[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const bool in = i0 + j < R;
      k[j] = score_key(z[j]);
      l[j] = yy[j] == 1.0f ? 1 : 0;
      if (in) {
        if (!(fabsf(z[j]) <= 3.402823466e38f)) bad |= 1;  // NaN or +-inf
        if (!(yy[j] == 0.0f || yy[j] == 1.0f)) bad |= 2;
        const double zd = (double)z[j];
        acc += fmax(zd, 0.0) - zd * (double)yy[j] + log1p(exp(-fabs(zd)));
      }
    }
    if (full) {  // the workspace arrays are 256-byte aligned and i0 is a multiple of 8
      reinterpret_cast<uint4*>(keys + i0)[0] = make_uint4(k[0], k[1], k[2], k[3]);
      reinterpret_cast<uint4*>(keys + i0)[1] = make_uint4(k[4], k[5], k[6], k[7]);
      uint2 p;
      p.x = l[0] | (l[1] << 8) | (l[2] << 16) | ((unsigned)l[3] << 24);
      p.y = l[4] | (l[5] << 8) | (l[6] << 16) | ((unsigned)l[7] << 24);
      *reinterpret_cast<uint2*>(lab + i0) = p;
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (i0 + j < R) {
          keys[i0 + j] = k[j];
          lab[i0 + j] = l[j];
        }
    }
  }
  if (bad) atomicOr(&sBad, bad);
  // fixed order: the thread's rows in row order, a fixed butterfly over the wave, the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) s += sW[w];
    lpart[blockIdx.x] = s;
    if (sBad) atomicOr(flag, sBad);
  }
}

struct TileArrays {
  int *neg, *head, *tail;     // per tile: negatives, local count at the last head / first tail
  int *negoff, *carry_h, *carry_t;  // be_carry_k's outputs
};

// One 2048-row tile of the sorted rows, 8 consecutive rows per thread.
template <bool APPLY>
__global__ __launch_bounds__(kThreads) void be_tile_k(const unsigned* __restrict__ skeys,
                                                       const uint8_t* __restrict__ slab, int64_t R, TileArrays ta,
                                                       unsigned long long* __restrict__ counts) {
  __shared__ int sm[kThreads / 64];
  __shared__ unsigned long long sU[kThreads / 64];
  const int64_t tile = blockIdx.x;
  const int64_t i0 = tile * kTile + (int64_t)threadIdx.x * kPer;
  unsigned k[kPer];
  unsigned l[kPer];
  if (i0 + kPer <= R) {
    const uint4 a = reinterpret_cast<const uint4*>(skeys + i0)[0], b = reinterpret_cast<const uint4*>(skeys + i0)[1];
    k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w, k[4] = b.x, k[5] = b.y, k[6] = b.z, k[7] = b.w;
    const uint2 p = *reinterpret_cast<const uint2*>(slab + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l[j] = (p.x >> (8 * j)) & 0xffu;
      l[4 + j] = (p.y >> (8 * j)) & 0xffu;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const bool in = i0 + j < R;
      k[j] = in ? skeys[i0 + j] : 0u;
      l[j] = in ? slab[i0 + j] : 0u;
    }
  }
  // the neighbours across the thread's (and the tile's) edges come from memory
  const unsigned kprev = (i0 > 0 && i0 - 1 < R) ? skeys[i0 - 1] : 0u;
  const unsigned knext = (i0 + kPer < R) ? skeys[i0 + kPer] : 0u;
  bool in[kPer], head[kPer], tail[kPer];
  int neg[kPer], nthr = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = i0 + j;
    in[j] = i < R;
    head[j] = in[j] && (i == 0 || (j == 0 ? kprev : k[j - 1]) != k[j]);
    tail[j] = in[j] && (i == R - 1 || (j == kPer - 1 ? knext : k[j + 1]) != k[j]);
    neg[j] = (in[j] && l[j] == 0u) ? 1 : 0;
    nthr += neg[j];
  }
  int tile_neg;
  const int base = block_scan_excl<kThreads, false>(nthr, Sum(), 0, sm, tile_neg);
  // tile-local counts: cx = negatives before row j, cx + neg[j] = up to and including it
  int cx[kPer], hthr = kNone, tthr = INT_MAX;
  {
    int c = base;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      cx[j] = c;
      c += neg[j];
      if (head[j]) hthr = cx[j];                      // the last head's (cx is non-decreasing)
      if (tail[j] && tthr == INT_MAX) tthr = c;       // the first tail's
    }
  }
  int tile_h, tile_t;
  const int pre_h = block_scan_excl<kThreads, false>(hthr, Max(), kNone, sm, tile_h);
  const int pre_t = block_scan_excl<kThreads, true>(tthr, Min(), INT_MAX, sm, tile_t);
  if (!APPLY) {
    if (threadIdx.x == 0) {
      ta.neg[tile] = tile_neg;
      ta.head[tile] = tile_h;
      ta.tail[tile] = tile_t;
    }
    return;
  }
  const int off = ta.negoff[tile], ch = ta.carry_h[tile], ct = ta.carry_t[tile];
  int hv[kPer];
  {
    int run = pre_h;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (head[j]) run = cx[j];
      hv[j] = run == kNone ? ch : off + run;
    }
  }
  unsigned long long u2 = 0ull;
  {
    int run = pre_t;
#pragma unroll
    for (int j = kPer - 1; j >= 0; --j) {
      if (tail[j]) run = cx[j] + neg[j];
      const int tv = run == INT_MAX ? ct : off + run;
      if (in[j] && l[j] != 0u) u2 += (unsigned long long)hv[j] + (unsigned long long)tv;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u2 += __shfl_xor(u2, o, 64);
  if ((threadIdx.x & 63) == 0) sU[threadIdx.x >> 6] = u2;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long u = 0ull;
    for (int w = 0; w < kThreads / 64; ++w) u += sU[w];
    if (u) atomicAdd(&counts[2], u);  // the one same-address atomic of the workgroup (they serialise at the L2)
  }
}

// One workgroup over the tiles (R / 2048 of them): negoff = exclusive sum of the tiles' negatives;
// carry_h[t] = the global exclusive count at the last group head before tile t (forward max-scan);
// carry_t[t] = the global inclusive count at the first group tail after tile t (backward min-scan).
// Row 0 is a head and row R - 1 a tail, so a row that needs a carry always finds one.
__global__ __launch_bounds__(1024) void be_carry_k(TileArrays ta, int64_t tiles, int64_t R,
                                                   const double* __restrict__ lpart, int nlpart,
                                                   unsigned long long* __restrict__ counts,
                                                   double* __restrict__ loss_sum) {
  __shared__ int sm[16];
  __shared__ double sPart[64];
  const int tid = threadIdx.x;
  int carry = 0, tot;
  for (int64_t b = 0; b < tiles; b += 1024) {
    const int64_t t = b + tid;
    const int v = t < tiles ? ta.neg[t] : 0;
    const int e = block_scan_excl<1024, false>(v, Sum(), 0, sm, tot);
    if (t < tiles) ta.negoff[t] = carry + e;
    carry += tot;
  }
  if (tid == 0) {  // every row is a positive (label 1) or a negative; U2 is added to by the last pass
    counts[0] = (unsigned long long)(R - carry);
    counts[1] = (unsigned long long)carry;
    counts[2] = 0ull;
  }
  __syncthreads();  // negoff is read below by other threads
  carry = kNone;
  for (int64_t b = 0; b < tiles; b += 1024) {
    const int64_t t = b + tid;
    const int h = t < tiles ? ta.head[t] : kNone;
    const int v = h == kNone ? kNone : ta.negoff[t] + h;
    const int e = block_scan_excl<1024, false>(v, Max(), kNone, sm, tot);
    if (t < tiles) ta.carry_h[t] = carry > e ? carry : e;
    carry = carry > tot ? carry : tot;
  }
  carry = INT_MAX;
  for (int64_t b = 0; b < tiles; b += 1024) {  // from the last tile down: thread 1023 holds the highest tile
    const int64_t t = tiles - 1 - b - (1023 - tid);
    const int x = t >= 0 ? ta.tail[t] : INT_MAX;
    const int v = x == INT_MAX ? INT_MAX : ta.negoff[t] + x;
    const int e = block_scan_excl<1024, true>(v, Min(), INT_MAX, sm, tot);
    if (t >= 0) ta.carry_t[t] = carry < e ? carry : e;
    carry = carry < tot ? carry : tot;
  }
  // the Logloss partials in a fixed two-level order (lane l its contiguous run, lane 0 the 64 sums)
  if (tid < 64) {
    const int per = (nlpart + 63) / 64;
    const int b0 = tid * per, b1 = b0 + per < nlpart ? b0 + per : nlpart;
    double acc = 0.0;
    for (int b = b0; b < b1; ++b) acc += lpart[b];
    sPart[tid] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int l = 0; l < 64; ++l) acc += sPart[l];
    loss_sum[0] = acc;
  }
}

struct BeLayout {
  int64_t keys, keys_o, lab, lab_o, neg, head, tail, negoff, carry_h, carry_t, lpart, temp, temp_bytes, total, tiles;
};

size_t sort_temp_bytes(int64_t R) {
  size_t s = 0;
  (void)sort_pairs(nullptr, s, nullptr, nullptr, nullptr, nullptr, R, nullptr);
  return s;
}

BeLayout be_layout(int64_t R) {
  BeLayout l;
  rsx::Bump bump{0, 256};
  l.tiles = (R + kTile - 1) / kTile;
  l.keys = bump.take(R * 4);
  l.keys_o = bump.take(R * 4);
  l.lab = bump.take(R);
  l.lab_o = bump.take(R);
  l.neg = bump.take(l.tiles * 4);
  l.head = bump.take(l.tiles * 4);
  l.tail = bump.take(l.tiles * 4);
  l.negoff = bump.take(l.tiles * 4);
  l.carry_h = bump.take(l.tiles * 4);
  l.carry_t = bump.take(l.tiles * 4);
  l.lpart = bump.take(kLossSlots * 8);
  // the library's sort picks its plan by size (one block, merge sort, radix passes), and a plan
  // for fewer rows could ask for more storage: take the largest request over R and the powers of
  // two below it, so that the total does not shrink where the plan changes (a guard, checked over
  // a sweep by tests/test_binary_eval_cpu.py, not a proof for every R)
  size_t tb = sort_temp_bytes(R);
  for (int64_t p = 1; p < R; p <<= 1) tb = std::max(tb, sort_temp_bytes(p));
  l.temp_bytes = (int64_t)tb;
  l.temp = bump.take(l.temp_bytes);
  l.total = bump.off;
  return l;
}

}  // namespace

RSX_API int64_t rsx_binary_eval_workspace_bytes(int64_t R) {
  if (R < 1 || R >= ((int64_t)1 << 31)) {
    rsx::set_error("%s: invalid argument: %s", __func__, "need 1 <= R < 2^31");
    return -1;
  }
  return be_layout(R).total;
}

RSX_API int rsx_binary_eval(const float* logit, const float* y, int64_t R, void* ws, int64_t ws_bytes, int64_t* counts,
                            double* loss_sum, int* flag, void* stream) {
  RSX_ARG(R >= 1 && R < ((int64_t)1 << 31), "need 1 <= R < 2^31");
  RSX_ARG(logit && y && ws && counts && loss_sum && flag, "null tensor");
  const BeLayout l = be_layout(R);
  RSX_ARG(ws_bytes >= l.total, "workspace too small (rsx_binary_eval_workspace_bytes)");
  RSX_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)logit & 3) == 0 && ((uintptr_t)y & 3) == 0 &&
              ((uintptr_t)counts & 7) == 0 && ((uintptr_t)loss_sum & 7) == 0,
          "misaligned pointer (workspace 16 bytes, counts / loss_sum 8)");
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(flag, 0, sizeof(int), st);
  const unsigned gk = (unsigned)std::min<int64_t>(l.tiles, kLossSlots);
  const bool vec = (((uintptr_t)logit | (uintptr_t)y) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(be_key_k<true>, dim3(gk), dim3(kThreads), 0, st, logit, y, R, l.tiles,
                       at<unsigned>(ws, l.keys), at<uint8_t>(ws, l.lab), at<double>(ws, l.lpart), flag);
  else
    hipLaunchKernelGGL(be_key_k<false>, dim3(gk), dim3(kThreads), 0, st, logit, y, R, l.tiles,
                       at<unsigned>(ws, l.keys), at<uint8_t>(ws, l.lab), at<double>(ws, l.lpart), flag);
  RSX_LAUNCHED();
  size_t tb = (size_t)l.temp_bytes;
  const hipError_t se = sort_pairs(at<void>(ws, l.temp), tb, at<unsigned>(ws, l.keys), at<unsigned>(ws, l.keys_o),
                                   at<uint8_t>(ws, l.lab), at<uint8_t>(ws, l.lab_o), R, st);
  if (se != hipSuccess) {
    rsx::set_error("%s: sort failed: %s", __func__, hipGetErrorString(se));
    return (int)se;
  }
  RSX_LAUNCHED();
  TileArrays ta{at<int>(ws, l.neg),    at<int>(ws, l.head),    at<int>(ws, l.tail),
                at<int>(ws, l.negoff), at<int>(ws, l.carry_h), at<int>(ws, l.carry_t)};
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(be_tile_k<false>, dim3((unsigned)l.tiles), dim3(kThreads), 0, st, at<unsigned>(ws, l.keys_o),
                     at<uint8_t>(ws, l.lab_o), R, ta, cnt);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(be_carry_k, dim3(1), dim3(1024), 0, st, ta, l.tiles, R, at<double>(ws, l.lpart), (int)gk, cnt,
                     loss_sum);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(be_tile_k<true>, dim3((unsigned)l.tiles), dim3(kThreads), 0, st, at<unsigned>(ws, l.keys_o),
                     at<uint8_t>(ws, l.lab_o), R, ta, cnt);
  RSX_LAUNCHED();
  return 0;
}
