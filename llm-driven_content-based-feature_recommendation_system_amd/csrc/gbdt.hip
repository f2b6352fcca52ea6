// Oblivious-tree gradient boosting (Logloss) on the device: the reference's rerank stage is a CatBoost
// classifier of 1000 symmetric trees of depth 6 (temp_model/ranker_skelet.py:95-149) and CatBoost's GPU
// trainer is CUDA-only. The model is specified in include/recsys_amd.h ("oblivious-tree boosting") and
// restated in float64 / int64 numpy by tests/gbdt_ref.py.
//
// Everything that is summed is an integer. Gradients and hessians are quantised once per tree to
// llrint(x 2^30), which fits an int32 (|g| <= 1, 0 <= h <= 1/4); a histogram cell is an int64 sum of
// them, so a sum does not depend on the order of its terms and every run gives the same bits:
//   hist_k        one workgroup per (row slab, feature): the feature's [leaf][bin][{g, h}] cells live in
//                 LDS (n_leaves x 4 KiB: 128 KiB at level 5, one workgroup per CU there), rows add with
//                 64-bit LDS integer atomics, and the non-zero cells merge with 64-bit global integer atomics;
//   split_feature_k  one workgroup per feature, one thread per bin: per leaf a reversed workgroup scan
//                 (rsx_block.h) gives the sums of the bins above b, the score is summed over the leaves in
//                 fp64, and a scan over "the better of" picks the feature's first best bin;
//   split_pick_k  the first best of the <= 32 features;
//   leaf_value_k  (last level) one workgroup per parent leaf: the children's sums from that level's
//                 histogram along the chosen split, and their values;
//   apply_k       leaf = 2 leaf + right per row, and at the last level F += value[leaf];
//   predict_k     one row per lane, the row's bins in LDS, the trees staged through LDS kTreeChunk at a time.
// Splits never leave the device: apply_k and predict_k read them from memory.
// rsx_gbdt_tree_grouped runs the same levels on the QuerySoftMax gradients of gbdt_rank.hip.
#include "rsx_block.h"
#include "rsx_common.h"
#include "rsx_pair_cols.h"

namespace {

using rsx::block_scan_excl;

constexpr int kThreads = 256;
constexpr int kBins = 256;          // cells per (leaf, feature)
constexpr int kMaxFeatures = 32;
constexpr int kMaxDepth = 6;
constexpr int kLeafStride = 64;     // leaf values per tree (2^kMaxDepth)
constexpr int kTreeChunk = 64;      // trees staged in LDS at a time by predict_k
constexpr int64_t kSlabRows = 8192; // fewest rows a histogram workgroup takes (but for the last slab)
constexpr double kInvScale = 1.0 / 1073741824.0;  // 2^-30

// ---- gradients --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grad_k(const float* __restrict__ F, const float* __restrict__ y, int64_t R,
                                                   int* __restrict__ qg, int* __restrict__ qh) {
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += (int64_t)gridDim.x * kThreads) {
    // the sigmoid in fp64, rounded once: the float64 oracle then reproduces p, and with it g and h, bit for bit
    const float p = (float)(1.0 / (1.0 + exp(-(double)F[r])));
    const float g = y[r] - p, h = p * (1.0f - p);
    qg[r] = (int)llrintf(g * 1073741824.0f);   // a power of two: the product is exact, llrintf rounds half to even
    qh[r] = (int)llrintf(h * 1073741824.0f);
  }
}

// ---- histogram ----------------------------------------------------------------------------------------
template <int NL>
__global__ __launch_bounds__(kThreads) void hist_k(const uint8_t* __restrict__ bins, const uint8_t* __restrict__ leaf,
                                                   const int* __restrict__ qg, const int* __restrict__ qh, int64_t R,
                                                   int64_t slab_rows, int F, unsigned long long* __restrict__ hist,
                                                   int* __restrict__ flag) {
  __shared__ unsigned long long sh[NL * kBins * 2];
  const int f = blockIdx.y;
  for (int i = threadIdx.x; i < NL * kBins * 2; i += kThreads) sh[i] = 0ull;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < R ? r0 + slab_rows : R;
  const uint8_t* bf = bins + (int64_t)f * R;
  bool bad = false;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const unsigned l = leaf[r];
    if (l >= (unsigned)NL) {
      bad = true;
      continue;
    }
    const unsigned cell = (l * kBins + bf[r]) * 2;
    atomicAdd(&sh[cell], (unsigned long long)(long long)qg[r]);
    atomicAdd(&sh[cell + 1], (unsigned long long)(long long)qh[r]);
  }
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  for (int i = threadIdx.x; i < NL * kBins * 2; i += kThreads) {
    const unsigned long long v = sh[i];
    if (v != 0ull) {
      const int l = i / (kBins * 2), rem = i % (kBins * 2);
      atomicAdd(&hist[((int64_t)l * F + f) * (kBins * 2) + rem], v);
    }
  }
}

// ---- split search -------------------------------------------------------------------------------------
struct GH {
  long long g, h;
};
struct AddGH {
  __device__ __forceinline__ GH operator()(GH a, GH b) const { return GH{a.g + b.g, a.h + b.h}; }
};
struct Best {
  double s;
  int b, f;
};
struct Better {  // the earlier one stays unless the later one is strictly better: ties go to the lower index
  __device__ __forceinline__ Best operator()(Best a, Best b) const { return b.s > a.s ? b : a; }
};

__device__ __forceinline__ double side_score(GH s, double l2) {
  const double g = (double)s.g * kInvScale, h = (double)s.h * kInvScale;
  return g * g / (h + l2);
}

__global__ __launch_bounds__(kThreads) void split_feature_k(const long long* __restrict__ hist,
                                                            const uint8_t* __restrict__ is_cat,
                                                            const int* __restrict__ n_bins, int F, int NL, double l2,
                                                            Best* __restrict__ best) {
  __shared__ GH smg[kThreads / 64];
  __shared__ Best smb[kThreads / 64];
  const int f = blockIdx.x, b = threadIdx.x;
  const bool cat = is_cat[f] != 0;
  const int nb = n_bins[f];
  double score = 0.0;
  for (int l = 0; l < NL; ++l) {
    const long long* p = hist + ((int64_t)l * F + f) * (kBins * 2) + b * 2;
    const GH x{p[0], p[1]};
    GH tot;
    const GH above = block_scan_excl<kThreads, true>(x, AddGH(), GH{0, 0}, smg, tot);
    const GH right = cat ? x : above;
    const GH left{tot.g - right.g, tot.h - right.h};
    score += side_score(left, l2) + side_score(right, l2);
  }
  const double ninf = -__builtin_huge_val();
  Best mine{b < nb ? score : ninf, b, f};
  Best tot;
  block_scan_excl<kThreads, false>(mine, Better(), Best{ninf, 0, f}, smb, tot);
  if (threadIdx.x == 0) best[f] = tot;
}

__global__ void split_pick_k(const Best* __restrict__ best, int F, int* __restrict__ split, double* __restrict__ score) {
  if (threadIdx.x != 0) return;
  Best top = best[0];
  for (int f = 1; f < F; ++f) top = Better()(top, best[f]);
  split[0] = top.f;
  split[1] = top.b;
  if (score != nullptr) *score = top.s;
}

// ---- leaf values (last level) and the row update --------------------------------------------------------
__global__ __launch_bounds__(kThreads) void leaf_value_k(const long long* __restrict__ hist, const int* __restrict__ split,
                                                         const uint8_t* __restrict__ is_cat, int F, double lr, double l2,
                                                         long long* __restrict__ leaf_sums, float* __restrict__ leaf_values) {
  __shared__ GH smg[kThreads / 64];
  const int l = blockIdx.x, b = threadIdx.x;
  int f = split[0];
  if ((unsigned)f >= (unsigned)F) f = 0;    // apply_k raises the flag
  const int sb = split[1];
  const bool cat = is_cat[f] != 0;
  const long long* p = hist + ((int64_t)l * F + f) * (kBins * 2) + b * 2;
  const GH x{p[0], p[1]};
  GH tot;
  const GH above = block_scan_excl<kThreads, true>(x, AddGH(), GH{0, 0}, smg, tot);
  if (b != (sb & (kBins - 1))) return;
  const GH right = cat ? x : above;
  const GH side[2] = {GH{tot.g - right.g, tot.h - right.h}, right};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    leaf_sums[(2 * l + c) * 2] = side[c].g;
    leaf_sums[(2 * l + c) * 2 + 1] = side[c].h;
    const double g = (double)side[c].g * kInvScale, h = (double)side[c].h * kInvScale;
    leaf_values[2 * l + c] = (float)(lr * (g / (h + l2)));
  }
}

__global__ __launch_bounds__(kThreads) void apply_k(const uint8_t* __restrict__ bins, int64_t R, int F,
                                                    const int* __restrict__ split, const uint8_t* __restrict__ is_cat,
                                                    int NL, uint8_t* __restrict__ leaf,
                                                    const float* __restrict__ leaf_values, float* __restrict__ Fx,
                                                    int* __restrict__ flag) {
  int f = split[0];
  const unsigned sb = (unsigned)split[1];
  bool bad = false;
  if ((unsigned)f >= (unsigned)F) {
    bad = true;
    f = 0;
  }
  const bool cat = is_cat[f] != 0;
  const uint8_t* bf = bins + (int64_t)f * R;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < R; r += (int64_t)gridDim.x * kThreads) {
    const unsigned bin = bf[r];
    unsigned l = leaf[r];
    if (l >= (unsigned)NL) {
      bad = true;
      l &= (unsigned)(NL - 1);
    }
    l = 2 * l + (unsigned)(cat ? bin == sb : bin > sb);
    leaf[r] = (uint8_t)l;
    if (leaf_values != nullptr) Fx[r] += leaf_values[l];
  }
  if (bad) atomicOr(flag, 2);
}

// ---- prediction ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void predict_k(const uint8_t* __restrict__ bins, int64_t R, int F,
                                                      const int* __restrict__ splits, const float* __restrict__ values,
                                                      const uint8_t* __restrict__ is_cat, int depth, int t0, int t1,
                                                      const float* init, float f0, float* out) {
  __shared__ uint8_t rb[kMaxFeatures * kThreads];   // [feature][thread]: the rows' bins
  __shared__ int sp[kTreeChunk * kMaxDepth];        // feature | bin << 8 | categorical << 16
  __shared__ float sv[kTreeChunk * kLeafStride];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kThreads + tid;
  const bool live = r < R;
  for (int f = 0; f < F; ++f) rb[f * kThreads + tid] = live ? bins[(int64_t)f * R + r] : (uint8_t)0;
  float acc = live ? (init != nullptr ? init[r] : f0) : 0.0f;
  for (int c = t0; c < t1; c += kTreeChunk) {
    const int n = t1 - c < kTreeChunk ? t1 - c : kTreeChunk;
    __syncthreads();
    for (int i = tid; i < n * kMaxDepth; i += kThreads) {
      const int* s = splits + ((int64_t)c * kMaxDepth + i) * 2;
      int f = s[0];
      if ((unsigned)f >= (unsigned)F) f = 0;
      sp[i] = f | (s[1] & 255) << 8 | (is_cat[f] != 0 ? 1 << 16 : 0);
    }
    for (int i = tid; i < n * kLeafStride; i += kThreads) sv[i] = values[(int64_t)c * kLeafStride + i];
    __syncthreads();
    for (int t = 0; t < n; ++t) {
      unsigned l = 0;
      for (int d = 0; d < depth; ++d) {
        const int w = sp[t * kMaxDepth + d];
        const unsigned bin = rb[(w & 255) * kThreads + tid], sb = (unsigned)(w >> 8) & 255u;
        l = 2 * l + (unsigned)((w >> 16) != 0 ? bin == sb : bin > sb);
      }
      acc += sv[t * kLeafStride + l];
    }
  }
  if (live) out[r] = acc;
}

// ---- numeric columns -> bins ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bin_k(const float* __restrict__ x, const float* __restrict__ borders,
                                                  const int* __restrict__ n_borders, int64_t R, uint8_t* __restrict__ bins) {
  __shared__ float sb[kBins];
  const int j = blockIdx.y;
  sb[threadIdx.x] = borders[j * kBins + threadIdx.x];
  int n = n_borders[j];
  n = n < 0 ? 0 : (n > kBins - 1 ? kBins - 1 : n);
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  const float v = x[(int64_t)j * R + r];
  int lo = 0, hi = n;    // #{borders < v}: the first index whose border is not below v (NaN: none is, bin 0)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < v) lo = mid + 1; else hi = mid;
  }
  bins[(int64_t)j * R + r] = (uint8_t)lo;
}

// ---- the FeatureEngineer numeric columns of [Q, K] candidates ---------------------------------------------
__global__ __launch_bounds__(kThreads) void rerank_k(const int64_t* __restrict__ cand, const float* __restrict__ score,
                                                     const float* __restrict__ U, const float* __restrict__ V,
                                                     const float* __restrict__ price, const float* __restrict__ avg,
                                                     int64_t R, int64_t K, int64_t N, int d, float* __restrict__ feats,
                                                     int64_t* __restrict__ ids, int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (c >= R) return;    // whole waves leave: nothing below meets a barrier
  const int64_t q = c / K;
  int64_t id = cand[c];
  if (id < 0 || id >= N) {
    if (lane == 0) atomicOr(flag, 1);
    id = 0;
  }
  rsx::pair_columns(U + q * d, V + id * d, d, lane, price + id, avg + q, feats, R, c);   // columns 1..6
  if (lane != 0) return;
  feats[c] = score[c];
  ids[c] = id;
}

// ---- launches ------------------------------------------------------------------------------------------
unsigned row_grid(int64_t R) {
  const int64_t want = (R + kThreads - 1) / kThreads, cap = (int64_t)rsx::cu_count() * 16;
  return (unsigned)(want < cap ? want : cap);
}

bool pow2_leaves(int n) { return n >= 1 && n <= 32 && (n & (n - 1)) == 0; }

void launch_grad(const float* F, const float* y, int64_t R, int* qg, int* qh, hipStream_t st) {
  hipLaunchKernelGGL(grad_k, dim3(row_grid(R)), dim3(kThreads), 0, st, F, y, R, qg, qh);
}

int64_t hist_slabs(int64_t R, int F) {
  const int64_t want = (R + kSlabRows - 1) / kSlabRows;
  int64_t cap = (int64_t)rsx::cu_count() * 4 / F;
  if (cap < 1) cap = 1;
  return want < cap ? want : cap;
}

template <int NL>
void launch_hist_nl(const uint8_t* bins, const uint8_t* leaf, const int* qg, const int* qh, int64_t R, int F, int64_t* hist,
                    int* flag, hipStream_t st) {
  const int64_t slabs = hist_slabs(R, F), slab_rows = (R + slabs - 1) / slabs;
  hipLaunchKernelGGL(hist_k<NL>, dim3((unsigned)slabs, (unsigned)F), dim3(kThreads), 0, st, bins, leaf, qg, qh, R, slab_rows,
                     F, reinterpret_cast<unsigned long long*>(hist), flag);
}

void launch_hist(const uint8_t* bins, const uint8_t* leaf, const int* qg, const int* qh, int64_t R, int F, int NL,
                 int64_t* hist, int* flag, hipStream_t st) {
  (void)hipMemsetAsync(hist, 0, (size_t)NL * F * kBins * 2 * sizeof(int64_t), st);
  switch (NL) {
    case 1: launch_hist_nl<1>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
    case 2: launch_hist_nl<2>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
    case 4: launch_hist_nl<4>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
    case 8: launch_hist_nl<8>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
    case 16: launch_hist_nl<16>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
    default: launch_hist_nl<32>(bins, leaf, qg, qh, R, F, hist, flag, st); break;
  }
}

void launch_split(const int64_t* hist, const uint8_t* is_cat, const int* n_bins, int F, int NL, double l2, void* ws,
                  int* split, double* score, hipStream_t st) {
  Best* best = reinterpret_cast<Best*>(ws);
  hipLaunchKernelGGL(split_feature_k, dim3((unsigned)F), dim3(kThreads), 0, st, reinterpret_cast<const long long*>(hist),
                     is_cat, n_bins, F, NL, l2, best);
  hipLaunchKernelGGL(split_pick_k, dim3(1), dim3(64), 0, st, best, F, split, score);
}

void launch_apply(const uint8_t* bins, int64_t R, int F, const int* split, const uint8_t* is_cat, int NL, uint8_t* leaf,
                  const int64_t* hist, double lr, double l2, int64_t* leaf_sums, float* leaf_values, float* Fx, int* flag,
                  hipStream_t st) {
  if (hist != nullptr)
    hipLaunchKernelGGL(leaf_value_k, dim3((unsigned)NL), dim3(kThreads), 0, st, reinterpret_cast<const long long*>(hist), split,
                       is_cat, F, lr, l2, reinterpret_cast<long long*>(leaf_sums), leaf_values);
  hipLaunchKernelGGL(apply_k, dim3(row_grid(R)), dim3(kThreads), 0, st, bins, R, F, split, is_cat, NL, leaf,
                     hist != nullptr ? leaf_values : nullptr, Fx, flag);
}

// A tree's levels on the gradients qg / qh already written: what rsx_gbdt_tree and rsx_gbdt_tree_grouped share.
void launch_levels(const uint8_t* bins, int64_t R, int F, const uint8_t* is_cat, const int* n_bins, int depth, double lr,
                   double l2, float* Fx, const int* qg, const int* qh, uint8_t* leaf, int64_t* hist, void* ws, int* splits,
                   int64_t* leaf_sums, float* leaf_values, int* flag, hipStream_t st) {
  (void)hipMemsetAsync(leaf, 0, (size_t)R, st);
  for (int d = 0; d < depth; ++d) {
    const int NL = 1 << d;
    const bool last = d == depth - 1;
    launch_hist(bins, leaf, qg, qh, R, F, NL, hist, flag, st);
    launch_split(hist, is_cat, n_bins, F, NL, l2, ws, splits + 2 * d, nullptr, st);
    launch_apply(bins, R, F, splits + 2 * d, is_cat, NL, leaf, last ? hist : nullptr, lr, l2, leaf_sums, leaf_values, Fx, flag,
                 st);
  }
}

}  // namespace

RSX_API int64_t rsx_gbdt_tree_chunk(void) { return kTreeChunk; }

RSX_API int64_t rsx_gbdt_histogram_slabs(int64_t R, int F) {
  if (R < 1 || R >= (1ll << 31) || F < 1 || F > kMaxFeatures) {
    rsx::set_error("rsx_gbdt_histogram_slabs: need 1 <= R < 2^31 and 1 <= F <= 32");
    return -1;
  }
  return hist_slabs(R, F);
}

RSX_API int rsx_gbdt_bin(const float* x, const float* borders, const int* n_borders, int64_t R, int Fn, uint8_t* bins,
                         void* stream) {
  RSX_ARG(x && borders && n_borders && bins, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(Fn >= 1 && Fn <= kMaxFeatures, "need 1 <= Fn <= 32");
  hipLaunchKernelGGL(bin_k, dim3((unsigned)((R + kThreads - 1) / kThreads), (unsigned)Fn), dim3(kThreads), 0,
                     (hipStream_t)stream, x, borders, n_borders, R, bins);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_grad(const float* F, const float* y, int64_t R, int* qg, int* qh, void* stream) {
  RSX_ARG(F && y && qg && qh, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  launch_grad(F, y, R, qg, qh, (hipStream_t)stream);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_histogram(const uint8_t* bins, const uint8_t* leaf, const int* qg, const int* qh, int64_t R, int F,
                               int n_leaves, int64_t* hist, int* flag, void* stream) {
  RSX_ARG(bins && leaf && qg && qh && hist && flag, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(pow2_leaves(n_leaves), "n_leaves must be 1, 2, 4, 8, 16 or 32");
  launch_hist(bins, leaf, qg, qh, R, F, n_leaves, hist, flag, (hipStream_t)stream);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_best_split(const int64_t* hist, const uint8_t* is_cat, const int* n_bins, int F, int n_leaves, double l2,
                                void* ws, int* split, double* score, void* stream) {
  RSX_ARG(hist && is_cat && n_bins && ws && split, "null tensor");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(pow2_leaves(n_leaves), "n_leaves must be 1, 2, 4, 8, 16 or 32");
  RSX_ARG(l2 > 0.0, "l2 must be positive");
  RSX_ARG(rsx::aligned16(ws), "ws must be 16-byte aligned");
  launch_split(hist, is_cat, n_bins, F, n_leaves, l2, ws, split, score, (hipStream_t)stream);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_apply_split(const uint8_t* bins, int64_t R, int F, const int* split, const uint8_t* is_cat, int n_leaves,
                                 uint8_t* leaf, const int64_t* hist, double lr, double l2, int64_t* leaf_sums,
                                 float* leaf_values, float* Fx, int* flag, void* stream) {
  RSX_ARG(bins && split && is_cat && leaf && flag, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(pow2_leaves(n_leaves), "n_leaves must be 1, 2, 4, 8, 16 or 32");
  if (hist != nullptr) {
    RSX_ARG(leaf_sums && leaf_values && Fx, "the last level needs leaf_sums, leaf_values and F");
    RSX_ARG(l2 > 0.0, "l2 must be positive");
  }
  launch_apply(bins, R, F, split, is_cat, n_leaves, leaf, hist, lr, l2, leaf_sums, leaf_values, Fx, flag, (hipStream_t)stream);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_tree(const uint8_t* bins, const float* y, int64_t R, int F, const uint8_t* is_cat, const int* n_bins,
                          int depth, double lr, double l2, float* Fx, int* qg, int* qh, uint8_t* leaf, int64_t* hist, void* ws,
                          int* splits, int64_t* leaf_sums, float* leaf_values, int* flag, void* stream) {
  RSX_ARG(bins && y && is_cat && n_bins && Fx && qg && qh && leaf && hist && ws && splits && leaf_sums && leaf_values && flag,
          "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(l2 > 0.0, "l2 must be positive");
  RSX_ARG(rsx::aligned16(ws), "ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  launch_grad(Fx, y, R, qg, qh, st);
  launch_levels(bins, R, F, is_cat, n_bins, depth, lr, l2, Fx, qg, qh, leaf, hist, ws, splits, leaf_sums, leaf_values, flag, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_tree_grouped(const uint8_t* bins, const float* y, const int* row_group, const int* goff, int64_t R,
                                  int64_t G, int F, const uint8_t* is_cat, const int* n_bins, int depth, double lr, double l2,
                                  float* Fx, int* qg, int* qh, uint8_t* leaf, int64_t* hist, void* ws, void* group_ws,
                                  int64_t group_ws_bytes, int* splits, int64_t* leaf_sums, float* leaf_values, int* flag,
                                  void* stream) {
  RSX_ARG(bins && y && row_group && goff && is_cat && n_bins && Fx && qg && qh && leaf && hist && ws && group_ws && splits &&
              leaf_sums && leaf_values && flag,
          "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(G >= 1 && G <= R, "need 1 <= G <= R");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(l2 > 0.0, "l2 must be positive");
  RSX_ARG(rsx::aligned16(ws) && rsx::aligned16(group_ws), "ws and group_ws must be 16-byte aligned");
  RSX_ARG(group_ws_bytes >= rsx::gbdt_query_softmax_workspace(R, G),
          "group workspace too small (rsx_gbdt_grad_query_softmax_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  rsx::gbdt_query_softmax_launch(Fx, y, row_group, goff, R, (int)G, group_ws, qg, qh, st);
  launch_levels(bins, R, F, is_cat, n_bins, depth, lr, l2, Fx, qg, qh, leaf, hist, ws, splits, leaf_sums, leaf_values, flag, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_predict(const uint8_t* bins, int64_t R, int F, const int* splits, const float* leaf_values,
                             const uint8_t* is_cat, int depth, int tree_begin, int tree_end, const float* init, float f0,
                             float* out, void* stream) {
  RSX_ARG(bins && is_cat && out, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(tree_begin >= 0 && tree_begin <= tree_end, "need 0 <= tree_begin <= tree_end");
  RSX_ARG(tree_begin == tree_end || (splits && leaf_values), "null tensor");
  hipLaunchKernelGGL(predict_k, dim3((unsigned)((R + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, bins,
                     R, F, splits, leaf_values, is_cat, depth, tree_begin, tree_end, init, f0, out);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_rerank_tabular(const int64_t* cand, const float* score, const float* U, const float* V, const float* item_price,
                               const float* user_avg_price, int64_t Q, int64_t K, int64_t N, int64_t d, float* feats,
                               int64_t* ids, int* flag, void* stream) {
  RSX_ARG(cand && score && U && V && item_price && user_avg_price && feats && ids && flag, "null tensor");
  RSX_ARG(Q >= 1 && K >= 1 && Q * K < (1ll << 31), "need Q, K >= 1 and Q K < 2^31");
  RSX_ARG(N >= 1 && d >= 1 && d <= 65536, "need N >= 1 and 1 <= d <= 65536");
  const int64_t R = Q * K;
  hipLaunchKernelGGL(rerank_k, dim3((unsigned)((R + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0,
                     (hipStream_t)stream, cand, score, U, V, item_price, user_avg_price, R, K, N, (int)d, feats, ids, flag);
  RSX_LAUNCHED();
  return 0;
}
