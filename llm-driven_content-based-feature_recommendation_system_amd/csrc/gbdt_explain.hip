// Explaining the oblivious-tree ranker on the device: leaf weights, the per-tree table of conditional values,
// PredictionValuesChange and exact path-dependent Shapley values. The model is specified in
// include/recsys_amd.h ("explaining the boosted ranker") and restated in float64 numpy by
// tests/gbdt_explain_ref.py.
//   leaf_weights_k  one workgroup per slab of rows, one row per lane, the tile's bins in LDS as predict_k has
//                   them. The trees go kWeightChunk at a time: the chunk's [tree][64] int32 counters live in LDS,
//                   rows add with LDS integer atomics over all of the slab's tiles, and the non-zero cells merge
//                   into the int64 weights with 64-bit global integer atomics. Integer sums: the same bits every
//                   run and in any row order.
//   explain_plan_k  one workgroup per tree: the covers of the 127 nodes, then the table level by level from
//                   the leaves up (level d holds 2^d nodes x 3^(depth-d) suffix states; two LDS buffers swap),
//                   and one thread per level sums that level's PredictionValuesChange pairs in leaf order.
//   shap_k          the hot path: one row per lane, the row's bins in LDS, the trees staged through LDS
//                   kShapChunk at a time (packed splits, the levels each player owns, the players' features
//                   and the 729-entry table). A tree of m players costs 2^m table reads: the coalition S reads
//                   table[3^depth - 1 - sum_{j in S} delta_j], delta_j = sum over j's levels of (2 - r_d) 3^(depth-1-d),
//                   and v(S) enters every phi_j with +W(|S| - 1) (j in S) or -W(|S|). The masks are unrolled, so
//                   the coefficients are uniform scalars and phi_j are six registers indexed statically; the
//                   F + 1 running sums are LDS columns [feature][lane], where indexing by feature id is free.
//                   Every sum of a row runs in tree order on its lane: the bits do not depend on R, the grid
//                   or the chunking.
#include "rsx_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFeatures = 32;
constexpr int kMaxDepth = 6;
constexpr int kLeafStride = 64;
constexpr int kTable = 729;          // 3^kMaxDepth states per tree
constexpr int kShapChunk = 8;        // trees shap_k stages in LDS at a time (8 x 5,832 B of tables)
constexpr int kWeightChunk = 256;    // trees leaf_weights_k counts in LDS at a time (64 KiB of counters)
constexpr int64_t kSlabRows = 1024;  // fewest rows a leaf_weights_k workgroup takes (but for the last slab)

// W[m][s] = s! (m - s - 1)! / m!: the Shapley weight of a coalition of s of the other m - 1 players
__constant__ double kShapleyW[kMaxDepth + 1][kMaxDepth] = {
    {0, 0, 0, 0, 0, 0},
    {1.0, 0, 0, 0, 0, 0},
    {1.0 / 2, 1.0 / 2, 0, 0, 0, 0},
    {1.0 / 3, 1.0 / 6, 1.0 / 3, 0, 0, 0},
    {1.0 / 4, 1.0 / 12, 1.0 / 12, 1.0 / 4, 0, 0},
    {1.0 / 5, 1.0 / 20, 1.0 / 30, 1.0 / 20, 1.0 / 5, 0},
    {1.0 / 6, 1.0 / 30, 1.0 / 60, 1.0 / 60, 1.0 / 30, 1.0 / 6},
};

__device__ __forceinline__ int pow3(int n) {
  int p = 1;
  for (int i = 0; i < n; ++i) p *= 3;
  return p;
}

// feature | bin << 8 | categorical << 16 of a split, as predict_k packs it (a feature >= F reads as feature 0)
__device__ __forceinline__ int pack_split(const int* __restrict__ s, const uint8_t* __restrict__ is_cat, int F) {
  int f = s[0];
  if ((unsigned)f >= (unsigned)F) f = 0;
  return f | (s[1] & 255) << 8 | (is_cat[f] != 0 ? 1 << 16 : 0);
}

__device__ __forceinline__ unsigned go_right(int w, const uint8_t* rb, int tid) {
  const unsigned bin = rb[(w & 255) * kThreads + tid], sb = (unsigned)(w >> 8) & 255u;
  return (unsigned)((w >> 16) != 0 ? bin == sb : bin > sb);
}

// ---- leaf weights ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void leaf_weights_k(const uint8_t* __restrict__ bins, int64_t R, int64_t slab_rows,
                                                           int F, const int* __restrict__ splits,
                                                           const uint8_t* __restrict__ is_cat, int depth, int t0, int t1,
                                                           unsigned long long* __restrict__ weights) {
  __shared__ uint8_t rb[kMaxFeatures * kThreads];
  __shared__ int sp[kWeightChunk * kMaxDepth];
  __shared__ int cnt[kWeightChunk * kLeafStride];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < R ? r0 + slab_rows : R;
  for (int c = t0; c < t1; c += kWeightChunk) {
    const int n = t1 - c < kWeightChunk ? t1 - c : kWeightChunk;
    __syncthreads();      // the previous chunk's flush has read cnt
    for (int i = tid; i < n * kMaxDepth; i += kThreads) sp[i] = pack_split(splits + ((int64_t)c * kMaxDepth + i) * 2, is_cat, F);
    for (int i = tid; i < n * kLeafStride; i += kThreads) cnt[i] = 0;
    __syncthreads();
    for (int64_t r = r0 + tid; r < r1; r += kThreads) {
      // a lane reads only the bins it wrote itself: no barrier between the staging and the use
      for (int f = 0; f < F; ++f) rb[f * kThreads + tid] = bins[(int64_t)f * R + r];
      for (int t = 0; t < n; ++t) {
        unsigned l = 0;
        for (int d = 0; d < depth; ++d) l = 2 * l + go_right(sp[t * kMaxDepth + d], rb, tid);
        atomicAdd(&cnt[t * kLeafStride + l], 1);
      }
    }
    __syncthreads();
    for (int i = tid; i < n * kLeafStride; i += kThreads) {
      const int v = cnt[i];
      if (v != 0) atomicAdd(&weights[(int64_t)c * kLeafStride + i], (unsigned long long)v);
    }
  }
}

// ---- the table of conditional values and PredictionValuesChange ---------------------------------------------
__global__ __launch_bounds__(kThreads) void explain_plan_k(const float* __restrict__ values,
                                                           const long long* __restrict__ weights, int depth, int t0,
                                                           double* __restrict__ table, double* __restrict__ pvc) {
  __shared__ double cover[2 * kLeafStride];    // node n of level d at (1 << d) + n: a heap, the root at 1
  __shared__ double val[kLeafStride];
  __shared__ double buf[2][kTable];
  const int tid = threadIdx.x;
  const int64_t t = t0 + blockIdx.x;
  const int NL = 1 << depth;
  if (tid < NL) {
    cover[NL + tid] = (double)weights[t * kLeafStride + tid];   // below 2^31 rows: exact
    val[tid] = (double)values[t * kLeafStride + tid];
    buf[depth & 1][tid] = val[tid];
  }
  __syncthreads();
  for (int d = depth - 1; d >= 0; --d) {       // integers below 2^53: the sums are exact in any order
    if (tid < (1 << d)) cover[(1 << d) + tid] = cover[2 * ((1 << d) + tid)] + cover[2 * ((1 << d) + tid) + 1];
    __syncthreads();
  }
  // level d: buf[d & 1][n * 3^(depth-d) + suffix], suffix = the states of the levels d .. depth-1, s_d leading
  for (int d = depth - 1; d >= 0; --d) {
    const double* below = buf[(d + 1) & 1];
    double* here = buf[d & 1];
    const int sub = pow3(depth - 1 - d), width = 3 * sub;
    for (int i = tid; i < (1 << d) * width; i += kThreads) {
      const int n = i / width, s = (i % width) / sub, rest = i % sub;
      const double a = below[(2 * n) * sub + rest], b = below[(2 * n + 1) * sub + rest];
      double e;
      if (s == 0) {
        e = a;
      } else if (s == 1) {
        e = b;
      } else {
        const double c0 = cover[2 * ((1 << d) + n)], c1 = cover[2 * ((1 << d) + n) + 1];
        e = c0 + c1 > 0.0 ? (c0 * a + c1 * b) / (c0 + c1) : 0.5 * a + 0.5 * b;
      }
      here[i] = e;
    }
    __syncthreads();
  }
  const int n_states = pow3(depth);
  for (int i = tid; i < n_states; i += kThreads) table[t * kTable + i] = buf[0][i];
  if (tid < kMaxDepth) {
    double s = 0.0;
    if (tid < depth) {
      const int bit = 1 << (depth - 1 - tid);
      for (int l = 0; l < NL; ++l) {
        if (l & bit) continue;
        const double c1 = cover[NL + l], c2 = cover[NL + l + bit], dv = val[l] - val[l + bit];
        if (c1 + c2 > 0.0) s += c1 * c2 / (c1 + c2) * (dv * dv);
      }
    }
    pvc[t * kMaxDepth + tid] = s;
  }
}

// ---- Shapley values ---------------------------------------------------------------------------------------
// The masks [2^K, 2^(K+1)) of the coalitions whose highest player is K; the compiler unrolls both loops, so
// a mask's index is a fixed sum of the delta and its coefficients are two of the six uniform weights.
template <int K>
__device__ __forceinline__ void shap_masks(const double* __restrict__ tb, int full, const int (&delta)[kMaxDepth],
                                           const double (&w)[kMaxDepth], double (&phi)[kMaxDepth]) {
#pragma unroll
  for (int mask = 1 << K; mask < 2 << K; ++mask) {
    int idx = full, size = 0;
#pragma unroll
    for (int j = 0; j <= K; ++j)
      if (mask >> j & 1) {
        idx -= delta[j];
        ++size;
      }
    const double v = tb[idx];
#pragma unroll
    for (int j = 0; j < kMaxDepth; ++j) {
      if (mask >> j & 1)
        phi[j] += w[size - 1] * v;
      else if (size < kMaxDepth)
        phi[j] -= w[size] * v;
    }
  }
}

struct ShapTree {       // what a staged tree carries besides its table
  int sp[kMaxDepth];    // packed splits
  int own[kMaxDepth];   // own[j]: the levels player j owns, a bit mask (0 for j >= m)
  int feat[kMaxDepth];  // feat[j]: player j's feature
  int m;
};

__global__ __launch_bounds__(kThreads) void shap_k(const uint8_t* __restrict__ bins, int64_t R, int F,
                                                   const int* __restrict__ splits, const uint8_t* __restrict__ is_cat,
                                                   int depth, int t0, int t1, const double* __restrict__ table, double f0,
                                                   double* __restrict__ phi_out) {
  extern __shared__ double smem[];
  double* tb = smem;                                             // [kShapChunk][kTable]
  double* acc = tb + kShapChunk * kTable;                        // [F][lane]
  ShapTree* tree = reinterpret_cast<ShapTree*>(acc + F * kThreads);
  uint8_t* rb = reinterpret_cast<uint8_t*>(tree + kShapChunk);   // [F][lane]
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kThreads + tid;
  const bool live = r < R;
  for (int f = 0; f < F; ++f) {
    rb[f * kThreads + tid] = live ? bins[(int64_t)f * R + r] : (uint8_t)0;
    acc[f * kThreads + tid] = 0.0;
  }
  int p3[kMaxDepth];
#pragma unroll
  for (int d = 0; d < kMaxDepth; ++d) p3[d] = d < depth ? pow3(depth - 1 - d) : 0;
  const int full = pow3(depth) - 1;
  double expected = f0;
  for (int c = t0; c < t1; c += kShapChunk) {
    const int n = t1 - c < kShapChunk ? t1 - c : kShapChunk;
    __syncthreads();
    for (int i = tid; i < n * kTable; i += kThreads) tb[i] = table[(int64_t)c * kTable + i];
    if (tid < n) {      // one thread per tree names the players: the distinct features in level order
      ShapTree& s = tree[tid];      // filled in LDS, where indexing by a run-time player costs nothing
      int m = 0;
      for (int j = 0; j < kMaxDepth; ++j) s.own[j] = 0, s.feat[j] = 0;
      for (int d = 0; d < kMaxDepth; ++d) {
        s.sp[d] = 0;
        if (d >= depth) continue;
        const int w = pack_split(splits + ((int64_t)(c + tid) * kMaxDepth + d) * 2, is_cat, F);
        s.sp[d] = w;
        int j = 0;
        while (j < m && s.feat[j] != (w & 255)) ++j;
        if (j == m) s.feat[m++] = w & 255;
        s.own[j] |= 1 << d;
      }
      s.m = m;
    }
    __syncthreads();
    for (int t = 0; t < n; ++t) {
      const ShapTree& s = tree[t];
      const double* tt = tb + t * kTable;
      int term[kMaxDepth];      // (2 - r_d) 3^(depth-1-d): what level d takes off the index when its owner joins
#pragma unroll
      for (int d = 0; d < kMaxDepth; ++d) term[d] = d < depth ? (2 - (int)go_right(s.sp[d], rb, tid)) * p3[d] : 0;
      int delta[kMaxDepth];
#pragma unroll
      for (int j = 0; j < kMaxDepth; ++j) {
        const int own = s.own[j];
        int x = 0;
#pragma unroll
        for (int d = 0; d < kMaxDepth; ++d) x += (own >> d & 1) ? term[d] : 0;
        delta[j] = x;
      }
      const int m = s.m;
      double w[kMaxDepth];
#pragma unroll
      for (int i = 0; i < kMaxDepth; ++i) w[i] = kShapleyW[m][i];
      const double v0 = tt[full];     // the empty coalition: E(*, ..., *), the same for every row
      expected += v0;
      double phi[kMaxDepth];
#pragma unroll
      for (int j = 0; j < kMaxDepth; ++j) phi[j] = -(w[0] * v0);
      if (m > 0) shap_masks<0>(tt, full, delta, w, phi);
      if (m > 1) shap_masks<1>(tt, full, delta, w, phi);
      if (m > 2) shap_masks<2>(tt, full, delta, w, phi);
      if (m > 3) shap_masks<3>(tt, full, delta, w, phi);
      if (m > 4) shap_masks<4>(tt, full, delta, w, phi);
      if (m > 5) shap_masks<5>(tt, full, delta, w, phi);
#pragma unroll
      for (int j = 0; j < kMaxDepth; ++j)
        if (j < m) acc[s.feat[j] * kThreads + tid] += phi[j];
    }
  }
  if (!live) return;
  for (int f = 0; f < F; ++f) phi_out[(int64_t)f * R + r] = acc[f * kThreads + tid];
  phi_out[(int64_t)F * R + r] = expected;
}

size_t shap_lds_bytes(int F) {
  return (size_t)kShapChunk * kTable * sizeof(double) + (size_t)F * kThreads * sizeof(double) +
         (size_t)kShapChunk * sizeof(ShapTree) + (size_t)F * kThreads;
}

int64_t weight_slabs(int64_t R) {
  const int64_t want = (R + kSlabRows - 1) / kSlabRows, cap = (int64_t)rsx::cu_count() * 4;   // two resident a CU, two rounds
  return want < cap ? want : cap;
}

}  // namespace

RSX_API int64_t rsx_gbdt_shap_tree_chunk(void) { return kShapChunk; }

RSX_API int rsx_gbdt_leaf_weights(const uint8_t* bins, int64_t R, int F, const int* splits, const uint8_t* is_cat, int depth,
                                  int tree_begin, int tree_end, int64_t* weights, void* stream) {
  RSX_ARG(bins && is_cat, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(tree_begin >= 0 && tree_begin <= tree_end, "need 0 <= tree_begin <= tree_end");
  RSX_ARG(tree_begin == tree_end || (splits && weights), "null tensor");
  if (tree_begin == tree_end) return 0;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(weights + (int64_t)tree_begin * kLeafStride, 0,
                       (size_t)(tree_end - tree_begin) * kLeafStride * sizeof(int64_t), st);
  const int64_t slabs = weight_slabs(R);
  const int64_t slab_rows = (R + slabs - 1) / slabs;
  hipLaunchKernelGGL(leaf_weights_k, dim3((unsigned)((R + slab_rows - 1) / slab_rows)), dim3(kThreads), 0, st, bins, R,
                     slab_rows, F, splits, is_cat, depth, tree_begin, tree_end, reinterpret_cast<unsigned long long*>(weights));
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_explain_plan(const int* splits, const float* leaf_values, const int64_t* weights, int depth,
                                  int tree_begin, int tree_end, double* table, double* pvc, void* stream) {
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(tree_begin >= 0 && tree_begin <= tree_end, "need 0 <= tree_begin <= tree_end");
  RSX_ARG(tree_begin == tree_end || (splits && leaf_values && weights && table && pvc), "null tensor");
  if (tree_begin == tree_end) return 0;
  // the table and the level sums depend on the tree's leaves and weights alone: splits is not read
  hipLaunchKernelGGL(explain_plan_k, dim3((unsigned)(tree_end - tree_begin)), dim3(kThreads), 0, (hipStream_t)stream,
                     leaf_values, reinterpret_cast<const long long*>(weights), depth, tree_begin, table, pvc);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_shap(const uint8_t* bins, int64_t R, int F, const int* splits, const uint8_t* is_cat, int depth,
                          int tree_begin, int tree_end, const double* table, double f0, double* phi, void* stream) {
  RSX_ARG(bins && is_cat && phi, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(F >= 1 && F <= kMaxFeatures, "need 1 <= F <= 32");
  RSX_ARG(depth >= 1 && depth <= kMaxDepth, "need 1 <= depth <= 6");
  RSX_ARG(tree_begin >= 0 && tree_begin <= tree_end, "need 0 <= tree_begin <= tree_end");
  RSX_ARG(tree_begin == tree_end || (splits && table), "null tensor");
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(shap_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)shap_lds_bytes(F));
  if (e != hipSuccess) {
    rsx::set_error("rsx_gbdt_shap: cannot raise the LDS limit: %s", hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(shap_k, dim3((unsigned)((R + kThreads - 1) / kThreads)), dim3(kThreads), shap_lds_bytes(F),
                     (hipStream_t)stream, bins, R, F, splits, is_cat, depth, tree_begin, tree_end, table, f0, phi);
  RSX_LAUNCHED();
  return 0;
}
