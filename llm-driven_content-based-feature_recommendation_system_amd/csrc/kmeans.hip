// Deterministic k-means on a fixed-point grid (the clustering of reference staticstics/preprocess_clustering.py, which
// calls scikit-learn on the host). Specified in include/recsys_amd.h ("k-means") and restated in numpy on the same
// integers by tests/persona_ref.py.
//
// The data are q int32 [d, C], feature-major, standing for q 2^-frac_bits exactly. A cluster's sum is then an
// integer: the adds commute, so the centres, and with them the whole trajectory, are the same bits every run and
// in any row order. Floating point enters in three places, each in a fixed order: the squared distance (j ascending,
// the subtraction first, no contraction), the centre = (double)sum / ((double)count 2^frac_bits), and the shift of
// the centres (one thread, k outer, j inner). The only atomics are integer.
//   standardize_k   (x - mean) / scale per column; the moments are the two-level sums of rsx_colsum.h
//   quantize_k      q = rint(x 2^frac_bits)
//   seed_round_k    one round of k-means++ as an exponential race: dmin, key = dmin / -ln u, a candidate per workgroup
//   seed_pick_k     one workgroup picks among the candidates (and writes the first seed); seed_centres_k copies the rows
//   assign_k<KD, ACC>  one row per thread, the centres in LDS; ACC: int64 sums, counts and changed labels in LDS,
//                   flushed once per workgroup
//   finalize_k      one workgroup: the new centres, the shift, done, and the accumulators cleared
#include "rsx_colsum.h"
#include "rsx_common.h"

#include <limits.h>

// diff * diff + acc stays two roundings: the distance is specified that way
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxD = 32;
constexpr int kMaxK = 256;
constexpr int kMaxKD = 4096;
constexpr int kSmallKD = 512;      // up to here the centres and sums take 8 KB of LDS, not 64

__host__ __device__ inline int64_t tiles_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void moments_k(const double* __restrict__ sum, const double* __restrict__ ss, int d,
                                                      int64_t C, double* __restrict__ mean, double* __restrict__ var,
                                                      double* __restrict__ scale) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= d) return;
  const double m = sum[j] / (double)C, v = ss[j] / (double)C;
  // a constant column by scikit-learn's rule (_is_constant_feature): the variance is what rounding alone can leave
  const double eps = 2.220446049250313e-16, t = (double)C * m * eps;
  const bool constant = v <= (double)C * eps * v + t * t;
  mean[j] = m;
  var[j] = v;
  scale[j] = constant ? 1.0 : sqrt(v);
}

__global__ __launch_bounds__(kThreads) void standardize_k(const double* __restrict__ x, int64_t C, const double* __restrict__ mean,
                                                          const double* __restrict__ scale, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= C) return;
  const int j = blockIdx.y;
  out[j * C + i] = (x[j * C + i] - mean[j]) / scale[j];
}

__global__ __launch_bounds__(kThreads) void quantize_k(const double* __restrict__ x, int64_t n, double mul, int* __restrict__ q,
                                                       int* flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double v = rint(x[i] * mul);
  bool bad = false;
  if (v != v) {
    v = 0.0;
    bad = true;
  } else if (v > 2147483647.0) {
    v = 2147483647.0;
    bad = true;
  } else if (v < -2147483647.0) {
    v = -2147483647.0;
    bad = true;
  }
  if (bad) atomicOr(flag, 1);
  q[i] = (int)v;
}

// ---------------------------------------------------------------------------------------------------------
// seeding. A candidate: the key's bits (keys are >= 0 or +inf, so the bits order as the values) and the row.
struct Cand {
  unsigned long long key;
  int row;
};
__device__ __forceinline__ bool better(Cand a, Cand b) { return a.key > b.key || (a.key == b.key && a.row < b.row); }

__device__ __forceinline__ Cand block_best(Cand c, Cand* sm) {
  for (int o = 32; o > 0; o >>= 1) {
    Cand x;
    x.key = __shfl_xor(c.key, o, 64);
    x.row = __shfl_xor(c.row, o, 64);
    if (better(x, c)) c = x;
  }
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  Cand best = sm[0];
  for (int w = 1; w < kThreads / 64; ++w)
    if (better(sm[w], best)) best = sm[w];
  __syncthreads();
  return best;
}

__global__ __launch_bounds__(kThreads) void seed_round_k(const int* __restrict__ q, int d, int64_t C, double inv, uint64_t seed,
                                                         int round, const int* __restrict__ seeds, double* __restrict__ dmin,
                                                         Cand* __restrict__ cand, int* flag) {
  __shared__ Cand sm[kThreads / 64];
  int s = seeds[round - 1];
  if ((uint64_t)s >= (uint64_t)C) {      // cannot happen for seeds this file wrote
    if (threadIdx.x == 0) atomicOr(flag, 1);
    s = 0;
  }
  Cand best{0ull, INT_MAX};
  for (int64_t tile = blockIdx.x; tile < tiles_of(C); tile += gridDim.x) {
    const int64_t i = tile * kThreads + threadIdx.x;
    if (i >= C) continue;
    double acc = 0.0;
    for (int j = 0; j < d; ++j) {
      const double diff = (double)q[j * C + i] * inv - (double)q[j * C + s] * inv;
      acc = acc + diff * diff;
    }
    const double old = dmin[i];
    const double dm = round == 1 || acc < old ? acc : old;
    dmin[i] = dm;
    const double u = ((double)rsx::hash_u32(seed + (uint64_t)round, (uint64_t)i) + 0.5) * 2.3283064365386963e-10;
    const double key = dm / -log(u);
    const Cand c{(unsigned long long)__double_as_longlong(key), (int)i};
    if (better(c, best)) best = c;
  }
  best = block_best(best, sm);
  if (threadIdx.x == 0) cand[blockIdx.x] = best;
}

// round 0: seeds[0] = first; round r >= 1: seeds[r] = the best of the n candidates
__global__ __launch_bounds__(kThreads) void seed_pick_k(const Cand* __restrict__ cand, int n, int round, int first, int* seeds) {
  __shared__ Cand sm[kThreads / 64];
  if (round == 0) {
    if (threadIdx.x == 0) seeds[0] = first;
    return;
  }
  Cand best{0ull, INT_MAX};
  for (int u = threadIdx.x; u < n; u += kThreads)
    if (better(cand[u], best)) best = cand[u];
  best = block_best(best, sm);
  if (threadIdx.x == 0) seeds[round] = best.row;
}

__global__ __launch_bounds__(kThreads) void seed_centres_k(const int* __restrict__ q, int d, int64_t C, double inv, int K,
                                                           const int* __restrict__ seeds, double* __restrict__ centres, int* flag) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= K * d) return;
  const int k = s / d, j = s - k * d;
  int row = seeds[k];
  if ((uint64_t)row >= (uint64_t)C) {
    atomicOr(flag, 1);
    row = 0;
  }
  centres[s] = (double)q[j * C + row] * inv;
}

// ---------------------------------------------------------------------------------------------------------
// Lloyd. ctl: [0] rows whose label changed (accumulator), [1] done = the iteration that converged or 0,
// [2] the iterations run so far.
template <int KD, bool ACC>
__global__ __launch_bounds__(kThreads) void assign_k(const int* __restrict__ q, int d, int64_t C, double inv, int K,
                                                     const double* __restrict__ centres, int* __restrict__ labels,
                                                     double* __restrict__ dmin, unsigned long long* __restrict__ sum_q,
                                                     int* __restrict__ count, int* ctl) {
  __shared__ double c_sm[KD];
  __shared__ unsigned long long sum_sm[ACC ? KD : 1];
  __shared__ int cnt_sm[ACC ? kMaxK : 1];
  __shared__ int changed_sm;
  if (ACC && ctl[1]) return;      // converged in an earlier iteration: nothing more moves
  const int kd = K * d;
  for (int s = threadIdx.x; s < kd; s += kThreads) {
    c_sm[s] = centres[s];
    if (ACC) sum_sm[s] = 0ull;
  }
  if (ACC) {
    for (int k = threadIdx.x; k < K; k += kThreads) cnt_sm[k] = 0;
    if (threadIdx.x == 0) changed_sm = 0;
  }
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < tiles_of(C); tile += gridDim.x) {
    const int64_t i = tile * kThreads + threadIdx.x;
    if (i >= C) continue;
    int qi[kMaxD];
#pragma unroll
    for (int j = 0; j < kMaxD; ++j) qi[j] = j < d ? q[j * C + i] : 0;
    int best = 0;
    double best_d = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* c = c_sm + k * d;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxD; ++j) {
        if (j < d) {
          const double diff = (double)qi[j] * inv - c[j];
          acc = acc + diff * diff;
        }
      }
      if (k == 0 || acc < best_d) {      // the smallest k among the minima
        best = k;
        best_d = acc;
      }
    }
    if (ACC) {
      if (labels[i] != best) atomicAdd(&changed_sm, 1);
      atomicAdd(&cnt_sm[best], 1);
#pragma unroll
      for (int j = 0; j < kMaxD; ++j)
        if (j < d) atomicAdd(&sum_sm[best * d + j], (unsigned long long)(long long)qi[j]);
    }
    labels[i] = best;
    if (dmin) dmin[i] = best_d;
  }
  if (!ACC) return;
  __syncthreads();
  for (int s = threadIdx.x; s < kd; s += kThreads)
    if (sum_sm[s]) atomicAdd(&sum_q[s], sum_sm[s]);
  for (int k = threadIdx.x; k < K; k += kThreads)
    if (cnt_sm[k]) atomicAdd(&count[k], cnt_sm[k]);
  if (threadIdx.x == 0 && changed_sm) atomicAdd(&ctl[0], changed_sm);
}

__global__ __launch_bounds__(kThreads) void finalize_k(int d, int K, double grid, double tol_abs, int iteration,
                                                       double* __restrict__ centres, long long* __restrict__ sum_q,
                                                       int* __restrict__ count, int* ctl, double* shift) {
  __shared__ double d2[kMaxKD];
  if (ctl[1]) return;
  const int kd = K * d;
  for (int s = threadIdx.x; s < kd; s += kThreads) {
    const int n = count[s / d];
    const double old = centres[s];
    const double now = n > 0 ? (double)sum_q[s] / ((double)n * grid) : old;      // a cluster without rows keeps its centre
    const double diff = now - old;
    d2[s] = diff * diff;
    centres[s] = now;
    sum_q[s] = 0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kThreads) count[k] = 0;
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  for (int s = 0; s < kd; ++s) acc = acc + d2[s];
  *shift = acc;
  if (ctl[0] == 0 || acc <= tol_abs) ctl[1] = iteration;
  ctl[0] = 0;
  ctl[2] = iteration;
}

// rsx::hash_u32(seed, 0) on the host: the formula of rsx_common.h at index 0
uint32_t hash_u32_host(uint64_t seed) {
  uint32_t x = (uint32_t)seed;
  x ^= (uint32_t)(seed >> 32) * 0x85EBCA77u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

bool shape_ok(int64_t d, int64_t C, int64_t K) {
  return d >= 1 && d <= kMaxD && K >= 1 && K <= kMaxK && K * d <= kMaxKD && C >= 1 && C < (1ll << 31) && C * d < (1ll << 40);
}
#define KM_SHAPE_MSG "need 1 <= d <= 32, 1 <= K <= 256, K d <= 4096 and 1 <= C < 2^31 rows"

unsigned grid_of(int64_t C, int64_t max_workgroups) {
  const int64_t t = tiles_of(C);
  return (unsigned)(t < max_workgroups ? t : max_workgroups);
}

template <bool ACC>
void launch_assign(const int* q, int d, int64_t C, double inv, int K, const double* centres, int* labels, double* dmin,
                   int64_t* sum_q, int* count, int* ctl, int64_t max_workgroups, hipStream_t st) {
  const dim3 grid(grid_of(C, max_workgroups)), block(kThreads);
  auto* sums = reinterpret_cast<unsigned long long*>(sum_q);
  if (K * d <= kSmallKD)
    hipLaunchKernelGGL((assign_k<kSmallKD, ACC>), grid, block, 0, st, q, d, C, inv, K, centres, labels, dmin, sums, count, ctl);
  else
    hipLaunchKernelGGL((assign_k<kMaxKD, ACC>), grid, block, 0, st, q, d, C, inv, K, centres, labels, dmin, sums, count, ctl);
}

}  // namespace

RSX_API int rsx_standardize_columns(const double* x, int64_t d, int64_t C, double* ws, int64_t ws_doubles, double* out,
                                    double* mean, double* var, double* scale, void* stream) {
  RSX_ARG(x && mean && var && scale, "null tensor");
  RSX_ARG(d >= 1 && d <= 65535 && C >= 1 && C < (1ll << 31), "need 1 <= d <= 65535 columns of 1 <= C < 2^31 values");
  RSX_ARG(ws && ws_doubles >= 2 * d + d * rsx::col_chunks(C), "workspace too small ((2 + ceil(C / 4096)) d doubles)");
  hipStream_t st = (hipStream_t)stream;
  double *sum = ws, *ss = ws + d, *part = ws + 2 * d;
  rsx::col_sums<double>(x, C, (int)d, nullptr, part, sum, st);
  rsx::col_sums<double>(x, C, (int)d, sum, part, ss, st);
  hipLaunchKernelGGL(moments_k, dim3((unsigned)tiles_of(d)), dim3(kThreads), 0, st, (const double*)sum, (const double*)ss, (int)d, C,
                     mean, var, scale);
  if (out)
    hipLaunchKernelGGL(standardize_k, dim3((unsigned)tiles_of(C), (unsigned)d), dim3(kThreads), 0, st, x, C, (const double*)mean,
                       (const double*)scale, out);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_kmeans_quantize(const double* x, int64_t d, int64_t C, int frac_bits, int* q, int* flag, void* stream) {
  RSX_ARG(x && q && flag, "null tensor");
  RSX_ARG(d >= 1 && C >= 1 && C < (1ll << 31) && d * C < (1ll << 40), "need d >= 1 columns of 1 <= C < 2^31 values");
  RSX_ARG(frac_bits >= 0 && frac_bits <= 30, "need 0 <= frac_bits <= 30");
  hipLaunchKernelGGL(quantize_k, dim3((unsigned)tiles_of(d * C)), dim3(kThreads), 0, (hipStream_t)stream, x, d * C,
                     (double)(1ll << frac_bits), q, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int64_t rsx_kmeans_seed_workspace_bytes(int64_t C, int64_t max_workgroups) {
  if (C < 1 || C >= (1ll << 31) || max_workgroups < 1) return -1;
  return 8 * C + 16 * (int64_t)grid_of(C, max_workgroups);
}

RSX_API int rsx_kmeans_seed(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, uint64_t seed, int64_t max_workgroups,
                            void* ws, int64_t ws_bytes, int* seeds, double* centres, int* flag, void* stream) {
  RSX_ARG(q && seeds && centres && flag, "null tensor");
  RSX_ARG(shape_ok(d, C, K), KM_SHAPE_MSG);
  RSX_ARG(frac_bits >= 0 && frac_bits <= 30, "need 0 <= frac_bits <= 30");
  RSX_ARG(max_workgroups >= 1, "max_workgroups must be >= 1");
  RSX_ARG(ws && rsx::aligned16(ws) && ws_bytes >= rsx_kmeans_seed_workspace_bytes(C, max_workgroups),
          "workspace too small (rsx_kmeans_seed_workspace_bytes) or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_of(C, max_workgroups);
  Cand* cand = reinterpret_cast<Cand*>(ws);
  double* dmin = rsx::at<double>(ws, 16 * (int64_t)grid);
  const double inv = 1.0 / (double)(1ll << frac_bits);
  const int first = (int)(hash_u32_host(seed) % (uint64_t)C);
  hipLaunchKernelGGL(seed_pick_k, dim3(1), dim3(kThreads), 0, st, (const Cand*)cand, 0, 0, first, seeds);
  for (int r = 1; r < (int)K; ++r) {
    hipLaunchKernelGGL(seed_round_k, dim3(grid), dim3(kThreads), 0, st, q, (int)d, C, inv, seed, r, (const int*)seeds, dmin, cand,
                       flag);
    hipLaunchKernelGGL(seed_pick_k, dim3(1), dim3(kThreads), 0, st, (const Cand*)cand, (int)grid, r, 0, seeds);
  }
  hipLaunchKernelGGL(seed_centres_k, dim3((unsigned)tiles_of(K * d)), dim3(kThreads), 0, st, q, (int)d, C, inv, (int)K,
                     (const int*)seeds, centres, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_kmeans_iterate(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, double* centres, int* labels,
                               int64_t* sum_q, int* count, int* ctl, double* shift, double tol_abs, int first_iteration,
                               int n_iter, int64_t max_workgroups, void* stream) {
  RSX_ARG(q && centres && labels && sum_q && count && ctl && shift, "null tensor");
  RSX_ARG(shape_ok(d, C, K), KM_SHAPE_MSG);
  RSX_ARG(frac_bits >= 0 && frac_bits <= 30, "need 0 <= frac_bits <= 30");
  RSX_ARG(max_workgroups >= 1, "max_workgroups must be >= 1");
  RSX_ARG(first_iteration >= 1 && n_iter >= 1 && n_iter <= (1 << 20), "need first_iteration >= 1 and 1 <= n_iter <= 2^20");
  RSX_ARG(tol_abs >= 0.0, "tol_abs must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  const double grid = (double)(1ll << frac_bits), inv = 1.0 / grid;
  for (int it = 0; it < n_iter; ++it) {
    launch_assign<true>(q, (int)d, C, inv, (int)K, centres, labels, nullptr, sum_q, count, ctl, max_workgroups, st);
    hipLaunchKernelGGL(finalize_k, dim3(1), dim3(kThreads), 0, st, (int)d, (int)K, grid, tol_abs, first_iteration + it, centres,
                       reinterpret_cast<long long*>(sum_q), count, ctl, shift);
  }
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_kmeans_assign(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, const double* centres,
                              int64_t max_workgroups, double* ws, int64_t ws_doubles, int* labels, double* dmin,
                              double* inertia, void* stream) {
  RSX_ARG(q && centres && labels, "null tensor");
  RSX_ARG(shape_ok(d, C, K), KM_SHAPE_MSG);
  RSX_ARG(frac_bits >= 0 && frac_bits <= 30, "need 0 <= frac_bits <= 30");
  RSX_ARG(max_workgroups >= 1, "max_workgroups must be >= 1");
  RSX_ARG(!inertia || (dmin && ws && ws_doubles >= rsx::col_chunks(C)), "inertia needs dmin and ceil(C / 4096) workspace doubles");
  hipStream_t st = (hipStream_t)stream;
  launch_assign<false>(q, (int)d, C, 1.0 / (double)(1ll << frac_bits), (int)K, centres, labels, dmin, nullptr, nullptr, nullptr,
                       max_workgroups, st);
  if (inertia) rsx::col_sums<double>(dmin, C, 1, nullptr, ws, inertia, st);
  RSX_LAUNCHED();
  return 0;
}
