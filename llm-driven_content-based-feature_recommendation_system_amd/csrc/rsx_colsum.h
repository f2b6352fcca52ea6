// Fixed-order column sums in two levels, shared by csrc/tx_features.hip (the cold-start means, the standardised user
// columns) and csrc/kmeans.hip (the column moments, the inertia). Workgroup (k, c) sums chunk k of x[c, 0 .. n), len
// elements (minus mean_of[c] / n_mean, squared, when mean_of is given): thread j takes the chunk's elements j, j + 256,
// ... in order, then the 256 partial sums meet in a fixed tree; out[c, k]. col_sums runs it over chunks of 4096, then
// once more over the chunk sums: the same bits every run.
#pragma once
#include "rsx_common.h"

// v * v + acc stays two roundings: the sums are specified that way (the including files say the same)
#pragma clang fp contract(off)

namespace rsx {

constexpr int kColThreads = 256;
constexpr int kColChunk = 4096;

inline int64_t col_chunks(int64_t n) { return (n + kColChunk - 1) / kColChunk; }

template <class T>
__global__ __launch_bounds__(kColThreads) void col_reduce_k(const T* __restrict__ x, int64_t n, int64_t len,
                                                            const double* __restrict__ mean_of, int64_t n_mean,
                                                            double* __restrict__ out) {
  __shared__ double sm[kColThreads];
  const T* col = x + (int64_t)blockIdx.y * n;
  const int64_t lo = (int64_t)blockIdx.x * len, hi = lo + len < n ? lo + len : n;
  const double mean = mean_of ? mean_of[blockIdx.y] / (double)n_mean : 0.0;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kColThreads) {
    const double v = (double)col[i] - mean;
    acc += mean_of ? v * v : v;
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kColThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sm[0];
}

// out[c] = the sum over x[c, 0 .. n) for c < cols; part holds cols * col_chunks(n) doubles
template <class T>
void col_sums(const T* x, int64_t n, int cols, const double* mean_of, double* part, double* out, hipStream_t st) {
  const int64_t nc = col_chunks(n);
  hipLaunchKernelGGL(col_reduce_k<T>, dim3((unsigned)nc, (unsigned)cols), dim3(kColThreads), 0, st, x, n, (int64_t)kColChunk,
                     mean_of, n, part);
  hipLaunchKernelGGL(col_reduce_k<double>, dim3(1, (unsigned)cols), dim3(kColThreads), 0, st, (const double*)part, nc, nc,
                     (const double*)nullptr, nc, out);
}

}  // namespace rsx
