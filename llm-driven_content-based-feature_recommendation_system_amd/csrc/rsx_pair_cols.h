// The FeatureEngineer numeric columns of one (user, item) pair, written once: rsx_rerank_tabular (gbdt.hip,
// the serving rows) and rsx_pair_tabular (ranker_rows.hip, the training rows) both call pair_columns, so
// columns 1..6 of a pair have the same bits in training and in serving and a candidate falls into the bin
// the same pair fell into when the model's borders were built.
#pragma once
#include "rsx_common.h"

namespace rsx {

// One wave per pair, called by all 64 lanes: u, v are the pair's rows of d floats, price and avg the item's
// price and the user's average price (read by lane 0 only). Lane 0 writes columns 1..6 of row c of the
// column-major feats [7, R]: the mean, the maximum and the population standard deviation of u * v, the
// price, the average and price_diff_ratio = (price - avg) / avg where avg > 0, else 0. Returns the wave's
// sum of u * v (the fp32 dot product, the same value in every lane); column 0 is the caller's.
__device__ __forceinline__ float pair_columns(const float* __restrict__ u, const float* __restrict__ v, int d, int lane,
                                              const float* __restrict__ price, const float* __restrict__ avg,
                                              float* __restrict__ feats, int64_t R, int64_t c) {
  float sum = 0.0f, mx = -__builtin_huge_valf();
  for (int i = lane; i < d; i += 64) {
    const float p = u[i] * v[i];
    sum += p;
    mx = fmax_nan(mx, p);
  }
  sum = wave_sum_width(sum, 64);
  for (int o = 32; o > 0; o >>= 1) mx = fmax_nan(mx, __shfl_xor(mx, o, 64));
  const float mean = sum / (float)d;
  float ss = 0.0f;
  for (int i = lane; i < d; i += 64) {
    const float t = u[i] * v[i] - mean;
    ss += t * t;
  }
  ss = wave_sum_width(ss, 64);
  if (lane != 0) return sum;
  const float pr = *price, a = *avg;
  feats[R + c] = mean;
  feats[2 * R + c] = mx;
  feats[3 * R + c] = sqrtf(ss / (float)d);
  feats[4 * R + c] = pr;
  feats[5 * R + c] = a;
  feats[6 * R + c] = a > 0.0f ? (pr - a) / a : 0.0f;
  return sum;
}

}  // namespace rsx
