// One element of torch's Adam / AdamW update, shared by the optimiser kernels (optim.hip's clipped
// AdamW, distill.hip's fused Adam): double-precision scalars, float state, the arithmetic of torch's
// fused implementation.
#pragma once
#include "rsx_common.h"

namespace rsx {

// g *= coef (the clip coefficient; 1 = none), the decoupled weight decay (wd = 0: plain Adam), both
// moments and the bias-corrected step: step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t).
__device__ __forceinline__ void adam_elem(float& p, float& g, float& m, float& v, float coef, double lr, double wd,
                                          double b1, double b2, double eps, double step_size, double bc2_sqrt) {
  g = g * coef;
  if (wd != 0.0) p = (float)(p - lr * wd * p);
  m = (float)(b1 * m + (1.0 - b1) * g);
  v = (float)(b2 * v + (1.0 - b2) * g * g);
  const float denom = (float)(sqrtf(v) / bc2_sqrt + eps);
  p -= (float)step_size * m / denom;
}

}  // namespace rsx
