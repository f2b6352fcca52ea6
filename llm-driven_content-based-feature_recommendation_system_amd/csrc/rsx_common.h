// Shared device/host helpers for the recsys_amd C-ABI library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stddef.h>

namespace rsx {

// Thread-local last-error text; read back through rsx_last_error().
void set_error(const char* fmt, ...);

constexpr int kWave = 64;

// Counter-based dropout RNG: murmur3's fmix32 finaliser over the element index mixed with
// the 64-bit seed (32-bit integer ops only: ~10 VALU per element, cheap enough to evaluate
// per attention score). Forward and backward regenerate the identical keep-mask from the
// same (seed, index).
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
  uint32_t x = (uint32_t)idx ^ ((uint32_t)(idx >> 32) * 0x9E3779B1u) ^ (uint32_t)seed;
  x ^= (uint32_t)(seed >> 32) * 0x85EBCA77u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
// hash_u32(seed, idx) for idx < 2^32, where the high-word term vanishes, in 32-bit ops only (the
// GEMM epilogues' flat index m*N + n). The two must agree bit for bit there: the tests rebuild the
// keep masks on the host from hash_u32's formula.
__device__ __forceinline__ uint32_t hash_u32_idx32(uint64_t seed, uint32_t idx) {
  uint32_t x = idx ^ (uint32_t)seed;
  x ^= (uint32_t)(seed >> 32) * 0x85EBCA77u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

struct Dropout {
  uint64_t seed;
  uint32_t thresh;  // keep iff hash >= thresh ; thresh == 0 => no dropout
  float scale;      // 1 / (1 - p)
  __device__ __forceinline__ bool active() const { return thresh != 0u; }
  __device__ __forceinline__ float apply(float v, uint64_t idx) const {
    if (thresh == 0u) return v;
    return hash_u32(seed, idx) >= thresh ? v * scale : 0.0f;
  }
};

inline Dropout make_dropout(float p, uint64_t seed) {
  Dropout d;
  d.seed = seed;
  if (p <= 0.0f) {
    d.thresh = 0u;
    d.scale = 1.0f;
  } else {
    double t = (double)p * 4294967296.0;
    if (t >= 4294967295.0) t = 4294967295.0;
    d.thresh = (uint32_t)t;
    if (d.thresh == 0u) d.thresh = 1u;
    d.scale = 1.0f / (1.0f - p);
  }
  return d;
}

template <typename T>
__device__ __forceinline__ T wave_sum_width(T v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float fmax_nan(float a, float b) { return a > b ? a : b; }

// GELU in its exact erf form (torch's default): gelu(z) = z Phi(z), gelu'(z) = Phi(z) + z phi(z)
__device__ __forceinline__ float gelu_erf_cdf(float z) { return 0.5f * (1.0f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float z) {
  const float cdf = gelu_erf_cdf(z);
  const float pdf = 0.3989422804014327f * __expf(-0.5f * z * z);
  return cdf + z * pdf;
}

// compute units of the current device (grid sizing, speed only); 256 when the query fails
inline int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 256;
    return v > 0 ? v : 256;
  }();
  return n;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Workspace layouts: take(n) returns the running offset and advances it by n rounded up to the
// granule (256 for byte layouts, 64 for float layouts: 256-B granules both); off ends as the total.
struct Bump {
  int64_t off, granule;
  int64_t take(int64_t n) {
    const int64_t r = off;
    off += (n + granule - 1) / granule * granule;
    return r;
  }
};

// Typed pointer to byte offset off of a workspace.
template <typename P>
P* at(void* ws, int64_t off) {
  return reinterpret_cast<P*>(reinterpret_cast<char*>(ws) + off);
}

// The Logloss head of the rerankers' training steps (csrc/deepfm_train.hip: head_k + head_sum_k),
// arguments as rsx_deepfm_train_head after its checks; relu_mask: dh2 = g wo [h2 > 0], else g wo.
int train_head_launch(const float* h2, const float* wo, const float* lin, const float* bias, const float* y,
                      int64_t R, int mean, bool relu_mask, float* logit, float* g, float* dh2, void* ws, double* loss,
                      float* dbias, float* dwo, void* stream);

// The QuerySoftMax gradient stage (csrc/gbdt_rank.hip), arguments as rsx_gbdt_grad_query_softmax after its
// checks; the workspace bytes it needs, or -1 unless 1 <= R < 2^31 and 1 <= G <= R.
int64_t gbdt_query_softmax_workspace(int64_t R, int64_t G);
void gbdt_query_softmax_launch(const float* F, const float* y, const int* row_group, const int* goff, int64_t R, int G,
                               void* ws, int* qg, int* qh, hipStream_t st);

}  // namespace rsx

#define RSX_ARG(cond, msg)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      rsx::set_error("%s: invalid argument: %s", __func__, msg); \
      return 1;                                              \
    }                                                        \
  } while (0)

#define RSX_LAUNCHED()                                                        \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess) {                                                   \
      rsx::set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
      return (int)e_;                                                         \
    }                                                                         \
  } while (0)

#define RSX_API extern "C" __attribute__((visibility("default")))
