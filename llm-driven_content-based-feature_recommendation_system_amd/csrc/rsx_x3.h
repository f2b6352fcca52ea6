// The bf16x3 building blocks every MFMA kernel family shares: the vector
// types, the 32x32 accumulator row map, the hi/lo split, the transposed-read LDS image and the
// ordered float keys. Kernels stay in their own file's anonymous namespace and take these with
// `using`.
#pragma once
#include "rsx_common.h"

namespace rsx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// 32x32 MFMA accumulator: register r of lane half h holds tile row tile_row(r, h), column lane & 31
__device__ __forceinline__ int tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The split x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32): a product
// hi*hi' + hi*lo' + lo*hi' on the bf16 MFMA with fp32 accumulation leaves ~2^-17 relative error
// per term. Two forms and no others: x3_lo for one value inside a larger expression, split_x3 for
// N values into a pair of bf16 vectors (callers that store u32x4 / s16x4 bit-cast the result).
// A scalar helper returning {hi, lo} as a struct is not one of them: it moves the schedule of
// deepfm_fused.hip's kernels.
__device__ __forceinline__ __bf16 x3_lo(float v, __bf16 hi) { return (__bf16)(v - (float)hi); }

template <typename V, int N>
__device__ __forceinline__ void split_x3(const float (&f)[N], V& hi, V& lo) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const __bf16 hk = (__bf16)f[k];
    hi[k] = hk;
    lo[k] = x3_lo(f[k], hk);
  }
}
// split_x3 of 8 fp32 as the staging stores take it: 8 hi + 8 lo bf16, one 16-B chunk each
__device__ __forceinline__ void split8(const float4& x, const float4& y, u32x4& hi, u32x4& lo) {
  const float f[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
  bf16x8 h, l;
  split_x3(f, h, l);
  hi = __builtin_bit_cast(u32x4, h);
  lo = __builtin_bit_cast(u32x4, l);
}

// Token-major [rows][128] bf16 LDS image: 320-B rows plus a 16-B skew per 8-row group, i.e. byte
// offset 320*row + 16*(row>>3) + 2*col. Conflict-free for the row reads (ds_read_b128, lane (c,h)
// -> row c, chunk 8h+s), the transposed reads (ds_read_b64_tr_b16) and the staging stores
// (ds_write_b128), and every read address is a per-lane base + an immediate (no per-step
// address registers); checked with tools/lds_banks.py.
constexpr int kImgRow = 160;  // bf16 elements per image row
__device__ __forceinline__ int img_off(int row, int col) { return row * kImgRow + 8 * (row >> 3) + col; }

// Transposed fragment reads of an image: lane (c, h) element j of step (ks, nb) is row
// 16ks + 8(j>>2) + 4h + (j&3), column 32nb + c, as two 4-row reads from the lane's base offset
// img_tr_base(lane) (+ img_off(16ks + 8half, 32nb) per read, an immediate).
__device__ __forceinline__ int img_tr_base(int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3, h = lane >> 5, cb = (lane >> 4) & 1;
  return img_off(4 * h + q, 16 * cb + 4 * p);
}
__device__ __forceinline__ bf16x8 img_read_tr(const __bf16* img, int base, int ks, int nb) {
  const int o0 = base + img_off(16 * ks, 32 * nb), o1 = base + img_off(16 * ks + 8, 32 * nb);
  const bf16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o0]));
  const bf16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(&img[o1]));
  return __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Order-preserving uint key of a float (larger float <=> larger key), on the float's bits and on
// the float, and its inverse.
__device__ __forceinline__ unsigned ordered_key_bits(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned ordered_key(float f) { return ordered_key_bits(__float_as_uint(f)); }
__device__ __forceinline__ float ordered_key_inv(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// Sort key of a score: the ordered key after -0.0 is made +0.0. The zero is canonicalised on the
// bits: through ordered_key(float) the key kernels of binary_eval.hip and group_eval.hip move.
__device__ __forceinline__ unsigned score_key(float z) {
  unsigned u = __float_as_uint(z);
  if (z == 0.0f) u = 0u;  // -0.0 and +0.0 tie
  return ordered_key_bits(u);
}

}  // namespace rsx
