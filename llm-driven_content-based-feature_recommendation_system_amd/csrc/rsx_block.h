// The integer workgroup primitives the selection and evaluation kernels share:
// the wave and workgroup scans, the descending digit search of a radix select and the bitonic sort of
// 64-bit codes. Workgroups are one-dimensional and made of whole 64-lane waves. Kernels stay in their
// own file's anonymous namespace and take these with `using`.
#pragma once
#include "rsx_common.h"
#include <string.h>
#include <type_traits>

namespace rsx {

// Inclusive sum over the wave's lanes: lane l returns x_0 + ... + x_l.
template <class T>
__device__ __forceinline__ T wave_scan_incl(T x) {
  static_assert(std::is_same<T, int>::value || std::is_same<T, unsigned>::value, "int or unsigned");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// The value of the lane d places earlier in scan order (REV: scan order runs from lane 63 down), for
// any type made of whole words.
template <bool REV, class T>
__device__ __forceinline__ T shfl_earlier(const T& v, int d) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  int w[sizeof(T) / 4];
  memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = REV ? __shfl_down(w[k], d, 64) : __shfl_up(w[k], d, 64);
  T r;
  memcpy(&r, w, sizeof(T));
  return r;
}

struct Sum {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// Exclusive scan of one value per thread over the NT threads of the workgroup (REV: from the last
// thread down); total = all NT values combined. op(earlier, later) need not commute, and the order of
// combination is fixed, so a floating-point scan gives the same bits every run: the lanes of a wave by
// doubling distance (incl = op(value d lanes earlier, incl)), then the wave totals in scan order
// (total = op(total, v), pre = op(pre, v)), and the result op(pre, e) with e the wave's inclusive
// value one lane earlier. sm holds NT / 64 values and is free again on return (two barriers).
template <int NT, bool REV = false, class T, class Op>
__device__ __forceinline__ T block_scan_excl(T x, Op op, T ident, T* sm, T& total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = shfl_earlier<REV>(incl, d);
    if (REV ? lane + d < 64 : lane >= d) incl = op(y, incl);
  }
  if (lane == (REV ? 0 : 63)) sm[w] = incl;
  __syncthreads();
  T pre = ident;
  total = ident;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int q = REV ? NW - 1 - k : k;
    const T v = sm[q];
    total = op(total, v);
    if (REV ? q > w : q < w) pre = op(pre, v);
  }
  T e = shfl_earlier<REV>(incl, 1);
  if (lane == (REV ? 63 : 0)) e = ident;
  __syncthreads();
  return op(pre, e);
}

// The segmented scan: a value with "a segment starts here". op(earlier, later) keeps the later one when it
// starts a segment, else combines: associative, so block_scan_excl scans every segment of the tile on its
// own, and the total is the tile's trailing piece with head = a segment starts somewhere in the tile.
template <class V>
struct Seg {
  V v;
  int head;
};
template <class V, class Op>
struct SegOp {
  __device__ __forceinline__ Seg<V> operator()(Seg<V> a, Seg<V> b) const {
    return b.head ? b : Seg<V>{Op()(a.v, b.v), a.head};
  }
};

// One step of a descending 8-bit radix select, called by every lane of ONE wave: count(bin) is the
// number of keys in bin 0..255. Lane l takes the bins 255 - 4l ... 252 - 4l and a scan over the lanes
// counts the keys above them. Returns true in exactly one lane, the owner of the bin where the running
// count from bin 255 downward first reaches need (1 <= need <= the sum of all bins): there digit = that
// bin and above = the count in the bins strictly above it.
template <class Count>
__device__ __forceinline__ bool digit_search_desc(Count count, unsigned need, int lane, int& digit, unsigned& above) {
  unsigned c[4];  // c[j] = bin 255 - 4 lane - j, read in ascending bin order: four LDS words become one 16-byte read
#pragma unroll
  for (int j = 0; j < 4; ++j) c[3 - j] = count(252 - 4 * lane + j);
  const unsigned s = c[0] + c[1] + c[2] + c[3];
  const unsigned incl = wave_scan_incl(s);
  const int first = __ffsll((long long)__ballot(incl >= need)) - 1;  // need <= the total guarantees a hit
  if (lane != first) return false;
  unsigned acc = incl - s;
  digit = 255 - 4 * lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (acc + c[j] >= need) {
      digit = 255 - 4 * lane - j;
      break;
    }
    acc += c[j];
  }
  above = acc;
  return true;
}

__host__ __device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// Bitonic sort of a[0, P) in LDS, descending; P a power of two. The codes are key << 32 | ~index, so
// the order is key descending, then index ascending, and 0 pads. Every thread of the NT-thread
// workgroup calls it: a barrier before the first step orders the callers' writes, and a is complete
// (and visible) on return. NT is a compile-time constant: strided by blockDim.x, hnm_select_k grew by
// some 390 lines of assembly and hnm_mine and select_topk_rows measured slower.
template <int NT>
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* a, int P) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (P >> 1); t += NT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long x = a[lo], y = a[hi];
        if ((x < y) == desc) {
          a[lo] = y;
          a[hi] = x;
        }
      }
    }
  }
  __syncthreads();
}

}  // namespace rsx
