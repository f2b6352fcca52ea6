// Internal header of the contrastive-loss units: the bf16x3 / fp16 tile images and the MFMA
// helpers that more than one of nce_plain.hip, nce_grouped.hip and nce_grouped_f16.hip use.
#pragma once
#include "nce_common.h"

namespace rsx {
namespace nce {

// =====================================================================================
// bf16x3 form of the grouped kernels (precision RSX_NCE_BF16X3).
// Every fp32 operand x is split x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (x - hi is exact
// in fp32), and a product is hi*hi' + hi*lo' + lo*hi' on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation (bf16 products are exact; the dropped lo*lo' and the rounding of lo leave
// ~2^-17 relative error per term: max |dot error| 2.7e-6 on unit vectors against 5e-7 for
// the fp32 MFMA and 1.2e-3 for plain bf16). Both products of the backward use it:
//   S tile  : streamed rows (A, ds_read_b128 row reads) x owner rows (B, registers)
//   gradient: G^T (A, straight from the S accumulator: its rows are the k index) x streamed
//             rows (B, ds_read_b64_tr_b16 transposed reads of the same LDS image)
// 3 x 32 cycles per 16 k per 32x32 tile instead of 8 x 64 for the fp32 MFMA (5.3x fewer
// MFMA cycles). The log-sum-exp runs in base 2 (v_exp_f32 without the log2e multiply).
using rsx::img_off, rsx::img_read_tr, rsx::img_tr_base;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
// s_waitcnt vmcnt(0) (expcnt, lgkmcnt left at their maxima): gfx9 encoding
constexpr int kVmcnt0 = 0x0F70;

// [32][128] bf16 tile in the transposed-read image layout of rsx_x3.h
constexpr int kImgElems = kTile * rsx::kImgRow;

struct X3Tile {
  __bf16 hi[kImgElems];
  __bf16 lo[kImgElems];
};

__device__ __forceinline__ void split8(const float4& a, const float4& b, bf16x8& h, bf16x8& l) {
  const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  split_x3(f, h, l);
}

// owner row (dims 64h .. 64h+63 on lane half h) -> hi/lo fragments of k-steps s = 0..7
// (fragment s, element j = dim 64h + 8s + j: the chunk 8h + s of the streamed row reads)
__device__ __forceinline__ void load_owner_x3(bf16x8 (&uh)[8], bf16x8 (&ul)[8], const float* base, int64_t row,
                                              int64_t ld, bool ok, int h) {
  // all 16 loads issued back to back from a clamped row, then zeroed past the rows (a branch
  // around each pair made hipcc wait for every pair before issuing the next)
  const float4* src = reinterpret_cast<const float4*>(base + (ok ? row : 0) * ld + h * 64);
  float4 v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) v[t] = src[t];
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int s = 0; s < 8; ++s) split8(ok ? v[2 * s] : z, ok ? v[2 * s + 1] : z, uh[s], ul[s]);
}

// Streamed operands are split once per call into global hi/lo bf16 images ([rows][128] each,
// nce_split_k), so staging a tile is a plain copy: thread tid moves row tid>>3, 16-B chunks
// tid&7 and 8+(tid&7) of both images (4 x 16-B loads, 4 ds_write_b128).
struct X3Src {
  const __bf16* hi;  // the streamed operand's hi/lo images [rows][128]
  const __bf16* lo;
};
struct X3Stage {
  u32x4 v[4];  // hi chunk0, hi chunk1, lo chunk0, lo chunk1
  __device__ __forceinline__ void load(const X3Src& s, int64_t row, bool ok, int tid) {
    load(s.hi, s.lo, row, ok, tid);
  }
  __device__ __forceinline__ void load(const __bf16* hi, const __bf16* lo, int64_t row, bool ok, int tid) {
    if (ok) {
      const int64_t o = row * kD + (tid & 7) * 8;
      v[0] = *reinterpret_cast<const u32x4*>(hi + o);
      v[1] = *reinterpret_cast<const u32x4*>(hi + o + 64);
      v[2] = *reinterpret_cast<const u32x4*>(lo + o);
      v[3] = *reinterpret_cast<const u32x4*>(lo + o + 64);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void store(X3Tile& t, int tid) const {
    const int row = tid >> 3, ch = tid & 7;
    const int o0 = img_off(row, 8 * ch), o1 = img_off(row, 64 + 8 * ch);
    *reinterpret_cast<u32x4*>(&t.hi[o0]) = v[0];
    *reinterpret_cast<u32x4*>(&t.hi[o1]) = v[1];
    *reinterpret_cast<u32x4*>(&t.lo[o0]) = v[2];
    *reinterpret_cast<u32x4*>(&t.lo[o1]) = v[3];
  }
  // the hi image alone (a pass whose products never read the streamed rows' lo image)
  __device__ __forceinline__ void load_hi(const __bf16* hi, int64_t row, bool ok, int tid) {
    if (ok) {
      const int64_t o = row * kD + (tid & 7) * 8;
      v[0] = *reinterpret_cast<const u32x4*>(hi + o);
      v[1] = *reinterpret_cast<const u32x4*>(hi + o + 64);
    } else {
      v[0] = v[1] = u32x4{0u, 0u, 0u, 0u};
    }
  }
};


// S tile: acc[r] = <streamed row tile_row(r,h), owner row c> (owner on the lane).
// The next k-step's fragments are read before this step's MFMAs (LDS latency under MFMA);
// the scheduling barrier keeps the compiler from hoisting more reads (VGPR budget).
__device__ __forceinline__ f32x16 dots_x3(const X3Tile& t, int c, int h, const bf16x8 (&uh)[8],
                                          const bf16x8 (&ul)[8]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int base = img_off(c, 64 * h);
  bf16x8 ah = *reinterpret_cast<const bf16x8*>(&t.hi[base]);
  bf16x8 al = *reinterpret_cast<const bf16x8*>(&t.lo[base]);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    bf16x8 nh = ah, nl = al;
    if (s < 7) {
      nh = *reinterpret_cast<const bf16x8*>(&t.hi[base + 8 * (s + 1)]);
      nl = *reinterpret_cast<const bf16x8*>(&t.lo[base + 8 * (s + 1)]);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, uh[s], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ul[s], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, uh[s], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    ah = nh;
    al = nl;
  }
  return acc;
}

// gacc[nb] += G^T X over the tile, G given as its hi/lo bf16 fragments (acc layout: streamed
// row tile_row(r,h) in register r, owner on the lane; k-step ks takes registers 8ks..8ks+7,
// i.e. streamed rows 16ks + 8(j>>2) + 4h + (j&3)). The B fragment is those rows of dims
// 32nb + c, two transposed 4-row reads per image. Steps (ks, nb) are software-pipelined by one.
__device__ __forceinline__ void grad_x3s(f32x16 (&gacc)[4], const bf16x8 (&gh)[2], const bf16x8 (&gl)[2],
                                         const X3Tile& t, int lane) {
  const int base = img_tr_base(lane);
  bf16x8 bh, bl;
  bh = img_read_tr(t.hi, base, 0, 0);
  bl = img_read_tr(t.lo, base, 0, 0);
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    bf16x8 nh = bh, nl = bl;
    if (step < 7) {
      nh = img_read_tr(t.hi, base, (step + 1) >> 2, (step + 1) & 3);
      nl = img_read_tr(t.lo, base, (step + 1) >> 2, (step + 1) & 3);
    }
    const int ks = step >> 2, nb = step & 3;
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[ks], bh, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[ks], bl, gacc[nb], 0, 0, 0);
    gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[ks], bh, gacc[nb], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    bh = nh;
    bl = nl;
  }
}

// (a, b) -> packed bf16 hi pair and lo pair (x = hi + lo, hi = RNE bf16(x), lo = bf16(x - hi)):
// one pair conversion for hi, its two halves unpacked as fp32 by a shift and a mask, two
// subtractions and one pair conversion for lo (the per-element form converted every element
// twice and re-packed).
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  const bf16x2 h = {(__bf16)a, (__bf16)b};
  hi = __builtin_bit_cast(uint32_t, h);
  const float ha = __uint_as_float(hi << 16), hb = __uint_as_float(hi & 0xffff0000u);
  const bf16x2 l = {(__bf16)(a - ha), (__bf16)(b - hb)};
  lo = __builtin_bit_cast(uint32_t, l);
}

__device__ __forceinline__ void split_tile(const f32x16& g, bf16x8 (&gh)[2], bf16x8 (&gl)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4 h, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t hq, lq;
      split_pair(g[8 * ks + 2 * q], g[8 * ks + 2 * q + 1], hq, lq);
      h[q] = hq;
      l[q] = lq;
    }
    gh[ks] = __builtin_bit_cast(bf16x8, h);
    gl[ks] = __builtin_bit_cast(bf16x8, l);
  }
}

// =====================================================================================
// Product types: everything the fp32 and the bf16x3 form of one kernel body differ in.
//   Owner, OwnerLo  the wave's 32 owner rows in registers (lane (c,h): dims 64h .. 64h+63 of row c),
//          filled by load_owner. Two blocks, each a variable of its own in the kernel: bf16x3 keeps
//          its hi and lo fragments apart (as one object hipcc vectorises their conversion differently
//          and every bf16x3 kernel changes); fp32 has one block and an empty tag for the other.
//   Src    where streamed rows come from; Stage: one thread's share of a tile on its way from Src to
//          LDS (thread tid: row tid>>3), made by stage(tid); Tile: the LDS image of 32 streamed rows
//   dots   acc[r] = <streamed row tile_row(r,h), owner row c> (owner on the lane)
//   grad   gacc[kb] += G^T X over the tile, G in the layout dots returns: owner row c's gradient
//          columns 32kb + n += sum_s G[s] X[tile_row(s,h)][32kb + n]; (c, h) = (lane & 31, lane >> 5)
//   kStoreAfterBarrier  the next tile's Stage::store sits between two barriers (true) or ahead of
//          the tile's only barrier (false: the buffer was last read in the previous tile)
// Two conditions keep hipcc's output what it is for the same text written out in the kernel (DESIGN.md,
// section 4): F32Prod::stage fixes the thread's row and column once, at kernel scope (computed inside
// load and store they are sunk into the branch and computed twice), and a Src is built where it is
// used (held in a local that the staging lambdas capture, it changes how the owner loads vectorise).
struct F32Prod {
  typedef float Tile[kTile][kLdsStride];
  struct Src {
    const float* p;
    int64_t ld;
  };
  static __device__ __forceinline__ Src src(const float* p, int64_t ld, const __bf16*, const __bf16*) {
    return {p, ld};
  }
  struct Owner {
    float u[64];  // k permuted as k = 64h + s: a contiguous half row per lane
  };
  struct OwnerLo {};  // taken by value: it never reaches the generated code
  static __device__ __forceinline__ void load_owner(Owner& o, OwnerLo, const float* base, int64_t row, int64_t ld,
                                                    bool ok, int h) {
    if (ok) {
      const float4* src = reinterpret_cast<const float4*>(base + row * ld + h * 64);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float4 v = src[t];
        o.u[4 * t + 0] = v.x; o.u[4 * t + 1] = v.y; o.u[4 * t + 2] = v.z; o.u[4 * t + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 64; ++t) o.u[t] = 0.0f;
    }
  }
  struct Stage {
    float4 v[4];     // 16 floats of row srow from column scol
    int srow, scol;  // set once by stage(tid), at kernel scope
    __device__ __forceinline__ void load(const Src& s, int64_t row, bool ok, int) {
      if (ok) {
        const float4* src = reinterpret_cast<const float4*>(s.p + row * s.ld + scol);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = src[t];
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __device__ __forceinline__ void store(Tile& t, int) const {
#pragma unroll
      for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(&t[srow][scol + 4 * k]) = v[k];
    }
  };
  static __device__ __forceinline__ Stage stage(int tid) {
    Stage s;
    s.srow = tid >> 3;
    s.scol = (tid & 7) * 16;
    return s;
  }
  static constexpr bool kStoreAfterBarrier = true;
  // v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain
  static __device__ __forceinline__ f32x16 dots(const Tile& t, const Owner& o, OwnerLo, int c, int h) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float* xrow = &t[c][h * 64];
#pragma unroll
    for (int s = 0; s < 64; s += 4) {
      const float4 bv = *reinterpret_cast<const float4*>(xrow + s);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, o.u[s + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, o.u[s + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.z, o.u[s + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.w, o.u[s + 3], acc, 0, 0, 0);
    }
    return acc;
  }
  // A operand (lane (c,h), step s) = G[own = c][str = tile_row(s,h)] = G[s], straight from the
  // dots accumulator; B operand = X[tile_row(s,h)][32kb + c]
  static __device__ __forceinline__ void grad(f32x16 (&gacc)[4], const f32x16& G, const Tile& t, int, int c,
                                              int h) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float* srow_p = &t[tile_row(s, h)][c];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        gacc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(G[s], srow_p[kb * 32], gacc[kb], 0, 0, 0);
    }
  }
};

struct X3Prod {
  typedef X3Tile Tile;
  typedef X3Src Src;
  static __device__ __forceinline__ Src src(const float*, int64_t, const __bf16* hi, const __bf16* lo) {
    return {hi, lo};
  }
  typedef bf16x8 Owner[8];
  typedef bf16x8 OwnerLo[8];
  static __device__ __forceinline__ void load_owner(Owner& uh, OwnerLo& ul, const float* base, int64_t row, int64_t ld,
                                                    bool ok, int h) {
    load_owner_x3(uh, ul, base, row, ld, ok, h);
  }
  typedef X3Stage Stage;
  static __device__ __forceinline__ Stage stage(int) { return Stage(); }
  static constexpr bool kStoreAfterBarrier = false;
  static __device__ __forceinline__ f32x16 dots(const Tile& t, const Owner& o, const OwnerLo& ul, int c, int h) {
    return dots_x3(t, c, h, o, ul);
  }
  static __device__ __forceinline__ void grad(f32x16 (&gacc)[4], const f32x16& G, const Tile& t, int lane, int,
                                              int) {
    bf16x8 gh[2], gl[2];
    split_tile(G, gh, gl);
    grad_x3s(gacc, gh, gl, t, lane);
  }
};

// fused forwards: the running max is raised only when a tile max exceeds it by more than 2^8
constexpr float kLazyLog2 = 8.0f;

// Bias / column-count staging of the fused forwards (nce_grouped_fwdg_x3p_k, nce_grouped_fwdg_h_k):
// thread tid < kTile carries column j0 + tid. Raw loads only (math on a load in flight would wait
// for it); columns past the split get bias +inf and count 0.
__device__ __forceinline__ void stage_bias_count_load(const GArgs& a, int64_t j0, int64_t j_end, int tid, float& stg_b,
                                                      float& stg_c) {
  if (tid < kTile) {
    const int64_t jj = j0 + tid;
    const bool ok = jj < j_end;
    stg_b = ok ? (a.bias ? a.bias[jj] : 0.0f) : INFINITY;
    stg_c = ok ? a.colcnt[jj] : 0.0f;
  }
}
// -bias log2e + log2 c_d: the multiplicity rides in the exponent (one fma per logit, no
// multiply); -inf past the split (c = 0, bias = inf)
__device__ __forceinline__ void stage_bias_count_store(float* sB2, float* sCnt, int tid, float stg_b, float stg_c) {
  if (tid < kTile) {
    sB2[tid] = -(stg_b * kLog2e) + __log2f(stg_c);
    sCnt[tid] = stg_c;
  }
}

// fp16 images of RSX_NCE_F16 (nce_grouped_f16.hip): hi + lo of x * 2^8 in the bf16 containers
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float kHScale = 256.0f;         // operand scale 2^8

__device__ __forceinline__ void split8_h(const float4& a, const float4& b, bf16x8& h, bf16x8& l) {
  const float f[8] = {a.x * kHScale, a.y * kHScale, a.z * kHScale, a.w * kHScale,
                      b.x * kHScale, b.y * kHScale, b.z * kHScale, b.w * kHScale};
  f16x8 hv, lv;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const _Float16 hk = (_Float16)f[k];
    hv[k] = hk;
    lv[k] = (_Float16)(f[k] - (float)hk);
  }
  h = __builtin_bit_cast(bf16x8, hv);
  l = __builtin_bit_cast(bf16x8, lv);
}

}  // namespace nce
}  // namespace rsx
