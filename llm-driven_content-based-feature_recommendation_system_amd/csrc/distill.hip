// Distillation of LightGCL's dot-product scores into unit vectors (gnn_model/distill_mag_to_cos_l2.py):
// MagnitudeEncoder = Linear(64, 128) + LeakyReLU + Dropout + Linear(128, 64) + F.normalize, trained so
// that cos(student_u, student_i) exp(logit_scale) reproduces the teacher's <u, i> (MSE, Adam).
//   * rsx_magnitude_encode  the eval forward over N rows
//   * rsx_distill_grads     gather, forward, loss and backward of one batch of pairs into
//                           per-workgroup partial slots
//   * rsx_distill_apply     the slots added in slot order, the gradients / loss written, Adam
// One training step is the last two launches. Exact fp32 products on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), no float atomics, every sum in a fixed order:
// bit-reproducible. Tile-to-workgroup assignment and slot count depend on B alone.
//
// A workgroup (4 waves) stages W1 and W2 in LDS once and walks its tiles of 32 pairs = 64 stacked rows
// (the 32 user rows, then the 32 item rows). Per tile, with 32x32 output tiles per wave:
//   P  [64,128] = X W1^T + b1    wave w: columns 32w.., both row halves        (K = 64)
//   H = dropout(lrelu(P)) -> LDS; the factor dP/dH stays in registers
//   Z  [64, 64] = H W2^T + b2    wave w: rows 32(w>>1).., columns 32(w&1)..    (K = 128)
//   n = max(|Z_r|, eps), Y = Z / n (4 lanes per row); per pair cos, s, t, ds and dZ in place (8 lanes)
//   dW2[64,128] += dZ^T H        wave w: columns 32w.., both row halves        (K = 64 rows)
//   dH [64,128] = dZ W2          the tiles of P, so dP = dH * factor in registers, then -> LDS over H
//   dW1[128,64] += dP^T X        wave w: rows 32w.., both column halves        (K = 64 rows)
// dW1 / dW2 stay in 64 accumulator registers per lane across tiles; db1 / db2 are column sums by one
// thread per column. LDS rows are padded to an odd stride (65 / 129 floats): a ds_read_b32 of 32
// rows at one k, or of 32 consecutive columns of one row, touches 32 different banks.
#include "rsx_common.h"
#include "rsx_adam.h"
#include "recsys_amd.h"

namespace {

constexpr int kIn = 64, kHid = 128, kOut = 64;
constexpr int kPairs = 32;       // pairs per tile
constexpr int kRows = 2 * kPairs;  // stacked rows per tile (and rows per tile of the forward)
constexpr int kMaxSlots = 256;
constexpr int kOffW1 = 0, kOffB1 = kHid * kIn, kOffW2 = kOffB1 + kHid, kOffB2 = kOffW2 + kOut * kHid,
              kOffLs = kOffB2 + kOut, kNP = kOffLs + 1;  // 16,577 parameters in module order
constexpr int LDX = kIn + 1, LDH = kHid + 1;
static_assert(kNP == 16577, "parameter count");

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Lds {
  float w1[kHid * LDX];   // W1[c][k]
  float w2[kOut * LDH];   // W2[o][c]
  float x[kRows * LDX];
  float h[kRows * LDH];   // H, later dP
  float z[kRows * LDX];   // Z, then Y, then dZ
  float nrm[kRows];       // max(|Z_r|, eps), negated where |Z_r| < eps
  float err[kPairs];      // (s - t)^2
  float dls[kPairs];      // ds * s
  int valid[kPairs];
};
static_assert(sizeof(Lds) <= 160 * 1024, "LDS");

// row of accumulator register reg in a 32x32 C/D tile (the column is lane & 31)
__device__ __forceinline__ int crow(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// acc{0,1} += sum_k A{0,1}(i, k) B(k, j), A(i, k) = a[i AI + k AK], B(k, j) = b[k BK + j BJ]
template <int AI, int AK, int BK, int BJ, int K>
__device__ __forceinline__ void mma_2a(f32x16& acc0, f32x16& acc1, const float* a0, const float* a1, const float* b) {
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  a0 += r * AI + h * AK;
  a1 += r * AI + h * AK;
  b += h * BK + r * BJ;
#pragma unroll 8
  for (int k = 0; k < K; k += 2) {
    const float bv = b[k * BK];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[k * AK], bv, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[k * AK], bv, acc1, 0, 0, 0);
  }
}

// acc{0,1} += sum_k A(i, k) B{0,1}(k, j)
template <int AI, int AK, int BK, int BJ, int K>
__device__ __forceinline__ void mma_2b(f32x16& acc0, f32x16& acc1, const float* a, const float* b0, const float* b1) {
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  a += r * AI + h * AK;
  b0 += h * BK + r * BJ;
  b1 += h * BK + r * BJ;
#pragma unroll 8
  for (int k = 0; k < K; k += 2) {
    const float av = a[k * AK];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0[k * BK], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1[k * BK], acc1, 0, 0, 0);
  }
}

template <int AI, int AK, int BK, int BJ, int K>
__device__ __forceinline__ void mma_1(f32x16& acc, const float* a, const float* b) {
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  a += r * AI + h * AK;
  b += h * BK + r * BJ;
#pragma unroll 8
  for (int k = 0; k < K; k += 2)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * AK], b[k * BK], acc, 0, 0, 0);
}

__device__ __forceinline__ f32x16 splat(float v) {
  f32x16 a;
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = v;
  return a;
}

__device__ __forceinline__ void stage_weights(Lds& L, const float* __restrict__ w1, const float* __restrict__ w2) {
  for (int e = threadIdx.x * 4; e < kHid * kIn; e += 256 * 4) {
    const float4 a = *reinterpret_cast<const float4*>(w1 + e);
    float* d = &L.w1[(e / kIn) * LDX + e % kIn];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
    const float4 b = *reinterpret_cast<const float4*>(w2 + e);
    float* q = &L.w2[(e / kHid) * LDH + e % kHid];
    q[0] = b.x; q[1] = b.y; q[2] = b.z; q[3] = b.w;
  }
}

// The forward of one tile from L.x: H into L.h, Y = Z / n into L.z, n into L.nrm. g0 / g1: the dropout
// row index of tile rows 0 and 32. TRAIN keeps dP/dH per element of this wave's two P tiles in fac.
// The eval forward and the step's forward are this one function: at p = 0 they agree bit for bit.
template <bool TRAIN>
__device__ __forceinline__ void tile_forward(Lds& L, const float* __restrict__ b1, const float* __restrict__ b2,
                                             float slope, float eps, const rsx::Dropout& drop, int64_t g0, int64_t g1,
                                             f32x16& fac0, f32x16& fac1) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  {
    const int c = 32 * w + (lane & 31);
    f32x16 p0 = splat(b1[c]), p1 = p0;
    mma_2a<LDX, 1, 1, LDX, kIn>(p0, p1, L.x, L.x + 32 * LDX, L.w1 + 32 * w * LDX);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x16& p = half ? p1 : p0;
      f32x16& fac = half ? fac1 : fac0;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = crow(reg, lane);
        const float v = p[reg];
        const float lr = v > 0.f ? 1.f : slope;
        float a = v * lr;
        if (TRAIN) {   // branch-free: at p = 0 thresh is 0 and the scale 1, so a is unchanged bit for bit
          const bool keep = rsx::hash_u32(drop.seed, (uint64_t)((half ? g1 : g0) + r) * kHid + c) >= drop.thresh;
          const float f = keep ? drop.scale : 0.f;
          a *= f;
          fac[reg] = lr * f;
        }
        L.h[(32 * half + r) * LDH + c] = a;
      }
    }
  }
  __syncthreads();
  {
    const int mi = w >> 1, oj = w & 1, o = 32 * oj + (lane & 31);
    f32x16 z = splat(b2[o]);
    mma_1<LDH, 1, 1, LDH, kHid>(z, L.h + 32 * mi * LDH, L.w2 + 32 * oj * LDH);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) L.z[(32 * mi + crow(reg, lane)) * LDX + o] = z[reg];
  }
  __syncthreads();
  {
    // four lanes per row, 16 columns each; the row's sum of squares = the four partial chains added
    // by two xor shuffles
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
    float* zr = &L.z[r * LDX + 16 * q];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) ss = fmaf(zr[e], zr[e], ss);
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    const float nz = sqrtf(ss);
    const float n = nz > eps ? nz : eps;
#pragma unroll
    for (int e = 0; e < 16; ++e) zr[e] = zr[e] / n;
    if (q == 0) L.nrm[r] = nz < eps ? -n : n;
  }
  __syncthreads();
}

// rows [16 q, 16 q + 16) of tile row r -> out (16-B aligned row)
__device__ __forceinline__ void store_row_quarter(const Lds& L, int r, int q, float* __restrict__ out) {
  const float* y = &L.z[r * LDX + 16 * q];
#pragma unroll
  for (int e = 0; e < 16; e += 4)
    *reinterpret_cast<float4*>(out + 16 * q + e) = make_float4(y[e], y[e + 1], y[e + 2], y[e + 3]);
}

__global__ __launch_bounds__(256) void encode_k(const float* __restrict__ X, int64_t ldx, int64_t N,
                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                               float slope, float eps, float* __restrict__ Y, int64_t ldy) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Lds& L = *reinterpret_cast<Lds*>(smem);
  stage_weights(L, w1, w2);
  rsx::Dropout drop;
  drop.seed = 0; drop.thresh = 0u; drop.scale = 1.f;
  const int64_t tiles = (N + kRows - 1) / kRows;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t base = t * kRows;
    for (int i = threadIdx.x; i < kRows * (kIn / 4); i += 256) {
      const int r = i / (kIn / 4), c4 = i % (kIn / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (base + r < N) v = reinterpret_cast<const float4*>(X + (base + r) * ldx)[c4];
      float* d = &L.x[r * LDX + 4 * c4];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    f32x16 f0, f1;
    tile_forward<false>(L, b1, b2, slope, eps, drop, 0, 0, f0, f1);
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (base + r < N) store_row_quarter(L, r, q, Y + (base + r) * ldy);
    __syncthreads();
  }
}

struct GradArgs {
  const float* U; int64_t ldu, n_users;
  const float* I; int64_t ldi, n_items;
  const int64_t* users; const int64_t* items; int64_t B;
  const float* w1; const float* b1; const float* w2; const float* b2; const float* ls;
  float slope, eps;
  rsx::Dropout drop;
  double* loss_part; float* slots;
  float* student; float* teacher; float* rows_out;
  int* flag;
};

__global__ __launch_bounds__(256) void distill_grads_k(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Lds& L = *reinterpret_cast<Lds*>(smem);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  stage_weights(L, a.w1, a.w2);
  const float els = expf(a.ls[0]);
  const float fB = (float)a.B;
  f32x16 dw1_0 = splat(0.f), dw1_1 = dw1_0, dw2_0 = dw1_0, dw2_1 = dw1_0;
  float db = 0.f;            // db1[tid], tid < 128
  float db2 = 0.f;           // db2[tid], tid < 64
  double loss_acc = 0.0, dls_acc = 0.0;   // wave 0
  const int64_t tiles = (a.B + kPairs - 1) / kPairs;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t k0 = t * kPairs;
    // gather: 16 lanes per row, tile rows [0, 32) the users, [32, 64) the items of pairs k0 ..
    for (int i = tid; i < kRows * (kIn / 4); i += 256) {
      const int r = i / (kIn / 4), c4 = i % (kIn / 4);
      const int64_t k = k0 + (r & (kPairs - 1));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      bool ok = false;
      if (k < a.B) {
        const int64_t u = a.users[k], it = a.items[k];
        ok = u >= 0 && u < a.n_users && it >= 0 && it < a.n_items;
        if (ok)
          v = r < kPairs ? reinterpret_cast<const float4*>(a.U + u * a.ldu)[c4]
                         : reinterpret_cast<const float4*>(a.I + it * a.ldi)[c4];
        else if (c4 == 0 && r < kPairs)
          *a.flag = 1;
      }
      float* d = &L.x[r * LDX + 4 * c4];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      if (c4 == 0 && r < kPairs) L.valid[r] = ok;
    }
    __syncthreads();
    f32x16 fac0, fac1;
    tile_forward<true>(L, a.b1, a.b2, a.slope, a.eps, a.drop, k0, a.B + k0, fac0, fac1);
    if (a.rows_out) {
      const int r = tid >> 2, q = tid & 3;
      const int64_t k = k0 + (r & (kPairs - 1));
      if (k < a.B) store_row_quarter(L, r, q, a.rows_out + (r < kPairs ? k : a.B + k) * kOut);
      __syncthreads();   // Y is overwritten with dZ below
    }
    {
      // eight lanes per pair, 8 columns each: cos and the teacher's dot, then dZ over Y in place
      const int k = tid >> 3, sub = tid & 7;
      float* yu = &L.z[k * LDX + 8 * sub];
      float* yi = &L.z[(kPairs + k) * LDX + 8 * sub];
      const float* xu = &L.x[k * LDX + 8 * sub];
      const float* xi = &L.x[(kPairs + k) * LDX + 8 * sub];
      float cs = 0.f, tt = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        cs = fmaf(yu[e], yi[e], cs);
        tt = fmaf(xu[e], xi[e], tt);
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        cs += __shfl_xor(cs, o, 64);
        tt += __shfl_xor(tt, o, 64);
      }
      const bool ok = L.valid[k] != 0;
      const float s = cs * els;
      const float d = s - tt;
      const float ds = ok ? 2.f * d / fB : 0.f;
      const float g = ds * els, gc = g * cs;
      const float nu = L.nrm[k], ni = L.nrm[kPairs + k];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float u = yu[e], v = yi[e];
        yu[e] = nu < 0.f ? g * v / a.eps : (g * v - u * gc) / nu;
        yi[e] = ni < 0.f ? g * u / a.eps : (g * u - v * gc) / ni;
      }
      if (sub == 0) {
        L.err[k] = ok ? d * d : 0.f;
        L.dls[k] = ds * s;
        if (k0 + k < a.B) {
          if (a.student) a.student[k0 + k] = s;
          if (a.teacher) a.teacher[k0 + k] = tt;
        }
      }
    }
    __syncthreads();
    if (w == 0) {   // the tile's 32 terms by a fixed shuffle tree, in double
      loss_acc += rsx::wave_sum_width(lane < kPairs ? (double)L.err[lane & (kPairs - 1)] : 0.0, 64);
      dls_acc += rsx::wave_sum_width(lane < kPairs ? (double)L.dls[lane & (kPairs - 1)] : 0.0, 64);
    }
    // dW2 += dZ^T H, db2 += column sums of dZ
    mma_2a<1, LDX, LDH, 1, kRows>(dw2_0, dw2_1, L.z, L.z + 32, L.h + 32 * w);
    if (tid < kOut)
      for (int r = 0; r < kRows; ++r) db2 += L.z[r * LDX + tid];
    // dH = dZ W2 on the tiles of P, dP = dH * factor
    f32x16 dp0 = splat(0.f), dp1 = dp0;
    mma_2a<LDX, 1, LDH, 1, kOut>(dp0, dp1, L.z, L.z + 32 * LDX, L.w2 + 32 * w);
    __syncthreads();   // every wave has read H
    {
      const int c = 32 * w + (lane & 31);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = crow(reg, lane);
        L.h[r * LDH + c] = dp0[reg] * fac0[reg];
        L.h[(32 + r) * LDH + c] = dp1[reg] * fac1[reg];
      }
    }
    __syncthreads();
    // dW1 += dP^T X, db1 += column sums of dP
    mma_2b<1, LDH, LDX, 1, kRows>(dw1_0, dw1_1, L.h + 32 * w, L.x, L.x + 32);
    if (tid < kHid)
      for (int r = 0; r < kRows; ++r) db += L.h[r * LDH + tid];
    __syncthreads();
  }
  float* slot = a.slots + (int64_t)blockIdx.x * kNP;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = crow(reg, lane), j = lane & 31;
    slot[kOffW1 + (32 * w + r) * kIn + j] = dw1_0[reg];
    slot[kOffW1 + (32 * w + r) * kIn + 32 + j] = dw1_1[reg];
    slot[kOffW2 + r * kHid + 32 * w + j] = dw2_0[reg];
    slot[kOffW2 + (32 + r) * kHid + 32 * w + j] = dw2_1[reg];
  }
  if (tid < kHid) slot[kOffB1 + tid] = db;
  if (tid < kOut) slot[kOffB2 + tid] = db2;
  if (tid == 0) {
    slot[kOffLs] = (float)dls_acc;
    a.loss_part[blockIdx.x] = loss_acc;
  }
}

struct ApplyArgs {
  const double* loss_part; const float* slots; int n_slots; int64_t B;
  float* p[5];   // W1, b1, W2, b2, logit_scale
  float* m; float* v; float* grads; double* loss;
  int update;
  double lr, b1, b2, eps;
  float step;
};

// element e of the flat parameter vector: its slots added in slot order, then (optionally) Adam; small
// workgroups, so that the 16,577 serial sums spread over every CU
constexpr int kApplyThreads = 64;
__global__ __launch_bounds__(kApplyThreads) void distill_apply_k(ApplyArgs a) {
  const int e = blockIdx.x * kApplyThreads + threadIdx.x;
  if (e == 0 && a.loss) {
    double s = 0.0;
    for (int k = 0; k < a.n_slots; ++k) s += a.loss_part[k];
    a.loss[0] = s / (double)a.B;
  }
  if (e >= kNP) return;
  float g = 0.f;
#pragma unroll 32   // the loads of 32 slots in flight; the adds stay in slot order
  for (int k = 0; k < a.n_slots; ++k) g += a.slots[(int64_t)k * kNP + e];
  if (a.grads) a.grads[e] = g;
  if (!a.update) return;
  float* pp = e < kOffB1 ? a.p[0] + e : e < kOffW2 ? a.p[1] + (e - kOffB1) : e < kOffB2 ? a.p[2] + (e - kOffW2)
              : e < kOffLs ? a.p[3] + (e - kOffB2) : a.p[4];
  const double bc1 = 1.0 - pow(a.b1, (double)a.step);
  const double bc2_sqrt = sqrt(1.0 - pow(a.b2, (double)a.step));
  float p = *pp, m = a.m[e], v = a.v[e];
  rsx::adam_elem(p, g, m, v, 1.f, a.lr, 0.0, a.b1, a.b2, a.eps, a.lr / bc1, bc2_sqrt);
  *pp = p;
  a.m[e] = m;
  a.v[e] = v;
}

using rsx::aligned16;

template <typename K>
int raise_lds(K kernel, const char* fn) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)sizeof(Lds));
  if (e != hipSuccess) {
    rsx::set_error("%s: cannot raise the LDS limit: %s", fn, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace

RSX_API int64_t rsx_distill_rows_per_workgroup(void) { return kPairs; }

RSX_API int64_t rsx_distill_slots(int64_t B) {
  if (B < 1) return 0;
  const int64_t tiles = (B + kPairs - 1) / kPairs;
  return tiles < kMaxSlots ? tiles : kMaxSlots;
}

RSX_API int64_t rsx_distill_workspace_bytes(int64_t B) {
  return rsx_distill_slots(B) * (int64_t)(sizeof(double) + kNP * sizeof(float));
}

RSX_API int rsx_magnitude_encode(const float* X, int64_t ldx, int64_t N, const float* w1, const float* b1,
                                 const float* w2, const float* b2, float slope, float eps, float* Y, int64_t ldy,
                                 void* stream) {
  RSX_ARG(N >= 0, "negative size");
  RSX_ARG(eps > 0.f, "eps must be positive");
  if (N == 0) return 0;
  RSX_ARG(X && w1 && b1 && w2 && b2 && Y, "null tensor");
  RSX_ARG(ldx >= kIn && ldx % 4 == 0 && ldy >= kOut && ldy % 4 == 0, "bad leading dimensions");
  RSX_ARG(aligned16(X) && aligned16(Y) && aligned16(w1) && aligned16(w2), "rows must be 16-byte aligned");
  static const int attr = raise_lds(encode_k, "rsx_magnitude_encode");
  if (attr) return attr;
  const int64_t tiles = (N + kRows - 1) / kRows;
  const int64_t grid = tiles < rsx::cu_count() ? tiles : rsx::cu_count();
  hipLaunchKernelGGL(encode_k, dim3((unsigned)grid), dim3(256), sizeof(Lds), (hipStream_t)stream, X, ldx, N, w1, b1,
                     w2, b2, slope, eps, Y, ldy);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_distill_grads(const float* user_table, int64_t ldu, int64_t n_users, const float* item_table,
                              int64_t ldi, int64_t n_items, const int64_t* users, const int64_t* items, int64_t B,
                              const float* w1, const float* b1, const float* w2, const float* b2,
                              const float* logit_scale, float slope, float p_drop, uint64_t seed, float eps, void* ws,
                              int64_t ws_bytes, float* student_scores, float* teacher_scores, float* rows_out,
                              int32_t* flag, void* stream) {
  RSX_ARG(B >= 1, "B must be at least 1");
  RSX_ARG(n_users >= 0 && n_items >= 0, "negative size");
  RSX_ARG(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0, 1)");
  RSX_ARG(eps > 0.f, "eps must be positive");
  RSX_ARG(user_table && item_table && users && items && w1 && b1 && w2 && b2 && logit_scale && flag, "null tensor");
  RSX_ARG(ldu >= kIn && ldu % 4 == 0 && ldi >= kIn && ldi % 4 == 0, "bad leading dimensions");
  RSX_ARG(aligned16(user_table) && aligned16(item_table) && aligned16(w1) && aligned16(w2) && aligned16(rows_out),
          "rows must be 16-byte aligned");
  RSX_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= rsx_distill_workspace_bytes(B), "workspace too small");
  static const int attr = raise_lds(distill_grads_k, "rsx_distill_grads");
  if (attr) return attr;
  const int64_t slots = rsx_distill_slots(B);
  GradArgs a;
  a.U = user_table; a.ldu = ldu; a.n_users = n_users;
  a.I = item_table; a.ldi = ldi; a.n_items = n_items;
  a.users = users; a.items = items; a.B = B;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.ls = logit_scale;
  a.slope = slope; a.eps = eps;
  a.drop = rsx::make_dropout(p_drop, seed);
  a.loss_part = (double*)ws;
  a.slots = (float*)((double*)ws + slots);
  a.student = student_scores; a.teacher = teacher_scores; a.rows_out = rows_out;
  a.flag = flag;
  hipLaunchKernelGGL(distill_grads_k, dim3((unsigned)slots), dim3(256), sizeof(Lds), (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_distill_apply(const void* ws, int64_t ws_bytes, int64_t B, float* w1, float* b1, float* w2, float* b2,
                              float* logit_scale, float* exp_avg, float* exp_avg_sq, float* grads, double* loss,
                              int update, double lr, double beta1, double beta2, double eps, int64_t step,
                              void* stream) {
  RSX_ARG(B >= 1, "B must be at least 1");
  RSX_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= rsx_distill_workspace_bytes(B), "workspace too small");
  if (update) {
    RSX_ARG(w1 && b1 && w2 && b2 && logit_scale && exp_avg && exp_avg_sq, "null tensor");
    RSX_ARG(step >= 1, "step counts from 1");
  }
  const int64_t slots = rsx_distill_slots(B);
  ApplyArgs a;
  a.loss_part = (const double*)ws;
  a.slots = (const float*)((const double*)ws + slots);
  a.n_slots = (int)slots; a.B = B;
  a.p[0] = w1; a.p[1] = b1; a.p[2] = w2; a.p[3] = b2; a.p[4] = logit_scale;
  a.m = exp_avg; a.v = exp_avg_sq; a.grads = grads; a.loss = loss;
  a.update = update ? 1 : 0;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.step = (float)step;
  hipLaunchKernelGGL(distill_apply_k, dim3((kNP + kApplyThreads - 1) / kApplyThreads), dim3(kApplyThreads), 0,
                     (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}
