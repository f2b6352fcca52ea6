// LightGCL's whole-graph passes (gnn_model/v1_lightgcl.py:163-186), fp32, no float atomics, every sum
// in a fixed order (bit-reproducible from run to run):
//   * rsx_spmm_norm       Y = alpha (R + A^ X), A^ = diag(dinv) B diag(dinv) over the binary CSR B:
//                         torch.sparse.mm(self.adj, x) of :171 and, A^ being symmetric, its backward
//   * rsx_lowrank_proj    P = V^T X                      torch.matmul(self.V.t(), x_g) of :180
//   * rsx_lowrank_update  Y += V W                       torch.matmul(self.U, temp) of :182
// Every row is D fp32 owned by D/4 lanes (one float4 each, a 256-B or 512-B row per lane group).
#include "rsx_common.h"
#include "recsys_amd.h"

namespace {

// Neighbour lists longer than this are cut into chunks of this many neighbours, each summed on its
// own; a row's sum is its chunk sums added in chunk order (the full-graph form sums the chunks of the
// long rows in separate lane groups, the listed-rows form one after the other: the same arithmetic).
constexpr int kChunk = 512;
constexpr int kRowsPerWG = 64;    // contiguous destination rows of one workgroup (spmm)
constexpr int kProjRows = 256;    // rows of one lowrank_proj tile
constexpr int kProjMaxSlots = 512;
constexpr int kMaxQ = 8;

template <int D>
struct Geo {
  static constexpr int LPR = D / 4;        // lanes per row
  static constexpr int RPW = 64 / LPR;     // rows per wave
  static constexpr int NG = 256 / LPR;     // lane groups per workgroup
};

__device__ __forceinline__ void fma4(float4& a, float s, const float4& x) {
  a.x = fmaf(s, x.x, a.x); a.y = fmaf(s, x.y, a.y); a.z = fmaf(s, x.z, a.z); a.w = fmaf(s, x.w, a.w);
}

// sum_{k in [k0, k1)} dinv[col[k]] * X[col[k]] in CSR order, this lane's float4 column c: eight
// index loads, then eight row loads in flight before the first add
__device__ __forceinline__ float4 chunk_sum(const float* __restrict__ X, int64_t ldx, const int32_t* __restrict__ col,
                                            const float* __restrict__ dinv, int64_t k0, int64_t k1, int c) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t k = k0; k < k1; k += 8) {
    int32_t j[8];
    float s[8];
    float4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) j[i] = k + i < k1 ? col[k + i] : -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s[i] = j[i] >= 0 ? dinv[j[i]] : 0.f;
      x[i] = j[i] >= 0 ? reinterpret_cast<const float4*>(X + (int64_t)j[i] * ldx)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (j[i] >= 0) fma4(acc, s[i], x[i]);
  }
  return acc;
}

__device__ __forceinline__ float4 epilogue(float4 sum, float dr, const float* __restrict__ R, int64_t ldr, int64_t r,
                                           float alpha, int c) {
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
  if (R) y = reinterpret_cast<const float4*>(R + r * ldr)[c];
  fma4(y, dr, sum);
  y.x *= alpha; y.y *= alpha; y.z *= alpha; y.w *= alpha;
  return y;
}

// One lane group per destination. LIST: destinations rows[i] into the dense Y[i] (a row outside
// [0, n) gives a zero row), long rows summed chunk after chunk by the one lane group; otherwise every
// row of the graph, workgroup b the rows [64 b, 64 b + 64), long rows left to the two kernels below.
template <int D, bool LIST>
__global__ __launch_bounds__(256) void spmm_rows_k(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  const float* __restrict__ dinv, int64_t n,
                                                  const float* __restrict__ X, int64_t ldx,
                                                  const float* __restrict__ R, int64_t ldr, float alpha,
                                                  const int64_t* __restrict__ rows, int64_t n_out,
                                                  float* __restrict__ Y, int64_t ldy) {
  constexpr int LPR = Geo<D>::LPR, NG = Geo<D>::NG;
  const int g = threadIdx.x / LPR, c = threadIdx.x % LPR;
  const int64_t base = (int64_t)blockIdx.x * kRowsPerWG;
  for (int i0 = 0; i0 < kRowsPerWG; i0 += NG) {
    const int64_t i = base + i0 + g;
    if (i >= n_out) continue;
    const int64_t r = LIST ? rows[i] : i;
    float4* out = reinterpret_cast<float4*>(Y + i * ldy) + c;
    if (LIST && (r < 0 || r >= n)) {
      *out = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int64_t k0 = row_ptr[r], k1 = row_ptr[r + 1];
    float4 sum;
    if (k1 - k0 <= kChunk) {
      sum = chunk_sum(X, ldx, col, dinv, k0, k1, c);
    } else {
      if (!LIST) continue;
      sum = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t k = k0; k < k1; k += kChunk) {
        const float4 p = chunk_sum(X, ldx, col, dinv, k, k + kChunk < k1 ? k + kChunk : k1, c);
        sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
      }
    }
    *out = epilogue(sum, dinv[r], R, ldr, r, alpha, c);
  }
}

// chunk ch of the plan -> part[ch] = its neighbours' sum
template <int D>
__global__ __launch_bounds__(256) void spmm_chunks_k(const int32_t* __restrict__ col, const float* __restrict__ dinv,
                                                    const float* __restrict__ X, int64_t ldx,
                                                    const int64_t* __restrict__ chunk_beg,
                                                    const int64_t* __restrict__ chunk_end, int64_t n_chunks,
                                                    float* __restrict__ part) {
  constexpr int LPR = Geo<D>::LPR, NG = Geo<D>::NG;
  const int g = threadIdx.x / LPR, c = threadIdx.x % LPR;
  const int64_t ch = (int64_t)blockIdx.x * NG + g;
  if (ch >= n_chunks) return;
  const float4 s = chunk_sum(X, ldx, col, dinv, chunk_beg[ch], chunk_end[ch], c);
  reinterpret_cast<float4*>(part + ch * D)[c] = s;
}

// long row l -> Y[long_rows[l]] from its partial slots [part_off[l], part_off[l+1]) in slot order
template <int D>
__global__ __launch_bounds__(256) void spmm_long_k(const float* __restrict__ dinv, const float* __restrict__ R,
                                                  int64_t ldr, float alpha, const int64_t* __restrict__ long_rows,
                                                  const int64_t* __restrict__ part_off, int64_t n_long,
                                                  const float* __restrict__ part, float* __restrict__ Y, int64_t ldy) {
  constexpr int LPR = Geo<D>::LPR, NG = Geo<D>::NG;
  const int g = threadIdx.x / LPR, c = threadIdx.x % LPR;
  const int64_t l = (int64_t)blockIdx.x * NG + g;
  if (l >= n_long) return;
  const int64_t r = long_rows[l];
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t s = part_off[l]; s < part_off[l + 1]; ++s) {
    const float4 p = reinterpret_cast<const float4*>(part + s * D)[c];
    sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
  }
  reinterpret_cast<float4*>(Y + r * ldy)[c] = epilogue(sum, dinv[r], R, ldr, r, alpha, c);
}

// P = V^T X, first pass: workgroup b sums the row tiles b, b + G, ... (256 rows each; lane group g the
// rows g, g + NG, ... of a tile), adds its lane groups' sums in group order through LDS and stores
// slot[b] [q, D].
template <int D>
__global__ __launch_bounds__(256) void lowrank_proj_k(const float* __restrict__ V, int64_t ldv,
                                                     const float* __restrict__ X, int64_t ldx, int64_t n, int q,
                                                     float* __restrict__ slots) {
  constexpr int LPR = Geo<D>::LPR, NG = Geo<D>::NG;
  __shared__ __attribute__((aligned(16))) float s_acc[NG][kMaxQ][D];
  const int g = threadIdx.x / LPR, c = threadIdx.x % LPR;
  float4 acc[kMaxQ];
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t t0 = (int64_t)blockIdx.x * kProjRows; t0 < n; t0 += (int64_t)gridDim.x * kProjRows) {
    for (int i = g; i < kProjRows; i += NG) {
      const int64_t r = t0 + i;
      if (r >= n) break;
      const float4 x = reinterpret_cast<const float4*>(X + r * ldx)[c];
      const float* v = V + r * ldv;
#pragma unroll
      for (int j = 0; j < kMaxQ; ++j)
        if (j < q) fma4(acc[j], v[j], x);
    }
  }
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j)
    if (j < q) reinterpret_cast<float4*>(&s_acc[g][j][0])[c] = acc[j];
  __syncthreads();
  float* out = slots + (int64_t)blockIdx.x * q * D;
  for (int e = threadIdx.x; e < q * D; e += 256) {
    const int j = e / D, d = e % D;
    float s = 0.f;
    for (int k = 0; k < NG; ++k) s += s_acc[k][j][d];
    out[e] = s;
  }
}

// second pass: P[e] = the slots' element e added in slot order
__global__ __launch_bounds__(64) void lowrank_proj_sum_k(const float* __restrict__ slots, int n_slots, int qd,
                                                        float* __restrict__ P) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= qd) return;
  float s = 0.f;
  for (int k = 0; k < n_slots; ++k) s += slots[(int64_t)k * qd + e];
  P[e] = s;
}

// Y[r] += sum_j V[r][j] W[j], j ascending
template <int D>
__global__ __launch_bounds__(256) void lowrank_update_k(const float* __restrict__ V, int64_t ldv,
                                                       const float* __restrict__ W, int64_t n, int q,
                                                       float* __restrict__ Y, int64_t ldy) {
  constexpr int LPR = Geo<D>::LPR, NG = Geo<D>::NG;
  const int g = threadIdx.x / LPR, c = threadIdx.x % LPR;
  float4 w[kMaxQ];
#pragma unroll
  for (int j = 0; j < kMaxQ; ++j)
    w[j] = j < q ? reinterpret_cast<const float4*>(W + j * D)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r = (int64_t)blockIdx.x * NG + g; r < n; r += (int64_t)gridDim.x * NG) {
    float4* p = reinterpret_cast<float4*>(Y + r * ldy) + c;
    float4 y = *p;
    const float* v = V + r * ldv;
#pragma unroll
    for (int j = 0; j < kMaxQ; ++j)
      if (j < q) fma4(y, v[j], w[j]);
    *p = y;
  }
}

int64_t proj_slots(int64_t n) {
  const int64_t tiles = (n + kProjRows - 1) / kProjRows;
  return tiles < 1 ? 1 : (tiles > kProjMaxSlots ? kProjMaxSlots : tiles);
}

using rsx::aligned16;

}  // namespace

RSX_API int64_t rsx_spmm_norm_chunk_len(void) { return kChunk; }
RSX_API int64_t rsx_spmm_norm_rows_per_workgroup(void) { return kRowsPerWG; }
RSX_API int64_t rsx_lowrank_rows_per_workgroup(void) { return kProjRows; }

RSX_API int64_t rsx_spmm_norm_workspace_bytes(int64_t n_chunks, int64_t D) {
  return n_chunks > 0 && D > 0 ? n_chunks * D * (int64_t)sizeof(float) : 0;
}

RSX_API int rsx_spmm_norm(const int64_t* row_ptr, const int32_t* col, const float* dinv, int64_t n, const float* X,
                          int64_t ldx, const float* R, int64_t ldr, int64_t D, float alpha, const int64_t* rows,
                          int64_t n_rows, const int64_t* long_rows, const int64_t* part_off, const int64_t* chunk_beg,
                          const int64_t* chunk_end, int64_t n_long, int64_t n_chunks, void* ws, int64_t ws_bytes,
                          float* Y, int64_t ldy, void* stream) {
  RSX_ARG(D == 64 || D == 128, "D must be 64 or 128");
  RSX_ARG(n >= 0 && n_rows >= 0 && n_long >= 0 && n_chunks >= 0, "negative size");
  RSX_ARG(rows || n_rows == 0, "n_rows without rows");
  const int64_t n_out = rows ? n_rows : n;
  if (n_out == 0) return 0;
  RSX_ARG(row_ptr && dinv && X && Y, "null tensor");
  RSX_ARG(ldx >= D && ldx % 4 == 0 && ldy >= D && ldy % 4 == 0 && (!R || (ldr >= D && ldr % 4 == 0)),
          "bad leading dimensions");
  RSX_ARG(aligned16(X) && aligned16(Y) && aligned16(R), "rows must be 16-byte aligned");
  RSX_ARG(X != Y, "Y must not alias X");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((n_out + kRowsPerWG - 1) / kRowsPerWG);
  const bool list = rows != nullptr;
  const bool plan = !list && n_long > 0;
  if (plan) {
    RSX_ARG(long_rows && part_off && chunk_beg && chunk_end && n_chunks > 0, "long rows without a chunk plan");
    RSX_ARG(ws && aligned16(ws) && ws_bytes >= rsx_spmm_norm_workspace_bytes(n_chunks, D), "workspace too small");
  }
#define RSX_SP(DD)                                                                                                    \
  if (D == DD) {                                                                                                      \
    if (list)                                                                                                         \
      hipLaunchKernelGGL((spmm_rows_k<DD, true>), dim3(grid), dim3(256), 0, st, row_ptr, col, dinv, n, X, ldx, R, ldr, \
                         alpha, rows, n_out, Y, ldy);                                                                 \
    else                                                                                                              \
      hipLaunchKernelGGL((spmm_rows_k<DD, false>), dim3(grid), dim3(256), 0, st, row_ptr, col, dinv, n, X, ldx, R,    \
                         ldr, alpha, rows, n_out, Y, ldy);                                                            \
    if (plan) {                                                                                                       \
      constexpr int NG = Geo<DD>::NG;                                                                                 \
      hipLaunchKernelGGL(spmm_chunks_k<DD>, dim3((unsigned)((n_chunks + NG - 1) / NG)), dim3(256), 0, st, col, dinv,  \
                         X, ldx, chunk_beg, chunk_end, n_chunks, (float*)ws);                                         \
      hipLaunchKernelGGL(spmm_long_k<DD>, dim3((unsigned)((n_long + NG - 1) / NG)), dim3(256), 0, st, dinv, R, ldr,   \
                         alpha, long_rows, part_off, n_long, (const float*)ws, Y, ldy);                               \
    }                                                                                                                 \
  }
  RSX_SP(64) RSX_SP(128)
#undef RSX_SP
  RSX_LAUNCHED();
  return 0;
}

RSX_API int64_t rsx_lowrank_proj_workspace_bytes(int64_t n, int64_t q, int64_t D) {
  return proj_slots(n) * q * D * (int64_t)sizeof(float);
}

RSX_API int rsx_lowrank_proj(const float* V, int64_t ldv, const float* X, int64_t ldx, int64_t n, int64_t q, int64_t D,
                             void* ws, int64_t ws_bytes, float* P, void* stream) {
  RSX_ARG(D == 64 || D == 128, "D must be 64 or 128");
  RSX_ARG(q >= 1 && q <= kMaxQ, "q must be 1..8");
  RSX_ARG(n >= 0, "negative size");
  RSX_ARG(P, "null tensor");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e = hipMemsetAsync(P, 0, q * D * sizeof(float), st);
    if (e != hipSuccess) {
      rsx::set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
      return (int)e;
    }
    return 0;
  }
  RSX_ARG(V && X && ws, "null tensor");
  RSX_ARG(ldv >= q && ldx >= D && ldx % 4 == 0 && aligned16(X), "bad leading dimensions");
  RSX_ARG(ws_bytes >= rsx_lowrank_proj_workspace_bytes(n, q, D), "workspace too small");
  const int slots = (int)proj_slots(n);
  const int qd = (int)(q * D);
  if (D == 64)
    hipLaunchKernelGGL(lowrank_proj_k<64>, dim3(slots), dim3(256), 0, st, V, ldv, X, ldx, n, (int)q, (float*)ws);
  else
    hipLaunchKernelGGL(lowrank_proj_k<128>, dim3(slots), dim3(256), 0, st, V, ldv, X, ldx, n, (int)q, (float*)ws);
  hipLaunchKernelGGL(lowrank_proj_sum_k, dim3((qd + 63) / 64), dim3(64), 0, st, (const float*)ws, slots, qd, P);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_lowrank_update(const float* V, int64_t ldv, const float* W, int64_t n, int64_t q, int64_t D, float* Y,
                               int64_t ldy, void* stream) {
  RSX_ARG(D == 64 || D == 128, "D must be 64 or 128");
  RSX_ARG(q >= 1 && q <= kMaxQ, "q must be 1..8");
  RSX_ARG(n >= 0, "negative size");
  if (n == 0) return 0;
  RSX_ARG(V && W && Y, "null tensor");
  RSX_ARG(ldv >= q && ldy >= D && ldy % 4 == 0 && aligned16(Y) && aligned16(W), "bad leading dimensions");
  hipStream_t st = (hipStream_t)stream;
  const int64_t ng = D == 64 ? Geo<64>::NG : Geo<128>::NG;
  int64_t grid = (n + ng - 1) / ng;
  if (grid > 8192) grid = 8192;
  if (D == 64)
    hipLaunchKernelGGL(lowrank_update_k<64>, dim3((unsigned)grid), dim3(256), 0, st, V, ldv, W, n, (int)q, Y, ldy);
  else
    hipLaunchKernelGGL(lowrank_update_k<128>, dim3((unsigned)grid), dim3(256), 0, st, V, ldv, W, n, (int)q, Y, ldy);
  RSX_LAUNCHED();
  return 0;
}
