// DCN-V2 cross network of the reference's second neural reranker (temp_model/ranker_skelet.py:
// 239-272, RankingModel :274-357) fused with the cross half of its final head:
//
//   x_{l+1}[d] = x_0[d] * (<x_l, k_l> + b_l[d]) + x_l[d]      l = 0 .. L-1   (kernel k_l [D, 1])
//   head_part  = <x_L, w_head[0:D]>                            (final_head on cat(cross, deep))
//
// One wave per row: the row stays in registers (D/4 float4 over 64 lanes, D <= 512), every
// <x_l, k_l> is a wave reduction, and only head_part (and optionally x_L) is written. The
// deep half (two Linear + LayerNorm + GELU) runs on the token GEMMs and the LayerNorm kernel.
#include "rsx_common.h"

namespace {

constexpr int kMaxLayers = 8;

struct CArgs {
  const float* x;         // [B, ldx]
  int64_t ldx, B;
  int D, L;
  const float* k[kMaxLayers];
  const float* b[kMaxLayers];
  const float* w_head;    // [D] or nullptr
  float* x_out;           // [B, D] or nullptr
  float* head_part;       // [B] or nullptr
};

template <int NC>  // float4 chunks per lane: D <= 256 * NC
__global__ __launch_bounds__(256) void crossnet_k(CArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int n4 = a.D / 4;
  for (int64_t r = wave_g; r < a.B; r += nw) {
    const float4* xr = reinterpret_cast<const float4*>(a.x + r * a.ldx);
    float4 x0[NC], xl[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = j * 64 + lane;
      x0[j] = c < n4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      xl[j] = x0[j];
    }
    for (int l = 0; l < a.L; ++l) {
      const float4* kk = reinterpret_cast<const float4*>(a.k[l]);
      const float4* bb = reinterpret_cast<const float4*>(a.b[l]);
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = j * 64 + lane;
        if (c < n4) {
          const float4 kv = kk[c];
          s += (xl[j].x * kv.x + xl[j].y * kv.y) + (xl[j].z * kv.z + xl[j].w * kv.w);
        }
      }
      s = rsx::wave_sum_width(s, 64);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = j * 64 + lane;
        if (c < n4) {
          const float4 bv = bb[c];
          xl[j].x = fmaf(x0[j].x, s + bv.x, xl[j].x);
          xl[j].y = fmaf(x0[j].y, s + bv.y, xl[j].y);
          xl[j].z = fmaf(x0[j].z, s + bv.z, xl[j].z);
          xl[j].w = fmaf(x0[j].w, s + bv.w, xl[j].w);
        }
      }
    }
    float h = 0.0f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = j * 64 + lane;
      if (c < n4) {
        if (a.x_out) reinterpret_cast<float4*>(a.x_out + r * a.D)[c] = xl[j];
        if (a.w_head) {
          const float4 wv = reinterpret_cast<const float4*>(a.w_head)[c];
          h += (xl[j].x * wv.x + xl[j].y * wv.y) + (xl[j].z * wv.z + xl[j].w * wv.w);
        }
      }
    }
    if (a.head_part) {
      h = rsx::wave_sum_width(h, 64);
      if (lane == 0) a.head_part[r] = h;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Backward of the sweep above. Per row, with G = dx_{l+1} and l going down:
//   db_l += G * x_0;  ds = <G, x_0>;  dk_l += ds * x_l;  dx_0 += G * (s_l + b_l);  G += ds * k_l
// and dx = dx_0 + G after layer 0. G starts as dhead[r] * w_head (+ dx_out[r]).
//
// Same shape as the forward: one wave per row, the row in registers. The x_l (and s_l) of a row
// are recomputed by the forward recurrence in the same sweep and stay in registers (L is a
// template parameter, so every per-layer array is indexed statically and the per-layer pointers
// of the argument block are read as scalars: no scratch, no flat loads); no [L, B, D]
// activation is stored, x is read once and dx written at most once. The parameter gradients are
// sums over rows: every wave accumulates its rows' (in grid-stride order) in registers, the
// workgroup's four waves are added through LDS one vector at a time in wave order, and the
// per-workgroup partials are added in workgroup order by crossnet_bwd_sum_k. No atomics.
constexpr int kBwdMaxBlocks = 1024;  // grid cap: bounds the partials (1024 * (2L+1) * D floats)

struct CBArgs {
  const float* x;         // [B, ldx]
  int64_t ldx, B;
  int D;
  const float* k[kMaxLayers];
  const float* b[kMaxLayers];
  const float* w_head;    // [D] or nullptr (with dhead)
  const float* dhead;     // [B] or nullptr
  const float* dx_out;    // [B, D] or nullptr
  float* dx;              // [B, D] or nullptr
  float* part;            // [gridDim.x, NV, D]: dk_0.., db_0.., dw_head
};

__device__ __forceinline__ float4 ld4(const float* p, int c, bool live) {
  return live ? reinterpret_cast<const float4*>(p)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}
__device__ __forceinline__ void fma4(float4& acc, const float s, const float4 v) {
  acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y);
  acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}
__device__ __forceinline__ void fmul4(float4& acc, const float4 a, const float4 b) {
  acc.x = fmaf(a.x, b.x, acc.x); acc.y = fmaf(a.y, b.y, acc.y);
  acc.z = fmaf(a.z, b.z, acc.z); acc.w = fmaf(a.w, b.w, acc.w);
}

template <int NC, int L>
__global__ __launch_bounds__(256) void crossnet_bwd_k(CBArgs a) {
  constexpr int NL = L > 0 ? L : 1;   // no zero-length arrays
  constexpr int NV = 2 * L + 1;
  __shared__ float4 sRed[4][NC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + wave;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int n4 = a.D / 4;
  bool live[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) live[j] = j * 64 + lane < n4;

  float4 acc[NV][NC];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[v][j] = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int64_t r = wave_g; r < a.B; r += nw) {
    const float* xr = a.x + r * a.ldx;
    float4 xs[NL + 1][NC];   // x_0 .. x_L
    float s[NL];
#pragma unroll
    for (int j = 0; j < NC; ++j) xs[0][j] = ld4(xr, j * 64 + lane, live[j]);
#pragma unroll
    for (int l = 0; l < L; ++l) {   // the forward's arithmetic
      float t = 0.0f;
#pragma unroll
      for (int j = 0; j < NC; ++j) t += dot4(xs[l][j], ld4(a.k[l], j * 64 + lane, live[j]));
      t = rsx::wave_sum_width(t, 64);
      s[l] = t;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const float4 bv = ld4(a.b[l], j * 64 + lane, live[j]);
        xs[l + 1][j].x = fmaf(xs[0][j].x, t + bv.x, xs[l][j].x);
        xs[l + 1][j].y = fmaf(xs[0][j].y, t + bv.y, xs[l][j].y);
        xs[l + 1][j].z = fmaf(xs[0][j].z, t + bv.z, xs[l][j].z);
        xs[l + 1][j].w = fmaf(xs[0][j].w, t + bv.w, xs[l][j].w);
      }
    }
    float4 G[NC], d0[NC];
    const float g = a.dhead ? a.dhead[r] : 0.0f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = j * 64 + lane;
      G[j] = a.dx_out ? ld4(a.dx_out + r * a.D, c, live[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
      d0[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.dhead) {
        fma4(G[j], g, ld4(a.w_head, c, live[j]));
        fma4(acc[2 * L][j], g, xs[L][j]);
      }
    }
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
      float ds = 0.0f;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        fmul4(acc[L + l][j], G[j], xs[0][j]);
        ds += dot4(G[j], xs[0][j]);
      }
      ds = rsx::wave_sum_width(ds, 64);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int c = j * 64 + lane;
        fma4(acc[l][j], ds, xs[l][j]);
        if (a.dx) {
          const float4 bv = ld4(a.b[l], c, live[j]);
          d0[j].x = fmaf(G[j].x, s[l] + bv.x, d0[j].x);
          d0[j].y = fmaf(G[j].y, s[l] + bv.y, d0[j].y);
          d0[j].z = fmaf(G[j].z, s[l] + bv.z, d0[j].z);
          d0[j].w = fmaf(G[j].w, s[l] + bv.w, d0[j].w);
        }
        fma4(G[j], ds, ld4(a.k[l], c, live[j]));
      }
    }
    if (a.dx) {
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        if (live[j]) {
          float4 o;
          o.x = d0[j].x + G[j].x; o.y = d0[j].y + G[j].y; o.z = d0[j].z + G[j].z; o.w = d0[j].w + G[j].w;
          reinterpret_cast<float4*>(a.dx + r * a.D)[j * 64 + lane] = o;
        }
      }
    }
  }

  // the workgroup's partial of every vector: four waves through LDS, added in wave order
  const int nv = 2 * L + (a.dhead ? 1 : 0);
  float4* part = reinterpret_cast<float4*>(a.part) + (int64_t)blockIdx.x * nv * n4;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    if (v < nv) {   // uniform
#pragma unroll
      for (int j = 0; j < NC; ++j) sRed[wave][j * 64 + lane] = acc[v][j];
      __syncthreads();
      if ((int)threadIdx.x < n4) {
        const int c = threadIdx.x;   // n4 <= NC * 64 <= 128 < 256
        float4 t = sRed[0][c];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const float4 u = sRed[w][c];
          t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        part[(int64_t)v * n4 + c] = t;
      }
      __syncthreads();
    }
  }
}

struct CSArgs {
  const float* part;   // [blocks, nv, D]
  int blocks, nv, n4;
  float* out[2 * kMaxLayers + 1];   // dk_0.., db_0.., dw_head
};

// One workgroup per (16 float4 columns, vector): thread (split, col) adds its contiguous run of
// workgroup partials in order, thread (0, col) adds the 16 runs in order.
__global__ __launch_bounds__(256) void crossnet_bwd_sum_k(CSArgs a) {
  __shared__ float4 sRun[16][16];
  const int col = threadIdx.x & 15, split = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + col, v = blockIdx.y;
  const int per = (a.blocks + 15) / 16;
  const int b0 = split * per, b1 = b0 + per < a.blocks ? b0 + per : a.blocks;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < a.n4) {
    const float4* p = reinterpret_cast<const float4*>(a.part) + (int64_t)v * a.n4 + c;
    for (int b = b0; b < b1; ++b) {
      const float4 u = p[(int64_t)b * a.nv * a.n4];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
  }
  sRun[split][col] = t;
  __syncthreads();
  if (split != 0 || c >= a.n4) return;
  t = sRun[0][col];
  for (int q = 1; q < 16; ++q) {
    const float4 u = sRun[q][col];
    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
  }
  float* out = nullptr;
#pragma unroll
  for (int i = 0; i < 2 * kMaxLayers + 1; ++i)
    if (i == v) out = a.out[i];   // v is uniform: scalar selects, no indexed read of the argument block
  reinterpret_cast<float4*>(out)[c] = t;
}

inline int64_t bwd_blocks(int64_t B, int max_blocks) {
  int64_t cap = max_blocks > 0 && max_blocks < kBwdMaxBlocks ? max_blocks : kBwdMaxBlocks;
  const int64_t blocks = (B + 3) / 4;
  return blocks < cap ? blocks : cap;
}

using BwdFn = void (*)(CBArgs);

template <int NC>
BwdFn bwd_fn(int L) {
  switch (L) {
#define RSX_CB_CASE(l) case l: return crossnet_bwd_k<NC, l>;
    RSX_CB_CASE(0) RSX_CB_CASE(1) RSX_CB_CASE(2) RSX_CB_CASE(3) RSX_CB_CASE(4)
    RSX_CB_CASE(5) RSX_CB_CASE(6) RSX_CB_CASE(7) RSX_CB_CASE(8)
#undef RSX_CB_CASE
  }
  return nullptr;
}

// Workgroups of this instance that the device holds at once (its register count sets that: 3 per CU
// at L = 3, D > 256). The sweep is bound by the latency of its chained wave reductions, so a grid of
// exactly the resident workgroups, each striding over more rows, beats a larger one whose second
// round leaves most of the machine idle. Queried once per instance; the cap when the query fails.
int64_t bwd_resident_blocks(BwdFn fn, int nc, int L) {
  static int cached[2][kMaxLayers + 1] = {};
  int& c = cached[nc - 1][L];
  if (c == 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), 256, 0) != hipSuccess ||
        per_cu < 1) {
      (void)hipGetLastError();
      c = kBwdMaxBlocks;
    } else {
      c = per_cu * rsx::cu_count();
    }
  }
  return c;
}

using rsx::aligned16;

}  // namespace

RSX_API int64_t rsx_crossnet_bwd_workspace_bytes(int64_t B, int D, int L, int max_blocks) {
  if (B < 0 || D < 4 || D > 512 || D % 4 || L < 0 || L > kMaxLayers) return -1;
  return bwd_blocks(B, max_blocks) * (2 * L + 1) * (int64_t)D * (int64_t)sizeof(float);
}

RSX_API int rsx_crossnet_bwd(const float* x, int64_t ldx, int64_t B, int D, int L, const float* const* kernels,
                             const float* const* biases, const float* w_head, const float* dhead,
                             const float* dx_out, float* const* dk, float* const* db, float* dw_head, float* dx,
                             void* ws, int64_t ws_bytes, int max_blocks, void* stream) {
  RSX_ARG(D % 4 == 0 && D >= 4 && D <= 512, "D must be a multiple of 4 in [4, 512]");
  RSX_ARG(L >= 0 && L <= kMaxLayers, "L must be in [0, 8]");
  RSX_ARG(ldx >= D && ldx % 4 == 0, "bad ldx");
  RSX_ARG(B >= 0, "negative row count");
  RSX_ARG(max_blocks >= 0, "max_blocks must be >= 0 (0: the default cap)");
  if (B == 0) return 0;   // nothing is written: the caller zeroes the gradients of an empty batch
  RSX_ARG((w_head != nullptr) == (dhead != nullptr) && (dhead != nullptr) == (dw_head != nullptr),
          "w_head, dhead and dw_head go together");
  RSX_ARG(dhead || dx_out, "no upstream gradient: give (w_head, dhead) and / or dx_out");
  RSX_ARG(x && (L == 0 || (kernels && biases && dk && db)), "null tensor");
  CBArgs a = {};
  CSArgs s = {};
  for (int l = 0; l < L; ++l) {
    RSX_ARG(kernels[l] && biases[l] && dk[l] && db[l], "null layer kernel / bias / gradient");
    RSX_ARG(aligned16(kernels[l]) && aligned16(biases[l]) && aligned16(dk[l]) && aligned16(db[l]),
            "layer kernels, biases and their gradients must be 16-byte aligned");
    a.k[l] = kernels[l]; a.b[l] = biases[l];
    s.out[l] = dk[l]; s.out[L + l] = db[l];
  }
  s.out[2 * L] = dw_head;
  RSX_ARG(aligned16(x) && aligned16(w_head) && aligned16(dx_out) && aligned16(dw_head) && aligned16(dx) && aligned16(ws),
          "x, w_head, dx_out, dw_head, dx and ws must be 16-byte aligned");
  const int nv = 2 * L + (dhead ? 1 : 0);
  int64_t blocks = bwd_blocks(B, max_blocks);   // what the workspace is sized for; the grid may be smaller
  RSX_ARG(nv == 0 || (ws && ws_bytes >= blocks * nv * (int64_t)D * (int64_t)sizeof(float)),
          "workspace too small");
  const int nc = D <= 256 ? 1 : 2;
  const BwdFn fn = nc == 1 ? bwd_fn<1>(L) : bwd_fn<2>(L);
  const int64_t resident = bwd_resident_blocks(fn, nc, L);
  if (blocks > resident) blocks = resident;
  a.x = x; a.ldx = ldx; a.B = B; a.D = D;
  a.w_head = w_head; a.dhead = dhead; a.dx_out = dx_out; a.dx = dx;
  a.part = reinterpret_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), 0, st, a);
  RSX_LAUNCHED();
  if (nv > 0) {
    s.part = a.part; s.blocks = (int)blocks; s.nv = nv; s.n4 = D / 4;
    hipLaunchKernelGGL(crossnet_bwd_sum_k, dim3((unsigned)((s.n4 + 15) / 16), (unsigned)nv), dim3(256), 0, st, s);
    RSX_LAUNCHED();
  }
  return 0;
}

RSX_API int rsx_crossnet(const float* x, int64_t ldx, int64_t B, int D, int L, const float* const* kernels,
                         const float* const* biases, const float* w_head, float* x_out, float* head_part,
                         void* stream) {
  RSX_ARG(x && kernels && biases && (x_out || head_part), "null tensor");
  RSX_ARG(D % 4 == 0 && D >= 4 && D <= 512, "D must be a multiple of 4 in [4, 512]");
  RSX_ARG(L >= 0 && L <= kMaxLayers, "L must be in [0, 8]");
  RSX_ARG(ldx >= D && ldx % 4 == 0, "bad ldx");
  RSX_ARG(!head_part || w_head, "head_part needs w_head");
  if (B == 0) return 0;
  CArgs a;
  a.x = x; a.ldx = ldx; a.B = B; a.D = D; a.L = L;
  for (int l = 0; l < kMaxLayers; ++l) {
    a.k[l] = l < L ? kernels[l] : nullptr;
    a.b[l] = l < L ? biases[l] : nullptr;
  }
  for (int l = 0; l < L; ++l) RSX_ARG(a.k[l] && a.b[l], "null layer kernel/bias");
  a.w_head = w_head; a.x_out = x_out; a.head_part = head_part;
  int64_t blocks = (B + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  hipStream_t st = (hipStream_t)stream;
  if (D <= 256) hipLaunchKernelGGL(crossnet_k<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(crossnet_k<2>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  RSX_LAUNCHED();
  return 0;
}
