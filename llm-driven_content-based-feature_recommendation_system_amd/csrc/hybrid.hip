// Inference kernels of HybridUserTower (tower_code/mined_inference.py):
//   * rsx_hybrid_adapter_fwd  ParallelAdapter over gathered rows of the content table [*, 128] and the
//                             GNN table [*, 64]:  m = GELU(LN(Wc c + bc)) + c + GELU(LN(Wg g + bg)),
//                             written as merged / unit = m / max(|m|, eps) / seq_in = m scale + time[delta]
//   * rsx_hybrid_seq_gather   seq_in from a precomputed merged table (the adapter once per item)
//   * rsx_hybrid_fuse_fwd     SequenceCentricFusion per token row: v = x / max(|x|, eps),
//                             g = sigmoid(W2 gelu(W1 v + b1) + b2), f = v + g0 Ugnn[u] + g1 Umeta[u],
//                             out = normalize(LN(f)); optional v and the two gate means
// Exact fp32 products on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain per output
// element, as csrc/distill.hip), no float atomics, every row statistic by a fixed lane pattern: a row's
// result depends on the row alone, not on its tile, slot or neighbours; the gate sums are per-workgroup
// partials (the workgroup count depends on the row count alone) added in workgroup order.
//
// Adapter: a workgroup (4 waves) stages Wc and Wg in LDS once (fp32, 97 KB) and walks tiles of 32 rows;
// the next tile's gathered rows are in flight in registers while the current tile computes. Per tile
// wave w takes output columns [32w, 32w + 32): Pc = Xc Wc^T + bc (K = 128), Pg = Xg Wg^T + bg (K = 64)
// -> LDS; then eight lanes per row do both LayerNorms, the GELUs, the residual, the sum, the norm and
// the time row, and store float4s. LDS rows are padded to an odd stride (129 / 65 floats).
// Fusion: W1 [64, 128] staged once; tiles of 64 rows, four lanes per row normalise the row into LDS,
// wave w computes H rows [32 (w >> 1), +32) x hidden [32 (w & 1), +32) (K = 128), then four lanes per
// row finish the gate, the gated add, the LayerNorm and the last normalise.
#include "rsx_common.h"
#include "recsys_amd.h"

namespace {

constexpr int kD = 128, kG = 64, kHid = 64;
constexpr int kTimeRows = 1001;   // nn.Embedding(1001, 128); deltas are clamped to 1000
constexpr int kARows = 32;        // adapter rows per tile
constexpr int kFRows = 64;        // fusion rows per tile
constexpr int kMaxSlots = 256;    // fusion workgroups (gate partials): min(tiles, 256)
constexpr int LDC = kD + 1, LDG = kG + 1;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// row of accumulator register reg in a 32x32 C/D tile (the column is lane & 31)
__device__ __forceinline__ int crow(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ f32x16 splat(float v) {
  f32x16 a;
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = v;
  return a;
}

// acc += X W^T for one 32x32 tile: X rows at x (row stride LDX), W rows (= output columns) at w (LDW)
template <int LDX, int LDW, int K>
__device__ __forceinline__ void mma_xwt(f32x16& acc, const float* x, const float* w) {
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  x += r * LDX + h;
  w += r * LDW + h;
#pragma unroll 8
  for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[k], w[k], acc, 0, 0, 0);
}

// W [rows, K] (dense) -> LDS rows of stride K + 1
template <int K>
__device__ __forceinline__ void stage_matrix(float* dst, const float* __restrict__ w, int rows) {
  for (int e = threadIdx.x * 4; e < rows * K; e += 256 * 4) {
    const float4 a = *reinterpret_cast<const float4*>(w + e);
    float* d = &dst[(e / K) * (K + 1) + e % K];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// sum over the lanes of a group of W consecutive lanes, by xor shuffles in a fixed order
template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LayerNorm statistics of a row of W * N values spread over W lanes, N per lane: the mean, then the
// biased variance about it (two passes), rstd = 1 / sqrt(var + eps)
template <int W, int N>
__device__ __forceinline__ void row_stats(const float (&v)[N], float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < N; ++e) s += v[e];
  mean = group_sum<W>(s) * (1.0f / (float)(W * N));
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float d = v[e] - mean;
    q = fmaf(d, d, q);
  }
  const float var = group_sum<W>(q) * (1.0f / (float)(W * N));
  rstd = 1.0f / sqrtf(var + eps);
}

// ------------------------------------------------------------------------------------------ adapter
struct AdapterLds {
  float wc[kD * LDC];      // Wc[o][k]
  float wg[kD * LDG];      // Wg[o][k]
  float xc[kARows * LDC];  // gathered content rows
  float xg[kARows * LDG];  // gathered GNN rows
  float pc[kARows * LDC];  // Wc c + bc
  float pg[kARows * LDC];  // Wg g + bg
};
static_assert(sizeof(AdapterLds) <= 160 * 1024, "LDS");

struct AdapterArgs {
  const float* content; int64_t ldc, Nc;
  const float* gnn; int64_t ldg, Ng;
  const int64_t* ids; int64_t first_row, R;
  const float* wc; const float* bc; const float* lnc_w; const float* lnc_b;
  const float* wg; const float* bg; const float* lng_w; const float* lng_b;
  float ln_eps, eps, scale;
  const int64_t* deltas; const float* time_tab;
  float* merged; float* unit; float* seq_in;
  int* flag;
};

// seq_in = m * scale + t, the product rounded before the sum (both forms of seq_in share it bit for bit)
__device__ __forceinline__ float4 scale_add(const float4& m, float s, const float4& t) {
  return make_float4(__fadd_rn(__fmul_rn(m.x, s), t.x), __fadd_rn(__fmul_rn(m.y, s), t.y),
                     __fadd_rn(__fmul_rn(m.z, s), t.z), __fadd_rn(__fmul_rn(m.w, s), t.w));
}

// the time row of a delta: min(delta, 1000); a negative delta sets the flag and reads row 0
__device__ __forceinline__ const float* time_row(const float* tab, int64_t d, int* flag) {
  if (d < 0) {
    *flag = 1;
    d = 0;
  }
  return tab + (d > kTimeRows - 1 ? kTimeRows - 1 : d) * kD;
}

struct AdapterRegs {
  float4 c[4];
  float4 g[2];
};

// the gathered rows of tile t that this thread stages: content piece i = tid + 256 j (row i / 32, float4
// i % 32), GNN piece i = tid + 256 j (row i / 16, float4 i % 16). Rows past R and ids outside the tables
// read zeros / row 0 (the flag is set).
__device__ __forceinline__ void adapter_load(const AdapterArgs& a, int64_t t, AdapterRegs& x) {
  const int tid = threadIdx.x;
  const int64_t lim = a.Nc < a.Ng ? a.Nc : a.Ng;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j, r = i >> 5, c4 = i & 31;
    const int64_t row = t * kARows + r;
    x.c[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < a.R) {
      int64_t id = a.ids ? a.ids[row] : a.first_row + row;
      if (id < 0 || id >= lim) {
        if (c4 == 0) *a.flag = 1;
        id = 0;
      }
      x.c[j] = ld4(a.content + id * a.ldc + 4 * c4);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + 256 * j, r = i >> 4, c4 = i & 15;
    const int64_t row = t * kARows + r;
    x.g[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < a.R) {
      int64_t id = a.ids ? a.ids[row] : a.first_row + row;
      if (id < 0 || id >= lim) id = 0;
      x.g[j] = ld4(a.gnn + id * a.ldg + 4 * c4);
    }
  }
}

__device__ __forceinline__ void adapter_store(AdapterLds& L, const AdapterRegs& x) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    float* d = &L.xc[(i >> 5) * LDC + 4 * (i & 31)];
    d[0] = x.c[j].x; d[1] = x.c[j].y; d[2] = x.c[j].z; d[3] = x.c[j].w;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + 256 * j;
    float* d = &L.xg[(i >> 4) * LDG + 4 * (i & 15)];
    d[0] = x.g[j].x; d[1] = x.g[j].y; d[2] = x.g[j].z; d[3] = x.g[j].w;
  }
}

__global__ __launch_bounds__(256) void hybrid_adapter_k(AdapterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  AdapterLds& L = *reinterpret_cast<AdapterLds*>(smem);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  stage_matrix<kD>(L.wc, a.wc, kD);
  stage_matrix<kG>(L.wg, a.wg, kD);
  const int64_t tiles = (a.R + kARows - 1) / kARows;
  AdapterRegs x;
  if ((int64_t)blockIdx.x < tiles) adapter_load(a, blockIdx.x, x);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    adapter_store(L, x);
    __syncthreads();
    if (t + gridDim.x < tiles) adapter_load(a, t + gridDim.x, x);
    {
      const int o = 32 * w + (lane & 31);
      f32x16 pc = splat(a.bc[o]), pg = splat(a.bg[o]);
      mma_xwt<LDC, LDC, kD>(pc, L.xc, L.wc + 32 * w * LDC);
      mma_xwt<LDG, LDG, kG>(pg, L.xg, L.wg + 32 * w * LDG);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = crow(reg, lane);
        L.pc[r * LDC + o] = pc[reg];
        L.pg[r * LDC + o] = pg[reg];
      }
    }
    __syncthreads();
    {
      // eight lanes per row; lane q holds columns 4 q + 32 j + {0..3}, j = 0..3 (as v[4 j + i])
      const int r = tid >> 3, q = tid & 7;
      const int64_t row = t * kARows + r;
      float vc[16], vg[16];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          vc[4 * j + i] = L.pc[r * LDC + 4 * q + 32 * j + i];
          vg[4 * j + i] = L.pg[r * LDC + 4 * q + 32 * j + i];
        }
      float mc, rc, mg, rg;
      row_stats<8, 16>(vc, a.ln_eps, mc, rc);
      row_stats<8, 16>(vg, a.ln_eps, mg, rg);
      float m[16];
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = 4 * q + 32 * j;
        const float4 cw = ld4(a.lnc_w + col), cb = ld4(a.lnc_b + col), gw = ld4(a.lng_w + col), gb = ld4(a.lng_b + col);
        const float cwv[4] = {cw.x, cw.y, cw.z, cw.w}, cbv[4] = {cb.x, cb.y, cb.z, cb.w};
        const float gwv[4] = {gw.x, gw.y, gw.z, gw.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 4 * j + i;
          const float yc = rsx::gelu_erf((vc[e] - mc) * rc * cwv[i] + cbv[i]);
          const float yg = rsx::gelu_erf((vg[e] - mg) * rg * gwv[i] + gbv[i]);
          m[e] = (yc + L.xc[r * LDC + col + i]) + yg;
          ss = fmaf(m[e], m[e], ss);
        }
      }
      ss = group_sum<8>(ss);
      if (row < a.R) {
        const float nz = sqrtf(ss);
        const float n = nz > a.eps ? nz : a.eps;
        const float* trow = a.seq_in ? time_row(a.time_tab, a.deltas[row], a.flag) : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = 4 * q + 32 * j;
          const float4 mv = make_float4(m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]);
          if (a.merged) *reinterpret_cast<float4*>(a.merged + row * kD + col) = mv;
          if (a.unit)
            *reinterpret_cast<float4*>(a.unit + row * kD + col) = make_float4(mv.x / n, mv.y / n, mv.z / n, mv.w / n);
          if (a.seq_in) *reinterpret_cast<float4*>(a.seq_in + row * kD + col) = scale_add(mv, a.scale, ld4(trow + col));
        }
      }
    }
    __syncthreads();   // xc / pc / pg are rewritten by the next tile
  }
}

// seq_in[t] = merged[ids[t] - first_row] * scale + time[min(delta, 1000)]; 32 lanes per token. An id
// below first_row (the padding id of a table that starts at row 1) reads a zero row; an id past the
// table sets the flag and reads a zero row.
__global__ __launch_bounds__(256) void hybrid_seq_gather_k(const float* __restrict__ merged, int64_t Nm,
                                                           int64_t first_row, const int64_t* __restrict__ ids,
                                                           const int64_t* __restrict__ deltas, int64_t T,
                                                           const float* __restrict__ time_tab, float scale,
                                                           float* __restrict__ seq_in, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int c4 = threadIdx.x & 31;
  if (t >= T) return;
  const int64_t id = ids[t], row = id - first_row;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  if (id < 0 || row >= Nm) {
    if (c4 == 0) *flag = 1;
  } else if (row >= 0) {
    m = ld4(merged + row * kD + 4 * c4);
  }
  const float* trow = time_row(time_tab, deltas[t], flag);
  *reinterpret_cast<float4*>(seq_in + t * kD + 4 * c4) = scale_add(m, scale, ld4(trow + 4 * c4));
}

// ------------------------------------------------------------------------------------------- fusion
struct FuseLds {
  float w1[kHid * LDC];     // W1[j][k]
  float v[kFRows * LDC];    // the normalised rows
  float h[kFRows * LDG];    // gelu(W1 v + b1)
  float w2[2 * kHid];
  float gate[kFRows * 2];
};
static_assert(sizeof(FuseLds) <= 160 * 1024, "LDS");

struct FuseArgs {
  const float* seq_out; int64_t T, L;
  const int64_t* rows; int64_t n, B;
  const float* u_gnn; const float* u_meta;
  const float* w1; const float* b1; const float* w2; const float* b2;
  const float* ln_w; const float* ln_b;
  float ln_eps, eps;
  float* out; float* v_seq;
  double* gate_part;   // [slots][2] (nullable)
  int* flag;
};

__global__ __launch_bounds__(256) void hybrid_fuse_k(FuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  FuseLds& L = *reinterpret_cast<FuseLds*>(smem);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  stage_matrix<kD>(L.w1, a.w1, kHid);
  if (tid < 2 * kHid) L.w2[tid] = a.w2[tid];
  const float b2_0 = a.b2[0], b2_1 = a.b2[1];
  double g0_acc = 0.0, g1_acc = 0.0;   // wave 0
  const int64_t tiles = (a.n + kFRows - 1) / kFRows;
  // four lanes per row; lane q holds columns 4 q + 16 j + {0..3}, j = 0..7 (as x[4 j + i])
  const int r = tid >> 2, q = tid & 3;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t * kFRows + r;
    int64_t src = -1;
    if (i < a.n) {
      src = a.rows ? a.rows[i] : i;
      if (src < 0 || src >= a.T) {
        if (q == 0) *a.flag = 1;
        src = 0;
      }
    }
    float x[32];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 p = src >= 0 ? ld4(a.seq_out + src * kD + 4 * q + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[4 * j] = p.x; x[4 * j + 1] = p.y; x[4 * j + 2] = p.z; x[4 * j + 3] = p.w;
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) ss = fmaf(x[e], x[e], ss);
    ss = group_sum<4>(ss);
    {
      const float nz = sqrtf(ss);
      const float nrm = nz > a.eps ? nz : a.eps;
#pragma unroll
      for (int e = 0; e < 32; ++e) x[e] = x[e] / nrm;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) L.v[r * LDC + 4 * q + 16 * j + e] = x[4 * j + e];
        if (a.v_seq && src >= 0)
          *reinterpret_cast<float4*>(a.v_seq + i * kD + 4 * q + 16 * j) =
              make_float4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
      }
    }
    __syncthreads();
    {
      const int mi = w >> 1, oj = w & 1, o = 32 * oj + (lane & 31);
      f32x16 hacc = splat(a.b1[o]);
      mma_xwt<LDC, LDC, kD>(hacc, L.v + 32 * mi * LDC, L.w1 + 32 * oj * LDC);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) L.h[(32 * mi + crow(reg, lane)) * LDG + o] = rsx::gelu_erf(hacc[reg]);
    }
    __syncthreads();
    {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float hv = L.h[r * LDG + 16 * q + e];
        s0 = fmaf(hv, L.w2[16 * q + e], s0);
        s1 = fmaf(hv, L.w2[kHid + 16 * q + e], s1);
      }
      s0 = group_sum<4>(s0) + b2_0;
      s1 = group_sum<4>(s1) + b2_1;
      const float g0 = 1.0f / (1.0f + expf(-s0)), g1 = 1.0f / (1.0f + expf(-s1));
      if (q == 0) {
        L.gate[2 * r] = src >= 0 ? g0 : 0.f;
        L.gate[2 * r + 1] = src >= 0 ? g1 : 0.f;
      }
      if (src >= 0) {
        int64_t u = src / a.L;
        if (u >= a.B) u = a.B - 1;   // src < T = B L, so only a caller's inconsistent B could reach this
        const float* ug = a.u_gnn + u * kD;
        const float* um = a.u_meta + u * kD;
        float f[32];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int col = 4 * q + 16 * j;
          const float4 pg = ld4(ug + col), pm = ld4(um + col);
          f[4 * j] = (x[4 * j] + g0 * pg.x) + g1 * pm.x;
          f[4 * j + 1] = (x[4 * j + 1] + g0 * pg.y) + g1 * pm.y;
          f[4 * j + 2] = (x[4 * j + 2] + g0 * pg.z) + g1 * pm.z;
          f[4 * j + 3] = (x[4 * j + 3] + g0 * pg.w) + g1 * pm.w;
        }
        float mean, rstd;
        row_stats<4, 32>(f, a.ln_eps, mean, rstd);
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int col = 4 * q + 16 * j;
          const float4 lw = ld4(a.ln_w + col), lb = ld4(a.ln_b + col);
          f[4 * j] = (f[4 * j] - mean) * rstd * lw.x + lb.x;
          f[4 * j + 1] = (f[4 * j + 1] - mean) * rstd * lw.y + lb.y;
          f[4 * j + 2] = (f[4 * j + 2] - mean) * rstd * lw.z + lb.z;
          f[4 * j + 3] = (f[4 * j + 3] - mean) * rstd * lw.w + lb.w;
        }
#pragma unroll
        for (int e = 0; e < 32; ++e) s2 = fmaf(f[e], f[e], s2);
        s2 = group_sum<4>(s2);
        const float nz = sqrtf(s2);
        const float nrm = nz > a.eps ? nz : a.eps;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<float4*>(a.out + i * kD + 4 * q + 16 * j) =
              make_float4(f[4 * j] / nrm, f[4 * j + 1] / nrm, f[4 * j + 2] / nrm, f[4 * j + 3] / nrm);
      }   // the shuffles above stay inside a row's four lanes, which share src
    }
    __syncthreads();
    if (w == 0 && a.gate_part) {   // the tile's 64 gate pairs by a fixed shuffle tree, in double
      g0_acc += rsx::wave_sum_width((double)L.gate[2 * lane], 64);
      g1_acc += rsx::wave_sum_width((double)L.gate[2 * lane + 1], 64);
    }
    // L.gate is rewritten only after the next tile's two barriers; L.v after its first
  }
  if (tid == 0 && a.gate_part) {
    a.gate_part[2 * blockIdx.x] = g0_acc;
    a.gate_part[2 * blockIdx.x + 1] = g1_acc;
  }
}

// gate_mean[k] = (sum of the partials in slot order) / n
__global__ void hybrid_gate_mean_k(const double* __restrict__ part, int slots, int64_t n, float* __restrict__ mean) {
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int k = 0; k < slots; ++k) s += part[2 * k + threadIdx.x];
    mean[threadIdx.x] = (float)(s / (double)n);
  }
}

using rsx::aligned16;

template <typename K>
int raise_lds(K kernel, size_t bytes, const char* fn) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) {
    rsx::set_error("%s: cannot raise the LDS limit: %s", fn, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace

RSX_API int64_t rsx_hybrid_fuse_slots(int64_t n) {
  if (n < 1) return 0;
  const int64_t tiles = (n + kFRows - 1) / kFRows;
  return tiles < kMaxSlots ? tiles : kMaxSlots;
}

RSX_API int rsx_hybrid_adapter_fwd(const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn,
                                   int64_t ldg, int64_t Ng, int64_t Dg, const int64_t* ids, int64_t first_row,
                                   int64_t R, const float* wc, const float* bc, const float* lnc_w,
                                   const float* lnc_b, const float* wg, const float* bg, const float* lng_w,
                                   const float* lng_b, float ln_eps, float eps, const int64_t* deltas,
                                   const float* time_tab, float scale, float* merged, float* unit, float* seq_in,
                                   int32_t* flag, void* stream) {
  RSX_ARG(Dc == kD && Dg == kG, "the content rows must be 128 wide and the GNN rows 64 wide");
  RSX_ARG(R >= 0 && Nc >= 0 && Ng >= 0, "negative size");
  RSX_ARG(ln_eps > 0.f && eps > 0.f, "eps must be positive");
  if (R == 0) return 0;
  RSX_ARG(content && gnn && Nc >= 1 && Ng >= 1, "null tensor (content / gnn table)");
  RSX_ARG(wc && bc && lnc_w && lnc_b && wg && bg && lng_w && lng_b && flag, "null tensor");
  RSX_ARG(merged || unit || seq_in, "no output requested");
  RSX_ARG(!seq_in || (deltas && time_tab), "seq_in needs deltas and time_tab");
  RSX_ARG(ids || (first_row >= 0 && first_row + R <= (Nc < Ng ? Nc : Ng)), "first_row + R exceeds the tables");
  RSX_ARG(ldc >= kD && ldc % 4 == 0 && ldg >= kG && ldg % 4 == 0, "bad leading dimensions");
  RSX_ARG(aligned16(content) && aligned16(gnn) && aligned16(wc) && aligned16(wg) && aligned16(lnc_w) &&
              aligned16(lnc_b) && aligned16(lng_w) && aligned16(lng_b) && aligned16(time_tab) && aligned16(merged) &&
              aligned16(unit) && aligned16(seq_in), "rows must be 16-byte aligned");
  static const int attr = raise_lds(hybrid_adapter_k, sizeof(AdapterLds), "rsx_hybrid_adapter_fwd");
  if (attr) return attr;
  AdapterArgs a;
  a.content = content; a.ldc = ldc; a.Nc = Nc;
  a.gnn = gnn; a.ldg = ldg; a.Ng = Ng;
  a.ids = ids; a.first_row = first_row; a.R = R;
  a.wc = wc; a.bc = bc; a.lnc_w = lnc_w; a.lnc_b = lnc_b;
  a.wg = wg; a.bg = bg; a.lng_w = lng_w; a.lng_b = lng_b;
  a.ln_eps = ln_eps; a.eps = eps; a.scale = scale;
  a.deltas = deltas; a.time_tab = time_tab;
  a.merged = merged; a.unit = unit; a.seq_in = seq_in;
  a.flag = flag;
  const int64_t tiles = (R + kARows - 1) / kARows;
  const int64_t grid = tiles < rsx::cu_count() ? tiles : rsx::cu_count();
  hipLaunchKernelGGL(hybrid_adapter_k, dim3((unsigned)grid), dim3(256), sizeof(AdapterLds), (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_hybrid_seq_gather(const float* merged, int64_t Nm, int64_t D, int64_t first_row, const int64_t* ids,
                                  const int64_t* deltas, int64_t T, const float* time_tab, float scale,
                                  float* seq_in, int32_t* flag, void* stream) {
  RSX_ARG(D == kD, "the merged rows must be 128 wide");
  RSX_ARG(T >= 0 && Nm >= 0 && first_row >= 0, "negative size");
  if (T == 0) return 0;
  RSX_ARG(merged && Nm >= 1, "null tensor (merged table)");
  RSX_ARG(ids && deltas && time_tab && seq_in && flag, "null tensor");
  RSX_ARG(aligned16(merged) && aligned16(time_tab) && aligned16(seq_in), "rows must be 16-byte aligned");
  RSX_ARG((T + 7) / 8 < (1LL << 31), "too many rows");
  hipLaunchKernelGGL(hybrid_seq_gather_k, dim3((unsigned)((T + 7) / 8)), dim3(256), 0, (hipStream_t)stream, merged, Nm,
                     first_row, ids, deltas, T, time_tab, scale, seq_in, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_hybrid_fuse_fwd(const float* seq_out, int64_t B, int64_t L, int64_t D, const int64_t* rows,
                                int64_t n_rows, const float* u_gnn, const float* u_meta, const float* w1,
                                const float* b1, int64_t hidden, const float* w2, const float* b2,
                                const float* ln_w, const float* ln_b, float ln_eps, float eps, float* out,
                                float* v_seq, float* gate_mean, void* ws, int64_t ws_bytes, int32_t* flag,
                                void* stream) {
  RSX_ARG(D == kD && hidden == kHid, "the rows must be 128 wide and the gate's hidden layer 64 wide");
  RSX_ARG(B >= 0 && n_rows >= 0, "negative size");
  RSX_ARG(L >= 1 && L <= 64, "L must be in [1, 64]");
  RSX_ARG(ln_eps > 0.f && eps > 0.f, "eps must be positive");
  const int64_t n = rows ? n_rows : B * L;
  if (n == 0) return 0;
  RSX_ARG(B >= 1, "rows given for an empty batch");
  RSX_ARG(seq_out && u_gnn && u_meta && w1 && b1 && w2 && b2 && ln_w && ln_b && out && flag, "null tensor");
  RSX_ARG(aligned16(seq_out) && aligned16(u_gnn) && aligned16(u_meta) && aligned16(w1) && aligned16(ln_w) &&
              aligned16(ln_b) && aligned16(out) && aligned16(v_seq), "rows must be 16-byte aligned");
  const int64_t slots = rsx_hybrid_fuse_slots(n);
  RSX_ARG(!gate_mean || (ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= slots * 2 * (int64_t)sizeof(double)),
          "the gate means need a workspace of rsx_hybrid_fuse_slots(n) * 16 bytes");
  static const int attr = raise_lds(hybrid_fuse_k, sizeof(FuseLds), "rsx_hybrid_fuse_fwd");
  if (attr) return attr;
  FuseArgs a;
  a.seq_out = seq_out; a.T = B * L; a.L = L;
  a.rows = rows; a.n = n; a.B = B;
  a.u_gnn = u_gnn; a.u_meta = u_meta;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.ln_w = ln_w; a.ln_b = ln_b;
  a.ln_eps = ln_eps; a.eps = eps;
  a.out = out; a.v_seq = v_seq;
  a.gate_part = gate_mean ? (double*)ws : nullptr;
  a.flag = flag;
  hipLaunchKernelGGL(hybrid_fuse_k, dim3((unsigned)slots), dim3(256), sizeof(FuseLds), (hipStream_t)stream, a);
  RSX_LAUNCHED();
  if (gate_mean) {
    hipLaunchKernelGGL(hybrid_gate_mean_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, (int)slots, n,
                       gate_mean);
    RSX_LAUNCHED();
  }
  return 0;
}
