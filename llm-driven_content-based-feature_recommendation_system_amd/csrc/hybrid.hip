// Kernels of HybridUserTower (tower_code/mined_inference.py). Inference:
//   * rsx_hybrid_adapter_fwd  ParallelAdapter over gathered rows of the content table [*, 128] and the
//                             GNN table [*, 64]:  m = GELU(LN(Wc c + bc)) + c + GELU(LN(Wg g + bg)),
//                             written as merged / unit = m / max(|m|, eps) / seq_in = m scale + time[delta]
//   * rsx_hybrid_seq_gather   seq_in from a precomputed merged table (the adapter once per item)
//   * rsx_hybrid_fuse_fwd     SequenceCentricFusion per token row: v = x / max(|x|, eps),
//                             g = sigmoid(W2 gelu(W1 v + b1) + b2), f = v + g0 Ugnn[u] + g1 Umeta[u],
//                             out = normalize(LN(f)); optional v and the two gate means
// With gradients: hybrid_adapter_k<true> / hybrid_fuse_k<true> add the dropout sites of
// training mode to the two forwards (rsx_hybrid_adapter_train_fwd, rsx_hybrid_fuse_train_fwd);
// rsx_hybrid_adapter_bwd and rsx_hybrid_fuse_bwd are their backward passes (comments at the kernels).
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
  // training form (hybrid_adapter_k<true>): the two Dropout(p) after the GELUs, keep index row * 128 + col,
  // and what the backward reads: the gathered rows and the two pre-LayerNorm products
  rsx::Dropout drop_c, drop_g;
  float* xc_out; float* xg_out;   // [R, 128], [R, 64]
  float* zc_out; float* zg_out;   // [R, 128] each
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

// the staged pieces of tile t to the backward's copies of the gathered rows (training form)
__device__ __forceinline__ void adapter_save_rows(const AdapterArgs& a, int64_t t, const AdapterRegs& x) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    const int64_t row = t * kARows + (i >> 5);
    if (row < a.R) *reinterpret_cast<float4*>(a.xc_out + row * kD + 4 * (i & 31)) = x.c[j];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + 256 * j;
    const int64_t row = t * kARows + (i >> 4);
    if (row < a.R) *reinterpret_cast<float4*>(a.xg_out + row * kG + 4 * (i & 15)) = x.g[j];
  }
}

template <bool TRAIN>
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
    if (TRAIN) adapter_save_rows(a, t, x);
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
          float yc = rsx::gelu_erf((vc[e] - mc) * rc * cwv[i] + cbv[i]);
          float yg = rsx::gelu_erf((vg[e] - mg) * rg * gwv[i] + gbv[i]);
          if (TRAIN) {
            const uint64_t idx = (uint64_t)row * kD + (uint64_t)(col + i);
            yc = a.drop_c.apply(yc, idx);
            yg = a.drop_g.apply(yg, idx);
          }
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
          if (TRAIN) {
            *reinterpret_cast<float4*>(a.zc_out + row * kD + col) =
                make_float4(vc[4 * j], vc[4 * j + 1], vc[4 * j + 2], vc[4 * j + 3]);
            *reinterpret_cast<float4*>(a.zg_out + row * kD + col) =
                make_float4(vg[4 * j], vg[4 * j + 1], vg[4 * j + 2], vg[4 * j + 3]);
          }
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

// ------------------------------------------------------------------------------- adapter, backward
// Per tile of 32 rows. Phase 1, eight lanes per row as the forward: the LayerNorm statistics, the GELU
// and the keep masks are recomputed from the saved products zc / zg; dz = LN'(dm keep / (1 - p) gelu'(y))
// goes to global memory (the weight gradients' operand) and to LDS. Phase 2: wave w computes
// dc[:, 32 w ..] = dm + dz_c Wc and (w < 2) dg[:, 32 w ..] = dz_g Wg on the fp32 MFMA against the
// transposed weights staged once. The four LayerNorm vectors' sums stay in registers across the tiles
// and are folded over the 32 rows in row order at the end: one partial [4][128] per workgroup.
struct AdapterBwdLds {
  float wct[kD * LDC];       // wct[o][k] = Wc[k][o]
  float wgt[kG * LDC];       // wgt[o][k] = Wg[k][o]
  float dzc[kARows * LDC];
  float dzg[kARows * LDC];
};
static_assert(sizeof(AdapterBwdLds) <= 160 * 1024, "LDS");
static_assert(kARows * 4 * kD <= kD * LDC, "the LayerNorm partials are folded in wct");

struct AdapterBwdArgs {
  const float* dy; float gscale; int64_t R;
  const float* zc; const float* zg;
  const float* wc; const float* wg;
  const float* lnc_w; const float* lnc_b; const float* lng_w; const float* lng_b;
  float ln_eps;
  rsx::Dropout drop_c, drop_g;
  float* dzc; float* dzg; float* dc; float* dg;
  float* ln_part;   // [grid][4][128]: d lnc_w, d lnc_b, d lng_w, d lng_b
};

// W [128][IN] (dense) -> dst[o * LDC + k] = W[k * IN + o]
template <int IN>
__device__ __forceinline__ void stage_transposed(float* dst, const float* __restrict__ w) {
  for (int e = threadIdx.x; e < kD * IN; e += 256) dst[(e % IN) * LDC + e / IN] = w[e];
}

// one branch of the adapter for this lane's 16 columns of a row: dz from dm, and the row's terms of
// d ln_w / d ln_b added to aw / ab
__device__ __forceinline__ void adapter_branch_bwd(const float (&v)[16], const float (&dm)[16], const float* ln_w,
                                                   const float* ln_b, float ln_eps, const rsx::Dropout& drop,
                                                   int64_t row, int q, float (&aw)[16], float (&ab)[16],
                                                   float (&dz)[16]) {
  float mean, rstd;
  row_stats<8, 16>(v, ln_eps, mean, rstd);
  float xh[16], g[16];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = 4 * q + 32 * j;
    const float4 w4 = ld4(ln_w + col), b4 = ld4(ln_b + col);
    const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * j + i;
      xh[e] = (v[e] - mean) * rstd;
      float dyv = dm[e] * rsx::gelu_erf_grad(xh[e] * wv[i] + bv[i]);
      dyv = drop.apply(dyv, (uint64_t)row * kD + (uint64_t)(col + i));
      aw[e] = fmaf(dyv, xh[e], aw[e]);
      ab[e] += dyv;
      g[e] = dyv * wv[i];
      s1 += g[e];
      s2 = fmaf(g[e], xh[e], s2);
    }
  }
  s1 = group_sum<8>(s1) * (1.0f / kD);
  s2 = group_sum<8>(s2) * (1.0f / kD);
#pragma unroll
  for (int e = 0; e < 16; ++e) dz[e] = rstd * ((g[e] - s1) - xh[e] * s2);
}

__global__ __launch_bounds__(256) void hybrid_adapter_bwd_k(AdapterBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  AdapterBwdLds& L = *reinterpret_cast<AdapterBwdLds*>(smem);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  stage_transposed<kD>(L.wct, a.wc);
  stage_transposed<kG>(L.wgt, a.wg);
  const int64_t tiles = (a.R + kARows - 1) / kARows;
  const int r = tid >> 3, q = tid & 7;
  float acw[16], acb[16], agw[16], agb[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acw[e] = acb[e] = agw[e] = agb[e] = 0.f;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t row = t * kARows + r;
    float dm[16], vc[16], vg[16], dzc[16], dzg[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 4 * q + 32 * j;
      float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f), c4 = d4, g4 = d4;
      if (row < a.R) {
        d4 = ld4(a.dy + row * kD + col);
        c4 = ld4(a.zc + row * kD + col);
        g4 = ld4(a.zg + row * kD + col);
      }
      dm[4 * j] = d4.x * a.gscale; dm[4 * j + 1] = d4.y * a.gscale;
      dm[4 * j + 2] = d4.z * a.gscale; dm[4 * j + 3] = d4.w * a.gscale;
      vc[4 * j] = c4.x; vc[4 * j + 1] = c4.y; vc[4 * j + 2] = c4.z; vc[4 * j + 3] = c4.w;
      vg[4 * j] = g4.x; vg[4 * j + 1] = g4.y; vg[4 * j + 2] = g4.z; vg[4 * j + 3] = g4.w;
    }
    adapter_branch_bwd(vc, dm, a.lnc_w, a.lnc_b, a.ln_eps, a.drop_c, row, q, acw, acb, dzc);
    adapter_branch_bwd(vg, dm, a.lng_w, a.lng_b, a.ln_eps, a.drop_g, row, q, agw, agb, dzg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 4 * q + 32 * j;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        L.dzc[r * LDC + col + i] = dzc[4 * j + i];
        L.dzg[r * LDC + col + i] = dzg[4 * j + i];
      }
      if (row < a.R) {
        *reinterpret_cast<float4*>(a.dzc + row * kD + col) =
            make_float4(dzc[4 * j], dzc[4 * j + 1], dzc[4 * j + 2], dzc[4 * j + 3]);
        *reinterpret_cast<float4*>(a.dzg + row * kD + col) =
            make_float4(dzg[4 * j], dzg[4 * j + 1], dzg[4 * j + 2], dzg[4 * j + 3]);
      }
    }
    __syncthreads();
    {
      const int o = 32 * w + (lane & 31);
      f32x16 acc = splat(0.f);
      mma_xwt<LDC, LDC, kD>(acc, L.dzc, L.wct + 32 * w * LDC);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t row2 = t * kARows + crow(reg, lane);
        if (row2 < a.R) a.dc[row2 * kD + o] = a.dy[row2 * kD + o] * a.gscale + acc[reg];
      }
      if (w < 2) {   // wave-uniform
        f32x16 acg = splat(0.f);
        mma_xwt<LDC, LDC, kD>(acg, L.dzg, L.wgt + 32 * w * LDC);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int64_t row2 = t * kARows + crow(reg, lane);
          if (row2 < a.R) a.dg[row2 * kG + o] = acg[reg];
        }
      }
    }
    __syncthreads();   // dzc / dzg are rewritten by the next tile
  }
  // fold the LayerNorm sums over the tile's 32 row slots, in row order (wct is no longer read)
  __syncthreads();
  float* red = L.wct;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int col = 4 * q + 32 * (e >> 2) + (e & 3);
    red[r * 4 * kD + col] = acw[e];
    red[r * 4 * kD + kD + col] = acb[e];
    red[r * 4 * kD + 2 * kD + col] = agw[e];
    red[r * 4 * kD + 3 * kD + col] = agb[e];
  }
  __syncthreads();
  for (int c = tid; c < 4 * kD; c += 256) {
    float s = 0.f;
    for (int rr = 0; rr < kARows; ++rr) s += red[rr * 4 * kD + c];
    a.ln_part[(int64_t)blockIdx.x * 4 * kD + c] = s;
  }
}

// out[c] = the partials' column c added in workgroup order, c < n
__global__ __launch_bounds__(256) void hybrid_part_sum_k(const float* __restrict__ part, int nparts, int n,
                                                         float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(int64_t)k * n + c];
  out[c] = s;
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
  // training form (hybrid_fuse_k<true>): Dropout(p) over each token's copy of the two projected rows,
  // keep index token_row * 128 + col
  rsx::Dropout drop_a, drop_b;
};

template <bool TRAIN>
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
          float4 pg = ld4(ug + col), pm = ld4(um + col);
          if (TRAIN) {
            const uint64_t idx = (uint64_t)src * kD + (uint64_t)col;
            pg = make_float4(a.drop_a.apply(pg.x, idx), a.drop_a.apply(pg.y, idx + 1), a.drop_a.apply(pg.z, idx + 2),
                             a.drop_a.apply(pg.w, idx + 3));
            pm = make_float4(a.drop_b.apply(pm.x, idx), a.drop_b.apply(pm.y, idx + 1), a.drop_b.apply(pm.z, idx + 2),
                             a.drop_b.apply(pm.w, idx + 3));
          }
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

// -------------------------------------------------------------------------------- fusion, backward
// Per tile of 64 rows, four lanes per row as the forward, which is recomputed from seq_out (nothing but
// the inputs is saved): v, the gate's pre-activations (MFMA, kept raw in LDS), the gates, the masked
// rows, f, its LayerNorm and the last normalise. Then backwards through them: df, the two gate
// gradients, dpre (to global memory for dW1 / db1, and to LDS), dv = df (+ d v_seq) + dpre W1 on the
// MFMA against the transposed W1, and dx through v = x / max(|x|, eps). A row whose |x| or |LN(f)| is at
// the eps floor is divided by eps, a constant: no division by a zero norm, so an all-zero row with zero
// upstream gradients gives exact zeros. The per-token gradients of the two projected rows go to global
// memory and are summed per user by hybrid_user_sum_k; the small parameter gradients (ln_w, ln_b, W2, b2)
// stay in registers across tiles and are folded over the 64 row slots in row order at the end.
constexpr int kFSmall = 2 * kD + 2 * kHid + 2;   // d ln_w | d ln_b | d W2 [2][64] | d b2

struct FuseBwdLds {
  float w1[kHid * LDC];     // W1[j][k]
  float w1t[kD * LDG];      // w1t[o][j] = W1[j][o]
  float v[kFRows * LDC];    // the normalised rows; later dpre W1
  float pre[kFRows * LDG];  // W1 v + b1
  float dpre[kFRows * LDG];
  float w2[2 * kHid];
};
static_assert(sizeof(FuseBwdLds) <= 160 * 1024, "LDS");
static_assert(kFRows * kFSmall <= kHid * LDC + kD * LDG + kFRows * LDC, "the small partials are folded in w1..v");

struct FuseBwdArgs {
  const float* seq_out; int64_t n, L, B;
  const float* u_gnn; const float* u_meta;
  const float* w1; const float* b1; const float* w2; const float* b2;
  const float* ln_w; const float* ln_b;
  float ln_eps, eps;
  rsx::Dropout drop_a, drop_b;
  const float* dout; const float* dv;   // dv nullable
  float* dx; float* dpre; float* dug_tok; float* dum_tok;
  float* part;   // [grid][kFSmall]
};

__global__ __launch_bounds__(256) void hybrid_fuse_bwd_k(FuseBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  FuseBwdLds& L = *reinterpret_cast<FuseBwdLds*>(smem);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  stage_matrix<kD>(L.w1, a.w1, kHid);
  for (int e = tid; e < kHid * kD; e += 256) L.w1t[(e % kD) * LDG + e / kD] = a.w1[e];
  if (tid < 2 * kHid) L.w2[tid] = a.w2[tid];
  const float b2_0 = a.b2[0], b2_1 = a.b2[1];
  const int64_t tiles = (a.n + kFRows - 1) / kFRows;
  const int r = tid >> 2, q = tid & 3;
  float alw[32], alb[32], aw0[16], aw1[16];
  float ab0 = 0.f, ab1 = 0.f;
#pragma unroll
  for (int e = 0; e < 32; ++e) alw[e] = alb[e] = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) aw0[e] = aw1[e] = 0.f;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t * kFRows + r;
    const bool ok = i < a.n;
    float x[32];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 p = ok ? ld4(a.seq_out + i * kD + 4 * q + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[4 * j] = p.x; x[4 * j + 1] = p.y; x[4 * j + 2] = p.z; x[4 * j + 3] = p.w;
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) ss = fmaf(x[e], x[e], ss);
    ss = group_sum<4>(ss);
    const float nz = sqrtf(ss);
    const float nrm = nz > a.eps ? nz : a.eps;
#pragma unroll
    for (int e = 0; e < 32; ++e) x[e] = x[e] / nrm;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) L.v[r * LDC + 4 * q + 16 * j + e] = x[4 * j + e];
    __syncthreads();
    {
      const int mi = w >> 1, oj = w & 1, o = 32 * oj + (lane & 31);
      f32x16 hacc = splat(a.b1[o]);
      mma_xwt<LDC, LDC, kD>(hacc, L.v + 32 * mi * LDC, L.w1 + 32 * oj * LDC);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) L.pre[(32 * mi + crow(reg, lane)) * LDG + o] = hacc[reg];
    }
    __syncthreads();
    float dvr[32];   // df (+ d v_seq): the part of dv that needs no MFMA
    {
      float hv[16], s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        hv[e] = rsx::gelu_erf(L.pre[r * LDG + 16 * q + e]);
        s0 = fmaf(hv[e], L.w2[16 * q + e], s0);
        s1 = fmaf(hv[e], L.w2[kHid + 16 * q + e], s1);
      }
      s0 = group_sum<4>(s0) + b2_0;
      s1 = group_sum<4>(s1) + b2_1;
      const float g0 = 1.0f / (1.0f + expf(-s0)), g1 = 1.0f / (1.0f + expf(-s1));
      int64_t u = ok ? i / a.L : 0;
      if (u >= a.B) u = a.B - 1;
      const float* ug = a.u_gnn + u * kD;
      const float* um = a.u_meta + u * kD;
      float pa[32], pb[32], f[32];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = 4 * q + 16 * j;
        const float4 pg = ld4(ug + col), pm = ld4(um + col);
        const float pgv[4] = {pg.x, pg.y, pg.z, pg.w}, pmv[4] = {pm.x, pm.y, pm.z, pm.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint64_t idx = (uint64_t)i * kD + (uint64_t)(col + e);
          pa[4 * j + e] = a.drop_a.apply(pgv[e], idx);
          pb[4 * j + e] = a.drop_b.apply(pmv[e], idx);
          f[4 * j + e] = (x[4 * j + e] + g0 * pa[4 * j + e]) + g1 * pb[4 * j + e];
        }
      }
      float mean, rstd;
      row_stats<4, 32>(f, a.ln_eps, mean, rstd);
      float y[32], s2 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = 4 * q + 16 * j;
        const float4 lw = ld4(a.ln_w + col), lb = ld4(a.ln_b + col);
        const float lwv[4] = {lw.x, lw.y, lw.z, lw.w}, lbv[4] = {lb.x, lb.y, lb.z, lb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f[4 * j + e] = (f[4 * j + e] - mean) * rstd;   // xhat
          y[4 * j + e] = f[4 * j + e] * lwv[e] + lbv[e];
          s2 = fmaf(y[4 * j + e], y[4 * j + e], s2);
        }
      }
      s2 = group_sum<4>(s2);
      const float nz2 = sqrtf(s2);
      const float nrm2 = nz2 > a.eps ? nz2 : a.eps;
      // out = y / nrm2: dy = (dout - out (dout . out)) / nrm2 above the floor, dout / eps at it
      float dy[32], dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 d4 = ok ? ld4(a.dout + i * kD + 4 * q + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        dy[4 * j] = d4.x; dy[4 * j + 1] = d4.y; dy[4 * j + 2] = d4.z; dy[4 * j + 3] = d4.w;
      }
#pragma unroll
      for (int e = 0; e < 32; ++e) dot = fmaf(dy[e], y[e] / nrm2, dot);
      dot = group_sum<4>(dot);
      if (!(nz2 > a.eps)) dot = 0.f;
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 lw = ld4(a.ln_w + 4 * q + 16 * j);
        const float lwv[4] = {lw.x, lw.y, lw.z, lw.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 4 * j + e;
          const float d = (dy[k] - (y[k] / nrm2) * dot) / nrm2;
          alw[k] = fmaf(d, f[k], alw[k]);
          alb[k] += d;
          dy[k] = d * lwv[e];   // d xhat
          t1 += dy[k];
          t2 = fmaf(dy[k], f[k], t2);
        }
      }
      t1 = group_sum<4>(t1) * (1.0f / kD);
      t2 = group_sum<4>(t2) * (1.0f / kD);
      float dg0 = 0.f, dg1 = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const float df = rstd * ((dy[k] - t1) - f[k] * t2);
        dvr[k] = df;
        dg0 = fmaf(df, pa[k], dg0);
        dg1 = fmaf(df, pb[k], dg1);
      }
      dg0 = group_sum<4>(dg0);
      dg1 = group_sum<4>(dg1);
      if (ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int col = 4 * q + 16 * j;
          float ta[4], tb[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint64_t idx = (uint64_t)i * kD + (uint64_t)(col + e);
            ta[e] = a.drop_a.apply(g0 * dvr[4 * j + e], idx);
            tb[e] = a.drop_b.apply(g1 * dvr[4 * j + e], idx);
          }
          *reinterpret_cast<float4*>(a.dug_tok + i * kD + col) = make_float4(ta[0], ta[1], ta[2], ta[3]);
          *reinterpret_cast<float4*>(a.dum_tok + i * kD + col) = make_float4(tb[0], tb[1], tb[2], tb[3]);
          if (a.dv) {
            const float4 d4 = ld4(a.dv + i * kD + col);
            dvr[4 * j] += d4.x; dvr[4 * j + 1] += d4.y; dvr[4 * j + 2] += d4.z; dvr[4 * j + 3] += d4.w;
          }
        }
      }
      const float ds0 = dg0 * g0 * (1.0f - g0), ds1 = dg1 * g1 * (1.0f - g1);
      if (q == 0) {
        ab0 += ds0;
        ab1 += ds1;
      }
      float dp[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        aw0[e] = fmaf(ds0, hv[e], aw0[e]);
        aw1[e] = fmaf(ds1, hv[e], aw1[e]);
        dp[e] = (ds0 * L.w2[16 * q + e] + ds1 * L.w2[kHid + 16 * q + e]) *
                rsx::gelu_erf_grad(L.pre[r * LDG + 16 * q + e]);
        L.dpre[r * LDG + 16 * q + e] = dp[e];
      }
      if (ok) {
#pragma unroll
        for (int e = 0; e < 16; e += 4)
          *reinterpret_cast<float4*>(a.dpre + i * kHid + 16 * q + e) = make_float4(dp[e], dp[e + 1], dp[e + 2], dp[e + 3]);
      }
    }
    __syncthreads();
    {   // L.v <- dpre W1: rows [32 (w >> 1), +32), column tiles 2 (w & 1) + {0, 1}
      const int mi = w >> 1;
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const int ct = 2 * (w & 1) + c2;
        f32x16 acc = splat(0.f);
        mma_xwt<LDG, LDG, kHid>(acc, L.dpre + 32 * mi * LDG, L.w1t + 32 * ct * LDG);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) L.v[(32 * mi + crow(reg, lane)) * LDC + 32 * ct + (lane & 31)] = acc[reg];
      }
    }
    __syncthreads();
    {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dvr[4 * j + e] += L.v[r * LDC + 4 * q + 16 * j + e];
          dot = fmaf(dvr[4 * j + e], x[4 * j + e], dot);
        }
      dot = group_sum<4>(dot);
      if (!(nz > a.eps)) dot = 0.f;
      if (ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<float4*>(a.dx + i * kD + 4 * q + 16 * j) =
              make_float4((dvr[4 * j] - x[4 * j] * dot) / nrm, (dvr[4 * j + 1] - x[4 * j + 1] * dot) / nrm,
                          (dvr[4 * j + 2] - x[4 * j + 2] * dot) / nrm, (dvr[4 * j + 3] - x[4 * j + 3] * dot) / nrm);
      }
    }
    __syncthreads();   // L.v is rewritten by the next tile
  }
  __syncthreads();
  float* red = L.w1;   // w1 | w1t | v are contiguous and no longer read
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int col = 4 * q + 16 * (k >> 2) + (k & 3);
    red[r * kFSmall + col] = alw[k];
    red[r * kFSmall + kD + col] = alb[k];
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    red[r * kFSmall + 2 * kD + 16 * q + e] = aw0[e];
    red[r * kFSmall + 2 * kD + kHid + 16 * q + e] = aw1[e];
  }
  if (q == 0) {
    red[r * kFSmall + 2 * kD + 2 * kHid] = ab0;
    red[r * kFSmall + 2 * kD + 2 * kHid + 1] = ab1;
  }
  __syncthreads();
  for (int c = tid; c < kFSmall; c += 256) {
    float s = 0.f;
    for (int rr = 0; rr < kFRows; ++rr) s += red[rr * kFSmall + c];
    a.part[(int64_t)blockIdx.x * kFSmall + c] = s;
  }
}

// out[b][c] = tok[b L + 0][c] + ... + tok[b L + L - 1][c], in that order
__global__ __launch_bounds__(256) void hybrid_user_sum_k(const float* __restrict__ tok, int64_t B, int64_t L,
                                                         float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * kD) return;
  const int64_t b = e / kD, c = e % kD;
  float s = 0.f;
  for (int64_t l = 0; l < L; ++l) s += tok[(b * L + l) * kD + c];
  out[e] = s;
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

// what the training form adds to the forward's arguments (null: the inference form)
struct AdapterTrain {
  float p_drop;
  uint64_t seed_c, seed_g;
  float* xc; float* xg; float* zc; float* zg;
};

// RSX_ARG under the calling entry point's name (adapter_forward, fuse_forward)
#define A_ARG(cond, msg)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      rsx::set_error("%s: invalid argument: %s", fn, msg);     \
      return 1;                                                \
    }                                                          \
  } while (0)
static int adapter_forward(const char* fn, const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn,
                           int64_t ldg, int64_t Ng, int64_t Dg, const int64_t* ids, int64_t first_row, int64_t R,
                           const float* wc, const float* bc, const float* lnc_w, const float* lnc_b, const float* wg,
                           const float* bg, const float* lng_w, const float* lng_b, float ln_eps, float eps,
                           const int64_t* deltas, const float* time_tab, float scale, float* merged, float* unit,
                           float* seq_in, int32_t* flag, const AdapterTrain* tr, void* stream) {
  A_ARG(Dc == kD && Dg == kG, "the content rows must be 128 wide and the GNN rows 64 wide");
  A_ARG(R >= 0 && Nc >= 0 && Ng >= 0, "negative size");
  A_ARG(ln_eps > 0.f && eps > 0.f, "eps must be positive");
  if (R == 0) return 0;
  A_ARG(content && gnn && Nc >= 1 && Ng >= 1, "null tensor (content / gnn table)");
  A_ARG(wc && bc && lnc_w && lnc_b && wg && bg && lng_w && lng_b && flag, "null tensor");
  A_ARG(merged || unit || seq_in, "no output requested");
  A_ARG(!seq_in || (deltas && time_tab), "seq_in needs deltas and time_tab");
  A_ARG(ids || (first_row >= 0 && first_row + R <= (Nc < Ng ? Nc : Ng)), "first_row + R exceeds the tables");
  A_ARG(ldc >= kD && ldc % 4 == 0 && ldg >= kG && ldg % 4 == 0, "bad leading dimensions");
  A_ARG(aligned16(content) && aligned16(gnn) && aligned16(wc) && aligned16(wg) && aligned16(lnc_w) &&
              aligned16(lnc_b) && aligned16(lng_w) && aligned16(lng_b) && aligned16(time_tab) && aligned16(merged) &&
              aligned16(unit) && aligned16(seq_in), "rows must be 16-byte aligned");
  if (tr) {
    A_ARG(tr->p_drop >= 0.f && tr->p_drop < 1.f, "p_drop must be in [0, 1)");
    A_ARG(tr->xc && tr->xg && tr->zc && tr->zg, "null tensor (saved rows / products)");
    A_ARG(aligned16(tr->xc) && aligned16(tr->xg) && aligned16(tr->zc) && aligned16(tr->zg),
            "rows must be 16-byte aligned");
  }
  static const int attr = raise_lds(hybrid_adapter_k<false>, sizeof(AdapterLds), "rsx_hybrid_adapter_fwd");
  static const int attr_t = raise_lds(hybrid_adapter_k<true>, sizeof(AdapterLds), "rsx_hybrid_adapter_train_fwd");
  if (attr || attr_t) return attr ? attr : attr_t;
  AdapterArgs a = {};
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
  if (tr) {
    a.drop_c = rsx::make_dropout(tr->p_drop, tr->seed_c);
    a.drop_g = rsx::make_dropout(tr->p_drop, tr->seed_g);
    a.xc_out = tr->xc; a.xg_out = tr->xg; a.zc_out = tr->zc; a.zg_out = tr->zg;
    hipLaunchKernelGGL(hybrid_adapter_k<true>, dim3((unsigned)grid), dim3(256), sizeof(AdapterLds), (hipStream_t)stream,
                       a);
  } else {
    hipLaunchKernelGGL(hybrid_adapter_k<false>, dim3((unsigned)grid), dim3(256), sizeof(AdapterLds),
                       (hipStream_t)stream, a);
  }
  RSX_LAUNCHED();
  return 0;
}


RSX_API int rsx_hybrid_adapter_fwd(const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn,
                                   int64_t ldg, int64_t Ng, int64_t Dg, const int64_t* ids, int64_t first_row,
                                   int64_t R, const float* wc, const float* bc, const float* lnc_w,
                                   const float* lnc_b, const float* wg, const float* bg, const float* lng_w,
                                   const float* lng_b, float ln_eps, float eps, const int64_t* deltas,
                                   const float* time_tab, float scale, float* merged, float* unit, float* seq_in,
                                   int32_t* flag, void* stream) {
  return adapter_forward(__func__, content, ldc, Nc, Dc, gnn, ldg, Ng, Dg, ids, first_row, R, wc, bc, lnc_w, lnc_b, wg,
                         bg, lng_w, lng_b, ln_eps, eps, deltas, time_tab, scale, merged, unit, seq_in, flag, nullptr,
                         stream);
}

// The adapter's training forward: rsx_hybrid_adapter_fwd's arithmetic with the two Dropout(p_drop) after
// the GELUs (keep = hash(seed, row * 128 + col) >= p 2^32; seed_c for the content branch, seed_g for the
// GNN branch), writing merged and / or seq_in and, for the backward, the gathered rows xc [R, 128],
// xg [R, 64] and the pre-LayerNorm products zc, zg [R, 128].
RSX_API int rsx_hybrid_adapter_train_fwd(const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn,
                                         int64_t ldg, int64_t Ng, int64_t Dg, const int64_t* ids, int64_t R,
                                         const float* wc, const float* bc, const float* lnc_w, const float* lnc_b,
                                         const float* wg, const float* bg, const float* lng_w, const float* lng_b,
                                         float ln_eps, const int64_t* deltas, const float* time_tab, float scale,
                                         float p_drop, uint64_t seed_c, uint64_t seed_g, float* merged,
                                         float* seq_in, float* xc, float* xg, float* zc, float* zg, int32_t* flag,
                                         void* stream) {
  RSX_ARG(ids || R == 0, "null tensor (ids)");
  const AdapterTrain tr = {p_drop, seed_c, seed_g, xc, xg, zc, zg};
  return adapter_forward(__func__, content, ldc, Nc, Dc, gnn, ldg, Ng, Dg, ids, 0, R, wc, bc, lnc_w, lnc_b, wg, bg,
                         lng_w, lng_b, ln_eps, 1e-12f, deltas, time_tab, scale, merged, nullptr, seq_in, flag, &tr,
                         stream);
}

static int64_t adapter_bwd_grid(int64_t R) {
  const int64_t tiles = (R + kARows - 1) / kARows;
  return tiles < rsx::cu_count() ? tiles : rsx::cu_count();
}

RSX_API int64_t rsx_hybrid_adapter_bwd_workspace_floats(int64_t R) { return R < 1 ? 0 : adapter_bwd_grid(R) * 4 * kD; }

// The adapter's backward from dy = d seq_in (gscale = the forward's scale) or d merged (gscale = 1),
// [R, 128]: dzc, dzg [R, 128], the gradients of the two pre-LayerNorm products (the operands of the weight
// gradients: dWc = dzc^T xc, dbc = column sums of dzc, and so for the GNN branch); dc [R, 128] = gscale dy +
// dzc Wc and dg [R, 64] = dzg Wg, the gradients of the gathered rows; dln [4][128] = d lnc_w, d lnc_b,
// d lng_w, d lng_b from per-workgroup partials in ws added in workgroup order. zc, zg, p_drop and the
// seeds are the forward's. No atomics: identical inputs give identical bits.
RSX_API int rsx_hybrid_adapter_bwd(const float* dy, float gscale, int64_t R, const float* zc, const float* zg,
                                   const float* wc, const float* wg, const float* lnc_w, const float* lnc_b,
                                   const float* lng_w, const float* lng_b, float ln_eps, float p_drop,
                                   uint64_t seed_c, uint64_t seed_g, float* dzc, float* dzg, float* dc, float* dg,
                                   float* dln, float* ws, int64_t ws_floats, void* stream) {
  RSX_ARG(R >= 0, "negative size");
  RSX_ARG(ln_eps > 0.f, "eps must be positive");
  RSX_ARG(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0, 1)");
  RSX_ARG(dln, "null tensor");
  if (R == 0) {
    (void)hipMemsetAsync(dln, 0, 4 * kD * sizeof(float), (hipStream_t)stream);
    RSX_LAUNCHED();
    return 0;
  }
  RSX_ARG(dy && zc && zg && wc && wg && lnc_w && lnc_b && lng_w && lng_b && dzc && dzg && dc && dg, "null tensor");
  RSX_ARG(aligned16(dy) && aligned16(zc) && aligned16(zg) && aligned16(lnc_w) && aligned16(lnc_b) &&
              aligned16(lng_w) && aligned16(lng_b) && aligned16(dzc) && aligned16(dzg), "rows must be 16-byte aligned");
  const int64_t grid = adapter_bwd_grid(R);
  RSX_ARG(ws && ws_floats >= grid * 4 * kD, "workspace of rsx_hybrid_adapter_bwd_workspace_floats(R) floats needed");
  static const int attr = raise_lds(hybrid_adapter_bwd_k, sizeof(AdapterBwdLds), "rsx_hybrid_adapter_bwd");
  if (attr) return attr;
  AdapterBwdArgs a;
  a.dy = dy; a.gscale = gscale; a.R = R;
  a.zc = zc; a.zg = zg; a.wc = wc; a.wg = wg;
  a.lnc_w = lnc_w; a.lnc_b = lnc_b; a.lng_w = lng_w; a.lng_b = lng_b;
  a.ln_eps = ln_eps;
  a.drop_c = rsx::make_dropout(p_drop, seed_c);
  a.drop_g = rsx::make_dropout(p_drop, seed_g);
  a.dzc = dzc; a.dzg = dzg; a.dc = dc; a.dg = dg;
  a.ln_part = ws;
  hipLaunchKernelGGL(hybrid_adapter_bwd_k, dim3((unsigned)grid), dim3(256), sizeof(AdapterBwdLds), (hipStream_t)stream,
                     a);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(hybrid_part_sum_k, dim3(2), dim3(256), 0, (hipStream_t)stream, (const float*)ws, (int)grid, 4 * kD,
                     dln);
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

struct FuseTrain {
  float p_drop;
  uint64_t seed_a, seed_b;
};

static int fuse_forward(const char* fn, const float* seq_out, int64_t B, int64_t L, int64_t D, const int64_t* rows,
                        int64_t n_rows, const float* u_gnn, const float* u_meta, const float* w1, const float* b1,
                        int64_t hidden, const float* w2, const float* b2, const float* ln_w, const float* ln_b,
                        float ln_eps, float eps, float* out, float* v_seq, float* gate_mean, void* ws,
                        int64_t ws_bytes, int32_t* flag, const FuseTrain* tr, void* stream) {
  A_ARG(D == kD && hidden == kHid, "the rows must be 128 wide and the gate's hidden layer 64 wide");
  A_ARG(B >= 0 && n_rows >= 0, "negative size");
  A_ARG(L >= 1 && L <= 64, "L must be in [1, 64]");
  A_ARG(ln_eps > 0.f && eps > 0.f, "eps must be positive");
  const int64_t n = rows ? n_rows : B * L;
  if (n == 0) return 0;
  A_ARG(B >= 1, "rows given for an empty batch");
  A_ARG(seq_out && u_gnn && u_meta && w1 && b1 && w2 && b2 && ln_w && ln_b && out && flag, "null tensor");
  A_ARG(aligned16(seq_out) && aligned16(u_gnn) && aligned16(u_meta) && aligned16(w1) && aligned16(ln_w) &&
              aligned16(ln_b) && aligned16(out) && aligned16(v_seq), "rows must be 16-byte aligned");
  const int64_t slots = rsx_hybrid_fuse_slots(n);
  A_ARG(!gate_mean || (ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= slots * 2 * (int64_t)sizeof(double)),
          "the gate means need a workspace of rsx_hybrid_fuse_slots(n) * 16 bytes");
  A_ARG(!tr || (tr->p_drop >= 0.f && tr->p_drop < 1.f), "p_drop must be in [0, 1)");
  static const int attr = raise_lds(hybrid_fuse_k<false>, sizeof(FuseLds), "rsx_hybrid_fuse_fwd");
  static const int attr_t = raise_lds(hybrid_fuse_k<true>, sizeof(FuseLds), "rsx_hybrid_fuse_train_fwd");
  if (attr || attr_t) return attr ? attr : attr_t;
  FuseArgs a = {};
  a.seq_out = seq_out; a.T = B * L; a.L = L;
  a.rows = rows; a.n = n; a.B = B;
  a.u_gnn = u_gnn; a.u_meta = u_meta;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.ln_w = ln_w; a.ln_b = ln_b;
  a.ln_eps = ln_eps; a.eps = eps;
  a.out = out; a.v_seq = v_seq;
  a.gate_part = gate_mean ? (double*)ws : nullptr;
  a.flag = flag;
  if (tr) {
    a.drop_a = rsx::make_dropout(tr->p_drop, tr->seed_a);
    a.drop_b = rsx::make_dropout(tr->p_drop, tr->seed_b);
    hipLaunchKernelGGL(hybrid_fuse_k<true>, dim3((unsigned)slots), dim3(256), sizeof(FuseLds), (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(hybrid_fuse_k<false>, dim3((unsigned)slots), dim3(256), sizeof(FuseLds), (hipStream_t)stream, a);
  }
  RSX_LAUNCHED();
  if (gate_mean) {
    hipLaunchKernelGGL(hybrid_gate_mean_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, (int)slots, n,
                       gate_mean);
    RSX_LAUNCHED();
  }
  return 0;
}
#undef A_ARG

RSX_API int rsx_hybrid_fuse_fwd(const float* seq_out, int64_t B, int64_t L, int64_t D, const int64_t* rows,
                                int64_t n_rows, const float* u_gnn, const float* u_meta, const float* w1,
                                const float* b1, int64_t hidden, const float* w2, const float* b2,
                                const float* ln_w, const float* ln_b, float ln_eps, float eps, float* out,
                                float* v_seq, float* gate_mean, void* ws, int64_t ws_bytes, int32_t* flag,
                                void* stream) {
  return fuse_forward(__func__, seq_out, B, L, D, rows, n_rows, u_gnn, u_meta, w1, b1, hidden, w2, b2, ln_w, ln_b,
                      ln_eps, eps, out, v_seq, gate_mean, ws, ws_bytes, flag, nullptr, stream);
}

// The fusion's training forward over all B L token rows: rsx_hybrid_fuse_fwd's arithmetic with each
// token's own Dropout(p_drop) masks over its copies of the two projected rows (the reference projects the
// expanded [B, L, 128] tensors): f = v + g0 drop_a(u_gnn[u]) + g1 drop_b(u_meta[u]), keep = hash(seed,
// token_row * 128 + col) >= p 2^32, seed_a for the GNN row, seed_b for the meta row. The gate means are
// those of the gates themselves, as in the inference form.
RSX_API int rsx_hybrid_fuse_train_fwd(const float* seq_out, int64_t B, int64_t L, const float* u_gnn,
                                      const float* u_meta, const float* w1, const float* b1, const float* w2,
                                      const float* b2, const float* ln_w, const float* ln_b, float ln_eps, float eps,
                                      float p_drop, uint64_t seed_a, uint64_t seed_b, float* out, float* v_seq,
                                      float* gate_mean, void* ws, int64_t ws_bytes, int32_t* flag, void* stream) {
  const FuseTrain tr = {p_drop, seed_a, seed_b};
  return fuse_forward(__func__, seq_out, B, L, kD, nullptr, 0, u_gnn, u_meta, w1, b1, kHid, w2, b2, ln_w, ln_b, ln_eps,
                      eps, out, v_seq, gate_mean, ws, ws_bytes, flag, &tr, stream);
}

RSX_API int64_t rsx_hybrid_fuse_bwd_workspace_floats(int64_t B, int64_t L) {
  const int64_t n = B * L;
  return n < 1 ? 0 : 2 * n * kD + rsx_hybrid_fuse_slots(n) * kFSmall;
}

// The fusion's backward from dout (and dv, the gradient of v_seq; nullable), recomputing the forward from
// its inputs: dx [B L, 128] = d seq_out; dpre [B L, 64], the gradient of the gate's pre-activations (dW1 =
// dpre^T v_seq, db1 = its column sums); du_gnn, du_meta [B, 128], each user's L token rows added in
// position order; dsmall [386] = d ln_w [128] | d ln_b [128] | d W2 [2][64] | d b2 [2] from per-workgroup
// partials added in workgroup order. ws: rsx_hybrid_fuse_bwd_workspace_floats(B, L) floats.
RSX_API int rsx_hybrid_fuse_bwd(const float* seq_out, int64_t B, int64_t L, const float* u_gnn, const float* u_meta,
                                const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* ln_w, const float* ln_b, float ln_eps, float eps, float p_drop,
                                uint64_t seed_a, uint64_t seed_b, const float* dout, const float* dv, float* dx,
                                float* dpre, float* du_gnn, float* du_meta, float* dsmall, float* ws,
                                int64_t ws_floats, void* stream) {
  RSX_ARG(B >= 0, "negative size");
  RSX_ARG(L >= 1 && L <= 64, "L must be in [1, 64]");
  RSX_ARG(ln_eps > 0.f && eps > 0.f, "eps must be positive");
  RSX_ARG(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0, 1)");
  RSX_ARG(dsmall, "null tensor");
  const int64_t n = B * L;
  if (n == 0) {
    (void)hipMemsetAsync(dsmall, 0, kFSmall * sizeof(float), (hipStream_t)stream);
    RSX_LAUNCHED();
    return 0;
  }
  RSX_ARG(seq_out && u_gnn && u_meta && w1 && b1 && w2 && b2 && ln_w && ln_b && dout && dx && dpre && du_gnn &&
              du_meta, "null tensor");
  RSX_ARG(aligned16(seq_out) && aligned16(u_gnn) && aligned16(u_meta) && aligned16(w1) && aligned16(ln_w) &&
              aligned16(ln_b) && aligned16(dout) && aligned16(dv) && aligned16(dx) && aligned16(dpre),
          "rows must be 16-byte aligned");
  const int64_t slots = rsx_hybrid_fuse_slots(n);
  RSX_ARG(ws && aligned16(ws) && ws_floats >= rsx_hybrid_fuse_bwd_workspace_floats(B, L),
          "workspace of rsx_hybrid_fuse_bwd_workspace_floats(B, L) floats needed");
  RSX_ARG((B * kD + 255) / 256 < (1LL << 31), "too many users");
  static const int attr = raise_lds(hybrid_fuse_bwd_k, sizeof(FuseBwdLds), "rsx_hybrid_fuse_bwd");
  if (attr) return attr;
  FuseBwdArgs a;
  a.seq_out = seq_out; a.n = n; a.L = L; a.B = B;
  a.u_gnn = u_gnn; a.u_meta = u_meta;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.ln_w = ln_w; a.ln_b = ln_b;
  a.ln_eps = ln_eps; a.eps = eps;
  a.drop_a = rsx::make_dropout(p_drop, seed_a);
  a.drop_b = rsx::make_dropout(p_drop, seed_b);
  a.dout = dout; a.dv = dv;
  a.dx = dx; a.dpre = dpre;
  a.dug_tok = ws; a.dum_tok = ws + n * kD;
  a.part = ws + 2 * n * kD;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hybrid_fuse_bwd_k, dim3((unsigned)slots), dim3(256), sizeof(FuseBwdLds), st, a);
  RSX_LAUNCHED();
  const unsigned ub = (unsigned)((B * kD + 255) / 256);
  hipLaunchKernelGGL(hybrid_user_sum_k, dim3(ub), dim3(256), 0, st, (const float*)a.dug_tok, B, L, du_gnn);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(hybrid_user_sum_k, dim3(ub), dim3(256), 0, st, (const float*)a.dum_tok, B, L, du_meta);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(hybrid_part_sum_k, dim3((kFSmall + 255) / 256), dim3(256), 0, st, (const float*)a.part, (int)slots,
                     kFSmall, dsmall);
  RSX_LAUNCHED();
  return 0;
}
