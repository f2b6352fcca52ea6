// DeepFM training step: Logloss head, backward glue and the sparse Adam update of the per-field
// tables (the forward's model is csrc/deepfm.hip's: deepctr-torch 0.2.9 DeepFM semantics). The
// reference trains the ranker in this slot before using it (RecommendationRanker.train, CatBoost
// loss_function="Logloss", temp_model/ranker_skelet.py:114-137); deepctr-torch's own fit() cannot
// be run against this tree, so as for the forward: parity unpinned. The arithmetic is pinned by
// oracle/deepfm.py + binary_cross_entropy_with_logits + torch.optim.SparseAdam / Adam instead.
//
// One step (ops.deepfm_train_step orders the calls; nothing here reads a size on the host):
//   keys_k          x [R, F] -> one int64 key (field << 40 | id) per (row, field), the checked ids
//                   (an id outside its field's vocab -> 0 for the gathers, key id = kDropped,
//                   device flag set); the caller sorts the keys (one stable sort)
//   seg_heads_k     sorted keys -> head flag per sorted position, inverse permutation
//   seg_starts_k    inclusive scan of the flags -> segment starts [U + 1] and U on the device
//   (forward: rsx_deepfm_embed + 2 x rsx_linear_fwd keep emb, h1, h2)
//   head_k/_sum_k   logit, per-row loss (double), g_r = dloss/dlogit, dh2 = g wo [h2 > 0], and
//                   per-64-row partials of sum loss, sum g, dwo reduced in a fixed two-level order
//   relu_bwd_k      dx *= [h > 0]
//   (dense backward: rsx_linear_wgrad(_x3), rsx_gemm_x3_tn)
//   contrib_k       per (row, field): g_r (S_r - v_rf) + dE[r, f] (16 floats) and g_r, stored ONCE
//                   at the pair's sorted position (plain stores through the inverse permutation)
//   tile_partial_k  segments longer than kLong: every aligned kTile-run inside one is summed by its
//                   own lanes (hot ids do not serialise on one wave)
//   sparse_adam_k   per distinct (field, id): contributions in sorted order (or unaligned head +
//                   tile partials in tile order), then the SparseAdam row update of V_f, W_f and
//                   their moments. Only touched rows are read or written; no float atomics; the
//                   same state and batch give bit-identical tables.
#include "rsx_common.h"
#include <math.h>

namespace {

constexpr int kMaxFields = 64;
constexpr int kIdBits = 40;
constexpr int64_t kDropped = ((int64_t)1 << kIdBits) - 1;  // key id of a contribution that is not applied
constexpr int kTile = 64;         // contributions per partial sum of a long segment
constexpr int kLong = 2 * kTile;  // segments up to this length are summed by their own lanes
constexpr int kHeadCols = 128;    // h2 width
constexpr int kHeadSlot = 132;    // floats per block partial: dwo [128], sum g, pad

struct KeyArgs {
  const int64_t* x;
  int64_t n;
  int F;
  int64_t vocab[kMaxFields];
  int64_t* keys;
  int64_t* xs;
  int* flag;
};

__global__ __launch_bounds__(256) void keys_k(KeyArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int f = (int)(i % a.F);
  const int64_t id = a.x[i];
  const bool ok = id >= 0 && id < a.vocab[f];
  a.keys[i] = ((int64_t)f << kIdBits) | (ok ? id : kDropped);
  a.xs[i] = ok ? id : 0;
  if (!ok) *a.flag = 1;
}

__global__ __launch_bounds__(256) void seg_heads_k(const int64_t* __restrict__ ks, const int64_t* __restrict__ perm,
                                                   int64_t n, int* __restrict__ head, int* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || ks[i] != ks[i - 1]) ? 1 : 0;
  const int64_t p = perm[i];
  if (p >= 0 && p < n) inv[p] = (int)i;
}

__global__ __launch_bounds__(256) void seg_starts_k(const int* __restrict__ cum, int64_t n, int* __restrict__ seg_start,
                                                    int* __restrict__ nseg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = cum[i];
  if (c < 1 || c > n) return;
  if (i == 0 || cum[i - 1] != c) seg_start[c - 1] = (int)i;
  if (i == n - 1) {
    seg_start[c] = (int)n;
    *nseg = c;
  }
}

// ---------------------------------------------------------------------------------------
struct HeadArgs {
  const float* h2;   // [R, 128]
  const float* wo;   // [128]
  const float* lin;  // [R] first order + FM (+ bias when bias is null)
  const float* bias; // [1] added to every logit (nullable)
  const float* y;    // [R] labels
  int64_t R;
  float scale;       // 1/R (mean) or 1 (sum)
  float* logit;      // [R]
  float* g;          // [R]
  float* dh2;        // [R, 128]
  float* pf;         // [blocks, kHeadSlot]
  double* pl;        // [blocks]
};

// 64 rows per workgroup, 4 lanes per row (32 columns each). kReluMask: dh2 = g wo [h2 > 0] (the
// DeepFM DNN ends in a ReLU); without it dh2 = g wo (the DCN-V2 ranker's h2 is a GELU output, whose
// derivative the LayerNorm backward applies).
template <bool kReluMask>
__global__ __launch_bounds__(256) void head_k(HeadArgs a) {
  __shared__ float sG[64];
  __shared__ double sL[64];
  const int tid = threadIdx.x, row = tid >> 2, q = tid & 3;
  const int64_t r = (int64_t)blockIdx.x * 64 + row;
  const bool live = r < a.R;
  const float4* wp = reinterpret_cast<const float4*>(a.wo + q * 32);
  float4 hv[8];
  float dot = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) hv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4* hp = reinterpret_cast<const float4*>(a.h2 + r * kHeadCols + q * 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      hv[j] = hp[j];
      const float4 w = wp[j];
      dot += hv[j].x * w.x + hv[j].y * w.y + hv[j].z * w.z + hv[j].w * w.w;
    }
  }
  dot += __shfl_xor(dot, 1, 64);
  dot += __shfl_xor(dot, 2, 64);
  float gr = 0.0f;
  double loss = 0.0;
  if (live) {
    const float z = dot + a.lin[r] + (a.bias ? a.bias[0] : 0.0f);
    const float yy = a.y[r];
    if (q == 0) {  // one lane per row takes the double-precision loss
      const double zd = (double)z;
      loss = fmax(zd, 0.0) - zd * (double)yy + log1p(exp(-fabs(zd)));
    }
    const float e = expf(-fabsf(z));
    const float sig = z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
    gr = (sig - yy) * a.scale;
    if (q == 0) {
      a.logit[r] = z;
      a.g[r] = gr;
    }
    float4* dp = reinterpret_cast<float4*>(a.dh2 + r * kHeadCols + q * 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 w = wp[j];
      float4 o;
      o.x = !kReluMask || hv[j].x > 0.0f ? gr * w.x : 0.0f;
      o.y = !kReluMask || hv[j].y > 0.0f ? gr * w.y : 0.0f;
      o.z = !kReluMask || hv[j].z > 0.0f ? gr * w.z : 0.0f;
      o.w = !kReluMask || hv[j].w > 0.0f ? gr * w.w : 0.0f;
      dp[j] = o;
    }
  }
  if (q == 0) {
    sG[row] = gr;
    sL[row] = loss;
  }
  __syncthreads();
  if (tid < kHeadCols) {
    float acc = 0.0f;
    for (int rr = 0; rr < 64; ++rr) {
      const int64_t r2 = (int64_t)blockIdx.x * 64 + rr;
      if (r2 < a.R) acc += sG[rr] * a.h2[r2 * kHeadCols + tid];
    }
    a.pf[(int64_t)blockIdx.x * kHeadSlot + tid] = acc;
  } else if (tid == kHeadCols) {
    float acc = 0.0f;
    for (int rr = 0; rr < 64; ++rr) acc += sG[rr];
    a.pf[(int64_t)blockIdx.x * kHeadSlot + kHeadCols] = acc;
  } else if (tid == kHeadCols + 1) {
    double acc = 0.0;
    for (int rr = 0; rr < 64; ++rr) acc += sL[rr];
    a.pl[blockIdx.x] = acc;
  }
}

// Fixed-slot partials in a fixed two-level order: one wave per output (128 dwo columns, sum g, the
// loss); lane l adds its contiguous run of blocks in block order, lane 0 adds the 64 lane sums in
// lane order.
__global__ __launch_bounds__(64) void head_sum_k(const float* __restrict__ pf, const double* __restrict__ pl,
                                                 int64_t blocks, double loss_scale, double* __restrict__ loss,
                                                 float* __restrict__ dbias, float* __restrict__ dwo) {
  __shared__ double sPart[64];
  const int out = blockIdx.x, lane = threadIdx.x;
  const int64_t per = (blocks + 63) / 64;
  const int64_t b0 = lane * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  if (out <= kHeadCols) {
    float acc = 0.0f;
    for (int64_t b = b0; b < b1; ++b) acc += pf[b * kHeadSlot + out];
    sPart[lane] = (double)acc;
  } else {
    double acc = 0.0;
    for (int64_t b = b0; b < b1; ++b) acc += pl[b];
    sPart[lane] = acc;
  }
  __syncthreads();
  if (lane != 0) return;
  if (out <= kHeadCols) {
    float acc = 0.0f;
    for (int l = 0; l < 64; ++l) acc += (float)sPart[l];
    if (out < kHeadCols) dwo[out] = acc;
    else dbias[0] = acc;
  } else {
    double acc = 0.0;
    for (int l = 0; l < 64; ++l) acc += sPart[l];
    loss[0] = acc * loss_scale;
  }
}

__global__ __launch_bounds__(256) void relu_bwd_k(float4* __restrict__ dx, const float4* __restrict__ h, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 d = dx[i];
  const float4 v = h[i];
  d.x = v.x > 0.0f ? d.x : 0.0f;
  d.y = v.y > 0.0f ? d.y : 0.0f;
  d.z = v.z > 0.0f ? d.z : 0.0f;
  d.w = v.w > 0.0f ? d.w : 0.0f;
  dx[i] = d;
}

// ---------------------------------------------------------------------------------------
struct ContribArgs {
  const float* emb;  // [R, F*16] the forward's gathered rows
  const float* g;    // [R]
  const float* dE;   // [R, ldE] DNN input gradient
  int64_t ldE;
  const int* inv;    // [R*F] sorted position of pair (r, f)
  int64_t R;
  int F;
  float* gV;         // [R*F, 16] by sorted position
  float* gW;         // [R*F]
};

// As deepfm_embed_k: a row is owned by 4 lanes (one float4 of every field each).
__global__ __launch_bounds__(256) void contrib_k(ContribArgs a) {
  const int64_t r = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  if (r >= a.R) return;
  const int64_t n = a.R * a.F;
  const float4* __restrict__ er = reinterpret_cast<const float4*>(a.emb + r * (int64_t)a.F * 16);
  const float* __restrict__ de = a.dE + r * a.ldE;
  const int* __restrict__ iv = a.inv + r * a.F;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int f = 0; f < a.F; ++f) {
    const float4 v = er[f * 4 + q];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float gr = a.g[r];
  for (int f = 0; f < a.F; ++f) {
    const float4 v = er[f * 4 + q];
    const float4 d = reinterpret_cast<const float4*>(de + f * 16)[q];
    const int64_t pos = iv[f];
    float4 o;
    o.x = gr * (s.x - v.x) + d.x;
    o.y = gr * (s.y - v.y) + d.y;
    o.z = gr * (s.z - v.z) + d.z;
    o.w = gr * (s.w - v.w) + d.w;
    if (pos >= 0 && pos < n) {
      reinterpret_cast<float4*>(a.gV + pos * 16)[q] = o;
      if (q == 0) a.gW[pos] = gr;
    }
  }
}

// ---------------------------------------------------------------------------------------
struct SparseArgs {
  const int64_t* keys;   // [n] sorted
  const int* cum;        // [n] inclusive scan of the head flags (segment index + 1)
  const int* seg_start;  // [U + 1]
  const int* nseg;       // U
  int64_t n;
  int F;
  const float* gV;
  const float* gW;
  float* pV;             // [tiles, 16]
  float* pW;             // [tiles]
  float* V[kMaxFields];
  float* W[kMaxFields];
  float* mV[kMaxFields];
  float* vV[kMaxFields];
  float* mW[kMaxFields];
  float* vW[kMaxFields];
  int64_t vocab[kMaxFields];
  float step_size, omb1, omb2, eps;  // omb = 1 - beta, rounded once from the double
  float* oV;             // [n, 16] coalesced gradient per segment (nullable)
  float* oW;             // [n]
};

__device__ __forceinline__ void add4(float4& a, const float4 b) {
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
}

// 4 lanes per aligned tile of kTile sorted positions; acts only when the tile's first position lies
// in a long segment, and sums that segment's positions inside the tile.
__global__ __launch_bounds__(256) void tile_partial_k(SparseArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  const int64_t p0 = t * kTile;
  if (p0 >= a.n) return;
  const int64_t sid = (int64_t)a.cum[p0] - 1;
  if (sid < 0 || sid >= a.n) return;
  const int64_t s = a.seg_start[sid];
  int64_t e = a.seg_start[sid + 1];
  if (e > a.n) e = a.n;
  if (s < 0 || s > p0 || e - s <= kLong) return;
  const int64_t end = e < p0 + kTile ? e : p0 + kTile;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float w = 0.0f;
  for (int64_t p = p0; p < end; ++p) {
    add4(acc, reinterpret_cast<const float4*>(a.gV + p * 16)[q]);
    if (q == 0) w += a.gW[p];
  }
  reinterpret_cast<float4*>(a.pV + t * 16)[q] = acc;
  if (q == 0) a.pW[t] = w;
}

__device__ __forceinline__ float adam_elem(float g, float& m, float& v, float omb1, float omb2, float eps) {
  m = m + (g - m) * omb1;
  v = v + (g * g - v) * omb2;
  return m / (sqrtf(v) + eps);
}

// 4 lanes per distinct (field, id).
__global__ __launch_bounds__(256) void sparse_adam_k(SparseArgs a) {
  const int64_t sg = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  const int64_t ns = *a.nseg;
  if (sg >= ns || sg >= a.n) return;
  const int64_t s = a.seg_start[sg];
  int64_t e = a.seg_start[sg + 1];
  if (e > a.n) e = a.n;
  if (s < 0 || s >= e) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float w = 0.0f;
  if (e - s <= kLong) {
    for (int64_t p = s; p < e; ++p) {
      add4(acc, reinterpret_cast<const float4*>(a.gV + p * 16)[q]);
      if (q == 0) w += a.gW[p];
    }
  } else {
    const int64_t h = (s + kTile - 1) / kTile * kTile;  // first aligned tile of the segment
    for (int64_t p = s; p < h; ++p) {
      add4(acc, reinterpret_cast<const float4*>(a.gV + p * 16)[q]);
      if (q == 0) w += a.gW[p];
    }
    for (int64_t t = h / kTile; t * kTile < e; ++t) {
      add4(acc, reinterpret_cast<const float4*>(a.pV + t * 16)[q]);
      if (q == 0) w += a.pW[t];
    }
  }
  if (a.oV) {
    reinterpret_cast<float4*>(a.oV + sg * 16)[q] = acc;
    if (q == 0) a.oW[sg] = w;
  }
  const int64_t key = a.keys[s];
  const int64_t f = key >> kIdBits, id = key & kDropped;
  if (f < 0 || f >= a.F) return;
  if (id == kDropped || id >= a.vocab[f]) return;  // a dropped (out-of-range) contribution
  float4* pp = reinterpret_cast<float4*>(a.V[f] + id * 16) + q;
  float4* mp = reinterpret_cast<float4*>(a.mV[f] + id * 16) + q;
  float4* vp = reinterpret_cast<float4*>(a.vV[f] + id * 16) + q;
  float4 p = *pp, m = *mp, v = *vp;
  p.x -= a.step_size * adam_elem(acc.x, m.x, v.x, a.omb1, a.omb2, a.eps);
  p.y -= a.step_size * adam_elem(acc.y, m.y, v.y, a.omb1, a.omb2, a.eps);
  p.z -= a.step_size * adam_elem(acc.z, m.z, v.z, a.omb1, a.omb2, a.eps);
  p.w -= a.step_size * adam_elem(acc.w, m.w, v.w, a.omb1, a.omb2, a.eps);
  *pp = p;
  *mp = m;
  *vp = v;
  if (q == 0) {
    float pw = a.W[f][id], mw = a.mW[f][id], vw = a.vW[f][id];
    pw -= a.step_size * adam_elem(w, mw, vw, a.omb1, a.omb2, a.eps);
    a.W[f][id] = pw;
    a.mW[f][id] = mw;
    a.vW[f][id] = vw;
  }
}

using rsx::aligned16;
inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

#define RSX_TRAIN_SHAPE(R, F)                                                   \
  RSX_ARG((F) >= 1 && (F) <= kMaxFields, "F must be in [1,64]");                \
  RSX_ARG((R) >= 0 && (R) * (int64_t)(F) < ((int64_t)1 << 31), "R * F must be below 2^31")

RSX_API int rsx_deepfm_train_keys(const int64_t* x, int64_t R, int F, const int64_t* vocab, int64_t* keys,
                                  int64_t* xs, int* flag, void* stream) {
  RSX_ARG(x && vocab && keys && xs && flag, "null tensor");
  RSX_TRAIN_SHAPE(R, F);
  KeyArgs a = {};
  for (int f = 0; f < F; ++f) {
    RSX_ARG(vocab[f] >= 1 && vocab[f] < kDropped, "field vocab must be in [1, 2^40 - 1)");
    a.vocab[f] = vocab[f];
  }
  if (R == 0) return 0;
  a.x = x; a.n = R * F; a.F = F; a.keys = keys; a.xs = xs; a.flag = flag;
  hipLaunchKernelGGL(keys_k, dim3(blocks_of(a.n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_deepfm_train_segments(const int64_t* keys_sorted, const int64_t* perm, int64_t n, int* head, int* inv,
                                      void* stream) {
  RSX_ARG(keys_sorted && perm && head && inv, "null tensor");
  RSX_ARG(n >= 0 && n < ((int64_t)1 << 31), "n must be below 2^31");
  if (n == 0) return 0;
  hipLaunchKernelGGL(seg_heads_k, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)stream, keys_sorted, perm, n, head,
                     inv);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_deepfm_train_starts(const int* head_cum, int64_t n, int* seg_start, int* nseg, void* stream) {
  RSX_ARG(head_cum && seg_start && nseg, "null tensor");
  RSX_ARG(n >= 1 && n < ((int64_t)1 << 31), "n must be in [1, 2^31)");
  hipLaunchKernelGGL(seg_starts_k, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)stream, head_cum, n, seg_start,
                     nseg);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int64_t rsx_deepfm_train_head_workspace_bytes(int64_t R) {
  const int64_t blocks = (R + 63) / 64;
  return blocks * (kHeadSlot * (int64_t)sizeof(float) + (int64_t)sizeof(double));
}

// The two launches of the Logloss head, shared with rsx_dcn_train_head (csrc/dcn_train.hip), which
// checks its own arguments: ws holds rsx_deepfm_train_head_workspace_bytes(R) bytes.
int rsx::train_head_launch(const float* h2, const float* wo, const float* lin, const float* bias, const float* y,
                           int64_t R, int mean, bool relu_mask, float* logit, float* g, float* dh2, void* ws,
                           double* loss, float* dbias, float* dwo, void* stream) {
  const int64_t blocks = (R + 63) / 64;
  HeadArgs a = {};
  a.h2 = h2; a.wo = wo; a.lin = lin; a.bias = bias; a.y = y; a.R = R;
  a.scale = mean ? (float)(1.0 / (double)R) : 1.0f;
  a.logit = logit; a.g = g; a.dh2 = dh2;
  a.pl = reinterpret_cast<double*>(ws);  // doubles first: 8-byte aligned
  a.pf = reinterpret_cast<float*>(a.pl + blocks);
  if (relu_mask) hipLaunchKernelGGL(head_k<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_k<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(head_sum_k, dim3(kHeadCols + 2), dim3(64), 0, (hipStream_t)stream, a.pf, a.pl, blocks,
                     mean ? 1.0 / (double)R : 1.0, loss, dbias, dwo);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_deepfm_train_head(const float* h2, int64_t H, const float* wo, const float* lin, const float* bias,
                                  const float* y, int64_t R, int mean, float* logit, float* g, float* dh2, void* ws, int64_t ws_bytes,
                                  double* loss, float* dbias, float* dwo, void* stream) {
  RSX_ARG(h2 && wo && lin && y && logit && g && dh2 && ws && loss && dbias && dwo, "null tensor");
  RSX_ARG(H == kHeadCols, "the last hidden layer must be 128 wide");
  RSX_ARG(aligned16(h2) && aligned16(wo) && aligned16(dh2) && aligned16(ws), "h2, wo, dh2 and ws must be 16-byte aligned");
  RSX_ARG(R >= 1, "R must be positive");
  RSX_ARG(mean == 0 || mean == 1, "mean must be 0 (sum) or 1 (mean)");
  RSX_ARG(ws_bytes >= rsx_deepfm_train_head_workspace_bytes(R), "workspace too small");
  return rsx::train_head_launch(h2, wo, lin, bias, y, R, mean, true, logit, g, dh2, ws, loss, dbias, dwo, stream);
}

RSX_API int rsx_relu_bwd(float* dx, const float* h, int64_t n, void* stream) {
  RSX_ARG(dx && h, "null tensor");
  RSX_ARG(n >= 0 && n % 4 == 0, "n must be a multiple of 4");
  RSX_ARG(aligned16(dx) && aligned16(h), "dx and h must be 16-byte aligned");
  if (n == 0) return 0;
  hipLaunchKernelGGL(relu_bwd_k, dim3(blocks_of(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<float4*>(dx), reinterpret_cast<const float4*>(h), n / 4);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_deepfm_train_contrib(const float* emb, const float* g, const float* dE, int64_t ldE, const int* inv,
                                     int64_t R, int F, int E, float* gV, float* gW, void* stream) {
  RSX_ARG(emb && g && dE && inv && gV && gW, "null tensor");
  RSX_TRAIN_SHAPE(R, F);
  RSX_ARG(E == 16, "embedding dim must be 16");
  RSX_ARG(ldE >= (int64_t)F * 16 && ldE % 4 == 0, "ldE must cover F*16 columns and be a multiple of 4");
  RSX_ARG(aligned16(emb) && aligned16(dE) && aligned16(gV), "emb, dE and gV must be 16-byte aligned");
  if (R == 0) return 0;
  ContribArgs a = {emb, g, dE, ldE, inv, R, F, gV, gW};
  hipLaunchKernelGGL(contrib_k, dim3(blocks_of(R, 64)), dim3(256), 0, (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int64_t rsx_deepfm_train_sparse_workspace_bytes(int64_t n) {
  return (n + kTile - 1) / kTile * 17 * (int64_t)sizeof(float);
}

RSX_API int rsx_deepfm_train_sparse_adam(const int64_t* keys_sorted, const int* head_cum, const int* seg_start,
                                         const int* nseg, int64_t n, int F, int E, const int64_t* vocab,
                                         const float* gV, const float* gW, float* const* V, float* const* W,
                                         float* const* mV, float* const* vV, float* const* mW, float* const* vW,
                                         double lr, double beta1, double beta2, double eps, int64_t step, void* ws,
                                         int64_t ws_bytes, float* out_dV, float* out_dW, void* stream) {
  RSX_ARG(keys_sorted && head_cum && seg_start && nseg && vocab && gV && gW && V && W && mV && vV && mW && vW && ws,
          "null tensor");
  RSX_ARG(F >= 1 && F <= kMaxFields, "F must be in [1,64]");
  RSX_ARG(E == 16, "embedding dim must be 16");
  RSX_ARG(n >= 1 && n < ((int64_t)1 << 31), "n must be in [1, 2^31)");
  RSX_ARG(step >= 1, "step counts from 1");
  RSX_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas must be in [0, 1)");
  RSX_ARG((out_dV == nullptr) == (out_dW == nullptr), "out_dV and out_dW go together");
  RSX_ARG(ws_bytes >= rsx_deepfm_train_sparse_workspace_bytes(n), "workspace too small");
  RSX_ARG(aligned16(gV) && aligned16(ws) && aligned16(out_dV), "gV, ws and out_dV must be 16-byte aligned");
  SparseArgs a = {};
  for (int f = 0; f < F; ++f) {
    RSX_ARG(V[f] && W[f] && mV[f] && vV[f] && mW[f] && vW[f], "null field table");
    RSX_ARG(aligned16(V[f]) && aligned16(mV[f]) && aligned16(vV[f]), "field tables must be 16-byte aligned");
    RSX_ARG(vocab[f] >= 1 && vocab[f] < kDropped, "field vocab must be in [1, 2^40 - 1)");
    a.V[f] = V[f]; a.W[f] = W[f]; a.mV[f] = mV[f]; a.vV[f] = vV[f]; a.mW[f] = mW[f]; a.vW[f] = vW[f];
    a.vocab[f] = vocab[f];
  }
  const int64_t tiles = (n + kTile - 1) / kTile;
  a.keys = keys_sorted; a.cum = head_cum; a.seg_start = seg_start; a.nseg = nseg; a.n = n; a.F = F;
  a.gV = gV; a.gW = gW;
  a.pV = reinterpret_cast<float*>(ws);
  a.pW = a.pV + tiles * 16;
  // torch.optim.SparseAdam: step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
  a.step_size = (float)(lr * sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step)));
  a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
  a.oV = out_dV; a.oW = out_dW;
  hipLaunchKernelGGL(tile_partial_k, dim3(blocks_of(tiles, 64)), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sparse_adam_k, dim3(blocks_of(n, 64)), dim3(256), 0, (hipStream_t)stream, a);
  RSX_LAUNCHED();
  return 0;
}
