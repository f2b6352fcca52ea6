// The listwise objective of the oblivious-tree model: QuerySoftMax, the group-normalised softmax loss the
// reference's per-customer ranker rows (utils/monitor/log_importer.py: X_user, X_item, y, groups) are made
// for. Specified in include/recsys_amd.h ("QuerySoftMax") and restated in int64 / float64 numpy by
// tests/gbdt_rank_ref.py. The rows arrive in group order: row_group [R] is each row's dense group index
// and goff [G + 1] the groups' offsets (ops.GBDTGroupPlan).
//
// Every reduction over a group is order-free: the maximum is a maximum of ordered integer keys, Z a sum
// of int64 fixed-point terms and S a count, so the gradients do not depend on the order of the rows, of
// the tiles or of the atomics, and every run gives the same bits. No thread walks a group: each pass is
// one row per thread over fixed 256-row tiles, a segmented workgroup scan (rsx_block.h, the operator
// below) combines the rows of a group inside the tile, and the last row of every (group, tile) piece
// hands the piece's value to the group's slot in the workspace: a plain store when the whole group lies
// in the tile, an integer atomic when it crosses a tile edge. One group of all R rows costs what R
// groups of one row cost.
//   qs_max_k    mkey[q] = max ordered_key(a_i)                      (unsigned atomicMax)
//   qs_sum_k    zs[q] = (Z_q = sum E_i, S_q = #{y_i = 1}), E_i = llrint(exp(a_i - m_q) 2^32)  (64-bit atomicAdd)
//   qs_grad_k   p_i = (float)(E_i / Z_q), g = t - p, h = p (1 - p) -> qg, qh as rsx_gbdt_grad writes them
//   qs_loss_k   the monitoring loss: per-workgroup fp64 partials in a fixed order, qs_loss_sum_k adds them
// E_i is recomputed by qs_grad_k (the same expression on the same inputs: the same bits) rather than kept:
// the stage then moves some 30 bytes per row.
#include "rsx_block.h"
#include "rsx_common.h"
#include "rsx_x3.h"

namespace {

using rsx::at, rsx::block_scan_excl, rsx::ordered_key, rsx::ordered_key_inv, rsx::Seg, rsx::SegOp;

constexpr int kThreads = 256;      // rows per tile: one row per thread
constexpr int kLossSlots = 1024;   // workgroups of qs_loss_k (each one partial)
constexpr double kTwo32 = 4294967296.0;

// ---- the segmented scan (rsx_block.h: Seg, SegOp) over these values ---------------------------------------
struct MaxU {
  __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a > b ? a : b; }
};
struct ZS {
  unsigned long long z, s;
};
struct AddZS {
  __device__ __forceinline__ ZS operator()(ZS a, ZS b) const { return ZS{a.z + b.z, a.s + b.s}; }
};

// What a row knows of its group and its tile [t0, t0 + 256): a row past R, or one whose group index is
// not in [0, G) (its gradients are 0), is not live and starts a segment of its own, so nothing flows
// through it. tail: the last row of its group's piece in this tile; inside: the group lies in the tile.
struct Row {
  int q;
  bool live, head, tail, inside;
};
__device__ __forceinline__ Row row_of(const int* __restrict__ row_group, const int* __restrict__ goff, int64_t r,
                                      int64_t R, int G, int64_t t0) {
  Row c{0, false, true, false, false};
  if (r >= R) return c;
  const int q = row_group[r];
  if ((unsigned)q >= (unsigned)G) return c;
  const int64_t t1 = t0 + kThreads < R ? t0 + kThreads : R;
  const int64_t lo = goff[q], hi = goff[q + 1];
  c.q = q;
  c.live = true;
  c.head = r == lo;
  c.tail = r == hi - 1 || r == t1 - 1;
  c.inside = lo >= t0 && hi <= t1;
  return c;
}

__device__ __forceinline__ unsigned long long softmax_term(float a, float m) {
  return (unsigned long long)llrint(exp((double)a - (double)m) * kTwo32);   // in [0, 2^32]: a <= m
}

// ---- m_q ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void qs_max_k(const float* __restrict__ F, const int* __restrict__ row_group,
                                                     const int* __restrict__ goff, int64_t R, int G,
                                                     unsigned* __restrict__ mkey) {
  __shared__ Seg<unsigned> sm[kThreads / 64];
  const int64_t t0 = (int64_t)blockIdx.x * kThreads, r = t0 + threadIdx.x;
  const Row c = row_of(row_group, goff, r, R, G, t0);
  const Seg<unsigned> x{c.live ? ordered_key(F[r]) : 0u, c.head ? 1 : 0};
  Seg<unsigned> tot;
  const SegOp<unsigned, MaxU> op;
  const Seg<unsigned> before = block_scan_excl<kThreads, false>(x, op, Seg<unsigned>{0u, 0}, sm, tot);
  if (!c.live || !c.tail) return;
  const unsigned k = op(before, x).v;
  if (c.inside)
    mkey[c.q] = k;
  else
    atomicMax(&mkey[c.q], k);    // the slots were zeroed: 0 is below every key
}

// ---- Z_q and S_q ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void qs_sum_k(const float* __restrict__ F, const float* __restrict__ y,
                                                     const int* __restrict__ row_group, const int* __restrict__ goff,
                                                     int64_t R, int G, const unsigned* __restrict__ mkey,
                                                     unsigned long long* __restrict__ zs) {
  __shared__ Seg<ZS> sm[kThreads / 64];
  const int64_t t0 = (int64_t)blockIdx.x * kThreads, r = t0 + threadIdx.x;
  const Row c = row_of(row_group, goff, r, R, G, t0);
  ZS mine{0ull, 0ull};
  if (c.live) {
    mine.z = softmax_term(F[r], ordered_key_inv(mkey[c.q]));
    mine.s = y[r] == 1.0f ? 1ull : 0ull;
  }
  const Seg<ZS> x{mine, c.head ? 1 : 0};
  Seg<ZS> tot;
  const SegOp<ZS, AddZS> op;
  const Seg<ZS> before = block_scan_excl<kThreads, false>(x, op, Seg<ZS>{ZS{0ull, 0ull}, 0}, sm, tot);
  if (!c.live || !c.tail) return;
  const ZS v = op(before, x).v;
  unsigned long long* slot = zs + 2 * (int64_t)c.q;
  if (c.inside) {
    slot[0] = v.z;
    slot[1] = v.s;
  } else {
    atomicAdd(&slot[0], v.z);
    if (v.s != 0ull) atomicAdd(&slot[1], v.s);
  }
}

// ---- g and h ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void qs_grad_k(const float* __restrict__ F, const float* __restrict__ y,
                                                      const int* __restrict__ row_group, int64_t R, int G,
                                                      const unsigned* __restrict__ mkey,
                                                      const unsigned long long* __restrict__ zs, int* __restrict__ qg,
                                                      int* __restrict__ qh) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  const int q = row_group[r];
  float g = 0.0f, h = 0.0f;
  if ((unsigned)q < (unsigned)G) {
    const unsigned long long Z = zs[2 * (int64_t)q], S = zs[2 * (int64_t)q + 1];
    if (S != 0ull && Z != 0ull) {    // a group without a positive carries no signal
      const unsigned long long E = softmax_term(F[r], ordered_key_inv(mkey[q]));
      const float p = (float)((double)E / (double)Z);
      const float t = y[r] == 1.0f ? (float)(1.0 / (double)S) : 0.0f;
      g = t - p;
      h = p * (1.0f - p);
    }
  }
  qg[r] = (int)llrintf(g * 1073741824.0f);   // as grad_k of gbdt.hip: an exact product, half to even
  qh[r] = (int)llrintf(h * 1073741824.0f);
}

// ---- the monitoring loss ------------------------------------------------------------------------------------
// sum over the groups with a positive of L_q = -(1 / S_q) sum_{y_i = 1} [a_i - m_q - log(Z_q 2^-32)], formed row
// by row in fp64 in a fixed order: the thread's rows in row order, a fixed butterfly over the wave, the waves in
// order, and the workgroups' partials in order by qs_loss_sum_k. live counts the groups with a positive at their
// first rows.
__global__ __launch_bounds__(kThreads) void qs_loss_k(const float* __restrict__ F, const float* __restrict__ y,
                                                      const int* __restrict__ row_group, const int* __restrict__ goff,
                                                      int64_t R, int G, int64_t tiles, const unsigned* __restrict__ mkey,
                                                      const unsigned long long* __restrict__ zs, double* __restrict__ lpart,
                                                      long long* __restrict__ cpart) {
  __shared__ double sL[kThreads / 64];
  __shared__ long long sC[kThreads / 64];
  double acc = 0.0;
  long long live = 0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r = t * kThreads + threadIdx.x;
    if (r >= R) continue;
    const int q = row_group[r];
    if ((unsigned)q >= (unsigned)G) continue;
    const unsigned long long Z = zs[2 * (int64_t)q], S = zs[2 * (int64_t)q + 1];
    if (S == 0ull || Z == 0ull) continue;
    if (r == goff[q]) ++live;
    if (y[r] == 1.0f) {
      const double d = (double)F[r] - (double)ordered_key_inv(mkey[q]);
      acc -= (d - log((double)Z * (1.0 / kTwo32))) / (double)S;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    live += __shfl_xor(live, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sL[threadIdx.x >> 6] = acc;
    sC[threadIdx.x >> 6] = live;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    long long n = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      s += sL[w];
      n += sC[w];
    }
    lpart[blockIdx.x] = s;
    cpart[blockIdx.x] = n;
  }
}

// the partials in a fixed two-level order (lane l its contiguous run, lane 0 the 64 sums), as be_carry_k
__global__ __launch_bounds__(64) void qs_loss_sum_k(const double* __restrict__ lpart, const long long* __restrict__ cpart,
                                                    int n, double* __restrict__ loss_sum, long long* __restrict__ live) {
  __shared__ double sL[64];
  __shared__ long long sC[64];
  const int tid = threadIdx.x, per = (n + 63) / 64;
  const int b0 = tid * per, b1 = b0 + per < n ? b0 + per : n;
  double acc = 0.0;
  long long cnt = 0;
  for (int b = b0; b < b1; ++b) {
    acc += lpart[b];
    cnt += cpart[b];
  }
  sL[tid] = acc;
  sC[tid] = cnt;
  __syncthreads();
  if (tid != 0) return;
  acc = 0.0;
  cnt = 0;
  for (int l = 0; l < 64; ++l) {
    acc += sL[l];
    cnt += sC[l];
  }
  loss_sum[0] = acc;
  live[0] = cnt;
}

// ---- workspace and launches -----------------------------------------------------------------------------
struct QsLayout {
  int64_t zs, mkey, lpart, cpart, slots, total;   // slots: the bytes zeroed per call (zs and mkey)
};

QsLayout qs_layout(int64_t G) {
  QsLayout l;
  rsx::Bump bump{0, 256};
  l.zs = bump.take(G * 16);
  l.mkey = bump.take(G * 4);
  l.slots = bump.off;
  l.lpart = bump.take(kLossSlots * 8);
  l.cpart = bump.take(kLossSlots * 8);
  l.total = bump.off;
  return l;
}

bool rows_ok(int64_t R, int64_t G) { return R >= 1 && R < (1ll << 31) && G >= 1 && G <= R; }

unsigned tiles_of(int64_t R) { return (unsigned)((R + kThreads - 1) / kThreads); }

// m_q, Z_q and S_q of every group into the workspace's slots
void launch_group_sums(const float* F, const float* y, const int* row_group, const int* goff, int64_t R, int G, void* ws,
                       const QsLayout& l, hipStream_t st) {
  (void)hipMemsetAsync(ws, 0, (size_t)l.slots, st);
  hipLaunchKernelGGL(qs_max_k, dim3(tiles_of(R)), dim3(kThreads), 0, st, F, row_group, goff, R, G, at<unsigned>(ws, l.mkey));
  hipLaunchKernelGGL(qs_sum_k, dim3(tiles_of(R)), dim3(kThreads), 0, st, F, y, row_group, goff, R, G,
                     at<unsigned>(ws, l.mkey), at<unsigned long long>(ws, l.zs));
}

}  // namespace

namespace rsx {

int64_t gbdt_query_softmax_workspace(int64_t R, int64_t G) { return rows_ok(R, G) ? qs_layout(G).total : -1; }

void gbdt_query_softmax_launch(const float* F, const float* y, const int* row_group, const int* goff, int64_t R, int G,
                               void* ws, int* qg, int* qh, hipStream_t st) {
  const QsLayout l = qs_layout(G);
  launch_group_sums(F, y, row_group, goff, R, G, ws, l, st);
  hipLaunchKernelGGL(qs_grad_k, dim3(tiles_of(R)), dim3(kThreads), 0, st, F, y, row_group, R, G, at<unsigned>(ws, l.mkey),
                     at<unsigned long long>(ws, l.zs), qg, qh);
}

}  // namespace rsx

RSX_API int64_t rsx_gbdt_grad_query_softmax_workspace_bytes(int64_t R, int64_t G) {
  const int64_t n = rsx::gbdt_query_softmax_workspace(R, G);
  if (n < 0) rsx::set_error("%s: invalid argument: %s", __func__, "need 1 <= R < 2^31 and 1 <= G <= R");
  return n;
}

RSX_API int rsx_gbdt_grad_query_softmax(const float* F, const float* y, const int* row_group, const int* goff, int64_t R,
                                        int64_t G, void* ws, int64_t ws_bytes, int* qg, int* qh, void* stream) {
  RSX_ARG(F && y && row_group && goff && ws && qg && qh, "null tensor");
  RSX_ARG(rows_ok(R, G), "need 1 <= R < 2^31 and 1 <= G <= R");
  RSX_ARG(ws_bytes >= qs_layout(G).total, "workspace too small (rsx_gbdt_grad_query_softmax_workspace_bytes)");
  RSX_ARG(rsx::aligned16(ws), "ws must be 16-byte aligned");
  rsx::gbdt_query_softmax_launch(F, y, row_group, goff, R, (int)G, ws, qg, qh, (hipStream_t)stream);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_query_softmax_eval(const float* F, const float* y, const int* row_group, const int* goff, int64_t R, int64_t G,
                                   void* ws, int64_t ws_bytes, void* out, void* stream) {
  RSX_ARG(F && y && row_group && goff && ws && out, "null tensor");
  RSX_ARG(rows_ok(R, G), "need 1 <= R < 2^31 and 1 <= G <= R");
  const QsLayout l = qs_layout(G);
  RSX_ARG(ws_bytes >= l.total, "workspace too small (rsx_gbdt_grad_query_softmax_workspace_bytes)");
  RSX_ARG(rsx::aligned16(ws) && ((uintptr_t)out & 7) == 0, "misaligned pointer (workspace 16 bytes, out 8)");
  hipStream_t st = (hipStream_t)stream;
  launch_group_sums(F, y, row_group, goff, R, (int)G, ws, l, st);
  const int64_t tiles = tiles_of(R);
  const unsigned grid = (unsigned)(tiles < kLossSlots ? tiles : kLossSlots);
  hipLaunchKernelGGL(qs_loss_k, dim3(grid), dim3(kThreads), 0, st, F, y, row_group, goff, R, (int)G, tiles,
                     at<unsigned>(ws, l.mkey), at<unsigned long long>(ws, l.zs), at<double>(ws, l.lpart),
                     at<long long>(ws, l.cpart));
  hipLaunchKernelGGL(qs_loss_sum_k, dim3(1), dim3(64), 0, st, at<double>(ws, l.lpart), at<long long>(ws, l.cpart), (int)grid,
                     reinterpret_cast<double*>(out), reinterpret_cast<long long*>(out) + 1);
  RSX_LAUNCHED();
  return 0;
}
