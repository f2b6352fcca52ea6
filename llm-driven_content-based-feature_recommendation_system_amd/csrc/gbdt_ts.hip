// Ordered target statistics of wide categorical columns: what turns a column of up to 2^22 codes into one
// numeric column of the oblivious-tree model. Specified in include/recsys_amd.h ("ordered target statistics")
// and restated in integer / float64 numpy by tests/gbdt_ts_ref.py.
//
// Column k has the codes c_i in [0, V_k]. rsx_gbdt_ts_keys writes the sort keys c_i << 32 | hash_u32(seed + k,
// i); a stable sort of them (the caller's, plumbing) is `order`: the rows by code, inside a code by (hash, row).
// Along that order a row's statistic is the exclusive scan of (1, y) over its run of equal codes:
//   ts_tile_k<false>  per 256-row tile the segmented workgroup scan (rsx_block.h) -> the tile's aggregate: the
//                     sums of its trailing piece and "a run starts in this tile"
//   ts_carry_k        one workgroup per column scans the tile aggregates in chunks of 256 -> per tile the carry
//                     into its leading piece
//   ts_tile_k<true>   the in-tile scan again, plus the carry where no run started before the row in its tile;
//                     ts scattered to order[i]; the last row of a run writes N_c, S_c and table[c]
// One row per thread, no thread walks a run, no workgroup waits on another (three launches in stream order),
// every slot has one writer and every sum is an integer: the same bits every run. The only atomic is the OR
// into flag.
#include "rsx_block.h"
#include "rsx_common.h"

#include <limits.h>

namespace {

using rsx::block_scan_excl, rsx::hash_u32, rsx::Seg, rsx::SegOp;

constexpr int kThreads = 256;              // rows per tile: one row per thread
constexpr int kMaxColumns = 32;            // GBDT_MAX_FEATURES
constexpr int64_t kMaxCodes = 1ll << 22;   // GBDT_TS_MAX_CODES
constexpr int kNone = INT_MIN;             // the code of a position outside [0, R) or of a bad order entry

struct NS {
  int n, s;      // rows and positives: both < 2^31
};
struct AddNS {
  __device__ __forceinline__ NS operator()(NS a, NS b) const { return NS{a.n + b.n, a.s + b.s}; }
};
using SegNS = Seg<NS>;

__device__ __forceinline__ float ts_value(int s, int n, double ap, double a) {
  return (float)(((double)s + ap) / ((double)n + a));
}

__global__ __launch_bounds__(kThreads) void ts_keys_k(const int* __restrict__ codes, int64_t R, uint64_t seed,
                                                      int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R) return;
  const int k = blockIdx.y;
  const int64_t c = codes[k * R + i];
  keys[k * R + i] = (int64_t)(((uint64_t)c << 32) | (uint64_t)hash_u32(seed + (uint64_t)k, (uint64_t)i));
}

__global__ __launch_bounds__(kThreads) void ts_fill_k(float* __restrict__ table, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) table[i] = v;
}

// the code at sorted position s of column k, kNone outside [0, R) or behind an order entry outside [0, R)
__device__ __forceinline__ int code_at(const int* __restrict__ codes, const int64_t* __restrict__ order, int64_t R,
                                       int k, int64_t s) {
  if (s < 0 || s >= R) return kNone;
  const int64_t r = order[k * R + s];
  return (uint64_t)r < (uint64_t)R ? codes[k * R + r] : kNone;
}

// APPLY false: tiles[k, tile] = (n, s, head, 0) of the tile. APPLY true: tiles holds the carries (ts_carry_k).
template <bool APPLY>
__global__ __launch_bounds__(kThreads) void ts_tile_k(const int* __restrict__ codes, const int64_t* __restrict__ order,
                                                      const float* __restrict__ y, const int* __restrict__ V, int64_t Vmax,
                                                      int64_t R, int64_t n_tiles, double ap, double a, int4* tiles,
                                                      float* __restrict__ ts, int* __restrict__ totals,
                                                      float* __restrict__ table, int* __restrict__ flag) {
  __shared__ int sc[kThreads + 2];      // the codes at the sorted positions t0 - 1 .. t0 + 256
  __shared__ SegNS sm[kThreads / 64];
  const int tid = threadIdx.x, k = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * kThreads, s = t0 + tid;
  int Vk = V[k];
  Vk = Vk < 0 ? 0 : ((int64_t)Vk > Vmax ? (int)Vmax : Vk);

  int c = kNone, yi = 0;
  int64_t row = -1;
  bool live = false;
  if (s < R) {
    const int64_t r = order[k * R + s];
    if ((uint64_t)r < (uint64_t)R) {
      row = r;
      c = codes[k * R + r];
      live = (unsigned)c <= (unsigned)Vk;
      if (live) yi = y[r] == 1.0f ? 1 : 0;
    }
    if (!live && !APPLY) atomicOr(flag, 1);
  }
  sc[tid + 1] = c;
  if (tid < 2) sc[tid == 0 ? 0 : kThreads + 1] = code_at(codes, order, R, k, tid == 0 ? t0 - 1 : t0 + kThreads);
  __syncthreads();
  const bool head = s >= R || s == 0 || sc[tid] != c;
  const bool tail = live && (s == R - 1 || sc[tid + 2] != c);

  const SegNS x{NS{live ? 1 : 0, yi}, head ? 1 : 0};
  SegNS tot;
  const SegNS before = block_scan_excl<kThreads, false>(x, SegOp<NS, AddNS>(), SegNS{NS{0, 0}, 0}, sm, tot);
  const int64_t slot = (int64_t)k * n_tiles + blockIdx.x;
  if (!APPLY) {
    if (tid == 0) tiles[slot] = make_int4(tot.v.n, tot.v.s, tot.head, 0);
    return;
  }
  if (row < 0) return;
  NS pre{0, 0};
  if (!head) {
    pre = before.v;
    if (!before.head) {      // the run began in an earlier tile
      const int4 carry = tiles[slot];
      pre.n += carry.x;
      pre.s += carry.y;
    }
  }
  ts[k * R + row] = live ? ts_value(pre.s, pre.n, ap, a) : ts_value(0, 0, ap, a);
  if (tail) {
    const int64_t e = (int64_t)k * (Vmax + 1) + c;
    const int n = pre.n + 1, sy = pre.s + yi;
    totals[2 * e] = n;
    totals[2 * e + 1] = sy;
    table[e] = ts_value(sy, n, ap, a);
  }
}

// tiles[k, t] = (n, s, head, 0) -> the carry into tile t: the sums over the trailing pieces of the tiles since the
// last one in which a run started (that one included). One workgroup per column, the tiles in chunks of 256.
__global__ __launch_bounds__(kThreads) void ts_carry_k(int4* tiles, int64_t n_tiles) {
  __shared__ SegNS sm[kThreads / 64];
  int4* mine = tiles + (int64_t)blockIdx.y * n_tiles;
  const SegOp<NS, AddNS> op;
  const SegNS ident{NS{0, 0}, 0};
  SegNS run = ident;
  for (int64_t b = 0; b < n_tiles; b += kThreads) {
    const int64_t t = b + threadIdx.x;
    SegNS x = ident;
    if (t < n_tiles) {
      const int4 v = mine[t];
      x = SegNS{NS{v.x, v.y}, v.z};
    }
    SegNS tot;
    const SegNS before = block_scan_excl<kThreads, false>(x, op, ident, sm, tot);
    if (t < n_tiles) {
      const SegNS res = op(run, before);
      mine[t] = make_int4(res.v.n, res.v.s, 0, 0);
    }
    run = op(run, tot);
  }
}

bool shape_ok(int64_t R, int64_t Fts) { return R >= 1 && R < (1ll << 31) && Fts >= 1 && Fts <= kMaxColumns; }

int64_t tiles_of(int64_t R) { return (R + kThreads - 1) / kThreads; }

}  // namespace

RSX_API int rsx_gbdt_ts_keys(const int* codes, int64_t R, int Fts, uint64_t seed, int64_t* keys, void* stream) {
  RSX_ARG(codes && keys, "null tensor");
  RSX_ARG(shape_ok(R, Fts), "need 1 <= R < 2^31 and 1 <= Fts <= 32");
  hipLaunchKernelGGL(ts_keys_k, dim3((unsigned)tiles_of(R), (unsigned)Fts), dim3(kThreads), 0, (hipStream_t)stream, codes, R,
                     seed, keys);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_gbdt_ordered_ts(const int* codes, const int64_t* order, const float* y, const int* V, int64_t R, int Fts,
                                int64_t Vmax, double ap, double a, void* ws, int64_t ws_bytes, float* ts, int* totals,
                                float* table, int* flag, void* stream) {
  RSX_ARG(codes && order && y && V && ws && ts && totals && table && flag, "null tensor");
  RSX_ARG(shape_ok(R, Fts), "need 1 <= R < 2^31 and 1 <= Fts <= 32");
  RSX_ARG(Vmax >= 0 && Vmax <= kMaxCodes, "need 0 <= Vmax <= 2^22 known values (GBDT_TS_MAX_CODES)");
  RSX_ARG(a > 0.0 && a <= 1e300 && ap >= 0.0 && ap <= 1e300, "the prior needs a weight a > 0 and a p >= 0");
  const int64_t n_tiles = tiles_of(R);
  RSX_ARG(ws_bytes >= 16 * Fts * n_tiles, "workspace too small (16 Fts ceil(R / 256) bytes)");
  RSX_ARG(rsx::aligned16(ws), "ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = (int64_t)Fts * (Vmax + 1);
  const dim3 grid((unsigned)n_tiles, (unsigned)Fts);
  int4* tiles = reinterpret_cast<int4*>(ws);
  (void)hipMemsetAsync(totals, 0, (size_t)cells * 8, st);
  const float prior = (float)((0.0 + ap) / (0.0 + a));      // ts_value(0, 0): a code nobody had, a row behind a bad entry
  hipLaunchKernelGGL(ts_fill_k, dim3((unsigned)tiles_of(cells)), dim3(kThreads), 0, st, table, cells, prior);
  hipLaunchKernelGGL(ts_fill_k, dim3((unsigned)tiles_of(Fts * R)), dim3(kThreads), 0, st, ts, Fts * R, prior);
  hipLaunchKernelGGL(ts_tile_k<false>, grid, dim3(kThreads), 0, st, codes, order, y, V, Vmax, R, n_tiles, ap, a, tiles, ts,
                     totals, table, flag);
  hipLaunchKernelGGL(ts_carry_k, dim3(1, (unsigned)Fts), dim3(kThreads), 0, st, tiles, n_tiles);
  hipLaunchKernelGGL(ts_tile_k<true>, grid, dim3(kThreads), 0, st, codes, order, y, V, Vmax, R, n_tiles, ap, a, tiles, ts,
                     totals, table, flag);
  RSX_LAUNCHED();
  return 0;
}
