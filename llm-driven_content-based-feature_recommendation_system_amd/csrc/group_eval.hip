// Grouped (per-query) evaluation of a binary ranker on the device: for R scored rows with a group id
// each, every group's P, N, U2 (twice the tie-aware Mann-Whitney U within the group) and tie-averaged
// DCG@top, and the two summary sums behind QueryAUC and NDCG, for one host read.
// Reference: the ranker's training rows are grouped per customer (utils/monitor/log_importer.py,
// HMLogImporter.load_and_preprocess -> X_user, X_item, y, groups); the per-query metrics a CatBoost
// user evaluates on them are NDCG and QueryAUC. binary_eval.hip is the pooled form of the same idea.
//
// The rows are sorted by (group ascending, score descending). In that order, with cx / cn the
// exclusive / inclusive count of negatives, a tie group [s, e] of the group that starts at row gs holds
//   pos = (e - s + 1) - (cn[e] - cx[s]) positives, and contributes
//   V   += pos * ((cx[s] - cx[gs]) + (cn[e] - cx[gs]))      negatives scored above + at or above
//   DCG += pos * (D[min(e + 1 - gs, top)] - D[min(s - gs, top)]) / (e - s + 1)
// and the group that ends at row ge has N = cn[ge] - cx[gs], P = (ge - gs + 1) - N and
// U2 = 2 P N - V (#{z_j < z_i} + #{z_j <= z_i} = 2 N - #{z_j > z_i} - #{z_j >= z_i}). Every term is
// formed at a tie group's last row from values that only look backwards (the latest group head and
// the latest tie head, each with its cx: two forward max-scans of (row << 32 | cx), monotone in the
// row), so no step walks a tie group or a group.
//
//   ge_key_k    (group, z) -> 64-bit key group << 32 | ~score key, y -> a uint8 label, the flags
//   rocprim::radix_sort_pairs over the key bits in use
//   ge_tile_k<false>  per 2048-row tile: its negatives and group heads, its last group / tie head
//   ge_carry_k  one workgroup over the tiles: exclusive sums (negatives, group heads = the groups'
//               ordinals; their total is G) and the exclusive max-scans of the two heads
//   ge_tile_k<true>   the terms at the tie tails, a tile-local segmented (by group) scan of (V, DCG);
//               a group that starts and ends in the tile is written to out[ordinal] here; a group that
//               started earlier leaves (ordinal, its partial sums) in the tile's record; the tile's
//               trailing open sums are its aggregate
//   ge_fix_k    one workgroup: segmented exclusive scan of the tiles' aggregates = what each tile's
//               first group had gathered before the tile; finishes the recorded groups
//   ge_group_k  NDCG_g and AUC_g of the G groups, block b its contiguous slice, a fixed-order sum
//   ge_sum_k    the blocks' partial sums in block order -> the summary
// The double sums have a fixed order (the trees of rsx_block.h's block_scan_excl depend on the sizes
// only) and the integer sums are exact: the outputs are the same bits every run. No float atomics.
#include "rsx_block.h"
#include "rsx_common.h"
#include "rsx_x3.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <string.h>

namespace {

using rsx::at, rsx::block_scan_excl, rsx::score_key;

constexpr int kThreads = 256, kPer = 8, kTile = kThreads * kPer;
constexpr int kGroupBlocks = 256;  // most workgroups of ge_group_k (each one partial of the summary)
constexpr int kMaxTop = 65536;
typedef unsigned long long u64;
typedef long long i64;

// The library's radix sort; the size up to which it merge-sorts instead of running the onesweep radix
// passes stays at its default of 2^20 rows: with these 9-byte pairs and up to 63 key bits (eight
// passes) the merge sort holds on longer than with binary_eval's 5-byte pairs. Measured on an MI355X
// (whole evaluation with its host read, groups of 100, merge sort / onesweep): 65,536 rows
// 0.178 / 0.316 ms, 262,144 rows 0.263 / 0.365 ms, 524,288 rows 0.315 / 0.379 ms, 1,048,576 rows
// 0.361 / 0.401 ms; with max_group_id given (46 key bits at 1,048,576 rows) 0.358 / 0.344 ms there
// (profiles/group_eval_sort_ab.json).
#ifndef RSX_GE_MERGE_LIMIT
#define RSX_GE_MERGE_LIMIT (1024 * 1024)
#endif
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                              rocprim::default_config, RSX_GE_MERGE_LIMIT>;

hipError_t sort_pairs(void* tmp, size_t& bytes, const u64* kin, u64* kout, const uint8_t* vin, uint8_t* vout, int64_t R,
                      unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs<SortConfig>(tmp, bytes, kin, kout, vin, vout, (size_t)R, 0u, end_bit, st);
}

struct Cnt {  // negatives, group heads
  int neg, heads;
};
struct CntSum {
  __device__ __forceinline__ Cnt operator()(Cnt a, Cnt b) const { return Cnt{a.neg + b.neg, a.heads + b.heads}; }
};
struct Heads {  // row << 32 | cx of the latest group head / tie head; -1 = none
  i64 g, t;
};
struct HeadsMax {
  __device__ __forceinline__ Heads operator()(Heads a, Heads b) const {
    return Heads{a.g > b.g ? a.g : b.g, a.t > b.t ? a.t : b.t};
  }
};
struct Seg {  // the sums of the open group; head: a group head lies in the range
  int head, pad;
  u64 v;
  double d;
};
struct SegOp {
  __device__ __forceinline__ Seg operator()(Seg a, Seg b) const {
    if (b.head) return b;
    return Seg{a.head, 0, a.v + b.v, a.d + b.d};
  }
};

__device__ __forceinline__ i64 pack(int64_t row, int cx) { return (i64)((u64)row << 32 | (unsigned)cx); }
__device__ __forceinline__ int64_t pack_row(i64 p) { return (int64_t)(p >> 32); }
__device__ __forceinline__ int pack_cx(i64 p) { return (int)(unsigned)(p & 0xffffffffll); }

__global__ __launch_bounds__(kThreads) void ge_key_k(const float* __restrict__ logit, const float* __restrict__ y,
                                                      const int* __restrict__ gid, int64_t R, int64_t max_gid,
                                                      u64* __restrict__ keys, uint8_t* __restrict__ lab,
                                                      int* __restrict__ flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < R; i += (int64_t)gridDim.x * kThreads) {
    const float z = logit[i], yy = y[i];
    const int g = gid[i];
    if (!(fabsf(z) <= 3.402823466e38f)) bad |= 1;  // NaN or +-inf
    if (!(yy == 0.0f || yy == 1.0f)) bad |= 2;
    if (g < 0 || (int64_t)g > max_gid) bad |= 4;
    keys[i] = (u64)((unsigned)g & 0x7fffffffu) << 32 | (u64)(~score_key(z));  // descending score
    lab[i] = yy == 1.0f ? 1 : 0;
  }
  if (bad) atomicOr(flag, bad);  // only on input that is rejected anyway
}

struct TileArrays {
  int *neg, *heads;            // per tile: negatives, group heads
  i64 *ghead, *thead;          // its last group head / tie head (row << 32 | tile-local cx), -1 = none
  int *negoff, *headoff;       // ge_carry_k: exclusive sums
  i64 *carry_g, *carry_t;      // ge_carry_k: the latest heads before the tile, cx global
  int* agg_head;               // ge_tile_k<true>: the tile's aggregate (Seg) ...
  u64* agg_v;
  double* agg_d;
  int* rec_ord;                // ... and its record: the group that started before the tile and ends in it
  u64* rec_v;
  double* rec_d;
};

struct GroupOut {
  int* gid;
  i64 *P, *N, *U2;
  double* dcg;
};

// One 2048-row tile of the sorted rows, 8 consecutive rows per thread.
template <bool APPLY>
__global__ __launch_bounds__(kThreads) void ge_tile_k(const u64* __restrict__ skeys, const uint8_t* __restrict__ slab,
                                                       int64_t R, int top, const double* __restrict__ D, TileArrays ta,
                                                       GroupOut out) {
  __shared__ Cnt smC[kThreads / 64];
  __shared__ Heads smH[kThreads / 64];
  __shared__ Seg smS[kThreads / 64];
  __shared__ int sRecOrd;
  __shared__ u64 sRecV;
  __shared__ double sRecD;
  const int64_t tile = blockIdx.x;
  const int64_t i0 = tile * kTile + (int64_t)threadIdx.x * kPer;
  u64 k[kPer];
  unsigned l[kPer];
  if (i0 + kPer <= R) {  // the workspace arrays are 256-byte aligned and i0 is a multiple of 8
#pragma unroll
    for (int q = 0; q < kPer / 2; ++q) {
      const ulonglong2 a = reinterpret_cast<const ulonglong2*>(skeys + i0)[q];
      k[2 * q] = a.x, k[2 * q + 1] = a.y;
    }
    const uint2 p = *reinterpret_cast<const uint2*>(slab + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l[j] = (p.x >> (8 * j)) & 0xffu;
      l[4 + j] = (p.y >> (8 * j)) & 0xffu;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const bool in = i0 + j < R;
      k[j] = in ? skeys[i0 + j] : 0ull;
      l[j] = in ? slab[i0 + j] : 0u;
    }
  }
  // the neighbours across the thread's (and the tile's) edges come from memory
  const u64 kprev = (i0 > 0 && i0 - 1 < R) ? skeys[i0 - 1] : 0ull;
  const u64 knext = (i0 + kPer < R) ? skeys[i0 + kPer] : 0ull;
  bool in[kPer], ghead[kPer], thead[kPer], ttail[kPer], gtail[kPer];
  int neg[kPer];
  Cnt cthr{0, 0};
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = i0 + j;
    in[j] = i < R;
    const u64 kp = j == 0 ? kprev : k[j - 1], kn = j == kPer - 1 ? knext : k[j + 1];
    thead[j] = in[j] && (i == 0 || kp != k[j]);
    ghead[j] = in[j] && (i == 0 || (kp >> 32) != (k[j] >> 32));
    ttail[j] = in[j] && (i == R - 1 || kn != k[j]);
    gtail[j] = in[j] && (i == R - 1 || (kn >> 32) != (k[j] >> 32));
    neg[j] = (in[j] && l[j] == 0u) ? 1 : 0;
    cthr.neg += neg[j];
    cthr.heads += ghead[j] ? 1 : 0;
  }
  Cnt ctile;
  const Cnt cbase = block_scan_excl<kThreads>(cthr, CntSum(), Cnt{0, 0}, smC, ctile);
  const int off = APPLY ? ta.negoff[tile] : 0;  // the first pass keeps cx tile-local
  int cx[kPer];
  Heads hthr{-1, -1};
  {
    int c = cbase.neg;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      cx[j] = off + c;
      c += neg[j];
      if (ghead[j]) hthr.g = pack(i0 + j, cx[j]);
      if (thead[j]) hthr.t = pack(i0 + j, cx[j]);
    }
  }
  Heads htile;
  const Heads hbase = block_scan_excl<kThreads>(hthr, HeadsMax(), Heads{-1, -1}, smH, htile);
  if (!APPLY) {
    if (threadIdx.x == 0) {
      ta.neg[tile] = ctile.neg;
      ta.heads[tile] = ctile.heads;
      ta.ghead[tile] = htile.g;
      ta.thead[tile] = htile.t;
    }
    return;
  }
  if (threadIdx.x == 0) sRecOrd = -1;
  // the terms at the tie tails. Row 0 is a group head and a tie head, so a head is always found.
  const Heads hcarry = HeadsMax()(Heads{ta.carry_g[tile], ta.carry_t[tile]}, hbase);
  u64 v[kPer];
  double d[kPer];
  i64 gh[kPer];
  Seg sthr{0, 0, 0ull, 0.0};
  {
    Heads run = hcarry;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (ghead[j]) run.g = pack(i0 + j, cx[j]);
      if (thead[j]) run.t = pack(i0 + j, cx[j]);
      gh[j] = run.g;
      v[j] = 0ull;
      d[j] = 0.0;
      if (ttail[j]) {
        const int64_t i = i0 + j, s = pack_row(run.t), gs = pack_row(run.g);
        const int cs = pack_cx(run.t), cg = pack_cx(run.g), ce = cx[j] + neg[j];
        const int64_t len = i - s + 1, pos = len - (int64_t)(ce - cs);
        if (pos > 0) {
          v[j] = (u64)pos * (u64)((int64_t)(cs - cg) + (int64_t)(ce - cg));
          const int64_t pa = s - gs, pb = i + 1 - gs;
          const double da = D[pa < top ? pa : top], db = D[pb < top ? pb : top];
          d[j] = (double)pos * (db - da) / (double)len;
        }
      }
      if (ghead[j]) sthr = Seg{1, 0, 0ull, 0.0};
      sthr.v += v[j];
      sthr.d += d[j];
    }
  }
  Seg stile;
  const Seg sbase = block_scan_excl<kThreads>(sthr, SegOp(), Seg{0, 0, 0ull, 0.0}, smS, stile);  // syncs: sRecOrd is set
  {
    Seg run = sbase;
    int hc = ta.headoff[tile] + cbase.heads;  // group heads before the row
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (ghead[j]) {
        run = Seg{1, 0, 0ull, 0.0};
        ++hc;
      }
      run.v += v[j];
      run.d += d[j];
      if (gtail[j]) {
        const int64_t i = i0 + j, ord = hc - 1;  // 0 <= ord < G <= R
        const int64_t n = (cx[j] + neg[j]) - pack_cx(gh[j]), p = (i - pack_row(gh[j]) + 1) - n;
        out.gid[ord] = (int)(k[j] >> 32);
        out.P[ord] = p;
        out.N[ord] = n;
        if (run.head) {
          out.U2[ord] = (i64)(2ull * (u64)p * (u64)n - run.v);
          out.dcg[ord] = run.d;
        } else {  // the group began before this tile: at most one such row per tile
          sRecOrd = (int)ord;
          sRecV = run.v;
          sRecD = run.d;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ta.agg_head[tile] = stile.head;
    ta.agg_v[tile] = stile.v;
    ta.agg_d[tile] = stile.d;
    ta.rec_ord[tile] = sRecOrd;
    ta.rec_v[tile] = sRecOrd >= 0 ? sRecV : 0ull;
    ta.rec_d[tile] = sRecOrd >= 0 ? sRecD : 0.0;
  }
}

// One workgroup over the tiles: negoff / headoff = exclusive sums of the tiles' negatives / group
// heads (the heads' total is G); carry_g / carry_t = the latest group / tie head before the tile with
// its cx made global (a forward max-scan: row << 32 | cx grows with the row).
__global__ __launch_bounds__(1024) void ge_carry_k(TileArrays ta, int64_t tiles, i64* __restrict__ summary) {
  __shared__ Cnt smC[16];
  __shared__ Heads smH[16];
  const int tid = threadIdx.x;
  Cnt ccarry{0, 0};
  Heads hcarry{-1, -1};
  for (int64_t b = 0; b < tiles; b += 1024) {
    const int64_t t = b + tid;
    const Cnt c = t < tiles ? Cnt{ta.neg[t], ta.heads[t]} : Cnt{0, 0};
    Cnt ctot;
    const Cnt ce = CntSum()(ccarry, block_scan_excl<1024>(c, CntSum(), Cnt{0, 0}, smC, ctot));
    Heads h{-1, -1};
    if (t < tiles) {
      ta.negoff[t] = ce.neg;
      ta.headoff[t] = ce.heads;
      const i64 g = ta.ghead[t], th = ta.thead[t];
      h.g = g < 0 ? -1 : g + ce.neg;  // cx stays below 2^31: no carry into the row
      h.t = th < 0 ? -1 : th + ce.neg;
    }
    Heads htot;
    const Heads he = HeadsMax()(hcarry, block_scan_excl<1024>(h, HeadsMax(), Heads{-1, -1}, smH, htot));
    if (t < tiles) {
      ta.carry_g[t] = he.g;
      ta.carry_t[t] = he.t;
    }
    ccarry = CntSum()(ccarry, ctot);
    hcarry = HeadsMax()(hcarry, htot);
  }
  if (tid == 0) summary[0] = ccarry.heads;  // G
}

// One workgroup over the tiles: what the tile's first group gathered in the tiles before it (a
// segmented exclusive scan of the aggregates), added to the tile's record.
__global__ __launch_bounds__(1024) void ge_fix_k(TileArrays ta, int64_t tiles, GroupOut out) {
  __shared__ Seg smS[16];
  const int tid = threadIdx.x;
  const Seg ident{0, 0, 0ull, 0.0};
  Seg carry = ident;
  for (int64_t b = 0; b < tiles; b += 1024) {
    const int64_t t = b + tid;
    const Seg x = t < tiles ? Seg{ta.agg_head[t], 0, ta.agg_v[t], ta.agg_d[t]} : ident;
    Seg tot;
    const Seg cin = SegOp()(carry, block_scan_excl<1024>(x, SegOp(), ident, smS, tot));
    if (t < tiles) {
      const int ord = ta.rec_ord[t];
      if (ord >= 0) {
        const u64 p = (u64)out.P[ord], n = (u64)out.N[ord];
        out.U2[ord] = (i64)(2ull * p * n - (cin.v + ta.rec_v[t]));
        out.dcg[ord] = cin.d + ta.rec_d[t];
      }
    }
    carry = SegOp()(carry, tot);
  }
}

// NDCG_g = DCG_g / D[min(P_g, top)] over the groups with a positive, AUC_g = U2_g / (2 P_g N_g) over
// those with both classes: block b sums the groups [b chunk, (b + 1) chunk) in a fixed order.
__global__ __launch_bounds__(kThreads) void ge_group_k(GroupOut out, const i64* __restrict__ summary, int top,
                                                        const double* __restrict__ D, double* __restrict__ part) {
  __shared__ double sA[kThreads / 64], sB[kThreads / 64];
  __shared__ i64 sC[kThreads / 64], sE[kThreads / 64];
  const int64_t G = summary[0];
  const int64_t chunk = (G + gridDim.x - 1) / gridDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * chunk, g1 = g0 + chunk < G ? g0 + chunk : G;
  double a = 0.0, b = 0.0;
  i64 na = 0, nb = 0;
  for (int64_t g = g0 + threadIdx.x; g < g1; g += kThreads) {
    const i64 p = out.P[g], n = out.N[g];
    if (p > 0) {
      a += out.dcg[g] / D[p < top ? p : top];
      ++na;
      if (n > 0) {
        b += (double)out.U2[g] / (double)(2ull * (u64)p * (u64)n);
        ++nb;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    na += __shfl_xor(na, o, 64);
    nb += __shfl_xor(nb, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sA[w] = a, sB[w] = b, sC[w] = na, sE[w] = nb;
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0.0, tb = 0.0;
    i64 ca = 0, cb = 0;
    for (int q = 0; q < kThreads / 64; ++q) ta += sA[q], tb += sB[q], ca += sC[q], cb += sE[q];
    part[4 * blockIdx.x] = ta;
    part[4 * blockIdx.x + 1] = tb;
    reinterpret_cast<i64*>(part)[4 * blockIdx.x + 2] = ca;
    reinterpret_cast<i64*>(part)[4 * blockIdx.x + 3] = cb;
  }
}

__global__ void ge_sum_k(const double* __restrict__ part, int nblocks, i64* __restrict__ summary) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, b = 0.0;
  i64 na = 0, nb = 0;
  for (int q = 0; q < nblocks; ++q) {
    a += part[4 * q];
    b += part[4 * q + 1];
    na += reinterpret_cast<const i64*>(part)[4 * q + 2];
    nb += reinterpret_cast<const i64*>(part)[4 * q + 3];
  }
  summary[1] = na;
  summary[2] = nb;
  reinterpret_cast<double*>(summary)[3] = a;
  reinterpret_cast<double*>(summary)[4] = b;
}

struct GeLayout {
  int64_t keys, keys_o, lab, lab_o, neg, heads, ghead, thead, negoff, headoff, carry_g, carry_t, agg_head, agg_v, agg_d,
      rec_ord, rec_v, rec_d, part, temp, temp_bytes, total, tiles;
};

size_t sort_temp_bytes(int64_t R) {
  size_t s = 0;
  (void)sort_pairs(nullptr, s, nullptr, nullptr, nullptr, nullptr, R, 63u, nullptr);
  return s;
}

GeLayout ge_layout(int64_t R) {
  GeLayout l;
  rsx::Bump bump{0, 256};
  l.tiles = (R + kTile - 1) / kTile;
  l.keys = bump.take(R * 8);
  l.keys_o = bump.take(R * 8);
  l.lab = bump.take(R);
  l.lab_o = bump.take(R);
  l.neg = bump.take(l.tiles * 4);
  l.heads = bump.take(l.tiles * 4);
  l.ghead = bump.take(l.tiles * 8);
  l.thead = bump.take(l.tiles * 8);
  l.negoff = bump.take(l.tiles * 4);
  l.headoff = bump.take(l.tiles * 4);
  l.carry_g = bump.take(l.tiles * 8);
  l.carry_t = bump.take(l.tiles * 8);
  l.agg_head = bump.take(l.tiles * 4);
  l.agg_v = bump.take(l.tiles * 8);
  l.agg_d = bump.take(l.tiles * 8);
  l.rec_ord = bump.take(l.tiles * 4);
  l.rec_v = bump.take(l.tiles * 8);
  l.rec_d = bump.take(l.tiles * 8);
  l.part = bump.take(kGroupBlocks * 4 * 8);
  // as binary_eval.hip: the sort's plan depends on the size, so take its largest request over R and
  // the powers of two below it (the total must not shrink where the plan changes)
  size_t tb = sort_temp_bytes(R);
  for (int64_t p = 1; p < R; p <<= 1) tb = std::max(tb, sort_temp_bytes(p));
  l.temp_bytes = (int64_t)tb;
  l.temp = bump.take(l.temp_bytes);
  l.total = bump.off;
  return l;
}

}  // namespace

RSX_API int64_t rsx_group_eval_workspace_bytes(int64_t R) {
  if (R < 1 || R >= ((int64_t)1 << 31)) {
    rsx::set_error("%s: invalid argument: %s", __func__, "need 1 <= R < 2^31");
    return -1;
  }
  return ge_layout(R).total;
}

RSX_API int rsx_group_eval(const float* logit, const float* y, const int32_t* group_id, int64_t R, int top,
                           const double* D, int64_t max_group_id, void* ws, int64_t ws_bytes, int64_t* summary,
                           int32_t* gid, int64_t* P, int64_t* N, int64_t* U2, double* dcg, int* flag, void* stream) {
  RSX_ARG(R >= 1 && R < ((int64_t)1 << 31), "need 1 <= R < 2^31");
  RSX_ARG(top >= 1 && top <= kMaxTop, "need 1 <= top <= 65536");
  RSX_ARG(max_group_id >= -1 && max_group_id < ((int64_t)1 << 31), "need -1 <= max_group_id < 2^31");
  RSX_ARG(logit && y && group_id && D && ws && summary && gid && P && N && U2 && dcg && flag, "null tensor");
  const GeLayout l = ge_layout(R);
  RSX_ARG(ws_bytes >= l.total, "workspace too small (rsx_group_eval_workspace_bytes)");
  RSX_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)logit & 3) == 0 && ((uintptr_t)y & 3) == 0 &&
              ((uintptr_t)group_id & 3) == 0 && ((uintptr_t)gid & 3) == 0 && ((uintptr_t)flag & 3) == 0 &&
              (((uintptr_t)D | (uintptr_t)summary | (uintptr_t)P | (uintptr_t)N | (uintptr_t)U2 | (uintptr_t)dcg) & 7) == 0,
          "misaligned pointer (workspace 16 bytes, 8-byte arrays 8, 4-byte arrays 4)");
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(flag, 0, sizeof(int), st);
  const int64_t gmax = max_group_id < 0 ? (((int64_t)1 << 31) - 1) : max_group_id;
  unsigned gbits = 0;
  while (gbits < 31 && (gmax >> gbits) != 0) ++gbits;
  const unsigned gk = (unsigned)std::min<int64_t>((R + kThreads - 1) / kThreads, 4096);
  hipLaunchKernelGGL(ge_key_k, dim3(gk), dim3(kThreads), 0, st, logit, y, group_id, R, gmax, at<u64>(ws, l.keys),
                     at<uint8_t>(ws, l.lab), flag);
  RSX_LAUNCHED();
  size_t tb = (size_t)l.temp_bytes;
  const hipError_t se = sort_pairs(at<void>(ws, l.temp), tb, at<u64>(ws, l.keys), at<u64>(ws, l.keys_o),
                                   at<uint8_t>(ws, l.lab), at<uint8_t>(ws, l.lab_o), R, 32u + gbits, st);
  if (se != hipSuccess) {
    rsx::set_error("%s: sort failed: %s", __func__, hipGetErrorString(se));
    return (int)se;
  }
  RSX_LAUNCHED();
  TileArrays ta{at<int>(ws, l.neg),      at<int>(ws, l.heads),   at<i64>(ws, l.ghead),   at<i64>(ws, l.thead),
                at<int>(ws, l.negoff),   at<int>(ws, l.headoff), at<i64>(ws, l.carry_g), at<i64>(ws, l.carry_t),
                at<int>(ws, l.agg_head), at<u64>(ws, l.agg_v),   at<double>(ws, l.agg_d), at<int>(ws, l.rec_ord),
                at<u64>(ws, l.rec_v),    at<double>(ws, l.rec_d)};
  GroupOut out{gid, reinterpret_cast<i64*>(P), reinterpret_cast<i64*>(N), reinterpret_cast<i64*>(U2), dcg};
  i64* sum = reinterpret_cast<i64*>(summary);
  const u64* sk = at<u64>(ws, l.keys_o);
  const uint8_t* sl = at<uint8_t>(ws, l.lab_o);
  hipLaunchKernelGGL(ge_tile_k<false>, dim3((unsigned)l.tiles), dim3(kThreads), 0, st, sk, sl, R, top, D, ta, out);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(ge_carry_k, dim3(1), dim3(1024), 0, st, ta, l.tiles, sum);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(ge_tile_k<true>, dim3((unsigned)l.tiles), dim3(kThreads), 0, st, sk, sl, R, top, D, ta, out);
  RSX_LAUNCHED();
  hipLaunchKernelGGL(ge_fix_k, dim3(1), dim3(1024), 0, st, ta, l.tiles, out);
  RSX_LAUNCHED();
  const int gb = (int)std::min<int64_t>((R + 1023) / 1024, kGroupBlocks);
  hipLaunchKernelGGL(ge_group_k, dim3(gb), dim3(kThreads), 0, st, out, sum, top, D, at<double>(ws, l.part));
  RSX_LAUNCHED();
  hipLaunchKernelGGL(ge_sum_k, dim3(1), dim3(64), 0, st, at<double>(ws, l.part), gb, sum);
  RSX_LAUNCHED();
  return 0;
}
