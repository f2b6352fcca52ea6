// The towers' feature frames from the transaction log (reference staticstics/preprosess_agg_parallel.py): the
// calendar columns, per-customer and per-item statistics, the weekly sales matrix, the item and user columns,
// quantile buckets and the cleaned sequences; and the passes behind the persona columns (reference
// staticstics/preprocess_clustering.py): run statistics, float64 segment sums and the price ratio. Specified in
// include/recsys_amd.h ("transaction features") and restated in pandas / numpy float64 by tests/tx_features_ref.py
// and tests/persona_ref.py.
//
// Every per-segment quantity is a segmented scan over the rows in their sorted order, the shape of gbdt_ts.hip:
//   seg_tile_k<P, REV, false>  per 256-row tile the segmented workgroup scan (rsx_block.h) -> the tile's aggregate
//   seg_carry_k<P, REV>        one workgroup scans the tile aggregates in chunks of 256 -> the carry into each tile
//   seg_tile_k<P, REV, true>   the in-tile scan again plus the carry; P::store sees every row's inclusive value
// P (a "pass") says what a row contributes, how two values combine and what is kept. One row per thread, no
// thread walks a segment, no workgroup waits on another (launches in stream order), every slot has one writer and
// the order of combination is fixed: the same bits every run, floating-point sums included. The only atomics are
// integer: the OR into flag, the maximum of the segment marks and the counts of the weekly matrix.
#include "rsx_block.h"
#include "rsx_colsum.h"
#include "rsx_common.h"

#include <limits.h>

// a * b + c stays two roundings: the quantile edges and the two-pass moments are specified that way
#pragma clang fp contract(off)

namespace {

using rsx::block_scan_excl, rsx::Seg, rsx::SegOp;

constexpr int kThreads = 256;      // rows per tile: one row per thread
constexpr int kTileBytes = 64;     // workspace bytes per tile: every pass's Seg<V> fits
constexpr int kMaxQ = 126;         // quantile buckets fit an int8
constexpr int kScaled = 4;           // the standardised user columns

int64_t tiles_of(int64_t n) { return (n + kThreads - 1) / kThreads; }
bool rows_ok(int64_t T) { return T >= 1 && T < (1ll << 31); }

// ---------------------------------------------------------------------------------------------------------
// the three launches of a pass
template <class P, bool REV, bool APPLY>
__global__ __launch_bounds__(kThreads) void seg_tile_k(P p, const int* __restrict__ row_seg, int64_t T,
                                                       Seg<typename P::V>* tiles) {
  using V = typename P::V;
  using SV = Seg<V>;
  using Op = typename P::Op;
  static_assert(sizeof(SV) <= kTileBytes, "a tile aggregate fits its workspace slot");
  __shared__ SV sm[kThreads / 64];
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool in = t < T;
  // segment of the row and of its neighbours; row_seg NULL: all rows are one segment. -2 = no such row
  int sid = -2, sprev = -2, snext = -2;
  if (in) {
    sid = row_seg ? row_seg[t] : 0;
    if (t > 0) sprev = row_seg ? row_seg[t - 1] : 0;
    if (t + 1 < T) snext = row_seg ? row_seg[t + 1] : 0;
  }
  const bool first = !in || sprev != sid, last = !in || snext != sid;
  const bool head = REV ? last : first, tail = REV ? first : last;
  if (sid >= 0 && sprev > sid) p.unordered();      // equal segments must be contiguous: row_seg may not decrease
  const V x = in ? p.load(t, sid, first) : P::ident();
  SV tot;
  const SV before = block_scan_excl<kThreads, REV>(SV{x, head ? 1 : 0}, SegOp<V, Op>(), SV{P::ident(), 0}, sm, tot);
  if (!APPLY) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
    return;
  }
  if (!in) return;
  V incl = x;
  if (!head) {
    V pre = before.v;
    if (!before.head) pre = Op()(tiles[blockIdx.x].v, pre);      // the segment began in an earlier tile
    incl = Op()(pre, x);
  }
  p.store(t, sid, incl, x, tail);
}

// tiles[u] = the aggregate of tile u -> the carry into it: the values of the trailing pieces of the tiles since the
// last one in which a segment started (that one included), in scan order (REV: from the last tile down).
template <class P, bool REV>
__global__ __launch_bounds__(kThreads) void seg_carry_k(Seg<typename P::V>* tiles, int64_t n_tiles) {
  using V = typename P::V;
  using SV = Seg<V>;
  __shared__ SV sm[kThreads / 64];
  const SegOp<V, typename P::Op> op;
  const SV ident{P::ident(), 0};
  SV run = ident;
  for (int64_t b = 0; b < n_tiles; b += kThreads) {
    const int64_t u = b + threadIdx.x, at = REV ? n_tiles - 1 - u : u;
    const SV x = u < n_tiles ? tiles[at] : ident;
    SV tot;
    const SV before = block_scan_excl<kThreads, false>(x, op, ident, sm, tot);
    if (u < n_tiles) tiles[at] = SV{op(run, before).v, 0};
    run = op(run, tot);
  }
}

template <class P, bool REV>
void run_pass(const P& p, const int* row_seg, int64_t T, void* ws, hipStream_t st) {
  auto* tiles = reinterpret_cast<Seg<typename P::V>*>(ws);
  const int64_t n_tiles = tiles_of(T);
  const dim3 grid((unsigned)n_tiles), block(kThreads);
  hipLaunchKernelGGL((seg_tile_k<P, REV, false>), grid, block, 0, st, p, row_seg, T, tiles);
  hipLaunchKernelGGL((seg_carry_k<P, REV>), dim3(1), block, 0, st, tiles, n_tiles);
  hipLaunchKernelGGL((seg_tile_k<P, REV, true>), grid, block, 0, st, p, row_seg, T, tiles);
}

struct IntV {
  int n;
};
struct AddInt {
  __device__ __forceinline__ IntV operator()(IntV a, IntV b) const { return IntV{a.n + b.n}; }
};
struct MaxInt {
  __device__ __forceinline__ IntV operator()(IntV a, IntV b) const { return IntV{a.n > b.n ? a.n : b.n}; }
};
struct DblV {
  double s;
};
struct AddDbl {
  __device__ __forceinline__ DblV operator()(DblV a, DblV b) const { return DblV{a.s + b.s}; }
};

// ---------------------------------------------------------------------------------------------------------
// 1. calendar
__global__ __launch_bounds__(kThreads) void calendar_k(const int* __restrict__ day, int64_t T, uint8_t* __restrict__ weekend,
                                                       int* __restrict__ month, int* __restrict__ week, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  int d = day[t];
  if (d < 0) {
    atomicOr(flag, 1);
    d = 0;
  }
  // civil-from-days on the proleptic Gregorian calendar, the era shifted to 0000-03-01
  const int64_t z = (int64_t)d + 719468;
  const int64_t era = z / 146097;
  const int doe = (int)(z - era * 146097);
  const int yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const int mp = (5 * doy + 2) / 153;
  const int m = mp < 10 ? mp + 3 : mp - 9;
  const int64_t y = (int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0);
  const int64_t dd = (int64_t)d + 3;      // 1970-01-01 was a Thursday
  weekend[t] = dd % 7 >= 5 ? 1 : 0;
  month[t] = (int)(12 * y + m - 1);
  week[t] = (int)(dd / 7);
}

// ---------------------------------------------------------------------------------------------------------
// the segment of every row from the offsets: marks, then an inclusive maximum scan over all rows
__global__ __launch_bounds__(kThreads) void seg_mark_k(const int64_t* __restrict__ off, int64_t S, int64_t T, int* marks,
                                                       int* flag) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s > S) return;
  const int64_t a = off[s];
  const int64_t lo = a < 0 ? 0 : (a > T ? T : a);
  bool bad = a != lo || (s == 0 && a != 0) || (s == S && a != T);
  if (s < S) {
    const int64_t b = off[s + 1];
    const int64_t hi = b < 0 ? 0 : (b > T ? T : b);
    if (hi < lo) bad = true;
    if (hi > lo) atomicMax(&marks[lo], (int)s + 1);
  } else if (lo < T) {
    atomicMax(&marks[lo], (int)S + 1);      // the rows behind the last offset belong to nobody
  }
  if (bad) atomicOr(flag, 1);
}

struct RowsP {
  using V = IntV;
  using Op = MaxInt;
  int* row_seg;      // in: the marks, out: the segment
  int S;
  __device__ static V ident() { return V{0}; }
  __device__ void unordered() const {}
  __device__ V load(int64_t t, int, bool) const { return V{row_seg[t]}; }
  __device__ void store(int64_t t, int, V incl, V, bool) const { row_seg[t] = incl.n >= 1 && incl.n <= S ? incl.n - 1 : -1; }
};

// ---------------------------------------------------------------------------------------------------------
// 2. segment statistics
struct StatV {
  double sum;
  long long chan;
  int cnt, dmin, dmax, wk;
};
struct StatOp {
  __device__ __forceinline__ StatV operator()(StatV a, StatV b) const {
    return StatV{a.sum + b.sum, a.chan + b.chan, a.cnt + b.cnt, a.dmin < b.dmin ? a.dmin : b.dmin,
                 a.dmax > b.dmax ? a.dmax : b.dmax, a.wk + b.wk};
  }
};

// the table row behind sorted position t: t itself, or perm[t]; -1 (and flag bit 0) outside [0, T)
__device__ __forceinline__ int64_t row_at(const int64_t* __restrict__ perm, int64_t t, int64_t T, int* flag) {
  if (!perm) return t;
  const int64_t r = perm[t];
  if ((uint64_t)r < (uint64_t)T) return r;
  atomicOr(flag, 1);
  return -1;
}

struct StatsP {
  using V = StatV;
  using Op = StatOp;
  const int64_t* perm;
  const float* price;
  const int* day;
  const uint8_t *channel, *weekend;
  int64_t T;
  int S;
  int *count, *dmin, *dmax, *wkend;
  double* sum;
  float* last;
  long long* chan;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0.0, 0, 0, INT_MAX, INT_MIN, 0}; }
  __device__ V load(int64_t t, int sid, bool first) const {
    if (first && sid >= S) atomicOr(flag, 1);
    if ((unsigned)sid >= (unsigned)S) return ident();
    const int64_t r = row_at(perm, t, T, flag);
    if (r < 0) return ident();
    const int d = day[r];
    return V{(double)price[r], (long long)channel[r], 1, d, d, weekend[r] ? 1 : 0};
  }
  __device__ void store(int64_t t, int sid, V incl, V x, bool tail) const {
    if (!tail || (unsigned)sid >= (unsigned)S) return;
    count[sid] = incl.cnt;
    sum[sid] = incl.sum;
    chan[sid] = incl.chan;
    wkend[sid] = incl.wk;
    dmin[sid] = incl.cnt ? incl.dmin : 0;
    dmax[sid] = incl.cnt ? incl.dmax : 0;
    last[sid] = x.cnt ? (float)x.sum : 0.0f;      // the segment's last row: its own price
  }
};

// the second pass: M2 = sum (price - mean)^2 with mean = sum / n of the first
struct M2P {
  using V = DblV;
  using Op = AddDbl;
  const int64_t* perm;
  const float* price;
  int64_t T;
  int S;
  const int* count;
  const double* sum;
  double* m2;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0.0}; }
  __device__ V load(int64_t t, int sid, bool) const {
    if ((unsigned)sid >= (unsigned)S) return ident();
    const int64_t r = row_at(perm, t, T, flag);
    const int n = count[sid];
    if (r < 0 || n <= 0) return ident();
    const double d = (double)price[r] - sum[sid] / (double)n;
    return V{d * d};
  }
  __device__ void store(int64_t, int sid, V incl, V, bool tail) const {
    if (tail && (unsigned)sid < (unsigned)S) m2[sid] = incl.s;
  }
};

// ---------------------------------------------------------------------------------------------------------
// 3. distinct values of a column that is non-decreasing inside every segment: the number of heads
struct DistinctP {
  using V = IntV;
  using Op = AddInt;
  const int* val;
  int S;
  int* out;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0}; }
  __device__ V load(int64_t t, int sid, bool first) const {
    if ((unsigned)sid >= (unsigned)S) {
      if (first && sid >= S) atomicOr(flag, 1);
      return ident();
    }
    if (first) return V{1};
    const int a = val[t - 1], b = val[t];
    if (b < a) atomicOr(flag, 2);
    return V{a != b ? 1 : 0};
  }
  __device__ void store(int64_t, int sid, V incl, V, bool tail) const {
    if (tail && (unsigned)sid < (unsigned)S) out[sid] = incl.n;
  }
};

// ---------------------------------------------------------------------------------------------------------
// 4. weekly sales: one row per thread, the week's column by binary search, integer atomics. In the table's order
// an item's rows are spread over the customers, so the adds of one wave go to different cells.
__global__ __launch_bounds__(kThreads) void weekly_k(const int* __restrict__ item, const int* __restrict__ week, int64_t T,
                                                     const int* __restrict__ weeks, int W, int64_t N, int* weekly, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const int i = item[t], w = week[t];
  int lo = 0, hi = W;      // the first column with weeks[col] >= w
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (weeks[mid] < w) lo = mid + 1;
    else hi = mid;
  }
  if ((uint64_t)i >= (uint64_t)N || lo >= W || weeks[lo] != w) {
    atomicOr(flag, 1);
    return;
  }
  atomicAdd(&weekly[(int64_t)i * W + lo], 1);
}

// ---------------------------------------------------------------------------------------------------------
// fixed-order column sums in two levels: rsx_colsum.h
using rsx::col_sums;
int64_t chunks_of(int64_t n) { return rsx::col_chunks(n); }

// ---------------------------------------------------------------------------------------------------------
// 5. item columns
__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void item_cols_k(const int* __restrict__ weekly, int64_t N, int W,
                                                        const int* __restrict__ count, const double* __restrict__ sum,
                                                        const int* __restrict__ dmin, int64_t T, int max_day,
                                                        float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int* row = weekly + i * W;
  const int n = count[i];
  long long cur_m = 0, prev_m = 0;
  for (int c = W - 4 > 0 ? W - 4 : 0; c < W; ++c) cur_m += row[c];
  for (int c = W - 8 > 0 ? W - 8 : 0; c < W - 4; ++c) prev_m += row[c];
  const int cur_w = row[W - 1], prev_w = W > 1 ? row[W - 2] : 0;
  const int k = W < 12 ? W : 12;
  double steady = 0.0;      // one column: the standard deviation is NaN and the frame's fillna(0) makes it 0
  if (k > 1) {
    long long s = 0;
    for (int c = W - k; c < W; ++c) s += row[c];
    const double mean = (double)s / k;
    double ss = 0.0;
    for (int c = W - k; c < W; ++c) {
      const double d = (double)row[c] - mean;
      ss += d * d;
    }
    steady = log1p(mean / (sqrt(ss / (k - 1)) + 1e-9));
  }
  const double days = n > 0 ? (double)((int64_t)max_day - dmin[i]) : 0.0;
  out[0 * N + i] = (float)((double)n / (double)T);
  out[1 * N + i] = (float)log1p((double)cur_w);
  out[2 * N + i] = (float)log1p((double)cur_m);
  out[3 * N + i] = (float)clip((double)(cur_w - prev_w) / ((double)prev_w + 1.0), -1.0, 5.0);
  out[4 * N + i] = (float)clip((double)(cur_m - prev_m) / ((double)prev_m + 1.0), -1.0, 5.0);
  out[5 * N + i] = (float)steady;
  out[6 * N + i] = (float)log1p(n > 0 ? sum[i] / (double)n : 0.0);
  out[7 * N + i] = (float)log1p(days < 0.0 ? 0.0 : days);
}

// the cold-start imputation: the four popularity / velocity columns of an item released fewer than cold_days ago
// become the column's mean over all items (col_sum / N, taken before this kernel)
__global__ __launch_bounds__(kThreads) void item_impute_k(int64_t N, const int* __restrict__ count, const int* __restrict__ dmin,
                                                          int max_day, int cold_days, const double* __restrict__ col_sum,
                                                          float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int64_t days = count[i] > 0 ? (int64_t)max_day - dmin[i] : 0;
  if (days >= cold_days) return;
  for (int c = 0; c < 4; ++c) out[(1 + c) * N + i] = (float)(col_sum[c] / (double)N);
}

// ---------------------------------------------------------------------------------------------------------
// 6. user columns
__global__ __launch_bounds__(kThreads) void user_cols_k(const int* __restrict__ count, const double* __restrict__ sum,
                                                        const double* __restrict__ m2, const float* __restrict__ last,
                                                        const int* __restrict__ dmax, const long long* __restrict__ chan,
                                                        const int* __restrict__ wkend, const int* __restrict__ uniq,
                                                        const int* __restrict__ months, int64_t C, int max_day,
                                                        double* __restrict__ x, double* __restrict__ f64,
                                                        float* __restrict__ cols, int8_t* __restrict__ channel,
                                                        int16_t* __restrict__ active) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  const int n = count[c];
  double mean = 0.0, sd = 0.0, diff = 0.0, rep = 0.0, wk = 0.0, rec = 0.0, ch = 0.0;
  if (n > 0) {
    mean = sum[c] / (double)n;
    sd = n > 1 ? sqrt(m2[c] / (double)(n - 1)) : 0.0;
    diff = (double)last[c] - mean;
    rep = 1.0 - (double)uniq[c] / (double)n;
    wk = (double)wkend[c] / (double)n;
    rec = (double)((int64_t)max_day - dmax[c]);
    ch = (double)chan[c] / (double)n;
  }
  const float sd32 = (float)sd, diff32 = (float)diff, rep32 = (float)rep;
  f64[0 * C + c] = mean;
  f64[1 * C + c] = (double)n;
  f64[2 * C + c] = rec;
  // what is standardised: the three float32 columns as stored, weekend_ratio in float64 (the reference's dtypes)
  x[0 * C + c] = (double)sd32;
  x[1 * C + c] = (double)diff32;
  x[2 * C + c] = (double)rep32;
  x[3 * C + c] = wk;
  cols[0 * C + c] = sd32;
  cols[1 * C + c] = diff32;
  cols[2 * C + c] = rep32;
  cols[3 * C + c] = (float)wk;
  cols[8 * C + c] = (float)log1p(mean);
  cols[9 * C + c] = (float)log1p((double)n);
  cols[10 * C + c] = (float)log1p(rec < 0.0 ? 0.0 : rec);
  channel[c] = ch > 1.5 ? 2 : 1;
  const int am = months[c];
  active[c] = (int16_t)(am < 0 ? 0 : (am > 32767 ? 32767 : am));
}

__global__ __launch_bounds__(kThreads) void user_scale_k(const double* __restrict__ x, int64_t C, const double* __restrict__ col_sum,
                                                         const double* __restrict__ col_ss, float* __restrict__ cols) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  for (int j = 0; j < kScaled; ++j) {
    float v = 0.0f;      // one customer: the standard deviation is NaN and the frame's fillna(0) makes it 0
    if (C > 1) {
      const double mean = col_sum[j] / (double)C, sd = sqrt(col_ss[j] / (double)(C - 1));
      v = (float)((x[j * C + c] - mean) / (sd + 1e-9));
    }
    cols[(4 + j) * C + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// 7. quantile buckets: the edges by one thread (q + 1 <= 127 of them), then one value per thread
__global__ void quantile_edges_k(const double* __restrict__ s, int64_t n, int q, double* __restrict__ edges, int* __restrict__ n_edges) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int m = 0;
  const double step = 1.0 / (double)q;
  for (int k = 0; k <= q; ++k) {
    // h = (n - 1) k / q in the floating-point steps of pandas' quantile (numpy.percentile of linspace(0, 1, q + 1))
    double p = k == q ? 1.0 : (double)k * step;
    p = (p * 100.0) / 100.0;
    const double h = (double)(n - 1) * p;
    int64_t lo = (int64_t)floor(h);
    double t = h - (double)lo;
    if (lo >= n - 1) {
      lo = n - 1;
      t = 0.0;
    }
    const double a = s[lo], b = s[lo + 1 < n ? lo + 1 : lo], d = b - a;
    const double e = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
    if (m == 0 || e != edges[m - 1]) edges[m++] = e;
  }
  *n_edges = m;
}

__global__ __launch_bounds__(kThreads) void quantile_bucket_k(const double* __restrict__ x, int64_t n, const double* __restrict__ edges,
                                                              const int* __restrict__ n_edges, int8_t* __restrict__ bucket) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int m = *n_edges;
  m = m < 0 ? 0 : (m > kMaxQ + 1 ? kMaxQ + 1 : m);
  const double v = x[i];
  int b = 0;
  for (int k = 0; k < m; ++k) b += edges[k] < v ? 1 : 0;
  if (m >= 2 && b > m - 1) b = m - 1;      // above the top edge: cannot happen for the column the edges came from
  bucket[i] = (int8_t)(b < 1 ? 1 : b);     // the lowest edge itself is in the first bucket; a constant column is all 1
}

// ---------------------------------------------------------------------------------------------------------
// 8. sequences: the rank of a valid row among the valid rows of its customer, counted from the end
struct SeqRankP {
  using V = IntV;
  using Op = AddInt;
  const int *item, *day;
  const uint8_t* valid;
  int64_t N;
  int C;
  int *rank, *n_valid, *last_day;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0}; }
  __device__ V load(int64_t t, int sid, bool first) const {
    if ((unsigned)sid >= (unsigned)C) {
      if (first && sid >= C) atomicOr(flag, 1);
      return ident();
    }
    const int i = item[t];
    if ((uint64_t)i >= (uint64_t)N) {
      atomicOr(flag, 1);
      return ident();
    }
    return V{valid[i] ? 1 : 0};
  }
  // REV: incl counts the valid rows from t to the end of the customer; tail = the customer's first row
  __device__ void store(int64_t t, int sid, V incl, V x, bool tail) const {
    rank[t] = x.n ? incl.n - 1 : -1;
    if ((unsigned)sid >= (unsigned)C) return;
    if (x.n && incl.n == 1) last_day[sid] = day[t];
    if (tail) n_valid[sid] = incl.n;
  }
};

__global__ __launch_bounds__(kThreads) void seq_write_k(const int* __restrict__ row_seg, int64_t C, int64_t T,
                                                        const int* __restrict__ item, const int* __restrict__ day,
                                                        const int* __restrict__ rank, const int* __restrict__ last_day,
                                                        const int64_t* __restrict__ seq_off, int max_len, int64_t n_out,
                                                        int* __restrict__ seq_item, int* __restrict__ seq_delta, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const int r = rank[t], sid = row_seg[t];
  if (r < 0 || r >= max_len || (uint64_t)sid >= (uint64_t)C) return;
  const int64_t a = seq_off[sid], b = seq_off[sid + 1], pos = b - 1 - r;
  if (a < 0 || b > n_out || pos < a) {      // offsets that are not those of min(n_valid, max_len)
    atomicOr(flag, 1);
    return;
  }
  seq_item[pos] = item[t];
  seq_delta[pos] = last_day[sid] - day[t];
}

// ---------------------------------------------------------------------------------------------------------
// 9. runs of a column that is non-decreasing inside every segment (the persona columns). A run starts at a segment's
// first row and wherever val changes. RunLenP: the inclusive maximum of "t + 1 where a run starts" is the start of
// the run a row is in, so a run's last row knows its length; tail_len[t] = that length there and 0 elsewhere.
// RunSumP sums what the run tails contribute per segment.
struct RunLenP {
  using V = IntV;
  using Op = MaxInt;
  const int* val;
  int S;
  int* tail_len;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0}; }
  __device__ V load(int64_t t, int sid, bool first) const {
    if ((unsigned)sid >= (unsigned)S) {
      if (first && sid >= S) atomicOr(flag, 1);
      return ident();
    }
    if (first) return V{(int)t + 1};
    const int a = val[t - 1], b = val[t];
    if (b < a) atomicOr(flag, 2);
    return V{a != b ? (int)t + 1 : 0};
  }
  __device__ void store(int64_t t, int sid, V incl, V, bool tail) const {
    int len = 0;
    if ((unsigned)sid < (unsigned)S && incl.n >= 1 && (tail || val[t + 1] != val[t])) len = (int)t + 2 - incl.n;
    tail_len[t] = len;
  }
};

struct RunV {
  double nlogn;
  int runs, repeated;
};
struct RunOp {
  __device__ __forceinline__ RunV operator()(RunV a, RunV b) const {
    return RunV{a.nlogn + b.nlogn, a.runs + b.runs, a.repeated + b.repeated};
  }
};
struct RunSumP {
  using V = RunV;
  using Op = RunOp;
  const int* tail_len;
  int S;
  int *runs, *repeated;
  double* nlogn;
  __device__ void unordered() const {}
  __device__ static V ident() { return V{0.0, 0, 0}; }
  __device__ V load(int64_t t, int sid, bool) const {
    if ((unsigned)sid >= (unsigned)S) return ident();
    const int n = tail_len[t];
    if (n <= 0) return ident();
    return V{(double)n * log((double)n), 1, n > 1 ? n : 0};
  }
  __device__ void store(int64_t, int sid, V incl, V, bool tail) const {
    if (!tail || (unsigned)sid >= (unsigned)S) return;
    runs[sid] = incl.runs;
    repeated[sid] = incl.repeated;
    nlogn[sid] = incl.nlogn;
  }
};

// ---------------------------------------------------------------------------------------------------------
// 10. count, sum and two-pass M2 of a double column per segment: StatsP / M2P without the table's columns
struct SumV {
  double sum;
  int cnt;
};
struct SumOp {
  __device__ __forceinline__ SumV operator()(SumV a, SumV b) const { return SumV{a.sum + b.sum, a.cnt + b.cnt}; }
};
struct SumF64P {
  using V = SumV;
  using Op = SumOp;
  const int64_t* perm;
  const double* x;
  int64_t T;
  int S;
  int* count;
  double* sum;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0.0, 0}; }
  __device__ V load(int64_t t, int sid, bool first) const {
    if (first && sid >= S) atomicOr(flag, 1);
    if ((unsigned)sid >= (unsigned)S) return ident();
    const int64_t r = row_at(perm, t, T, flag);
    if (r < 0) return ident();
    return V{x[r], 1};
  }
  __device__ void store(int64_t, int sid, V incl, V, bool tail) const {
    if (!tail || (unsigned)sid >= (unsigned)S) return;
    count[sid] = incl.cnt;
    sum[sid] = incl.sum;
  }
};
struct M2F64P {
  using V = DblV;
  using Op = AddDbl;
  const int64_t* perm;
  const double* x;
  int64_t T;
  int S;
  const int* count;
  const double* sum;
  double* m2;
  int* flag;
  __device__ void unordered() const { atomicOr(flag, 1); }
  __device__ static V ident() { return V{0.0}; }
  __device__ V load(int64_t t, int sid, bool) const {
    if ((unsigned)sid >= (unsigned)S) return ident();
    const int64_t r = row_at(perm, t, T, flag);
    const int n = count[sid];
    if (r < 0 || n <= 0) return ident();
    const double d = x[r] - sum[sid] / (double)n;
    return V{d * d};
  }
  __device__ void store(int64_t, int sid, V incl, V, bool tail) const {
    if (tail && (unsigned)sid < (unsigned)S) m2[sid] = incl.s;
  }
};

// ---------------------------------------------------------------------------------------------------------
// 11. the price of a row over the mean price of its item's category
__global__ __launch_bounds__(kThreads) void price_ratio_k(const int* __restrict__ item, const float* __restrict__ price, int64_t T,
                                                          const int* __restrict__ item_cat, const double* __restrict__ cat_mean,
                                                          int64_t N, int n_cat, double* __restrict__ ratio, int* flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const int i = item[t];
  int c = -1;
  if ((uint64_t)i < (uint64_t)N) c = item_cat[i];
  if ((unsigned)c >= (unsigned)n_cat) {
    atomicOr(flag, 1);
    ratio[t] = 0.0;
    return;
  }
  ratio[t] = (double)price[t] / cat_mean[c];
}

bool ws_ok(const void* ws, int64_t ws_bytes, int64_t T) { return ws && rsx::aligned16(ws) && ws_bytes >= kTileBytes * tiles_of(T); }

}  // namespace

#define TX_WS_MSG "workspace too small (rsx_tx_workspace_bytes) or not 16-byte aligned"

RSX_API int64_t rsx_tx_workspace_bytes(int64_t T) { return rows_ok(T) ? kTileBytes * tiles_of(T) : -1; }

RSX_API int rsx_tx_calendar(const int* day, int64_t T, uint8_t* weekend, int* month, int* week, int* flag, void* stream) {
  RSX_ARG(day && weekend && month && week && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  hipLaunchKernelGGL(calendar_k, dim3((unsigned)tiles_of(T)), dim3(kThreads), 0, (hipStream_t)stream, day, T, weekend, month,
                     week, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_segment_rows(const int64_t* seg_off, int64_t S, int64_t T, void* ws, int64_t ws_bytes, int* row_seg,
                                int* flag, void* stream) {
  RSX_ARG(seg_off && row_seg && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(S >= 1 && S < (1ll << 31) - 1, "need 1 <= S < 2^31 - 1 segments");
  RSX_ARG(ws_ok(ws, ws_bytes, T), TX_WS_MSG);
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(row_seg, 0, (size_t)T * 4, st);
  hipLaunchKernelGGL(seg_mark_k, dim3((unsigned)tiles_of(S + 1)), dim3(kThreads), 0, st, seg_off, S, T, row_seg, flag);
  run_pass<RowsP, false>(RowsP{row_seg, (int)S}, nullptr, T, ws, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_segment_stats(const int* row_seg, int64_t S, int64_t T, const int64_t* perm, const float* price,
                                 const int* day, const uint8_t* channel, const uint8_t* weekend, void* ws, int64_t ws_bytes,
                                 int* count, double* sum, double* m2, float* last, int* dmin, int* dmax, int64_t* chan,
                                 int* wkend, int* flag, void* stream) {
  RSX_ARG(row_seg && price && day && channel && weekend && count && sum && m2 && last && dmin && dmax && chan && wkend && flag,
          "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(S >= 1 && S < (1ll << 31) - 1, "need 1 <= S < 2^31 - 1 segments");
  RSX_ARG(ws_ok(ws, ws_bytes, T), TX_WS_MSG);
  hipStream_t st = (hipStream_t)stream;
  // a segment without rows keeps zeros everywhere
  (void)hipMemsetAsync(count, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(sum, 0, (size_t)S * 8, st);
  (void)hipMemsetAsync(m2, 0, (size_t)S * 8, st);
  (void)hipMemsetAsync(last, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(dmin, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(dmax, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(chan, 0, (size_t)S * 8, st);
  (void)hipMemsetAsync(wkend, 0, (size_t)S * 4, st);
  run_pass<StatsP, false>(StatsP{perm, price, day, channel, weekend, T, (int)S, count, dmin, dmax, wkend, sum, last,
                                 reinterpret_cast<long long*>(chan), flag},
                          row_seg, T, ws, st);
  run_pass<M2P, false>(M2P{perm, price, T, (int)S, count, sum, m2, flag}, row_seg, T, ws, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_segment_distinct(const int* row_seg, int64_t S, int64_t T, const int* val, void* ws, int64_t ws_bytes,
                                    int* distinct, int* flag, void* stream) {
  RSX_ARG(row_seg && val && distinct && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(S >= 1 && S < (1ll << 31) - 1, "need 1 <= S < 2^31 - 1 segments");
  RSX_ARG(ws_ok(ws, ws_bytes, T), TX_WS_MSG);
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(distinct, 0, (size_t)S * 4, st);
  run_pass<DistinctP, false>(DistinctP{val, (int)S, distinct, flag}, row_seg, T, ws, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_weekly_sales(const int* item, const int* week, int64_t T, const int* weeks, int64_t W, int64_t N,
                                int* weekly, int* flag, void* stream) {
  RSX_ARG(item && week && weeks && weekly && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(W >= 1 && W <= 65536 && N >= 1 && N * W < (1ll << 31), "need 1 <= W <= 65536 weeks, N >= 1 items and N W < 2^31");
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(weekly, 0, (size_t)(N * W) * 4, st);
  hipLaunchKernelGGL(weekly_k, dim3((unsigned)tiles_of(T)), dim3(kThreads), 0, st, item, week, T, weeks, (int)W, N, weekly, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_item_features(const int* weekly, int64_t N, int64_t W, const int* count, const double* sum,
                                 const int* dmin, int64_t T, int max_day, int cold_days, double* col_sum, int64_t col_sum_doubles,
                                 float* out,
                                 void* stream) {
  RSX_ARG(weekly && count && sum && dmin && col_sum && out, "null tensor");
  RSX_ARG(col_sum_doubles >= 4 + 4 * chunks_of(N), "col_sum too small (4 + 4 ceil(N / 4096) doubles)");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(W >= 1 && W <= 65536 && N >= 1 && N * W < (1ll << 31), "need 1 <= W <= 65536 weeks, N >= 1 items and N W < 2^31");
  RSX_ARG(cold_days >= 0, "cold_days must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles_of(N)), block(kThreads);
  hipLaunchKernelGGL(item_cols_k, grid, block, 0, st, weekly, N, (int)W, count, sum, dmin, T, max_day, out);
  col_sums<float>(out + N, N, 4, nullptr, col_sum + 4, col_sum, st);
  hipLaunchKernelGGL(item_impute_k, grid, block, 0, st, N, count, dmin, max_day, cold_days, (const double*)col_sum, out);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_user_features(const int* count, const double* sum, const double* m2, const float* last, const int* dmax,
                                 const int64_t* chan, const int* wkend, const int* uniq, const int* months, int64_t C,
                                 int max_day, void* ws, int64_t ws_bytes, double* f64, float* cols, int8_t* channel,
                                 int16_t* active_months, void* stream) {
  RSX_ARG(count && sum && m2 && last && dmax && chan && wkend && uniq && months && f64 && cols && channel && active_months,
          "null tensor");
  RSX_ARG(C >= 1 && C < (1ll << 31), "need 1 <= C < 2^31 customers");
  RSX_ARG(ws && rsx::aligned16(ws) && ws_bytes >= (kScaled * C + 2 * kScaled + kScaled * chunks_of(C)) * 8,
          "workspace too small ((4 C + 8 + 4 ceil(C / 4096)) * 8 bytes) or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* x = reinterpret_cast<double*>(ws);
  double *col_sum = x + kScaled * C, *col_ss = col_sum + kScaled, *part = col_ss + kScaled;
  const dim3 grid((unsigned)tiles_of(C)), block(kThreads);
  hipLaunchKernelGGL(user_cols_k, grid, block, 0, st, count, sum, m2, last, dmax, reinterpret_cast<const long long*>(chan), wkend,
                     uniq, months, C, max_day, x, f64, cols, channel, active_months);
  col_sums<double>(x, C, kScaled, nullptr, part, col_sum, st);
  col_sums<double>(x, C, kScaled, col_sum, part, col_ss, st);
  hipLaunchKernelGGL(user_scale_k, grid, block, 0, st, (const double*)x, C, (const double*)col_sum, (const double*)col_ss, cols);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_quantile_bucket(const double* x, const double* sorted, int64_t n, int q, double* edges, int* n_edges,
                                int8_t* bucket, void* stream) {
  RSX_ARG(x && sorted && edges && n_edges && bucket, "null tensor");
  RSX_ARG(n >= 1 && n < (1ll << 31), "need 1 <= n < 2^31 values");
  RSX_ARG(q >= 1 && q <= kMaxQ, "need 1 <= q <= 126 buckets");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(quantile_edges_k, dim3(1), dim3(64), 0, st, sorted, n, q, edges, n_edges);
  hipLaunchKernelGGL(quantile_bucket_k, dim3((unsigned)tiles_of(n)), dim3(kThreads), 0, st, x, n, (const double*)edges,
                     (const int*)n_edges, bucket);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_sequence_ranks(const int* row_seg, int64_t C, int64_t T, const int* item, const int* day,
                                  const uint8_t* valid, int64_t N, void* ws, int64_t ws_bytes, int* rank, int* n_valid,
                                  int* last_day, int* flag, void* stream) {
  RSX_ARG(row_seg && item && day && valid && rank && n_valid && last_day && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(C >= 1 && C < (1ll << 31) - 1 && N >= 1 && N < (1ll << 31), "need 1 <= C < 2^31 - 1 customers and 1 <= N < 2^31 items");
  RSX_ARG(ws_ok(ws, ws_bytes, T), TX_WS_MSG);
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(n_valid, 0, (size_t)C * 4, st);
  (void)hipMemsetAsync(last_day, 0, (size_t)C * 4, st);
  run_pass<SeqRankP, true>(SeqRankP{item, day, valid, N, (int)C, rank, n_valid, last_day, flag}, row_seg, T, ws, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_sequences(const int* row_seg, int64_t C, int64_t T, const int* item, const int* day, const int* rank,
                             const int* last_day, const int64_t* seq_off, int max_len, int64_t n_out, int* seq_item,
                             int* seq_delta, int* flag, void* stream) {
  RSX_ARG(row_seg && item && day && rank && last_day && seq_off && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(C >= 1 && C < (1ll << 31) - 1, "need 1 <= C < 2^31 - 1 customers");
  RSX_ARG(max_len >= 1, "max_len must be >= 1");
  RSX_ARG(n_out >= 0 && n_out <= T && (n_out == 0 || (seq_item && seq_delta)), "need 0 <= n_out <= T kept rows and their arrays");
  if (n_out == 0) return 0;
  hipLaunchKernelGGL(seq_write_k, dim3((unsigned)tiles_of(T)), dim3(kThreads), 0, (hipStream_t)stream, row_seg, C, T, item, day,
                     rank, last_day, seq_off, max_len, n_out, seq_item, seq_delta, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_segment_runs(const int* row_seg, int64_t S, int64_t T, const int* val, void* ws, int64_t ws_bytes,
                                int* runs, int* repeated, double* nlogn, int* flag, void* stream) {
  RSX_ARG(row_seg && val && runs && repeated && nlogn && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(S >= 1 && S < (1ll << 31) - 1, "need 1 <= S < 2^31 - 1 segments");
  RSX_ARG(ws && rsx::aligned16(ws) && ws_bytes >= kTileBytes * tiles_of(T) + 4 * T,
          "workspace too small (rsx_tx_workspace_bytes(T) + 4 T bytes) or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* tail_len = rsx::at<int>(ws, kTileBytes * tiles_of(T));      // behind the tiles' slots
  (void)hipMemsetAsync(runs, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(repeated, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(nlogn, 0, (size_t)S * 8, st);
  run_pass<RunLenP, false>(RunLenP{val, (int)S, tail_len, flag}, row_seg, T, ws, st);
  run_pass<RunSumP, false>(RunSumP{tail_len, (int)S, runs, repeated, nlogn}, row_seg, T, ws, st);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_segment_sum_f64(const int* row_seg, int64_t S, int64_t T, const int64_t* perm, const double* x, void* ws,
                                   int64_t ws_bytes, int* count, double* sum, double* m2, int* flag, void* stream) {
  RSX_ARG(row_seg && x && count && sum && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(S >= 1 && S < (1ll << 31) - 1, "need 1 <= S < 2^31 - 1 segments");
  RSX_ARG(ws_ok(ws, ws_bytes, T), TX_WS_MSG);
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(count, 0, (size_t)S * 4, st);
  (void)hipMemsetAsync(sum, 0, (size_t)S * 8, st);
  run_pass<SumF64P, false>(SumF64P{perm, x, T, (int)S, count, sum, flag}, row_seg, T, ws, st);
  if (m2) {
    (void)hipMemsetAsync(m2, 0, (size_t)S * 8, st);
    run_pass<M2F64P, false>(M2F64P{perm, x, T, (int)S, count, sum, m2, flag}, row_seg, T, ws, st);
  }
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_tx_price_ratio(const int* item, const float* price, int64_t T, const int* item_cat, const double* cat_mean,
                               int64_t N, int64_t n_cat, double* ratio, int* flag, void* stream) {
  RSX_ARG(item && price && item_cat && cat_mean && ratio && flag, "null tensor");
  RSX_ARG(rows_ok(T), "need 1 <= T < 2^31 rows");
  RSX_ARG(N >= 1 && N < (1ll << 31) && n_cat >= 1 && n_cat <= N, "need 1 <= n_cat <= N < 2^31 categories and items");
  hipLaunchKernelGGL(price_ratio_k, dim3((unsigned)tiles_of(T)), dim3(kThreads), 0, (hipStream_t)stream, item, price, T, item_cat,
                     cat_mean, N, (int)n_cat, ratio, flag);
  RSX_LAUNCHED();
  return 0;
}
