// Internal header of the contrastive-loss (InfoNCE) units nce_*.hip (file map: DESIGN.md, section 4).
// Kernels stay in an anonymous namespace of their own file; only host launchers cross files.
#pragma once
#include "rsx_common.h"
#include "rsx_x3.h"
#include <math.h>
#include <algorithm>
#include <type_traits>

namespace rsx {
namespace nce {

// named here so that the units' `using namespace rsx::nce` finds them
using rsx::bf16x2, rsx::bf16x4, rsx::bf16x8, rsx::f32x16, rsx::f32x2, rsx::f32x4, rsx::tile_row, rsx::u32x4;

constexpr int kD = 128;        // embedding width (fixed by the reference: d_model=128)
constexpr int kTile = 32;      // streamed rows per tile
constexpr int kWaves = 4;      // waves per workgroup
constexpr int kOwnRows = 32 * kWaves;  // owner rows per workgroup
constexpr int kLdsStride = kD + 4;     // padded row (conflict-free ds_read_b128 columns)

enum : int { F_EXCL_DIAG = 1, F_MASK_K1 = 2, F_MASK_K2 = 4, F_POS = 8 };
// the label logit carries no bias: S_ii = <A_i, B_i> / tau ("positive recovery" of
// efficient_corrected_logq_loss, tower_code/mined_inference.py:772-775); plain kernels, with F_MASK_K1 only
enum : int { F_DIAG_NOBIAS = 16 };
enum : int { RSX_NCE_FP32 = 0, RSX_NCE_BF16X3 = 1, RSX_NCE_F16 = 2 };  // logit/gradient precision of the grouped kernels
constexpr int kNsplitBwdGrouped = 8;  // split partials the grouped backward's region is sized for (GroupedLayout)

struct FwdArgs {
  const float* A;     // [N, lda] owner rows (queries)
  const float* B;     // [M, ldb] streamed rows (columns)
  const float* bias;  // [M] or nullptr
  const int* k1a;     // [N] or nullptr
  const int* k1b;     // [M]
  const int* k2a;
  const int* k2b;
  int64_t N, M, lda, ldb;
  int64_t diag_off;  // row i's label / diagonal column is i + diag_off (data-parallel shards)
  float inv_tau;
  int nsplit;
  int64_t cols_per_split;
  float* part;  // [4][nsplit][N] : running max, sum-exp, positive-logit sum, positive count
  const __bf16* shi;  // bf16x3: hi/lo images [M][128] of the streamed rows
  const __bf16* slo;
};

// Block-id remap: all workgroups of one column split share an XCD group (b % 8), so the
// split's streamed operand is re-read from that XCD's L2. Speed only, never correctness.
// I: the block index type (int, or int64_t where the caller's row-block arithmetic is 64-bit).
template <typename I>
__host__ __device__ __forceinline__ void remap_block(I b, int nsplit, int& split, I& rb) {
  const int xcd = (int)(b & 7);
  const I q = b >> 3;
  if (nsplit >= 8) {  // multiple of 8: each split on one XCD group
    const int nsub = nsplit >> 3;
    split = xcd + 8 * (int)(q % nsub);
    rb = q / nsub;
  } else {  // nsplit in {1, 2, 4}: 8 / nsplit XCD groups per split
    split = xcd % nsplit;
    rb = (8 / nsplit) * q + xcd / nsplit;
  }
}
__device__ __forceinline__ void remap_block(int nsplit, int& split, int& rb) {
  remap_block<int>((int)blockIdx.x, nsplit, split, rb);
}

// ---------------------------------------------------------------------------------
// Merge the column splits: LSE, label term, per-row loss/valid/1-over-count.
struct MergeArgs {
  const float* A;
  const float* B;
  const float* bias;
  int64_t N, lda, ldb;
  int64_t diag_off;
  float inv_tau;
  int nsplit;
  const float* part;
  int pos_mode;      // 0: label = diagonal, 1: label = positive set
  int diag_nobias;   // F_DIAG_NOBIAS: the label logit without its bias
  float* lse;       // [N]
  float* row_loss;   // [N]
  float* row_valid;  // [N] 0/1
  float* inv_cnt;    // [N] (pos mode) or nullptr
};

// ---------------------------------------------------------------------------------
// Backward. G_ij = w_i * (P_ij - Y_ij) / tau, P_ij = exp(S_ij - LSE_i) (0 if excluded),
// Y = diagonal (pos_mode 0) or M_ij / cnt_i (pos_mode 1), w_i = g * valid_i where g is the
// upstream gradient of the row-loss SUM (device scalar).
// ROW_OWNED: dA_i = sum_j G_ij B_j ; else dB_j = sum_i G_ij A_i.
struct BwdArgs {
  const float* A;
  const float* B;
  const float* bias;
  const int* k1a;
  const int* k1b;
  const int* k2a;
  const int* k2b;
  int64_t N, M, lda, ldb;
  int64_t diag_off;
  float inv_tau;
  const float* lse;
  const float* row_valid;
  const float* inv_cnt;
  const float* gout;   // upstream gradient of the row-loss sum (device scalar)
  int nsplit;
  int64_t span_per_split;  // streamed rows per split
  float* dout;             // [nsplit][owner_rows][128] (split partials) or final when nsplit==1
  const __bf16* shi;       // bf16x3: hi/lo images [streamed rows][128]
  const __bf16* slo;
};

// ---------------------------------------------------------------------------------
// Device helpers shared by the plain and the grouped kernels.
//
// Fold the two lane halves (same row i, complementary column sets) and write the split's partials
// part[4][nsplit][N]. POS: the positive-logit sum and count planes carry ps / pc, else zeros.
template <bool POS>
__device__ __forceinline__ void fold_store_partials(float* part, int nsplit, int split, int64_t N, int64_t i,
                                                    bool row_ok, int h, float m, float l, float ps, float pc) {
  const float m2 = __shfl_xor(m, 32, 64);
  const float l2 = __shfl_xor(l, 32, 64);
  const float ps2 = POS ? __shfl_xor(ps, 32, 64) : 0.0f;
  const float pc2 = POS ? __shfl_xor(pc, 32, 64) : 0.0f;
  const float mm = fmaxf(m, m2);
  float ll = 0.0f;
  if (mm != -INFINITY) {
    if (m != -INFINITY) ll += l * __expf(m - mm);
    if (m2 != -INFINITY) ll += l2 * __expf(m2 - mm);
  }
  if (h == 0 && row_ok) {
    const int64_t stride = (int64_t)nsplit * N;
    const int64_t o = (int64_t)split * N + i;
    part[o] = mm;
    part[stride + o] = ll;
    part[2 * stride + o] = POS ? ps + ps2 : 0.0f;
    part[3 * stride + o] = POS ? pc + pc2 : 0.0f;
  }
}

// One wave's 32 x 128 gradient tile to its owner rows: D[own_base + tile_row(r,h)][32kb + c] =
// gacc[kb][r], times scale where SCALED (the fp16 kernels' operand scales)
template <bool SCALED = false>
__device__ __forceinline__ void store_d_own(int64_t own_base, float* dst, int64_t n_own, int h, int c,
                                            const f32x16 (&gacc)[4], float scale = 1.0f) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = own_base + tile_row(r, h);
    if (orow < n_own) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) dst[orow * kD + kb * 32 + c] = SCALED ? gacc[kb][r] * scale : gacc[kb][r];
    }
  }
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline bool valid_flags(int f) {
  // supported combinations (see header)
  return f == 0 || f == F_MASK_K1 || f == (F_MASK_K1 | F_MASK_K2) || f == (F_EXCL_DIAG | F_POS) ||
         f == (F_MASK_K1 | F_DIAG_NOBIAS);
}

// fn(std::integral_constant<int, FL>) for the kernel instantiation FL of a valid flag combination
template <typename Fn>
void with_flags(int flags, Fn&& fn) {
  switch (flags) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case F_MASK_K1: fn(std::integral_constant<int, F_MASK_K1>{}); break;
    case F_MASK_K1 | F_MASK_K2: fn(std::integral_constant<int, F_MASK_K1 | F_MASK_K2>{}); break;
    case F_MASK_K1 | F_DIAG_NOBIAS: fn(std::integral_constant<int, F_MASK_K1 | F_DIAG_NOBIAS>{}); break;
    default: fn(std::integral_constant<int, F_EXCL_DIAG | F_POS>{}); break;
  }
}

// =====================================================================================
// Grouped form of the live LogQ loss (v1_refine_usertower.py:826-861).
// The logit S_ij depends on column j only through its target t_j, so the N x N problem is
// evaluated over the D distinct targets of the batch with exact integer multiplicities:
//   w_{i,d} = 1                         if d == d(i) (the row's own target: only j == i survives
//                                       the same-item mask)
//           = c_d - n_{u_i,d}           otherwise (c_d: columns with target d, n_{u,d}: those
//                                       belonging to row i's user, removed by the same-user mask)
//   LSE_i = log sum_d w_{i,d} exp(x_{i,d}),  x_{i,d} = <A_i,B_d>/tau - bias_d
// This is the same sum as the reference's (only the summation order differs); FLOPs drop by
// N / D (4.7x on Zipf(1.0) H&M-shaped batches). The user's own targets are the sparse
// exceptions, walked with a monotone pointer per lane.
struct GArgs {
  const float* A;        // [N, lda] rows (normalised user steps)
  const float* B;        // [D, ldb] distinct target rows (normalised item vectors)
  const float* bias;     // [D] logQ * lambda (nullable)
  const float* colcnt;   // [D] c_d
  const int* row_col;    // [N] d(i)
  const int* row_beg;    // [N] row exception list range [row_beg, row_end) in exc_cols
  const int* row_end;
  const int* exc_cols;   // sorted d values of the row's user's targets (with repeats)
  const int* col_beg;    // [D] column exception list range into exc_s/exc_e/exc_n
  const int* col_end;
  const int* exc_s;      // user row range [s, e) and multiplicity n_{u,d}, sorted by s
  const int* exc_e;
  const int* exc_n;
  int64_t N, M, lda, ldb;
  float inv_tau;
  int nsplit;
  int64_t span;          // streamed rows per split
  float* part;           // fwd: [4][nsplit][N]
  const float* lse;      // bwd
  const float* row_loss; // bwd, f16 column pass: lse_i - s_ii of the forward's merge (fp32 label logit)
  const float* gout;     // bwd: gradient of the row-loss sum
  float* dout;           // bwd: [nsplit][owner][128]
  const __bf16* ahi;     // bf16x3: hi/lo images of A [N][128] and B [M][128]
  const __bf16* alo;
  const __bf16* bhi;
  const __bf16* blo;
  // fused forward, two-region geometry (fwdg_schedule / fwdg_block): row blocks [0, rb1) run nsplit
  // splits of span columns, the rest nsplit2 splits of span2; partial slots per row: nslots
  int64_t rb1, span2;
  int nsplit2, nslots;
  int split_major;       // grouped backward: split-major block order (nce_grouped_bwd_x3_k)
};

__device__ __forceinline__ int lower_bound_i(const int* a, int lo, int hi, int64_t key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Block geometry of the fused forwards (nce_grouped_fwdg_x3p_k, nce_grouped_fwdg_h_k): the one place
// that turns a block index into (row block, split, column range). Row blocks [0, rb1) run nsplit
// column splits of span columns, the rest nsplit2 splits of span2 (their workgroups are shorter
// and are dispatched last, so the final round of the grid is filled by short workgroups instead of
// part of the chip running long ones). Both counts are 1, 2, 4 or a multiple of 8, and each region
// keeps the XCD-aware remap of remap_block: rb1 * nsplit is a multiple of 8 (fwdg_schedule), so in
// the tail region b & 7 still names the XCD group.
__host__ __device__ __forceinline__ void fwdg_block(int64_t b, int nsplit, int64_t span, int64_t rb1, int nsplit2,
                                                    int64_t span2, int64_t M, int& split, int64_t& rb,
                                                    int64_t& j_begin, int64_t& j_end) {
  const int64_t n1 = rb1 * nsplit;
  if (b < n1) {
    remap_block<int64_t>(b, nsplit, split, rb);
  } else {
    remap_block<int64_t>(b - n1, nsplit2, split, rb);
    rb += rb1;
    span = span2;
  }
  j_begin = (int64_t)split * span;
  j_end = j_begin + span;
  if (j_end > M) j_end = M;
}
__device__ __forceinline__ void fwdg_geometry(const GArgs& a, int& split, int64_t& rb, int64_t& j_begin,
                                              int64_t& j_end) {
  fwdg_block(blockIdx.x, a.nsplit, a.span, a.rb1, a.nsplit2, a.span2, a.M, split, rb, j_begin, j_end);
}

// streamed rows (or columns) per split: whole tiles, at least one
inline int64_t split_span(int64_t n_str, int nsplit) {
  const int64_t s = round_up((n_str + nsplit - 1) / nsplit, kTile);
  return s < kTile ? kTile : s;
}

// Grid of the fused forward for the caller's slot count nsplit, over slots = 2 x CUs co-resident
// workgroups (two 256-VGPR workgroups per CU). A pure function of (N, D, slots): no atomics, no
// work claiming, so a step is bit-reproducible.
//   nsplit 4: every row block runs 4 splits; nsplit 8: the leading row blocks, as many as fill
//     whole rounds, run 4 splits and the rest 8 (the plain-family view's geometry).
//   nsplit 1, 2 (rounds model; slots rounded down to whole XCD groups of 8): the first
//     rb1 = floor(rbs / slots) * slots row blocks run as
//     whole-row workgroups (one split over all D columns, one partial slot: whole rounds of equal
//     workgroups have no tail), the remaining t < slots row blocks run ns2 splits, ns2 in
//     {1, 2, 4, 8} minimising the tail's makespan ceil(t ns2 / slots) / ns2 row sweeps (ties: the
//     smaller ns2, less partial traffic). With 2 splits everywhere the makespan was
//     ceil(2 rbs / slots) / 2 sweeps; ns2 = 2 is a candidate, so the model never gets worse.
//     Batch 8192 (rbs 1,197, slots 512): 1,024 whole-row blocks, then 173 x 8: 2 + 3/8 = 2.375
//     sweeps against 2.5; batch 4096 (601): 512, then 89 x 4: 1.25 against 1.5.
// nslots: partial slots per row (the stride of part and of the row-gradient partials).
struct FwdgSchedule {
  int64_t rb1;   // leading row blocks
  int ns1, ns2;  // splits of the leading / tail row blocks
  int nslots;
  int64_t span1, span2, blocks;
};
inline FwdgSchedule fwdg_schedule(int64_t N, int64_t D, int nsplit, int64_t slots) {
  const int64_t rbs = (N + kOwnRows - 1) / kOwnRows;
  FwdgSchedule s;
  if (slots < 8) slots = 8;
  if (nsplit == 4) {
    s.rb1 = rbs; s.ns1 = 4; s.ns2 = 8; s.nslots = 4;
  } else if (nsplit == 8) {
    s.ns1 = 4; s.ns2 = 8; s.nslots = 8;
    s.rb1 = (4 * rbs / slots) * slots / 4;  // whole rounds of the 4-split blocks
  } else {
    s.ns1 = 1;
    slots -= slots % 8;  // whole XCD groups: the tail region starts where b & 7 == 0
    s.rb1 = rbs / slots * slots;
    const int64_t t = rbs - s.rb1;
    s.ns2 = 1;
    int64_t best = (t + slots - 1) / slots;  // rounds / ns2, compared as fractions
    for (int c = 2; c <= 8; c *= 2) {
      const int64_t r = (t * c + slots - 1) / slots;
      if (r * s.ns2 < best * c) { best = r; s.ns2 = c; }
    }
    s.nslots = t > 0 ? s.ns2 : 1;
  }
  s.span1 = split_span(D, s.ns1);
  s.span2 = split_span(D, s.ns2);
  s.blocks = s.rb1 * s.ns1 + (rbs - s.rb1) * s.ns2;
  return s;
}

// split count of one pass of the plain bf16x3 kernels: the smallest power of two (<= 64) that gives
// the owner side >= 1024 workgroups while every split keeps >= 2 streamed tiles
inline int plain_split(int64_t n_own, int64_t n_str) {
  const int64_t ob = (n_own + kOwnRows - 1) / kOwnRows;
  // workgroup target: one round of two workgroups per CU (512 on MI355X) measured 8 % faster than
  // 1024 over the DuoRec + SupCon passes at B = 8192 (tools/nce_plain_micro.py: 0.763 vs 0.830 ms;
  // 256: 1.05, 2048: 0.93).
  const int64_t target = 2 * rsx::cu_count();
  int ps = 1;
  while (ps < 64 && ob * ps < target && n_str >= (int64_t)ps * 4 * kTile) ps *= 2;
  return ps;
}

// ---- workspace layouts: float offsets into ws, and the total *_workspace_floats returns ----
// Every family starts with part [4][nf][N] | lse [N] | row_loss [N] | row_valid [N] | inv_cnt [N];
// then come the backward's split partials (dpart, room for dpart_cap floats) and the hi/lo
// 16-bit images of A and B (img: ahi [N][128] | alo | bhi [M][128] | blo, two per float).
struct StatsLayout {
  int nf;  // forward splits
  int64_t part = 0, lse, row_loss, row_valid, inv_cnt, stats_end;
  StatsLayout(int64_t N, int nf_)
      : nf(nf_), lse(4 * (int64_t)nf_ * N), row_loss(lse + N), row_valid(row_loss + N), inv_cnt(row_valid + N),
        stats_end(inv_cnt + N) {}
};
// plain fp32: stats | dpart [nsplit_bwd][max(N, M)][128] | 16
struct PlainLayout : StatsLayout {
  int64_t dpart, dpart_cap, total;
  PlainLayout(int64_t N, int64_t M, int nsplit_fwd, int nsplit_bwd)
      : StatsLayout(N, nsplit_fwd), dpart(stats_end), dpart_cap((int64_t)nsplit_bwd * std::max(N, M) * kD),
        total(dpart + dpart_cap + 16) {}
};
// plain bf16x3: stats | (64-float aligned) img | dpart [max(pr N, pc M)][128] | 16; the splits of
// the forward (nf), the row pass (pr) and the column pass (pc) come from plain_split
struct PlainX3Layout : StatsLayout {
  int pr, pc;
  int64_t img, dpart, dpart_cap, total;
  PlainX3Layout(int64_t N, int64_t M)
      : StatsLayout(N, plain_split(N, M)), pr(plain_split(N, M)), pc(plain_split(M, N)), img(round_up(stats_end, 64)),
        dpart(img + (N + M) * kD), dpart_cap(std::max((int64_t)pr * N, (int64_t)pc * M) * kD),
        total(dpart + dpart_cap + 16) {}
};
// grouped: the plain fp32 layout over (N, D), then (bf16x3, f16: 64-float aligned) img | 64. The
// fused forward's per-slot row gradients (nslots x N x 128) and the column pass's up to 32 splits
// also live in dpart: both are checked against dpart_cap where they are chosen.
// The fused forward called with 1 or 2 slots gives its tail rows up to 8 (fwdg_schedule), more than
// the stats region's part [4][nf][N] holds, and the totals are fixed (callers size their buffers
// with them): its partial stats [4][nslots][N] (<= 32 N floats) go to the head of A's image region
// (fwd_part = img, N x 128 floats), which is idle between the calls: the forward streams B's
// images and reads A itself, and A's images are written by the backward's column pass, after the
// merge has consumed the partials. lse / row_loss / row_valid stay where StatsLayout puts them.
struct GroupedLayout : PlainLayout {
  int64_t img, total;
  int64_t fwd_part(int nsplit_fwd) const { return nsplit_fwd <= 2 ? img : part; }
  GroupedLayout(int64_t N, int64_t D, int nsplit_fwd, int precision, int nsplit_bwd = kNsplitBwdGrouped)
      : PlainLayout(N, D, nsplit_fwd, nsplit_bwd), img(round_up(PlainLayout::total, 64)),
        total(img + (precision != RSX_NCE_FP32 ? (N + D) * kD + 64 : 0)) {}
};

// Plain-family view of the grouped kernels (rsx_nce_fwd_grad / rsx_nce_bwd_cols): the plain N x M
// problem as a grouped one with trivial groups. D = M, every column distinct with multiplicity 1;
// row i's one exception is its diagonal column i + off, column j's one exception the row j - off.
// The weight rule c - n = 0 then excludes the diagonal and the label rule keeps it at weight 1.
// The arrays depend on (N, M, off) only; 5 N + 3 M ints:
//   lab [N] = i + off (row_col of flags 0, and every row's exception list exc_cols)
//   none [N] = -1     (row_col of flags 9: no label column)
//   beg [N] = i, end [N] = i + 1  (row_beg / row_end, and the columns' row ranges exc_s / exc_e)
//   one [N] = 1       (exc_n)
//   col_beg [M], col_end [M]: [j - off, j - off + 1) where 0 <= j - off < N, else empty
//   colcnt [M] = 1.0f (float bits)
struct ViewLayout {
  int64_t lab = 0, none, beg, end, one, col_beg, col_end, colcnt, total;
  ViewLayout(int64_t N, int64_t M)
      : none(N), beg(2 * N), end(3 * N), one(4 * N), col_beg(5 * N), col_end(5 * N + M), colcnt(5 * N + 2 * M),
        total(5 * N + 3 * M) {}
};
// entry k of the view (host and device: the device fill and the host fill of the CPU tests share it)
__host__ __device__ inline int view_entry(int64_t k, int64_t N, int64_t M, int64_t off) {
  if (k < 5 * N) {
    const int64_t a = k / N, i = k % N;
    return a == 0 ? (int)(i + off) : a == 1 ? -1 : a == 2 ? (int)i : a == 3 ? (int)(i + 1) : 1;
  }
  k -= 5 * N;
  const int64_t a = k / M, r = k % M - off;
  if (a == 2) return 0x3f800000;  // 1.0f
  if (r < 0 || r >= N) return 0;
  return a == 0 ? (int)r : (int)(r + 1);
}
// fused plain view (bf16x3 products only, see rsx_nce_fwd_grad): the grouped layout over (N, M) with
// 8 forward slots and 8 column-pass splits, then SupCon's positive term: cnt [N] | ps [N] | P [N][128]
constexpr int kNsplitFused = 8;
struct FusedLayout : GroupedLayout {
  int64_t pos_cnt, pos_ps, pos_P, total;
  FusedLayout(int64_t N, int64_t M)
      : GroupedLayout(N, M, kNsplitFused, RSX_NCE_BF16X3, kNsplitFused), pos_cnt(round_up(GroupedLayout::total, 4)),
        pos_ps(pos_cnt + N), pos_P(round_up(pos_ps + N, 4)), total(pos_P + N * kD + 16) {}
};

struct Images {
  __bf16 *ahi, *alo, *bhi, *blo;
};
inline Images images_at(float* ws, int64_t img, int64_t N, int64_t M) {
  __bf16* p = reinterpret_cast<__bf16*>(ws + img);
  return {p, p + N * kD, p + 2 * N * kD, p + 2 * N * kD + M * kD};
}

// ---- argument checks shared by the entry points: nullptr, or the message for RSX_ARG ----
inline const char* operand_error(const float* A, const float* B, int64_t lda, int64_t ldb) {
  if (!(lda % 4 == 0 && ldb % 4 == 0 && lda >= kD && ldb >= kD)) return "row strides must be >=128 and multiples of 4";
  if (((uintptr_t)A % 16) != 0 || ((uintptr_t)B % 16) != 0) return "A/B must be 16-byte aligned";
  return nullptr;
}
inline const char* diag_error(int64_t N, int64_t M, int64_t diag_offset) {
  if (!(diag_offset >= 0 && diag_offset + N <= M)) return "need 0 <= diag_offset and diag_offset + N <= M";
  return nullptr;
}
#define NCE_REQUIRE(err)           \
  do {                             \
    const char* m_ = (err);        \
    RSX_ARG(m_ == nullptr, m_);    \
  } while (0)

// the forwards' N == 0 case: out2 = {0, 0}
inline int zero_sums(float* out2, hipStream_t st) {
  (void)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
  RSX_LAUNCHED();
  return 0;
}

// ---- host launchers that cross files; the kernels are defined once: in nce_plain.hip ...
void launch_reduce(const float* row_loss, const float* row_valid, int64_t N, float* out2, hipStream_t st);
void launch_sum_splits(const float* part, int nsplit, int64_t n_own, float* out, int accumulate, hipStream_t st);
// rows x 128 fp32 -> hi/lo images: bf16 (half = false) or the fp16 images of RSX_NCE_F16
void launch_split(const float* src, int64_t ld, int64_t rows, __bf16* hi, __bf16* lo, bool half, hipStream_t st);
// ... and in nce_grouped_f16.hip
void launch_grouped_fwdg_h(const GArgs& g, int blocks, hipStream_t st);
void launch_grouped_bwd_cols_h(const GArgs& g, int blocks, hipStream_t st);

}  // namespace nce
}  // namespace rsx
