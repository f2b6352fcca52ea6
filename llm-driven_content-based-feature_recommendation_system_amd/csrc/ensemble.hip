// Late-fusion evaluation of two retrievers on the device (tower_code/mined_inference.py): exact top-k
// of materialised score rows for k up to 2048, the fusion of two retrievers over a per-user candidate
// pool with its alpha sweep and hit bits, and the first hit of a ranked list.
// Reference: tower_code/mined_inference.py, evaluate_weighted_score_ensemble (:1103-1189),
// evaluate_rrf_ensemble (:1330-1410) and evaluate_multi_vector_ensemble (:901-953): two torch.topk over
// [B, N_items], a [B, 2 pool, D] gather, a torch.topk and a device-to-host copy per alpha, and Python
// loops over the users with np.unique.
//
//   select_topk_k  one workgroup per row; a thread loads 16 row elements before it uses the first (a
//                  row pass is bound by the loads in flight). The k-th largest key by a radix select,
//                  four 8-bit passes from the top byte down over per-wave LDS histograms (a wave adds one count per
//                  distinct byte it holds, so equal bytes do not serialise); then the waves, each over
//                  its own contiguous part of the row, count the keys equal to the k-th, and collect
//                  every larger key plus the equal keys whose rank among the equal ones (in index
//                  order) is below the number still needed; then a bitonic sort of the k pairs
//                  (key, ~index) in LDS. The pairs are distinct, so the order of the collecting
//                  atomics does not reach the output.
//   fuse_rank_k    one workgroup per user: both dot products of every pool entry (16 lanes per entry),
//                  the per-list normalisation (min-max, or ranks from a sort), once per user the
//                  entries' duplicate groups (a sort by id) and truth flags (binary search), then per
//                  alpha a sort of (key(f), ~position), the first `cut` entries, the first occurrence
//                  of each id among them (an LDS atomicMin per duplicate group: a minimum, the same
//                  whatever the arrival order), their ranks by a workgroup scan, the hit bits and
//                  the list.
//   first_hit_k    one workgroup per list: the smallest position whose id is in the user's truth.
//
// The fp32 expressions of the fusion are written to be reproduced bit for bit on the host: contraction
// is off in this file, and only the dot products, whose summation order is free, use explicit FMAs.
#include "rsx_block.h"
#include "rsx_common.h"
#include "rsx_x3.h"
#include "recsys_amd.h"
#include <string.h>

#pragma clang fp contract(off)

namespace {

using rsx::score_key;
using rsx::bitonic_sort_desc, rsx::block_scan_excl, rsx::digit_search_desc, rsx::pow2_at_least;
typedef unsigned long long u64;

constexpr int kMaxK = 2048;      // rsx_select_topk_rows: largest k
constexpr int kMaxC = 2048;      // rsx_fuse_rank: largest pool
constexpr int kMaxAlpha = 32, kMaxKs = 16;
constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64;
constexpr int kSelLoads = 16;  // row elements a thread loads before it uses the first: 64 KB in flight per workgroup
constexpr int kFuseThreads = 256, kFusePer = kMaxC / kFuseThreads;  // entries of the cut per thread
constexpr int kHitThreads = 256;
constexpr int kNone = 0x7fffffff;

// (key, position) as one sortable word: larger key first, then the lower position. A real pair is
// never 0 (position < 2^31), so 0 pads a sort to a power of two and sorts last.
__device__ __forceinline__ u64 pair_of(unsigned key, int pos) { return (u64)key << 32 | (u64)(0xffffffffu - (unsigned)pos); }
__device__ __forceinline__ int pair_pos(u64 p) { return (int)(0xffffffffu - (unsigned)(p & 0xffffffffull)); }
__device__ __forceinline__ unsigned pair_key(u64 p) { return (unsigned)(p >> 32); }

// Is id among the ascending, distinct t[lo, hi)?
__device__ __forceinline__ bool in_truth(const int32_t* __restrict__ t, int64_t lo, int64_t hi, int id) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int v = t[mid];
    if (v == id) return true;
    if (v < id) lo = mid + 1; else hi = mid;
  }
  return false;
}

// The user's slice of the truth, clamped into [0, n_truth] so that no offset leads outside the array.
__device__ __forceinline__ void truth_range(const int64_t* __restrict__ off, int64_t q, int64_t n_truth, int64_t& lo,
                                            int64_t& hi) {
  lo = off[q];
  hi = off[q + 1];
  lo = lo < 0 ? 0 : (lo > n_truth ? n_truth : lo);
  hi = hi < lo ? lo : (hi > n_truth ? n_truth : hi);
}

// ---- rsx_select_topk_rows ---------------------------------------------------------------------------
// One count per distinct byte held by the wave's lanes that are `on`, into the wave's own histogram.
// Every lane of the wave calls it (the loop is wave-uniform).
__device__ __forceinline__ void hist_add(unsigned* h, unsigned bin, bool on, int lane) {
  u64 todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned b = (unsigned)__shfl((int)bin, leader, 64);
    const u64 same = __ballot(on && bin == b);
    if (lane == leader) atomicAdd(&h[b], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(kSelThreads) void select_topk_k(const float* __restrict__ S, int64_t ld, int N, int k,
                                                              int32_t* __restrict__ idx, float* __restrict__ val) {
  __shared__ unsigned hist[kSelWaves][256];
  __shared__ u64 buf[kMaxK];
  __shared__ unsigned sPrefix, sNeed;
  __shared__ int sTies[kSelWaves];
  __shared__ int sCount;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* __restrict__ row = S + (int64_t)blockIdx.x * ld;
  const int P = pow2_at_least(k);
  for (int j = k + tid; j < P; j += kSelThreads) buf[j] = 0ull;
  if (tid == 0) sCount = 0;

  // the k-th largest key: `prefix` holds its bytes found so far, `need` how many keys with that prefix
  // are still wanted (the keys above the prefix are all taken)
  unsigned prefix = 0u, need = (unsigned)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int j = tid; j < kSelWaves * 256; j += kSelThreads) (&hist[0][0])[j] = 0u;
    __syncthreads();
    for (int base = 0; base < N; base += kSelThreads * kSelLoads) {  // wave-uniform: hist_add needs whole waves
      float v[kSelLoads];
#pragma unroll
      for (int u = 0; u < kSelLoads; ++u) {
        const int i = base + u * kSelThreads + tid;
        v[u] = i < N ? row[i] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kSelLoads; ++u) {
        const int i = base + u * kSelThreads + tid;
        const unsigned key = score_key(v[u]);
        hist_add(hist[w], (key >> shift) & 255u, i < N && (key & himask) == prefix, lane);
      }
    }
    __syncthreads();
    if (w == 0) {  // the prefix holds >= need keys, so one lane finds the byte
      int byte;
      unsigned above;
      const auto count = [&](int b) {
        unsigned c = 0u;
#pragma unroll
        for (int q = 0; q < kSelWaves; ++q) c += hist[q][b];
        return c;
      };
      if (digit_search_desc(count, need, lane, byte, above)) {
        sPrefix = prefix | ((unsigned)byte << shift);
        sNeed = need - above;
      }
    }
    __syncthreads();
    prefix = sPrefix;
    need = sNeed;
  }
  const unsigned kth = prefix;
  const int above = k - (int)need;  // keys larger than the k-th: all taken

  // wave w owns the row's part [w span, (w + 1) span): the equal keys are ranked in index order
  const int span = ((N + kSelWaves - 1) / kSelWaves + 63) / 64 * 64;  // N <= 2^30: no overflow
  const int beg = w * span < N ? w * span : N, end = beg + span < N ? beg + span : N;
  int ties = 0;
  for (int base = beg; base < end; base += 64 * kSelLoads) {
    float v[kSelLoads];
#pragma unroll
    for (int u = 0; u < kSelLoads; ++u) {
      const int i = base + u * 64 + lane;
      v[u] = i < end ? row[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kSelLoads; ++u) {
      const int i = base + u * 64 + lane;
      ties += __popcll(__ballot(i < end && score_key(v[u]) == kth));
    }
  }
  if (lane == 0) sTies[w] = ties;
  __syncthreads();
  int run = 0;
  for (int q = 0; q < w; ++q) run += sTies[q];
  const u64 below = lane == 0 ? 0ull : (~0ull >> (64 - lane));  // the lanes before this one
  for (int base = beg; base < end; base += 64 * kSelLoads) {
    float v[kSelLoads];
#pragma unroll
    for (int u = 0; u < kSelLoads; ++u) {
      const int i = base + u * 64 + lane;
      v[u] = i < end ? row[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kSelLoads; ++u) {  // in index order
      const int i = base + u * 64 + lane;
      const unsigned key = score_key(v[u]);
      if (i < end && key > kth) {
        const int slot = atomicAdd(&sCount, 1);  // `above` of them in the row
        if (slot < above) buf[slot] = pair_of(key, i);
      }
      const bool eq = i < end && key == kth;
      const u64 m = __ballot(eq);
      const int r = run + __popcll(m & below);
      if (eq && r < (int)need) buf[above + r] = pair_of(key, i);
      run += __popcll(m);
    }
  }
  bitonic_sort_desc<kSelThreads>(buf, P);
  int32_t* __restrict__ oi = idx + (int64_t)blockIdx.x * k;
  float* __restrict__ ov = val + (int64_t)blockIdx.x * k;
  for (int j = tid; j < k; j += kSelThreads) {
    const int i = pair_pos(buf[j]);  // < N: slots [0, k) hold collected pairs only
    oi[j] = i;
    ov[j] = row[i];
  }
}

// ---- rsx_fuse_rank ------------------------------------------------------------------------------------
struct FuseConsts {
  float wa[kMaxAlpha], wb[kMaxAlpha];
  int ks[kMaxKs];
  int A, nK, cut, mode;
  float k_rrf;
};

struct FuseArgs {
  const float *ua, *Ia, *ub, *Ib;
  int64_t ldua, ldia, ldub, ldib;
  int Da, Db;
  int64_t NI;
  const int32_t* cand;
  int C;
  const int64_t* truth_off;
  const int32_t* truth;
  int64_t n_truth;
  int32_t *hits, *lists;
  float *sa, *sb;
  int32_t* flag;
};

// min and max of v[0, C) over the workgroup (C >= 1); sm holds 2 NT / 64 floats.
template <int NT>
__device__ __forceinline__ void block_min_max(const float* v, int C, float* sm, float& mn, float& mx) {
  float a = v[0], b = v[0];
  for (int c = threadIdx.x; c < C; c += NT) {
    const float x = v[c];
    a = x < a ? x : a;
    b = x > b ? x : b;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a2 = __shfl_xor(a, o, 64), b2 = __shfl_xor(b, o, 64);
    a = a2 < a ? a2 : a;
    b = b2 > b ? b2 : b;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[2 * w] = a, sm[2 * w + 1] = b;
  __syncthreads();
  mn = sm[0], mx = sm[1];
#pragma unroll
  for (int q = 1; q < NT / 64; ++q) {
    mn = sm[2 * q] < mn ? sm[2 * q] : mn;
    mx = sm[2 * q + 1] > mx ? sm[2 * q + 1] : mx;
  }
  __syncthreads();
}

// The list's normalisation in place: v[c] = (v[c] - min) / ((max - min) + 1e-9f), or
// 1 / ((k_rrf + rank) + 1) with the rank from a sort of (key, ~position).
template <int NT>
__device__ __forceinline__ void normalise(float* v, int C, int P, int mode, float k_rrf, u64* sortbuf, float* smf) {
  if (mode == RSX_FUSE_MINMAX) {
    float mn, mx;
    block_min_max<NT>(v, C, smf, mn, mx);
    const float den = (mx - mn) + 1e-9f;
    for (int c = threadIdx.x; c < C; c += NT) v[c] = __fdiv_rn(v[c] - mn, den);
  } else {
    for (int c = threadIdx.x; c < P; c += NT) sortbuf[c] = c < C ? pair_of(score_key(v[c]), c) : 0ull;
    bitonic_sort_desc<NT>(sortbuf, P);
    for (int r = threadIdx.x; r < C; r += NT) v[pair_pos(sortbuf[r])] = __fdiv_rn(1.0f, (k_rrf + (float)r) + 1.0f);
  }
  __syncthreads();
}

__device__ __forceinline__ float dot4(const float4& x, const float4& y, float acc) {
  acc = __builtin_fmaf(x.x, y.x, acc);
  acc = __builtin_fmaf(x.y, y.y, acc);
  acc = __builtin_fmaf(x.z, y.z, acc);
  return __builtin_fmaf(x.w, y.w, acc);
}

__global__ __launch_bounds__(kFuseThreads) void fuse_rank_k(FuseArgs g, FuseConsts k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int smi[kFuseThreads / 64];
  __shared__ float smf[2 * kFuseThreads / 64];
  __shared__ int sHit;
  constexpr int NT = kFuseThreads;
  const int tid = threadIdx.x, C = g.C, P = pow2_at_least(C);
  const int64_t q = blockIdx.x;
  u64* sortbuf = reinterpret_cast<u64*>(smem);                     // [P]
  float* na = reinterpret_cast<float*>(sortbuf + P);               // [P]
  float* nb = na + P;                                              // [P]
  int* cid = reinterpret_cast<int*>(nb + P);                       // [P] corpus id of the entry
  int* first = cid + P;                                            // [P] per duplicate group: its first place in the order
  unsigned short* grp = reinterpret_cast<unsigned short*>(first + P);  // [P] group (its lowest position) | truth << 15

  bool bad = false;
  for (int c = tid; c < C; c += NT) {
    const int id = g.cand[q * C + c];
    if (id < 0 || (int64_t)id >= g.NI) bad = true;
    cid[c] = id;
  }
  if (bad) atomicOr(g.flag, 1);  // only on input that the caller rejects
  __syncthreads();

  // 1. the scores: 16 lanes per entry, lane s the columns 4s ... 4s + 3 (and 64 more at D = 128)
  {
    const int grp16 = tid >> 4, s = tid & 15;
    const float* __restrict__ uaq = g.ua + q * g.ldua;
    const float* __restrict__ ubq = g.ub + q * g.ldub;
    float4 ua4[2], ub4[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ua4[h] = 4 * s + 64 * h < g.Da ? *reinterpret_cast<const float4*>(uaq + 4 * s + 64 * h) : float4{0.f, 0.f, 0.f, 0.f};
      ub4[h] = 4 * s + 64 * h < g.Db ? *reinterpret_cast<const float4*>(ubq + 4 * s + 64 * h) : float4{0.f, 0.f, 0.f, 0.f};
    }
    for (int c0 = 0; c0 < C; c0 += NT / 16) {
      const int c = c0 + grp16;
      float pa = 0.0f, pb = 0.0f;
      if (c < C) {
        const int id = cid[c];
        if (id >= 0 && (int64_t)id < g.NI) {  // an id outside the corpus scores 0 (and has set the flag)
          const float* __restrict__ ra = g.Ia + (int64_t)id * g.ldia;
          const float* __restrict__ rb = g.Ib + (int64_t)id * g.ldib;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (4 * s + 64 * h < g.Da) pa = dot4(ua4[h], *reinterpret_cast<const float4*>(ra + 4 * s + 64 * h), pa);
            if (4 * s + 64 * h < g.Db) pb = dot4(ub4[h], *reinterpret_cast<const float4*>(rb + 4 * s + 64 * h), pb);
          }
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        pa += __shfl_xor(pa, o, 64);
        pb += __shfl_xor(pb, o, 64);
      }
      if (s == 0 && c < C) {
        na[c] = pa;
        nb[c] = pb;
        if (g.sa) g.sa[q * C + c] = pa;
        if (g.sb) g.sb[q * C + c] = pb;
      }
    }
  }
  __syncthreads();

  // 2./3. per-list normalisation
  normalise<NT>(na, C, P, k.mode, k.k_rrf, sortbuf, smf);
  normalise<NT>(nb, C, P, k.mode, k.k_rrf, sortbuf, smf);

  // once per user: the entries sorted by (id, position); a group of equal ids is named by its lowest
  // position, found by walking back to the group's head (groups are pairs in a two-retriever pool; a
  // pool of one repeated id walks C steps)
  {
    int64_t tlo, thi;
    truth_range(g.truth_off, q, g.n_truth, tlo, thi);
    for (int c = tid; c < P; c += NT) sortbuf[c] = c < C ? pair_of((unsigned)cid[c], c) : 0ull;
    bitonic_sort_desc<NT>(sortbuf, P);
    for (int s = tid; s < C; s += NT) {
      const u64 e = sortbuf[s];
      const unsigned id = pair_key(e);
      int h = s;
      while (h > 0 && pair_key(sortbuf[h - 1]) == id) --h;
      const unsigned hit = in_truth(g.truth, tlo, thi, (int)id) ? 0x8000u : 0u;
      grp[pair_pos(e)] = (unsigned short)((unsigned)pair_pos(sortbuf[h]) | hit);
    }
    __syncthreads();
  }

  const int cut = k.cut, kmax = k.ks[k.nK - 1];
  for (int a = 0; a < k.A; ++a) {
    const float wa = k.wa[a], wb = k.wb[a];
    // 4./5. f = wa na + wb nb (two roundings, then one) and the order by (key(f), position)
    for (int c = tid; c < P; c += NT) {
      sortbuf[c] = c < C ? pair_of(score_key(wa * na[c] + wb * nb[c]), c) : 0ull;
      first[c] = kNone;
    }
    if (tid == 0) sHit = kNone;
    bitonic_sort_desc<NT>(sortbuf, P);
    // 6.-8. the first `cut` entries; an entry is kept when it is its id's first in the order
    int pos[kFusePer];
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      const int j = tid * kFusePer + e;
      pos[e] = j < cut ? pair_pos(sortbuf[j]) : -1;
      if (j < cut) atomicMin(&first[grp[pos[e]] & 0x7fffu], j);
    }
    __syncthreads();
    int cnt = 0;
    unsigned keep = 0u;
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      const int j = tid * kFusePer + e;
      if (j < cut && first[grp[pos[e]] & 0x7fffu] == j) {
        keep |= 1u << e;
        ++cnt;
      }
    }
    int total;
    int rank = block_scan_excl<NT>(cnt, rsx::Sum(), 0, smi, total);
    // 9. the rank of the first kept entry that is in the truth decides every hit@k
    int32_t* __restrict__ lst = g.lists ? g.lists + (q * k.A + a) * (int64_t)kmax : nullptr;
#pragma unroll
    for (int e = 0; e < kFusePer; ++e) {
      if (keep >> e & 1u) {
        if (lst && rank < kmax) lst[rank] = cid[pos[e]];
        if (grp[pos[e]] & 0x8000u) atomicMin(&sHit, rank);
        ++rank;
      }
    }
    if (lst)
      for (int j = total + tid; j < kmax; j += NT) lst[j] = -1;
    __syncthreads();
    if (tid == 0) {
      int bits = 0;
      for (int j = 0; j < k.nK; ++j)
        if (sHit < k.ks[j]) bits |= 1 << j;
      g.hits[q * k.A + a] = bits;
    }
    __syncthreads();
  }
}

// ---- rsx_first_hit -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHitThreads) void first_hit_k(const int32_t* __restrict__ lists, int64_t ld, int K,
                                                            const int64_t* __restrict__ truth_off,
                                                            const int32_t* __restrict__ truth, int64_t n_truth,
                                                            int32_t* __restrict__ out) {
  __shared__ int sBest;
  const int64_t q = blockIdx.x;
  if (threadIdx.x == 0) sBest = K;
  __syncthreads();
  int64_t lo, hi;
  truth_range(truth_off, q, n_truth, lo, hi);
  int best = K;
  for (int j = threadIdx.x; j < K && best == K; j += kHitThreads)
    if (in_truth(truth, lo, hi, lists[q * ld + j])) best = j;
  if (best < K) atomicMin(&sBest, best);
  __syncthreads();
  if (threadIdx.x == 0) out[q] = sBest;
}

size_t fuse_lds_bytes(int C) {
  return (size_t)pow2_at_least(C) * (8 + 4 + 4 + 4 + 4 + 2);
}

}  // namespace

RSX_API int rsx_select_topk_rows(const float* S, int64_t ld, int64_t Q, int64_t N, int64_t k, int32_t* idx,
                                 float* val, void* stream) {
  RSX_ARG(N >= 1 && N <= ((int64_t)1 << 30), "need 1 <= N <= 2^30");
  RSX_ARG(k >= 1 && k <= kMaxK && k <= N, "need 1 <= k <= min(N, 2048)");
  RSX_ARG(Q >= 0 && Q < ((int64_t)1 << 31), "need 0 <= Q < 2^31");
  RSX_ARG(ld >= N, "need ld >= N");
  if (Q == 0) return 0;
  RSX_ARG(S && idx && val, "null tensor");
  RSX_ARG(((uintptr_t)S & 3) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)val & 3) == 0, "misaligned pointer");
  hipLaunchKernelGGL(select_topk_k, dim3((unsigned)Q), dim3(kSelThreads), 0, (hipStream_t)stream, S, ld, (int)N, (int)k,
                     idx, val);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_fuse_rank(const float* ua, int64_t ldua, const float* Ia, int64_t ldia, int64_t Da, const float* ub,
                          int64_t ldub, const float* Ib, int64_t ldib, int64_t Db, int64_t Q, int64_t NI,
                          const int32_t* cand, int64_t C, const float* wa, const float* wb, int A, int mode,
                          float k_rrf, int cut, const int32_t* ks, int nK, const int64_t* truth_off,
                          const int32_t* truth, int64_t n_truth, int32_t* hits, int32_t* lists, float* sa, float* sb,
                          int32_t* flag, void* stream) {
  RSX_ARG(C >= 1 && C <= kMaxC, "need 1 <= C <= 2048");
  RSX_ARG((Da == 64 || Da == 128) && (Db == 64 || Db == 128), "Da and Db must each be 64 or 128");
  RSX_ARG(A >= 1 && A <= kMaxAlpha, "need 1 <= A <= 32");
  RSX_ARG(nK >= 1 && nK <= kMaxKs, "need 1 <= nK <= 16");
  RSX_ARG(mode == RSX_FUSE_MINMAX || mode == RSX_FUSE_RRF, "mode must be RSX_FUSE_MINMAX or RSX_FUSE_RRF");
  RSX_ARG(cut >= 1 && cut <= C, "need 1 <= cut <= C");
  RSX_ARG(wa && wb && ks, "null host array (wa, wb, ks)");
  RSX_ARG(ks[0] >= 1, "need ks[0] >= 1");
  for (int j = 1; j < nK; ++j) RSX_ARG(ks[j] >= ks[j - 1], "ks must be ascending");
  RSX_ARG(ks[nK - 1] <= cut, "need ks[nK - 1] <= cut");
  RSX_ARG(Q >= 0 && Q < ((int64_t)1 << 31), "need 0 <= Q < 2^31");
  RSX_ARG(NI >= 1 && NI < ((int64_t)1 << 31), "need 1 <= NI < 2^31");
  RSX_ARG(n_truth >= 0, "need n_truth >= 0");
  RSX_ARG(ldua >= Da && ldia >= Da && ldub >= Db && ldib >= Db && ((ldua | ldia | ldub | ldib) & 3) == 0,
          "row strides must cover the width and be multiples of 4 floats");
  if (Q == 0) return 0;
  RSX_ARG(ua && Ia && ub && Ib && cand && truth_off && hits && flag && (truth || n_truth == 0), "null tensor");
  RSX_ARG((((uintptr_t)ua | (uintptr_t)Ia | (uintptr_t)ub | (uintptr_t)Ib) & 15) == 0 &&
              (((uintptr_t)cand | (uintptr_t)truth | (uintptr_t)hits | (uintptr_t)lists | (uintptr_t)sa | (uintptr_t)sb |
                (uintptr_t)flag) & 3) == 0 &&
              ((uintptr_t)truth_off & 7) == 0,
          "misaligned pointer (vector matrices 16 bytes, truth_off 8, the rest 4)");
  FuseArgs g{ua, Ia, ub, Ib, ldua, ldia, ldub, ldib, (int)Da, (int)Db, NI, cand, (int)C, truth_off, truth, n_truth,
             hits, lists, sa, sb, flag};
  FuseConsts k;
  memset(&k, 0, sizeof(k));
  for (int a = 0; a < A; ++a) k.wa[a] = wa[a], k.wb[a] = wb[a];
  for (int j = 0; j < nK; ++j) k.ks[j] = ks[j];
  k.A = A, k.nK = nK, k.cut = cut, k.mode = mode, k.k_rrf = k_rrf;
  hipLaunchKernelGGL(fuse_rank_k, dim3((unsigned)Q), dim3(kFuseThreads), fuse_lds_bytes((int)C), (hipStream_t)stream, g,
                     k);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_first_hit(const int32_t* lists, int64_t ld, int64_t Q, int64_t K, const int64_t* truth_off,
                          const int32_t* truth, int64_t n_truth, int32_t* out, void* stream) {
  RSX_ARG(K >= 1 && K < ((int64_t)1 << 31), "need 1 <= K < 2^31");
  RSX_ARG(ld >= K, "need ld >= K");
  RSX_ARG(Q >= 0 && Q < ((int64_t)1 << 31), "need 0 <= Q < 2^31");
  RSX_ARG(n_truth >= 0, "need n_truth >= 0");
  if (Q == 0) return 0;
  RSX_ARG(lists && truth_off && out && (truth || n_truth == 0), "null tensor");
  RSX_ARG((((uintptr_t)lists | (uintptr_t)truth | (uintptr_t)out) & 3) == 0 && ((uintptr_t)truth_off & 7) == 0,
          "misaligned pointer (truth_off 8 bytes, the rest 4)");
  hipLaunchKernelGGL(first_hit_k, dim3((unsigned)Q), dim3(kHitThreads), 0, (hipStream_t)stream, lists, ld, (int)K,
                     truth_off, truth, n_truth, out);
  RSX_LAUNCHED();
  return 0;
}
