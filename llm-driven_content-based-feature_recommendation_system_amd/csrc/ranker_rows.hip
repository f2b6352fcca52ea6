// The boosted ranker's training rows, built on the device (include/recsys_amd.h, "ranker training rows").
// The reference builds them on the host: utils/monitor/log_importer.py emits one positive and negative_ratio
// uniformly drawn non-bought items per purchase (a rejection loop over Python's random), and
// FeatureEngineer.prepare_batch (temp_model/ranker_skelet.py:13-89) turns every row into columns with numpy.
//   sample_k  one thread per (positive, slot): slot 0 copies the positive, slot 1 + k draws negative k as the
//             r-th item the customer has not bought, r from a counter hash, by one binary search over
//             s_j - j (the customer's sorted distinct bought items): no rejection, no walk over the list,
//             the same rows for every launch shape;
//   pair_k    one wave per (user, item) row: the columns of rsx_pair_cols.h, which rsx_rerank_tabular also
//             calls, the dot product as column 0 where no score is given and, on request, the label "the item
//             is in the user's truth set" by a binary search.
// Integer atomics only (the OR into the flag); every loop has a fixed bound.
#include "rsx_common.h"
#include "rsx_pair_cols.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSearchSteps = 32;   // a binary search over fewer than 2^31 entries ends within 32 halvings

// [off[i], off[i + 1]) of a CSR whose values array holds len entries, forced into [0, len] and non-negative
// length: a malformed offset table costs wrong rows, never an access outside the array.
__device__ __forceinline__ void csr_range(const int64_t* __restrict__ off, int64_t i, int64_t len, int64_t& b, int64_t& e) {
  b = off[i];
  e = off[i + 1];
  b = b < 0 ? 0 : (b > len ? len : b);
  e = e < b ? b : (e > len ? len : e);
}

__global__ __launch_bounds__(kThreads) void sample_k(const int* __restrict__ pos_user, const int* __restrict__ pos_item,
                                                     int64_t Pv, const int64_t* __restrict__ bought_off,
                                                     const int* __restrict__ bought, int64_t n_bought, int64_t C,
                                                     int64_t N, int64_t K, uint64_t seed, int* __restrict__ row_user,
                                                     int* __restrict__ row_item, float* __restrict__ y,
                                                     int* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= Pv * (K + 1)) return;
  const int64_t p = t / (K + 1), slot = t - p * (K + 1);
  int64_t user = pos_user[p], item = pos_item[p];
  if (user < 0 || user >= C || item < 0 || item >= N) {
    atomicOr(flag, 2);
    user = user < 0 || user >= C ? 0 : user;
    item = item < 0 || item >= N ? 0 : item;
  }
  if (slot != 0) {
    int64_t b, e;
    csr_range(bought_off, user, n_bought, b, e);
    const int64_t D = e - b, M = N - D;
    if (M <= 0) {      // nothing left to draw from: the reference's loop would never end
      atomicOr(flag, 1);
      item = 0;
    } else {
      const uint32_t h = rsx::hash_u32(seed, (uint64_t)(p * K + (slot - 1)));
      const int64_t r = (int64_t)(((uint64_t)h * (uint64_t)M) >> 32);      // in [0, M)
      // the r-th non-bought item is r + #{j : s_j - j <= r}; s_j - j never decreases, so the count is the
      // first j at which it exceeds r
      int64_t lo = 0, hi = D;
      for (int step = 0; step < kSearchSteps && lo < hi; ++step) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)bought[b + mid] - mid <= r) lo = mid + 1; else hi = mid;
      }
      item = r + lo;
      if (item >= N) {   // only a list that is not ascending and distinct within [0, N) gets here
        atomicOr(flag, 2);
        item = N - 1;
      }
    }
  }
  row_user[t] = (int)user;
  row_item[t] = (int)item;
  y[t] = slot == 0 ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(kThreads) void pair_k(const int* __restrict__ row_user, const int* __restrict__ row_item,
                                                   const float* __restrict__ score, const float* __restrict__ U,
                                                   const float* __restrict__ V, const float* __restrict__ price,
                                                   const float* __restrict__ avg, int64_t R, int64_t C, int64_t N, int d,
                                                   const int64_t* __restrict__ truth_off, const int* __restrict__ truth,
                                                   int64_t n_truth, float* __restrict__ feats, float* __restrict__ y_out,
                                                   int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (c >= R) return;    // whole waves leave: nothing below meets a barrier
  int64_t user = row_user[c], item = row_item[c];
  if (user < 0 || user >= C || item < 0 || item >= N) {
    if (lane == 0) atomicOr(flag, 1);
    user = user < 0 || user >= C ? 0 : user;
    item = item < 0 || item >= N ? 0 : item;
  }
  const float dot = rsx::pair_columns(U + user * d, V + item * d, d, lane, price + item, avg + user, feats, R, c);
  if (lane != 0) return;
  feats[c] = score != nullptr ? score[c] : dot;
  if (y_out == nullptr) return;
  int64_t lo, hi;
  csr_range(truth_off, user, n_truth, lo, hi);
  const int64_t end = hi;
  for (int step = 0; step < kSearchSteps && lo < hi; ++step) {      // the first entry >= item
    const int64_t mid = (lo + hi) >> 1;
    if (truth[mid] < item) lo = mid + 1; else hi = mid;
  }
  y_out[c] = lo < end && truth[lo] == item ? 1.0f : 0.0f;
}

}  // namespace

RSX_API int rsx_ranker_rows_sample(const int* pos_user, const int* pos_item, int64_t Pv, const int64_t* bought_off,
                                   const int* bought, int64_t n_bought, int64_t C, int64_t N, int64_t K, uint64_t seed,
                                   int* row_user, int* row_item, float* y, int* flag, void* stream) {
  RSX_ARG(pos_user && pos_item && bought_off && row_user && row_item && y && flag, "null tensor");
  RSX_ARG(n_bought >= 0 && n_bought < (1ll << 31) && (bought || n_bought == 0), "need 0 <= n_bought < 2^31 and bought");
  RSX_ARG(C >= 1 && N >= 1 && N < (1ll << 31), "need C >= 1 and 1 <= N < 2^31");
  RSX_ARG(K >= 0 && K < (1ll << 31), "need 0 <= K < 2^31");
  RSX_ARG(Pv >= 1 && Pv * (K + 1) < (1ll << 31), "need Pv >= 1 and Pv (K + 1) < 2^31");
  const int64_t rows = Pv * (K + 1);
  hipLaunchKernelGGL(sample_k, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     pos_user, pos_item, Pv, bought_off, bought, n_bought, C, N, K, seed, row_user, row_item, y, flag);
  RSX_LAUNCHED();
  return 0;
}

RSX_API int rsx_pair_tabular(const int* row_user, const int* row_item, const float* score, const float* U, const float* V,
                             const float* item_price, const float* user_avg_price, int64_t R, int64_t C, int64_t N,
                             int64_t d, const int64_t* truth_off, const int* truth, int64_t n_truth, float* feats,
                             float* y_out, int* flag, void* stream) {
  RSX_ARG(row_user && row_item && U && V && item_price && user_avg_price && feats && flag, "null tensor");
  RSX_ARG(R >= 1 && R < (1ll << 31), "need 1 <= R < 2^31");
  RSX_ARG(C >= 1 && N >= 1 && d >= 1 && d <= 65536, "need C, N >= 1 and 1 <= d <= 65536");
  if (y_out != nullptr) {
    RSX_ARG(truth_off && n_truth >= 0 && n_truth < (1ll << 31) && (truth || n_truth == 0),
            "y_out needs truth_off, truth and 0 <= n_truth < 2^31");
  }
  hipLaunchKernelGGL(pair_k, dim3((unsigned)((R + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0,
                     (hipStream_t)stream, row_user, row_item, score, U, V, item_price, user_avg_price, R, C, N, (int)d,
                     truth_off, truth, n_truth, feats, y_out, flag);
  RSX_LAUNCHED();
  return 0;
}
