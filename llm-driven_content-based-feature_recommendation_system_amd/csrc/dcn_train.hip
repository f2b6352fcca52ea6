// Training step of the DCN-V2 RankingModel (temp_model/ranker_skelet.py:274-357), the pieces that
// are not the cross network (csrc/dcn.hip: rsx_crossnet, rsx_crossnet_bwd). One step
// (ops.dcn_train_step orders the calls; nothing reads a value on the host):
//   x = cat(user, item[, context]) in a [B, Dp] buffer, Dp = D rounded up to 16, pad columns zero
//   rsx_crossnet            head_part = <x_L, w_head[0:D]>
//   rsx_linear_fwd, rsx_ln_fwd(GELU), dropout (rsx_dropout_bwd's mask: hash(seed, row*256 + col)),
//   rsx_linear_fwd, rsx_ln_fwd(GELU)                      -> h2 [B, 128]
//   rsx_dcn_train_head      logit, loss, g, dh2 = g w_d, dw_d, dbias (below)
//   rsx_ln_bwd, rsx_linear_wgrad, rsx_gemm_x3_tn, the same dropout mask, rsx_ln_bwd,
//   rsx_linear_wgrad (K = Dp)                              -> the deep half's gradients
//   rsx_crossnet_bwd        dk_l, db_l, dw_head from g
// The head is the DeepFM step's (csrc/deepfm_train.hip: same row loss, same fixed-order partials)
// without the ReLU mask on dh2: h2 is a GELU output here, negative for negative inputs, and the
// LayerNorm backward applies the GELU derivative itself.
#include "rsx_common.h"

namespace {
constexpr int kHeadCols = 128;
using rsx::aligned16;
}  // namespace

extern "C" int64_t rsx_deepfm_train_head_workspace_bytes(int64_t R);

RSX_API int64_t rsx_dcn_train_head_workspace_bytes(int64_t R) { return rsx_deepfm_train_head_workspace_bytes(R); }

RSX_API int rsx_dcn_train_head(const float* h2, int64_t H, const float* w_d, const float* head_part, const float* bias,
                               const float* y, int64_t R, int mean, float* logit, float* g, float* dh2, void* ws,
                               int64_t ws_bytes, double* loss, float* dbias, float* dw_d, void* stream) {
  RSX_ARG(h2 && w_d && head_part && bias && y && logit && g && dh2 && ws && loss && dbias && dw_d, "null tensor");
  RSX_ARG(H == kHeadCols, "the last hidden layer must be 128 wide");
  RSX_ARG(aligned16(h2) && aligned16(w_d) && aligned16(dh2) && aligned16(ws), "h2, w_d, dh2 and ws must be 16-byte aligned");
  RSX_ARG(R >= 1, "R must be positive");
  RSX_ARG(mean == 0 || mean == 1, "mean must be 0 (sum) or 1 (mean)");
  RSX_ARG(ws_bytes >= rsx_dcn_train_head_workspace_bytes(R), "workspace too small");
  return rsx::train_head_launch(h2, w_d, head_part, bias, y, R, mean, false, logit, g, dh2, ws, loss, dbias, dw_d,
                                stream);
}
