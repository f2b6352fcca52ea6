/*
 * recsys_amd.h - C ABI of librecsys_amd.so, the MI355X (gfx950) kernels behind the
 * two-tower retrieval + contrastive training + DeepFM rerank hot path of
 * DotBlossom/LLM-driven_content-based-feature_recommendation_system.
 *
 * Conventions (every entry point):
 *   - plain device pointers (fp32 row-major unless stated), int64 sizes, no torch types;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously, no
 *     host synchronisation, no device allocation inside (callers own every buffer, so a
 *     call can be captured into a hipGraph);
 *   - return 0 on success; non-zero = error code, text via rsx_last_error()
 *     (thread-local; argument errors return 1 before anything is launched);
 *   - "accumulated" outputs are added into and must be zeroed by the caller.
 * Each function names the reference interface it replaces (path:line under the
 * reference tree). The reference is pure Python/PyTorch; these are the kernels under its
 * nn.Module / loss-function surface (see INTEGRATION.md for the ctypes binding).
 */
#ifndef RECSYS_AMD_H
#define RECSYS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library identity / errors ------------------------------------------------------ */
const char* rsx_last_error(void);
int rsx_abi_version(void);
const char* rsx_target_arch(void);
/* sha256 (first 16 hex digits) of the sources the library was built from (csrc/Makefile: the .hip
 * files sorted by name, rsx_common.h, this header): a caller can tell a stale prebuilt binary. */
const char* rsx_build_hash(void);

/* ---- A2: SASRecUserTower embedding stage --------------------------------------------
 * Replaces tower_code/v1_refine_usertower.py:434-459:
 *   seq_emb = item_proj(pretrained_vecs); seq_emb += E_j(ids_j) * s_g[j] (j = 0..5);
 *   seq_emb += pos_emb(arange(L)); seq_emb = emb_ln(seq_emb); emb_dropout(seq_emb)
 * over T tokens: dense [B, L] (tok_pos NULL => position = token % L) or any packed token
 * list with tok_pos[T] (int64) giving each token's position (L <= 64).
 * base      [T, D] = item_proj output (nullable => 0)
 * base_idx  int64 [T] (nullable): token t reads base[base_idx[t]] instead of base[t] (base then
 *           holds one row per distinct item); the backward's dbase stays per token [T, D]
 * ids/tables: ntab (<=6) device pointers, ids int64 [T], tables [rows_j, D]
 * gate      [ntab] device (s_g = sigmoid(seq_gate) * s_mask); a gate that is exactly 0
 *           skips its gather (forward-exact) and reports a zero gate/table gradient
 *           (exact for the reference, whose zero gates come from a constant 0 mask)
 * pos [L, D], ln_w/ln_b [D] (ln_w == NULL => no LayerNorm: out = pre-LN sum, bit-exact
 * with the reference's op order), mean/rstd [T] saved for the backward.
 * D in {64, 128, 256}. Dropout p in [0,1) via counter hash (seed). */
int rsx_seq_embed_fwd(const float* base, const int64_t* base_idx, const int64_t* const* ids,
                      const float* const* tables, int ntab, const float* gate, const float* pos,
                      const int64_t* tok_pos, const float* ln_w, const float* ln_b, float eps, int64_t T, int64_t L,
                      int64_t D, float p_drop, uint64_t seed, float* out, float* mean, float* rstd, void* stream);

/* Backward of rsx_seq_embed_fwd. dbase [T,D] written; dtables[j], dgate [ntab], dpos [L,D],
 * dln_w/dln_b [D] accumulated (nullable). padding_idx[j]: rows excluded from the table
 * gradient exactly like nn.Embedding(padding_idx=...) (-1 = none). table_rows[j] lets small
 * tables (time buckets) accumulate in LDS. Position, small-table, LN and gate gradients are
 * per-workgroup LDS sums; with a workspace (>= rsx_seq_embed_bwd_workspace_floats floats) they
 * are stored per workgroup and folded in block order by a second kernel (deterministic);
 * workspace NULL flushes them with global float atomics (last bits vary run to run). */
int64_t rsx_seq_embed_bwd_workspace_floats(int64_t T, int64_t L, int64_t D);
int rsx_seq_embed_bwd(const float* base, const int64_t* base_idx, const int64_t* const* ids,
                      const float* const* tables, const int64_t* table_rows, const int64_t* padding_idx, int ntab, const float* gate,
                      const float* pos, const int64_t* tok_pos, const float* ln_w, const float* mean,
                      const float* rstd, float eps, int64_t T, int64_t L, int64_t D, float p_drop, uint64_t seed,
                      const float* dout, float* dbase, float* const* dtables, float* dgate, float* dpos,
                      float* dln_w, float* dln_b, float* workspace, int64_t ws_floats, void* stream);

/* ---- A3 / A9: masked multi-head self-attention core (L <= 64) -----------------------
 * Replaces the attention inside nn.TransformerEncoderLayer (norm_first, batch_first) at
 * tower_code/v1_refine_usertower.py:343-352,461-466 (causal + key padding) and
 * item_tower.py:169-182,281 (unmasked). Tokens are dense sequences (seg_off NULL: T = B*L)
 * or packed variable-length segments (seg_off [B+1] int32 token offsets, each <= 64 long).
 * qkv [T, 3*H*Dh] = in_proj output; out [T, H*Dh] = pre-out_proj head concat; lse [T, H].
 * key_pad [T] uint8 (1 = pad, nullable). Causal = key position <= query position within
 * the sequence. Training-path semantics: a fully masked query row gets zero probabilities.
 * Dh in {16, 32, 64} (backward: {16, 32}). */
int rsx_mha_fwd(const float* qkv, const uint8_t* key_pad, const int* seg_off, int64_t B, int64_t L, int64_t H,
                int64_t Dh, int causal, float p_drop, uint64_t seed, float* out, float* lse, void* stream);
/* dqkv [T, 3*H*Dh] written. */
int rsx_mha_bwd(const float* qkv, const uint8_t* key_pad, const int* seg_off, const float* out, const float* lse,
                const float* dout, int64_t B, int64_t L, int64_t H, int64_t Dh, int causal, float p_drop,
                uint64_t seed, float* dqkv, void* stream);
/* bf16x3 forms (Dh == 32; the forward also Dh == 64, the item tower's BERT at inference,
 * item_tower.py:264-268; same arguments, masks, dropout stream and lse convention):
 * 16x16 score tiles on v_mfma_f32_16x16x32_bf16 and token sums on v_mfma_f32_16x16x16_bf16
 * with every fp32 operand split hi + lo (~2^-17 relative error per product). The forward of
 * one form may be paired with the backward of the other. */
int rsx_mha_fwd_x3(const float* qkv, const uint8_t* key_pad, const int* seg_off, int64_t B, int64_t L, int64_t H,
                   int64_t Dh, int causal, float p_drop, uint64_t seed, float* out, float* lse, void* stream);
int rsx_mha_bwd_x3(const float* qkv, const uint8_t* key_pad, const int* seg_off, const float* out, const float* lse,
                   const float* dout, int64_t B, int64_t L, int64_t H, int64_t Dh, int causal, float p_drop,
                   uint64_t seed, float* dqkv, void* stream);
/* Fused in-projection + attention forward (replaces nn.TransformerEncoderLayer's
 * self_attn in_proj GEMM followed by the attention core, v1_refine_usertower.py:343-352 ->
 * torch.nn.functional.multi_head_attention_forward): x [T, D] the norm1 output, w [3D, D]
 * in_proj_weight, bias [3D] in_proj_bias (nullable); D = 128 (4 heads of 32), bf16x3. Writes
 * out [T, D] and lse [T, H] as rsx_mha_fwd_x3 does, and qkv [T, 3D] (nullable) for
 * rsx_mha_bwd_x3 and the in_proj weight gradient. */
int rsx_mha_qkv_fwd_x3(const float* x, const float* w, const float* bias, const uint8_t* key_pad, const int* seg_off,
                       int64_t B, int64_t L, int64_t H, int causal, float p_drop, uint64_t seed, float* qkv,
                       float* out, float* lse, void* stream);

/* ---- A6 / A7 / A12: fused in-batch contrastive cross-entropy ------------------------
 * S_ij = <A_i,B_j>/tau - bias_j over an implicit N x M matrix (never materialised),
 * fp32-input MFMA, online log-sum-exp. Row i's label column is i + diag_offset (0 on one
 * GPU; the shard offset when A holds one rank's rows and B the all-gathered columns).
 * flags (supported combinations):
 *   0                 plain InfoNCE, label = diagonal  (duorec unsup v1_refine_usertower.py:588-590,
 *                                                       item_tower.py:1075-1082 per direction)
 *   2 (MASK_K1)       + exclude off-diagonal j with k1_j == k1_i   (shadowed logq loss :520-573)
 *   6 (MASK_K1|K2)    + also k2 (user) keys               (live inbatch_corrected_logq_loss :826-861)
 *   9 (EXCL_DIAG|POS) SupCon term of duorec_loss_refined (:595-625): diagonal excluded,
 *                     positives k1_i == k1_j != 0, loss_i = LSE_i - mean positive logit
 *   18 (MASK_K1|DIAG_NOBIAS) flags 2 with the label logit left uncorrected: S_ii = <A_i,B_i>/tau, the
 *                     bias on the other columns only (efficient_corrected_logq_loss with lambda > 0,
 *                     tower_code/mined_inference.py:751-789: its "positive recovery"). 16 alone or with
 *                     any other bit is refused.
 * Keys are int32. D = 128 (row strides lda/ldb >= 128, multiple of 4, 16-B aligned).
 * ws: rsx_nce_workspace_floats(N, M, nsplit_fwd, nsplit_bwd) floats, shared by fwd and bwd.
 * out2 (device, 2 floats) = {sum of row losses over valid rows, number of valid rows};
 * the reference's mean is out2[0] / out2[1] (0 when no row is valid). */
int64_t rsx_nce_workspace_floats(int64_t N, int64_t M, int nsplit_fwd, int nsplit_bwd);
int rsx_nce_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, const int* k2a,
                const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau,
                int flags, int nsplit, float* ws, float* out2, void* stream);
/* gout = device scalar: gradient of the objective w.r.t. the row-loss SUM out2[0].
 * dA [N,128] / dB [M,128] (nullable; NULL skips that pass) written, or added into when
 * accumulate != 0. Must follow rsx_nce_fwd on the same ws. */
int rsx_nce_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, const int* k2a,
                const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau,
                int flags, int nsplit_fwd, int nsplit, const float* gout, float* ws, float* dA, float* dB,
                int accumulate, void* stream);

/* bf16x3 form of the two calls above (same flags, objective and outputs; products as
 * hi*hi + hi*lo + lo*hi on the bf16 MFMA, see RSX_NCE_BF16X3 below). The split counts are
 * chosen by the library (enough workgroups for the chip at any N, M); the workspace is
 * rsx_nce_x3_workspace_floats(N, M) floats and carries the hi/lo images between the calls. */
int64_t rsx_nce_x3_workspace_floats(int64_t N, int64_t M);
int rsx_nce_fwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                   const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                   int64_t diag_offset, float tau, int flags, float* ws, float* out2, void* stream);
int rsx_nce_bwd_x3(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                   const int* k2a, const int* k2b, int64_t N, int64_t M, int64_t lda, int64_t ldb,
                   int64_t diag_offset, float tau, int flags, const float* gout, float* ws, float* dA, float* dB,
                   int accumulate, void* stream);

/* Plain-family view of the fused grouped kernels (rsx_nce_grouped_fwd_grad and the grouped column
 * pass, below): the same objective as rsx_nce_fwd_x3 for
 *   flags 0                          (label = column i + diag_offset), and
 *   flags 9 (EXCL_DIAG|POS) with bias == NULL  (SupCon; keys k1a [N], k1b [M]),
 * anything else is an argument error. The N x M problem is run as a grouped one whose groups are
 * trivial (every column distinct with multiplicity 1; row i's one exception is its diagonal column,
 * kept at weight 1 as the label for flags 0 and dropped for flags 9), so the forward also gives the
 * row gradient and the backward is the column pass alone: two sweeps over the logits instead of
 * the plain family's three.
 *   view: rsx_nce_view_ints(N, M) ints filled by rsx_nce_view_fill (device memory, one launch) or
 *         rsx_nce_view_fill_host (host memory); depends on (N, M, diag_offset) only, so a caller
 *         with a fixed batch size fills it once.
 *   ws:   rsx_nce_fused_workspace_floats(N, M) floats, shared by the two calls.
 * Products: RSX_NCE_BF16X3 (see below) in both sweeps, whatever the grouped loss's mode. The one-fp16-MFMA
 * gradient products of RSX_NCE_F16 are not offered here: near convergence these two terms' gradients are
 * what is left after the softmax-weighted sum cancels against the label / the positives' mean, and 11-bit
 * products then leave up to 2.5e-2 of the gradient's scale (bf16x3: below 1e-3).
 * rsx_nce_fwd_grad: out2 as rsx_nce_fwd_x3; ga [N][128] = d(out2[0])/dA per unit upstream gradient
 * (dA = gout * ga); lse stays in ws. rsx_nce_bwd_cols writes dB [M][128] and must follow the forward
 * on the same ws. SupCon's positive term (mean positive logit) is sparse and runs in fp32 beside
 * the sweeps: per row cnt_i, P_i = sum of the positives' rows of B (ascending j) before the merge,
 * per column the sum of A_i / cnt_i over the rows that hold it as a positive (ascending i) after the
 * split sum. No float atomics: both calls are deterministic. A row without positives has zero loss
 * and gradient and is not counted in out2[1]. */
int64_t rsx_nce_fused_workspace_floats(int64_t N, int64_t M);
int64_t rsx_nce_view_ints(int64_t N, int64_t M);
int rsx_nce_view_fill(int64_t N, int64_t M, int64_t diag_offset, int* view, void* stream);
int rsx_nce_view_fill_host(int64_t N, int64_t M, int64_t diag_offset, int* view);
int rsx_nce_fwd_grad(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, int64_t N,
                     int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau, int flags,
                     const int* view, float* ws, float* out2, float* ga, void* stream);
int rsx_nce_bwd_cols(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b, int64_t N,
                     int64_t M, int64_t lda, int64_t ldb, int64_t diag_offset, float tau, int flags,
                     const int* view, const float* gout, float* ws, float* dB, void* stream);

/* Hard-emphasis term of full_batch_hard_emphasis_loss (replaces the reference's dense emphasis tensor,
 * scatter_ and masked cross-entropy over N x N logits, tower_code/v1_refine_usertower.py:762-822): row i's
 * K mined columns top[i*K + r] (int64, from rsx_hnm_mine) get +margin (already divided by tau) on top of
 * the flags-2 objective (k1 = target ids: same-item columns off the label excluded; bias = lambda*logQ).
 * Call rsx_nce_emphasis_fwd after rsx_nce_fwd / rsx_nce_fwd_x3 on the same ws (precision RSX_NCE_FP32 with
 * that call's nsplit_fwd, or RSX_NCE_BF16X3): each row's log-sum-exp and loss are corrected in ws from the
 * K mined logits alone and out2 is recomputed. Then rsx_nce_bwd(_x3) gives the dense gradient and
 * rsx_nce_emphasis_bwd adds the mined entries' extra (e^margin - 1) softmax weight into dA [N,128] / dB [M,128]
 * (nullable; dB by vector atomics: the summation order of a column shared by several rows is not fixed).
 * Mined ids outside [0, M) are skipped. O(N K) work and memory.
 * Precondition: the K mined ids of one row are distinct (a repeated id is counted twice where the
 * reference's scatter_ sets it once; rsx_hnm_mine's top-k never repeats one). */
int rsx_nce_emphasis_fwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                         const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb,
                         int64_t diag_offset, float tau, float margin, int precision, int nsplit_fwd, float* ws,
                         float* out2, void* stream);
int rsx_nce_emphasis_bwd(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                         const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb,
                         int64_t diag_offset, float tau, float margin, int precision, int nsplit_fwd,
                         const float* gout, float* ws, float* dA, float* dB, void* stream);
/* The same without float atomics: the mined entries' weights go to cbuf [N*K] (floats) and one wave per
 * column j adds them into dB from the column-sorted CSR of top (col_ptr [M+1] offsets, col_ent the entry
 * ids i*K + r in column order; ids outside [0, M) left out) -- deterministic for a fixed entry order. */
int rsx_nce_emphasis_bwd_csr(const float* A, const float* B, const float* bias, const int* k1a, const int* k1b,
                             const int64_t* top, int64_t N, int64_t M, int64_t K, int64_t lda, int64_t ldb,
                             int64_t diag_offset, float tau, float margin, int precision, int nsplit_fwd,
                             const int64_t* col_ptr, const int64_t* col_ent, float* cbuf, const float* gout,
                             float* ws, float* dA, float* dB, void* stream);

/* ---- A6 grouped: the live LogQ loss over the batch's DISTINCT targets ------------------
 * Same objective as rsx_nce_fwd flags 6 on columns normalize(item_matrix)[t_j], evaluated
 * over the D distinct targets (B[d] = normalised item uniq[d], bias[d] = logQ*lambda) with
 * exact integer multiplicities w_{i,d} = 1 if d == d(i) else c_d - n_{user(i),d}:
 *   colcnt [D] float  c_d = number of columns with target d
 *   row_col [N] int   d(i), the row's own target column
 *   row_beg/row_end [N] int  range of the row's user's targets in exc_cols (sorted d's)
 *   col_beg/col_end [D] int  range into exc_s/exc_e/exc_n: the user row ranges [s,e) that
 *                            hold target d and their multiplicity n (backward, dB pass only)
 * Rows of one user must be contiguous (flat (b, t) order). FLOPs: N*D instead of N*N.
 * precision: RSX_NCE_FP32 (0) = logits on the fp32-input MFMA (exact fp32 products);
 *            RSX_NCE_BF16X3 (1) = logits as hi*hi + hi*lo + lo*hi of a bf16 hi/lo split
 *            (fp32 accumulate, max |dot error| ~3e-6 on unit vectors), 5.3x fewer MFMA cycles;
 *            the gradient products (dS x rows) use the same split;
 *            RSX_NCE_F16 (2) = in the fused forward and the column pass: logits as the same three
 *            products of an fp16 hi/lo split of x * 2^8 on the fp16 MFMA (~2^-22 relative per term,
 *            tighter than bf16x3), gradient products as ONE fp16 MFMA of the rounded softmax weights
 *            and the rows' fp16 hi image (the reference's autocast(float16) arithmetic for these
 *            products, v1_usertower_train.py:787, with fp32 accumulation; RSX_NCE_F16_GP=2 adds the
 *            lo image); in the column pass the logits take two of the three products (the streamed rows'
 *            lo image dropped: ~2e-5 on unit vectors); elsewhere
 *            (rsx_nce_grouped_fwd, the row pass) as RSX_NCE_BF16X3. RSX_NCE_F16 covers the grouped
 *            loss only: the plain view above (rsx_nce_fwd_grad / rsx_nce_bwd_cols) runs bf16x3 products.
 *            Precondition of RSX_NCE_F16: every component of A and B has |x| < 256, so that x * 2^8
 *            stays inside fp16's range; the callers pass unit-norm rows. */
#define RSX_NCE_FP32 0
#define RSX_NCE_BF16X3 1
#define RSX_NCE_F16 2
/* ws for the grouped pair: >= rsx_nce_grouped_workspace_floats(N, D, nsplit_fwd, 8, precision)
 * (bf16x3 adds the hi/lo bf16 images of A and B; the forward writes B's, the backward's
 * column pass A's). The grouped backward's nsplit is 8. */
int64_t rsx_nce_grouped_workspace_floats(int64_t N, int64_t D, int nsplit_fwd, int nsplit_bwd, int precision);
int rsx_nce_grouped_fwd(const float* A, const float* B, const float* bias, const float* colcnt, const int* row_col,
                        const int* row_beg, const int* row_end, const int* exc_cols, int64_t N, int64_t D,
                        int64_t lda, int64_t ldb, float tau, int precision, int nsplit, float* ws, float* out2,
                        void* stream);
/* Forward fused with the row-side gradient (precision RSX_NCE_BF16X3 or RSX_NCE_F16): same loss as rsx_nce_grouped_fwd
 * (out2, and lse in ws for a later column pass), plus ga [N][128] = d(sum of row losses)/dA
 * per unit upstream gradient, i.e. dA = gout * ga. The row gradient is a softmax-weighted sum
 * of B's rows (an attention output), accumulated in the same sweep over S as the loss, so the
 * backward runs only the column pass (rsx_nce_grouped_bwd with dA = NULL). nsplit in
 * {1, 2, 4, 8}. Replaces the forward of the reference's live loss
 * (tower_code/v1_usertower_train.py:787-845) plus the row half of its autograd backward. */
int rsx_nce_grouped_fwd_grad(const float* A, const float* B, const float* bias, const float* colcnt,
                             const int* row_col, const int* row_beg, const int* row_end, const int* exc_cols,
                             int64_t N, int64_t D, int64_t lda, int64_t ldb, float tau, int precision, int nsplit,
                             float* ws, float* out2, float* ga, void* stream);
/* The fused forward's grid for (N, D, nsplit) on a device of cus compute units (cus <= 0: the current
 * device's), computed on the host without a launch (no reference counterpart: tests and tools read it).
 * With nsplit 1 or 2 the library lays the grid out in whole rounds of 2 x cus co-resident workgroups:
 * the leading rb1 row blocks (128 rows each) run ns1 column splits, the rest ns2, nslots partial slots
 * per row. sched[7] = {rb1, ns1, span1, ns2, span2, nslots, blocks} (span: columns per split);
 * block_map (nullable) receives {row block, split, first column, end column} of blocks
 * 0 .. min(blocks, max_blocks) - 1, exactly as the kernels derive them from their block index. */
int rsx_nce_fwdg_schedule(int64_t N, int64_t D, int nsplit, int cus, int64_t* sched, int64_t* block_map,
                          int64_t max_blocks);
/* Measurement hooks (no reference counterpart; bench.py's roofline): while enabled,
 * rsx_nce_grouped_fwd_grad brackets the fused forward kernel's own launch (not the B split or the
 * merge) with two HIP events on its stream; rsx_kernel_events_read waits for them and writes up to
 * max_n durations (ms, launch order), returning how many were recorded (-1 on a HIP error).
 * Enabling clears the list. */
int rsx_kernel_events(int on);
int rsx_kernel_events_read(float* ms, int max_n);
/* The same for the embedding gather (rsx_seq_embed_fwd's kernel, whichever caller issues it: the per-op
 * path or rsx_tower_fwd): rsx_gather_events(1) clears and starts recording; _read waits and writes up to
 * max_n launch times (ms) with each launch's token count. */
int rsx_gather_events(int on);
int rsx_gather_events_read(float* ms, int64_t* tokens, int max_n);
int rsx_nce_grouped_bwd(const float* A, const float* B, const float* bias, const float* colcnt, const int* row_col,
                        const int* row_beg, const int* row_end, const int* exc_cols, const int* col_beg,
                        const int* col_end, const int* exc_s, const int* exc_e, const int* exc_n, int64_t N,
                        int64_t D, int64_t lda, int64_t ldb, float tau, int precision, int nsplit_fwd,
                        int nsplit, const float* gout, float* ws, float* dA, float* dB, int accumulate,
                        void* stream);

/* ---- static-profile embeddings: gated lookups of several tiny tables, concatenated ------
 * out[b, off_j + c] = E_j[ids_j[b]][c] * gate[j]. The backward's dout has B rows, row b from
 * user b % ids_rows (ids hold ids_rows entries: the contrastive step's two dropout views share
 * their users), and gives dE_j (padding_idx rows: 0 when written, untouched when added) and
 * dgate[j], added into (accumulate = 1) or written (0); per-64-row workgroup partials in ws
 * (rsx_static_embed_bwd_workspace_floats) reduced in a fixed order, so the gradients are
 * identical run to run. Replaces the nine nn.Embedding lookups x u_g of
 * tower_code/v1_refine_usertower.py:472-494 (and their sort-based embedding backward).
 * <= 16 tables, <= 256 columns, <= 4096 table floats in total. */
int rsx_static_embed_fwd(const int64_t* const* ids, const float* const* tables, const int64_t* table_rows,
                         const int64_t* dims, int ntab, const float* gate, int64_t B, float* out, int64_t ld_out,
                         void* stream);
int64_t rsx_static_embed_bwd_workspace_floats(int64_t B, int ntab, const int64_t* table_rows, const int64_t* dims);
int rsx_static_embed_bwd(const int64_t* const* ids, const float* const* tables, const int64_t* table_rows,
                         const int64_t* dims, const int64_t* padding_idx, int ntab, const float* gate,
                         const float* dout, int64_t ld_dout, int64_t B, int64_t ids_rows, float* const* dtables,
                         float* dgate, int accumulate, float* ws, int64_t ws_floats, void* stream);

/* ---- LayerNorm fused with the preceding residual add + dropout and a following GELU ----
 * s = x + dropout(res) (res nullable), y = act(LN(s) * w + b), act 0 none / 2 GELU(erf).
 * Replaces norm1/norm2 and the residual adds of the norm_first TransformerEncoderLayer and the
 * output head LayerNorm+GELU (tower_code/v1_refine_usertower.py:40-50, 68-72, 447-510).
 * sum_out (nullable) receives s when res is given; mean/rstd [T] are saved for the backward.
 * Backward: ds_out = LN-backward(dy) + ds_in (ds_in nullable), dres = dropout-backward(ds_out),
 * dw/db via per-block partials (ws >= rsx_ln_bwd_workspace_floats). D in {64, 128, 256}; the
 * forward also takes D in {512, 768, 1024} (the item tower's BERT LayerNorms, item_tower.py:175,
 * inference: rsx_ln_bwd stays at D <= 256). rsx_ln_bwd_workspace_floats returns -1 for a D that
 * rsx_ln_bwd does not accept. */
int rsx_ln_fwd(const float* x, const float* res, float p_drop, uint64_t seed, const float* w, const float* b,
               float eps, int act, int64_t T, int64_t D, float* sum_out, float* y, float* mean, float* rstd,
               void* stream);
/* Backward of the add-only form of rsx_ln_fwd (y = NULL: s = x + dropout_p(res), as after the
 * encoder's last layer, v1_refine_usertower.py:343-352): dres = the forward's keep-mask / (1 - p)
 * applied to ds (flat index row*D + col); dx is ds itself. */
int rsx_dropout_bwd(const float* ds, int64_t T, int64_t D, float p_drop, uint64_t seed, float* dres, void* stream);
int64_t rsx_ln_bwd_workspace_floats(int64_t T, int64_t D);
int rsx_ln_bwd(const float* s, const float* mean, const float* rstd, const float* w, const float* b, int act,
               const float* dy, const float* ds_in, float p_drop, uint64_t seed, int64_t T, int64_t D, float* ds_out,
               float* dres, float* dw, float* db, float* ws, int64_t ws_floats, void* stream);

/* ---- weight gradient of token-level linear layers ---------------------------------------
 * dW[n][k] (+)= sum_t dY[t][n] X[t][k], db[n] (+)= sum_t dY[t][n] (db nullable), fp32 MFMA,
 * split over tokens with a deterministic partial reduction. Replaces autograd's weight-grad
 * GEMM of every per-token nn.Linear in the user tower's step (tower_code/v1_refine_usertower.py
 * :447-510 — item_proj, in_proj/out_proj/linear1/linear2 of both encoder layers, output_proj).
 * N, K multiples of 16; ws >= rsx_linear_wgrad_workspace_floats(T, N, K) floats. */
int64_t rsx_linear_wgrad_workspace_floats(int64_t T, int64_t N, int64_t K);
int rsx_linear_wgrad(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t T, int64_t N, int64_t K,
                     float* dW, int64_t ldw, float* db, int accumulate, float* ws, int64_t ws_floats, void* stream);
/* Same contract in bf16x3 split precision (hi*hi + hi*lo + lo*hi on the bf16 MFMA, fp32
 * accumulate; db summed in fp32): the default of the training step. */
int rsx_linear_wgrad_x3(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t T, int64_t N,
                        int64_t K, float* dW, int64_t ldw, float* db, int accumulate, float* ws, int64_t ws_floats,
                        void* stream);

/* ---- forward / input-gradient GEMMs of the token-level linear layers (bf16x3) ------------
 * C[M, N] = epi(A[M, K] . B[N, K]^T + bias): the forward Y = X W^T + b (B = W) and the input
 * gradient dX = dY W (B = W^T) of the same per-token nn.Linear layers as rsx_linear_wgrad,
 * replacing autograd's library GEMMs. epi: 0 bias; 1 z = acc + bias, C = dropout_p(gelu_erf(z))
 * (keep-mask hash(seed, m*N + n)), aux = gelu_erf'(z) (aux may be NULL: inference, e.g. the
 * item tower's BERT intermediate layer, item_tower.py:175); 2 C = acc * keep / (1-p) * aux, its
 * backward (same seed, aux from epi 1). Epilogues 1/2 fuse nn.TransformerEncoderLayer's feed-forward
 * dropout(gelu(linear1(x))) (v1_refine_usertower.py:343-352) into its GEMMs. 3 (rsx_gemm_x3 and
 * rsx_gemm_x3_ws only) C = max(acc + bias, 0), inference only: aux must be NULL and p_drop 0 (the
 * ReLU feed-forward of HybridUserTower's encoder, tower_code/mined_inference.py:635-638).
 * N % 128 == 0, K % 32 == 0, A/B 16-byte aligned, leading dimensions multiples of 4. */
int rsx_gemm_x3(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int64_t M, int N, int K,
                int epi, float* aux, int64_t ldaux, float p_drop, uint64_t seed, float* C, int64_t ldc, void* stream);
/* The same with a caller workspace for split-K: when the output has fewer 128 x 128 tiles than the device
 * has CUs and K is long (K not 128 / 256 / 384), S K-ranges per tile run as separate workgroups writing
 * partial sums to ws, and one pass adds them in split order and applies epi. ws_floats >=
 * rsx_gemm_x3_split_floats(M, N, K) (0 = no split for this shape; ws may then be null). Deterministic; the
 * summation order over K differs from rsx_gemm_x3's (fp32 rounding level). */
int64_t rsx_gemm_x3_split_floats(int64_t M, int N, int K);
int rsx_gemm_x3_ws(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int64_t M, int N,
                   int K, int epi, float* aux, int64_t ldaux, float p_drop, uint64_t seed, float* C, int64_t ldc,
                   float* ws, int64_t ws_floats, void* stream);
/* The kernel form rsx_gemm_x3_ws takes for a shape with ws_floats of workspace (0: rsx_gemm_x3, or a null ws):
 * 0 weight-stationary (K 128 / 256 / 384; C, and aux when given, must then be 16-byte aligned with row strides
 * that are multiples of 4), 1 LDS-staged two-stage stream, 2 four stages in flight at 32 of K per stage,
 * 3 four stages at 16 of K per stage, 4 split-K (split count = rsx_gemm_x3_split_floats / (M * N));
 * -1 for a shape the entry refuses. epi 0..3 as rsx_gemm_x3, 4 = rsx_gemm_x3_relu_train's epilogue. The
 * dispatcher switches on this function; it launches nothing and needs no device (256 CUs are assumed then). */
int rsx_gemm_x3_form(int64_t M, int N, int K, int epi, int64_t ws_floats);
/* The ReLU feed-forward's first GEMM with gradients (nn.TransformerEncoderLayer's default activation:
 * dropout(relu(linear1(x))) of HybridUserTower's encoder, tower_code/mined_inference.py:635-638, in
 * training): z = A . B^T + bias, C = dropout_p(max(z, 0)) with keep-mask hash(seed, m*N + n) as epi 1,
 * aux[m][n] = z > 0 ? 1 : 0 (required; 16-byte aligned, ldaux >= N and a multiple of 4, as C and ldc).
 * Its backward is epi 2 of rsx_gemm_x3 / rsx_gemm_x3_tn with the same aux, p_drop and seed. Shapes,
 * ws and ws_floats as rsx_gemm_x3_ws. */
int rsx_gemm_x3_relu_train(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int64_t M,
                           int N, int K, float* aux, int64_t ldaux, float p_drop, uint64_t seed, float* C,
                           int64_t ldc, float* ws, int64_t ws_floats, void* stream);
/* C = epi(A . Bt + bias) with Bt [K, N] as stored (row stride ldbt >= N): the input gradient
 * dX = dY . W of the same token linears straight from W [out, in] (K = out, N = in; autograd's
 * dX GEMM of nn.Linear, v1_refine_usertower.py:447-510), no transposed copy of W; epi / aux /
 * p_drop / seed as rsx_gemm_x3 (EPI_DGELU_DROP: the feed-forward's backward through GELU and
 * dropout). K in {128, 256, 384}, N % 128 == 0, A/C 16-byte aligned. */
int rsx_gemm_x3_tn(const float* A, int64_t lda, const float* Bt, int64_t ldbt, const float* bias, int64_t M, int N,
                   int K, int epi, float* aux, int64_t ldaux, float p_drop, uint64_t seed, float* C, int64_t ldc,
                   void* stream);
/* C[m] = A[m] . B^T + bias + R[ridx[m]]: a per-row table added in the epilogue. Replaces
 * output_proj[0](cat(enc_out, profile.expand)) of SASRecUserTower.forward
 * (v1_refine_usertower.py:498-505) over the packed tokens: A = encoder output, B = the token
 * half of output_proj[0].weight (ldb = 256), R = profile half + bias per user, ridx = user of
 * each token. K 128 or 256, N % 128 == 0, every pointer 16-byte aligned. */
int rsx_gemm_x3_rowadd(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int64_t M, int N,
                       int K, const float* R, int64_t ldr, const int64_t* ridx, float* C, int64_t ldc, void* stream);
/* S = X + dropout_p(A . B^T + bias); Y = LayerNorm(S) * ln_w + ln_b; mean / rstd per row.
 * Replaces a norm_first encoder layer's `x = x + dropout(out_proj(attn)); norm2(x)`
 * (v1_refine_usertower.py:343-352, nn.TransformerEncoderLayer._sa_block + norm2) in one
 * weight-stationary GEMM: the add and the LayerNorm run in its epilogue. N = 128, K 128 or 256,
 * every pointer 16-byte aligned; dropout mask = rsx_ln_fwd's (hash(seed, m * N + n)), so
 * rsx_ln_bwd (ds_in, dres) is its backward. ln_w / ln_b nullable (1 / 0). */
int rsx_gemm_x3_addln(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, int64_t M, int N,
                      int K, const float* X, int64_t ldx, float p_drop, uint64_t seed, const float* ln_w,
                      const float* ln_b, float eps, float* S, int64_t lds, float* Y, int64_t ldy, float* mean,
                      float* rstd, void* stream);

/* Device-side id range check (no host sync): out[i] = ids[i] if lo <= ids[i] < hi else 0, and
 * *flag = 1 if any id was outside [lo, hi) (untouched otherwise). Replaces the out-of-range
 * failure of nn.Embedding on the item tower's STD ids (item_tower.py:240, vocab ids 0..383,
 * utils/vocab.py:436-441): the caller raises when the flag reaches the host. */
int rsx_ids_check(const int64_t* ids, int64_t n, int64_t lo, int64_t hi, int64_t* out, int* flag, void* stream);

/* ---- A8: the step index on the device ----------------------------------------------------
 * Every data-dependent structure of one contrastive step (train_user_tower_all_time's per-batch
 * flattening, v1_usertower_train.py:794-835, plus the grouped loss's target index) from the
 * batch's [B, L] tensors, with ONE host read (the totals). pm: padding_mask as bytes (1 = pad),
 * tgt / item: target_ids / item_ids int64 [B, L], ids in [0, n_items); L <= 64.
 *   1. rsx_step_index_count   -> tloc [B*L + 1] int32: this rank's loss-row targets (flat
 *      order, -1 padded) and its row count in the last slot
 *   2. (world > 1) the caller all-gathers tloc blocks rank-major into tglob [world][B*L + 1]
 *   3. rsx_step_index_totals  -> totals [8 + world] int64 on the device: T (packed tokens per
 *      view), N (loss rows), D (distinct target columns over tglob), E (distinct (user, target)
 *      pairs), U (distinct item ids among the tokens), C (segment-sum chunks), error flag (ids
 *      out of range), 0, then every rank's row count
 *   4. rsx_step_index_fill(sizes = totals[0..5] read on the host) writes out[0..33]:
 *      0 flat [T] i64, 1 tok_user [T] i64, 2 tok_pos [T] i64, 3 tok_pad [T] u8, 4 seg_off [B+1] i32,
 *      5 seg_off [B+1] i64, 6 valid_tok [N] i64, 7 last_tok [B] i64; the doubled two-view batch:
 *      8 flat [2T], 9 tok_user [2T], 10 tok_pos [2T] i64, 11 tok_pad [2T] u8, 12 seg_off [2B+1]
 *      i32, 13 seg_off [2B+1] i64, 14 tok_ids [6][2T] i64 (seq_ids per token, both views),
 *      15 pretrained rows of the distinct items [U][128] f32 in the order of 20 (nullable; from
 *      lookup [n_items][ld_lookup]; token t of either view owns row 33[t]); the
 *      item-id segment-sum plan: 16 perm [2T], 17 cb [C+1], 18 chunk ids [C], 19 ch_off [U+1],
 *      20 ids [U] (all i64); the grouped-loss index: 21 uniq [D] i64, 22 colcnt [D] f32,
 *      23 row_col, 24 row_beg, 25 row_end, 26 exc_cols [N] i32, 27 exc_s, 28 exc_e, 29 exc_n [E]
 *      i32, 30 col_beg, 31 col_end [D] i32; 32 last_t [B] i32 (the SupCon keys: last targets);
 *      33 tok_uidx [2T] i64 (each token's slot in 20, the same for both views).
 * ws: rsx_step_index_workspace_bytes(B, L, n_items), the same buffer for all three calls. */
int64_t rsx_step_index_workspace_bytes(int64_t B, int64_t L, int64_t n_items);
int rsx_step_index_count(const uint8_t* pm, const int64_t* tgt, const int64_t* item, int64_t B, int64_t L,
                         int64_t n_items, void* ws, int64_t ws_bytes, int* tloc, void* stream);
int rsx_step_index_totals(const int* tglob, int world, int64_t B, int64_t L, int64_t n_items, void* ws,
                          int64_t ws_bytes, int64_t* totals, void* stream);
int rsx_step_index_fill(const uint8_t* pm, const int64_t* tgt, const int64_t* const* seq_ids, const float* lookup,
                        int64_t ld_lookup, int64_t B, int64_t L, int64_t n_items, const int64_t* sizes, void* ws,
                        int64_t ws_bytes, void* const* out, void* stream);

/* ---- A14: retrieval top-k ------------------------------------------------------------
 * scores = U I^T (fp32 MFMA, never materialised), per query the k best items sorted by
 * (score desc, index asc). Replaces `scores = matmul(user, items.T); topk(k)` at
 * tower_code/v1_usertower_train.py:672-675 and temp_model/ranker_skelet.py:193-196.
 * U [Q, ldu], I [NI, ldi], D = 128, 1 <= k <= rsx_topk_max_k() = 2048. ws: rsx_topk_workspace_bytes(Q, NI, k).
 * k <= 512: every corpus; out_idx = -1 where fewer than k items exist. 512 < k <= 2048: k <= NI, and
 * only where rsx_topk_path returns 2 (NI >= 131,072 for k <= 1024, NI >= 262,144 beyond); elsewhere
 * the call is an argument error (select from a materialised score matrix: rsx_select_topk_rows). */
int64_t rsx_topk_workspace_bytes(int64_t Q, int64_t NI, int64_t k);
int rsx_retrieve_topk(const float* U, int64_t ldu, const float* I, int64_t ldi, int64_t Q, int64_t NI, int64_t k,
                      void* ws, float* out_scores, int64_t* out_idx, void* stream);
/* Which exact path a (Q, NI, k) call takes: 0 list kernels, 1 fp32 candidate/threshold path,
 * 2 bf16 single scan + exact fp32 rescoring (large corpora), 3 (k > 512 only) not served natively.
 * Every call writes a workspace
 * header: int32 ws[0] = queries path 2 sent to the exact kernels, ws[1] = path id, ws[2] = path
 * 1's whole-batch fallback flag. Path 2 runs the queries in chunks of at most 4096 (workspace
 * bounded in Q). Its exact kernels for listed queries are the list kernels for k <= 512 and, for
 * k > 512, fp32 score rows in a scratch of at most 256 MB (whatever Q is) with a radix select per row. */
int rsx_topk_path(int64_t Q, int64_t NI, int64_t k);
/* Path 2's capacities: the largest k; entries per lane stream of the collect pass; collected entries
 * per query; entries of the rescored margin set for a given k. A query that exceeds one of them
 * runs on the exact kernels. */
int64_t rsx_topk_max_k(void);
int64_t rsx_topk_stream_capacity(void);
int64_t rsx_topk_entry_capacity(void);
int64_t rsx_topk_margin_capacity(int64_t k);
/* Path 2 with a caller-cached corpus image (a static corpus, e.g. the serving item matrix of
 * controller.py:62-124 or evaluate_model's normalised item table, :672): rsx_topk_prepare_corpus
 * writes max ||w||, max ||w - bf16(w)|| and the bf16 image of I into `corpus` (rsx_topk_corpus_bytes(NI) bytes) once;
 * rsx_retrieve_topk_corpus then skips that pass (ws: rsx_topk_workspace_bytes_corpus). I must
 * be the corpus the image was made from (the exact rescoring reads it). */
int64_t rsx_topk_corpus_bytes(int64_t NI);
int rsx_topk_prepare_corpus(const float* I, int64_t ldi, int64_t NI, void* corpus, void* stream);
int64_t rsx_topk_workspace_bytes_corpus(int64_t Q, int64_t NI, int64_t k);
int rsx_retrieve_topk_corpus(const float* U, int64_t ldu, const float* I, int64_t ldi, const void* corpus, int64_t Q,
                             int64_t NI, int64_t k, void* ws, float* out_scores, int64_t* out_idx, void* stream);

/* ---- A16: DeepFM rerank forward ------------------------------------------------------
 * deepctr-torch 0.2.9 DeepFM semantics (absent from the reference tree).
 * rsx_deepfm_embed: x [R, F] int64 per-field ids, V[f] [vocab_f, 16], W[f] [vocab_f] (nullable)
 *   -> emb_out [R, F*16] (concatenated DNN input, nullable) and
 *      lin_out[r] = bias + sum_f W[f][x] + 0.5 * sum_k((sum_f v)^2 - sum_f v^2).
 * rsx_linear_fwd: Y [M, N] = act(X W^T + b), W [N, K] torch Linear layout, N <= 256,
 *   K % 4 == 0, act 0 none / 1 relu / 2 gelu (erf). fp32 MFMA.
 * rsx_linear_dot_fwd: logit[m] = sum_n act(X W^T + b)[m, n] * wo[n] + add[m];
 *   prob = sigmoid(logit) (nullable). */
int rsx_deepfm_embed(const int64_t* x, int64_t R, int F, int E, const float* const* V, const float* const* W,
                     float bias, float* emb_out, float* lin_out, void* stream);
int rsx_linear_fwd(const float* X, int64_t ldx, const float* W, const float* b, int64_t M, int64_t N, int64_t K,
                   int act, float* Y, void* stream);
int rsx_linear_dot_fwd(const float* X, int64_t ldx, const float* W, const float* b, int64_t M, int64_t N, int64_t K,
                       int act, const float* wo, const float* add, float* logit, float* prob, void* stream);

/* rsx_deepfm_fused: the whole forward in one kernel (gather + first-order + FM + the
 *   (256, 128) ReLU DNN on bf16x3 MFMA + final dot + sigmoid); the [R, F*16] DNN input never
 *   reaches HBM. Same arguments as the three calls above with w1 [256, F*16], b1 [256],
 *   w2 [128, 256], b2 [128], wo [128] (torch Linear layouts; dnn_hidden_units = (256, 128),
 *   embed_dim 16). ws: rsx_deepfm_fused_workspace_bytes(F) (per-call bf16 weight images).
 *   Replaces the same deepctr-torch DeepFM forward. */
int64_t rsx_deepfm_fused_workspace_bytes(int F);
int rsx_deepfm_fused(const int64_t* x, int64_t R, int F, const float* const* V, const float* const* W, float bias,
                     const float* w1, const float* b1, const float* w2, const float* b2, const float* wo, void* ws,
                     float* logit, float* prob, void* stream);
/* The two halves of rsx_deepfm_fused, for callers that keep ws across calls (the weight images
 * are a function of w1/w2 only: rebuild them with rsx_deepfm_fused_prep after an update).
 * F in [25, 48] runs the persistent kernel (one workgroup per CU looping over 64-row blocks). */
int rsx_deepfm_fused_prep(int F, const float* w1, const float* w2, void* ws, void* stream);
/* packed: nullable per-field tables from rsx_deepfm_pack, read instead of V/W when
 * rsx_deepfm_fused_uses_packed(F) == 1 (F = 39: deepfm_rows2m_k, 256-row workgroups of eight 32-row
 * waves, 130 KiB of LDS; other F in [25, 48]: the persistent kernel): a field's V row and first-order
 * weight then share one 128-B line, halving the lines fetched per (row, field) on random ids. NULL:
 * V/W are read directly (F = 39: deepfm_rows5_k). */
int rsx_deepfm_fused_run(const int64_t* x, int64_t R, int F, const float* const* V, const float* const* W,
                         const float* const* packed, float bias, const float* b1, const float* b2, const float* wo,
                         const void* ws, float* logit, float* prob, void* stream);
/* packed [vocab][32] = (V [vocab][16] row, W [vocab] (0 if NULL), 15 zeros): one field's table. */
int rsx_deepfm_pack(const float* V, const float* W, int64_t vocab, float* packed, void* stream);
int rsx_deepfm_fused_uses_packed(int F);

/* ---- A16 training: one DeepFM step (Logloss backward + sparse Adam), csrc/deepfm_train.hip ----
 * Trains the model of the forward above where the reference trains its ranker before use
 * (RecommendationRanker.train, CatBoost Logloss, temp_model/ranker_skelet.py:114-137); deepctr-torch's
 * own fit() cannot be run here: parity unpinned. Loss = binary cross-entropy on the logit, table rows
 * updated with torch.optim.SparseAdam semantics, deterministic (no float atomics). embed_dim 16,
 * last hidden layer 128, 1 <= F <= 64, R * F < 2^31. Call order (ops.deepfm_train_step):
 * rsx_deepfm_train_keys: x [R, F] -> keys [R*F] = field << 40 | id, xs [R*F] = the ids with every id
 *   outside [0, vocab[f]) (vocab: F host values) replaced by 0 (what the gathers read); such a pair's
 *   key id is 2^40 - 1 (its contribution is summed but never applied) and *flag (device int32) = 1.
 * The caller sorts the keys (stable) -> keys_sorted, perm.
 * rsx_deepfm_train_segments: head [n] = 1 where a new key starts, inv [n] = inverse of perm.
 * rsx_deepfm_train_starts: head_cum [n] = inclusive scan of head -> seg_start [U + 1] (last = n) and
 *   *nseg = U, the number of distinct (field, id), all on the device.
 * rsx_deepfm_train_head: h2 [R, H = 128], wo [128], lin [R] (rsx_deepfm_embed's lin_out), bias [1]
 *   (device, nullable: added to every logit, so the step never reads out.bias on the host), y [R] ->
 *   logit [R], g [R] = (sigmoid(logit) - y) * (mean ? 1/R : 1), dh2 [R, 128] = g wo [h2 > 0],
 *   loss[0] (double) = sum or mean of max(z,0) - z y + log1p(exp(-|z|)), dbias[0] = sum g,
 *   dwo [128] = sum_r g_r h2_r; per-64-row partials in ws, added in a fixed two-level order.
 * rsx_relu_bwd: dx[i] = h[i] > 0 ? dx[i] : 0 (n floats, n % 4 == 0).
 * rsx_deepfm_train_contrib: emb [R, F*16] (the forward's), dE [R, ldE] (DNN input gradient) ->
 *   gV [n, 16] / gW [n] at each pair's sorted position inv[r*F + f]:
 *   g_r (sum_f' v_rf' - v_rf) + dE[r, f*16 ..] and g_r.
 * rsx_deepfm_train_sparse_adam: sums gV / gW per distinct key in sorted order (segments longer than
 *   128 as 64-contribution partials in ws, added in order) and applies, for step count `step` (>= 1,
 *   shared by all tables), m += (1-b1)(g-m); v += (1-b2)(g^2-v);
 *   p -= lr sqrt(1-b2^step)/(1-b1^step) m / (sqrt(v) + eps) to row id of V[f] [vocab_f, 16],
 *   W[f] [vocab_f] and their moments; no other row is read or written. out_dV [n, 16] / out_dW [n]
 *   (nullable, together) receive the summed gradient of segment u at row u (the values the update
 *   consumed; segments in keys_sorted[seg_start[u]] order). */
int rsx_deepfm_train_keys(const int64_t* x, int64_t R, int F, const int64_t* vocab, int64_t* keys, int64_t* xs,
                          int* flag, void* stream);
int rsx_deepfm_train_segments(const int64_t* keys_sorted, const int64_t* perm, int64_t n, int* head, int* inv,
                              void* stream);
int rsx_deepfm_train_starts(const int* head_cum, int64_t n, int* seg_start, int* nseg, void* stream);
int64_t rsx_deepfm_train_head_workspace_bytes(int64_t R);
int rsx_deepfm_train_head(const float* h2, int64_t H, const float* wo, const float* lin, const float* bias,
                          const float* y, int64_t R, int mean, float* logit, float* g, float* dh2, void* ws,
                          int64_t ws_bytes, double* loss, float* dbias, float* dwo, void* stream);
int rsx_relu_bwd(float* dx, const float* h, int64_t n, void* stream);
int rsx_deepfm_train_contrib(const float* emb, const float* g, const float* dE, int64_t ldE, const int* inv,
                             int64_t R, int F, int E, float* gV, float* gW, void* stream);
int64_t rsx_deepfm_train_sparse_workspace_bytes(int64_t n);
int rsx_deepfm_train_sparse_adam(const int64_t* keys_sorted, const int* head_cum, const int* seg_start,
                                 const int* nseg, int64_t n, int F, int E, const int64_t* vocab, const float* gV,
                                 const float* gW, float* const* V, float* const* W, float* const* mV,
                                 float* const* vV, float* const* mW, float* const* vW, double lr, double beta1,
                                 double beta2, double eps, int64_t step, void* ws, int64_t ws_bytes, float* out_dV,
                                 float* out_dW, void* stream);

/* ---- A16 validation: exact AUC and Logloss of a binary ranker, csrc/binary_eval.hip ---------------
 * The metrics the reference's ranker is trained against (CatBoostClassifier(eval_metric='AUC',
 * early_stopping_rounds=50), temp_model/ranker_skelet.py:98-108; eval_set / use_best_model, :123-135),
 * for R scored rows with one host read. logit [R], y [R] fp32 ->
 *   counts [3] (int64) = P = #{y == 1}, N = #{y == 0}, U2 = sum over positive rows i of
 *     #{negative j : z_j < z_i} + #{negative j : z_j <= z_i}: twice the Mann-Whitney U statistic with
 *     ties at one half, an exact integer (U2 <= 2 P N < 2^61); AUC = U2 / (2 P N), formed by the
 *     caller in double. Scores compare as reals: -0.0 and +0.0 tie.
 *   loss_sum [1] (double) = sum_r max(z,0) - z y + log1p(exp(-|z|)) (rsx_deepfm_train_head's row
 *     expression), from per-workgroup partials added in a fixed order: the same bits every run.
 *   flag [1] (int32): bit 0 = a logit is NaN or +-inf, bit 1 = a label is neither 0 nor 1; with a flag
 *     set the other outputs are unspecified (every access stays in bounds).
 * Key pass, radix sort of (key, label), three scans over 2048-row tiles; no step walks a tie group, so
 * one group spanning all R rows costs what distinct scores cost. Integer sums and one fixed-order
 * double sum: deterministic, no float atomics. 1 <= R < 2^31 (rsx_binary_eval_workspace_bytes
 * returns -1 outside it); ws 16-byte aligned, counts / loss_sum 8-byte aligned; the outputs need no
 * zeroing by the caller. */
int64_t rsx_binary_eval_workspace_bytes(int64_t R);
int rsx_binary_eval(const float* logit, const float* y, int64_t R, void* ws, int64_t ws_bytes, int64_t* counts,
                    double* loss_sum, int* flag, void* stream);

/* ---- A16 grouped validation: per-query NDCG@top and QueryAUC, csrc/group_eval.hip ------------------
 * The reference's ranker rows come in per-customer groups (utils/monitor/log_importer.py,
 * HMLogImporter.load_and_preprocess -> X_user, X_item, y, groups: the "CatBoost Group ID"); a reranker
 * is judged on the order inside each group. logit [R], y [R] fp32 in {0, 1}, group_id [R] int32 in
 * [0, 2^31), rows of a group anywhere in the input. For each distinct group g with rows I_g:
 *   P_g = #{y == 1}, N_g = |I_g| - P_g;
 *   U2_g = sum over the positives i of I_g of #{negative j in I_g : z_j < z_i} + #{... : z_j <= z_i}
 *     (twice the tie-aware Mann-Whitney U within the group, an exact integer); AUC_g = U2_g / (2 P_g N_g);
 *   DCG_g = the tie-averaged DCG@top (McSherry & Najork; sklearn's ndcg_score(ignore_ties=False)): with
 *     disc[p] = 1 / log2(p + 2) for the 0-based position p < top, else 0, and D[i] = sum_{p<i} disc[p],
 *     a tie group at the positions [s, e] of the group sorted by descending score with pos positives
 *     adds pos (D[min(e + 1, top)] - D[min(s, top)]) / (e - s + 1); IDCG_g = D[min(P_g, top)],
 *     NDCG_g = DCG_g / IDCG_g. Scores compare as reals: -0.0 and +0.0 tie.
 * D [top + 1] (double, device) is the caller's table D[0..top], 1 <= top <= 65536: the device takes no
 * logarithm. max_group_id: an upper bound of the ids known on the host (the sort then skips the bits
 * above it), -1 = unknown.
 * Per-group outputs, each sized R by the caller, their first G entries written, groups ascending:
 *   gid (int32), P, N, U2 (int64), dcg (double).
 * summary (int64 [5], 8-byte aligned): [0] = G, [1] = ndcg_groups = #{g : P_g > 0}, [2] = auc_groups =
 *   #{g : P_g > 0 and N_g > 0}, [3] = (double) ndcg_sum = sum of NDCG_g over the former, [4] = (double)
 *   auc_sum = sum of AUC_g over the latter; NDCG = ndcg_sum / ndcg_groups, QueryAUC = auc_sum / auc_groups.
 * flag [1] (int32): bit 0 = a logit is NaN or +-inf, bit 1 = a label is neither 0 nor 1, bit 2 = a
 *   group id is negative or above max_group_id; with a flag set the other outputs are unspecified
 *   (every access stays in bounds).
 * Key pass, radix sort of (group << 32 | ~score key, label), two passes over 2048-row tiles with a
 * one-workgroup carry pass after each, the per-group quotients; no step walks a group or a tie group,
 * so the cost does not depend on the groups' sizes. Integer sums and fixed-order double sums:
 * deterministic, no float atomics. 1 <= R < 2^31 (rsx_group_eval_workspace_bytes returns -1 outside
 * it, and is non-decreasing in R); ws 16-byte aligned, D / summary / P / N / U2 / dcg 8-byte aligned;
 * the outputs need no zeroing by the caller; everything is enqueued on stream. */
int64_t rsx_group_eval_workspace_bytes(int64_t R);
int rsx_group_eval(const float* logit, const float* y, const int32_t* group_id, int64_t R, int top, const double* D,
                   int64_t max_group_id, void* ws, int64_t ws_bytes, int64_t* summary, int32_t* gid, int64_t* P,
                   int64_t* N, int64_t* U2, double* dcg, int* flag, void* stream);

/* ---- §8f #3: GDCN reranker batch (utils/data_preprocessing/feature_processor.py:144-195) ----
 * rsx_reranker_batch replaces RerankerDataset.__getitem__ (:156-181) + reranker_collate_fn
 * (:184-191) for a batch of (user row uidx[b], item row iidx[b]) on device tables:
 *   dense [B, 12] = user_scaled[u] (3) | item_scaled[i] (6) | price gap, trend 1w, trend 1m
 *     (cross features in float64 from u_raw [U, 2] = (user_avg_price_log, total_cnt_log) and
 *     i_raw [I, 3] = (avg_item_price_log, velocity_1w, velocity_1m), rounded to fp32 once);
 *   cat [B] = u_cat[u]; target [B] = i_num[i];
 *   seq/mask [B, L]: the last min(len, max_len) ids of the user's CSR sequence (seq_off [U+1],
 *     seq_ids), right-padded with 0; mask = seq != 0. L = the batch maximum of min(len, max_len)
 *     (rsx_reranker_seq_lens gives the per-row lengths). */
int rsx_reranker_seq_lens(const int64_t* uidx, const int64_t* seq_off, int64_t B, int max_len, int64_t* lens,
                          void* stream);
int rsx_reranker_batch(const int64_t* uidx, const int64_t* iidx, int64_t B, const float* u_scaled, const double* u_raw,
                       const int64_t* u_cat, const float* i_scaled, const double* i_raw, const int64_t* i_num,
                       const int64_t* seq_off, const int64_t* seq_ids, int max_len, int64_t L, float* dense,
                       int64_t* cat, int64_t* target, int64_t* seq, int64_t* mask, void* stream);

/* ---- A9: item-tower RE path ------------------------------------------------------------
 * out[t] = LayerNorm((word[ids[t]] + type_row) + pos[tok_pos[t]]) * ln_w + ln_b over packed
 * tokens: BertEmbeddings (word + token type 0 + absolute position, LayerNorm, eval) for the
 * valid tokens of the RE fields only (HybridItemTower.forward, item_tower.py:247-262; their
 * masked mean ignores the padded ones). D in {256, 512, 768, 1024}. */
int rsx_embed3_ln(const float* word, int64_t ld_word, const float* pos, const float* type_row, const float* ln_w,
                  const float* ln_b, float eps, const int64_t* ids, const int64_t* tok_pos, int64_t T, int64_t D,
                  float* out, void* stream);

/* ---- DCN-V2 reranker ------------------------------------------------
 * CrossNet (temp_model/ranker_skelet.py:239-272): x_{l+1} = x_0 * (x_l . k_l + b_l) + x_l for L
 * layers (k_l [D], b_l [D]); writes x_L (x_out, nullable) and/or head_part[b] = x_L . w_head
 * (the cross half of RankingModel.final_head, :313-338). D % 4 == 0, D <= 512, L <= 8. */
int rsx_crossnet(const float* x, int64_t ldx, int64_t B, int D, int L, const float* const* kernels,
                 const float* const* biases, const float* w_head, float* x_out, float* head_part, void* stream);
/* Backward of rsx_crossnet: replaces autograd through CrossNet.forward (:258-272) and the cross
 * half of final_head when the RankingModel is trained (the reference never trains it: dead code
 * there; arithmetic pinned by the closed form in tests/dcn_train_ref.py). Upstream: dhead [B], the
 * gradient of head_part (with w_head [D]; together with dw_head [D] or all three NULL), and / or
 * dx_out [B, D], the gradient of x_L; both given means their sum. Per row, G = dx_{l+1}, l going
 * down: db_l += G x_0; ds = <G, x_0>; dk_l += ds x_l; dx_0 += G (s_l + b_l); G += ds k_l; dx =
 * dx_0 + G. Writes dk[l] [D], db[l] [D], dw_head [D] = sum_r dhead_r x_L and dx [B, D] (nullable:
 * training the ranker alone does not need it). One wave per row, the x_l recomputed in registers
 * (no [L, B, D] activations; x read once, dx written once); the parameter gradients as
 * per-workgroup partials in ws (>= rsx_crossnet_bwd_workspace_bytes, -1 for a refused shape), added
 * in workgroup order by a second launch: no atomics, the same bits every run. max_blocks: 0 = the
 * default grid cap (1024 workgroups of 4 rows), else a smaller cap (tests). Limits as rsx_crossnet;
 * B = 0 returns 0 and writes nothing. */
int64_t rsx_crossnet_bwd_workspace_bytes(int64_t B, int D, int L, int max_blocks);
int rsx_crossnet_bwd(const float* x, int64_t ldx, int64_t B, int D, int L, const float* const* kernels,
                     const float* const* biases, const float* w_head, const float* dhead, const float* dx_out,
                     float* const* dk, float* const* db, float* dw_head, float* dx, void* ws, int64_t ws_bytes,
                     int max_blocks, void* stream);
/* Logloss head of the RankingModel's training step (csrc/dcn_train.hip; replaces
 * binary_cross_entropy_with_logits on final_head(cat(cross, deep)) and its autograd, :313-338):
 * h2 [R, H = 128], w_d [128] = final_head.weight[D:], head_part [R] (rsx_crossnet's), bias [1]
 * (device: the host never reads it), y [R] -> logit [R] = head_part + <h2, w_d> + bias, g [R] =
 * (sigmoid(logit) - y) * (mean ? 1/R : 1), dh2 [R, 128] = g w_d (no ReLU mask: h2 is a GELU
 * output), dw_d [128] = sum_r g_r h2_r, dbias[0] = sum g, loss[0] (double) with
 * rsx_deepfm_train_head's row expression and fixed-order partials (ws >=
 * rsx_dcn_train_head_workspace_bytes(R)). */
int64_t rsx_dcn_train_head_workspace_bytes(int64_t R);
int rsx_dcn_train_head(const float* h2, int64_t H, const float* w_d, const float* head_part, const float* bias,
                       const float* y, int64_t R, int mean, float* logit, float* g, float* dh2, void* ws,
                       int64_t ws_bytes, double* loss, float* dbias, float* dw_d, void* stream);

/* ---- row gather / scatter / L2 normalise ---------------------------------------------
 * out[r] = src[idx[r]] (idx NULL => r), optionally F.normalize'd (eps) with norms saved:
 *   pretrained_lookup[item_ids]            tower_code/v1_usertower_train.py:760
 *   normalize(item_matrix)[target_ids]     v1_usertower_train.py:810-811 + v1_refine_usertower.py:833
 *   F.normalize(x, p=2, dim=-1)            v1_refine_usertower.py:504,584-585; v1_usertower_train.py:807
 * D in {64,128,256}. */
int rsx_gather_rows(const float* src, int64_t ld_src, const int64_t* idx, int64_t n, int64_t D, int normalize,
                    float eps, float* out, float* nrm_out, void* stream);
/* Backward scatter: dst[idx[r]] (op)= g_r where g = dy (or the F.normalize backward of dy
 * given y and norms). mode 0 store, 1 add (unique idx), 2 atomic add (duplicates allowed).
 * Rows whose index equals skip_idx are dropped (nn.Embedding padding_idx), -1 = none. */
int rsx_scatter_rows(const float* dy, const float* y, const float* nrm, const int64_t* idx, int64_t n, int64_t D,
                     int normalize, float eps, int mode, int64_t skip_idx, float* dst, int64_t ld_dst, void* stream);
/* Segmented row sums, the atomic-free scatter-add when the sort by destination is known:
 * dst[rows[u]] (+)= scale[0] * sum_{k in [seg_off[u], seg_off[u+1])} src[perm[k]] (scale
 * nullable = 1; perm nullable = identity; rows nullable = u; rows[u] == skip_row untouched;
 * rows unique). Used for the user tower's item-id embedding gradient
 * (v1_refine_usertower.py:447-459, nn.Embedding backward) with the sort built ahead of the
 * step, and for the per-user profile gradient (the broadcast of :498-505 over each user's
 * contiguous packed tokens); deterministic. */
int rsx_segment_sum_rows(const float* src, int64_t ld_src, const int64_t* perm, const int64_t* seg_off,
                         const int64_t* rows, int64_t nseg, int64_t D, const float* scale, int64_t skip_row,
                         float* dst, int64_t ld_dst, int accumulate, void* stream);
/* The same, and from the same pass raw[u] = the unscaled sum of segment u, dense [nseg, D], for every
 * segment (rows[u] == skip_row included): the item-id plan's per-item sums feed both the gated table
 * gradient (dst) and item_proj's weight gradient over the distinct items (raw). */
int rsx_segment_sum_rows2(const float* src, int64_t ld_src, const int64_t* perm, const int64_t* seg_off,
                          const int64_t* rows, int64_t nseg, int64_t D, const float* scale, int64_t skip_row,
                          float* dst, int64_t ld_dst, int accumulate, float* raw, int64_t ld_raw, void* stream);

/* The contrastive step's objective from its device loss sums, one launch instead of the
 * scalar tensor ops of train_user_tower_all_time (tower_code/v1_usertower_train.py:814-845):
 * main = s_main * inv_n (s_main nullable: 0), cl = s_un * inv_b + lambda_sup * s_sup / max(cnt, 1)
 * (s_sup nullable), total = main + lambda_cl * cl; total[1] and logs[3] = {total, main, cl} (separate
 * storage: a detached copy for logging / all-reduce). Backward: g3[3] = gradients of g * total w.r.t. s_main, s_un,
 * s_sup (cnt nullable when s_sup was). All device scalars. */
int rsx_loss_combine(const float* s_main, const float* s_un, const float* s_sup, const float* cnt, float inv_n,
                     float inv_b, float lambda_sup, float lambda_cl, float* total, float* logs, void* stream);
int rsx_loss_combine_bwd(const float* g, const float* cnt, float inv_n, float inv_b, float lambda_sup,
                         float lambda_cl, float* g3, void* stream);

/* The user tower's static profile (v1_refine_usertower.py:472-494) as one call per direction:
 *   u_g = sigmoid(static_gate); x = cat(E_j[id_j] * u_g[j] (j < ntab), relu(cont @ Wc^T + bc) * u_g[ntab]);
 *   out = dropout_p(gelu_erf(LayerNorm(x @ Wm^T + bm)))     [U, 128]
 * p[] pointer table (RSX_SP_*; table slots beyond ntab unused): ids int64 [U] and tables
 * [rows_j, dim_j] per table, static_gate [ntab + 1] (raw parameter), cont [U, C], Wc [P, C],
 * bc [P], Wm [128, K], bm [128], ln_w / ln_b [128]. dims[] = {U, ntab, C, P, K, src, rows[ntab],
 * dim[ntab], padding_idx[ntab]} with sum(dim) + P == K <= 128, C == 4, P == 16; the ids and cont
 * hold src rows and output row r reads input row r % src (U % src == 0: the contrastive step's two
 * dropout views share their users' inputs, so they are not duplicated). arena:
 * rsx_static_profile_arena_bytes(U), written by the forward and read by the backward; its first
 * int32 is an error flag the forward sets when an id lies outside [0, rows_j) (nn.Embedding's
 * IndexError: such an id reads row 0 and the backward scatters to row 0, never out of bounds; the
 * caller raises on the flag, ops.py _StaticProfile).
 * Backward: grads[] parallel to p[] (the ids' and cont's slots unused), every gradient WRITTEN
 * (padding rows 0); U > 0; ws: rsx_static_profile_bwd_workspace_bytes(U). Dropout mask
 * hash(seed, row * 128 + col). */
enum {
  RSX_SP_IDS = 0, RSX_SP_TABLES = 16, RSX_SP_GATE = 32, RSX_SP_CONT = 33, RSX_SP_WC = 34, RSX_SP_BC = 35,
  RSX_SP_WM = 36, RSX_SP_BM = 37, RSX_SP_LNW = 38, RSX_SP_LNB = 39, RSX_SP_N = 40
};
int64_t rsx_static_profile_arena_bytes(int64_t U);
int64_t rsx_static_profile_bwd_workspace_bytes(int64_t U);
int rsx_static_profile_fwd(const void* const* p, const int64_t* dims, float eps, float p_drop, uint64_t seed,
                           void* arena, int64_t arena_bytes, float* out, void* stream);
int rsx_static_profile_bwd(const void* const* p, const int64_t* dims, float p_drop, uint64_t seed, const void* arena,
                           const float* dout, float* const* grads, void* ws, int64_t ws_bytes, void* stream);

/* The step's tail: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) followed by
 * torch.optim.AdamW.step() (tower_code/v1_usertower_train.py:852-853, :495-496) in two launches.
 * n tensors, each fp32 contiguous with its gradient and both moments (exp_avg, exp_avg_sq);
 * clip[i] != 0 marks the tensors whose gradients form the clipped norm (and are scaled in
 * place by min(max_norm / (norm + 1e-6), 1), as clip_grad_norm_ does); the others (e.g. the item
 * matrix's parameter group) get the unclipped update. Per-tensor hyper-parameters lr,
 * weight_decay, beta1, beta2, eps; the step count AFTER this step's increment is step_dev[i][0]
 * (a device scalar, torch's fused/capturable state) when step_dev and step_dev[i] are non-null,
 * else step[i]. norm_out (device, nullable) receives the total norm. Deterministic: fixed-slot
 * partials reduced in a fixed order. ws: rsx_clip_adamw_workspace_bytes(n, numel, clip). */
int64_t rsx_clip_adamw_workspace_bytes(int n, const int64_t* numel, const int* clip);
int rsx_clip_adamw(int n, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const int64_t* numel, const int* clip, const float* step, const float* const* step_dev,
                   const double* lr, const double* weight_decay, const double* beta1, const double* beta2,
                   const double* eps, float max_norm, void* ws, int64_t ws_bytes, float* norm_out, void* stream);

/* Hard-negative mining: for each row i of u_norm [N,D] against the columns
 * i_norm [N,D] (both already L2-normalised), ignore column j when target_ids[j] ==
 * target_ids[i] or (i_norm[i].i_norm[j] > hnm_threshold and j != i); mining value =
 * (u_norm[i].i_norm[j]) / temperature (-inf when ignored). Writes the k largest per row (value
 * desc, column asc) as top_idx [N,k] int64 with their raw cosines top_cos [N,k], and avail [N]
 * int32 = number of columns not ignored. Two kernels: both products on the fp32 MFMA with the
 * mask applied in registers -> ONE masked N x ld fp32 workspace (ws, 16-B aligned,
 * >= rsx_hnm_workspace_bytes(N)) -> per-row radix select + sort in LDS. Replaces the N x N
 * cos / item_sim / mask tensors and torch.topk of v1_refine_usertower.py:641-669
 * (inbatch_hnm_corrected_loss_with_stats), :705-728 (inbatch_mixed_hnm_loss_with_stats),
 * :776-790 (full_batch_hard_emphasis_loss).
 * D in {64,128}; 1 <= k <= min(N, 4096); N <= rsx_hnm_max_rows() (one row's values live in LDS). */
int rsx_hnm_mine(const float* u_norm, const float* i_norm, const int64_t* target_ids, int64_t N, int64_t D,
                 int64_t k, float hnm_threshold, float temperature, void* ws, size_t ws_bytes, int64_t* top_idx,
                 float* top_cos, int32_t* avail, void* stream);
int64_t rsx_hnm_workspace_bytes(int64_t N);
int64_t rsx_hnm_max_rows(void);

/* ---- A2 + A3 + A4: the user tower's packed-token training program ---------------------
 * SASRecUserTower.forward in training mode over the contrastive step's packed tokens
 * (tower_code/v1_refine_usertower.py:434-510: item_proj, the gated embedding sum + position +
 * emb_ln + dropout, the norm_first TransformerEncoder stack, output_proj[0] over
 * cat(token, profile[user]), LayerNorm + GELU, output_proj[3], F.normalize) and its backward,
 * each as ONE call that launches the same kernels as the per-op entry points above, in the
 * same order with the same arguments (bit-identical results), from the library instead of
 * one host-language call per op. Shapes: d_model 128, 4 heads of 32, feed-forward 256,
 * bf16x3 token linears and attention, L <= 64, 1..8 layers. The static profile rows
 * (:472-494) are an input (computed by the caller, whose autograd takes their gradient).
 *
 * p[] (device pointers, RSX_TW_* order; layer l's 12 parameters at RSX_TW_LAYER0 + 12 l, the
 * output head's 6 after the last layer):
 *   inputs  pretrained rows [T,128], six id arrays int64 [T] (item, time, type, colour,
 *           graphic, section), token positions int64 [T], key-pad flags uint8 [T], user token
 *           offsets int32 / int64 [U+1], token user int64 [T], seq gate [6] (sigmoid(seq_gate)
 *           * s_mask), profile rows [U,128], the item-id gradient plan (perm [T], chunk bounds
 *           [C+1], chunk ids [C], chunk offsets per id [Uq+1], ids [Uq]; ops.sort_segments),
 *           the tokens' distinct-item slots int64 [T] (RSX_TW_UIDX, nullable). With the slots
 *           (and C > 0) the pretrained rows are [Uq,128], one per distinct item in the plan's id
 *           order: item_proj runs over those Uq rows, the embedding stage reads row slot[t] of
 *           its output for token t, and item_proj's weight / bias gradient comes from the
 *           per-item sums of the embedding stage's per-token input gradient (the plan's segment
 *           sums, ungated) against the same Uq rows; the pretrained rows' gradient must then be
 *           null. Without the slots: one pretrained row per token.
 *   params  item_proj w/b, the six tables, pos_emb, emb_ln w/b; per layer norm1 w/b,
 *           in_proj w/b, out_proj w/b, norm2 w/b, linear1 w/b, linear2 w/b; output_proj[0] w/b,
 *           output_proj[1] w/b, output_proj[3] w/b
 * dims[]  T, U, pos rows (max_len), layers, C, Uq, rows of the six tables, tail B, tail T1
 * tail    (dims[12] = B > 0, round 5) the packed rows are two views of B users each (U = 2B,
 *         T = 2 T1, view 2's token t at row T1 + t) and p[rsx_tower_n_ptrs - 1] holds view 1's
 *         "last" token of each user [B] int64: the last layer past its attention and the output
 *         head run on the R = T1 + B rows the contrastive step reads (all of view 1, then view
 *         2's last row of user b at row T1 + b), `out` is [R,128] and the backward expands their
 *         gradients to every row (the dropped rows' are zero). dims[12] = 0: every row.
 * fargs[] p_drop, emb_ln eps, per layer norm1 eps, norm2 eps, output LayerNorm eps
 * seeds[] 1 + 4 x layers dropout seeds: embedding, then per layer attention, out-projection
 *         add, feed-forward, closing add (the per-op entry points' seed order)
 * arena   saved activations (rsx_tower_arena_bytes; pv_rows = the pretrained rows given: T, or Uq
 *         with the slots), read by the backward; out [T or R,128] (the backward reads it too: the
 *         F.normalize backward).
 * grads[] parallel to p[]: params' gradients written, except the embedding stage's (six
 *         tables, pos_emb, emb_ln w/b) and the seq gate's, which are ACCUMULATED (caller
 *         zeroes); the profile's [U,128] written; the pretrained rows' nullable (written).
 * ws      backward scratch (rsx_tower_bwd_workspace_bytes); it includes a [C,128] buffer for the
 *         per-item sums of the embedding stage's input gradient (Uq <= C rows used, slots form). */
enum {
  RSX_TW_PV = 0, RSX_TW_IDS = 1, RSX_TW_TOK_POS = 7, RSX_TW_TOK_PAD = 8, RSX_TW_SEG32 = 9, RSX_TW_SEG64 = 10,
  RSX_TW_TOK_USER = 11, RSX_TW_GATE = 12, RSX_TW_PROFILE = 13, RSX_TW_ITEMSEG = 14, RSX_TW_UIDX = 19,
  RSX_TW_ITEM_PROJ = 20, RSX_TW_TABLES = 22, RSX_TW_POS = 28, RSX_TW_EMB_LN = 29, RSX_TW_LAYER0 = 31
};
int64_t rsx_tower_n_ptrs(int layers);
int64_t rsx_tower_arena_bytes(int64_t T, int64_t U, int layers, int64_t pv_rows);
int64_t rsx_tower_bwd_workspace_bytes(int64_t T, int64_t U, int64_t L, int layers, int64_t C);
int rsx_tower_fwd(const void* const* p, const int64_t* dims, const float* fargs, const uint64_t* seeds, void* arena,
                  int64_t arena_bytes, float* out, void* stream);
int rsx_tower_bwd(const void* const* p, const int64_t* dims, const float* fargs, const uint64_t* seeds,
                  const void* arena, const float* out, const float* dout, void* const* grads, void* ws,
                  int64_t ws_bytes, void* stream);

/* ---- LightGCL: graph propagation and the low-rank view (csrc/lightgcl.hip) -------------
 * fp32, no float atomics, every sum in a fixed order: each call is bit-reproducible.
 *
 * rsx_spmm_norm: Y = alpha (R + A^ X) with A^ = diag(dinv) B diag(dinv), B the binary symmetric
 * bipartite adjacency in CSR (row_ptr int64 [n+1], col int32 [nnz], ascending within a row) and
 * dinv [n] = deg^-1/2 (0 for an isolated node). Replaces torch.sparse.mm(self.adj, x) of
 * gnn_model/v1_lightgcl.py:171 (the normalised values of :123-135 are never stored) and, A^ being
 * symmetric, its autograd backward; with R and alpha also the stack / mean of :166-173 (Horner).
 *   y_r = alpha (R_r + dinv_r sum_{c in row r} dinv_c x_c), neighbours in CSR order.
 * X [n, D] (ldx), R [n, D] (ldr) nullable, D in {64, 128}; Y must not alias X.
 * rows NULL (then n_rows == 0): every row, Y [n, D] (ldy). A row with more than rsx_spmm_norm_chunk_len() neighbours is
 * cut into chunks of that length (the last one shorter) summed by separate lane groups into the
 * partial slots ws [n_chunks, D], which a second pass adds in chunk order. The plan is built once with
 * the graph: long_rows int64 [n_long] ascending, part_off int64 [n_long + 1] (row l owns the slots
 * [part_off[l], part_off[l+1])), chunk_beg / chunk_end int64 [n_chunks] (CSR positions of each slot's
 * neighbours); ws >= rsx_spmm_norm_workspace_bytes(n_chunks, D).
 * rows int64 [n_rows]: only those destinations, into the dense Y [n_rows, D] (ldy); repeats allowed, a
 * row outside [0, n) gives zeros; R is still indexed by the graph row. The plan and ws are not used:
 * a long row's chunks are summed one after the other by its lane group, the same arithmetic.
 * Workgroup b takes the rsx_spmm_norm_rows_per_workgroup() destinations from b times that on. */
int64_t rsx_spmm_norm_chunk_len(void);
int64_t rsx_spmm_norm_rows_per_workgroup(void);
int64_t rsx_spmm_norm_workspace_bytes(int64_t n_chunks, int64_t D);
int rsx_spmm_norm(const int64_t* row_ptr, const int32_t* col, const float* dinv, int64_t n, const float* X,
                  int64_t ldx, const float* R, int64_t ldr, int64_t D, float alpha, const int64_t* rows,
                  int64_t n_rows, const int64_t* long_rows, const int64_t* part_off, const int64_t* chunk_beg,
                  const int64_t* chunk_end, int64_t n_long, int64_t n_chunks, void* ws, int64_t ws_bytes,
                  float* Y, int64_t ldy, void* stream);
/* P [q, D] = V^T X over n rows, V [n, q] (ldv), X [n, D] (ldx), 1 <= q <= 8, D in {64, 128}: one
 * streaming pass, replacing torch.matmul(self.V.t(), x_g) of gnn_model/v1_lightgcl.py:180. Workgroup b
 * sums the tiles b, b + G, ... of rsx_lowrank_rows_per_workgroup() rows into slot b of ws (G = min(tiles,
 * 512), a function of n alone); a second kernel adds the slots in slot order. n == 0 gives zeros.
 * ws >= rsx_lowrank_proj_workspace_bytes(n, q, D). */
int64_t rsx_lowrank_rows_per_workgroup(void);
int64_t rsx_lowrank_proj_workspace_bytes(int64_t n, int64_t q, int64_t D);
int rsx_lowrank_proj(const float* V, int64_t ldv, const float* X, int64_t ldx, int64_t n, int64_t q, int64_t D,
                     void* ws, int64_t ws_bytes, float* P, void* stream);
/* Y [n, D] (ldy) += V W, V [n, q] (ldv), W [q, D] contiguous, the terms of a row added for j = 0..q-1:
 * the dense rank-q update torch.matmul(self.U, temp) of gnn_model/v1_lightgcl.py:182 as its own
 * streaming pass (not fused into the last rsx_spmm_norm: the two views are separate outputs). */
int rsx_lowrank_update(const float* V, int64_t ldv, const float* W, int64_t n, int64_t q, int64_t D, float* Y,
                       int64_t ldy, void* stream);

/* ---- Distillation of dot-product scores into unit vectors (csrc/distill.hip) -----------
 * Replaces gnn_model/distill_mag_to_cos_l2.py: MagnitudeEncoder = Linear(64, 128) + LeakyReLU(slope) +
 * Dropout(p) + Linear(128, 64) + F.normalize (:16-35), and one step of train_projector (:63-103) as two
 * launches. w1 [128, 64], b1 [128], w2 [64, 128], b2 [64], logit_scale [1], all on the device, 16-B
 * aligned matrices. Exact fp32 products (f32-input MFMA), no float atomics, every sum in a fixed
 * order: each call is bit-reproducible. With the stacked rows X = [U[users]; I[items]] ([2B, 64]):
 *   P = X W1^T + b1; A = P > 0 ? P : slope P; H = A keep / (1 - p), keep from (seed, r 128 + c) over the
 *   stacked row r; Z = H W2^T + b2; n = max(|Z_r|, eps); Y = Z / n; s_k = <Y_k, Y_{B+k}> exp(logit_scale);
 *   t_k = <X_k, X_{B+k}>; loss = mean_k (s_k - t_k)^2; no gradient to X.
 * rsx_distill_rows_per_workgroup(): the pairs of one tile T (a tile of the forward is 2 T rows).
 * rsx_distill_slots(B): the workgroups and partial slots of a step, min(ceil(B / T), 256); workgroup g
 * takes the tiles g, g + slots, ... ws >= rsx_distill_workspace_bytes(B), 8-B aligned.
 *
 * rsx_magnitude_encode: Y [N, 64] (ldy) = the forward of X [N, 64] (ldx) without dropout; the same
 * arithmetic as the step's forward at p = 0, bit for bit. N == 0 does nothing.
 *
 * rsx_distill_grads: gather, forward, loss and backward of the B pairs (users[k], items[k]) (int64) over
 * the tables [n_users, 64] (ldu) / [n_items, 64] (ldi) into ws: per workgroup one slot of the 16,577
 * gradients in parameter order (w1, b1, w2, b2, logit_scale) and a double loss partial. A pair with an
 * id outside its table sets flag[0] = 1 (the caller zeroes it) and contributes nothing; the mean still
 * divides by B. Nullable outputs: student_scores / teacher_scores [B] (s_k, t_k) and rows_out [2B, 64]
 * (Y, 16-B aligned, for tests).
 *
 * rsx_distill_apply: every gradient = its slots added in slot order; grads [16,577] (nullable) and
 * loss [1] double (nullable) written; update != 0 applies torch.optim.Adam's step number `step`
 * (>= 1; no weight decay, bias-corrected, double scalars, float state) to the five parameters with the
 * flat moments exp_avg / exp_avg_sq [16,577] in parameter order. */
int64_t rsx_distill_rows_per_workgroup(void);
int64_t rsx_distill_slots(int64_t B);
int64_t rsx_distill_workspace_bytes(int64_t B);
int rsx_magnitude_encode(const float* X, int64_t ldx, int64_t N, const float* w1, const float* b1,
                         const float* w2, const float* b2, float slope, float eps, float* Y, int64_t ldy,
                         void* stream);
int rsx_distill_grads(const float* user_table, int64_t ldu, int64_t n_users, const float* item_table,
                      int64_t ldi, int64_t n_items, const int64_t* users, const int64_t* items, int64_t B,
                      const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* logit_scale, float slope, float p_drop, uint64_t seed, float eps, void* ws,
                      int64_t ws_bytes, float* student_scores, float* teacher_scores, float* rows_out,
                      int32_t* flag, void* stream);
int rsx_distill_apply(const void* ws, int64_t ws_bytes, int64_t B, float* w1, float* b1, float* w2, float* b2,
                      float* logit_scale, float* exp_avg, float* exp_avg_sq, float* grads, double* loss,
                      int update, double lr, double beta1, double beta2, double eps, int64_t step,
                      void* stream);

/* ---- Late fusion of two retrievers: pool, fuse, hits (csrc/ensemble.hip) ---------------
 * Replaces the per-batch body of tower_code/mined_inference.py's evaluators:
 * evaluate_weighted_score_ensemble (:1103-1189), evaluate_rrf_ensemble (:1330-1410) and the hit test
 * of evaluate_multi_vector_ensemble (:926-953). Floats compare through the score key (-0.0 and +0.0
 * tie); every input float must be finite (a NaN or an infinity is ordered by its bits, not refused).
 * No float atomics; each call is bit-reproducible.
 *
 * rsx_select_topk_rows: the k largest of each row of S [Q, N] (row stride ld >= N floats), replacing
 * torch.topk(scores, k=pool_k, dim=1) of :1104 / :1108. 1 <= k <= min(N, 2048), N <= 2^30. idx [Q, k]
 * int32 and val [Q, k] in the order (value descending, index ascending): among equal values the lower
 * indices are taken, and come first. One workgroup per row: radix select of the k-th key (four
 * 8-bit passes over the row), a counting and a collecting pass, a sort of the k pairs in LDS.
 *
 * rsx_fuse_rank: per user q the fusion of retrievers a and b over the pool cand [Q, C] int32 (corpus
 * rows in [0, NI), 1 <= C <= 2048, the reference's cat([pool_a, pool_b]), duplicates kept). ua [Q, Da]
 * (ldua), Ia [NI, Da] (ldia), ub [Q, Db] (ldub), Ib [NI, Db] (ldib); Da, Db in {64, 128}; rows 16-B
 * aligned, strides multiples of 4. wa / wb [A] (HOST arrays, A <= 32): the weights of each alpha, for
 * the reference wa = float(alpha), wb = float(1.0 - alpha). ks [nK] (HOST, nK <= 16, ascending,
 * 1 <= ks[0], ks[nK-1] <= cut); cut in [1, C], for the reference min(C, max_k + 20) (:1170).
 * truth_off int64 [Q+1] / truth int32 [n_truth]: user q's items truth[truth_off[q] .. truth_off[q+1]),
 * ascending and distinct, any length (offsets are clamped into [0, n_truth]).
 * The fp32 operations, in this order and uncontracted:
 *   sa[c] = <ua_q, Ia[cand[c]]>, sb[c] = <ub_q, Ib[cand[c]]>        (summation order unspecified)
 *   RSX_FUSE_MINMAX  na = (sa - min sa) / ((max sa - min sa) + 1e-9f), likewise nb            (:1139-1145)
 *   RSX_FUSE_RRF     ra = 0-based rank of entry c by (key(sa) descending, c ascending),
 *                    na = 1.0f / ((k_rrf + ra) + 1.0f), likewise nb                          (:1358-1380)
 *   per alpha a      f = wa[a] * na + wb[a] * nb (each product rounded, then the sum); the entries in
 *                    the order (key(f) descending, c ascending); the first `cut` of them; their corpus
 *                    ids; later repeats of an id dropped (:1170-1183). The cut precedes the removal
 *                    of repeats, as in the reference: an item first seen beyond `cut` is a miss.
 *   hits [Q, A] int32: bit j set when one of the first ks[j] ids of that list is in the user's truth.
 * Optional outputs (nullable): lists [Q, A, ks[nK-1]] int32, the list's head padded with -1; sa / sb
 * [Q, C]. A pool entry outside [0, NI) sets flag[0] |= 1 (int32, the caller zeroes it) and scores 0.
 *
 * rsx_first_hit: out [Q] int32 = the smallest j with lists[q, j] (int32 [Q, K], row stride ld) in user
 * q's truth (CSR as above), or K: the hit test `actual & set(indices[u, :n])` of :944-952 is
 * out[q] < n. */
enum { RSX_FUSE_MINMAX = 0, RSX_FUSE_RRF = 1 };
int rsx_select_topk_rows(const float* S, int64_t ld, int64_t Q, int64_t N, int64_t k, int32_t* idx, float* val,
                         void* stream);
int rsx_fuse_rank(const float* ua, int64_t ldua, const float* Ia, int64_t ldia, int64_t Da, const float* ub,
                  int64_t ldub, const float* Ib, int64_t ldib, int64_t Db, int64_t Q, int64_t NI,
                  const int32_t* cand, int64_t C, const float* wa, const float* wb, int A, int mode, float k_rrf,
                  int cut, const int32_t* ks, int nK, const int64_t* truth_off, const int32_t* truth,
                  int64_t n_truth, int32_t* hits, int32_t* lists, float* sa, float* sb, int32_t* flag,
                  void* stream);
int rsx_first_hit(const int32_t* lists, int64_t ld, int64_t Q, int64_t K, const int64_t* truth_off,
                  const int32_t* truth, int64_t n_truth, int32_t* out, void* stream);

/* ---- HybridUserTower inference: adapter, sequence input, fusion (csrc/hybrid.hip) --------
 * The eval forward of tower_code/mined_inference.py's ParallelAdapter (:582-602), the sequence input
 * of HybridUserTower.forward (:687-695) and SequenceCentricFusion with the two normalisations around
 * it (:703-710). Exact fp32 products (f32-input MFMA), no float atomics, bit-reproducible; a row's
 * result does not depend on the rows around it. All float rows 16-B aligned.
 *
 * rsx_hybrid_adapter_fwd: R rows; row r takes id = ids[r] (int64, repeats allowed) or, with ids NULL,
 * id = first_row + r (first_row + R <= min(Nc, Ng)), c = content[id] (Dc = 128 floats, row stride ldc),
 * g = gnn[id] (Dg = 64, ldg), and
 *   m = (gelu(LN(wc c + bc; lnc_w, lnc_b, ln_eps)) + c) + gelu(LN(wg g + bg; lng_w, lng_b, ln_eps))
 * with wc [128, 128], wg [128, 64] dense, erf GELU, biased variance. Outputs [R, 128], each nullable
 * (at least one given): merged = m; unit = m / max(|m|, eps); seq_in = m * scale + time_tab[min(deltas[r],
 * 1000)] (the product rounded, then the sum; deltas int64 [R], time_tab [1001, 128] dense). An id outside
 * [0, min(Nc, Ng)) or a negative delta sets flag[0] = 1 (int32, zeroed by the caller) and reads row 0.
 *
 * rsx_hybrid_seq_gather: seq_in[t] = merged[ids[t] - first_row] * scale + time_tab[min(deltas[t], 1000)]
 * over T tokens from a table merged [Nm, D = 128] (dense) of rsx_hybrid_adapter_fwd: the same bits as its
 * seq_in. An id in [0, first_row) reads a zero row (the padding id of a table that starts at row 1); a
 * negative id, an id >= first_row + Nm or a negative delta sets flag[0] = 1.
 *
 * rsx_hybrid_fuse_fwd: seq_out [B * L, D = 128] dense, 1 <= L <= 64. The rows fused are rows[0 .. n_rows)
 * (int64 token rows in [0, B L); outside sets flag[0] = 1 and reads row 0) or, with rows NULL, all B L
 * rows in order; row i of the outputs belongs to token row s = rows[i], user u = s / L:
 *   v = x / max(|x|, eps); g = sigmoid(w2 gelu(w1 v + b1) + b2)     w1 [hidden = 64, 128], w2 [2, 64]
 *   f = (v + g0 u_gnn[u]) + g1 u_meta[u]                             u_gnn, u_meta [B, 128] dense
 *   out = y / max(|y|, eps), y = LN(f; ln_w, ln_b, ln_eps)
 * out [n, 128]; v_seq [n, 128] = v (nullable); gate_mean [2] float (nullable) = the means of g0 and g1
 * over the n rows: per-workgroup double partials in ws (>= rsx_hybrid_fuse_slots(n) * 16 bytes, 8-B
 * aligned; the slot count depends on n alone) added in slot order by a second launch. */
int rsx_hybrid_adapter_fwd(const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn, int64_t ldg,
                           int64_t Ng, int64_t Dg, const int64_t* ids, int64_t first_row, int64_t R,
                           const float* wc, const float* bc, const float* lnc_w, const float* lnc_b,
                           const float* wg, const float* bg, const float* lng_w, const float* lng_b, float ln_eps,
                           float eps, const int64_t* deltas, const float* time_tab, float scale, float* merged,
                           float* unit, float* seq_in, int32_t* flag, void* stream);
int rsx_hybrid_seq_gather(const float* merged, int64_t Nm, int64_t D, int64_t first_row, const int64_t* ids,
                          const int64_t* deltas, int64_t T, const float* time_tab, float scale, float* seq_in,
                          int32_t* flag, void* stream);
int64_t rsx_hybrid_fuse_slots(int64_t n);
int rsx_hybrid_fuse_fwd(const float* seq_out, int64_t B, int64_t L, int64_t D, const int64_t* rows, int64_t n_rows,
                        const float* u_gnn, const float* u_meta, const float* w1, const float* b1, int64_t hidden,
                        const float* w2, const float* b2, const float* ln_w, const float* ln_b, float ln_eps,
                        float eps, float* out, float* v_seq, float* gate_mean, void* ws, int64_t ws_bytes,
                        int32_t* flag, void* stream);

/* ---- HybridUserTower with gradients: the adapter's and the fusion's training forward and backward ----
 * rsx_hybrid_adapter_train_fwd: rsx_hybrid_adapter_fwd over ids [R] (required) with the two Dropout(p_drop)
 * after the GELUs (tower_code/mined_inference.py:582-602 in training): m = (drop_c(gelu(LN(Wc c + bc))) + c) +
 * drop_g(gelu(LN(Wg g + bg))), keep = hash(seed, r * 128 + col) >= p_drop 2^32 (seed_c, seed_g). Writes
 * merged and / or seq_in (nullable, one required) and, for the backward, the gathered rows xc [R, 128],
 * xg [R, 64] and the pre-LayerNorm products zc, zg [R, 128] (1,792 bytes per row).
 * rsx_hybrid_adapter_bwd: from dy [R, 128] = d seq_in (gscale = the forward's scale) or d merged (gscale = 1):
 * dzc, dzg [R, 128] = the gradients of the two products (dWc = dzc^T xc, dbc = column sums of dzc; so Wg, bg);
 * dc [R, 128] = gscale dy + dzc Wc, dg [R, 64] = dzg Wg (exact fp32 MFMA), the gradients of the gathered rows;
 * dln [4][128] = d lnc_w, d lnc_b, d lng_w, d lng_b, per-workgroup partials in ws
 * (rsx_hybrid_adapter_bwd_workspace_floats(R) floats) added in workgroup order. The gradient of the time
 * rows is dy itself. No atomics: identical inputs give identical bits.
 * rsx_hybrid_fuse_train_fwd: rsx_hybrid_fuse_fwd over all B L rows with each token's own Dropout(p_drop)
 * masks over its copies of the two projected rows (the reference applies gnn_proj / meta_proj to the expanded
 * [B, L, 128] tensors, :514-577): f = v + g0 drop_a(u_gnn[u]) + g1 drop_b(u_meta[u]), keep index token_row *
 * 128 + col (seed_a, seed_b). The gate means are those of the gates, before dropout.
 * rsx_hybrid_fuse_bwd: from dout [B L, 128] and dv (gradient of v_seq, nullable), recomputing the forward
 * from its inputs: dx [B L, 128] = d seq_out; dpre [B L, 64] = the gradient of the gate's pre-activations
 * (dW1 = dpre^T v_seq, db1 = its column sums); du_gnn, du_meta [B, 128] = each user's L token rows added in
 * position order; dsmall [386] = d ln_w [128] | d ln_b [128] | d W2 [2][64] | d b2 [2]. A row at the eps
 * floor of either normalise is divided by eps (a constant): an all-zero seq_out row with zero upstream
 * gradients gives exact zeros. ws: rsx_hybrid_fuse_bwd_workspace_floats(B, L) floats, 16-byte aligned. */
int rsx_hybrid_adapter_train_fwd(const float* content, int64_t ldc, int64_t Nc, int64_t Dc, const float* gnn,
                                 int64_t ldg, int64_t Ng, int64_t Dg, const int64_t* ids, int64_t R, const float* wc,
                                 const float* bc, const float* lnc_w, const float* lnc_b, const float* wg,
                                 const float* bg, const float* lng_w, const float* lng_b, float ln_eps,
                                 const int64_t* deltas, const float* time_tab, float scale, float p_drop,
                                 uint64_t seed_c, uint64_t seed_g, float* merged, float* seq_in, float* xc, float* xg,
                                 float* zc, float* zg, int32_t* flag, void* stream);
int64_t rsx_hybrid_adapter_bwd_workspace_floats(int64_t R);
int rsx_hybrid_adapter_bwd(const float* dy, float gscale, int64_t R, const float* zc, const float* zg, const float* wc,
                           const float* wg, const float* lnc_w, const float* lnc_b, const float* lng_w,
                           const float* lng_b, float ln_eps, float p_drop, uint64_t seed_c, uint64_t seed_g, float* dzc,
                           float* dzg, float* dc, float* dg, float* dln, float* ws, int64_t ws_floats, void* stream);
int rsx_hybrid_fuse_train_fwd(const float* seq_out, int64_t B, int64_t L, const float* u_gnn, const float* u_meta,
                              const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_w,
                              const float* ln_b, float ln_eps, float eps, float p_drop, uint64_t seed_a,
                              uint64_t seed_b, float* out, float* v_seq, float* gate_mean, void* ws, int64_t ws_bytes,
                              int32_t* flag, void* stream);
int64_t rsx_hybrid_fuse_bwd_workspace_floats(int64_t B, int64_t L);
int rsx_hybrid_fuse_bwd(const float* seq_out, int64_t B, int64_t L, const float* u_gnn, const float* u_meta,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_w,
                        const float* ln_b, float ln_eps, float eps, float p_drop, uint64_t seed_a, uint64_t seed_b,
                        const float* dout, const float* dv, float* dx, float* dpre, float* du_gnn, float* du_meta,
                        float* dsmall, float* ws, int64_t ws_floats, void* stream);

/* ---- A17 oblivious-tree boosting: the rerank stage's classifier, csrc/gbdt.hip ------------------------
 * The reference reranks with CatBoostClassifier(iterations=1000, learning_rate=0.05, depth=6, Logloss)
 * over the FeatureEngineer columns (temp_model/ranker_skelet.py:95-149). CatBoost's GPU trainer is CUDA-only
 * and its file format and ordered boosting are not reproduced: the model below is self-contained.
 *   bins   uint8 [F, R], F <= 32 features, 1 <= R < 2^31 rows. A numeric column has at most 254 ascending
 *          fp32 borders and bin = #{borders < x} (NaN: 0); a categorical column's bin is its code (0 = unknown).
 *   F0     = log(p / (1 - p)) of the training base rate. Per tree: g = y - sigmoid(F), h = sigmoid(F)(1 -
 *          sigmoid(F)) in fp32 (the sigmoid itself evaluated in fp64 and rounded once), quantised once to qg =
 *          llrint(g 2^30), qh = llrint(h 2^30) (round half to even; both fit an int32). Every sum of g or h is
 *          an exact int64 sum of these.
 *   level d < depth <= 6: hist [2^d, F, 256, 2] int64 = the sums of (qg, qh) per (leaf, feature, bin). The
 *          candidate (f, b), b < n_bins[f], sends bin > b right (numeric) or bin == b right (categorical) and
 *          scores sum over the leaves in ascending order of G_L^2 / (H_L + l2) + G_R^2 / (H_R + l2) in fp64 with
 *          G = (double)sum 2^-30. The level takes the argmax, ties to the lowest f, then the lowest b. No
 *          validity rule: a candidate with an empty side scores the parent term (a real split may score
 *          below it, each side paying l2; the level then leaves the leaves as they are). leaf = 2 leaf + right.
 *   leaf values: (float)(lr (G / (H + l2))) in fp64 from the children's exact sums (an empty leaf: 0), then
 *          F += value[leaf] in fp32. Prediction adds F0 and then the values in tree order in fp32, so it
 *          equals the training approximant after the same number of trees bit for bit.
 * Integer LDS and global atomics only: every output has the same bits every run. Nothing synchronises with
 * the host; splits are read from device memory. flag (int32, OR-ed): bit 0 = a leaf index >= n_leaves
 * (rsx_gbdt_histogram skips the row), bit 1 = a split feature >= F or a leaf index >= n_leaves
 * (rsx_gbdt_apply_split uses feature 0 / the index masked); every access stays in bounds. */
/* trees predict_k stages in LDS at a time; the row slabs rsx_gbdt_histogram cuts R rows of F features into */
int64_t rsx_gbdt_tree_chunk(void);
int64_t rsx_gbdt_histogram_slabs(int64_t R, int F);
/* x [Fn, R] fp32 -> bins rows 0..Fn-1 of a [*, R] uint8 matrix; borders [Fn, 256] ascending, the first
 * n_borders[j] <= 254 (int32, device) of row j valid. */
int rsx_gbdt_bin(const float* x, const float* borders, const int* n_borders, int64_t R, int Fn, uint8_t* bins,
                 void* stream);
/* F, y [R] fp32 -> qg, qh [R] int32. */
int rsx_gbdt_grad(const float* F, const float* y, int64_t R, int* qg, int* qh, void* stream);
/* leaf uint8 [R] < n_leaves in {1, 2, 4, 8, 16, 32} -> hist [n_leaves, F, 256, 2] int64 (zeroed here). */
int rsx_gbdt_histogram(const uint8_t* bins, const uint8_t* leaf, const int* qg, const int* qh, int64_t R, int F,
                       int n_leaves, int64_t* hist, int* flag, void* stream);
/* is_cat uint8 [F], n_bins int32 [F] (device), l2 > 0, ws 16 F bytes (16-byte aligned) -> split int32 [2] =
 * (f, b) and, when score is not NULL, the winning score. */
int rsx_gbdt_best_split(const int64_t* hist, const uint8_t* is_cat, const int* n_bins, int F, int n_leaves, double l2,
                        void* ws, int* split, double* score, void* stream);
/* leaf = 2 leaf + right in place. hist not NULL marks the last level (hist = that level's histogram): then
 * leaf_sums int64 [2 n_leaves, 2] and leaf_values fp32 [2 n_leaves] are written and Fx [R] += value[leaf]. */
int rsx_gbdt_apply_split(const uint8_t* bins, int64_t R, int F, const int* split, const uint8_t* is_cat, int n_leaves,
                         uint8_t* leaf, const int64_t* hist, double lr, double l2, int64_t* leaf_sums,
                         float* leaf_values, float* Fx, int* flag, void* stream);
/* One whole tree on Fx [R] (the stages above enqueued back to back: 2 + 4 depth kernels and 1 + depth fills): qg, qh
 * int32 [R], leaf uint8 [R], hist int64 [2^(depth-1) F 512] and ws (16 F bytes) are scratch; splits int32
 * [depth, 2], leaf_sums int64 [2^depth, 2] and leaf_values fp32 [2^depth] are the tree. */
int rsx_gbdt_tree(const uint8_t* bins, const float* y, int64_t R, int F, const uint8_t* is_cat, const int* n_bins,
                  int depth, double lr, double l2, float* Fx, int* qg, int* qh, uint8_t* leaf, int64_t* hist, void* ws,
                  int* splits, int64_t* leaf_sums, float* leaf_values, int* flag, void* stream);
/* ---- QuerySoftMax: the listwise objective of the oblivious-tree model, csrc/gbdt_rank.hip ----
 * Rows carry y in {0, 1} and a group (the reference's per-customer ranker rows: utils/monitor/log_importer.py
 * returns X_user, X_item, y, groups). They are given in group order: row_group int32 [R] is the dense group
 * index of each row (ascending), goff int32 [G + 1] the groups' offsets, 1 <= G <= R. Group q has the rows
 * I_q and the fp32 approximant a; the base score is F0 = 0.
 *   per group: m_q = max a_i over I_q (fp32, exact);
 *          E_i = llrint(exp((double)a_i - (double)m_q) 2^32), round half to even, an int64 in [0, 2^32];
 *          Z_q = sum E_i, an exact int64 sum in any order (no overflow for R < 2^31);
 *          p_i = (float)((double)E_i / (double)Z_q);   S_q = #{i in I_q : y_i = 1}.
 *   per row: S_q = 0 -> g_i = h_i = 0 (the group carries no signal); else t_i = y_i ? (float)(1.0 / S_q) : 0,
 *          g_i = t_i - p_i, h_i = p_i (1 - p_i) in fp32: the negative gradient and the Hessian diagonal of
 *          L_q = -(1 / S_q) sum_{y_i = 1} log softmax(a)_i, so every group with a positive weighs the same.
 *          qg = llrint(g 2^30), qh = llrint(h 2^30) as rsx_gbdt_grad writes them (|g| <= 1, h <= 1/4: both
 *          fit an int32). From there the tree is exactly the tree above.
 *   monitoring: L_q = -(1 / S_q) sum_{y_i = 1} [(double)a_i - (double)m_q - log((double)Z_q 2^-32)] in fp64;
 *          the metric QuerySoftMax = sum_{S_q > 0} L_q / #{q : S_q > 0}.
 * The maximum, Z and S are order-free (a maximum of ordered integer keys, integer sums), so the gradients do
 * not depend on the order of the rows within or across groups and every run gives the same bits. No thread
 * walks a group: the cost does not depend on the group sizes. Integer atomics only. A row whose row_group is
 * outside [0, G) gets g = h = 0 and no access leaves its array. */
/* bytes of the workspace ws of the three entries below (-1 unless 1 <= R < 2^31 and 1 <= G <= R) */
int64_t rsx_gbdt_grad_query_softmax_workspace_bytes(int64_t R, int64_t G);
/* F, y [R] fp32, row_group [R], goff [G + 1] int32 -> qg, qh [R] int32; ws 16-byte aligned. */
int rsx_gbdt_grad_query_softmax(const float* F, const float* y, const int* row_group, const int* goff, int64_t R,
                                int64_t G, void* ws, int64_t ws_bytes, int* qg, int* qh, void* stream);
/* out (16 bytes, 8-byte aligned) = [loss_sum double = sum_{S_q > 0} L_q, live_groups int64 = #{q : S_q > 0}]; the
 * fp64 sum runs row by row in a fixed order (as rsx_binary_eval's loss_sum): the same bits every run. */
int rsx_query_softmax_eval(const float* F, const float* y, const int* row_group, const int* goff, int64_t R, int64_t G,
                           void* ws, int64_t ws_bytes, void* out, void* stream);
/* rsx_gbdt_tree with the gradient stage replaced by rsx_gbdt_grad_query_softmax (group_ws: its workspace): one
 * whole tree by one call, three kernels and one fill in place of rsx_gbdt_tree's one gradient kernel. */
int rsx_gbdt_tree_grouped(const uint8_t* bins, const float* y, const int* row_group, const int* goff, int64_t R,
                          int64_t G, int F, const uint8_t* is_cat, const int* n_bins, int depth, double lr, double l2,
                          float* Fx, int* qg, int* qh, uint8_t* leaf, int64_t* hist, void* ws, void* group_ws,
                          int64_t group_ws_bytes, int* splits, int64_t* leaf_sums, float* leaf_values, int* flag,
                          void* stream);
/* out [R] = (init ? init : f0) + the leaf values of the trees [tree_begin, tree_end) in order; splits int32
 * [T, 6, 2] (the first depth levels used) and leaf_values fp32 [T, 64]; out may be init. One row per lane. */
int rsx_gbdt_predict(const uint8_t* bins, int64_t R, int F, const int* splits, const float* leaf_values,
                     const uint8_t* is_cat, int depth, int tree_begin, int tree_end, const float* init, float f0,
                     float* out, void* stream);
/* The FeatureEngineer numeric columns (temp_model/ranker_skelet.py:29-68) of the candidates cand [Q, K]
 * (int64 item ids < N) with their retrieval scores score [Q, K]: U [Q, d] user vectors, V [N, d] item vectors,
 * item_price [N], user_avg_price [Q] -> feats fp32 [7, Q K] = two_tower_score; the mean, the maximum and the
 * population standard deviation of u * v; item_price; user_avg_price; price_diff_ratio = (price - avg) / avg
 * where avg > 0, else 0. ids int64 [Q K] = the candidates with an id outside [0, N) replaced by 0, which sets
 * flag bit 0. One wave per candidate. */
int rsx_rerank_tabular(const int64_t* cand, const float* score, const float* U, const float* V, const float* item_price,
                       const float* user_avg_price, int64_t Q, int64_t K, int64_t N, int64_t d, float* feats,
                       int64_t* ids, int* flag, void* stream);

/* ---- A18 ranker training rows: purchase logs -> rows -> columns, csrc/ranker_rows.hip -----------------
 * The reference builds the ranker's rows on the host: HMLogImporter (utils/monitor/log_importer.py:36-87)
 * emits, per purchase, the positive and negative_ratio items drawn uniformly among those the customer has
 * not bought (a rejection loop over Python's random), and FeatureEngineer.prepare_batch turns each row into
 * columns with numpy. Here both run on the device.
 *   sampling: the valid positives in order are pos_user, pos_item int32 [Pv] (user < C, item < N); customer
 *          c's distinct bought items are bought[bought_off[c] .. bought_off[c + 1]) = s_0 < s_1 < ... (int32,
 *          ascending and distinct; bought_off int64 [C + 1]), D_c of them, and M = N - D_c items are left.
 *          With K = negative_ratio >= 0 the rows are row_user, row_item int32 and y fp32 [Pv (K + 1)]: row
 *          p (K + 1) is positive p with y = 1 and rows p (K + 1) + 1 + k, k < K, its negatives with y = 0
 *          (the reference's order, :59-84). Negative (p, k): h = hash_u32(seed, p K + k) (csrc/rsx_common.h),
 *          r = ((uint64)h M) >> 32 in [0, M), item = r + #{j : s_j - j <= r}: the r-th item not in s, found
 *          by one binary search over the non-decreasing s_j - j. For a uniform h this is the reference's
 *          distribution (its rejection loop is uniform over the non-bought items too) up to the bias of the
 *          multiply-shift map: an item's probability differs from 1 / M by less than 2^-32, a relative
 *          bias of at most M / 2^32. The draw always terminates, is a function of (seed, p, k) alone and so
 *          does not depend on the launch shape; Python's random stream is not reproduced.
 *          flag (int32, OR-ed): bit 0 = a customer with M <= 0 (the reference would loop forever; the row's
 *          item is 0), bit 1 = a pos_user outside [0, C) or a pos_item outside [0, N) (0 is used), or a bought
 *          list that is not ascending and distinct within [0, N) (the item is clamped to N - 1). Offsets are
 *          clamped to [0, n_bought]: no access leaves its array. One thread per row; no thread walks a list.
 *   columns: rsx_pair_tabular gives the rows row_user, row_item int32 [R] the columns rsx_rerank_tabular
 *          gives candidates: U [C, d], V [N, d], item_price [N], user_avg_price [C] -> feats fp32 [7, R].
 *          Columns 1..6 come from the one device function both kernels call (csrc/rsx_pair_cols.h) and so
 *          have the same bits for the same pair. Column 0 is score[r], or with score NULL the fp32 dot
 *          product u . v of the same wave reduction (mean = dot / d). With y_out not NULL, y_out[r] = 1 where
 *          row_item[r] is among truth[truth_off[u] .. truth_off[u + 1]) (int32 ascending and distinct,
 *          truth_off int64 [C + 1], n_truth entries; a binary search), else 0. A user outside [0, C) or an
 *          item outside [0, N) is replaced by 0 and sets flag bit 0. One wave per row, 1 <= d <= 65536.
 * The only atomics are the integer ORs into flag: the same inputs give the same bits every run. Every loop
 * is bounded by its array length or by 32 halvings. */
int rsx_ranker_rows_sample(const int* pos_user, const int* pos_item, int64_t Pv, const int64_t* bought_off,
                           const int* bought, int64_t n_bought, int64_t C, int64_t N, int64_t K, uint64_t seed,
                           int* row_user, int* row_item, float* y, int* flag, void* stream);
int rsx_pair_tabular(const int* row_user, const int* row_item, const float* score, const float* U, const float* V,
                     const float* item_price, const float* user_avg_price, int64_t R, int64_t C, int64_t N, int64_t d,
                     const int64_t* truth_off, const int* truth, int64_t n_truth, float* feats, float* y_out, int* flag,
                     void* stream);

/* ---- A19 ordered target statistics: wide categorical columns of the oblivious-tree model, csrc/gbdt_ts.hip ----
 * The reference hands CatBoost six cat_features (temp_model/ranker_skelet.py:20-27, 106) and CatBoost encodes
 * them by ordered target statistics. Here a categorical column with more known values than one_hot_max_size
 * becomes one numeric column: one permutation, one prior; CatBoost's several permutations, feature combinations
 * and counter statistics are not reproduced. For TS column k (its index among the TS columns of the call) with
 * the codes c_i in [0, V_k] (0 = unknown / unseen, V_k <= GBDT_TS_MAX_CODES = 2^22), the labels y_i in {0, 1}
 * and R < 2^31 rows in the caller's row order, the prior (p, a), a > 0, and ap = a * p formed once on the host in
 * float64:
 *   order:  k_i = hash_u32(ts_seed + k, i) (csrc/rsx_common.h). Row j precedes row i iff (k_j, j) < (k_i, i): a
 *          total order, so nothing depends on a sort's tie-breaking.
 *   training value: n_i = #{j precedes i, c_j = c_i}, s_i = #{such j with y_j = 1},
 *          ts_i = (float)(((double)s_i + ap) / ((double)n_i + a)): two additions and one division in fp64,
 *          nothing to contract, then one rounding to fp32. A row that is first of its code gets the prior value
 *          (float)(ap / a), which is (float)p wherever a * p / a rounds back to p (the default (0.5, 1) does).
 *   table:  N_c, S_c = the totals over all training rows of code c; table[c] = (float)((S_c + ap) / (N_c + a)),
 *          the prior value for a code nobody had. Validation and serving rows read table[c]; a code outside
 *          [0, V_k] reads table[0].
 *   downstream: a TS column is a numeric column from there on: its borders are those of the ordered training
 *          values, its bins rsx_gbdt_bin's, its is_cat entry 0. The model's internal column order is numeric,
 *          then TS, then one-hot: that is the order in which ties between equally good splits are broken. At the
 *          end of the fit each TS column keeps the byte table bins(table) uint8 [V_k + 1]: serving it is a
 *          one-byte gather. Training rows see the ordered value and served rows the table's, so the prediction
 *          on the training rows no longer equals the training approximant of a model with TS columns.
 * rsx_gbdt_ts_keys writes keys int64 [Fts, R] = c_i << 32 | k_i; a stable ascending sort of each row of keys is
 * order int64 [Fts, R] (ties fall to the row index: the order above inside every code). rsx_gbdt_ordered_ts walks
 * that order on fixed 256-row tiles, one row per thread: a segmented exclusive scan of (1, y) over the runs of
 * equal code inside the tile, one scan over the tiles' aggregates per column, and a second tile pass that adds
 * the carry and scatters. No thread walks a run, no workgroup waits on another, every slot has one writer and all
 * sums are integers: the same bits every run. codes int32 [Fts, R], y fp32 [R], V int32 [Fts] (device), Vmax >=
 * every V_k the row stride - 1 of totals int32 [Fts, Vmax + 1, 2] = (N_c, S_c) and table fp32 [Fts, Vmax + 1]
 * (both written whole), ts fp32 [Fts, R] in the caller's row order, ws 16 Fts ceil(R / 256) bytes, 16-byte
 * aligned. flag (int32, OR-ed) bit 0: an order entry outside [0, R) (skipped) or a code outside [0, V_k] (its
 * row gets the prior value and counts nowhere); no access leaves its array. */
int rsx_gbdt_ts_keys(const int* codes, int64_t R, int Fts, uint64_t seed, int64_t* keys, void* stream);
int rsx_gbdt_ordered_ts(const int* codes, const int64_t* order, const float* y, const int* V, int64_t R, int Fts,
                        int64_t Vmax, double ap, double a, void* ws, int64_t ws_bytes, float* ts, int* totals,
                        float* table, int* flag, void* stream);

/* ---- A22 explaining the boosted ranker: leaf weights, SHAP values and importances, csrc/gbdt_explain.hip ----
 * CatBoost's get_feature_importance() on the oblivious-tree model of A17; restated in float64 numpy by
 * tests/gbdt_explain_ref.py. Everything below is fp64 but the weights, which are integers.
 *   row bits: for a tree with the levels d < depth and the splits (f_d, b_d), r_d = go right exactly as
 *          rsx_gbdt_predict decides it (a feature >= F reads as feature 0); leaf = sum_d r_d 2^(depth-1-d).
 *   leaf weights: w[t][l] = the number of rows of a data set that reach leaf l of tree t, int64 [T, 64], 0 at and
 *          beyond 2^depth. Integer sums: the same bits every run and in any row order.
 *   cover: the cover of node n of level d is the sum of w over the leaves below it.
 *   E(s), s in {0, 1, *}^depth: E(s) = ev(root, 0) with ev(n, depth) = value[n]; ev(n, d) = ev(2n + s_d, d + 1)
 *          where s_d is 0 or 1; else ev(n, d) = (c0 ev(2n, d+1) + c1 ev(2n+1, d+1)) / (c0 + c1) with c0, c1 the
 *          children's covers, and 1/2 ev(2n, d+1) + 1/2 ev(2n+1, d+1) where c0 + c1 = 0 (this model's own
 *          convention: Lundberg's path-dependent recursion divides 0 by 0 there). table[t][idx] = E(s) at idx =
 *          sum_d s_d 3^(depth-1-d) with * as digit 2, double [T, 729]; entries at and beyond 3^depth are unused.
 *   Shapley values of a tree: the players are its distinct split features, m <= depth of them; a feature that
 *          splits on several levels is one player and owns all of them. v(S) = table[idx] with s_d = r_d where
 *          f_d is in S and * elsewhere; phi_j = sum over S not holding j of |S|! (m - |S| - 1)! / m! (v(S + j) -
 *          v(S)). A feature not in the tree has phi_j = 0 exactly.
 *   Shapley values of a model: phi[j][r] = sum_t phi_j, j < F, and phi[F][r] = f0 + sum_t E(*, ..., *), the
 *          expected value (CatBoost's last column), each summed in tree order by one lane: the bits do not
 *          depend on R, the grid or the chunking. A row's F + 1 entries sum to its raw score.
 *   PredictionValuesChange: pvc[t][d] = the sum over the pairs of leaves (l1, l2) that differ only in the bit of
 *          level d, in ascending order, of c1 c2 / (c1 + c2) (v1 - v2)^2 (0 where c1 + c2 = 0), double [T, 6], 0
 *          at and beyond depth. A feature's importance is the sum of its levels over the trees in tree order,
 *          the vector scaled to sum 100 (all zeros stay zeros).
 *   LossFunctionChange of feature j: metric(F - phi_j) - metric(F) on labelled rows, the metric the model's own
 *          loss (CatBoost's SHAP-based approximation; positive = the feature helps). Composed in Python from
 *          rsx_gbdt_shap and the evaluation entries.
 * Every access stays in its array whatever the splits and bins hold. */
/* trees rsx_gbdt_shap stages in LDS at a time */
int64_t rsx_gbdt_shap_tree_chunk(void);
/* weights int64 [T, 64]: the rows [tree_begin, tree_end) are zeroed here, then counted (LDS and 64-bit global integer
 * atomics); splits int32 [T, 6, 2]. */
int rsx_gbdt_leaf_weights(const uint8_t* bins, int64_t R, int F, const int* splits, const uint8_t* is_cat, int depth,
                          int tree_begin, int tree_end, int64_t* weights, void* stream);
/* leaf_values fp32 [T, 64], weights int64 [T, 64] -> table double [T, 729], pvc double [T, 6], the rows [tree_begin,
 * tree_end). One workgroup per tree. splits is not read: both depend on the leaves and the weights alone. */
int rsx_gbdt_explain_plan(const int* splits, const float* leaf_values, const int64_t* weights, int depth, int tree_begin,
                          int tree_end, double* table, double* pvc, void* stream);
/* phi double [F + 1, R] of the trees [tree_begin, tree_end). One row per lane, the trees staged through LDS. */
int rsx_gbdt_shap(const uint8_t* bins, int64_t R, int F, const int* splits, const uint8_t* is_cat, int depth,
                  int tree_begin, int tree_end, const double* table, double f0, double* phi, void* stream);

/* ---- A20 transaction features: the towers' frames from the purchase log, csrc/tx_features.hip --------------
 * The reference builds features_user_w_meta, features_item and features_sequence with pandas groupbys and a
 * pandarallel apply per customer (staticstics/preprosess_agg_parallel.py). Here the log is a table sorted by
 * (customer, day), same-day ties in file order (the reference's sort_values leaves them open; file order is this
 * project's definition and decides last_price and the order of same-day sequence entries): item, day int32 [T],
 * price fp32 [T], channel uint8 [T], T < 2^31 rows, and cust_off int64 [C + 1]. Every per-segment quantity is a
 * segmented scan on fixed 256-row tiles: a tile pass, one scan over the tiles' aggregates, a second tile pass.
 * No thread walks a segment, no workgroup waits on another, every slot has one writer and the order in which
 * floating-point values combine is fixed: the same bits every run. Integer results are exact. ws is
 * rsx_tx_workspace_bytes(T) bytes, 16-byte aligned; flag is int32, OR-ed, and no access leaves its array
 * whatever the inputs hold.
 *   calendar: day = days since 1970-01-01 in [0, 2^31): weekend = ((day + 3) mod 7 >= 5) (Monday = 0), month =
 *          12 year + month - 1 by the civil-from-days integer algorithm, week = floor((day + 3) / 7) (weeks start
 *          on Monday). A negative day is taken as 0 and sets flag bit 0.
 *   segment rows: row_seg[t] = the s with seg_off[s] <= t < seg_off[s + 1], -1 for a row in no segment.
 *          Offsets are clamped to [0, T]; an offset outside it, a decreasing pair, seg_off[0] != 0 or
 *          seg_off[S] != T set flag bit 0. The entries below take row_seg: non-decreasing over the rows (this
 *          entry's output, or a sorted column such as the item of a by-item order); a value outside [0, S) is a
 *          row of no segment; a value >= S or a value below its predecessor's sets flag bit 0 (equal values
 *          must be contiguous: each run would write the slot again).
 *   segment stats: with perm NULL the rows are the table's, else sorted position t is table row perm[t] (an
 *          entry outside [0, T) is skipped, flag bit 0). Per segment: count, sum = the fp64 sum of the fp32
 *          prices, m2 = sum (price - mean)^2 in fp64 with mean = sum / count (a second pass), last = the last
 *          row's price, dmin / dmax = the smallest / largest day, chan = the sum of channel, wkend = the
 *          number of rows with weekend != 0. A segment without rows has zeros everywhere.
 *   segment distinct: val int32 [T] non-decreasing inside every segment -> the number of distinct values per
 *          segment (the rows whose value differs from their predecessor's, and the first). A decreasing pair
 *          inside a segment sets flag bit 1.
 *   weekly sales: weeks int32 [W] ascending and distinct, the weeks with at least one row -> weekly int32 [N, W],
 *          weekly[i, j] = #{t : item[t] = i, week[t] = weeks[j]}: the reference's groupby([article_id,
 *          week_start]).size().unstack(fill_value=0).sort_index(axis=1); a week nobody bought in has no column.
 *          Integer atomics. An item outside [0, N) or a week not in weeks is skipped and sets flag bit 0.
 *   item features (:171-237): out fp32 [8, N] = raw_probability = n / T; pop_1w_log = log1p(last column);
 *          pop_1m_log = log1p(sum of the last four columns that exist); velocity_1w = clip((cur - prev) / (prev +
 *          1), -1, 5) over the last two columns, velocity_1m the same over the last four and the columns [-8:-4]
 *          that exist (prev = 0 where none does); steady_score_log = log1p(mean / (std + 1e-9)) over the last
 *          min(12, W) columns, std with ddof = 1 from the two-pass sum of squares, 0 when W = 1 (the NaN the
 *          frame's fillna(0) removes); avg_item_price_log = log1p(sum / n); days_since_release_log = log1p(max_day
 *          - dmin). Then for an item with max_day - dmin < cold_days (14) rows 1..4 are replaced by the row's
 *          mean over all items taken before any replacement: the fixed-order fp64 sum of the fp32 values, / N. The
 *          sum has two levels: per chunk of 4096 values thread j of 256 adds the elements j, j + 256, ... in order
 *          and the 256 partial sums meet in a fixed tree; the chunk sums are summed the same way. col_sum:
 *          col_sum_doubles >= 4 + 4 ceil(N / 4096) doubles, the four sums first.
 *          Every value is evaluated in fp64 and rounded once.
 *   user features (:329-351, :549-570): from the per-customer stats, uniq (distinct items) and months (distinct
 *          months): f64 double [3, C] = user_avg_price = sum / n, total_cnt, recency_days = max_day - dmax (what
 *          the buckets are cut from); cols fp32 [11, C] = price_std = sqrt(m2 / (n - 1)) (0 for n = 1),
 *          last_price_diff = last - mean, repurchase_ratio = 1 - uniq / n, weekend_ratio = wkend / n, then
 *          their four standardised forms (x - mean) / (std + 1e-9), then the reranker frame's user_avg_price_log
 *          = log1p(mean), total_cnt_log = log1p(n), recency_log = log1p(recency_days). x is the fp32 column as
 *          stored for the first three and the fp64 ratio for weekend_ratio (the reference's dtypes); mean and std
 *          (ddof = 1) come from the two-pass fixed-order fp64 sums above over all C customers; C = 1 gives 0.
 *          channel int8 = 2 where chan / n > 1.5, else 1; active_months int16 = months. ws: (4 C + 8 + 4 ceil(C /
 *          4096)) * 8 bytes.
 *   quantile buckets: pd.qcut(x, q, labels=False, duplicates='drop') + 1 for x double [n] with its ascending
 *          copy s. Edge k = 0..q interpolates s at h = (n - 1) k / q, formed in float64 in the steps pandas'
 *          quantile takes (numpy.percentile of linspace(0, 1, q + 1), method 'linear'): p = k * (1 / q), 1 for k =
 *          q; p = (p * 100) / 100; h = (n - 1) * p; lo = floor(h), t = h - lo; e_k = s[lo] + (s[lo + 1] - s[lo]) t,
 *          or s[lo + 1] - (s[lo + 1] - s[lo]) (1 - t) where t >= 0.5 (numpy's _lerp; a product and a sum, not
 *          contracted), s[n - 1] where lo >= n - 1. These are the bits pandas 2 / numpy 2 give: h is not the
 *          exact fraction (at n = 701, q = 10, k = 7 it is 489.99999999999994 and the edge lies just below
 *          s[490]). Equal edges are dropped: edges double [q + 1] holds the n_edges (int32) that remain. bucket
 *          int8 = #{edges < x}, at least 1: the lowest edge is in bucket 1 and a constant column is 1 everywhere
 *          (the reference raises there on its int8 cast of NaN). q <= 126.
 *   sequences: valid uint8 [N] marks the items kept. rsx_tx_sequence_ranks: rank[t] = the number of valid rows
 *          behind row t in its customer (a reversed segmented scan), -1 for a row whose item is not valid (an item
 *          outside [0, N): flag bit 0); n_valid [C] = the customer's valid rows, last_day [C] = the day of the last
 *          one. The caller forms seq_off int64 [C + 1] = the running sum of min(n_valid, max_len), n_out its last
 *          entry. rsx_tx_sequences: a row with 0 <= rank < max_len goes to slot seq_off[c + 1] - 1 - rank:
 *          seq_item = its item, seq_delta = last_day[c] - day. One writer per slot; a slot outside its
 *          customer's range (offsets that are not those of n_valid) is skipped and sets flag bit 0. */
int64_t rsx_tx_workspace_bytes(int64_t T);
int rsx_tx_calendar(const int* day, int64_t T, uint8_t* weekend, int* month, int* week, int* flag, void* stream);
int rsx_tx_segment_rows(const int64_t* seg_off, int64_t S, int64_t T, void* ws, int64_t ws_bytes, int* row_seg,
                        int* flag, void* stream);
int rsx_tx_segment_stats(const int* row_seg, int64_t S, int64_t T, const int64_t* perm, const float* price,
                         const int* day, const uint8_t* channel, const uint8_t* weekend, void* ws, int64_t ws_bytes,
                         int* count, double* sum, double* m2, float* last, int* dmin, int* dmax, int64_t* chan,
                         int* wkend, int* flag, void* stream);
int rsx_tx_segment_distinct(const int* row_seg, int64_t S, int64_t T, const int* val, void* ws, int64_t ws_bytes,
                            int* distinct, int* flag, void* stream);
int rsx_tx_weekly_sales(const int* item, const int* week, int64_t T, const int* weeks, int64_t W, int64_t N,
                        int* weekly, int* flag, void* stream);
int rsx_tx_item_features(const int* weekly, int64_t N, int64_t W, const int* count, const double* sum,
                         const int* dmin, int64_t T, int max_day, int cold_days, double* col_sum, int64_t col_sum_doubles,
                         float* out, void* stream);
int rsx_tx_user_features(const int* count, const double* sum, const double* m2, const float* last, const int* dmax,
                         const int64_t* chan, const int* wkend, const int* uniq, const int* months, int64_t C,
                         int max_day, void* ws, int64_t ws_bytes, double* f64, float* cols, int8_t* channel,
                         int16_t* active_months, void* stream);
int rsx_quantile_bucket(const double* x, const double* sorted, int64_t n, int q, double* edges, int* n_edges,
                        int8_t* bucket, void* stream);
int rsx_tx_sequence_ranks(const int* row_seg, int64_t C, int64_t T, const int* item, const int* day,
                          const uint8_t* valid, int64_t N, void* ws, int64_t ws_bytes, int* rank, int* n_valid,
                          int* last_day, int* flag, void* stream);
int rsx_tx_sequences(const int* row_seg, int64_t C, int64_t T, const int* item, const int* day, const int* rank,
                     const int* last_day, const int64_t* seq_off, int max_len, int64_t n_out, int* seq_item,
                     int* seq_delta, int* flag, void* stream);
/* The persona columns (reference staticstics/preprocess_clustering.py) add three passes in the same shape:
 *   segment runs: val int32 [T] non-decreasing inside every segment (flag bit 1 on a decreasing pair, as segment
 *          distinct). A run is a maximal stretch of equal val inside one segment, of length n. Per segment: runs
 *          int32 = the number of runs (= segment distinct), repeated int32 = the sum of n over the runs with n > 1,
 *          nlogn double = the sum of n ln n over the runs, in fp64, the runs in their order through the fixed
 *          scan. Two passes: the inclusive maximum of "t + 1 where a run starts" gives every run's last row its
 *          length; the lengths' contributions are summed per segment. With n = count: ln n - nlogn / n is the
 *          entropy of the value counts (natural log), repeated / n the share of rows whose value occurs more than
 *          once. ws: rsx_tx_workspace_bytes(T) + 4 T bytes (the tiles' slots, then one int32 per row).
 *   segment sum f64: x double [T] (read through perm as segment stats does): count int32, sum double = the fp64
 *          sum, m2 double = sum (x - sum / count)^2 (a second pass; NULL: not computed). A flag column is summed
 *          as 0.0 / 1.0, exactly. A segment without rows has zeros.
 *   price ratio: ratio[t] = (double)price[t] / cat_mean[item_cat[item[t]]] in fp64, item_cat int32 [N], cat_mean
 *          double [n_cat]. An item outside [0, N) or a category outside [0, n_cat) gives 0 and sets flag bit 0. */
int rsx_tx_segment_runs(const int* row_seg, int64_t S, int64_t T, const int* val, void* ws, int64_t ws_bytes,
                        int* runs, int* repeated, double* nlogn, int* flag, void* stream);
int rsx_tx_segment_sum_f64(const int* row_seg, int64_t S, int64_t T, const int64_t* perm, const double* x, void* ws,
                           int64_t ws_bytes, int* count, double* sum, double* m2, int* flag, void* stream);
int rsx_tx_price_ratio(const int* item, const float* price, int64_t T, const int* item_cat, const double* cat_mean,
                       int64_t N, int64_t n_cat, double* ratio, int* flag, void* stream);

/* ---- A21 k-means on a fixed-point grid: the customer personas, csrc/kmeans.hip ---------------------------------
 * The reference standardises seven per-customer columns and runs scikit-learn's KMeans on the host
 * (staticstics/preprocess_clustering.py). Here the clustering runs on q int32 [d, C], feature-major, standing for
 * the values q 2^-frac_bits exactly. A cluster's sum is then an integer, so the centres, and with them the whole
 * trajectory, are the same bits every run and in any row order. Limits: d <= 32, K <= 256, K d <= 4096, C < 2^31;
 * anything else is an error. max_workgroups caps every row kernel's grid (min(ceil(C / 256), max_workgroups)
 * workgroups stride over the 256-row tiles); it changes no result. flag is int32, OR-ed; no access leaves its
 * array whatever the inputs hold (a label is written, never used as an index unchecked).
 *   standardize columns: x double [d, C]: mean = sum / C and var = sum (x - mean)^2 / C (ddof = 0) from the
 *          two-pass fixed-order two-level sums of "item features" above; scale = sqrt(var), or 1 for a constant
 *          column: var <= C eps var + (C mean eps)^2 with eps = 2^-52, scikit-learn's rule, which holds var = 0.
 *          out = (x - mean) / scale (NULL: the moments only). ws: (2 + ceil(C / 4096)) d doubles.
 *   quantize: q = rint(x 2^frac_bits) (ties to even), 0 <= frac_bits <= 30. A value outside +-(2^31 - 1) is
 *          clamped there, a NaN becomes 0; both set flag bit 0.
 *   distance: D(i, k) = sum_j (x_ij - c_kj)^2 with x_ij = (double)q 2^-frac_bits, in fp64, j ascending from an
 *          accumulator of 0, the subtraction first, product and sum not contracted. The label of a row is the
 *          smallest k among the minima.
 *   seed (k-means++ as an exponential race): seeds[0] = hash_u32(seed, 0) mod C. Round r = 1 .. K - 1: dmin_i =
 *          min(dmin_i, D(i, row seeds[r - 1])); u_i = (hash_u32(seed + r, i) + 0.5) 2^-32 (csrc/rsx_common.h);
 *          key_i = dmin_i / -ln u_i; seeds[r] = the row with the largest key, the lowest row on ties. Row i wins
 *          with probability dmin_i / sum dmin, and a row with dmin = 0 only when every row has. One launch per
 *          round leaves a candidate per workgroup, a one-workgroup launch picks among them; no host read.
 *          centres double [K, d] = the seed rows. ws: rsx_kmeans_seed_workspace_bytes(C, max_workgroups) = 8 C +
 *          16 min(ceil(C / 256), max_workgroups) bytes, 16-byte aligned.
 *   iterate (Lloyd): n_iter iterations numbered from first_iteration >= 1, all enqueued. An iteration assigns
 *          every row (the centres in LDS, one row per thread), each workgroup adds int64 sum_q [K, d], int32 count
 *          [K] and the number of rows whose label changed in LDS over its tiles and flushes the non-zero slots
 *          with integer atomic adds; then one workgroup sets c_kj = (double)sum_q / ((double)count 2^frac_bits) (a
 *          cluster without rows keeps its centre), shift = sum_k sum_j (c_new - c_old)^2 sequentially, k outer, j
 *          inner, ctl[1] (done) = the iteration's number the first time changed == 0 or shift <= tol_abs, and
 *          clears the accumulators. Once done is set the later kernels return at once, so the result does not
 *          depend on n_iter. The caller zeroes sum_q, count and ctl int32 [4] = {changed, done, iterations run, 0}
 *          and fills labels with -1 before the first call; shift double [1] holds the last shift.
 *   assign: labels int32 [C] and, when given, dmin double [C] = D(i, label) and inertia double [1] = the fixed-order
 *          two-level sum of dmin (ws: ceil(C / 4096) doubles). */
int rsx_standardize_columns(const double* x, int64_t d, int64_t C, double* ws, int64_t ws_doubles, double* out,
                            double* mean, double* var, double* scale, void* stream);
int rsx_kmeans_quantize(const double* x, int64_t d, int64_t C, int frac_bits, int* q, int* flag, void* stream);
int64_t rsx_kmeans_seed_workspace_bytes(int64_t C, int64_t max_workgroups);
int rsx_kmeans_seed(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, uint64_t seed, int64_t max_workgroups,
                    void* ws, int64_t ws_bytes, int* seeds, double* centres, int* flag, void* stream);
int rsx_kmeans_iterate(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, double* centres, int* labels,
                       int64_t* sum_q, int* count, int* ctl, double* shift, double tol_abs, int first_iteration,
                       int n_iter, int64_t max_workgroups, void* stream);
int rsx_kmeans_assign(const int* q, int64_t d, int64_t C, int frac_bits, int64_t K, const double* centres,
                      int64_t max_workgroups, double* ws, int64_t ws_doubles, int* labels, double* dmin,
                      double* inertia, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RECSYS_AMD_H */
