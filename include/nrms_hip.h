/*
 * nrms_hip.h — C ABI of the MI355X (gfx950) NRMS scoring library
 * (libnrms_hip.so, built from newsrecommendationsystem_amd/csrc/).
 *
 * Drop-in boundary for the NRMS scoring path of Maguire1999/
 * NewsRecommendationSystem (paths below are relative to that repo). The
 * reference is PyTorch only and has no FFI of its own; each entry point here
 * replaces the ATen op sequence of one reference method, cited per function.
 * The Python host mirror (newsrecommendationsystem_amd/nrms.py) binds these
 * through ctypes behind the reference's own NRMS module interface.
 *
 * Conventions
 *   - All tensor arguments are caller-allocated DEVICE pointers, borrowed for
 *     the call (except the descriptor arrays of nrms_adam_step_multi,
 *     nrms_params_pack and nrms_params_unpack_div: HOST arrays read during
 *     the call). The library never allocates or frees device
 *     memory and never synchronises the stream; any host thread may call it
 *     on any stream, and every call is capturable into a hipGraph. It keeps
 *     no per-call state. Process-wide state is limited to: the GEMM
 *     arithmetic, title-dedupe and token-compaction switches (atomics read at
 *     enqueue time; each can be overridden per host thread), the last HIP
 *     error (thread-local), and a mutex-guarded record of which (device,
 *     kernel) pairs have had their dynamic-LDS limit raised.
 *   - fp32 row-major everywhere; ids are int64 (the reference's LongTensor).
 *   - Every function returns NRMS_OK (0) or an nrms_status_t error code; a
 *     launch failure returns NRMS_ERR_HIP and the HIP error is kept for
 *     nrms_last_hip_error().
 *   - Kernels assume ids are in [0, V); callers validate (the Python glue does,
 *     mirroring nn.Embedding's IndexError). An out-of-range id never reads out
 *     of bounds: its row is produced as NaN.
 *   - Eval-mode semantics (dropout = identity, src/model/NRMS/news_encoder.py:
 *     38-40,43-45) for the scoring path; the training kernels at the end of
 *     this header provide the train-mode forward pieces and the backward.
 */
#ifndef NRMS_HIP_H
#define NRMS_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: nrms_user_encode takes batch / row strides; nrms_adam_step_multi takes a
 *    host descriptor array (no device table, no total_blocks); q|k|v buffers
 *    carry a row stride (nrms_qkv_row_stride). */
/* 3: nrms_forward_timed / nrms_forward_stage_name; nrms_forward's workspace
 *    holds the UserEncoder row list (nrms_forward_workspace_size grew). */
/* 4: nrms_qkv_project_ws; the encode / forward workspaces hold the split
 *    Q|K|V weight (their *_workspace_size functions grew). */
/* 5: nrms_set_token_compaction; title-level padding dedupe; the encode /
 *    forward workspaces hold the title buckets (*_workspace_size grew). */
/* 6: nrms_set_thread_gemm_arith / _title_dedupe / _token_compaction
 *    (per-thread overrides of the process-wide switches). */
/* 7: host-side readers of the eval split files (nrms_behaviors_scan /
 *    nrms_behaviors_parse / nrms_news_parse); nrms_forward's workspace holds
 *    the UserEncoder dispatch order (nrms_forward_workspace_size grew). */
/* 8: deterministic training backward (workspaces of nrms_additive_backward /
 *    nrms_qkv_project_backward; nrms_embedding_backward_ws). */
/* 9: nrms_recommend_topk / nrms_recommend_topk_workspace_size. Recorded here
 *    as well, since it went in under 8 without a bump: nrms_embedding_backward_ws
 *    sums an id with more than 256 tokens in 64-token segments added in
 *    segment order (round 6), no longer in one token-order chain; ids with
 *    <= 256 tokens are unchanged.
 *    ABI 9, added later (additive, no bump): nrms_forward_state_t,
 *    nrms_forward_state_size, nrms_forward_prepare,
 *    nrms_forward_prepared_workspace_size (and _folded_), nrms_forward_prepared
 *    and nrms_forward_prepared_timed.
 *    ABI 9, added later (additive, no bump): nrms_rank_impressions, and the
 *    host readers nrms_behaviors_scan_any / nrms_behaviors_parse_any.
 *    ABI 9, added later (additive, no bump): nrms_train_batch_gather and
 *    nrms_xent_class0 (the fit loop's batch assembly and fused loss).
 *    ABI 9, added later (additive, no bump): nrms_train_batch_sample_gather
 *    (batch assembly from raw impressions, negatives drawn in the launch).
 *    ABI 9, added later (additive, no bump): nrms_views_weights_t,
 *    nrms_views_state_size, nrms_views_prepare,
 *    nrms_news_views_fuse_workspace_size, nrms_news_views_fuse and
 *    nrms_rows_add_position (the Exp1 model's category views and position
 *    embedding, csrc/views.hip). */
#define NRMS_ABI_VERSION 9

typedef enum {
  NRMS_OK = 0,
  NRMS_ERR_INVALID_ARG = 1,   /* null pointer, negative size, misalignment   */
  NRMS_ERR_UNSUPPORTED = 2,   /* shape outside the compiled kernel set       */
  NRMS_ERR_WORKSPACE = 3,     /* workspace missing or too small              */
  NRMS_ERR_HIP = 4            /* a HIP launch/API call failed                */
} nrms_status_t;

/* One encoder's parameters (device pointers), nn.Linear layout [out, in].
 * Mirrors MultiHeadSelfAttention (src/model/general/attention/
 * multihead_self.py:27-44) + AdditiveAttention (src/model/general/attention/
 * additive.py:13-20). */
typedef struct {
  const float* w_q; const float* b_q;   /* [D, D], [D] */
  const float* w_k; const float* b_k;   /* [D, D], [D] */
  const float* w_v; const float* b_v;   /* [D, D], [D] */
  const float* w_add; const float* b_add; /* additive linear [Q, D], [Q] */
  const float* q_add;                   /* attention_query_vector [Q]  */
  int32_t d_model;                      /* D  (300)                    */
  int32_t n_heads;                      /* H  (15); D / H must be 20   */
  int32_t query_dim;                    /* Q  (200); must be <= 208    */
} nrms_encoder_weights_t;

/* News-encoder projection strategy. FOLDED projects the whole vocabulary once
 * (qkv_table[V, 3D] = E W^T + b) and gathers projected rows per token; DIRECT
 * gathers embedding rows and projects every token. Both give the same result
 * (each projected row depends only on its token id); AUTO picks FOLDED when
 * the batch has more tokens than the vocabulary. */
typedef enum { NRMS_PROJ_AUTO = 0, NRMS_PROJ_DIRECT = 1, NRMS_PROJ_FOLDED = 2 } nrms_proj_mode_t;

/* Arithmetic of the matrix-core GEMMs (Q|K|V projections and the news
 * encoder's additive projection; attention contractions are always f32 MFMA).
 * SPLIT_BF16X6: each fp32 operand is split exactly into three bf16 planes
 * (hi + mid + lo, 8 significand bits each) and the six plane products with
 * i + j <= 2 are accumulated in fp32 on v_mfma_f32_16x16x32_bf16; every bf16
 * product is exact and the dropped terms are below 2^-25 |a||b|, so the result
 * has fp32-GEMM accuracy (measured: normwise error vs fp64 at or below the F32
 * mode's) at 6/16 of the f32-MFMA cycles.
 * SPLIT_F16X3 (default): the news encoder's additive projection splits each
 * operand into two fp16 planes, a = hi + 2^-11 lo (22 significand bits), and
 * accumulates lo·hi + hi·lo + hi·(2^11 hi) in one fp32 accumulator on
 * v_mfma_f32_16x16x32_f16 (3 products instead of 6); the dropped terms are
 * ~2^-22 |a||b|, normwise error vs fp64 still below a plain fp32 GEMM's. An
 * operand outside fp16's range (|a| >= 65,520) turns its outputs into NaN,
 * and those title groups are recomputed by the SPLIT_BF16X6 / reference-exp
 * recheck pass, so results never depend on the range. The encoders' Q|K|V
 * projections (nrms_qkv_project_ws, nrms_forward, the encode entry points)
 * scale every input row and every weight row by a power of two into fp16's
 * range (exact, any magnitude), split the input exactly into three fp16
 * pieces and the weights into two (22 bits), and accumulate three products
 * (four when some weight column fits in 11 bits; NRMS_PROJ_PRODUCTS=4 forces
 * four): fp32-GEMM accuracy, and products as exact as fp32's for weights
 * that fit in 11 bits. The fused UserEncoder's additive GEMM scales each context row
 * the same way and accumulates three fp16 products (22-bit operands). The
 * staged nrms_qkv_project and the stage kernels run SPLIT_BF16X6 in this mode.
 * F32: v_mfma_f32_16x16x4_f32, each product an exact fp32 FMA.
 * Process-wide; the initial value comes from the environment (NRMS_GEMM=f32
 * selects F32, NRMS_GEMM=x6 SPLIT_BF16X6). Returns the previous mode, or
 * -NRMS_ERR_INVALID_ARG for an unknown mode. Not synchronised with launches
 * in flight: set it before enqueuing work. */
typedef enum {
  NRMS_GEMM_SPLIT_BF16X6 = 0,
  NRMS_GEMM_F32 = 1,
  NRMS_GEMM_SPLIT_F16X3 = 2
} nrms_gemm_arith_t;
int32_t nrms_set_gemm_arith(int32_t mode);
int32_t nrms_get_gemm_arith(void);

/* All-padding titles (20 zero ids: the left-padding of short histories,
 * src/dataset.py:79-83, ~45 % of the clicked slots at BASELINE config 3) all
 * have the same news vector. With dedupe on (default), the fused news tail
 * encodes one of them per call and copies its vector to the others; every
 * output is bitwise the same as encoding each title (a title's vector depends
 * on its own ids only, never on where in the launch it is encoded). Applies
 * where ids are passed (16-B aligned id rows). Process-wide, read at enqueue
 * time; returns the previous setting. NRMS_DEDUPE=0 in the environment starts
 * with it off. */
int32_t nrms_set_title_dedupe(int32_t on);

/* Token compaction in the fused news tail (default on): the id-0 tokens of a
 * title (its right-padding, src/data_preprocess.py:115,132-139) share one
 * q|k|v row, so a title with c real tokens is encoded on c + 1 distinct rows,
 * the padding row carrying its multiplicity 20 - c in the raw-exp sums, the
 * attention context and the additive softmax / pooling (news_fused.hip). For
 * right-padded titles (all id-0 tokens after the real ones) the raw-exp row
 * sums are bitwise the uncompacted ones (the padding row's exp is added
 * 20 - c times, in the reference's key order). An id-0 token in the middle
 * of a title (an out-of-vocabulary word, src/data_preprocess.py:134-135) is
 * summed after the real keys instead, so its row sums agree only to fp32
 * rounding. The context and pooling replace 20 - c equal additions by one
 * product: results agree with the uncompacted computation to fp32 rounding. Process-wide, read at enqueue
 * time; returns the previous setting. NRMS_COMPACT=0 in the environment
 * starts with it off. */
int32_t nrms_set_token_compaction(int32_t on);

/* Per-thread overrides of the three process-wide switches above (ABI 6): a
 * value >= 0 applies to the work the CALLING host thread enqueues, in place
 * of the process-wide setting, so host threads driving different arithmetics
 * (or dedupe / compaction settings) on different streams do not race; -1
 * clears the thread's override. Each returns the thread's previous override
 * (-1: none), or -NRMS_ERR_INVALID_ARG. nrms_get_gemm_arith reports the
 * calling thread's effective mode. */
int32_t nrms_set_thread_gemm_arith(int32_t mode);
int32_t nrms_set_thread_title_dedupe(int32_t on);
int32_t nrms_set_thread_token_compaction(int32_t on);

int32_t nrms_abi_version(void);
const char* nrms_status_string(int32_t status);
int32_t nrms_last_hip_error(void);

/* nn.Embedding forward (src/model/NRMS/news_encoder.py:38): out[t,:] =
 * table[ids[t],:] for t < n_tok, bit-exact copy; id 0 is gathered like any id. */
int32_t nrms_embedding_gather(const int64_t* ids, int64_t n_tok, const float* table,
                              int64_t V, int32_t D, float* out, hipStream_t stream);

/* Row stride (floats) of the q|k|v rows the fused kernels prefer: 3D (900 for
 * D = 300; rows padded to whole 128-B lines, 928, measured 5 % slower per
 * step: DESIGN.md). Any stride >= 3D that is a multiple of 4 is accepted. */
int32_t nrms_qkv_row_stride(int32_t D);

/* Q|K|V projection (multihead_self.py:53-58): qkv[m * ld_qkv + 0:3D] =
 * x[row(m)] [W_Q;W_K;W_V]^T + [b_Q;b_K;b_V], row(m) = row_ids ? row_ids[m] : m
 * (row_ids index x's rows, n_rows_x bounds them); ld_qkv = 0 means 3D.
 * MFMA GEMM (arithmetic: nrms_set_gemm_arith). */
int32_t nrms_qkv_project(const float* x, int64_t n_rows_x, const int64_t* row_ids, int64_t M,
                         const nrms_encoder_weights_t* w, float* qkv, int64_t ld_qkv,
                         hipStream_t stream);

/* The same projection through the workspace — the one the encode / forward
 * entry points use. For the NRMS shape (D = 300, split arithmetic) the weight
 * is split once per call into MFMA fragments (workspace) and one persistent
 * workgroup per CU keeps a 64-row tile of x resident in LDS while it streams
 * the fragments from L2. Bitwise equal to nrms_qkv_project under
 * NRMS_GEMM_SPLIT_BF16X6 (same x6 products in the same order) and under
 * NRMS_GEMM_F32 (both run the f32 GEMM). Under NRMS_GEMM_SPLIT_F16X3 (the
 * default) it runs the scaled split-f16 arithmetic instead — each x row and
 * each weight row scaled by a power of two into fp16's range, x split exactly
 * into three fp16 pieces, the weight into two (22 bits), three products
 * summed in fp32 (four when some weight column fits in 11 bits): within
 * ~2^-22 |x||w| per product of the exact result (fp32-GEMM accuracy; exact
 * products for weights that fit in 11 bits) — so only within
 * rounding of nrms_qkv_project's x6 rows, not bitwise. Other shapes: as
 * nrms_qkv_project. */
size_t nrms_qkv_project_workspace_size(int32_t D);
int32_t nrms_qkv_project_ws(const float* x, int64_t n_rows_x, const int64_t* row_ids, int64_t M,
                            const nrms_encoder_weights_t* w, float* qkv, int64_t ld_qkv,
                            void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Multi-head raw-exp self-attention over sequences of length L
 * (ScaledDotProductAttention, multihead_self.py:15-23, heads concatenated
 * :74-75) over packed q|k|v rows (stride 3D): for sequence s, token i reads qkv row r(s,i) = tok_ids ?
 * tok_ids[s*L+i] : s*L+i (tok_ids index qkv's n_rows_qkv rows). Sequences
 * s >= n_seq_a take their ids from tok_ids_b + (s-n_seq_a)*L (NULL: same
 * array). ctx[s*L+i, :] is the [D] context row. L <= 4096 (beyond 64 the
 * K|V rows are read through L2 instead of LDS). */
int32_t nrms_self_attention(const float* qkv, int64_t n_rows_qkv, const int64_t* tok_ids,
                            int64_t n_seq_a, const int64_t* tok_ids_b, int64_t n_seq,
                            int32_t L, const nrms_encoder_weights_t* w, float* ctx,
                            hipStream_t stream);

/* AdditiveAttention (additive.py:27-53) over x[n_seq, L, D]:
 * out[s] = sum_l softmax_l(tanh(x W^T + b) . q) x[s,l]. scores_ws: device
 * scratch of n_seq*L floats. */
int32_t nrms_additive_attention(const float* x, int64_t n_seq, int32_t L,
                                const nrms_encoder_weights_t* w, float* scores_ws,
                                float* out, hipStream_t stream);

/* The two halves of nrms_additive_attention, for callers that time or fuse
 * them separately: per-token scores[m] = tanh(x[m] W^T + b) . q for m <
 * n_rows (additive.py:35-38; the [n_rows, Q] tile stays in registers), and
 * the pooling out[s] = sum_l softmax_l(scores[s, :]) x[s, l] (:39,51-52). */
int32_t nrms_additive_scores(const float* x, int64_t n_rows, const nrms_encoder_weights_t* w,
                             float* scores, hipStream_t stream);
int32_t nrms_additive_pool(const float* x, const float* scores, int64_t n_seq, int32_t L,
                           int32_t D, float* out, hipStream_t stream);

/* Fused NewsEncoder tail (news_encoder.py:42-47): raw-exp MHSA over projected
 * rows + additive attention + pooling, 4 titles per workgroup per step, all
 * contractions on the matrix cores, the context kept in LDS for the additive
 * GEMM and the pooling (workspace: only a packed copy of W_add). Row
 * addressing as
 * nrms_self_attention. Compiled for the reference geometry (L = 20, D = 300,
 * H = 15, Q = 200); other shapes return NRMS_ERR_UNSUPPORTED (use the stage
 * entry points). Used by nrms_news_encode* and nrms_forward when it applies. */
size_t nrms_news_attention_pool_workspace_size(int64_t n_titles, int32_t L, int32_t D);
int32_t nrms_news_attention_pool(const float* qkv, int64_t ld_qkv, int64_t n_rows_qkv,
                                 const int64_t* tok_ids, int64_t n_seq_a, const int64_t* tok_ids_b,
                                 int64_t n_titles, int32_t L, const nrms_encoder_weights_t* w,
                                 float* out, void* workspace, size_t workspace_bytes,
                                 hipStream_t stream);

/* NewsEncoder.forward (src/model/NRMS/news_encoder.py:27-48), eval mode:
 * ids[n_titles, L] -> out[n_titles, D]. */
size_t nrms_news_encode_workspace_size(int64_t n_titles, int32_t L, int64_t V, int32_t D,
                                       int32_t proj_mode);
int32_t nrms_news_encode(const int64_t* ids, int64_t n_titles, int32_t L, const float* table,
                         int64_t V, const nrms_encoder_weights_t* w, int32_t proj_mode,
                         float* out, void* workspace, size_t workspace_bytes,
                         hipStream_t stream);

/* Same, from a caller-held folded table qkv_table[V] (rows at stride ld_qkv,
 * nrms_qkv_project of the whole embedding table; 0 = 3D): lets an eval loop
 * reuse one projection across calls while the weights are unchanged. */
size_t nrms_news_encode_folded_workspace_size(int64_t n_titles, int32_t L, int32_t D);
int32_t nrms_news_encode_folded(const int64_t* ids, int64_t n_titles, int32_t L,
                                const float* qkv_table, int64_t ld_qkv, int64_t V,
                                const nrms_encoder_weights_t* w, float* out,
                                void* workspace, size_t workspace_bytes, hipStream_t stream);

/* UserEncoder.forward (src/model/NRMS/user_encoder.py:15-26), also
 * NRMS.get_user_vector (src/model/NRMS/__init__.py:63-71): clicked is a
 * [B, N, D] view, element (b, n, d) at clicked[b*stride_b + n*stride_n + d]
 * (strides in floats, multiples of 4; the innermost stride is 1) -> out[B, D].
 * Contiguous input: stride_b = N*D, stride_n = D. The reference caller's
 * torch.stack(..., dim=0).transpose(0, 1) view (src/evaluate.py:220-224) is
 * stride_b = D, stride_n = B*D and is read in place, without a copy. */
size_t nrms_user_encode_workspace_size(int64_t B, int32_t N, int32_t D);
int32_t nrms_user_encode(const float* clicked, int64_t B, int32_t N, int64_t stride_b,
                         int64_t stride_n, const nrms_encoder_weights_t* w, float* out,
                         void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Fused UserEncoder tail (user_encoder.py:15-26 after the projection): raw-exp
 * MHSA over qkv rows b*N + i (stride ld_qkv, 0 = 3D) + additive attention + pooling, one
 * workgroup per user, the context kept in LDS; out[B, D]. N <= 64, reference
 * geometry (D = 300, H = 15, Q = 200). Used by nrms_user_encode and
 * nrms_forward when it applies. Workspace: a packed copy of W_add. */
size_t nrms_user_attention_pool_workspace_size(int64_t B, int32_t N, int32_t D);
int32_t nrms_user_attention_pool(const float* qkv, int64_t ld_qkv, int64_t B, int32_t N,
                                 const nrms_encoder_weights_t* w, float* out, void* workspace,
                                 size_t workspace_bytes, hipStream_t stream);
/* The same with pad_flags[B * N] (uint8, non-zero: position b*N + i holds an
 * all-padding title, src/dataset.py:79-83 -- all such positions carry one
 * news vector, so their qkv rows are equal). With token compaction on
 * (nrms_set_token_compaction) each user is encoded on its distinct rows: the
 * padding positions collapse into one row, counted once per position in the
 * raw-exp sums (bitwise the uncompacted sums for left padding), the context
 * and the softmax / pooling (fp32-rounding-level difference); nrms_forward
 * does the same. Off: as nrms_user_attention_pool. */
int32_t nrms_user_attention_pool_padded(const float* qkv, int64_t ld_qkv, int64_t B, int32_t N,
                                        const uint8_t* pad_flags, const nrms_encoder_weights_t* w, float* out,
                                        void* workspace, size_t workspace_bytes, hipStream_t stream);

/* DotProductClickPredictor.forward (src/model/general/click_predictor/
 * dot_product.py:8-19): out[b, c] = <news[b*stride_b + c*stride_c, :], user[b*stride_u, :]>,
 * strides in floats. Also NRMS.get_prediction (src/model/NRMS/__init__.py:73-84)
 * with B = 1. */
int32_t nrms_score(const float* news, int64_t B, int32_t C, int64_t stride_b,
                   int64_t stride_c, const float* user, int64_t stride_u, int32_t D,
                   float* out, hipStream_t stream);

/* Eval-semantics scoring (src/evaluate.py:245-260): out[k] = <news[news_idx[k]],
 * user[user_idx[k]]> for k < n_pairs — all candidates of all impressions of a
 * split in one launch (each impression's get_prediction, __init__.py:73-84,
 * becomes a contiguous run of pairs). Indices out of range give NaN. */
int32_t nrms_score_pairs(const float* news, int64_t n_news, const float* user, int64_t n_users,
                         const int64_t* news_idx, const int64_t* user_idx, int64_t n_pairs,
                         int32_t D, float* out, hipStream_t stream);

/* (ABI 9) Catalogue-wide recommendation, the end use of the reference's
 * recommend() (src/recommend.py:352-386, which ranks 20 randomly drawn
 * candidates): for every user the K best rows of the whole news table, the
 * rows of exclude[u, :] (the user's history) left out. One fused kernel scores
 * users x news on the matrix cores and keeps a running top-K per user, so the
 * [n_users, n_news] score matrix is never written (topk.hip).
 *   - out_score[u, j] = <news[out_idx[u, j]], user[u]> at fp32-GEMM accuracy,
 *     in the arithmetic of nrms_get_gemm_arith at enqueue time: F32 exact fp32
 *     products, SPLIT_BF16X6 and SPLIT_F16X3 both the exact split-bf16 x6 (no
 *     fp16 planes: the vectors carry no range guarantee). A zero score is
 *     returned as +0. An infinite operand scores NaN in the split modes.
 *   - Per user the entries are sorted by (score descending, row ascending):
 *     np.argsort(-y, kind="stable"). (The reference's np.argsort(-y),
 *     recommend.py:340, leaves ties unspecified.)
 *   - A NaN score ranks after every number, -inf included, as numpy's sort
 *     places it; NaNs order among themselves by row.
 *   - Rows listed in exclude[u, :] ([n_users, n_excl] row-major, or NULL with
 *     n_excl = 0) are never returned for user u. An entry outside [0, n_news)
 *     is ignored and never read through (negative padding, or the len(corpus)
 *     row of PADDED_NEWS); duplicates are allowed.
 *   - When fewer than K rows are eligible the tail is out_idx = -1,
 *     out_score = NaN.
 *   - The result for user u depends only on user[u], exclude[u, :], news and
 *     K, bit for bit: not on n_users, on the other users of the call, on the
 *     chunking or on the grid (a score's accumulation order is a function of k
 *     only), and the first K entries do not depend on K.
 *   - Limits: D = 300, 1 <= K <= 256, 0 <= n_excl <= 256, n_news < 2^31, news
 *     and user 16-byte aligned (workspace 8-byte); anything else returns
 *     NRMS_ERR_UNSUPPORTED (the size function: 0). Null pointers or negative
 *     sizes: NRMS_ERR_INVALID_ARG. n_users == 0 is a successful no-op;
 *     n_news == 0 fills the padding values. A workspace smaller than
 *     nrms_recommend_topk_workspace_size(...): NRMS_ERR_WORKSPACE.
 *   - The workspace holds 512 (K + n_excl <= 128) or 1024 candidate keys of 8
 *     bytes per user and news chunk; the chunk count (1 for many users, up to
 *     64 for few) follows from the shapes, or from NRMS_TOPK_CHUNK = news rows
 *     per chunk in the environment (read once).
 *   - No allocation, no synchronisation, capturable into a hipGraph. */
size_t nrms_recommend_topk_workspace_size(int64_t n_users, int64_t n_news, int32_t D, int32_t K,
                                          int32_t n_excl);
int32_t nrms_recommend_topk(const float* news, int64_t n_news, const float* user, int64_t n_users,
                            int32_t D, const int64_t* exclude, int32_t n_excl, int32_t K,
                            int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                            hipStream_t stream);

/* Per-impression ranking metrics (src/evaluate.py:24-42,160-168) over ragged
 * impressions: impression i owns scores/labels [offsets[i], offsets[i+1]).
 * out[i*4 + {0,1,2,3}] = AUC, MRR, nDCG@5, nDCG@10 in fp64. A non-finite
 * score or an empty impression: all four NaN (roc_auc_score raises, the
 * reference's ValueError branch). One class only: AUC NaN (scikit-learn >= 1.3
 * warns instead of raising) and MRR / nDCG as numpy computes them (all
 * negative: NaN; all positive: MRR = mean(1/rank), nDCG = 1).
 *   - Tie order. The ranking is np.argsort(score, kind="stable")[::-1]:
 *     descending score, and among equal scores (-0 == +0) the candidate with
 *     the LARGER index first: rank_c = 1 + #{j : s_j > s_c or (s_j == s_c and
 *     j > c)}, the order nrms_rank_impressions calls NRMS_RANK_ORDER. MRR and
 *     both nDCGs follow that order, so a positive tied with a later negative
 *     ranks after it; AUC counts a positive tied with a negative as 1/2.
 *   - offsets[n_imp + 1] are ABSOLUTE positions into scores / labels,
 *     non-decreasing; offsets[0] need not be 0 (elements before it belong to
 *     no impression and are never read), and offsets[i] == offsets[i + 1] is
 *     an empty impression (a NaN row). */
int32_t nrms_impression_metrics(const float* scores, const int32_t* labels,
                                const int64_t* offsets, int64_t n_imp, double* out,
                                hipStream_t stream);

/* (ABI 9, added later) Scores and ranks of ragged impressions in one launch:
 * what a MIND prediction file lists. Impression i owns the candidates
 * k in [offsets[i], offsets[i+1]) (rows news_idx[k] of the news table) and
 * the user row imp_user[i]; offsets is non-decreasing and starts at 0.
 *   - Scores. out_score[k] is bitwise what nrms_score_pairs writes for the
 *     pair (news_idx[k], imp_user[i]): both kernels run one shared per-wave
 *     dot (lane-strided float4 FMAs when D % 4 == 0, scalar FMAs otherwise,
 *     then an xor-tree sum), NaN for a candidate row or user row out of
 *     range included. Any D >= 1; rows 16-byte aligned when D % 4 == 0, as
 *     for nrms_score_pairs. The impression's user vector is read once and
 *     held in registers (D % 4 == 0, its first 1024 floats; the scalar path
 *     re-reads it through the caches).
 *   - Ranks are 1-based, over a total order on the fp32 scores: numbers
 *     compare by value (-0 == +0), NaN ranks above +inf, all NaNs are equal.
 *       tie_mode NRMS_RANK_ORDER (0): rank_c = 1 + #{j : s_j > s_c or
 *         (s_j == s_c and j > c)}, j over the same impression: the position
 *         of c in np.argsort(s, kind="stable")[::-1], the order
 *         nrms_impression_metrics uses; always a permutation of 1..n.
 *         [0.5, nan, 0.5, -0.0, 0.0, inf, nan, -inf] orders as 6 1 5 2 0 4 3 7.
 *       tie_mode NRMS_RANK_SHARED (1): rank_c = 1 + #{j : s_j > s_c}; for
 *         finite scores the reference's value2rank (src/evaluate.py:45-48),
 *         sorted(values, reverse=True).index(x) + 1.
 *   - Any impression length is ranked correctly; an empty one writes nothing.
 *     Up to NRMS_RANK_LDS_CANDIDATES candidates the impression's order keys
 *     stay in LDS between scoring and counting. A longer impression takes a
 *     chunked path: its workgroup re-reads the out_score values it wrote
 *     (after a workgroup barrier), NRMS_RANK_LDS_CANDIDATES keys at a time,
 *     and accumulates each chunk's counts in out_rank. Either way ranking
 *     costs n^2 compares per impression, n^2 / 256 per thread; the chunked
 *     path adds n / NRMS_RANK_LDS_CANDIDATES passes over the impression's
 *     out_score and out_rank.
 *   - An impression's outputs depend only on its own candidates and user row,
 *     bit for bit: not on n_imp, on its neighbours or on the grid (one
 *     workgroup per impression; NRMS_RANK_WAVES = 1, 2 or 4 in the
 *     environment, read once, sets its size for measurements and changes no
 *     output).
 *   - Any other tie_mode, a null pointer with n_imp > 0, a negative size or
 *     D < 1: NRMS_ERR_INVALID_ARG, checked before anything else.
 *     n_imp == 0 is a successful no-op; n_imp >= 2^31: NRMS_ERR_UNSUPPORTED.
 *   - No allocation, no synchronisation, no atomics; capturable into a
 *     hipGraph. A launch failure returns NRMS_ERR_HIP. */
#define NRMS_RANK_LDS_CANDIDATES 2048
typedef enum {
  NRMS_RANK_ORDER = 0,
  NRMS_RANK_SHARED = 1
} nrms_rank_ties_t;
int32_t nrms_rank_impressions(const float* news, int64_t n_news, const float* user, int64_t n_users,
                              const int64_t* news_idx, const int64_t* imp_user, const int64_t* offsets,
                              int64_t n_imp, int32_t D, int32_t tie_mode, float* out_score,
                              int32_t* out_rank, hipStream_t stream);

/* NRMS.forward (src/model/NRMS/__init__.py:19-48), eval mode:
 * cand_ids[B, C, L], clicked_ids[B, N, L] -> logits[B, C]. Every one of the
 * B*(C+N) titles gets its news vector (forward semantics), then the user
 * vector and the scores. With title dedupe (nrms_set_title_dedupe, default)
 * all-padding history titles are encoded once per batch and copied, and the
 * UserEncoder projects their q|k|v rows once as well; the logits are bitwise
 * those of encoding and projecting every title. */
size_t nrms_forward_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int64_t V,
                                   int32_t D, int32_t proj_mode);
int32_t nrms_forward(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                     int32_t N, int32_t L, const float* table, int64_t V,
                     const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                     int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                     hipStream_t stream);

/* nrms_forward with per-stage timing: stage_events[i] (n_events =
 * NRMS_FORWARD_STAGES + 1 caller-created HIP events, or n_events = 0 for none)
 * is recorded on the stream before stage i and the last one after the final
 * stage. Stages: nrms_forward_stage_name(0 .. NRMS_FORWARD_STAGES - 1) =
 * qkv_news (Q|K|V projection), news_fused (news attention + additive pooling,
 * incl. the padding-group and recheck launches), qkv_user, user_fused, score. */
#define NRMS_FORWARD_STAGES 5
int32_t nrms_forward_timed(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                           int32_t N, int32_t L, const float* table, int64_t V,
                           const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                           int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                           hipStream_t stream, hipEvent_t* stage_events, int32_t n_events);
const char* nrms_forward_stage_name(int32_t stage);

/* (ABI 9, added later) The forward with its weight-derived state prepared once.
 *
 * nrms_forward recomputes, in every call, data that depends on the weights
 * alone: both encoders' split Q|K|V weights, both packed W_add (with the news
 * kernel's zero / NaN rows) and, in the folded mode, the projected vocabulary
 * [V][nrms_qkv_row_stride(D)]. Between two parameter updates those are bitwise
 * the same from call to call. nrms_forward_prepare enqueues exactly that work
 * (the same launches on the same inputs, so the same bits) into a caller-owned
 * state buffer, and nrms_forward_prepared runs the rest of the step against
 * it: everything that reads a token id (the titles' classification, the news
 * vectors, the user rows, the scores) still runs in every call. The logits are
 * bitwise nrms_forward's under the same arithmetic, dedupe and compaction
 * settings.
 *
 *   - The caller owns the buffer (nrms_forward_state_size bytes, 256-B aligned)
 *     and the nrms_forward_state_t that describes it; the library allocates
 *     nothing and keeps no pointer. With with_folded_table the table is the
 *     first V * nrms_qkv_row_stride(D) floats of the buffer.
 *   - The state is invalid once any parameter it was made from (the embedding
 *     table, either encoder's W_Q / W_K / W_V weight or bias, either W_add
 *     weight) changes, or under another GEMM arithmetic: the caller prepares
 *     again (into the same buffer if captured graphs read it). b_add and q_add
 *     are read by the step itself.
 *   - Under NRMS_GEMM_F32 there are no packs: the state holds the folded table
 *     only and the step packs W_add as nrms_forward does.
 *   - A step only reads the state, so any number of forwards (other batch
 *     sizes, other streams) may share one; everything a step writes lives in
 *     its own workspace. Stream order is the caller's: the prepare must have
 *     completed, or precede the step on its stream.
 *   - nrms_forward_prepare never synchronises and can be captured in a graph.
 *   - nrms_forward_prepared_workspace_size does not depend on V (the table is
 *     not in the workspace); it covers every projection mode, the per-token
 *     rows of the direct mode included. A call that resolves to the folded
 *     mode needs nrms_forward_prepared_folded_workspace_size only.
 *   - table is read in the direct mode only (it may be null otherwise).
 *   - NRMS_ERR_INVALID_ARG, with nothing launched: state null, prepared for
 *     another V or D or under another arithmetic than the current one, or
 *     without a folded table on a call that resolves to the folded mode.
 *     NRMS_ERR_WORKSPACE: a state buffer or workspace that is too small.
 *   - Stages and event positions as nrms_forward_timed; qkv_news holds the
 *     classification launches (folded) or the per-token projection (direct). */
#define NRMS_STATE_FOLDED_TABLE 1   /* flags of nrms_forward_state_t */
#define NRMS_STATE_QKV_PACKS 2
#define NRMS_STATE_ADD_PACKS 4
typedef struct {
  void* buffer;        /* device pointer of the state buffer               */
  size_t bytes;        /* its size                                         */
  int64_t V;           /* vocabulary rows it was prepared for              */
  int32_t D;
  int32_t ld_qkv;      /* q|k|v row stride of the folded table (floats)    */
  int32_t gemm_arith;  /* nrms_gemm_arith_t it was prepared under          */
  int32_t flags;       /* NRMS_STATE_*: what the buffer holds              */
} nrms_forward_state_t;
size_t nrms_forward_state_size(int64_t V, int32_t D, int32_t with_folded_table);
int32_t nrms_forward_prepare(const float* table, int64_t V, const nrms_encoder_weights_t* news_w,
                             const nrms_encoder_weights_t* user_w, int32_t with_folded_table, void* state_buf,
                             size_t state_bytes, nrms_forward_state_t* state, hipStream_t stream);
size_t nrms_forward_prepared_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int32_t D);
size_t nrms_forward_prepared_folded_workspace_size(int64_t B, int32_t C, int32_t N, int32_t L, int32_t D);
int32_t nrms_forward_prepared(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                              int32_t N, int32_t L, const float* table, int64_t V,
                              const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                              int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                              hipStream_t stream, const nrms_forward_state_t* state);
int32_t nrms_forward_prepared_timed(const int64_t* cand_ids, const int64_t* clicked_ids, int64_t B, int32_t C,
                                    int32_t N, int32_t L, const float* table, int64_t V,
                                    const nrms_encoder_weights_t* news_w, const nrms_encoder_weights_t* user_w,
                                    int32_t proj_mode, float* logits, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream, const nrms_forward_state_t* state,
                                    hipEvent_t* stage_events, int32_t n_events);

/* ---------------------------------------------------------------------------
 * (ABI 9, added later) The Exp1 model (src/model/Exp1/): NRMS plus a category
 * and a subcategory view of every article, pooled with the title vector by a
 * second additive attention, and a learned position embedding added to the
 * user history before its self-attention. Eval mode. The title encoder, the
 * user encoder and the scorers are the NRMS entry points above; these three
 * add what Exp1 has on top (csrc/views.hip).
 *
 * Element encoders (news_encoder.py:36-43): view(id) = relu(emb[id] W^T + b).
 * The reference shares one embedding table between both; emb_cat and emb_sub
 * may be the same pointer. final_attention is an AdditiveAttention over the
 * stacked views [title, category, subcategory] (news_encoder.py:104-110). */
typedef struct {
  const float* emb_cat; const float* emb_sub; int64_t n_cat; int32_t emb_dim;  /* [C, E] each; the reference shares one table */
  const float* w_cat; const float* b_cat;     /* [D, E], [D] */
  const float* w_sub; const float* b_sub;     /* [D, E], [D] */
  const float* w_fin; const float* b_fin; const float* q_fin;  /* final_attention: [Q, D], [Q], [Q] */
  int32_t d_model; int32_t query_dim;
} nrms_views_weights_t;

/* The weight-derived state: for every id c in [0, C)
 *   cat_vec[c] = relu(emb_cat[c] W_cat^T + b_cat), sub_vec[c] likewise, and
 *   each row's final-attention logit q_fin . tanh(W_fin v + b_fin),
 * laid out in `state` as floats: cat_vec[C, D], sub_vec[C, D], cat_logit[C],
 * sub_logit[C] (nrms_views_state_size bytes; 16-byte aligned). Id 0 is an
 * ordinary row (padding_idx only affects gradients). fp32 FMA chains; a ReLU
 * zero is an exact +0. The state is invalid once any field of w changes: the
 * caller prepares again. One launch, nothing allocated, no synchronisation.
 * Limits: E + D <= 12,280, Q <= 208, C <= 2^24 (else NRMS_ERR_UNSUPPORTED; the
 * size function: 0). Null pointers, n_cat < 0 or a non-positive dimension:
 * NRMS_ERR_INVALID_ARG; a short state buffer: NRMS_ERR_WORKSPACE. */
size_t nrms_views_state_size(int64_t n_cat, int32_t D);
int32_t nrms_views_prepare(const nrms_views_weights_t* w, void* state, size_t state_bytes, hipStream_t stream);

/* NewsEncoder.forward after the title encoder (news_encoder.py:95-111), for n
 * articles: title_vec[n, D] (the title encoder's output), category[n] and
 * subcategory[n] ids, state from nrms_views_prepare under the same w.
 *   logit_t = q_fin . tanh(W_fin title_vec[r] + b_fin)   (exact-f32 MFMA GEMM
 *             in every arithmetic mode; one float per row in the workspace)
 *   (w_t, w_c, w_s) = softmax(logit_t, cat_logit[cat], sub_logit[sub]),
 *             the maximum subtracted first
 *   out[r] = (w_t title_vec[r] + w_c cat_vec[cat]) + w_s sub_vec[sub]
 * out == title_vec is allowed and bitwise equal to the out-of-place call. A
 * category or subcategory outside [0, C) gives a NaN row and is never read
 * through; a title vector holding NaN gives a NaN row; no other row changes.
 * D % 4 == 0, Q <= 208, title_vec / state / out 16-byte aligned (else
 * NRMS_ERR_UNSUPPORTED). Two launches, nothing allocated. */
size_t nrms_news_views_fuse_workspace_size(int64_t n);
int32_t nrms_news_views_fuse(const float* title_vec, int64_t n, const int64_t* category,
                             const int64_t* subcategory, const nrms_views_weights_t* w, const void* state,
                             float* out, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* UserEncoder's position embedding (user_encoder.py:27-28) into a contiguous
 * out[B, N, D]: out[b, i, :] = x[b, i, :] + pos[i, :], pos[N, D].
 *   rows != NULL: x[b, i] = src[rows[b * N + i]], a gather from the
 *     [n_src_rows, D] table src (the eval path's news-vector table); a row
 *     outside [0, n_src_rows) gives a NaN row and is never read through.
 *   rows == NULL: src is a [B, N, D] view, element (b, i, d) at
 *     src[b * stride_b + i * stride_n + d] (strides in floats, >= 0): the
 *     views nrms_user_encode takes, the transpose(0, 1) one included.
 * One fp32 add per element: bitwise torch's x + P. 16-byte lanes when D % 4 ==
 * 0, src / pos / out are 16-byte aligned and (view form) the strides are
 * multiples of 4; scalar lanes otherwise, same result. N * D < 2^31. */
int32_t nrms_rows_add_position(const float* src, int64_t n_src_rows, const int64_t* rows, int64_t B,
                               int32_t N, int64_t stride_b, int64_t stride_n, const float* pos, int32_t D,
                               float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Training kernels: the train-mode forward pieces and the backward of the path
 * above, as src/train.py:202-236 needs them (loss.backward(), Adam step). The
 * Python glue (newsrecommendationsystem_amd/train_hip.py) chains them in a
 * torch.autograd.Function. Gradient outputs named d_* are ACCUMULATED into
 * (callers zero them), dx / dqkv / dnews outputs are overwritten. fp32; the
 * GEMMs of the backward (dx = dY W and dW += dY^T X) run on split-bf16 x6
 * under both split modes of nrms_set_gemm_arith and on f32 MFMA under
 * NRMS_GEMM_F32 (dW also when dY or X is not 16-byte aligned); the GEMM of
 * nrms_additive_forward_train is f32 MFMA in every mode. */

/* F.dropout(x, p, training=True) (news_encoder.py:38-40,43-45): y[i] = x[i] /
 * (1-p) if u(seed, i) >= p else 0, u a counter-based uniform (splitmix64 of
 * seed and i), so the same call on the gradient is the backward. 0 <= p < 1;
 * x == y allowed. */
int32_t nrms_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed,
                     hipStream_t stream);

/* AdditiveAttention.forward (additive.py:27-53) keeping what the backward
 * needs: y_tanh[n_seq*L, Q] = tanh(x W^T + b), scores[n_seq*L] = y . q,
 * out[n_seq, D] = sum_l softmax_l(scores) x_l. */
int32_t nrms_additive_forward_train(const float* x, int64_t n_seq, int32_t L,
                                    const nrms_encoder_weights_t* w, float* y_tanh, float* scores,
                                    float* out, hipStream_t stream);

/* Its backward: dx[n_seq*L, D] (written) from dout[n_seq, D]; d_w_add [Q, D],
 * d_b_add [Q], d_q_add [Q] accumulated. Workspace:
 * nrms_additive_backward_workspace_size bytes. */
size_t nrms_additive_backward_workspace_size(int64_t n_seq, int32_t L, int32_t D, int32_t Q);
int32_t nrms_additive_backward(const float* x, int64_t n_seq, int32_t L,
                               const nrms_encoder_weights_t* w, const float* y_tanh,
                               const float* scores, const float* dout, float* dx, float* d_w_add,
                               float* d_b_add, float* d_q_add, void* workspace,
                               size_t workspace_bytes, hipStream_t stream);

/* Backward of nrms_self_attention over per-token rows (row s*L + i of
 * qkv[n_seq*L, 3D]): dqkv[n_seq*L, 3D] (written) from dctx[n_seq*L, D],
 * recomputing the raw-exp attention (multihead_self.py:15-23). L <= 64. */
int32_t nrms_self_attention_backward(const float* qkv, const float* dctx, int64_t n_seq,
                                     int32_t L, const nrms_encoder_weights_t* w, float* dqkv,
                                     hipStream_t stream);

/* Backward of nrms_qkv_project (identity rows): dx[rows, D] = dqkv [W_Q; W_K;
 * W_V] (written; NULL skips it), d_w_qkv[3D, D] += dqkv^T x, d_b_qkv[3D] +=
 * column sums of dqkv. Workspace: nrms_qkv_project_backward_workspace_size. */
size_t nrms_qkv_project_backward_workspace_size(int32_t D);
int32_t nrms_qkv_project_backward(const float* x, int64_t rows, const nrms_encoder_weights_t* w,
                                  const float* dqkv, float* dx, float* d_w_qkv, float* d_b_qkv,
                                  void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Backward of nrms_score (dot_product.py:8-19): dnews[B, C, D] (contiguous,
 * written) = dlogits[b, c] user[b]; duser[B, D] (written) = sum_c dlogits[b, c]
 * news[b, c]. Strides as nrms_score. */
int32_t nrms_score_backward(const float* news, int64_t B, int32_t C, int64_t stride_b,
                            int64_t stride_c, const float* user, int64_t stride_u, int32_t D,
                            const float* dlogits, float* dnews, float* duser, hipStream_t stream);

/* Backward of nrms_embedding_gather as nn.Embedding(padding_idx) computes it:
 * dtable[ids[t]] += dx[t] for every t with ids[t] != padding_idx (dense
 * [V, D] gradient, accumulated). Float atomics: the additions to one row land
 * in arrival order, so results may differ by rounding from run to run; the _ws
 * form below is deterministic. */
int32_t nrms_embedding_backward(const int64_t* ids, int64_t n_tok, const float* dx, int64_t V,
                                int32_t D, int64_t padding_idx, float* dtable,
                                hipStream_t stream);

/* (ABI 8) The same gradient, deterministic: the tokens are sorted by id (a
 * stable radix sort) and each row's contributions added in a fixed order --
 * token order for an id with at most 256 tokens (the CPU reference's
 * index_add order, bitwise), and for a longer run sums of 64-token segments
 * (each in token order) added in segment order (round 6: parallel; within
 * fp32 rounding of index_add). Bitwise reproducible. Workspace:
 * nrms_embedding_backward_workspace_size(n_tok, V) bytes; n_tok, V < 2^31. */
size_t nrms_embedding_backward_workspace_size(int64_t n_tok, int64_t V);
int32_t nrms_embedding_backward_ws(const int64_t* ids, int64_t n_tok, const float* dx, int64_t V,
                                   int32_t D, int64_t padding_idx, float* dtable, void* workspace,
                                   size_t workspace_bytes, hipStream_t stream);

/* torch.optim.Adam step (src/train.py:127; amsgrad off, no weight decay) on
 * one parameter, in torch's operation order; `step` counts from 1. */
int32_t nrms_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float lr, float beta1, float beta2, float eps, int64_t step,
                       hipStream_t stream);

/* The same Adam step over many parameters: `tensors` is a HOST array of n
 * descriptors, read during the call; up to 32 of them go to the device by
 * value in the kernel arguments of one launch (ceil(n / 32) launches). All
 * tensors share lr / betas / eps / step. Replaces one nrms_adam_step launch
 * per parameter (torch.optim.Adam's foreach path). `first_block` is ignored
 * (kept for layout stability). */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int64_t first_block;
} nrms_adam_tensor_t;

int32_t nrms_adam_step_multi(const nrms_adam_tensor_t* tensors, int32_t n, float lr, float beta1,
                             float beta2, float eps, int64_t step, hipStream_t stream);

/* (ABI 9, added later) Batch assembly of the fit loop from a device-resident
 * training set (BaseDataset.__getitem__ + default collate, src/dataset.py:
 * 64-85). titles[n_title_rows, L]: the corpus titles (the caller appends an
 * all-zero row for PADDED_NEWS); sample_rows[n_samples, C + N]: per training
 * sample the title rows of its C candidates (positive first) and of its N
 * history slots (left-padded with the zero row); sample_idx[B]: the samples of
 * this batch. Writes cand_ids[B, C, L] and clicked_ids[B, N, L]:
 *   out[b, j, l] = titles[sample_rows[sample_idx[b], j], l].
 * A sample_idx[b] outside [0, n_samples) or a row outside [0, n_title_rows) is
 * never dereferenced: that sample's titles, or that title, are written as
 * zeros. One launch, nothing allocated, no host synchronisation. */
int32_t nrms_train_batch_gather(const int64_t* titles, int64_t n_title_rows, int32_t L,
                                const int32_t* sample_rows, int64_t n_samples, int32_t C, int32_t N,
                                const int64_t* sample_idx, int64_t B,
                                int64_t* cand_ids, int64_t* clicked_ids, hipStream_t stream);

/* (ABI 9, added later) nrms_train_batch_gather from a set that keeps the raw
 * impressions of a behaviors.tsv: the K negatives of every sample are drawn in
 * the launch, so each epoch sees new ones. A sample is one positive click:
 * pos_row[n_samples] its title row, pos_imp[n_samples] its impression;
 * neg_off[n_imps + 1] / neg_rows[n_neg]: CSR of the title rows of each
 * impression's label-0 candidates; imp_hist[n_imps]: impression -> distinct
 * history; hist_rows[n_hists, N]: the history's title rows (left-padded with
 * the zero row). With s = sample_idx[b], i = pos_imp[s], n = neg_off[i + 1] -
 * neg_off[i]:
 *   cand_ids[b, 0, :]     = titles[pos_row[s]]
 *   cand_ids[b, 1 + j, :] = titles[neg_rows[neg_off[i] + position_j]]
 *   clicked_ids[b, k, :]  = titles[hist_rows[imp_hist[i], k]]
 * The positions are a uniform ordered K-subset without replacement, a function
 * of (seed, epoch, s) alone; all arithmetic uint64 and wrapping, mix() the
 * splitmix64 finaliser (z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31):
 *   base = mix(mix(seed) + epoch)
 *   for j in 0 .. K-1:  r = ((mix(base + 16 s + j) >> 32) * (n - j)) >> 32
 *                       for p in ascending order of position_0..j-1: r += (r >= p)
 *                       position_j = r
 * No index is dereferenced unchecked: a sample_idx[b] outside [0, n_samples)
 * zeroes the sample's titles; a pos_imp / imp_hist / row outside its table, a
 * neg_off pair that decreases, is negative or runs past n_neg, and slots
 * 1 + j with j >= n zero the titles that depend on them. K outside 0..15:
 * NRMS_ERR_UNSUPPORTED, nothing launched. One launch, nothing allocated, no
 * host synchronisation. */
int32_t nrms_train_batch_sample_gather(const int64_t* titles, int64_t n_title_rows, int32_t L,
                                       const int32_t* pos_row, const int32_t* pos_imp, int64_t n_samples,
                                       const int64_t* neg_off, int64_t n_imps,
                                       const int32_t* neg_rows, int64_t n_neg,
                                       const int32_t* imp_hist, const int32_t* hist_rows, int64_t n_hists,
                                       int32_t K, int32_t N, const int64_t* sample_idx, int64_t B,
                                       uint64_t seed, int64_t epoch,
                                       int64_t* cand_ids, int64_t* clicked_ids, hipStream_t stream);

/* (ABI 9, added later) CrossEntropyLoss against class 0 and its gradient
 * (src/train.py:126,205-206) in one launch, B >= 1 rows of any C >= 1:
 *   loss_out[0]   = mean_b(logsumexp(z_b) - z_b0)       (DEVICE pointer)
 *   dlogits[b, c] = (softmax(z_b)[c] - [c == 0]) / B
 * with the row maximum subtracted first, as torch's log_softmax: a row holding
 * +inf or NaN gives a NaN loss. The per-row losses are summed in a fixed order
 * (fp64, no atomics): bitwise reproducible. One workgroup: meant for training
 * batches (B in the hundreds), not for scoring a split. */
int32_t nrms_xent_class0(const float* logits, int64_t B, int32_t C,
                         float* dlogits, float* loss_out, hipStream_t stream);

/* (ABI 9, added later) The FedAvg exchange's two copies (csrc/fedavg.hip):
 * n parameters to and from one contiguous fp32 buffer, the buffer an
 * all-reduce sums. `offset` counts floats into flat.
 *   nrms_params_pack:        flat[offset_t + i] = data_t[i]
 *   nrms_params_unpack_div:  data_t[i] = flat[offset_t + i] / divisor
 * for 0 <= i < numel_t. The quotient is the correctly rounded IEEE fp32
 * division (numpy.float32(x) / numpy.float32(divisor), subnormals kept), not a
 * reciprocal multiply; divisor 1 copies the bits. `tensors` is a HOST array
 * read during the call; up to 32 descriptors go to the device by value in one
 * launch's arguments (ceil(n / 32) launches). 16-byte loads and stores where a
 * tensor's base and its place in flat are both 16-byte aligned, scalar
 * otherwise and for the last numel % 4 floats: neither alignment nor numel % 4
 * matters for the result. flat must hold max_t(offset_t + numel_t) floats;
 * ranges must not overlap. Nothing allocated, no host synchronisation,
 * graph-capturable. numel == 0 is skipped; n == 0: NRMS_OK, nothing launched.
 * NRMS_ERR_INVALID_ARG, nothing launched: n < 0, a null `tensors` with n > 0,
 * numel < 0 or offset < 0, a null data or flat pointer with numel > 0, a
 * divisor that is 0 or NaN. */
typedef struct {
  float* data;
  int64_t numel;
  int64_t offset;
} nrms_flat_tensor_t;

int32_t nrms_params_pack(const nrms_flat_tensor_t* tensors, int32_t n, float* flat, hipStream_t stream);
int32_t nrms_params_unpack_div(const nrms_flat_tensor_t* tensors, int32_t n, const float* flat,
                               float divisor, hipStream_t stream);

/* ---------------------------------------------------------------------------
 * Host-side readers of the eval split (csrc/tsv_io.hip). HOST pointers, no
 * stream: they replace the Python line loop of the reference's readers
 * (src/evaluate.py:55-71 news_parsed.tsv, :133-157 behaviors.tsv) for the
 * MIND id form ("N<digits>" without leading zeros). Any other form -- a '\r',
 * a non-ASCII byte, a cell outside the plain form below -- returns
 * NRMS_ERR_UNSUPPORTED and the caller reads the file on its general path
 * (newsrecommendationsystem_amd/data.py), which also raises the reference's
 * errors. Values equal the general path's wherever these accept the input.
 *
 * behaviors.tsv: non-empty lines of at least five tab-separated columns
 * (impression id, user, time, history, impressions); impressions cell
 * "N<id>-<label>" tokens separated by single spaces (labels <= 9 digits);
 * history cell blank or "N<id>" tokens separated by single spaces (outer
 * spaces ignored, as str.strip). nrms_behaviors_scan checks the bytes and
 * writes upper bounds of the lines, candidate tokens and history ids into
 * counts[3]; nrms_behaviors_parse takes those (or any) capacities[3] and
 * fills, per line k: fields[10 k + 2 c], [.. + 1] = byte span of column c;
 * the candidates' numeric ids and labels and their count per line; the
 * history ids and their count; and hist_user[k] = the index of line k's
 * history string among the distinct history strings in first-seen order (an
 * empty field counts as " ", as the reference's fillna(' ')); counts[4] =
 * lines, candidates, history ids, distinct histories. NRMS_ERR_WORKSPACE
 * when a capacity is short. */
int32_t nrms_behaviors_scan(const char* buf, int64_t len, int64_t* counts);
int32_t nrms_behaviors_parse(const char* buf, int64_t len, const int64_t* capacity, int64_t* counts,
                             int64_t* fields, int64_t* cand_num, int32_t* labels, int64_t* cand_count,
                             int64_t* hist_num, int64_t* hist_count, int64_t* hist_user);
/* (ABI 9, added later) The same pair for splits with or without labels (MIND's
 * test split lists "N1 N2 N3"): each candidate token is "N<id>-<label>" or
 * "N<id>", and a token without a label gets label -1. Same signatures,
 * outputs and rejection rules otherwise; the scan bounds the candidates by
 * the tokens of each line's impressions column, not by the '-' bytes. */
int32_t nrms_behaviors_scan_any(const char* buf, int64_t len, int64_t* counts);
int32_t nrms_behaviors_parse_any(const char* buf, int64_t len, const int64_t* capacity, int64_t* counts,
                                 int64_t* fields, int64_t* cand_num, int32_t* labels, int64_t* cand_count,
                                 int64_t* hist_num, int64_t* hist_count, int64_t* hist_user);
/* news_parsed.tsv: a header naming "id" and "title" columns, then rows whose
 * id is N<digits> and whose title is a list literal of exactly L ints
 * ("[12, 7, 0, ...]"). Writes *n_rows, and for the first `capacity` rows the
 * numeric id, the id's byte span [2] and the title [L]; NRMS_ERR_WORKSPACE
 * when there are more rows than `capacity` (*n_rows says how many). */
int32_t nrms_news_parse(const char* buf, int64_t len, int32_t L, int64_t* n_rows, int64_t* ids,
                        int64_t* id_spans, int64_t* titles, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* NRMS_HIP_H */
