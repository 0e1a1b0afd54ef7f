/*
 * sola_hip.h — C ABI of libsola_hip.so: the MI355X (gfx950) implementation of SOLA's track-selection hot path.
 *
 * The reference (cvlab-kaist/SOLA) has no FFI layer: its boundary is the Python object interface used by
 * train.py / inference.py / evaluator.py.  The entry points below are what a binding for that
 * path binds; each cites the reference interface it replaces (paths relative to the reference root).
 * sola_amd/module.py, sola_amd/loss.py and sola_amd/seg_utils.py are the ctypes bindings that present the
 * reference's own Python interface on top of this ABI (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; every pointer named *dev* is a device (HBM) pointer owned by the caller;
 *   - every function returns 0 on success or a negative SolaStatus; sola_last_error() gives the message of the
 *     last failure on the calling thread; nothing throws across the ABI;
 *   - all work is enqueued asynchronously on the given hipStream_t (passed as void*; NULL = default stream);
 *   - a context is re-entrant across contexts but not thread-safe on one context;
 *   - fp32 row-major tensors; activations are channels-last: object tokens [B,N,T,d], text tokens [B,L,D].
 */
#ifndef SOLA_HIP_H
#define SOLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum SolaStatus {
    SOLA_OK = 0,
    SOLA_ERR_ARG = -1,       /* invalid argument / unsupported shape */
    SOLA_ERR_HIP = -2,       /* a HIP runtime call failed */
    SOLA_ERR_WEIGHT = -3,    /* unknown weight name, wrong size, or weights missing at forward time */
    SOLA_ERR_WORKSPACE = -4, /* workspace too small */
    SOLA_ERR_STATE = -5      /* call sequence error (e.g. backward without a saved forward) */
} SolaStatus;

/* configs["model"] of the reference (configs/mevis/default.yaml:3-13; consumed at module/module.py:59-63,76,19).
 * num_heads is hard-coded to 8 in the reference (module/module.py:13-15). */
typedef struct SolaConfig {
    int32_t object_token_dim;
    int32_t lang_token_dim;
    int32_t n_layers;
    int32_t max_temporal_length;
    int32_t n_negative;
    int32_t n_groups;        /* encoder GroupNorm groups */
    int32_t n_groups_module; /* alignment-layer GroupNorm groups */
    int32_t num_heads;
} SolaConfig;

typedef struct SolaCtx SolaCtx;

const char* sola_last_error(void);
const char* sola_version(void);

/* ---- context: replaces LanguageAlignedTrackSelectionModule.__init__ / .to(device) (module/module.py:55-110) ---- */
int sola_ctx_create(const SolaConfig* cfg, int device, SolaCtx** out);
int sola_ctx_destroy(SolaCtx* ctx);

/* Number of state_dict tensors and their names/sizes, in the reference's state_dict order
 * (84 entries for the default config: 83 parameters + the Fourier buffer: module/module.py:74-110, tools/attention.py:26-29). */
int sola_num_weights(const SolaCtx* ctx);
int sola_weight_info(const SolaCtx* ctx, int index, const char** name, int64_t* numel);

/* Borrow a device pointer for one state_dict tensor (fp32, contiguous).  Replaces load_state_dict / parameter
 * access (inference.py:33, train.py:46).  The pointer must stay valid until replaced or the ctx is destroyed. */
int sola_set_weight(SolaCtx* ctx, const char* name, const void* dev_ptr, int64_t numel);

/* Tell the context that weight VALUES changed in place (optimizer step): the standardised conv weights
 * (module/ws.py:9-13) are recomputed at the next forward.  recompute_every_forward=1 mirrors the reference,
 * which re-standardises on every call. */
int sola_weights_changed(SolaCtx* ctx);
int sola_set_ws_policy(SolaCtx* ctx, int recompute_every_forward);

/* Inference arithmetic of the dense contractions (convs and projections, 98 % of the FLOPs):
 *   0  exact f32: v_mfma_f32_32x32x2_f32 on f32 operands (default);
 *   1  split-f16: every operand value x is carried as (f16 hi, f16 lo) with hi + lo = x to 22 bits, in the same 4 bytes,
 *      and each product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with f32 accumulation - 3/16 of the f32
 *      matrix-pipe time (gfx950 has no xf32/TF32).  Softmax, GroupNorm statistics, score head and losses stay f32.
 *   2  16-bit activation STORAGE (sola_forward only; BASELINE configs C2 / C4 name bf16 / fp16 runs of this path): every
 *      activation between two kernels is a plain f16 (2 bytes per element), every product of the convs / projections /
 *      attention ONE f16 MFMA with f32 accumulation; softmax, GroupNorm statistics, biases, score head, losses stay f32.
 *      f16 rather than bf16: 11 significant bits for the same bytes, its range covered by the scales + guard below.  A
 *      reduced-precision mode with a heavy-tailed error (logits of magnitude ~10: 0.8 % rms, 99.5 % within 0.25, worst ~0.7;
 *      tests/test_gpu_f16.py states the bound), never the default; needs object_token_dim and lang_token_dim %% 64 == 0.
 *      sola_forward and sola_forward_ragged (round 3) both run it; a tripped range guard repeats the call in exact f32.
 * In training (sola_forward_train / sola_backward) precision 1 runs every GEMM of the step (forward, dX and dW of the
 * projections and convs) on split-f16 casts of the f32 activations / gradients, from 1024 token rows on; attention and
 * GroupNorm backward and everything saved for the backward stay f32.  Since round 3 the weight-gradient products dW = dY^T X
 * take PLAIN f16 casts (one MFMA per product; sola_tune "train_dw_f16" 0 = split pairs there too): a sum over >= 1024 token
 * rows averages the operand rounding out - median per-matrix error 1e-4 against the exact-f32 step, worst tensor and gradient
 * cosine unchanged (tests/test_gpu_backward.py::test_split_training_weight_gradient_products_on_f16_operands).  Precision 2 in training is MIXED precision (BASELINE
 * config C2): the same step with plain-f16 casts and ONE f16 MFMA per product (f32 accumulation, per-tensor power-of-two
 * scales); activations, statistics, softmax, saved tensors and master weights stay f32.  Reduced precision with a stated
 * tolerance: losses within 1 %, gradient cosine >= 0.95 against the exact-f32 step (tests/test_gpu_backward.py).
 *   3  TRAINING only (sola_forward_train[_ragged] / sola_backward[_ragged]; the inference entry points return SOLA_ERR_ARG):
 *      the mixed-precision step of precision 2 with BFLOAT16 GEMM operands (v_cvt_pk_bf16_f32 casts, v_mfma_f32_32x32x16_bf16,
 *      f32 accumulation) - the "bf16 training" BASELINE config C2 names.  8 significant bits instead of 11 for the same MFMA
 *      rate; the tolerance is stated in tests/test_gpu_backward.py next to the f16 one. */
int sola_set_precision(SolaCtx* ctx, int precision);
/* Range handling of precision 1 in sola_forward / sola_forward_ragged.  The split-f16 pairs keep 22 significant bits for
 * every value within 2^-16 of its tensor's largest, on top of a per-tensor power-of-two scale:
 *   - the caller's object tokens and text tokens and every projection weight matrix get a data-dependent scale found on the
 *     device (largest magnitude -> [2^13, 2^14)), undone in the consuming GEMM's epilogue: any input scale, weight outliers;
 *   - the activations between the stages use a fixed scale; every kernel that writes one checks the value against the f16
 *     range (non-finite or |v| >= 65000 sets a guard word), and when the weights change the rms each GroupNorm will emit,
 *     sqrt(mean(gamma^2 + beta^2)), is checked against [2^-6, 2^9].
 * With the guard enabled (default) the forward reads the guard words (an 8-byte copy and ONE host wait per call) and, when
 * one is set, repeats the call on the exact-f32 kernels in the same workspace, so the caller never sees a result computed
 * outside the format's range.  The wait is for an EVENT behind the last launch of the sequence that can set a guard bit
 * (precision 1: the last object -> language attention; precision 2: the out-projection behind it), not for the stream: a
 * guarded call may return while its tail - that out-projection, the last GroupNorm, the score head - is still running, so
 * its outputs are complete ON THE STREAM, as those of an unguarded call, not on return.  The repeat is enqueued on the same
 * stream behind that tail and overwrites the outputs in stream order.  enable = 0 keeps the call fully asynchronous (also while the stream is
 * being captured into a graph, where the check is skipped automatically); the words can then be read with
 * sola_split_fallback_count: *count = calls repeated in f32 so far, *last_guard = guard bits of the last checked call
 * (bit 0: a value left the f16 range, bit 1: GroupNorm weights outside the covered magnitude).  Once bit 1 has been seen for the
 * current weights, further calls skip the split pass and run the exact-f32 kernels directly (one line on stderr says so) until a
 * weight changes.  The guard words, their pinned host copy and the precision switch of the repeat belong to the CONTEXT: a
 * context serves one stream / one host thread at a time (use one context per stream for concurrent calls). */
int sola_set_split_guard(SolaCtx* ctx, int enable);

/* Operand-cast arena of the reduced-precision TRAINING modes (no reference counterpart).  In precisions 1 / 2 / 3 the training forward
 * keeps the 16-bit operand casts of its GEMM inputs so that the backward's weight-gradient products read them instead of casting the
 * same activations again (sola_tune "train_x16_keep").  The memory is the CALLER's: `dev_ptr` (256-byte aligned, `bytes` long) is
 * borrowed until it is replaced (null = keep nothing; the backward then casts as before - results are bit-identical either way).
 * Replace it only between a backward and the next forward.  sola_x16_arena_info reports what the LAST training forward asked for in
 * total (`need_bytes`, whether it fitted or not), the capacity and the bytes in use, so a caller can grow its buffer between steps
 * (sola_amd/module.py keeps a torch tensor 1/8 above the largest need seen).  Round 4; before, the ctx allocated this arena itself. */
int sola_set_x16_arena(SolaCtx* ctx, void* dev_ptr, size_t bytes);
int sola_x16_arena_info(const SolaCtx* ctx, size_t* need_bytes, size_t* capacity_bytes, size_t* used_bytes);
/* What the LAST training forward of the context decided for attention site `site` (0 inter-object, 1 motion, 2 object -> language) of
 * alignment layer `layer` - read-only, changes nothing: *qkv16 = q / k / v (and, in the backward, dq / dk / dv) are bfloat16 rows only,
 * *o16 = the attention output exists as bfloat16 rows only, *prenorm16 = the sub-block's pre-norm rows are bfloat16 (sola_tune
 * "train_bf16_store" 1 / 3 / 2).  Any pointer may be null.  All zero before the first training forward and outside the bf16 step. */
int sola_train_site_flags(const SolaCtx* ctx, int layer, int site, int* qkv16, int* o16, int* prenorm16);
int sola_split_fallback_count(const SolaCtx* ctx, int64_t* count, int32_t* last_guard);
/* f32 rows -> split-f16 rows (same bytes per element; K % 8 == 0); scale must be a power of two */
int sola_cast_sp16(const float* dev_in, int ld_in, float* dev_out, int ld_out, int64_t rows, int K, float scale, void* stream);
/* The same conversion with a data-dependent power-of-two scale, for operands whose magnitude the host does not know
 * (gradients: mostly below the f16 normal range).  dev_scal = 2 floats: [0] receives max|in| (float bits), [1] the
 * inverse of the scale applied (max|in| lands in [2^13, 2^14)); pass dev_scal + 1 as dev_out_scale below. */
int sola_cast_sp16_auto(const float* dev_in, int ld_in, float* dev_out, int ld_out, int64_t rows, int K, float* dev_scal, void* stream);
/* C = out_scale * (A W^T) + bias (+ R) with A [M,K], W [N,K] (and optionally R) in the split-f16 format; C is written
 * as f32, or as split-f16 pairs when c_is_split (N % 8 == 0) */
int sola_gemm_nt_split(const float* dev_a_sp, int lda, const float* dev_w_sp, const float* dev_bias, const float* dev_r,
                       int ldr, int r_is_split, float* dev_c, int ldc, int c_is_split, int M, int N, int K, float out_scale,
                       void* stream);
/* ... with a further result multiplier read from device memory (NULL = none) */
int sola_gemm_nt_split_scaled(const float* dev_a_sp, int lda, const float* dev_w_sp, const float* dev_bias, const float* dev_r,
                              int ldr, int r_is_split, float* dev_c, int ldc, int c_is_split, int M, int N, int K,
                              float out_scale, const float* dev_out_scale, void* stream);
/* Channels-last 1-d conv on split-f16 operands, exposed for the parity tests: x_sp [R * T_in][cin], w_sp [cout][k * cin] (both
 * from sola_cast_sp16, cin % 32 == 0), f32 y [R * T_out][cout] = conv + bias.  mode 0: one implicit-im2col GEMM (the taps in the
 * zero padding are multiplied); mode 1: one plain GEMM per output frame on the taps inside the sequence (at most five output
 * frames; an error where the conv has no such form); mode -1: what the split-f16 forward would take for this shape.  Both forms
 * give the same bits for finite weights.  The call synchronises the stream in modes 1 / -1. */
int sola_conv1d_cl_split(const float* dev_x_sp, const float* dev_w_sp, const float* dev_bias, float* dev_y, int64_t R, int T_in, int cin,
                         int cout, int k, int stride, int pad, int mode, void* stream);
/* The split-f16 standardised conv weights the context holds after a split-f16 forward, for the tests: encoder conv `layer` (0..5),
 * its whole [cout][k * cin] matrix (range -1) or the packed copy of tap range `range` (0 .. *n_ranges - 1: taps *lo .. *hi, a
 * [cout][(*hi - *lo + 1) * cin] matrix), copied to dev_out (NULL = only the numbers). */
int sola_conv_weights_split(const SolaCtx* ctx, int layer, int range, float* dev_out, int* lo, int* hi, int* n_ranges, void* stream);

/* Building blocks of precision 2 (16-bit activation storage), exposed for the parity tests: f32 rows -> _Float16 rows (fixed
 * power-of-two scale, or data-dependent with dev_scal as for sola_cast_sp16_auto); C = out_scale * (A W^T) + bias (+ R) on
 * _Float16 A [M,K] / W [N,K] / R with f32 accumulation, C written as _Float16 or f32 (K %% 64 == 0, lda %% 16 == 0; pitches in
 * elements); softmax(q k^T scale) v on _Float16 q / k / v / o with the addressing of sola_attention. */
int sola_cast_f16(const float* dev_in, int ld_in, void* dev_out, int ld_out, int64_t rows, int K, float scale, float* dev_scal, void* stream);
int sola_gemm_nt_f16(const void* dev_a_h, int lda, const void* dev_w_h, const float* dev_bias, const void* dev_r_h, int ldr,
                     void* dev_c, int ldc, int c_is_f16, int M, int N, int K, float out_scale, void* stream);
int sola_attention_f16(const void* dev_q, int ldq, const void* dev_k, int ldk, const void* dev_v, int ldv, void* dev_o, int ldo,
                       int G, int H, int head_dim, int Sq, int Sk, int inner, int64_t q_outer, int64_t q_inner, int64_t q_row_stride,
                       int64_t k_outer, int64_t k_inner, int64_t k_row_stride, float scale, void* stream);

/* Building blocks of the bf16 training step's 16-bit storage (precision 3, round 6), exposed for the parity tests.  BFLOAT16 matrices are
 * rows of 2-byte values, pitches in values.
 *   sola_gemm_nt_bf16: C = A W^T + bias (+ R) on bfloat16 A [M,K] / W [N,K], f32 accumulation; C and R f32 or (c_is_bf16 / r_is_bf16) bfloat16.
 *   sola_attention_bf16: softmax(q k^T scale) v on bfloat16 q / k / v (sola_attention's addressing, more than 16 queries or keys); the
 *     output as f32 rows (dev_o) and / or bfloat16 rows (dev_o_bf16), the log-sum-exp optional.
 *   sola_attention_backward_bf16: sola_attention_backward_ws on bfloat16 q / k / v with the gradients written as bfloat16 rows; dev_dq_scratch
 *     = an f32 [q rows, ld_dq] matrix (units of more keys than one key group accumulate dQ there).  One-pass kernel shapes and sequences
 *     of <= 4 steps.  dev_dout: f32 rows, or (dout_is_bf16, with the bf16 products on: sola_tune "attn_bwd_bf16_mfma") bfloat16 rows of pitch ldo;
 *     dev_o likewise (o_is_bf16, only together with dout_is_bf16). */
int sola_gemm_nt_bf16(const void* dev_a, int lda, const void* dev_w, const float* dev_bias, const void* dev_r, int ldr, int r_is_bf16,
                      void* dev_c, int ldc, int c_is_bf16, int M, int N, int K, void* stream);
int sola_attention_bf16(const void* dev_q, int ldq, const void* dev_k, int ldk, const void* dev_v, int ldv, float* dev_o, void* dev_o_bf16, int ldo,
                        int G, int H, int head_dim, int Sq, int Sk, int inner, int64_t q_outer, int64_t q_inner, int64_t q_row_stride,
                        int64_t k_outer, int64_t k_inner, int64_t k_row_stride, float scale, float* dev_lse, void* stream);
int sola_attention_backward_bf16(const void* dev_q, int ldq, const void* dev_k, int ldk, const void* dev_v, int ldv, const void* dev_o, int o_is_bf16,
                                 const void* dev_dout, int dout_is_bf16, int ldo, const float* dev_lse, void* dev_dq_bf16, void* dev_dk_bf16, void* dev_dv_bf16,
                                 int ld_dq, int ld_dk, int ld_dv, float* dev_dq_scratch, float* dev_dvec, int G, int H, int head_dim, int Sq, int Sk,
                                 int inner, int64_t q_outer, int64_t q_inner, int64_t q_row_stride, int64_t k_outer, int64_t k_inner,
                                 int64_t k_row_stride, float scale, int64_t q_rows, float* dev_scratch, size_t scratch_floats, void* stream);

/* ---- forward: replaces LanguageAlignedTrackSelectionModule.forward (module/module.py:130-162) ------------------ */
size_t sola_workspace_bytes(const SolaCtx* ctx, int B, int N, int T, int L);
int sola_forward(SolaCtx* ctx,
                 const float* dev_object_tokens, /* [B,N,T,object_token_dim] */
                 const float* dev_lang_tokens,   /* [B,L,lang_token_dim]     */
                 int B, int N, int T, int L,
                 float* dev_score_map,           /* [B,N]                    */
                 float* dev_score_tokens,        /* [B,N,lang_token_dim]     */
                 void* dev_workspace, size_t workspace_bytes, void* stream);

/* ---- ragged batches: many (video, expression) samples of different shapes in one pass ---------------------------------
 * The reference scores ONE sample per call (configs/mevis/default.yaml:37,42,47 batch_size 1; inference.py:44-58,
 * evaluator.py:88-112) with per-sample N tracks, T frames, L text tokens.  sola_forward_ragged takes the token rows of all
 * samples concatenated - no padding: no GroupNorm statistic or softmax sees a token that is not the sample's own - and
 * separates the VIDEOS (object sets) from the SAMPLES that refer to them: everything that does not depend on the text (the
 * motion encoder and layer 0's inter-object and motion sub-blocks, 57 % of a sample's FLOPs at the headline shape) is
 * computed once per video and shared by all its expressions, which inference.py:44-58 recomputes per expression.
 *   dev_object_tokens [sum_v N_v*T_v, object_token_dim]   video-major, then track, then frame (= [N_v,T_v,d] blocks)
 *   dev_lang_tokens   [sum_i L_i, lang_token_dim]          sample-major
 *   dev_score_map     [sum_i N_v(i)]                       sample-major, then track
 *   dev_score_tokens  [sum_i N_v(i), lang_token_dim]
 * All descriptor arrays are HOST arrays, read before the call returns.  n_samples == n_videos with sample_video[i] == i is
 * the plain ragged batch.  Results equal per-sample sola_forward calls up to f32 summation order. */
typedef struct SolaRaggedBatch {
    int32_t n_videos;
    const int32_t* video_tracks;     /* [n_videos]  N_v >= 1 */
    const int32_t* video_frames;     /* [n_videos]  T_v >= 1 */
    int32_t n_samples;
    const int32_t* sample_video;     /* [n_samples] index of the sample's video */
    const int32_t* sample_text_len;  /* [n_samples] L_i >= 1 */
} SolaRaggedBatch;
size_t sola_ragged_workspace_bytes(const SolaCtx* ctx, const SolaRaggedBatch* batch);
int sola_forward_ragged(SolaCtx* ctx, const float* dev_object_tokens, const float* dev_lang_tokens, const SolaRaggedBatch* batch,
                        float* dev_score_map, float* dev_score_tokens, void* dev_workspace, size_t workspace_bytes, void* stream);
/* sola_loss for a ragged batch: sample b owns the tracks dev_track_offsets[b] .. dev_track_offsets[b+1] (DEVICE int32,
 * n_samples + 1 entries) of the concatenated score_map / score_tokens / labels; dev_pos_tokens is [n_samples, D].  Every
 * sample gets its own means - what train.py:98-113 / evaluator.py compute at the reference's batch size of 1 - in
 * dev_loss3 [n_samples, 3] = {total, bce, alignment}.  Scratch: 3 * total_tracks floats. */
int sola_loss_ragged(const float* dev_score_map, const float* dev_score_tokens, const float* dev_labels,
                     const float* dev_pos_tokens, const float* dev_neg_tokens, int64_t neg_batch_stride, int n_samples,
                     const int32_t* dev_track_offsets, int max_tracks, int64_t total_tracks, int D, int n_neg,
                     float positive_weight, float temperature, float alignment_weight, float* dev_loss3,
                     int32_t* dev_neg_argmax, void* dev_scratch, size_t scratch_bytes, void* stream);

/* Location of a named intermediate of the LAST forward inside the workspace (parity tests / debugging).
 * Names: conv0..conv5 (pre-norm encoder conv outputs [B*N*T_l, C_l]), pe [T',D], lang [B*W,D],
 * l<i>_obj, l<i>_motion, l<i>_o2l (post-GroupNorm activations [B*N*T', D]). */
int sola_workspace_tap(const SolaCtx* ctx, const char* name, size_t* byte_offset, int64_t* rows, int64_t* cols);

/* ---- losses: replaces train.py:98-113 (weighted BCE + AlignmentLoss.forward, tools/loss.py:14-58) --------------
 * dev_neg_tokens is [B,n_neg,D] with neg_batch_stride = n_neg*D, or one [n_neg,D] table shared by every sample with
 * neg_batch_stride = 0 (train.py:92 repeats negative_token.weight over the batch).
 * dev_loss3 receives {total, bce, alignment}; dev_neg_argmax (optional, int32 [B,N]) the hardest-negative index.
 * Scratch: 3*B*N floats. */
int sola_loss(const float* dev_score_map, const float* dev_score_tokens,
              const float* dev_labels,     /* [B,N] {0,1} */
              const float* dev_pos_tokens, /* [B,1,D]     */
              const float* dev_neg_tokens, int64_t neg_batch_stride,
              int B, int N, int D, int n_neg,
              float positive_weight, float temperature, float alignment_weight,
              float* dev_loss3, int32_t* dev_neg_argmax,
              void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- selection: replaces inference.py:59-60 (sigmoid, strict > threshold) ------------------------------------- */
int sola_select(const float* dev_score_map, int64_t n, float threshold, float* dev_prob, float* dev_pred, void* stream);

/* ---- per-stage entry points (each is one kernel family; used by the parity tests and by sola_forward) ---------- */
/* module/ws.py:9-13: w [cout,cin,k] -> standardised, re-laid-out [cout, k*cin] (k-major) */
int sola_ws_standardize(const float* dev_w, int cout, int cin, int k, float* dev_out, void* stream);
/* C[M,N] = A[M,K] * W[N,K]^T + bias[N] (+ R[M,N]); F.linear (tools/attention.py:63-65,73). K % 4 == 0. */
int sola_gemm_nt(const float* dev_a, int lda, const float* dev_w, const float* dev_bias, const float* dev_r, int ldr,
                 float* dev_c, int ldc, int M, int N, int K, void* stream);
/* C[M,N] = A[M,K] * Wcat[K,N] (+ R[M,N]), Wcat = up to three row-major matrices of w_rows rows each stacked along K (dev_w1 / dev_w2 NULL
 * when K == w_rows / 2 w_rows): the input gradient of F.linear - dX = dY W, d[x] = [dq|dk|dv] [Wq;Wk;Wv] (tools/attention.py:63-65 backward)
 * - with the weights read where they lie, no transposed copy.  The few-row exact-f32 shape only (one sample per optimizer step,
 * train.py:116-125): M <= 2048, N % 32 == 0, K % 128 == 0, w_rows % 32 == 0, 16-byte aligned rows; SOLA_ERR_ARG otherwise.  Bit-identical
 * to sola_gemm_nt on the transposed copy. */
int sola_gemm_nn(const float* dev_a, int lda, const float* dev_w0, const float* dev_w1, const float* dev_w2, int w_rows, const float* dev_r,
                 int ldr, float* dev_c, int ldc, int M, int N, int K, void* stream);
/* channels-last conv1d along T (module/ws.py:14-22): x [R,T_in,cin], w_std [cout,k*cin] -> y [R,T_out,cout] */
int sola_conv1d_cl(const float* dev_x, const float* dev_wstd, const float* dev_bias, float* dev_y,
                   int R, int T_in, int cin, int cout, int k, int stride, int pad, void* stream);
/* GroupNorm over token sets (nn.GroupNorm; module/module.py:76,34,43,49): for instance i the tokens are rows
 * (i / inner) * outer_stride + (i % inner) * inner_stride + j * tok_stride, j < ntok, of an [*, C] matrix.
 * y = gn(x) (optionally LeakyReLU(slope)); if dev_pe != NULL also y2 = y + pe[(i % inner)] (module.py:38). */
int sola_group_norm(const float* dev_x, float* dev_y, float* dev_y2, const float* dev_pe,
                    const float* dev_gamma, const float* dev_beta,
                    int n_inst, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tok_stride,
                    int ntok, int C, int groups, float eps, float leaky_slope, int apply_leaky, void* stream);
/* softmax(q k^T * scale) v for G groups x H heads (tools/attention.py:66-72).  Row r of group g lives at matrix row
 * (g / inner) * outer + (g % inner) * inner_stride + r * row_stride (q and o share addressing; k and v share). */
int sola_attention(const float* dev_q, int ldq, const float* dev_k, int ldk, const float* dev_v, int ldv,
                   float* dev_o, int ldo, int G, int H, int head_dim, int Sq, int Sk, int inner,
                   int64_t q_outer, int64_t q_inner, int64_t q_row_stride,
                   int64_t k_outer, int64_t k_inner, int64_t k_row_stride, float scale,
                   float* dev_lse /* optional [q rows, H]: log-sum-exp, needed by the backward */, void* stream);
/* module/module.py:112-128: pe [t_len, D] */
int sola_pos_encoding(const float* dev_gauss, int D, int t_len, int max_temporal_length, float* dev_pe, void* stream);

/* ---- training: what loss.backward() does to this path under autograd (train.py:116-117) ----------------------------
 * sola_forward_train = sola_forward that keeps every attention's q/k/v/output/residual and the softmax log-sum-exp in
 * the workspace (sola_train_workspace_bytes); the workspace and dev_object_tokens must stay untouched until
 * sola_backward has run.  sola_backward consumes d(score_map), d(score_tokens) and OVERWRITES the gradient buffer
 * registered with sola_set_grad for each of the 83 parameters (same names and sizes as sola_set_weight; the Fourier
 * buffer has no gradient).  Gradients flowing into negative_token.weight through the loss's neg_tokens argument come
 * from sola_loss_backward (d_neg) and are added by the caller, exactly as autograd does for train.py:92. */
/* Dropout of the NEXT sola_forward_train (and of the sola_backward that follows it): p_encoder after every encoder
 * LeakyReLU (nn.Dropout(p=dropout_p), module/module.py:78-94), p_attention on the attention probabilities
 * (tools/attention.py:12,71, hard-coded 0.1 in the reference).  Masks are a pure function of (seed, element index), so
 * nothing is stored; a given seed reproduces the same masks.  p = 0 disables (eval-mode numerics). */
int sola_set_dropout(SolaCtx* ctx, float p_encoder, float p_attention, uint64_t seed);
/* The same mask generator for the per-stage entry points sola_group_norm[_backward] / sola_attention[_backward]
 * (thread-local; used by the parity tests). */
int sola_set_stage_dropout(float p, uint64_t seed);
size_t sola_train_workspace_bytes(const SolaCtx* ctx, int B, int N, int T, int L);
size_t sola_backward_workspace_bytes(const SolaCtx* ctx, int B, int N, int T, int L);
int sola_set_grad(SolaCtx* ctx, const char* name, void* dev_ptr, int64_t numel);
int sola_forward_train(SolaCtx* ctx, const float* dev_object_tokens, const float* dev_lang_tokens,
                       int B, int N, int T, int L, float* dev_score_map, float* dev_score_tokens,
                       void* dev_workspace, size_t workspace_bytes, void* stream);
int sola_backward(SolaCtx* ctx, const float* dev_d_score_map, const float* dev_d_score_tokens,
                  const void* dev_forward_workspace, void* dev_scratch, size_t scratch_bytes, void* stream);
/* ---- one optimizer step's device work in ONE call (round 5) ----------------------------------------------------------------------
 * The body of the reference's training loop - forward, weighted BCE + alignment loss, loss.backward(), get_grad_norm_dict(), gradient
 * clipping (train.py:62-125 at its batch size of one sample, configs/mevis/default.yaml:37) - enqueued from C++ on `stream`: the ~110
 * launches of a one-sample step cost 1.6-2.4 ms of host time when driven call by call from Python, more than their GPU time.
 * Same kernels, arguments and order as sola_forward_train + sola_loss + sola_loss_backward + sola_backward + sola_grad_sqnorms +
 * sola_grad_clip called one by one (bit-identical gradients).  The optimizer update is the caller's: the gradients are where
 * sola_set_grad bound them.
 *   sola_train_step_bind: the parameters in the order module/module.py:164-199 walks them (names[i] of group group[i]: encoder, every
 *     layer, negative tokens) - the gradient-norm reduction takes them in that order.  Call once per context (after sola_set_grad).
 *   dev_loss3 [3] = {total, bce, alignment} (train.py:98-113); dev_grad_sq [n_groups + 1] doubles = the groups' sums of squares of the
 *     UNclipped gradients and their total (module/module.py:164-199 reports the square roots); max_grad_norm <= 0: no clipping.
 *   dev_labels [B, N], dev_pos_tokens [B, 1, D]; the negative tokens are the context's own `negative_token.weight` (train.py:92), whose
 *     gradient receives both of its contributions (through the network and straight from the alignment loss).
 *   Workspaces (caller-owned): sola_train_workspace_bytes / sola_backward_workspace_bytes / sola_train_step_workspace_bytes. */
int sola_train_step_bind(SolaCtx* ctx, const char* const* names, const int32_t* group, int n, int n_groups);
size_t sola_train_step_workspace_bytes(const SolaCtx* ctx, int B, int N);
int sola_train_step(SolaCtx* ctx, const float* dev_object_tokens, const float* dev_lang_tokens, int B, int N, int T, int L,
                    const float* dev_labels, const float* dev_pos_tokens, float positive_weight, float temperature, float alignment_weight,
                    float max_grad_norm, float* dev_score_map, float* dev_score_tokens, float* dev_loss3, double* dev_grad_sq,
                    void* dev_train_workspace, size_t train_workspace_bytes, void* dev_backward_scratch, size_t backward_scratch_bytes,
                    void* dev_step_workspace, size_t step_workspace_bytes, void* stream);
/* Gradient clipping + the AdamW update (train.py:121-125) in ONE multi-tensor launch, with torch.optim.AdamW(fused=True)'s own arithmetic
 * (ATen/native/cuda/fused_adam_utils.cuh: double scalars, float tensors, the same expressions): bit-identical parameters and moments.
 *   sola_adamw_bind: the optimizer's state tensors per parameter name (exp_avg, exp_avg_sq as float arrays of the parameter's size; step =
 *     torch's per-parameter device float counter, or null).  Parameters and gradients are the context's own bindings
 *     (sola_set_weight / sola_set_grad): the update writes the caller's parameter storage.  Bind again when a pointer changes: a
 *     sola_set_weight / sola_set_grad with a NEW pointer unbinds the optimizer and sola_adamw_step fails until the next bind.
 *   sola_adamw_step: `step` = 0: this update's number is read from the bound step tensors ON THE DEVICE (counter + 1) and the kernel
 *     advances them, exactly as torch's own step() does - the two may be mixed on one optimizer, and a load_state_dict into the same
 *     storage is picked up (needs step tensors); `step` >= 1: an explicit number (1, 2, ...).  max_grad_norm > 0 scales every gradient by min(1, max_norm / (sqrt(*dev_total_sq)
 *     + 1e-6)) first (torch.nn.utils.clip_grad_norm_), decided on the device; write_back_grads != 0 leaves the scaled gradients in the
 *     gradient tensors as clip_grad_norm_ does, 0 leaves them unclipped (an eighth less traffic; train.py:121-125 never reads them again). */
int sola_adamw_bind(SolaCtx* ctx, const char* const* names, void* const* dev_exp_avg, void* const* dev_exp_avg_sq, void* const* dev_step, int n);
int sola_adamw_step(SolaCtx* ctx, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, const double* dev_total_sq,
                    float max_grad_norm, int write_back_grads, void* stream);
/* ---- ragged training step: many (video, expression) samples of DIFFERENT shapes per optimizer step -------------------------
 * The reference trains at batch size 1 (configs/mevis/default.yaml:37; train.py:62-137: one forward, one backward, one AdamW
 * step per sample) because every sample has its own N tracks, T frames and L text tokens (dataloader.py:119-163,187-199).
 * sola_forward_train_ragged / sola_backward_ragged run the same step over a SolaRaggedBatch: token rows concatenated without
 * padding (layouts as sola_forward_ragged), every GEMM of the forward and backward over all rows at once, every shape-dependent
 * kernel (conv windows and their transposes, GroupNorm and its backward, the three attentions and their backward, score head)
 * reading per-unit tables built on the device.  One sample per video, in order (n_samples == n_videos, sample_video[i] == i):
 * under training-mode dropout each sample has its own masks, so nothing is shared between the expressions of a video.
 * The parameter gradients sola_backward_ragged leaves are the SUM over the samples of what one-sample calls produce for the
 * same upstream d(score_map) / d(score_tokens) (weighting per sample is the caller's, through those: sola_loss_backward_ragged
 * takes one upstream triple per sample).  The workspace holds the unit tables: hand the SAME workspace to sola_backward_ragged. */
size_t sola_train_ragged_workspace_bytes(const SolaCtx* ctx, const SolaRaggedBatch* batch);
size_t sola_backward_ragged_workspace_bytes(const SolaCtx* ctx, const SolaRaggedBatch* batch);
int sola_forward_train_ragged(SolaCtx* ctx, const float* dev_object_tokens, const float* dev_lang_tokens, const SolaRaggedBatch* batch,
                              float* dev_score_map, float* dev_score_tokens, void* dev_workspace, size_t workspace_bytes, void* stream);
int sola_backward_ragged(SolaCtx* ctx, const float* dev_d_score_map, const float* dev_d_score_tokens,
                         const void* dev_forward_workspace, void* dev_scratch, size_t scratch_bytes, void* stream);
/* Backward of sola_loss_ragged: dev_g3 [n_samples, 3] = upstream gradients of every sample's {total, bce, alignment} (the mean
 * of the per-sample totals - train.py:113 averaged over the batch - is g3[b] = {1/n_samples, 0, 0}).  Outputs as
 * sola_loss_backward over the concatenated tracks; d_neg [n_samples, n_neg, D], or [n_neg, D] summed over the samples when
 * neg_batch_stride == 0.  Scratch: total_tracks*n_neg floats (+ n_samples*n_neg*D for shared negatives). */
int sola_loss_backward_ragged(const float* dev_score_map, const float* dev_score_tokens, const float* dev_labels,
                              const float* dev_pos_tokens, const float* dev_neg_tokens, int64_t neg_batch_stride, int n_samples,
                              const int32_t* dev_track_offsets, int max_tracks, int64_t total_tracks, int D, int n_neg,
                              float positive_weight, float temperature, float alignment_weight, const float* dev_g3,
                              float* dev_d_score_map, float* dev_d_score_tokens, float* dev_d_neg, void* dev_scratch,
                              size_t scratch_bytes, void* stream);
/* Gradient buckets for multi-GPU training (train.py under torchrun: one RCCL all-reduce of the gradient per step, the only
 * collective of the path).  sola_backward finishes the parameters' gradients in a fixed order: alignment layer n-1, ...,
 * layer 1, then layer 0 together with negative_token.weight (which collects contributions from every layer), then the
 * encoder - sola_grad_bucket_count() = n_layers + 1 buckets, sola_grad_bucket_of(name) gives a parameter's bucket.  A caller
 * that lays its gradient buffers out bucket by bucket in ONE flat allocation can all-reduce each bucket in place, and
 * sola_backward_wait_bucket(ctx, k, stream) makes `stream` wait (device-side, hipStreamWaitEvent) for the moment bucket k
 * is final, so its all-reduce overlaps the rest of the backward.  Valid after sola_backward until the next one. */
int sola_grad_bucket_count(const SolaCtx* ctx);
int sola_grad_bucket_of(const SolaCtx* ctx, const char* name);
int sola_backward_wait_bucket(SolaCtx* ctx, int bucket, void* stream);
/* Backward of sola_loss.  dev_g3 = upstream gradients of {total, bce, alignment} (3 floats on the device).
 * Writes d(score_map) [B,N], d(score_tokens) [B,N,D] and (optional) d(neg_tokens) [B,n_neg,D].  Scratch: B*N*n_neg floats. */
int sola_loss_backward(const float* dev_score_map, const float* dev_score_tokens, const float* dev_labels,
                       const float* dev_pos_tokens, const float* dev_neg_tokens, int64_t neg_batch_stride,
                       int B, int N, int D, int n_neg, float positive_weight, float temperature, float alignment_weight,
                       const float* dev_g3, float* dev_d_score_map, float* dev_d_score_tokens, float* dev_d_neg,
                       void* dev_scratch, size_t scratch_bytes, void* stream);
/* Gradient statistics of the training step.  sola_grad_sqnorms: out[g] = sum over the tensors of group g of |grad|^2
 * for g < n_groups and out[n_groups] = their total (dev_out holds n_groups + 1 doubles)
 * (replaces get_grad_norm_dict, module/module.py:164-199, which syncs the host once per parameter); the pointer /
 * numel / group arrays are HOST arrays of n <= 128 entries.  sola_grad_clip scales every tensor in place by
 * min(1, max_norm / (sqrt(*dev_total_sq) + 1e-6)) (torch.nn.utils.clip_grad_norm_, train.py:121-122) without a host sync. */
size_t sola_grad_sqnorms_scratch_bytes(int n, const int64_t* numel);
int sola_grad_sqnorms(const float* const* dev_grads, const int64_t* numel, const int32_t* group, int n, int n_groups,
                      double* dev_out, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_grad_clip(float* const* dev_grads, const int64_t* numel, int n, const double* dev_total_sq, float max_norm,
                   void* stream);
/* per-stage backward entry points (parity tests) */
int sola_ws_backward(const float* dev_w, const float* dev_dwstd, int cout, int cin, int k, float* dev_dw, void* stream);
/* The same attention with q, k, v given as split-f16 rows: every product runs as three v_mfma_f32_16x16x16_f16 with f32
 * accumulation instead of the exact-f32 MFMA (the inference fast path; sequences longer than 16 steps only). */
int sola_attention_split(const float* dev_q_sp, int ldq, const float* dev_k_sp, int ldk, const float* dev_v_sp, int ldv,
                         float* dev_o, int ldo, int o_is_split, int G, int H, int head_dim, int Sq, int Sk, int inner,
                         int64_t q_outer, int64_t q_inner, int64_t q_row_stride,
                         int64_t k_outer, int64_t k_inner, int64_t k_row_stride, float scale, float* dev_lse, void* stream);
/* C[N,K] = A[M,N]^T * B[M,K] (weight gradient), optional bias_grad[N] = column sums of A */
size_t sola_gemm_tn_scratch_bytes(int M, int N, int K);
int sola_gemm_tn(const float* dev_a, int lda, const float* dev_b, int ldb, float* dev_c, float* dev_bias_grad,
                 int M, int N, int K, void* dev_scratch, size_t scratch_bytes, void* stream);
/* The same weight gradient on the split-f16 MFMA path (training precision 1): both operands are written transposed in
 * the split-f16 format (dY with a power-of-two scale found on the device), the product is the NT split GEMM with the
 * reduction cut into ranges, partial sums folded in a fixed order.  N % 8 == 0, K % 8 == 0, M >= 64. */
size_t sola_gemm_tn_split_scratch_bytes(int M, int N, int K);
int sola_gemm_tn_split(const float* dev_a, int lda, const float* dev_b, int ldb, float* dev_c, int M, int N, int K,
                       void* dev_scratch, size_t scratch_bytes, void* stream);
/* The same weight gradient on plain 16-bit operands (fmt 1 = f16, 2 = bfloat16: training with 16-bit GEMM operands, and the dW
 * products of the default split-f16 step), ONE MFMA per product.  With N % 256 == 0 and K % 256 == 0 no transposed copy is made: the
 * operands are cast row-major and the kernel transposes between LDS and the matrix pipe (ds_read_b64_tr_b16; sola_tune "train_tn_tr"
 * 0 = the transposed-copy route for every shape).  Scratch as for sola_gemm_tn_split. */
int sola_gemm_tn_f16(const float* dev_a, int lda, const float* dev_b, int ldb, float* dev_c, int M, int N, int K, int fmt,
                     void* dev_scratch, size_t scratch_bytes, void* stream);
/* dW_std[cout][k*cin] of the channels-last conv (module/ws.py:14-22) on 16-bit operands: dy [R*T_out][cout], x [R*T_in][cin].  With
 * cout % 256 == 0 and cin % 256 == 0 the conv input is cast ONCE, row-major, and the kernel gathers the taps (implicit im2col) in its
 * LDS-DMA addresses; else one transposing cast per tap.  Scratch: sola_gemm_tn_split_scratch_bytes(R*T_out, cout, k*cin). */
int sola_conv1d_cl_wgrad_f16(const float* dev_x, const float* dev_dy, float* dev_dwstd, int R, int T_in, int cin, int cout, int k,
                             int stride, int pad, int fmt, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_conv1d_cl_backward(const float* dev_x, const float* dev_wstd, const float* dev_dy, float* dev_dx,
                            float* dev_dwstd, float* dev_dbias, int R, int T_in, int cin, int cout, int k, int stride,
                            int pad, void* dev_scratch, size_t scratch_bytes, void* stream);
/* ... on the split-f16 MFMA path (what sola_backward runs under precision 1); cout % 128 == 0, cin % 8 == 0, R*T_out >= 64 */
size_t sola_conv1d_cl_backward_split_scratch_bytes(int R, int T_in, int cin, int cout, int k, int stride, int pad);
int sola_conv1d_cl_backward_split(const float* dev_x, const float* dev_wstd, const float* dev_dy, float* dev_dx,
                                  float* dev_dwstd, float* dev_dbias, int R, int T_in, int cin, int cout, int k, int stride,
                                  int pad, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_group_norm_backward(const float* dev_x, const float* dev_dy, const float* dev_dy2, const float* dev_gamma,
                             const float* dev_beta, float* dev_dx, float* dev_dgamma, float* dev_dbeta,
                             int n_inst, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tok_stride,
                             int ntok, int C, int groups, float eps, float leaky_slope, int apply_leaky,
                             void* dev_scratch, size_t scratch_bytes, void* stream);
/* GroupNorm with every field of its descriptors (tests).  Formats are the codes of sola_set_precision's operand formats (0 f32, 1 split-f16
 * pairs, 2 f16, 3 bfloat16); 16-bit rows have the pitch C counted in their own elements.
 *   sola_group_norm_ex: sola_group_norm on in_fmt rows (0, 2, 3) writing out_fmt rows (0, 1, 2).  dev_units (NULL or n_inst int32 quadruples:
 *     first row, row stride, token count, pe row) replaces the strided pattern, ntok is then the largest count.  dev_in_scale: optional device
 *     scalar multiplied into x.  dev_guard: range guard word of 16-bit outputs (set to 1 by a value of 65000 or more; never cleared).
 *     dev_y_cast / dev_y2_cast: beside f32 outputs, the same values as cast_fmt (2, 3) rows.  dev_slice_ws: 8 bytes per (instance, group, slice)
 *     for units beyond the register shapes (NULL: the library's own).  dev_stats_out: where that shape leaves (mean, rstd) per (instance,
 *     group); *stats_written (host) is set to 1 when it did.
 *   sola_group_norm_backward_ex: sola_group_norm_backward with dev_units, x as x_fmt rows (0, 3), dy2 as dy2_fmt rows (0, 3), dx once more
 *     as bfloat16 rows (dev_dx16) and the forward's statistics (dev_stats_in, read by the shape beyond the register shapes only).
 *   sola_group_norm_shape: the kernel shape of a unit of ntok tokens x cg channels under the present sola_tune switches; direction 0 forward,
 *     1 backward (which ignores the formats); out5 = (kind: 0 wave, 1 block, 2 sliced, 3 three-pass; token slots per lane; threads per block;
 *     channels per lane; slices per unit).  Host only: needs no device. */
int sola_group_norm_ex(const void* dev_x, void* dev_y, void* dev_y2, const float* dev_pe, const float* dev_gamma, const float* dev_beta,
                       int n_inst, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tok_stride, int ntok, int C, int groups,
                       float eps, float leaky_slope, int apply_leaky, int in_fmt, int out_fmt, const int32_t* dev_units,
                       const float* dev_in_scale, int* dev_guard, void* dev_y_cast, void* dev_y2_cast, int cast_fmt, void* dev_slice_ws,
                       size_t slice_ws_bytes, void* dev_stats_out, int* stats_written, void* stream);
int sola_group_norm_backward_ex(const void* dev_x, const float* dev_dy, const void* dev_dy2, const float* dev_gamma, const float* dev_beta,
                                float* dev_dx, float* dev_dgamma, float* dev_dbeta, int n_inst, int inner, int64_t outer_stride,
                                int64_t inner_stride, int64_t tok_stride, int ntok, int C, int groups, float eps, float leaky_slope,
                                int apply_leaky, const int32_t* dev_units, int x_fmt, int dy2_fmt, void* dev_dx16, const void* dev_stats_in,
                                void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_group_norm_shape(int direction, int ntok, int cg, int in_fmt, int out_fmt, int dropout, int out5[5]);
int sola_attention_backward(const float* dev_q, int ldq, const float* dev_k, int ldk, const float* dev_v, int ldv,
                            const float* dev_o, const float* dev_dout, int ldo, const float* dev_lse,
                            float* dev_dq, float* dev_dk, float* dev_dv, float* dev_dvec /* [q rows, H] scratch */,
                            int G, int H, int head_dim, int Sq, int Sk, int inner,
                            int64_t q_outer, int64_t q_inner, int64_t q_row_stride,
                            int64_t k_outer, int64_t k_inner, int64_t k_row_stride, float scale, void* stream);
/* ... with scratch for the one-pass kernel's long query ranges (round 3).  Units of at most 128 queries and 128 keys take the
 * one-pass kernel either way (one block per (unit, head): S / dP / dS formed once, q, k, v, o, dO read once; sola_tune
 * "attn_bwd_fused" 0 = the two-pass kernels).  Longer query ranges against <= 64 keys (object -> language) take it when
 * dev_scratch holds sola_attention_backward_scratch_floats(q rows, G, H, Sk) floats and the units' rows are consecutive
 * (inner == 1 and q_row_stride == 1): 256-query chunks, one block each, dK / dV partial sums added in chunk order. */
size_t sola_attention_backward_scratch_floats(int64_t q_rows, int G, int H, int Sk);
int sola_attention_backward_ws(const float* dev_q, int ldq, const float* dev_k, int ldk, const float* dev_v, int ldv,
                               const float* dev_o, const float* dev_dout, int ldo, const float* dev_lse,
                               float* dev_dq, float* dev_dk, float* dev_dv, float* dev_dvec, int G, int H, int head_dim, int Sq, int Sk,
                               int inner, int64_t q_outer, int64_t q_inner, int64_t q_row_stride, int64_t k_outer, int64_t k_inner,
                               int64_t k_row_stride, float scale, int64_t q_rows, float* dev_scratch, size_t scratch_floats, void* stream);

/* ---- mask IoU: replaces track_generation/seg_utils.py:128-142 (compute_mask_iou), :109-125 (compute_masklet_iou)
 * and the prompt-mask nearest resize of generate_tokens_grid.py:269-272 ------------------------------------------
 * Masks are packed to 1 bit/pixel (words of 32 pixels, row-major over the H*W comparison grid).
 * elem_type: 0 = uint8, 1 = float32; a pixel is set when its value != 0.  If (h,w) != (H,W) the source is
 * resampled with ATen's nearest rule while packing.  dev_area receives the per-mask popcount (int64). */
int64_t sola_mask_words(int H, int W);
int sola_mask_pack(const void* dev_masks, int elem_type, int n, int h, int w, int H, int W,
                   uint32_t* dev_bits, int64_t* dev_area, void* stream);
/* inter[p,r] = popcount(A[a_index(p,r)] & B[r]), union = area_A + area_B - inter.
 * dev_a_frame (optional, int32 [R]): A holds P masklets of T frames (A index = p*T + frame[r]), which is the
 * "pred masklet at the prompt's frame" gather of generate_tokens_grid.py:269.  T=1, NULL = plain P x R matrix. */
int sola_mask_pair_counts(const uint32_t* dev_a_bits, const int64_t* dev_a_area, int P, int T,
                          const uint32_t* dev_b_bits, const int64_t* dev_b_area, int R,
                          const int32_t* dev_a_frame, int64_t words,
                          int64_t* dev_inter, int64_t* dev_union, void* stream);
/* One call for the common case: A [P,H,W], B [R,h,w] -> inter/union [P,R] (scratch: (P+R)*(words*4+8) bytes). */
size_t sola_mask_iou_scratch_bytes(int P, int R, int H, int W);
int sola_mask_iou_matrix(const void* dev_a, const void* dev_b, int elem_type, int P, int R, int H, int W, int h, int w,
                         int64_t* dev_inter, int64_t* dev_union, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- masklet resampling / decoding on the same packed representation ----------------------
 * sola_mask_bilinear_pack replaces track_generation/seg_utils.py:145-160 (reshape_masklet): bilinear resample
 * (align_corners=False, ATen's source-index rule) of n {0,1} masks [n,h,w] to H x W, `> 0.5`, bit-pack, area.
 * elem_type 0 = uint8 (non-zero counts as 1.0), 1 = float32 (any values; the fp32 arithmetic order is ATen's),
 * 2 = float32 tracker logits, binarised as (v > 0) while reading — the `(out_mask_logits > 0.0).float()` of
 * generate_tokens_grid.py:215-222 folded in.  W <= 4096. */
int sola_mask_bilinear_pack(const void* dev_masks, int elem_type, int n, int h, int w, int H, int W,
                            uint32_t* dev_bits, int64_t* dev_area, void* stream);
/* packed bits -> {0,1} images [n,H,W] (elem_type 0 = uint8, 1 = float32): the tensor reshape_masklet returns. */
int sola_mask_unpack(const uint32_t* dev_bits, int n, int H, int W, void* dev_out, int elem_type, void* stream);
/* COCO run-length masks -> OR of K masks per frame, replaces dataloader.py:305-369 (rle_masklet_decode + np.logical_or
 * in get_sam2_masklet / get_gt_masklet).  Mask (frame f, slot k) owns the runs dev_off[f*K+k] .. dev_off[f*K+k+1] of
 * dev_cum, the inclusive prefix sums of its run lengths (uint32, column-major positions as in pycocotools); an empty
 * range is an absent / unselected mask.  dev_out [n_frames,h,w] uint8 row-major and/or dev_bits + dev_area. */
int sola_rle_fill_or(const uint32_t* dev_cum, const int64_t* dev_off, int n_frames, int K, int h, int w,
                     uint8_t* dev_out, uint32_t* dev_bits, int64_t* dev_area, void* stream);

/* Host-only helper: COCO compressed RLE string (pycocotools rleFrString format) -> inclusive prefix sums of its run
 * lengths in host_cum[0..cap).  Returns the number of runs, or a negative status (malformed string, more than cap runs,
 * or runs covering more than `limit` pixels; limit < 0 disables that check). */
int64_t sola_rle_string_to_cum(const char* str, int64_t len, uint32_t* host_cum, int64_t cap, int64_t limit);

/* ---- mask-level J&F (evaluator.py:174-247): decode once per video, count every (expression, frame) in one launch --------
 * Column-major bit planes, internal to this path (never mixed with the row-major planes of sola_mask_pack): bit j of word i
 * is the pixel at COCO position 32*i + j (position = x*h + y), a plane is words_stride = sola_jf_plane_words(h, w) words
 * (a multiple of 4: planes start on 16 bytes), tail and pad bits are zero.  Mask m at frame t is plane m*T + t.
 *   sola_rle_pack_cm: n_planes masks given as sola_rle_fill_or's dev_cum / dev_off (plane p owns runs dev_off[p] ..
 *     dev_off[p+1]; an empty range is an absent frame = all zeros) -> dev_bits [n_planes, words_stride] (16-byte aligned).
 *     Any n_planes.  Runs covering fewer than h*w pixels follow sola_rle_fill_or's rule (value = parity of the run ends at
 *     or before the position), so the two decoders agree everywhere.
 *   sola_mask_select_counts: for every expression e < E and frame t < T, p = OR of the planes of the masks
 *     dev_pred_idx[dev_pred_off[e] .. dev_pred_off[e+1]), g = the same over dev_gt_idx / dev_gt_off (int32 CSR lists of
 *     mask ids < n_masks; an empty list is an all-zero mask, ids may repeat and appear in both lists; ids outside
 *     [0, n_masks) are ignored) -> dev_counts [E, T, 3] int64 = (popc(p & g), popc(p), popc(g)), exact.
 *   sola_rle_strings_to_cum_batch (host only): n compressed strings back to back in `chars`, string i at
 *     chars[str_off[i] .. str_off[i+1]) -> host_cum (prefix sums, as sola_rle_string_to_cum, runs <= limit pixels each
 *     string) and run_off [n+1] int64 (string i owns host_cum[run_off[i] .. run_off[i+1])).  An empty string has no runs.
 *     Returns the total number of runs (<= cap) or a negative status naming the string. */
int64_t sola_jf_plane_words(int h, int w);
int sola_rle_pack_cm(const uint32_t* dev_cum, const int64_t* dev_off, int64_t n_planes, int h, int w, int64_t words_stride,
                     uint32_t* dev_bits, void* stream);
int sola_mask_select_counts(const uint32_t* dev_bits, int64_t words_stride, int n_masks, int T, const int32_t* dev_pred_off,
                            const int32_t* dev_pred_idx, const int32_t* dev_gt_off, const int32_t* dev_gt_idx, int E,
                            int64_t* dev_counts, void* stream);
int64_t sola_rle_strings_to_cum_batch(const char* chars, const int64_t* str_off, int64_t n, uint32_t* host_cum, int64_t cap,
                                      int64_t limit, int64_t* run_off);

/* ---- J&F at K nested selections (a sweep of the selection threshold) from one counting pass ------------------------------
 * Planes, stride, alignment and id rules of sola_mask_select_counts.  dev_pred_idx[dev_pred_off[e] .. dev_pred_off[e+1]) is
 * expression e's ORDERED candidate list, len_e long: the selection of level k is its prefix of end(e, k) entries, with
 * end(e, -1) = 0 and end(e, k) = min(max(dev_level_end[e*K + k], end(e, k-1)), len_e): a decreasing or too-long entry is
 * clamped and nothing is read out of range; entries behind end(e, K-1) are never read.  p_k = OR of the planes of that prefix,
 * g = OR of the GT list -> dev_counts [E, K, T, 3] int64 = (popc(p_k & g), popc(p_k), popc(g)), exact; dev_counts[e, k] is
 * the [T, 3] table sola_mask_select_counts gives for the prefix as a prediction list.  One block per (e, t) carries p over the
 * levels and ORs in only the planes that enter at each, so every plane of the largest selection and of the GT list is read
 * once per (e, t) and SOLA_NESTED_MAX_LEVELS levels; K above that bound costs ceil(K / 16) launches, each of which reads the
 * prefix of its first level again.  Every entry is written by exactly one thread (no atomics, no memset; the result does not
 * depend on any order).  K, E, T > 0, n_masks >= 0, E*T < 2^31, words_stride a positive multiple of 4 below 2^26, planes
 * 16-byte aligned, no null pointer.  Asynchronous on the stream. */
#define SOLA_NESTED_MAX_LEVELS 16
int sola_mask_nested_counts(const uint32_t* dev_bits, int64_t words_stride, int n_masks, int T, const int32_t* dev_pred_off,
                            const int32_t* dev_pred_idx, const int32_t* dev_level_end, int K, const int32_t* dev_gt_off,
                            const int32_t* dev_gt_idx, int E, int64_t* dev_counts, void* stream);

/* ---- DAVIS boundary (contour) F on the same planes and id lists (no void pixels, both masks of one size) ----------------
 * For every expression e < E and frame t < T, fg / gt = the ORs sola_mask_select_counts forms.  The boundary map B(m) is 1
 * where m differs from an in-image neighbour among east (y, x+1), south (y+1, x) and south-east (y+1, x+1); dil(B) is B
 * dilated by the disk dy*dy + dx*dx <= radius*radius, positions outside the image contributing nothing (radius 0 = B
 * itself; the benchmark's radius is ceil(0.008 * sqrt(h*h + w*w))).  dev_counts [E, T, 4] int64 =
 * (|B(fg)|, |B(gt)|, |B(fg) & dil(B(gt))|, |B(gt) & dil(B(fg))|), exact; every entry is written.  0 <= radius <= 64,
 * h*w < 2^31, words_stride a multiple of 4 and >= sola_jf_plane_words(h, w), planes 16-byte aligned, E*T < 2^31; a frame
 * too tall for one column strip of 2*radius + 2 columns to fit a CU's LDS is refused (at radius 18 that is h > 8512).
 * Asynchronous on the stream.  The workspace is sized by sola_boundary_counts_workspace_bytes, which answers 0 (the strips
 * of a frame meet in int64 atomics after a memset of dev_counts on the stream): workspace may be NULL. */
int sola_mask_select_boundary_counts(const uint32_t* dev_bits, int64_t words_stride, int n_masks, int T, int h, int w, int radius,
                                     const int32_t* dev_pred_off, const int32_t* dev_pred_idx, const int32_t* dev_gt_off,
                                     const int32_t* dev_gt_idx, int E, int64_t* dev_counts, void* workspace, size_t workspace_bytes,
                                     void* stream);
size_t sola_boundary_counts_workspace_bytes(int h, int w, int radius, int E, int T);

/* Masks -> COCO compressed RLE strings, byte-identical to pycocotools encode + rleToString on {0,1} masks; replaces the
 * host copy + per-frame pycocotools loop of track_generation/seg_utils.py encode_rle_masklet_torch.  n masks [n,h,w]
 * row-major; elem_type 0 = uint8 (!= 0), 1 = float32 (!= 0), 2 = float32 tracker logits (> 0).  n >= 1 (any n: launches
 * are chunked by 65535 frames), h*w < 2^31.  Three calls on one stream, each output sized by the previous one's result:
 *   1. sola_rle_encode_runs: dev_run_off [n+1] int64 = first run of each frame (dev_run_off[n] = total runs).  dev_scratch
 *      (>= sola_rle_encode_scratch_bytes(n,h,w) bytes, 4-byte aligned) keeps per-segment offsets for call 2.
 *   2. sola_rle_encode_cum: the same masks and the scratch as call 1 left it -> dev_cum [total runs] uint32 = each
 *      frame's inclusive prefix sums of its run lengths (column-major, what sola_rle_fill_or reads with dev_run_off as its
 *      offsets and K = 1), and dev_char_off [n+1] int64 = first character of each frame (dev_char_off[n] = total).
 *   3. sola_rle_encode_chars: dev_chars [total characters] = every frame's string back to back (no terminators).  Reads
 *      dev_cum / dev_run_off / dev_char_off only, so it also encodes prefix sums that did not come from call 2.
 * Scratch: n * w * ceil(h/64) * 4 bytes, rounded up to 256; 0 for bad sizes (host-only). */
size_t sola_rle_encode_scratch_bytes(int n, int h, int w);
int sola_rle_encode_runs(const void* dev_masks, int elem_type, int n, int h, int w, int64_t* dev_run_off,
                         void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_rle_encode_cum(const void* dev_masks, int elem_type, int n, int h, int w, const int64_t* dev_run_off,
                        uint32_t* dev_cum, int64_t* dev_char_off, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_rle_encode_chars(const uint32_t* dev_cum, const int64_t* dev_run_off, const int64_t* dev_char_off, int n,
                          char* dev_chars, void* stream);

/* Masks -> the zlib streams of 8-bit greyscale PNG files (pixel 255 where the mask is set, else 0), one per frame; replaces
 * the host copy of the masklet + one general PNG encode per frame in inference.py.  n masks [n,h,w] row-major, elem_type as
 * sola_rle_encode_runs (0 = uint8 != 0, 1 = float32 != 0, 2 = float32 logits > 0).  n >= 1 (any n: launches are chunked by
 * 65535 frames), h*(w+1) < 2^31.
 * Format, fixed: bytes 78 01, ONE DEFLATE block (BFINAL=1, BTYPE=01: the fixed Huffman table), Adler-32 (big endian) of
 * the raw stream.  Raw stream = per row one byte 0 (filter None) then w pixel bytes.  It is cut into maximal runs of equal
 * bytes across row ends; a run of value v and length r is the literal v, then L = r-1 bytes as distance-1 matches: while
 * L > 0: L == 258 or L >= 261 -> 258; L in {259, 260} -> L-3; 3 <= L <= 257 -> L; L in {1, 2} -> L literals.  Then
 * end-of-block and zero bits to the byte boundary.  A frame's stream is at most 6 + (9*h*(w+1) + 17) / 8 bytes.  The
 * caller adds the PNG signature, IHDR, the IDAT length and CRC-32 (which covers the compressed bytes only) and IEND.
 * Two calls on one stream with one host read between them:
 *   1. sola_png_deflate_sizes: reads the masks once; dev_byte_off [n+1] int64 = first byte of each frame's complete stream
 *      (dev_byte_off[n] = total bytes), dev_adler [n] uint32 = Adler-32 of each raw stream (exact 64-bit sums on the GPU,
 *      reduced mod 65521 at the end).  dev_scratch (>= sola_png_deflate_scratch_bytes(n,h,w) bytes, 8-byte aligned) keeps
 *      the raw streams as bitmaps and the per-workgroup bit offsets for call 2.
 *   2. sola_png_deflate_write: dev_bytes [dev_byte_off[n]] = every frame's stream back to back.  Takes the scratch as call
 *      1 left it, with the same n, h, w, and does not read the masks again.  EVERY byte of dev_bytes is written with
 *      plain stores (each byte has one owning workgroup): nothing depends on what the buffer held.  A scratch or offsets
 *      that do not belong together give missing bytes, never a store outside a frame's [dev_byte_off[i], dev_byte_off[i+1]).
 * Both are asynchronous on the stream.  Scratch: n * (ceil(h*(w+1)/64) * 8 + ceil(h*(w+1)/16384) * 28) bytes, rounded up to
 * 256; 0 for bad sizes (host-only).  Bad arguments are refused before any launch. */
size_t sola_png_deflate_scratch_bytes(int n, int h, int w);
int sola_png_deflate_sizes(const void* dev_masks, int elem_type, int n, int h, int w, int64_t* dev_byte_off,
                           uint32_t* dev_adler, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_png_deflate_write(const void* dev_masks, int elem_type, int n, int h, int w, const int64_t* dev_byte_off,
                           const uint32_t* dev_adler, uint8_t* dev_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- PNG streams of selections of bit planes: every threshold's files of a video from one decode -------------------------
 * sola_planes_cm_to_rm: the column-major planes of sola_rle_pack_cm / sola_index_pack (bit x*h + y, stride >=
 *   sola_jf_plane_words(h, w)) -> the flat row-major layout of sola_mask_pack (bit j of word i is pixel 32*i + j at position
 *   y*w + x), plane p at dev_bits_rm + p * words_stride_rm.  Both strides are multiples of 4 and words_stride_rm >=
 *   sola_mask_words(h, w); both buffers 16-byte aligned; h*w < 2^31; any n_planes >= 1.  EVERY word of every output plane is
 *   written by exactly one thread (no atomics, no memset), tail and pad bits zero.  A bit-matrix transpose through ballots and
 *   LDS: up to 64 image rows per workgroup, fewer when 64 rows of w bits exceed 48 KiB (w > 393 152 is refused).
 * sola_png_deflate_sizes_select: sola_png_deflate_sizes for n = E*K*T streams that are never materialised as masks.  Stream
 *   (e*K + k)*T + t is the PNG zlib stream (format above) of the OR of the row-major planes m*T + t over m in
 *   dev_sel_idx[dev_sel_off[e] .. dev_sel_off[e] + end(e, k)), with the CSR list and level rules of sola_mask_nested_counts:
 *   end(e, k) = min(max(dev_level_end[e*K + k], end(e, k-1)), len_e), a null dev_level_end (K == 1 only) = the whole list, ids
 *   outside [0, n_masks) are ignored, ids may repeat, an empty list is an all-zero frame.  1 <= K <= SOLA_NESTED_MAX_LEVELS
 *   (more levels: several calls; a later call's first level is the whole prefix up to it).  One thread per 64-bit word of a
 *   raw stream carries the OR over the levels in one register and stores each level's bitmap word, so every plane of the
 *   largest selection is read once per (e, t).  dev_byte_off [n+1], dev_adler [n] and dev_scratch (>=
 *   sola_png_deflate_scratch_bytes(n, h, w), 8-byte aligned) are those of sola_png_deflate_sizes, and
 *   sola_png_deflate_write(dev_bits_rm, 0, n, h, w, ...) completes the streams (it reads the scratch, not the planes).
 *   E*K*T < 2^31, h*(w+1) < 2^31, words_stride a multiple of 4 and >= sola_mask_words(h, w), planes 16-byte aligned.
 * Both are asynchronous on the stream and refuse bad arguments before any launch. */
int sola_planes_cm_to_rm(const uint32_t* dev_bits_cm, int64_t words_stride_cm, int64_t n_planes, int h, int w,
                         uint32_t* dev_bits_rm, int64_t words_stride_rm, void* stream);
int sola_png_deflate_sizes_select(const uint32_t* dev_bits_rm, int64_t words_stride, int n_masks, int T, int h, int w,
                                  const int32_t* dev_sel_off, const int32_t* dev_sel_idx, const int32_t* dev_level_end,
                                  int K, int E, int64_t* dev_byte_off, uint32_t* dev_adler,
                                  void* dev_scratch, size_t scratch_bytes, void* stream);

/* Connected components of the set pixels of n independent frames [n,h,w] (row-major), and the fused rewrite of the small
 * ones: what SAM2's fill_holes_in_mask_scores needs in front of the `> 0` threshold.  connectivity 8 or 4; n*h*w < 2^31
 * and at most 2^24 - 1 tiles of SOLA_CC_TILE_W x SOLA_CC_TILE_H in one call.  elem_type: 0 = uint8 != 0, 1 = float32 != 0,
 * 2 = float32 logits > 0, 3 = background of float32 scores: x <= 0 (-0.0 is set, NaN is not), 4 = uint8 == 0 and
 * 5 = float32 == 0: the complement of kinds 0 / 1, taken on read (hole filling).
 *   sola_mask_components: labels, areas int32 [n,h,w].  labels = 0 on clear pixels, else 1 + (y*w + x) of the component's
 *     first pixel in raster order within its own frame; areas = 0 on clear pixels, else the pixel count of the pixel's
 *     component.  Pure functions of the input (integer atomics only): identical from run to run and on any stream.
 *   sola_mask_fill_small: out (the element type of in; may alias in) = in, except on the pixels of set components of at
 *     most max_area pixels.  Kind 3: those become fill_value, and every other float passes through bit for bit (NaN and
 *     both zeros included).  Kinds 0, 1, 2: they become 0 (island removal).  Kinds 4, 5: they become 1 (hole filling).
 *     fill_value is read for kind 3 only.  Labels and areas are never materialised for the caller.
 *   sola_mask_fill_small_profile: the same call, then a wait for the stream; launch_us [4] (host) = the time of its four
 *     launches (tile labelling, tile borders, flatten + counts, rewrite) between HIP events.  Bench tools only.
 * dev_scratch: >= sola_mask_components_scratch_bytes(n,h,w) = 8*n*h*w rounded up to 256 bytes (0 for empty or refused
 * sizes; host-only), 4-byte aligned.  It is written before it is read: nothing depends on what it held.  Asynchronous on
 * the stream.  Refused before any launch: connectivity other than 4 / 8, max_area < 0, a short scratch, n*h*w >= 2^31.  Any
 * of n, h, w equal to 0 is a successful no-op. */
#define SOLA_CC_TILE_W 64
#define SOLA_CC_TILE_H 16
size_t sola_mask_components_scratch_bytes(int n, int h, int w);
int sola_mask_components(const void* dev_masks, int elem_type, int n, int h, int w, int connectivity, int32_t* dev_labels,
                         int32_t* dev_areas, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_mask_fill_small(const void* dev_in, int elem_type, int n, int h, int w, int connectivity, int64_t max_area,
                         float fill_value, void* dev_out, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_mask_fill_small_profile(const void* dev_in, int elem_type, int n, int h, int w, int connectivity, int64_t max_area,
                                 float fill_value, void* dev_out, void* dev_scratch, size_t scratch_bytes, void* stream,
                                 float* launch_us);

/* ---- the grid-prompt stage: what SAM2's automatic mask generator computes per mask and per box (track_generation/
 * generate_prompts_grid.py:67,100; the stability score of prompt_generator.py:169-185) --------------------------------------
 * sola_mask_logit_stats: n maps [n,h,w] (row-major) -> dev_stats int64 [n,7] = (n_hi, n_lo, area, x0, y0, x1, y1), from ONE
 *   read of the maps (16-byte loads wherever the address allows, any w, any alignment of the element type).
 *   elem_type 2 = float32 logits: a pixel counts for a threshold t when x > t (strict; NaN never counts, -0.0 does not
 *   count at t = 0); n_hi, n_lo and area are the counts at thr_hi, thr_lo and thr.  elem_type 0 / 1 = uint8 / float32 masks,
 *   set where != 0: all three counts are the area and the thresholds are not read.  (x0, y0, x1, y1) is the INCLUSIVE
 *   bounding box of the pixels that count for thr; a map with none has (0, 0, 0, 0), batched_mask_to_box's convention.
 *   SAM2's stability score is n_hi / n_lo with thr_hi = mask_threshold + offset, thr_lo = mask_threshold - offset.
 *   Partial results meet in 64-bit integer atomics after a memset of the table on the stream (no workspace): exact in any
 *   order, identical from run to run.  Refused before any launch: negative sizes, elem_type outside 0..2, h*w >= 2^31 (a
 *   map is indexed in int32; n*h*w then fits 2^62), more than 2^31 - 1 pieces of 64 KiB in one call, masks not aligned to
 *   their element.  n == 0 is a successful no-op; with n > 0 and h*w == 0 the rows are written as zeros.  Asynchronous.
 * sola_box_nms: greedy non-maximum suppression of n boxes [n,4] float32 (x0, y0, x1, y1), 16-byte aligned.  dev_order [n]
 *   int64 is the visiting order, a permutation of 0..n-1 (an entry outside that range is read as 0, never outside the
 *   arrays); dev_idxs [n] int64 gives every box a category, NULL = one category.  Box order[a] is kept unless a KEPT box
 *   order[b], b < a, of the same category has iou > iou_threshold; categories never interact (torchvision's per-category
 *   batched_nms exactly, and its coordinate-offset form without that form's rounding).  dev_keep receives the kept original
 *   indices in visiting order, dev_n_keep [1] their number; dev_keep beyond that is not written.  The IoU is float32, every
 *   operation rounded on its own, in this order: area = (x1 - x0) * (y1 - y0); iw = max(0, min(x1a, x1b) - max(x0a, x0b)),
 *   ih likewise; inter = iw * ih; iou = inter / ((area_a + area_b) - inter), a correctly rounded division.  0/0 is NaN and
 *   does not suppress: two identical zero-area boxes both survive.  The decision equals a float32 restatement on any finite input.
 *   Two launches: the upper triangle of the suppression bit matrix (64 boxes per word), then one workgroup that settles the
 *   order 64 rows at a time.  dev_scratch: >= sola_box_nms_scratch_bytes(n) = n * ceil(n/64) * 8 rounded up to 256 bytes (0
 *   for n <= 0 or n > SOLA_BOX_NMS_MAX_N; host-only), 8-byte aligned; written before it is read.  n > SOLA_BOX_NMS_MAX_N, a
 *   negative n, a short scratch and null arguments are refused before any launch; n == 0 only writes dev_n_keep = 0.
 *   sola_box_nms_profile: the same call, then a wait for the stream; launch_us [2] (host) = the time of the matrix and the
 *   resolve launch between HIP events.  Bench tools only. */
#define SOLA_BOX_NMS_MAX_N 16384
int sola_mask_logit_stats(const void* dev_masks, int elem_type, int n, int h, int w, float thr, float thr_hi, float thr_lo,
                          int64_t* dev_stats, void* stream);
size_t sola_box_nms_scratch_bytes(int n);
int sola_box_nms(const float* dev_boxes, const int64_t* dev_order, const int64_t* dev_idxs, int n, float iou_threshold,
                 int64_t* dev_keep, int64_t* dev_n_keep, void* dev_scratch, size_t scratch_bytes, void* stream);
int sola_box_nms_profile(const float* dev_boxes, const int64_t* dev_order, const int64_t* dev_idxs, int n, float iou_threshold,
                         int64_t* dev_keep, int64_t* dev_n_keep, void* dev_scratch, size_t scratch_bytes, void* stream,
                         float* launch_us);

/* ---- index maps -> bit planes: the palette-PNG ground truth of Ref-DAVIS / Ref-YouTube-VOS (dataloader.py:260-276
 * load_gt_masklet; track_generation/seg_utils.py:29-49 get_masklets_ytbvos) -----------------------------------------------
 * dev_idx: T maps [T,h,w] of uint8 (row-major), the value of a pixel is its object id; any w, any alignment of the base.
 * sola_index_hist: dev_counts int64 [T,256] = the pixels of every value in every frame, from ONE read of the maps (16-byte
 *   loads wherever the address allows).  Per-block LDS histograms meet in 64-bit integer atomics after a memset of the table
 *   on the stream (no workspace): exact in any order, identical from run to run, also when a frame holds a single value.
 *   T == 0 is a successful no-op; with T > 0 and h*w == 0 the table is written as zeros.
 * sola_index_pack: plane (dev_first_plane ? dev_first_plane[k] : k*T) + t of dev_bits [planes, words_stride] receives
 *   (idx[t] == dev_ids[k]) for every k < K, t < T; the maps are read once for all K ids (the ids are taken
 *   SOLA_INDEX_ID_CHUNK at a time; a longer list loops inside the launch).  dev_ids / dev_first_plane: int32 [K] on the
 *   device.  An id outside 0..255 gives empty planes; 0 and 255 are ordinary values; ids may repeat.  dev_first_plane lets
 *   the planes fall into rows of a buffer whose other rows sola_rle_pack_cm fills: the ranges [first, first + T) must be
 *   disjoint and inside the buffer (a negative entry writes nothing).  Every word of every addressed plane up to
 *   words_stride is written, tail and pad bits as zeros, by exactly one thread (no atomics, no memset of the planes); rows
 *   not addressed are not touched.
 *     layout 0: row-major, the format of sola_mask_pack / sola_mask_pair_counts: bit j of word i is pixel 32*i + j of the
 *       raster; words_stride >= sola_mask_words(h, w).
 *     layout 1: column-major, the format of sola_rle_pack_cm / sola_mask_select_counts: position = x*h + y; words_stride a
 *       multiple of 4 and >= sola_jf_plane_words(h, w), planes 16-byte aligned; h <= SOLA_INDEX_MAX_H (frames of more than
 *       1259 rows take narrower column strips, a slower path with the same result).
 *   dev_area (optional, int64, indexed by plane like dev_bits): the popcount of every addressed plane, either layout.
 *   Refused before any launch: negative sizes, a layout other than 0 / 1, h*w >= 2^31, a short or (layout 1) odd
 *   words_stride, misaligned planes, null ids / bits.  T == 0 or K == 0 is a successful no-op.  Asynchronous. */
#define SOLA_INDEX_ID_CHUNK 8
#define SOLA_INDEX_MAX_H 16384
int sola_index_hist(const uint8_t* dev_idx, int T, int h, int w, int64_t* dev_counts, void* stream);
int sola_index_pack(const uint8_t* dev_idx, int T, int h, int w, const int32_t* dev_ids, int K, const int32_t* dev_first_plane,
                    int layout, int64_t words_stride, uint32_t* dev_bits, int64_t* dev_area, void* stream);

/* ---- frame preprocessing: Pillow's 8-bit resize and the normalisation behind it (SAM2's init_state does
 * `Image.open(p).convert("RGB").resize((1024, 1024))`, `/ 255.0`, `-= mean`, `/= std` per frame on the host; GroundingDINO's
 * transform is a PIL bilinear resize, ToTensor, Normalize).  Upstream details are from the public sources. -------------------
 * filter: SOLA_RESAMPLE_BILINEAR (triangle, support 1) or SOLA_RESAMPLE_BICUBIC (a = -0.5, support 2): PIL's own numbers.
 * sola_resample_taps: the taps of one axis, ceil(support * max(in/out, 1)) * 2 + 1; -1 for a filter or a size it refuses.
 * sola_resample_coeffs (host only, double arithmetic, Pillow's precompute_coeffs + normalize_coeffs_8bpc): for every output index
 *   bounds [out,2] = (first source index, taps used) and coeffs [out,taps] = the weights times 2^22 rounded half away from zero,
 *   zero past the taps used.  Both host arrays.
 * An axis TABLE of sola_resample_u8 is int32 [out][2 + taps] ON THE DEVICE: row o = (bounds[o][0], bounds[o][1], coeffs[o][:]).
 * sola_resample_u8: dev_src uint8 [T,H,W,C], interleaved, C 1 or 3, any byte alignment.  A null table (with taps 0) means that
 *   axis keeps its size and its pass is skipped, as Pillow does.  dev_lut null: dev_out uint8 [T,h,w,C].  dev_lut float32
 *   [C,256]: dev_out float32 planar [T,C,h,w] = lut[c][byte] (4-byte aligned; 16-byte aligned with w % 4 == 0 gets 16-byte
 *   stores).  Per pass a 32-bit accumulator starts at 1 << 21, adds pixel * k, is shifted right by 22 and clamped to 0..255;
 *   the horizontal result is a byte before the vertical pass reads it: the bytes of PIL.Image.resize.  One launch per batch
 *   (tiles of SOLA_RESAMPLE_TILE_W x SOLA_RESAMPLE_TILE_H output pixels staged in LDS); reductions whose staging does not fit
 *   take two launches through a byte intermediate in dev_scratch, >= sola_resample_u8_scratch_bytes(...) (host only; 0 for the
 *   one-launch geometries, where dev_scratch may be null).  No atomics, no allocation, asynchronous; the same bits on every run
 *   and stream.  Bounds read from a table are clamped to the source: a table that sola_resample_coeffs did not write gives
 *   wrong pixels, no access outside the buffers.  Refused before any launch: null src / out, C other than 1 / 3, an axis of 0
 *   or beyond SOLA_RESAMPLE_MAX_SIZE, a table without taps or taps without a table, a null table on an axis whose size
 *   changes, a short scratch.  T == 0 is a successful no-op. */
#define SOLA_RESAMPLE_BILINEAR 2
#define SOLA_RESAMPLE_BICUBIC 3
#define SOLA_RESAMPLE_MAX_SIZE 16384
#define SOLA_RESAMPLE_TILE_W 64
#define SOLA_RESAMPLE_TILE_H 64
int sola_resample_taps(int in_size, int out_size, int filter);
int sola_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs);
size_t sola_resample_u8_scratch_bytes(int T, int H, int W, int C, int h, int w, int taps_x, int taps_y);
int sola_resample_u8(const uint8_t* dev_src, int T, int H, int W, int C, int h, int w, const int32_t* dev_table_x, int taps_x,
                     const int32_t* dev_table_y, int taps_y, const float* dev_lut, void* dev_out, void* dev_scratch,
                     size_t scratch_bytes, void* stream);

/* ---- baseline JPEG decode: the bytes of PIL's `Image.open(f).convert("RGB")` (libjpeg's integer arithmetic) from the file's
 * bytes, entropy decode included, on the device. ------------------------------------------------------------------------------
 * Supported files: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding (default or optimised tables), 8-bit
 *   quantisation tables, ONE interleaved scan; one component (grey: three equal channels) or three read as YCbCr with luma
 *   sampling 1x1, 2x1 or 2x2 and chroma 1x1; restart intervals (DRI / RSTn); any number of APPn / COM segments (skipped; EXIF
 *   orientation is ignored, as PIL ignores it).
 * sola_jpeg_parse REFUSES, with sola_last_error() naming which: progressive, extended, lossless, hierarchical or arithmetic
 *   SOFs; 12-bit samples; 16-bit quantisation tables; four (or two) components; an Adobe segment with a transform other than 1
 *   on three components, or components named R, G, B without a JFIF / Adobe segment (libjpeg reads those as RGB); other
 *   sampling factors (4:4:0, 4:1:1, subsampled luma, chroma that is not 1x1); more than one scan (a non-interleaved scan, or a
 *   DHT / DQT / DRI / SOS behind the first); a DNL marker; an 0xFF fill byte or any marker other than RSTn / EOI inside the
 *   scan; RSTn out of order, without a DRI, or more of them than the frame has intervals; a missing table; a DHT that is no
 *   prefix code or holds a DC category above 15; width or height of 0 or above SOLA_JPEG_MAX_SIZE; a scan of 2^28 bytes or
 *   more; any length field that points outside the buffer.  A file cut short inside its scan (no EOI) is ACCEPTED: the scan
 *   ends with the buffer.
 * sola_jpeg_parse (host only, touches no device, reads data[0 .. len) and nothing else): fills *plan - geometry and sampling,
 *   the quantisation tables of the components in natural (row-major) order, the Huffman tables of the components in the
 *   lookup form below, the scan's byte range [scan_begin, scan_end) in the file, the restart interval (MCUs, 0 = none) and
 *   n_segments - and writes the first seg_cap restart segments' byte ranges to host_segs, int32 [seg_cap][2] = [begin, end)
 *   counted from scan_begin (a file without DRI is one segment; host_segs may be null with seg_cap 0: a caller that finds
 *   n_segments > seg_cap calls again).  scan_offset and seg_offset are left 0: the caller of sola_jpeg_decode sets them.
 * SolaJpegHuff: look[next 8 bits] = (length << 8) | symbol of the codes of <= 8 bits, else 0; a longer code has the smallest
 *   length l (9 .. 16) with (next 16 bits) < limit[l], and is vals[((next 16 bits) >> (16 - l)) + valoff[l]].
 * sola_jpeg_decode: T frames that share width, height, components and sampling (tables, restart intervals and scan lengths
 *   are per frame).  dev_scan holds their raw scan bytes, byte stuffing and restart markers in place: frame t's bytes
 *   [scan_begin, scan_end) of its file at dev_scan + plans[t].scan_offset.  dev_segs: the frames' segment ranges, int32
 *   [n_segs][2], frame t's at row plans[t].seg_offset.  plans (host) and dev_plans (the same T structs in device memory).
 *   dev_out uint8 [T,H,W,3].  Synchronous: the call returns when the pixels are written (it reads a device flag between the
 *   rounds of the decoder's synchronisation).  host_err int32 [T] receives each frame's error word (0: every restart segment
 *   decoded to its last block and no further; else bits 1 = a bit pattern without a code, 2 = a run past coefficient 63, 4 =
 *   entropy data behind the last block, 8 = a segment that ends early); host_rounds (optional) the number of launches of the
 *   synchronisation kernel.  The call succeeds whatever the error words say.
 *   Arithmetic: DC predicted per component, reset at each restart; coefficients times their quantiser as int16; the 8x8
 *   "islow" integer IDCT (13-bit constants, column pass descaled by 11, row pass by 18, + 128, clamped); each component plane
 *   cropped to ceil(W*h_i/h_max) x ceil(H*v_i/v_max) before upsampling; "fancy" (triangle) chroma upsampling 2x1 and 2x2
 *   with libjpeg's rounding (plain replication where the cropped chroma plane is 1 or 2 samples wide, as libjpeg does);
 *   YCbCr -> RGB in 16-bit fixed point.  Equal to Pillow in every byte for files an encoder produced.
 *   Entropy decode: each restart segment is cut into subsequences of subseq_bytes (0 = SOLA_JPEG_SUBSEQ_DEFAULT; a power of two
 *   SOLA_JPEG_SUBSEQ_MIN .. SOLA_JPEG_SUBSEQ_MAX), one thread each; a thread's start state (bit position, block in the MCU,
 *   zigzag index) is known at a segment start and guessed elsewhere, and is replaced by its predecessor's end state until
 *   nothing changes: behind barriers inside a workgroup, by another launch across workgroups (the self-synchronising decode
 *   of Weissenberger and Schmidt).  After round r the first r subsequences are final: at most as many launches as
 *   a frame has workgroups, enforced by the host loop; no kernel waits for another workgroup.  Integer arithmetic and two
 *   integer atomic ORs (error word, change flag): the same bits on every run and stream.
 *   Nothing read from the device is trusted: every read of the scan is checked against the frame's range and its segment, every
 *   coefficient write against the segment's block range, every table index is masked.  A damaged file, plan or segment table
 *   gives wrong pixels or an error word, never an access outside dev_scan, dev_scratch or dev_out.
 *   Refused before any launch: T < 1, null pointers, frames that differ in geometry, a plan whose numbers do not fit together,
 *   ranges outside scan_bytes / n_segs, subseq_bytes not as above, a scratch below sola_jpeg_scratch_bytes(plans, T,
 *   subseq_bytes) (host only; 0 for arguments it refuses) or not 16-byte aligned. */
#define SOLA_JPEG_MAX_SIZE 16384
#define SOLA_JPEG_SUBSEQ_MIN 16
#define SOLA_JPEG_SUBSEQ_MAX 4096
#define SOLA_JPEG_SUBSEQ_DEFAULT 128
typedef struct SolaJpegHuff {
    uint16_t look[256];
    uint32_t limit[18];  /* [1 .. 16] used; 18 entries keep the struct a multiple of 16 bytes */
    int32_t valoff[18];
    uint8_t vals[256];
} SolaJpegHuff;
typedef struct SolaJpegPlan {
    int32_t width, height, ncomp;
    int32_t hs, vs;                  /* luma sampling factors (chroma is 1x1); 1, 1 for one component */
    int32_t mcus_x, mcus_y, blocks_per_mcu, n_blocks;
    int32_t restart_interval, n_segments, reserved;
    int64_t scan_begin, scan_end;    /* the entropy-coded bytes of the file */
    int64_t scan_offset, seg_offset; /* set by the caller of sola_jpeg_decode: where this frame's scan and segments lie */
    uint16_t quant[3][64];           /* by component, natural order */
    SolaJpegHuff huff[6];            /* component * 2 + (0 DC, 1 AC) */
} SolaJpegPlan;
int sola_jpeg_parse(const uint8_t* data, int64_t len, SolaJpegPlan* plan, int32_t* host_segs, int64_t seg_cap);
size_t sola_jpeg_scratch_bytes(const SolaJpegPlan* plans, int T, int subseq_bytes);
int sola_jpeg_decode(const uint8_t* dev_scan, int64_t scan_bytes, const int32_t* dev_segs, int64_t n_segs, const SolaJpegPlan* plans,
                     const SolaJpegPlan* dev_plans, int T, int subseq_bytes, uint8_t* dev_out, void* dev_scratch, size_t scratch_bytes,
                     int32_t* host_err, int32_t* host_rounds, void* stream);
/* test / measurement hooks of the same call: sola_jpeg_coefficients copies frame t's coefficient buffer (int16 [n_blocks][64],
 * natural order, times the quantiser, DC as values) of the LAST sola_jpeg_decode on that scratch to the host;
 * sola_jpeg_profile: the HIP-event time in ms of each stage of the next calls is added to host_ms[6] (layout, synchronisation,
 * block indices + coefficient write, DC scan, IDCT, upsample + colour) - null switches it off.  Not for concurrent use. */
int sola_jpeg_coefficients(const SolaJpegPlan* plans, int T, int subseq_bytes, const void* dev_scratch, int t, int16_t* host_coef, void* stream);
int sola_jpeg_profile(float* host_ms);

/* ---- multi-scale deformable attention, forward (Deformable-DETR; GroundingDINO's one custom operator,
 * groundingdino._C.ms_deform_attn_forward; Mask2Former's pixel decoder).  Upstream details are from its public source. -------
 * All float32, contiguous:
 *   dev_value [N,S,M,D]: batch, S = sum_l H_l*W_l rows in level order, heads, channels per head;
 *   dev_spatial_shapes int64 [L,2] = (H_l, W_l) and dev_level_start int64 [L], both ON THE DEVICE (never read by the host);
 *   dev_sampling_loc [N,Lq,M,L,P,2], normalised, last axis (x, y);  dev_attn_weight [N,Lq,M,L,P];  dev_out [N,Lq,M*D].
 * For query q, head m, level l, point p: x = fma(loc_x, W_l, -0.5), y = fma(loc_y, H_l, -0.5) (one rounding each); x0 = floor(x),
 * y0 = floor(y), lx = x - x0, ly = y - y0; the corners (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) carry (1-ly)(1-lx),
 * (1-ly)lx, ly(1-lx), ly*lx; a corner outside [0,H_l) x [0,W_l) contributes nothing, one inside reads row
 * level_start[l] + yy*W_l + xx of value[n,:,m,:];  out[n,q,m*D:(m+1)*D] = sum_{l,p} attn_weight[n,q,m,l,p] * bilinear sample,
 * summed in float32 in the fixed order (l, p, corner), every step a fused multiply-add.  This is F.grid_sample(level map,
 * 2*loc - 1, "bilinear", "zeros", align_corners=False) per level, weighted and summed.
 * The table is not trusted: a corner whose row is not in [0,S) contributes nothing; so does a level with H_l or W_l outside
 * 1 .. 2^30 or a start outside (-2^62, S) (sides float32 cannot address to a pixel; starts from which no 64-bit row sum overflows).  No
 * table and no location, NaN and infinities included, makes the kernel read outside dev_value or write outside dev_out (rows
 * are fetched through a range-checked buffer descriptor of one batch element; what a non-finite location contributes is
 * unspecified).  One launch, no atomics, no workspace, no memset: every output element is written by exactly one thread, the
 * bits are the same from run to run and on any stream.  Asynchronous on the stream.
 * Refused before any launch: N, S, M or Lq < 1; D other than 16, 32, 64; L outside 1 .. SOLA_MSDA_MAX_LEVELS; P outside
 * 1 .. SOLA_MSDA_MAX_POINTS; null arguments; S*M*D*4 >= 2^31 bytes (32-bit row offsets), or N*S*M*D, N*Lq*M*L*P*2 or
 * N*Lq*M*D >= 2^31 elements; value, sampling_loc or out not 16-byte aligned (attn_weight: 4 bytes, and 16 for the P = 4
 * fast path - otherwise the any-P kernel runs, same bits; tables: 8).  The backward is sola_ms_deform_attn_backward below. */
#define SOLA_MSDA_MAX_LEVELS 8
#define SOLA_MSDA_MAX_POINTS 8
int sola_ms_deform_attn(const float* dev_value, const int64_t* dev_spatial_shapes, const int64_t* dev_level_start,
                        const float* dev_sampling_loc, const float* dev_attn_weight, int N, int S, int M, int D, int Lq, int L, int P,
                        float* dev_out, void* stream);

/* ---- multi-scale deformable attention, backward: the three gradients of sola_ms_deform_attn for dev_grad_out [N,Lq,M*D] (float32,
 * contiguous); the other inputs, their layout and the notation are the forward's.  With c_k the coefficient of corner k, v_k its row
 * of value[n,:,m,:] (zeros where the corner does not count), w = attn_weight[n,q,m,l,p] and g = grad_out[n,q,m*D:(m+1)*D]:
 *   dev_grad_weight [N,Lq,M,L,P]   = sum_d g_d * sum_k c_k v_k[d];
 *   dev_grad_loc    [N,Lq,M,L,P,2] = (W_l * w * sum_d g_d * ((1-ly)(v_01 - v_00) + ly (v_11 - v_10)),
 *                                     H_l * w * sum_d g_d * ((1-lx)(v_10 - v_00) + lx (v_11 - v_01)));
 *   dev_grad_value  [N,S,M,D]:       row_k of (n, m) receives w * c_k * g for every corner that counts.
 * This is the derivative on the cell [x0, x0+1) x [y0, y0+1), the one F.grid_sample's backward takes.
 * Each of the three outputs may be null: it is then not wanted and not computed; at least one must be given.  Every element of
 * every requested output is written by the call: dev_grad_value is zeroed by the entry point itself on the stream (the caller
 * need not), the entries of a level that does not count are written as zeros.
 * The table is distrusted exactly as in the forward: a corner that does not count issues no add and reads as zero, and no table and
 * no location, NaN and infinities included, makes the kernel read outside dev_value or write outside the three outputs.
 * dev_grad_loc and dev_grad_weight: one unit of D lanes owns each element, sums the channels in a fixed order and stores it
 * once - the bits are the same from run to run, on any stream, and with or without the other outputs.
 * dev_grad_value is a scatter accumulated with float32 atomic adds in the order the hardware delivers them: its last bits are
 * NOT repeatable from run to run (the only output of this library that is not; no ordered variant exists).  It must be ordinary
 * device memory (hipMalloc, what torch allocates): float atomics into host-coherent (fine-grained) memory are not supported.
 * One memset and one launch, no workspace.  Asynchronous on the stream.
 * Refused before any launch: everything the forward refuses (dev_grad_out in the place of dev_out, except that it needs 4-byte
 * alignment only), all three outputs null, dev_grad_value or dev_grad_weight not 4-byte aligned, dev_grad_loc not 8-byte. */
int sola_ms_deform_attn_backward(const float* dev_value, const int64_t* dev_spatial_shapes, const int64_t* dev_level_start,
                                 const float* dev_sampling_loc, const float* dev_attn_weight, const float* dev_grad_out,
                                 int N, int S, int M, int D, int Lq, int L, int P,
                                 float* dev_grad_value, float* dev_grad_loc, float* dev_grad_weight, void* stream);

/* ---- in-library kernel timing (HIP events on the launch stream; used by bench.py's roofline object) ------------ */
enum { SOLA_PROF_GEMM = 0,      /* gemm_nt_f32_kernel<128,128> */
       SOLA_PROF_ATTN = 1,      /* attn_fwd_f32_kernel */
       SOLA_PROF_NORM = 2,      /* group_norm_kernel */
       SOLA_PROF_WS = 3,        /* ws_standardize_kernel */
       SOLA_PROF_HEAD = 4,      /* score head / loss / select */
       SOLA_PROF_MISC = 5,      /* pos-encoding, lang concat */
       SOLA_PROF_IOU_PACK = 6,  /* mask_pack_kernel */
       SOLA_PROF_IOU_PAIR = 7,  /* mask_pair_kernel */
       SOLA_PROF_GEMM_SMALL = 8, /* gemm_nt_f32_kernel<64,64> (small grids) */
       SOLA_PROF_GEMM_TN = 9,   /* gemm_tn_f32_kernel (weight gradients) */
       SOLA_PROF_ATTN_BWD = 10, /* attn_bwd_* kernels */
       SOLA_PROF_GEMM_SPLIT = 11, /* split-f16 GEMMs other than the 256x256 shape (128x128 glds blocks, 64x64 small grids) */
       SOLA_PROF_GEMM_SPLIT256 = 12, /* gemm_nt_split_glds_persist_kernel<*> (and the one-tile <4,2,4,*> kernel): 256x256 blocks, split-f16, 3 x f16 MFMA */
       SOLA_PROF_GEMM_SPLIT256_GN = 13, /* the same kernel with GroupNorm + LeakyReLU applied in the epilogue (encoder conv0-2): its time includes the norm */
       SOLA_PROF_NCAT = 14 };
/* Kernel-schedule switches for within-process A/B measurements and tests (e.g. "train_bf16_store", "iou_fused", "attn_split_min_keys",
 * "infer_f32_rows", "train_split_min_rows").  Not part of the drop-in boundary: the defaults are the shipped path.  The catalogue of keys,
 * values and what each was measured to do lives in docs/tune_keys.md; an unknown key returns SOLA_ERR_ARG.  Except under the *_ablate keys
 * (measurement only), results are identical across variants up to f32 summation order. */
int sola_tune(const char* key, int value);
/* Read a key back without changing it; either pointer may be null, an unknown key returns SOLA_ERR_ARG as in sola_tune.  `value` is the
 * argument that, handed to sola_tune now, leaves the library as it is (so a borrower queries, sets, and hands the queried value back);
 * `default_value` is the same report taken when the library was loaded, before any sola_tune call.  For most keys both are simply the
 * switch; the keys whose setter clamps or writes two switches report as sola_amd/csrc/tune.h says. */
int sola_tune_query(const char* key, int* value, int* default_value);
/* The index-th key of this build (0, 1, ...), NULL past the end. */
const char* sola_tune_key(int index);
/* 1 when the library was built with EXPERIMENTS=1 (make -C sola_amd/csrc EXPERIMENTS=1): the closed experiments' kernels and their
 * sola_tune keys (SOLA_TUNE_EXPERIMENT_KEYS in sola_amd/csrc/tune.h; marked (EXPERIMENTS) in docs/tune_keys.md) exist only there; the
 * default library rejects those keys. */
int sola_has_experiments(void);
/* Self-test of the library's cross-lane primitives on the current device: wave sums / maxima on v_permlane*_swap + DPP against the
 * ds_bpermute butterfly, every lane of every step bit for bit (synchronises the stream).  SOLA_OK or SOLA_ERR_STATE + sola_last_error(). */
int sola_selftest(void* stream);

/* Measurement only (no reference counterpart): with sola_tune "gemm_trace" 1 the plain persistent split-f16 GEMM (no conv, no
 * residual, f32 output) runs an instrumented instantiation that records, per (block, wave), the cycles spent at the k-tile wait +
 * barrier, in the k-loops and in the epilogues, and real-time stamps per tile.  Copies the record of the last traced launch to
 * `host` (device-synchronising); returns the bytes written, 0 if nothing was traced, < 0 on error.  Layout: tools/gemm_trace.py. */
long long sola_gemm_trace_read(void* host, long long bytes);
/* In-library kernel timing: two HIP events on the launch stream around every kernel launch.  enable 0 = off, 1 = every category,
 * a larger value = only the categories c with bit (c + 1) set (each timed launch costs two event records, ~1.5 us of stream time
 * each: 2.8 % of the headline step with every category on, tools/prof_overhead.py). */
int sola_profile_enable(int enable);
/* Synchronises the recorded events and returns, per category: launches, total milliseconds, algorithmic flops,
 * algorithmic bytes accumulated since the last reset. Arrays have SOLA_PROF_NCAT entries. */
int sola_profile_read(int64_t* launches, double* ms, double* flops, double* bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif /* SOLA_HIP_H */
