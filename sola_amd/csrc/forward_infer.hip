// Inference forwards - of a uniform batch (sola_forward) and of a ragged one (sola_forward_ragged) - in all three inference
// precisions (sola_set_precision(ctx, 0 / 1 / 2)).  Same network, same kernels and the same single [B,N,T',D] layout as the
// training forward (forward.hip) without what only its backward reads; the modes differ in the arithmetic of the dense
// contractions (98 % of the FLOPs) and in the storage.  Both sequences are written on ONE set of layer builders (InferBuilder
// below), which holds everything that depends on the mode; a sequence says which units a sub-block runs over (sites.h).
//
// Precision 0: exact f32 MFMA on f32 activations.
//
// Precision 1, split-f16: f32 MFMA runs at 1/16 of the f16 MFMA rate on gfx950 and there is no xf32, so every GEMM operand is
// kept as an (f16 hi, f16 lo) pair in the 4 bytes of the f32 it replaces and each product is evaluated as hi*hi + hi*lo + lo*hi
// on v_mfma_f32_32x32x16_f16 with f32 accumulation (gemm.hip ARITH 1): ~22-bit products, 3/16 of the matrix-pipe time,
// identical bytes.  The producers emit the split format directly - GroupNorm epilogue, attention epilogue - so only three
// tensors are converted by a separate pass (the input tokens, the conv5 output that layer 0 consumes, the text tokens).
// Softmax, GroupNorm statistics, the score head and the losses stay in f32.  Parity: the same golden-vector tests and 1e-3
// bound as the f32 mode (tests/test_gpu_fast.py).
//
// Precision 2, 16-bit storage (BASELINE configs C2 / C4 name bf16 / fp16 runs of this path; the reference's only mixed-precision
// site is track_generation/generate_tokens_grid.py:84-88): every activation between two kernels is a plain _Float16 in the first
// half of its f32-sized buffer, so the HBM-bound kernels (GroupNorm, attention, GEMM epilogues) move half the bytes, and every
// product is ONE f16 MFMA with f32 accumulation.  Softmax, GroupNorm statistics, biases, the score head and the losses stay f32.
// f16, not bf16: 11 significant bits instead of 8 for the same bytes; its narrow exponent range is covered by the machinery of
// the split-f16 mode - device-side power-of-two scales for the caller's tokens and every weight matrix, range guard words on
// everything written, exact-f32 repeat of the call when one is set (include/sola_hip.h).  Parity: a REDUCED-precision mode
// with a stated tolerance (tests/test_gpu_f16.py), reported beside the f32-class modes, never as the headline number.
#include <math.h>

#include <algorithm>

#include "ragged.h"
#include "sites.h"

// Split-f16 copies of the 12 * n_layers projection weights, each with its own power-of-two scale (max|w| -> [2^13, 2^14),
// found on the device: a trained matrix may be far from the U(-1/32, 1/32) of the default init, and a few outliers must not
// push the rest into f16 subnormals - the pair format keeps 22 bits for everything within 2^-16 of the largest entry), plus
// the weight-time range check of the activations the GroupNorms will emit (kernels.h: launch_norm_range_check).
int sola_refresh_lin16(SolaCtx* c, hipStream_t s) {
    if (!c->lin16_dirty) return SOLA_OK;
    SOLA_ARG(c->lin16_buf && c->scal_buf, "split-f16 weights requested before sola_set_precision(ctx, 1)");
    const int D = c->cfg.lang_token_dim;
    const Elem fmt = operand_format(c->precision);
    std::vector<const float*> in;
    std::vector<float*> out;
    for (int l = 0; l < c->cfg.n_layers; ++l)
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 4; ++j) {
                const std::string nm = lin_name(l, a, j) + ".weight";
                const float* w = ctx_weight(c, nm);
                if (!w) {
                    sola_set_error("forward: weight '%s' has not been set", nm.c_str());
                    return SOLA_ERR_WEIGHT;
                }
                in.push_back(w);
                out.push_back(lin16_weight(c, fmt, l, a, j));
            }
    if (is_row16(fmt)) {  // 16-bit storage mode / 16-bit GEMM operands: plain f16 / bfloat16 copies, same per-matrix scales
        const std::vector<void*> outh(out.begin(), out.end());
        SOLA_TRY(launch_cast_f16_auto_multi(in.data(), outh.data(), (int)in.size(), D, D, c->scal_pair(2), fmt, s));
    } else {
        SOLA_TRY(launch_cast_sp16_auto_multi(in.data(), out.data(), (int)in.size(), D, D, c->scal_pair(2), s));
    }
    std::vector<NormPair> norms;
    for (int i = 0; i < 5; ++i) {
        const std::string np = enc_name(kNormIdx[i]);
        norms.push_back(NormPair{ctx_weight(c, np + ".weight"), ctx_weight(c, np + ".bias"), c->conv[i].cout});
    }
    for (int l = 0; l < c->cfg.n_layers; ++l)
        for (int j = 0; j < 3; ++j) {
            const std::string np = norm_name(l, j);
            norms.push_back(NormPair{ctx_weight(c, np + ".weight"), ctx_weight(c, np + ".bias"), D});
        }
    for (const NormPair& n : norms)
        if (!n.gamma || !n.beta) {
            sola_set_error("forward: a GroupNorm weight has not been set");
            return SOLA_ERR_WEIGHT;
        }
    SOLA_HIP(hipMemsetAsync(c->guard + 1, 0, sizeof(int), s));
    for (size_t i0 = 0; i0 < norms.size(); i0 += 32)
        SOLA_TRY(launch_norm_range_check(norms.data() + i0, (int)std::min<size_t>(32, norms.size() - i0), c->guard + 1, s));
    c->lin16_dirty = false;
    return SOLA_OK;
}

// Standardises the conv weights (module/ws.py:9-13) into ws_buf and casts them into ws16_buf in the GEMM operand format `fmt`
// (Elem::F32 = none).  Runs when the weights changed, on every forward
// under the reference's policy (ws_every_forward), when ws16_buf holds another format, and always with `force` (the
// training forward).  Standardised rows are unit-variance by construction: the casts take the fixed scale 1.
int sola_refresh_conv_weights(SolaCtx* c, Elem fmt, bool force, hipStream_t s) {
    if (!force && !c->ws_dirty && !c->ws_every_forward && (fmt == Elem::F32 || c->ws16_fmt == fmt)) return SOLA_OK;
    WsLayer layers[6];
    for (int i = 0; i < 6; ++i) {
        const std::string nm = enc_name(kConvIdx[i]) + ".weight";
        layers[i] = WsLayer{ctx_weight(c, nm), c->ws_buf + c->ws_off[i], c->conv[i].cout, c->conv[i].cin, c->conv[i].k};
    }
    SOLA_TRY(launch_ws_standardize(layers, 6, s));
    c->ws16_fmt = Elem::F32;  // ws_buf is new: ws16_buf is current once the casts below have rewritten it
    if (fmt == Elem::SP16) {
        // one launch for the six matrices and the packed tap ranges of the per-frame convs (ctx.h: ws_taps): the reference's policy
        // repeats this on every forward, at the head of the step where the queue is empty and each launch is paid in full.  A range
        // starts at a multiple of cin (a multiple of 8), so it is a whole number of 8-value pair groups: the packed copy is the
        // column slice of the full cast, bit for bit.
        std::vector<CastJob> jobs;
        for (int i = 0; i < 6; ++i) {
            const ConvGeom& g = c->conv[i];
            const int kc = g.k * g.cin;
            const float* w = c->ws_buf + c->ws_off[i];
            jobs.push_back(CastJob{w, c->ws16_buf + c->ws_off[i], g.cout, kc, kc, kc});
            for (int j = 0; j < c->ws_ntaps[i]; ++j) {
                const SolaCtx::TapRange& r = c->ws_taps[i][j];
                const int kr = (r.hi - r.lo + 1) * g.cin;
                jobs.push_back(CastJob{w + r.lo * g.cin, c->ws16_taps_buf + r.off, g.cout, kr, kc, kr});
            }
        }
        for (size_t i0 = 0; i0 < jobs.size(); i0 += CAST_JOBS_MAX)  // (ten jobs with the default geometry)
            SOLA_TRY(launch_cast_sp16_multi(jobs.data() + i0, (int)std::min<size_t>(CAST_JOBS_MAX, jobs.size() - i0), 1.f, s));
    }
    for (int i = 0; i < 6 && is_row16(fmt); ++i) {
        const int kc = c->conv[i].k * c->conv[i].cin;
        const float* w = c->ws_buf + c->ws_off[i];
        SOLA_TRY(launch_cast_f16(w, kc, reinterpret_cast<_Float16*>(c->ws16_buf) + c->ws_off[i], kc, c->conv[i].cout, kc, 1.f, nullptr, fmt, s));
    }
    c->ws_dirty = false;
    c->ws16_fmt = fmt;
    return SOLA_OK;
}

// The checks every forward makes before its first launch: all weights set, a workspace of at least `need` bytes, 256-byte aligned.
// `who` ("forward", "forward_ragged") prefixes the error messages.
int sola_check_forward_args(const SolaCtx* c, const char* who, size_t need, const void* workspace, size_t ws_bytes) {
    for (const Weight& w : c->weights)
        if (!w.ptr) {
            sola_set_error("%s: weight '%s' has not been set", who, w.name.c_str());
            return SOLA_ERR_WEIGHT;
        }
    if (ws_bytes < need) {
        sola_set_error("%s: workspace %zu bytes < required %zu", who, ws_bytes, need);
        return SOLA_ERR_WORKSPACE;
    }
    SOLA_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    return SOLA_OK;
}

// sola_tune "attn_split_min_keys": units with more keys than this take the split-f16 MFMA attention on q/k/v the projection GEMMs
// wrote as split pairs.  Rounds 1-2: 64.  Round 3: behind the one-pass / register-only f32 shapes (attn_simple.hip, attn_reg.hip)
// attn.hip's kernel for split inputs lost at 80 keys (401 vs 280 us per launch in the bench) and tied at 128, so the threshold went
// to 128; with the high-occupancy shape for split inputs (attn_fwd_spin_kernel: 262 vs 362 us at 128 tracks, 270 vs 285 at 80, 216
// vs 256 at 64) the attention wins from 64 keys on, but the q/k/v GEMM pays ~70 us per launch for the split-pair epilogue: net
// gain at 128 tracks (14.41 -> 14.30 ms per step, attention 0.43 -> 0.49 of the HBM peak), net loss at 80 and 64.  96.
int g_attn_split_min_keys = 96;

int g_lang_shared_neg = 1;  // sola_tune "lang_shared_neg": 0 = the negative tokens repeated per sample through the text-side projections (A/B)

namespace {

// What the two inference sequences below (uniform batch, ragged batch) have in common: the ctx's precision mode, written ONCE
// into every descriptor.  The geometry - strides or unit tables, instance counts, sequence lengths - comes from sites.h: the encoder
// norms' from the sequence, a layer sub-block's through sub_block().
struct InferBuilder {
    SolaCtx* c;
    hipStream_t s;
    Elem opfmt;             // the call's operand format: SP16 under precision 1, F16 under precision 2, else F32 (bfloat16 operands are the training step's)
    bool sp, h16, op16;  // split-f16 operands; 16-bit storage; either (activations and weights in a 16-bit operand format)
    int* guard;
    int D, H, DH;
    float scale;
    // pieces of the sequence's workspace (use_workspace)
    float* splitk_ws = nullptr;
    size_t splitk_bytes = 0;
    void* gn_slots = nullptr;
    size_t gn_slots_bytes = 0;
    const float* pe = nullptr;
    float *q = nullptr, *k = nullptr, *v = nullptr, *attn = nullptr, *res = nullptr;  // projections / attention output / pre-norm rows of the current sub-block
    const float* text = nullptr;     // text ++ negative rows in the mode's operand format, and their key / value projections (use_text)
    long long text_rows = 0;
    float *lk = nullptr, *lv = nullptr;

    InferBuilder(SolaCtx* ctx, hipStream_t stream)
        : c(ctx), s(stream), opfmt(ctx->precision == 1 || ctx->precision == 2 ? operand_format(ctx->precision) : Elem::F32), sp(opfmt == Elem::SP16), h16(opfmt == Elem::F16),
          op16(sp || h16), guard(op16 ? ctx->guard : nullptr),
          D(ctx->cfg.lang_token_dim), H(ctx->cfg.num_heads), DH(D / H), scale(1.0f / sqrtf((float)DH)) {}

    const float* W(const std::string& name) const { return ctx_weight(c, name); }
    Elem stored(bool on) const { return on ? opfmt : Elem::F32; }  // an activation kept in the mode's 16-bit storage, or f32 rows

    int check_mode() const {
        if (sp)
            SOLA_ARG(c->cfg.object_token_dim % 8 == 0 && (c->cfg.lang_token_dim / c->cfg.n_groups_module) % 8 == 0 &&
                         (2 * c->cfg.object_token_dim / c->cfg.n_groups) % 8 == 0 && (c->cfg.lang_token_dim / c->cfg.n_groups) % 8 == 0,
                     "split-f16 mode needs channel counts per GroupNorm group that are multiples of 8");
        if (h16)
            SOLA_ARG(c->cfg.object_token_dim % 64 == 0 && c->cfg.lang_token_dim % 64 == 0,
                     "16-bit storage mode needs object_token_dim and lang_token_dim to be multiples of 64");
        return SOLA_OK;
    }
    template <class Buf>  // buf(name): the sequence's workspace buffers
    void use_workspace(float* splitk, size_t splitk_b, void* slots, size_t slots_b, Buf&& buf) {
        splitk_ws = h16 ? nullptr : splitk;  // the 16-bit GEMMs never split K
        splitk_bytes = splitk_ws ? splitk_b : 0;
        gn_slots = slots; gn_slots_bytes = slots_b; pe = buf("pe");
        q = buf("q"); k = buf("k"); v = buf("v"); attn = buf("attn"); res = buf("res"); lk = buf("lk"); lv = buf("lv");
    }
    void use_text(const float* rows_in, long long rows) { text = rows_in; text_rows = rows; }
    // The projection weights are used as they are by the reference (no per-forward transform), so their 16-bit copies are
    // refreshed only when a weight pointer or value changed (sola_set_weight / sola_weights_changed).
    int prepare_weights() const {
        SOLA_TRY(sola_refresh_conv_weights(c, opfmt, false, s));
        if (op16) {
            SOLA_TRY(sola_refresh_lin16(c, s));
            SOLA_HIP(hipMemsetAsync(c->guard, 0, sizeof(int), s));  // per-call range guard word (ctx.h)
        }
        return SOLA_OK;
    }
    // The guard words travel to the host HERE, behind the last launch of the sequence that can set guard[0] (sub_block: `tail`), and the
    // ctx's event marks the copy: the caller waits for that event only (api.hip: sola_split_guard_tripped) and enqueues its next launches
    // while the tail of this sequence - launches that write f32 rows or carry no guard pointer - still runs.  guard[1], the weight-time
    // word, is final since prepare_weights and rides along.  Not with the guard switched off (nobody reads the words) and not while the
    // stream is being captured (the read-back is skipped there altogether).
    int read_guard() const {
        if (!op16 || !c->split_guard || !c->guard_ev) return SOLA_OK;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return SOLA_OK;
        SOLA_HIP(hipMemcpyAsync(c->guard_host, c->guard, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        SOLA_HIP(hipEventRecord(c->guard_ev, s));
        c->guard_ev_recorded = true;
        return SOLA_OK;
    }

    // ---- the weights in the mode's operand format: f32 as set, split-f16 pairs (D*D floats per matrix) or plain f16 (D*D halfs)
    const float* ws_w(int i) const { return op16 ? ws16_weight(c, opfmt, i) : c->ws_buf + c->ws_off[i]; }
    GemmProblem lin_problem(const float* a, int layer, int attn_i, int proj, const float* r, float* out) const {
        const std::string nm = lin_name(layer, attn_i, proj);
        const float* w = op16 ? lin16_weight(c, opfmt, layer, attn_i, proj) : W(nm + ".weight");
        return GemmProblem{a, w, W(nm + ".bias"), r, out, op16 ? c->lin_inv_scale(layer, attn_i, proj) : nullptr};
    }

    // ---- the caller's tensors.  Their magnitude is unknown (SAM2 memory-attention features here, anything elsewhere).  Split-f16:
    // the largest entry is mapped into [2^13, 2^14) by a power of two found on the device and the first GEMM's epilogue undoes it.
    // 16-bit storage: largest magnitude -> [2^6, 2^7), and conv0's output STAYS in those scaled units (its standardised weights
    // have a gain of sqrt(k*cin) = 28: tokens at 1e3 would leave the f16 range if the scale were undone here, tokens at 1e-5 would
    // sink into subnormals): the bias is multiplied by the scale in conv0's epilogue and the first GroupNorm multiplies by the
    // inverse while it reads, so its statistics (and eps) see the true values.  The scale is capped at 2^8: conv0's bias rides
    // along multiplied by it (tokens of 1e-5 would ask for 2^21 and carry a bias of 0.03 to 75 000); below the cap the smallest
    // token entries lose some of their 11 bits to f16 subnormals.
    int cast_obj(const float* obj, float* obj_sp, long long rows) const {
        const int d_in = c->cfg.object_token_dim;
        if (sp) return launch_cast_sp16_auto(obj, d_in, obj_sp, d_in, rows, d_in, c->scal_pair(0), s);
        return launch_cast_f16(obj, d_in, obj_sp, d_in, rows, d_in, 256.f, c->scal_pair(0), opfmt, s, 6, c->scal_extra(0));
    }
    int cast_lang(const float* lang, float* lang_sp, long long rows) const {
        if (sp) return launch_cast_sp16_auto(lang, D, lang_sp, D, rows, D, c->scal_pair(1), s);
        return launch_cast_f16(lang, D, lang_sp, D, rows, D, 1.f, c->scal_pair(1), opfmt, s, 6);
    }
    const float* lang_inv_scale() const { return op16 ? c->scal_pair(1) + 1 : nullptr; }  // undone by the text-side projections

    // ---- GEMMs
    GemmDesc gemm(long long rows, int N, int K) const {
        GemmDesc gd{};
        gd.M = (int)rows; gd.N = N; gd.K = K; gd.ldc = N;
        gd.ab = opfmt;
        if (op16) gd.out_scale = 1.f;
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        return gd;
    }
    // Encoder conv i over `rows` output rows (module/module.py:74-96).  conv5 (no norm behind it) feeds layer 0 both as the
    // projections' A operand and as the first residual: in the 16-bit modes its epilogue writes the operand format directly, no f32
    // copy and no cast pass.  (Split pairs need cout % 8 == 0: conv5's cout is lang_token_dim, a multiple of 8 * n_groups_module
    // under check_mode, so the mode always has it.)
    GemmDesc conv_gemm(int i, const float* x, float* out, long long rows) const {
        const ConvGeom& g = c->conv[i];
        GemmDesc gd = gemm(rows, g.cout, g.k * g.cin);
        gd.nprob = 1;
        gd.p[0] = GemmProblem{x, ws_w(i), W(enc_name(kConvIdx[i]) + ".bias"), nullptr, out};
        gd.lda = g.cin;
        gd.conv = g.k > 1 ? 1 : 0;
        gd.stride = g.stride; gd.pad = g.pad; gd.Cin = g.cin;
        gd.guard = guard;
        if (sp) {
            gd.c = stored(i == 5);
            if (i == 0) gd.out_scale_dev = c->scal_pair(0) + 1;
        }
        if (h16) {
            gd.c = opfmt;
            if (i == 0) gd.bias_scale_dev = c->scal_extra(0);
        }
        return gd;
    }
    // Launches encoder conv i of a UNIFORM batch (gd.T_in / gd.T_out set).  Split-f16 mode: where the conv has a per-frame form whose
    // launches all fill the persistent 256x256 kernel and save at least a sixteenth of the conv launch's rounds x K (conv3 and conv4
    // over T' = 4 frames from 128 samples of 64 tracks on: their two padding taps of twelve are not multiplied), it runs as plain
    // GEMMs per frame - same bits (conv_frames.hip).  conv0-2 (one padding tap, its launch would fill half a round), T' = 16 and
    // small batches keep the implicit-im2col launch by that rule.  So do, by construction, the exact-f32 and 16-bit storage modes,
    // the ragged forward (row maps, T varying by sequence) and the training forward: they do not come through here.
    int launch_conv(int i, const GemmDesc& gd) const {
        ConvFramePlan fp;
        if (sp && conv_frames_plan(gd, fp) && conv_frames_pays(gd, fp)) {
            ConvTapWeights tw;
            for (int j = 0; j < c->ws_ntaps[i]; ++j) {
                tw.e[tw.n].lo = c->ws_taps[i][j].lo; tw.e[tw.n].hi = c->ws_taps[i][j].hi;
                tw.e[tw.n++].w = c->ws16_taps_buf + c->ws_taps[i][j].off;
            }
            if (conv_frames_has_weights(gd, fp, tw)) return launch_conv_frames(gd, fp, tw, s);
        }
        return launch_gemm(gd, s);
    }
    // nprob projections first_proj.. of one attention in one launch.  out_sp: split-f16 q/k/v for the split attention kernel
    // (the 16-bit storage mode writes f16 always, f32 ignores it)
    int linear3(const float* a0, const float* a1, const float* a2, int layer, int attn_i, int nprob, long long rows, float* o0, float* o1,
                float* o2, int first_proj, bool out_sp, const float* a_inv_scale = nullptr) const {
        const float* as[3] = {a0, a1, a2};
        float* os[3] = {o0, o1, o2};
        GemmDesc gd = gemm(rows, D, D);
        gd.nprob = nprob;
        for (int j = 0; j < nprob; ++j) gd.p[j] = lin_problem(as[j], layer, attn_i, first_proj + j, nullptr, os[j]);
        gd.lda = D;
        gd.guard = guard;
        if (op16) gd.out_scale_dev = a_inv_scale;
        gd.c = h16 ? opfmt : stored(sp && out_sp);
        return launch_gemm(gd, s);
    }
    // res = attn * W_out^T + bias + resid; every residual of the path is in the mode's operand format
    int out_proj(int layer, int attn_i, long long rows, const float* resid) const {
        GemmDesc gd = gemm(rows, D, D);
        gd.nprob = 1;
        gd.p[0] = lin_problem(attn, layer, attn_i, 3, resid, res);
        gd.lda = D; gd.ldr = D;
        gd.r = opfmt;
        if (h16) { gd.c = opfmt; gd.guard = guard; }
        return launch_gemm(gd, s);
    }

    // ---- GroupNorms.  out16: y / y2 in the mode's 16-bit storage (split pairs or f16); f32 ignores it
    GroupNormDesc norm(const std::string& name, const float* x, float* y, int C, int groups, bool out16) const {
        GroupNormDesc nd{};
        nd.slice_ws = gn_slots; nd.slice_ws_bytes = gn_slots_bytes;
        nd.x = x; nd.y = y;
        nd.gamma = W(name + ".weight"); nd.beta = W(name + ".bias");
        nd.C = C; nd.groups = groups; nd.eps = 1e-5f;
        nd.guard = out16 ? guard : nullptr;  // f32 rows are never range-checked (norm.hip: launch_group_norm drops the pointer for them)
        nd.out = stored(out16);
        if (h16) nd.in = opfmt;
        return nd;
    }
    GroupNormDesc encoder_norm(int i, const float* x, float* y) const {
        GroupNormDesc nd = norm(enc_name(kNormIdx[i]), x, y, c->conv[i].cout, c->cfg.n_groups, true);
        nd.slope = 0.01f; nd.leaky = 1;
        if (h16 && i == 0) nd.in_scale_dev = c->scal_pair(0) + 1;  // conv0's output is in the scaled units of the tokens
        return nd;
    }
    GroupNormDesc layer_norm(int layer, int idx, float* y, float* y2, bool out16) const {  // y2: optional y + positional encoding
        GroupNormDesc nd = norm(norm_name(layer, idx), res, y, D, c->cfg.n_groups_module, out16);
        nd.y2 = y2; nd.pe = y2 ? pe : nullptr;
        return nd;
    }

    // ---- attention.  in_sp: q/k/v left the projection GEMM as split pairs
    AttnDesc attention(const float* q, const float* k, const float* v, bool in_sp) const {
        AttnDesc ad{};
        ad.q = q; ad.k = k; ad.v = v; ad.o = attn;
        ad.ldq = ad.ldk = ad.ldv = ad.ldo = D;
        ad.H = H; ad.DH = DH; ad.scale = scale;
        ad.in = h16 ? opfmt : stored(sp && in_sp); ad.out = opfmt; ad.split_math = sp ? 1 : 0;
        ad.guard = guard;
        return ad;
    }
    int launch(const AttnDesc& ad) const { return h16 ? launch_attention_f16(ad, s) : launch_attention(ad, s); }

    // ---- one sub-block: site a of `layer` over `rows` token rows whose units are g.  Projections (sites 0 and 1: q / k / v of xq / xk /
    // xv in one launch; site 2: q of xq, k / v of the text rows in a second) -> attention -> out-projection + resid -> norm into y (y2: y + PE).
    // Split-f16: q/k/v leave the projection GEMM already split when the attention that reads them runs the split-f16 MFMA shape.  Measured
    // (tools/attn_probe.py): with <= 64 keys per unit the exact-f32 MFMA kernel is as fast or faster (bound by latency and LDS traffic, not
    // by the matrix pipe); with 65..128 keys the split shape wins by 14 %.  Never the packed short-sequence shape (uniform: > 16 keys).
    // `tail`: the sequence's last sub-block, whose norm writes the f32 rows the score head reads (out16 = 0).  The last launch that can
    // set the guard word lies in it - split-f16: the attention (split-pair output; the out-projection writes f32 rows and carries no
    // guard pointer); 16-bit storage: the out-projection (f16 rows) - and the words are read back behind that launch (read_guard).
    int sub_block(int layer, int a, const SiteGeom& g, long long rows, const float* xq, const float* xk, const float* xv, const float* resid,
                  float* y, float* y2, bool out16, bool tail = false) const {
        SOLA_ARG(!tail || !out16, "forward: the tail sub-block's norm must write f32 rows (a 16-bit output could set the guard behind its read-back)");
        const bool in_sp = sp && g.k.len > g_attn_split_min_keys && (a == 2 || g.q.units || g.k.len > 16) && DH % 16 == 0;
        if (a < 2) {
            SOLA_TRY(linear3(xq, xk, xv, layer, a, 3, rows, q, k, v, 0, in_sp));
        } else {
            SOLA_TRY(linear3(xq, nullptr, nullptr, layer, a, 1, rows, q, nullptr, nullptr, 0, in_sp));
            SOLA_TRY(linear3(text, text, nullptr, layer, a, 2, text_rows, lk, lv, nullptr, 1, in_sp, lang_inv_scale()));
        }
        AttnDesc ad = attention(q, a < 2 ? k : lk, a < 2 ? v : lv, in_sp);
        site_fill_attn(ad, g);
        SOLA_TRY(launch(ad));
        if (tail && !h16) SOLA_TRY(read_guard());
        SOLA_TRY(out_proj(layer, a, rows, resid));
        if (tail && h16) SOLA_TRY(read_guard());
        GroupNormDesc nd = layer_norm(layer, a, y, y2, out16);
        site_fill_norm(nd, g.q);
        return launch_group_norm(nd, s);
    }
};

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// uniform batch: strided geometry on ONE [B,N,T',D] layout
// ---------------------------------------------------------------------------------------------------------------
int sola_forward_infer_impl(SolaCtx* c, const float* obj, const float* lang, int B, int N, int T, int L, float* score_map,
                            float* score_tokens, void* workspace, size_t ws_bytes, hipStream_t s) {
    SOLA_ARG(c && obj && lang && score_map && score_tokens && workspace, "forward: null argument");
    SOLA_ARG(B > 0 && N > 0 && T > 0 && L >= 1, "forward: bad sizes B=%d N=%d T=%d L=%d", B, N, T, L);
    InferBuilder b(c, s);
    SOLA_TRY(b.check_mode());
    const bool sp = b.sp;
    Plan p = make_plan(c, B, N, T, L, false);
    SOLA_TRY(sola_check_forward_args(c, "forward", p.total, workspace, ws_bytes));
    char* base = static_cast<char*>(workspace);
    // buffers are sized for 4 bytes per element; the 16-bit storage mode keeps its halfs in their first half
    auto buf = [&](const std::string& name) { return reinterpret_cast<float*>(base + p.bufs.at(name).off); };
    auto bytes = [&](const char* name) { return (size_t)p.bufs.at(name).rows * p.bufs.at(name).cols * sizeof(float); };
    const bool has_splitk = p.bufs.count("splitk") != 0;
    b.use_workspace(has_splitk ? buf("splitk") : nullptr, has_splitk ? bytes("splitk") : 0, buf("gn_slots"), bytes("gn_slots"), buf);
    const int D = b.D, H = b.H, DH = b.DH;
    const int Tp = p.Tp, M = p.M, Wn = p.W;
    const int R = B * N;

    SOLA_TRY(b.prepare_weights());
    if (!b.op16) {
        // exact f32 resets the kept-operand arena's record (sola_x16_arena_info sizes the 16-bit training arena by it); the 16-bit modes keep it
        c->x16.clear();
        c->x16_used = 0;
        c->x16_need = 0;
    }

    // ---- encoder (module/module.py:74-96,137-140)
    const float* x = obj;
    if (b.op16) {
        SOLA_TRY(b.cast_obj(obj, buf("obj_sp"), (long long)R * T));
        x = buf("obj_sp");
    }
    int t_in = T;
    for (int i = 0; i < 6; ++i) {
        const std::string is = std::to_string(i);
        // conv5 in the 16-bit modes: the layers' operand buffer
        GemmDesc gd = b.conv_gemm(i, x, (i == 5 && b.op16) ? buf("conv5_sp") : buf("conv" + is), (long long)R * p.Tl[i]);
        gd.T_in = t_in; gd.T_out = p.Tl[i];
        // split-f16, conv0-2 at GPU-filling batches: the norm behind the conv (64 channels per group, 16 / 8 / 4 tokens per instance)
        // is applied in the GEMM's epilogue and the activation written as split-f16 pairs directly (gemm_glds.hip, GNF)
        bool fused_norm = false;
        if (sp && i < 5) {
            GemmDesc probe = gd;
            probe.c = Elem::SP16;
            if (gemm_gn_fusable(probe, c->conv[i].cout / c->cfg.n_groups, p.Tl[i])) {
                const std::string np = enc_name(kNormIdx[i]);
                gd.c = Elem::SP16;
                gd.p[0].C = buf("act" + is);
                gd.gn_gamma = b.W(np + ".weight"); gd.gn_beta = b.W(np + ".bias");
                gd.gn_tokens = p.Tl[i]; gd.gn_eps = 1e-5f; gd.gn_slope = 0.01f;
                fused_norm = true;
            }
        }
        SOLA_TRY(b.launch_conv(i, gd));
        if (i < 5 && !fused_norm) {
            GroupNormDesc nd = b.encoder_norm(i, buf("conv" + is), buf("act" + is));
            site_fill_norm(nd, site_tracks(R, p.Tl[i]));
            SOLA_TRY(launch_group_norm(nd, s));
        }
        if (i < 5) x = buf("act" + is);
        t_in = p.Tl[i];
    }

    // ---- positional table; text tokens ++ negative tokens and their mean (module/module.py:143-147)
    SOLA_TRY(launch_pos_encoding(b.W("positional_encoding_gaussian_matrix"), D, Tp, c->cfg.max_temporal_length, buf("pe"), s));
    // round 5, split-f16 (sola_tune "lang_shared_neg", default 1): the negative tokens' key / value rows are the same for every sample -
    // project them once (B * L + n_neg rows through the two text-side GEMMs of a layer instead of B * (L + n_neg)) and let the object ->
    // language attention read the shared rows behind each sample's L own ones.  Same products per row, same bits - from 1024 text rows on:
    // below that the projection's 64x64 kernel splits K by the size of its grid, and the two forms would sum in different orders (nothing to
    // gain there).
    bool shared_neg = false;
    if (sp && g_lang_shared_neg && c->cfg.n_negative > 0 && Wn <= g_attn_split_min_keys && (long long)B * L + c->cfg.n_negative >= 1024) {
        AttnDesc probe{};
        probe.G = B; probe.H = H; probe.DH = DH; probe.Sq = N * Tp; probe.Sk = Wn; probe.inner = 1; probe.k_private = L;
        shared_neg = attention_shared_keys_supported(probe);
    }
    const long long lang_rows = shared_neg ? (long long)B * L + c->cfg.n_negative : (long long)B * Wn;
    if (shared_neg) SOLA_TRY(launch_lang_concat_shared(lang, b.W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s));
    else SOLA_TRY(launch_lang_concat(lang, b.W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s));
    const float* lang_in = buf("lang");
    if (b.op16) {
        SOLA_TRY(b.cast_lang(buf("lang"), buf("lang_sp"), lang_rows));
        lang_in = buf("lang_sp");
    }

    b.use_text(lang_in, lang_rows);
    // ---- alignment layers (module/module.py:22-52)
    const SiteShape shape = site_shape_uniform(B, N, Tp, Wn, shared_neg ? L : 0);
    const float* xin = b.op16 ? buf("conv5_sp") : buf("conv5");  // A operand of the layer and residual of its first sub-block
    for (int l = 0; l < c->cfg.n_layers; ++l) {
        const std::string ls = "l" + std::to_string(l);
        const bool last = l + 1 == c->cfg.n_layers;
        float* x_obj = buf(ls + "_obj");
        float* x_pe = buf(ls + "_xpe");
        float* x_mot = buf(ls + "_motion");
        float* x_o2l = buf(ls + "_o2l");
        // (i) inter-object attention over the N tracks of each (b, t'): module.py:31-35
        SOLA_TRY(b.sub_block(l, 0, site_geom(shape, 0), M, xin, xin, xin, xin, x_obj, x_pe, 1));
        // (ii) motion attention over T' per track, PE on q and k only: module.py:38-43
        SOLA_TRY(b.sub_block(l, 1, site_geom(shape, 1), M, x_pe, x_pe, x_obj, x_obj, x_mot, nullptr, 1));
        // (iii) object -> language cross attention: module.py:46-50 (the score head reads f32)
        SOLA_TRY(b.sub_block(l, 2, site_geom(shape, 2), M, x_mot, nullptr, nullptr, x_mot, x_o2l, nullptr, last ? 0 : 1, last));
        xin = x_o2l;
    }

    // ---- score head (module/module.py:152-160)
    HeadDesc hd{xin, buf("lbar"), score_map, score_tokens};
    hd.D = D;
    site_fill_head(hd, shape);
    SOLA_TRY(launch_score_head(hd, s));
    c->last = p;
    c->last_obj = nullptr;
    return SOLA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// ragged batch (sola_forward_ragged): many (video, expression) samples of DIFFERENT shapes in one pass.
//
// The reference scores one sample per call (configs/mevis/default.yaml:37,42,47 batch_size 1; inference.py:44-58,
// evaluator.py:88-112): per-sample N tracks, T frames, L text tokens.  At one sample per launch the GPU runs 0.5-1.3 ms
// per call at a few percent of its rate; here the token rows of all samples are concatenated, the dense contractions run
// as ONE GEMM over all rows, and everything whose extent depends on the sample (conv windows along T, GroupNorm statistics,
// the three attentions, the score head) takes per-unit descriptors built on the device from the (N, T, L) arrays (ragged.hip) -
// no padding, so no statistic or softmax ever sees a token that is not the sample's own.
//
// Two levels:
//   videos  (object sets): N_v tracks x T_v frames of object tokens;
//   samples (video, expression): index of a video + L_i text tokens.
// Everything that does not depend on the text is computed once per VIDEO and shared by its expressions
// (inference.py:44-58 re-runs it per expression): the motion encoder and layer 0's inter-object and motion sub-blocks,
// 9.3 of the 16.4 GFLOP per sample at the headline shape.  The text enters at layer 0's object->language attention
// (module/module.py:46-50); from there on the rows are per sample (a row gather repeats the video's activations).
// ---------------------------------------------------------------------------------------------------------------
namespace {

struct RagPlan {
    std::unordered_map<std::string, size_t> off;
    size_t total = 0;
    size_t add(const std::string& name, size_t bytes) {
        const size_t o = total;
        off[name] = o;
        total += (bytes + 255) & ~(size_t)255;
        return o;
    }
};
constexpr size_t kRagSplitkBytes = (size_t)8192 * 4096 * sizeof(float);

RagPlan rag_plan(const SolaCtx* c, const RagShape& r, int precision) {  // `precision`: the arithmetic the plan is sized for (the ctx's, or 0 for the guard's exact-f32 repeat)
    RagPlan p;
    const size_t D = c->cfg.lang_token_dim, f = sizeof(float);
    const bool sp = precision >= 1;  // split-f16 or plain-f16 copies of the caller's tensors
    p.add("tables", rag_tables_bytes(r, false));
    for (int i = 0; i < 6; ++i) {
        p.add("conv" + std::to_string(i), (size_t)r.rows[i + 1] * c->conv[i].cout * f);
        if (i < 5) p.add("act" + std::to_string(i), (size_t)r.rows[i + 1] * c->conv[i].cout * f);
    }
    if (sp) p.add("obj_sp", (size_t)r.rows[0] * c->cfg.object_token_dim * f);
    const size_t Mmax = (size_t)std::max(r.Mv, r.Ms);
    if (Mmax <= 8192) p.add("splitk", kRagSplitkBytes);
    p.add("pe", (size_t)r.maxT[6] * D * f);
    p.add("gn_slots", rag_gn_slots_bytes(r));  // sliced GroupNorm shape: 8 B per (unit, slice)
    p.add("lang", (size_t)r.LW * D * f);
    if (sp) p.add("lang_sp", (size_t)r.LW * D * f);
    p.add("lbar", (size_t)r.S * D * f);
    p.add("lk", (size_t)r.LW * D * f);
    p.add("lv", (size_t)r.LW * D * f);
    for (const char* nm : {"q", "k", "v", "attn", "res"}) p.add(nm, Mmax * D * f);
    p.add("v_obj", (size_t)r.Mv * D * f);
    p.add("v_xpe", (size_t)r.Mv * D * f);
    p.add("v_motion", (size_t)r.Mv * D * f);
    if (!r.identity) p.add("s_motion0", (size_t)r.Ms * D * f);
    p.add("s0_o2l", (size_t)r.Ms * D * f);
    for (int l = 1; l < c->cfg.n_layers; ++l) {
        const std::string ls = "s" + std::to_string(l);
        p.add(ls + "_obj", (size_t)r.Ms * D * f);
        p.add(ls + "_xpe", (size_t)r.Ms * D * f);
        p.add(ls + "_motion", (size_t)r.Ms * D * f);
        p.add(ls + "_o2l", (size_t)r.Ms * D * f);
    }
    return p;
}

}  // namespace

size_t sola_ragged_workspace_bytes_impl(const SolaCtx* c, const SolaRaggedBatch* b, int precision) {
    RagShape r;
    if (!c || rag_shape(c, b, r) != SOLA_OK) return 0;
    return rag_plan(c, r, precision).total;
}

int sola_forward_ragged_impl(SolaCtx* c, const float* obj, const float* lang, const SolaRaggedBatch* batch, float* score_map,
                             float* score_tokens, void* workspace, size_t ws_bytes, hipStream_t s) {
    SOLA_ARG(c && obj && lang && batch && score_map && score_tokens && workspace, "forward_ragged: null argument");
    InferBuilder b(c, s);
    SOLA_TRY(b.check_mode());
    RagShape r;
    SOLA_TRY(rag_shape(c, batch, r));
    const RagPlan p = rag_plan(c, r, c->precision);
    SOLA_TRY(sola_check_forward_args(c, "forward_ragged", p.total, workspace, ws_bytes));
    char* base = static_cast<char*>(workspace);
    auto raw = [&](const std::string& name) { return base + p.off.at(name); };
    auto buf = [&](const std::string& name) { return reinterpret_cast<float*>(raw(name)); };
    b.use_workspace(p.off.count("splitk") ? buf("splitk") : nullptr, kRagSplitkBytes, raw("gn_slots"), rag_gn_slots_bytes(r), buf);
    const int D = b.D, S = r.S;

    // ---- descriptors -> device, unit tables
    RagTables rt;
    SOLA_TRY(rag_build_tables(c, r, raw("tables"), false, &rt, s));

    SOLA_TRY(b.prepare_weights());

    // ---- encoder over the videos' tracks (module/module.py:74-96,137-140)
    const float* x = obj;
    if (b.op16) {
        SOLA_TRY(b.cast_obj(obj, buf("obj_sp"), r.rows[0]));
        x = buf("obj_sp");
    }
    for (int i = 0; i < 6; ++i) {
        const std::string is = std::to_string(i);
        // conv5 is written in the mode's operand format into its own buffer
        GemmDesc gd = b.conv_gemm(i, x, buf("conv" + is), r.rows[i + 1]);
        gd.T_in = 1; gd.T_out = 1;
        if (gd.conv) gd.rowmap = rt.rowmap[i];
        SOLA_TRY(launch_gemm(gd, s));
        if (i < 5) {
            GroupNormDesc nd = b.encoder_norm(i, buf("conv" + is), buf("act" + is));
            site_fill_norm(nd, site_tracks(rt, i + 1));
            SOLA_TRY(launch_group_norm(nd, s));
            x = buf("act" + is);
        }
    }
    const int maxTp = r.maxT[6];
    SOLA_TRY(launch_pos_encoding(b.W("positional_encoding_gaussian_matrix"), D, maxTp, c->cfg.max_temporal_length, buf("pe"), s));
    SOLA_TRY(launch_lang_concat_ragged(lang, b.W("negative_token.weight"), buf("lang"), buf("lbar"), S, rt.u_lang, c->cfg.n_negative, D, s));
    const float* lang_in = buf("lang");
    if (b.op16) {
        SOLA_TRY(b.cast_lang(buf("lang"), buf("lang_sp"), r.LW));
        lang_in = buf("lang_sp");
    }

    b.use_text(lang_in, r.LW);
    const SiteShape videos = site_shape_videos(rt), samples = site_shape_samples(rt);

    // ---- layer 0, text-independent half, once per VIDEO (module/module.py:31-43)
    const float* xin = buf("conv5");
    SOLA_TRY(b.sub_block(0, 0, site_geom(videos, 0), r.Mv, xin, xin, xin, xin, buf("v_obj"), buf("v_xpe"), 1));
    SOLA_TRY(b.sub_block(0, 1, site_geom(videos, 1), r.Mv, buf("v_xpe"), buf("v_xpe"), buf("v_obj"), buf("v_obj"), buf("v_motion"), nullptr, 1));
    // ---- from here on rows are per SAMPLE: repeat the video's activations for each of its expressions
    const float* x_mot = buf("v_motion");
    if (!r.identity) {
        SOLA_TRY(launch_gather_rows(buf("v_motion"), buf("s_motion0"), rt.u_gather, S, b.h16 ? D / 2 : D, r.Ms, s));  // f16 rows: D halfs
        x_mot = buf("s_motion0");
    }
    const long long M = r.Ms;
    for (int l = 0; l < c->cfg.n_layers; ++l) {
        const std::string ls = "s" + std::to_string(l);
        const bool last = l + 1 == c->cfg.n_layers;
        if (l > 0) {
            float* x_obj = buf(ls + "_obj");
            float* x_pe = buf(ls + "_xpe");
            SOLA_TRY(b.sub_block(l, 0, site_geom(samples, 0), M, xin, xin, xin, xin, x_obj, x_pe, 1));
            SOLA_TRY(b.sub_block(l, 1, site_geom(samples, 1), M, x_pe, x_pe, x_obj, x_obj, buf(ls + "_motion"), nullptr, 1));
            x_mot = buf(ls + "_motion");
        }
        // object -> language attention (module/module.py:46-50; the score head reads f32)
        float* x_o2l = buf(ls + "_o2l");
        SOLA_TRY(b.sub_block(l, 2, site_geom(samples, 2), M, x_mot, nullptr, nullptr, x_mot, x_o2l, nullptr, last ? 0 : 1, last));
        xin = x_o2l;
    }
    HeadDesc hd{xin, buf("lbar"), score_map, score_tokens};
    hd.D = D;
    site_fill_head(hd, samples);
    SOLA_TRY(launch_score_head(hd, s));
    return SOLA_OK;
}
