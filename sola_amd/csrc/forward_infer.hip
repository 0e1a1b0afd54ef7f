// Inference forward of a uniform batch (sola_forward) in all three inference precisions (sola_set_precision(ctx, 0 / 1 / 2)).
// Same network, same kernels and the same single [B,N,T',D] layout as the training forward (forward.hip) without what only
// its backward reads; the modes differ in the arithmetic of the dense contractions (98 % of the FLOPs) and in the storage.
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

#include "ctx.h"

// Split-f16 copies of the 12 * n_layers projection weights, each with its own power-of-two scale (max|w| -> [2^13, 2^14),
// found on the device: a trained matrix may be far from the U(-1/32, 1/32) of the default init, and a few outliers must not
// push the rest into f16 subnormals - the pair format keeps 22 bits for everything within 2^-16 of the largest entry), plus
// the weight-time range check of the activations the GroupNorms will emit (kernels.h: launch_norm_range_check).
int sola_refresh_lin16(SolaCtx* c, hipStream_t s) {
    if (!c->lin16_dirty) return SOLA_OK;
    SOLA_ARG(c->lin16_buf && c->scal_buf, "split-f16 weights requested before sola_set_precision(ctx, 1)");
    static const char* pn[4] = {"q_proj", "k_proj", "v_proj", "out_proj"};
    const int D = c->cfg.lang_token_dim;
    std::vector<const float*> in;
    std::vector<float*> out;
    for (int l = 0; l < c->cfg.n_layers; ++l)
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 4; ++j) {
                const std::string nm = "object_lang_align_layers." + std::to_string(l) + "." + kAttnLong[a] + "." + pn[j] + ".weight";
                const float* w = ctx_weight(c, nm);
                if (!w) {
                    sola_set_error("forward: weight '%s' has not been set", nm.c_str());
                    return SOLA_ERR_WEIGHT;
                }
                in.push_back(w);
                out.push_back(c->lin16_buf + ((size_t)(l * 3 + a) * 4 + j) * D * D);
            }
    if (c->precision >= 2) {  // 16-bit storage mode / 16-bit GEMM operands: plain f16 (precision 3: bfloat16) copies, same per-matrix
        std::vector<void*> outh;  // scales, packed in the first half of the buffer
        for (size_t i = 0; i < out.size(); ++i) outh.push_back(reinterpret_cast<_Float16*>(c->lin16_buf) + i * (size_t)D * D);
        SOLA_TRY(launch_cast_f16_auto_multi(in.data(), outh.data(), (int)in.size(), D, D, c->scal_pair(2), s, c->precision == 3 ? 1 : 0));
    } else {
        SOLA_TRY(launch_cast_sp16_auto_multi(in.data(), out.data(), (int)in.size(), D, D, c->scal_pair(2), s));
    }
    std::vector<NormPair> norms;
    for (int i = 0; i < 5; ++i) {
        const std::string np = "short_motion_encoder." + std::to_string(kNormIdx[i]);
        norms.push_back(NormPair{ctx_weight(c, np + ".weight"), ctx_weight(c, np + ".bias"), c->conv[i].cout});
    }
    for (int l = 0; l < c->cfg.n_layers; ++l)
        for (int j = 0; j < 3; ++j) {
            const std::string np = "object_lang_align_layers." + std::to_string(l) + ".norm." + std::to_string(j);
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
// (the SolaCtx::ws16_fmt codes: 0 = none, 1 = split-f16 pairs, 2 = f16, 3 = bf16).  Runs when the weights changed, on every
// forward under the reference's policy (ws_every_forward), when ws16_buf holds another format, and always with `force` (the
// training forward).  Standardised rows are unit-variance by construction: the casts take the fixed scale 1.
int sola_refresh_conv_weights(SolaCtx* c, int fmt, bool force, hipStream_t s) {
    if (!force && !c->ws_dirty && !c->ws_every_forward && (fmt == 0 || c->ws16_fmt == fmt)) return SOLA_OK;
    WsLayer layers[6];
    for (int i = 0; i < 6; ++i) {
        const std::string nm = "short_motion_encoder." + std::to_string(kConvIdx[i]) + ".weight";
        layers[i] = WsLayer{ctx_weight(c, nm), c->ws_buf + c->ws_off[i], c->conv[i].cout, c->conv[i].cin, c->conv[i].k};
    }
    SOLA_TRY(launch_ws_standardize(layers, 6, s));
    c->ws16_fmt = 0;  // ws_buf is new: ws16_buf is current once the casts below have rewritten it
    for (int i = 0; i < 6 && fmt != 0; ++i) {
        const int kc = c->conv[i].k * c->conv[i].cin;
        const float* w = c->ws_buf + c->ws_off[i];
        if (fmt == 1) SOLA_TRY(launch_cast_sp16(w, kc, c->ws16_buf + c->ws_off[i], kc, c->conv[i].cout, kc, 1.f, s));
        else SOLA_TRY(launch_cast_f16(w, kc, reinterpret_cast<_Float16*>(c->ws16_buf) + c->ws_off[i], kc, c->conv[i].cout, kc, 1.f, nullptr, s, 13,
                                      nullptr, fmt == 3 ? 1 : 0));
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

int launch_attention_f16(const AttnDesc& d, hipStream_t s);

int sola_forward_infer_impl(SolaCtx* c, const float* obj, const float* lang, int B, int N, int T, int L, float* score_map,
                            float* score_tokens, void* workspace, size_t ws_bytes, hipStream_t s) {
    SOLA_ARG(c && obj && lang && score_map && score_tokens && workspace, "forward: null argument");
    SOLA_ARG(B > 0 && N > 0 && T > 0 && L >= 1, "forward: bad sizes B=%d N=%d T=%d L=%d", B, N, T, L);
    const bool sp = c->precision == 1;   // split-f16 operands
    const bool h16 = c->precision == 2;  // 16-bit storage
    if (sp)
        SOLA_ARG(c->cfg.object_token_dim % 8 == 0 && (c->cfg.lang_token_dim / c->cfg.n_groups_module) % 8 == 0 &&
                     (2 * c->cfg.object_token_dim / c->cfg.n_groups) % 8 == 0 && (c->cfg.lang_token_dim / c->cfg.n_groups) % 8 == 0,
                 "split-f16 mode needs channel counts per GroupNorm group that are multiples of 8");
    if (h16)
        SOLA_ARG(c->cfg.object_token_dim % 64 == 0 && c->cfg.lang_token_dim % 64 == 0,
                 "16-bit storage mode needs object_token_dim and lang_token_dim to be multiples of 64");
    Plan p = make_plan(c, B, N, T, L, false);
    SOLA_TRY(sola_check_forward_args(c, "forward", p.total, workspace, ws_bytes));
    char* base = static_cast<char*>(workspace);
    // buffers are sized for 4 bytes per element; the 16-bit storage mode keeps its halfs in their first half
    auto buf = [&](const std::string& name) { return reinterpret_cast<float*>(base + p.bufs.at(name).off); };
    float* const splitk_ws = (!h16 && p.bufs.count("splitk")) ? buf("splitk") : nullptr;  // the 16-bit GEMMs never split K
    const size_t splitk_bytes = splitk_ws ? (size_t)p.bufs.at("splitk").rows * p.bufs.at("splitk").cols * sizeof(float) : 0;
    auto W = [&](const std::string& name) { return ctx_weight(c, name); };
    const int D = c->cfg.lang_token_dim, H = c->cfg.num_heads, DH = D / H, d_in = c->cfg.object_token_dim;
    const int Tp = p.Tp, M = p.M, Wn = p.W;
    const int R = B * N;
    int* const guard = (sp || h16) ? c->guard : nullptr;
    // the weights in the mode's operand format: f32 as set, split-f16 pairs (D*D floats per matrix) or plain f16 (D*D halfs)
    auto ws_w = [&](int i) -> const float* {
        if (h16) return reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(c->ws16_buf) + c->ws_off[i]);
        return sp ? c->ws16_buf + c->ws_off[i] : c->ws_buf + c->ws_off[i];
    };
    auto lin_w = [&](const std::string& an, const char* proj_name, int layer, int attn, int proj) -> const float* {
        const size_t idx = (size_t)(layer * 3 + attn) * 4 + proj;
        if (sp) return c->lin16_buf + idx * D * D;
        if (h16) return reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(c->lin16_buf) + idx * D * D);
        return W(an + "." + proj_name + ".weight");
    };
    auto lin_inv = [&](int layer, int attn, int proj) -> const float* { return (sp || h16) ? c->lin_inv_scale(layer, attn, proj) : nullptr; };

    // ---- weights.  The projection weights are used as they are by the reference (no per-forward transform), so their 16-bit
    // copies are refreshed only when a weight pointer or value changed (sola_set_weight / sola_weights_changed).
    SOLA_TRY(sola_refresh_conv_weights(c, sp ? 1 : (h16 ? 2 : 0), false, s));
    if (sp || h16) {
        SOLA_TRY(sola_refresh_lin16(c, s));
        SOLA_HIP(hipMemsetAsync(c->guard, 0, sizeof(int), s));  // per-call range guard word (ctx.h)
    } else {
        // exact f32 resets the kept-operand arena's record (sola_x16_arena_info sizes the 16-bit training arena by it); the 16-bit modes keep it
        c->x16.clear();
        c->x16_used = 0;
        c->x16_need = 0;
    }

    // ---- encoder (module/module.py:74-96,137-140)
    // The caller's tokens come with an unknown magnitude (SAM2 memory-attention features here, anything elsewhere).  Split-f16:
    // their largest entry is mapped into [2^13, 2^14) by a power of two found on the device and conv0's epilogue undoes it.
    // 16-bit storage: largest magnitude -> [2^6, 2^7), and conv0's output STAYS in those scaled units (its standardised weights
    // have a gain of sqrt(k*cin) = 28: tokens at 1e3 would leave the f16 range if the scale were undone here, tokens at 1e-5 would
    // sink into subnormals): the bias is multiplied by the scale in conv0's epilogue and the first GroupNorm multiplies by the
    // inverse while it reads, so its statistics (and eps) see the true values.  The scale is capped at 2^8: conv0's bias rides
    // along multiplied by it (tokens of 1e-5 would ask for 2^21 and carry a bias of 0.03 to 75 000); below the cap the smallest
    // token entries lose some of their 11 bits to f16 subnormals.
    const float* x = obj;
    if (sp) SOLA_TRY(launch_cast_sp16_auto(obj, d_in, buf("obj_sp"), d_in, (long long)R * T, d_in, c->scal_pair(0), s));
    if (h16) SOLA_TRY(launch_cast_f16(obj, d_in, buf("obj_sp"), d_in, (long long)R * T, d_in, 256.f, c->scal_pair(0), s, 6, c->scal_extra(0)));
    if (sp || h16) x = buf("obj_sp");
    // conv5 (no norm behind it) feeds layer 0 both as the projections' A operand and as the first residual: in the 16-bit modes its
    // epilogue writes the operand format directly, no f32 copy and no cast pass (split pairs need cout % 8 == 0)
    const bool conv5_16 = h16 || (sp && c->conv[5].cout % 8 == 0);
    int t_in = T;
    for (int i = 0; i < 6; ++i) {
        const ConvGeom& g = c->conv[i];
        const std::string cp = "short_motion_encoder." + std::to_string(kConvIdx[i]);
        const bool to16 = i == 5 && conv5_16;
        GemmDesc gd{};
        gd.nprob = 1;
        gd.p[0] = GemmProblem{x, ws_w(i), W(cp + ".bias"), nullptr, to16 ? buf("conv5_sp") : buf("conv" + std::to_string(i))};
        gd.M = R * p.Tl[i]; gd.N = g.cout; gd.K = g.k * g.cin;
        gd.lda = g.cin; gd.ldr = 0; gd.ldc = g.cout;
        gd.conv = g.k > 1 ? 1 : 0;
        gd.T_in = t_in; gd.T_out = p.Tl[i]; gd.stride = g.stride; gd.pad = g.pad; gd.Cin = g.cin;
        if (sp) {
            gd.arith = 1; gd.out_scale = 1.f; gd.c_sp16 = to16 ? 1 : 0; gd.guard = guard;
            if (i == 0) gd.out_scale_dev = c->scal_pair(0) + 1;
        }
        if (h16) {
            gd.arith = 2; gd.out_scale = 1.f; gd.c_f16 = 1; gd.guard = guard;
            if (i == 0) gd.bias_scale_dev = c->scal_extra(0);
        }
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        // split-f16, conv0-2 at GPU-filling batches: the norm behind the conv (64 channels per group, 16 / 8 / 4 tokens per instance)
        // is applied in the GEMM's epilogue and the activation written as split-f16 pairs directly (gemm_glds.hip, GNF)
        bool fused_norm = false;
        if (sp && i < 5) {
            GemmDesc probe = gd;
            probe.c_sp16 = 1;
            if (gemm_gn_fusable(probe, g.cout / c->cfg.n_groups, p.Tl[i])) {
                const std::string np = "short_motion_encoder." + std::to_string(kNormIdx[i]);
                gd.c_sp16 = 1;
                gd.p[0].C = buf("act" + std::to_string(i));
                gd.gn_gamma = W(np + ".weight"); gd.gn_beta = W(np + ".bias");
                gd.gn_tokens = p.Tl[i]; gd.gn_eps = 1e-5f; gd.gn_slope = 0.01f;
                fused_norm = true;
            }
        }
        SOLA_TRY(launch_gemm(gd, s));
        if (i < 5 && !fused_norm) {
            const std::string np = "short_motion_encoder." + std::to_string(kNormIdx[i]);
            GroupNormDesc nd{};
            nd.slice_ws = buf("gn_slots"); nd.slice_ws_bytes = (size_t)p.bufs.at("gn_slots").rows * p.bufs.at("gn_slots").cols * sizeof(float);
            nd.x = buf("conv" + std::to_string(i)); nd.y = buf("act" + std::to_string(i));
            nd.gamma = W(np + ".weight"); nd.beta = W(np + ".bias");
            nd.n_inst = R; nd.inner = 1; nd.outer_stride = p.Tl[i]; nd.inner_stride = 0; nd.tok_stride = 1;
            nd.ntok = p.Tl[i]; nd.C = g.cout; nd.groups = c->cfg.n_groups; nd.eps = 1e-5f; nd.slope = 0.01f; nd.leaky = 1;
            nd.out_sp16 = sp ? 1 : 0; nd.guard = guard;
            if (h16) {
                nd.in_f16 = 1; nd.out_f16 = 1;
                if (i == 0) nd.in_scale_dev = c->scal_pair(0) + 1;
            }
            SOLA_TRY(launch_group_norm(nd, s));
        }
        if (i < 5) x = buf("act" + std::to_string(i));
        t_in = p.Tl[i];
    }
    if (sp && !conv5_16) SOLA_TRY(launch_cast_sp16(buf("conv5"), D, buf("conv5_sp"), D, M, D, 1.f, s));

    // ---- positional table; text tokens ++ negative tokens and their mean (module/module.py:143-147)
    SOLA_TRY(launch_pos_encoding(W("positional_encoding_gaussian_matrix"), D, Tp, c->cfg.max_temporal_length, buf("pe"), s));
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
    if (shared_neg) SOLA_TRY(launch_lang_concat_shared(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s));
    else SOLA_TRY(launch_lang_concat(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s));
    if (sp) SOLA_TRY(launch_cast_sp16_auto(buf("lang"), D, buf("lang_sp"), D, lang_rows, D, c->scal_pair(1), s));
    if (h16) SOLA_TRY(launch_cast_f16(buf("lang"), D, buf("lang_sp"), D, lang_rows, D, 1.f, c->scal_pair(1), s, 6));
    const float* const lang_in = (sp || h16) ? buf("lang_sp") : buf("lang");

    // ---- alignment layers (module/module.py:22-52)
    const float scale = 1.0f / sqrtf((float)DH);
    // out16: split-f16 q/k/v for the split attention kernel (the 16-bit storage mode writes f16 always, f32 ignores it)
    auto linear3 = [&](const float* a0, const float* a1, const float* a2, int layer, int attn, int nprob, int rows, float* o0,
                       float* o1, float* o2, int first_proj, int out_sp16, const float* a_inv_scale = nullptr) -> int {
        static const char* pn[3] = {"q_proj", "k_proj", "v_proj"};
        const std::string an = "object_lang_align_layers." + std::to_string(layer) + "." + kAttnLong[attn];
        const float* as[3] = {a0, a1, a2};
        float* os[3] = {o0, o1, o2};
        GemmDesc gd{};
        gd.nprob = nprob;
        for (int j = 0; j < nprob; ++j)
            gd.p[j] = GemmProblem{as[j], lin_w(an, pn[first_proj + j], layer, attn, first_proj + j), W(an + "." + pn[first_proj + j] + ".bias"),
                                  nullptr, os[j], lin_inv(layer, attn, first_proj + j)};
        gd.M = rows; gd.N = D; gd.K = D; gd.lda = D; gd.ldr = 0; gd.ldc = D;
        if (sp) { gd.arith = 1; gd.out_scale = 1.f; gd.out_scale_dev = a_inv_scale; gd.c_sp16 = out_sp16; gd.guard = guard; }
        if (h16) { gd.arith = 2; gd.out_scale = 1.f; gd.out_scale_dev = a_inv_scale; gd.c_f16 = 1; gd.guard = guard; }
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        return launch_gemm(gd, s);
    };
    auto out_proj = [&](int layer, int attn, const float* resid, int resid_sp16) -> int {
        const std::string an = "object_lang_align_layers." + std::to_string(layer) + "." + kAttnLong[attn];
        GemmDesc gd{};
        gd.nprob = 1;
        gd.p[0] = GemmProblem{buf("attn"), lin_w(an, "out_proj", layer, attn, 3), W(an + ".out_proj.bias"), resid, buf("res"), lin_inv(layer, attn, 3)};
        gd.M = M; gd.N = D; gd.K = D; gd.lda = D; gd.ldr = D; gd.ldc = D;
        if (sp) { gd.arith = 1; gd.out_scale = 1.f; gd.r_sp16 = resid_sp16; }
        if (h16) { gd.arith = 2; gd.out_scale = 1.f; gd.r_f16 = 1; gd.c_f16 = 1; gd.guard = guard; }
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        return launch_gemm(gd, s);
    };
    // out16: y / y2 in the mode's 16-bit storage (split pairs or f16); f32 ignores it
    auto gn = [&](const std::string& lp, int idx, float* y, float* y2, int out16, int n_inst, int inner, long long outer,
                  long long inner_stride, long long tok_stride, int ntok) -> int {
        GroupNormDesc nd{};
        nd.slice_ws = buf("gn_slots"); nd.slice_ws_bytes = (size_t)p.bufs.at("gn_slots").rows * p.bufs.at("gn_slots").cols * sizeof(float);
        nd.x = buf("res"); nd.y = y; nd.y2 = y2; nd.pe = y2 ? buf("pe") : nullptr;
        nd.gamma = W(lp + "norm." + std::to_string(idx) + ".weight");
        nd.beta = W(lp + "norm." + std::to_string(idx) + ".bias");
        nd.n_inst = n_inst; nd.inner = inner; nd.outer_stride = outer; nd.inner_stride = inner_stride;
        nd.tok_stride = tok_stride; nd.ntok = ntok; nd.C = D; nd.groups = c->cfg.n_groups_module;
        nd.eps = 1e-5f; nd.slope = 0.f; nd.leaky = 0; nd.guard = guard;
        if (sp) nd.out_sp16 = out16;
        if (h16) { nd.in_f16 = 1; nd.out_f16 = out16; }
        return launch_group_norm(nd, s);
    };
    auto attention = [&](const float* q, const float* k, const float* v, int G, int Sq, int Sk, int inner, long long qo,
                         long long qi, long long qr, long long ko, long long ki, long long kr, int in_sp16, int k_private = 0,
                         long long k_shared_row = 0) -> int {
        AttnDesc ad{q, k, v, buf("attn"), D, D, D, D, G, H, DH, Sq, Sk, inner, qo, qi, qr, ko, ki, kr, scale, nullptr};
        ad.k_private = k_private;
        ad.k_shared_row = k_shared_row;
        ad.o_sp16 = sp ? 1 : 0;
        ad.in_sp16 = in_sp16;
        ad.guard = guard;
        ad.split_math = sp ? 1 : 0;
        return h16 ? launch_attention_f16(ad, s) : launch_attention(ad, s);
    };
    // split-f16: q/k/v leave the projection GEMM already split when the attention that reads them runs the split-f16 MFMA shape.
    // Measured (tools/attn_probe.py): with <= 64 keys per unit the exact-f32 MFMA kernel is as fast or faster (the kernel is then
    // bound by latency and LDS traffic, not by the matrix pipe); with 65..128 keys the split shape wins by 14 %.
    const int obj_sp = (sp && N > g_attn_split_min_keys && N > 16 && DH % 16 == 0) ? 1 : 0;
    const int mot_sp = (sp && Tp > g_attn_split_min_keys && Tp > 16 && DH % 16 == 0) ? 1 : 0;
    const int o2l_sp = (sp && Wn > g_attn_split_min_keys && DH % 16 == 0) ? 1 : 0;

    const float* xin = (sp || h16) ? buf("conv5_sp") : buf("conv5");  // A operand of the layer
    const float* xres = conv5_16 ? buf("conv5_sp") : buf("conv5");     // residual of the first sub-block
    int xres_sp = conv5_16 ? 1 : 0;
    for (int l = 0; l < c->cfg.n_layers; ++l) {
        const std::string lp = "object_lang_align_layers." + std::to_string(l) + ".";
        const std::string ls = "l" + std::to_string(l);
        const bool last = l + 1 == c->cfg.n_layers;
        float *q = buf("q"), *k = buf("k"), *v = buf("v");
        float* x_obj = buf(ls + "_obj");
        float* x_pe = buf(ls + "_xpe");
        float* x_mot = buf(ls + "_motion");
        float* x_o2l = buf(ls + "_o2l");
        // (i) inter-object attention over the N tracks of each (b, t'): module.py:31-35
        SOLA_TRY(linear3(xin, xin, xin, l, 0, 3, M, q, k, v, 0, obj_sp));
        SOLA_TRY(attention(q, k, v, B * Tp, N, N, Tp, (long long)N * Tp, 1, Tp, (long long)N * Tp, 1, Tp, obj_sp));
        SOLA_TRY(out_proj(l, 0, xres, xres_sp));
        SOLA_TRY(gn(lp, 0, x_obj, x_pe, 1, B * Tp, Tp, (long long)N * Tp, 1, Tp, N));
        // (ii) motion attention over T' per track, PE on q and k only: module.py:38-43
        SOLA_TRY(linear3(x_pe, x_pe, x_obj, l, 1, 3, M, q, k, v, 0, mot_sp));
        SOLA_TRY(attention(q, k, v, B * N, Tp, Tp, 1, (long long)Tp, 0, 1, (long long)Tp, 0, 1, mot_sp));
        SOLA_TRY(out_proj(l, 1, x_obj, 1));
        SOLA_TRY(gn(lp, 1, x_mot, nullptr, 1, B * N, 1, Tp, 0, 1, Tp));
        // (iii) object -> language cross attention: module.py:46-50
        SOLA_TRY(linear3(x_mot, nullptr, nullptr, l, 2, 1, M, q, nullptr, nullptr, 0, o2l_sp));
        SOLA_TRY(linear3(lang_in, lang_in, nullptr, l, 2, 2, (int)lang_rows, buf("lk"), buf("lv"), nullptr, 1, o2l_sp, c->scal_pair(1) + 1));
        if (shared_neg) SOLA_TRY(attention(q, buf("lk"), buf("lv"), B, N * Tp, Wn, 1, (long long)N * Tp, 0, 1, (long long)L, 0, 1, o2l_sp, L, (long long)B * L));
        else SOLA_TRY(attention(q, buf("lk"), buf("lv"), B, N * Tp, Wn, 1, (long long)N * Tp, 0, 1, (long long)Wn, 0, 1, o2l_sp));
        SOLA_TRY(out_proj(l, 2, x_mot, 1));
        SOLA_TRY(gn(lp, 2, x_o2l, nullptr, last ? 0 : 1, B, 1, (long long)N * Tp, 0, 1, N * Tp));  // the score head reads f32
        xin = x_o2l;
        xres = x_o2l;
        xres_sp = 1;
    }

    // ---- score head (module/module.py:152-160)
    HeadDesc hd{xin, buf("lbar"), score_map, score_tokens, B, N, Tp, D};
    SOLA_TRY(launch_score_head(hd, s));
    c->last = p;
    c->last_obj = nullptr;
    return SOLA_OK;
}
