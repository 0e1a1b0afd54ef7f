// Training forward of LanguageAlignedTrackSelectionModule.forward (module/module.py:130-162): host code that sequences the
// kernels of gemm.hip / attn.hip / norm.hip / head.hip over one workspace arena.  Every attention keeps its own
// q/k/v/output/residual buffers plus the softmax log-sum-exp, which backward.hip consumes.  The workspace plans of both
// forwards live here too; the inference forward is forward_infer.hip.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ragged.h"
#include "sites.h"

int g_train_gn_cast = 1;  // sola_tune "train_gn_cast": 1 = a GroupNorm of the training forward also writes the operand cast of the GEMM behind it
int g_train_attn_cast = 1;  // sola_tune "train_attn_cast": 1 = f16 / bf16 operand steps: the training forward's attention kernels also write the out-projection's operand cast; 2 = the split-f16 step too
int g_train_bf16_store = 3;  // sola_tune "train_bf16_store" (round 6): 1 = bf16 steps keep q / k / v and the backward's gradient operands as bfloat16 rows where the kernels take
                             // them; 2 = also the pre-norm rows of the layers (out-projection + residual -> GroupNorm); 3 (default) = also the conv input gradients' per-tap
                             // contributions between their GEMM and the gather; 0 = f32 storage (the round-5 step)
int g_train_gn_stats = 1;  // sola_tune "train_gn_stats": 1 = the training forward keeps the sliced GroupNorm shape's (mean, rstd) for the backward (A/B)
int g_train_x16_keep = 1;  // sola_tune "train_x16_keep": 1 = 16-bit operand modes keep the forward's operand casts for the backward's dW products (ctx.h)
int g_train_split_min_rows = 1024;  // sola_tune "train_split_min_rows": training takes the split-f16 GEMMs from this many token rows on

// Workspace layout shared by the uniform and the ragged plans: only the row counts differ.
namespace {
struct PlanSizes {
    int64_t rows0;      // object-token rows (level 0)
    int64_t rows[6];    // token rows behind each conv
    int64_t M, BW;      // layer rows, text ++ negative rows
    int64_t S;          // samples
    int64_t gn_slots;   // floats of the sliced GroupNorm shape's scratch
    size_t tables;      // ragged: bytes of the descriptor / unit-table region (0 = uniform batch)
};
void plan_fill(Plan& p, const SolaCtx* c, const PlanSizes& z, bool train) {
    const int D = c->cfg.lang_token_dim, H = c->cfg.num_heads;
    if (z.tables) p.add("tables", (int64_t)((z.tables + 3) / 4), 1);
    for (int i = 0; i < 6; ++i) {
        p.add("conv" + std::to_string(i), z.rows[i], c->conv[i].cout);
        if (i < 5) p.add("act" + std::to_string(i), z.rows[i], c->conv[i].cout);
    }
    // single-sample regime: scratch for the two-pass split-K of the GEMMs whose grid is smaller than the chip (gemm.hip)
    if (z.M <= 8192) p.add("splitk", 8192, 4096);
    p.add("pe", p.Tp, D);
    // slots of the sliced GroupNorm shape (8 bytes per (unit, slice); units of more than 256 tokens at 128 channels per group):
    // bounded by rows / 11 entries over every norm of the path
    p.add("gn_slots", z.gn_slots, 1);
    p.add("lang", z.BW, D);
    p.add("lbar", z.S, D);
    if (!train && c->precision >= 1) {  // split-f16 (or f16) copies of the three f32-born GEMM inputs (forward_infer.hip)
        p.add("obj_sp", z.rows0, c->cfg.object_token_dim);
        p.add("conv5_sp", z.M, D);
        p.add("lang_sp", z.BW, D);
    }
    if (train && c->precision >= 1 && z.M >= g_train_split_min_rows) {
        // split-f16 training forward: every GEMM input is cast into one of two scratch buffers right before its launch
        // (the f32 activations stay where the backward reads them)
        int64_t amax = std::max<int64_t>(z.rows0 * c->cfg.object_token_dim, std::max<int64_t>(z.M * D, z.BW * D));
        for (int i = 0; i < 5; ++i) amax = std::max<int64_t>(amax, z.rows[i] * c->conv[i].cout);
        p.add("sp_a", amax, 1);
        p.add("sp_b", z.M, D);
    }
    const int n_sets = train ? c->cfg.n_layers : 1;
    for (int l = 0; l < n_sets; ++l)
        for (int a = 0; a < (train ? 3 : 1); ++a) {
            p.add(abuf(train, l, kAttnShort[a], "q"), z.M, D);
            if (!train || a < 2) {
                p.add(abuf(train, l, kAttnShort[a], "k"), z.M, D);
                p.add(abuf(train, l, kAttnShort[a], "v"), z.M, D);
            }
            p.add(abuf(train, l, kAttnShort[a], "attn"), z.M, D);
            p.add(abuf(train, l, kAttnShort[a], "res"), z.M, D);
            if (train) p.add(abuf(train, l, kAttnShort[a], "lse"), z.M, H);
            if (!train || a == 2) {
                p.add(abuf(train, l, kAttnShort[a], "lk"), z.BW, D);
                p.add(abuf(train, l, kAttnShort[a], "lv"), z.BW, D);
            }
        }
    for (int l = 0; l < c->cfg.n_layers; ++l) {
        // training: (mean, rstd) of the object->language norm's (sample, group) units where the sliced shape computes them - the backward's
        // three-pass kernel of those units then walks x twice instead of four times (GroupNormDesc::stats_out)
        if (train) p.add("l" + std::to_string(l) + "_gn2st", z.S * c->cfg.n_groups_module, 2);
        p.add("l" + std::to_string(l) + "_obj", z.M, D);
        p.add("l" + std::to_string(l) + "_xpe", z.M, D);
        p.add("l" + std::to_string(l) + "_motion", z.M, D);
        p.add("l" + std::to_string(l) + "_o2l", z.M, D);
    }
}
}  // namespace

Plan make_plan(const SolaCtx* c, int B, int N, int T, int L, bool train) {
    Plan p;
    p.B = B; p.N = N; p.T = T; p.L = L; p.train = train;
    p.W = L + c->cfg.n_negative;
    int t = T;
    for (int i = 0; i < 6; ++i) {
        t = (t + 2 * c->conv[i].pad - c->conv[i].k) / c->conv[i].stride + 1;
        p.Tl[i] = t;
    }
    p.Tp = p.Tl[5];
    p.M = B * N * p.Tp;
    const int64_t R = (int64_t)B * N;
    PlanSizes z{};
    z.rows0 = R * T;
    for (int i = 0; i < 6; ++i) z.rows[i] = R * p.Tl[i];
    z.M = p.M; z.BW = (int64_t)B * p.W; z.S = B;
    z.gn_slots = std::max<int64_t>(R * T, (int64_t)p.M) / 4 + 1024;
    plan_fill(p, c, z, train);
    return p;
}

// Plan of a ragged TRAINING batch (sola_forward_train_ragged): the same buffers over the concatenated rows, plus the table
// region.  B = samples; N, T, L, W, Tl, Tp hold the LARGEST extents (they only select kernel shapes); M = all layer rows.
Plan make_plan_ragged(const SolaCtx* c, const RagShape& r) {
    Plan p;
    p.rag = true;
    p.B = r.S; p.N = r.maxN; p.T = r.maxT[0]; p.L = r.maxW - c->cfg.n_negative; p.train = true;
    p.W = r.maxW;
    for (int i = 0; i < 6; ++i) p.Tl[i] = r.maxT[i + 1];
    p.Tp = r.maxT[6];
    p.M = (int)r.Ms;
    PlanSizes z{};
    z.rows0 = r.rows[0];
    for (int i = 0; i < 6; ++i) z.rows[i] = r.rows[i + 1];
    z.M = r.Ms; z.BW = r.LW; z.S = r.S;
    z.gn_slots = (int64_t)(rag_gn_slots_bytes(r) / 4 + 64);
    z.tables = rag_tables_bytes(r, true);
    plan_fill(p, c, z, true);
    return p;
}

// rs != null: a ragged batch (sola_forward_train_ragged) - the token rows of all samples concatenated, every shape-dependent
// kernel reads the unit tables built here (ragged.h); B, N, T, L are then ignored.
int sola_forward_train_impl(SolaCtx* c, const float* obj, const float* lang, int B, int N, int T, int L, float* score_map,
                            float* score_tokens, void* workspace, size_t ws_bytes, hipStream_t s, const RagShape* rs) {
    SOLA_ARG(c && obj && lang && score_map && score_tokens && workspace, "forward: null argument");
    if (rs) SOLA_ARG(rs->identity, "forward: a ragged training batch has one sample per video (sample_video[i] == i)");
    else SOLA_ARG(B > 0 && N > 0 && T > 0 && L >= 1, "forward: bad sizes B=%d N=%d T=%d L=%d", B, N, T, L);
    Plan p = rs ? make_plan_ragged(c, *rs) : make_plan(c, B, N, T, L, true);
    SOLA_TRY(sola_check_forward_args(c, "forward", p.total, workspace, ws_bytes));
    char* base = static_cast<char*>(workspace);
    auto buf = [&](const std::string& name) { return reinterpret_cast<float*>(base + p.bufs.at(name).off); };
    float* const splitk_ws = p.bufs.count("splitk") ? buf("splitk") : nullptr;
    const size_t splitk_bytes = splitk_ws ? (size_t)p.bufs.at("splitk").rows * p.bufs.at("splitk").cols * sizeof(float) : 0;
    auto W = [&](const std::string& name) { return ctx_weight(c, name); };
    const int D = c->cfg.lang_token_dim, H = c->cfg.num_heads, DH = D / H;
    const int Tp = p.Tp, M = p.M, Wn = p.W;
    if (rs) { B = rs->S; N = rs->maxN; T = rs->maxT[0]; }
    const int R = rs ? rs->NT : B * N;
    RagTables rt;  // ragged: unit tables in the workspace (they stay valid for sola_backward_ragged)
    if (rs) SOLA_TRY(rag_build_tables(c, *rs, base + p.bufs.at("tables").off, true, &rt, s));
    auto level_rows = [&](int lvl) -> long long { return rs ? rs->rows[lvl] : (long long)R * (lvl == 0 ? T : p.Tl[lvl - 1]); };
    const long long text_rows = rs ? rs->LW : (long long)B * Wn;
    // training forward in the split-f16 mode (sola_set_precision 1): the same GEMM kernels as the inference forward on casts of
    // the f32 activations, everything the backward reads stays f32
    // (from ~1024 token rows on: below that the step is launch-bound and the extra cast launches cost more than the GEMMs gain)
    // precisions 2 / 3: the same structure with plain 16-bit GEMM operands, ONE MFMA per product - mixed-precision training:
    // activations, statistics, softmax, accumulation and everything the backward reads stay f32
    const Elem opfmt = operand_format(c->precision);  // the step's GEMM operand format (BF16: training only; BASELINE config C2)
    const bool op16 = is_row16(opfmt), is_bf = opfmt == Elem::BF16;
    const int k_unit = op16 ? 64 : 32;  // reduction lengths are whole k-tiles of the operands' kernels
    const bool split = opfmt != Elem::F32 && D % k_unit == 0 && c->cfg.object_token_dim % k_unit == 0 && p.M >= g_train_split_min_rows;
    auto cast_auto = [&](const float* in, int ld, float* out, long long rows, int K, float* scal) -> int {
        return op16 ? launch_cast_f16(in, ld, out, K, rows, K, 0.f, scal, opfmt, s) : launch_cast_sp16_auto(in, ld, out, K, rows, K, scal, s);
    };
    auto cast_fixed = [&](const float* in, int ld, float* out, long long rows, int K, float scale, void* side16 = nullptr) -> int {
        return op16 ? launch_cast_f16(in, ld, out, K, rows, K, scale, nullptr, opfmt, s) : launch_cast_sp16(in, ld, out, K, rows, K, scale, s, side16);
    };

    // a1: weight standardisation (module/ws.py:9-13), every training forward
    SOLA_TRY(sola_refresh_conv_weights(c, split ? opfmt : Elem::F32, true, s));
    auto lin_idx = [&](const std::string& attn, int proj) -> int {  // attn = "object_lang_align_layers.<l>.<name>"
        const int l = attn[attn.find('.') + 1] - '0';
        int a3 = 0;
        for (int a = 0; a < 3; ++a)
            if (attn.size() >= strlen(kAttnLong[a]) && attn.compare(attn.size() - strlen(kAttnLong[a]), std::string::npos, kAttnLong[a]) == 0) a3 = a;
        return (l * 3 + a3) * 4 + proj;
    };
    auto lin16 = [&](const std::string& attn, int proj) -> const float* {  // split pairs: D*D floats per matrix; plain f16: D*D halfs
        return op16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(c->lin16_buf) + (size_t)lin_idx(attn, proj) * D * D)
                    : c->lin16_buf + (size_t)lin_idx(attn, proj) * D * D;
    };
    auto lin_inv = [&](const std::string& attn, int proj) -> const float* { return c->scal_buf + 2 * (2 + lin_idx(attn, proj)) + 1; };
    if (split) SOLA_TRY(sola_refresh_lin16(c, s));
    float* const sp_a = split ? buf("sp_a") : nullptr;
    float* const sp_b = split ? buf("sp_b") : nullptr;
    // 16-bit operand modes: every fixed-scale operand cast gets its own slot of the ctx's arena and is listed by its f32 source - the
    // backward's dW products read it instead of casting the activation again (ctx.h; data-dependent scales keep the shared buffers)
    // The split-f16 step ("f16x3") keeps nothing of its split pairs (fetching their hi halves with every other 16-byte chunk slowed the
    // dW kernel's DMA by what the saved casts had cost); its operand casts instead write the hi halves ONCE MORE as plain f16 rows
    // into the arena (side16 below): 2 more bytes per value written here, 6 fewer moved by the backward's X cast.
    const bool keep16 = split && op16 && g_train_x16_keep != 0;
    const bool side16_on = split && !op16 && g_train_x16_keep != 0 && g_train_dw_f16 != 0;
    // the arena is the CALLER's (sola_set_x16_arena, round 4: an allocation of its own - half of the free device memory at most, grown with a
    // stream sync and a device-wide free inside the training forward - was memory torch's allocator could neither see nor reclaim);
    // what a forward asked for in total is read with sola_x16_arena_info; what does not fit is cast again by the backward as before
    c->x16.clear();
    c->x16_used = 0;
    c->x16_need = 0;
    auto side16 = [&](const float* src, long long rows, int cols) -> void* {  // f16x3: where the plain-f16 side copy of `src` goes
        if (!side16_on) return nullptr;
        void* q = c->x16_alloc((size_t)rows * cols * 2);
        if (q) c->x16.push_back(SolaCtx::X16Entry{src, q, cols, Elem::F16});
        return q;
    };
    auto slot16 = [&](int which, const float* src, long long rows, int cols) -> float* {  // the operand cast of `src` goes here
        if (keep16)
            if (void* q = c->x16_alloc((size_t)rows * cols * 2)) {
                c->x16.push_back(SolaCtx::X16Entry{src, q, cols, opfmt});
                return static_cast<float*>(q);
            }
        return which ? sp_b : sp_a;
    };

    // a2: encoder (module/module.py:74-96,137-140)
    // Operand casts written by the PRODUCING GroupNorm (GroupNormDesc::y_cast; sola_tune "train_gn_cast" 0 = separate cast launches):
    // the cast of a GEMM input was a launch of its own reading the f32 activation back - 24 of them per step
    const Elem gn_fmt = (split && op16 && g_train_gn_cast) ? opfmt : Elem::F32;  // 16-bit operand modes (split pairs: no gain, kernels.h)
    const float* pc_src[2] = {nullptr, nullptr};  // activations whose operand cast already sits in pc_dst (consumed by the next GEMM)
    float* pc_dst[2] = {nullptr, nullptr};
    const float* x = obj;
    int t_in = T;
    for (int i = 0; i < 6; ++i) {
        const ConvGeom& g = c->conv[i];
        const std::string cp = "short_motion_encoder." + std::to_string(kConvIdx[i]);
        GemmDesc gd{};
        gd.nprob = 1;
        gd.p[0] = GemmProblem{x, c->ws_buf + c->ws_off[i], W(cp + ".bias"), nullptr, buf("conv" + std::to_string(i))};
        gd.M = (int)level_rows(i + 1); gd.N = g.cout; gd.K = g.k * g.cin;
        gd.lda = g.cin; gd.ldr = 0; gd.ldc = g.cout;
        gd.conv = g.k > 1 ? 1 : 0;
        gd.T_in = t_in; gd.T_out = p.Tl[i]; gd.stride = g.stride; gd.pad = g.pad; gd.Cin = g.cin;
        if (rs && gd.conv) { gd.rowmap = rt.rowmap[i]; gd.T_in = 1; gd.T_out = 1; }
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        if (split && g.cin % k_unit == 0) {
            if (i == 0 && !is_bf) {  // the caller's tokens: data-dependent power-of-two scale (forward_fast.hip); bfloat16 has f32's range -
                                            // its cast is the fixed-scale one below, kept for the backward's dW product like every other operand
                SOLA_TRY(cast_auto(x, g.cin, sp_a, level_rows(i), g.cin, c->scal_pair(0)));
                gd.out_scale_dev = c->scal_pair(0) + 1;
                gd.p[0].A = sp_a;
            } else if (pc_src[0] != x) {
                float* dst = slot16(0, x, level_rows(i), g.cin);
                SOLA_TRY(cast_fixed(x, g.cin, dst, level_rows(i), g.cin, 1.f, side16(x, level_rows(i), g.cin)));
                gd.p[0].A = dst;
            } else {
                gd.p[0].A = pc_dst[0];
            }
            pc_src[0] = nullptr;
            gd.p[0].W = op16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(c->ws16_buf) + c->ws_off[i]) : c->ws16_buf + c->ws_off[i];
            gd.ab = opfmt; gd.out_scale = 1.f;
        }
        SOLA_TRY(launch_gemm(gd, s));
        if (i < 5) {
            const std::string np = "short_motion_encoder." + std::to_string(kNormIdx[i]);
            GroupNormDesc nd{};
            nd.slice_ws = buf("gn_slots"); nd.slice_ws_bytes = (size_t)p.bufs.at("gn_slots").rows * p.bufs.at("gn_slots").cols * sizeof(float);
            nd.x = buf("conv" + std::to_string(i)); nd.y = buf("act" + std::to_string(i)); nd.y2 = nullptr; nd.pe = nullptr;
            nd.gamma = W(np + ".weight"); nd.beta = W(np + ".bias");
            site_fill_norm(nd, rs ? site_tracks(rt, i + 1) : site_tracks(R, p.Tl[i]));
            nd.C = g.cout; nd.groups = c->cfg.n_groups; nd.eps = 1e-5f; nd.slope = 0.01f; nd.leaky = 1;
            nd.drop = c->enc_drop(i);
            if (gn_fmt != Elem::F32 && c->conv[i + 1].cin % 64 == 0) {  // conv i+1 takes the cast from here
                float* dst = slot16(0, nd.y, level_rows(i + 1), g.cout);
                nd.y_cast = dst; nd.cast = gn_fmt;
                pc_src[0] = nd.y; pc_dst[0] = dst;
            }
            SOLA_TRY(launch_group_norm(nd, s));
            x = buf("act" + std::to_string(i));
        } else {
            x = buf("conv5");
        }
        t_in = p.Tl[i];
    }

    // a3: positional table; text tokens ++ negative tokens and their mean (module/module.py:143-147)
    SOLA_TRY(launch_pos_encoding(W("positional_encoding_gaussian_matrix"), D, Tp, c->cfg.max_temporal_length, buf("pe"), s));
    if (rs) SOLA_TRY(launch_lang_concat_ragged(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, rt.u_lang, c->cfg.n_negative, D, s));
    else SOLA_TRY(launch_lang_concat(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s));

    // a5: alignment layers (module/module.py:22-52)
    const float scale = 1.0f / sqrtf((float)DH);
    // c16: the outputs are written as BFLOAT16 rows (bf16 steps, sites whose attention kernels read them: site16 below)
    auto linear3 = [&](const float* a0, const float* a1, const float* a2, const std::string& attn, int nprob, int rows,
                       float* o0, float* o1, float* o2, int first_proj, float* a_scal = nullptr, bool c16 = false) -> int {
        static const char* pn[3] = {"q_proj", "k_proj", "v_proj"};
        const float* as[3] = {a0, a1, a2};
        float* os[3] = {o0, o1, o2};
        GemmDesc gd{};
        gd.nprob = nprob;
        for (int j = 0; j < nprob; ++j)
            gd.p[j] = GemmProblem{as[j], W(attn + "." + pn[first_proj + j] + ".weight"),
                                  W(attn + "." + pn[first_proj + j] + ".bias"), nullptr, os[j]};
        gd.M = rows; gd.N = D; gd.K = D; gd.lda = D; gd.ldr = 0; gd.ldc = D;
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        if (split) {
            float* dst[2] = {sp_a, sp_b};
            const float* src[2] = {nullptr, nullptr};
            int nsrc = 0;
            for (int j = 0; j < nprob; ++j) {
                int at = -1;
                for (int e = 0; e < nsrc; ++e)
                    if (src[e] == as[j]) at = e;
                if (at < 0) {
                    at = nsrc++;
                    src[at] = as[j];
                    if (pc_src[at] == as[j]) dst[at] = pc_dst[at];  // the producing GroupNorm wrote this operand
                    else if (a_scal) SOLA_TRY(cast_auto(as[j], D, dst[at], rows, D, a_scal));
                    else {
                        dst[at] = slot16(at, as[j], rows, D);
                        SOLA_TRY(cast_fixed(as[j], D, dst[at], rows, D, 1.f, side16(as[j], rows, D)));
                    }
                }
                gd.p[j].A = dst[at];
                gd.p[j].W = lin16(attn, first_proj + j);
                gd.p[j].scale_dev = lin_inv(attn, first_proj + j);
            }
            gd.ab = opfmt; gd.out_scale = 1.f;
            if (a_scal) gd.out_scale_dev = a_scal + 1;
            if (c16) gd.c = opfmt;
            pc_src[0] = pc_src[1] = nullptr;
        }
        return launch_gemm(gd, s);
    };
    // bf16 steps: does attention site `ad` keep q / k / v (forward) and dq / dk / dv (backward) as bfloat16 rows?  Both kernels must take
    // the shape (attn_simple.hip's training instantiation; attn_bwd.hip's one-pass kernel)
    c->reset_sites();
    auto site16 = [&](const AttnDesc& ad, int a) -> bool {
        const bool o2l = a == 2;
        if (!(split && is_bf && g_train_bf16_store)) return false;
        // the backward's dW products of these gradients must take the row-major 16-bit kernel (no f32 copy exists to transpose)
        if (!gemm_tn_tr_supported(M, D, D, D, D) || (o2l && !gemm_tn_tr_supported((int)text_rows, D, D, D, D))) return false;
        // ... and hand its row-major operand to the dX GEMMs: with sola_tune "bwd_dual_cast" 0 grad_w_many / grad_x cast the f32 matrix
        // themselves.  (The rows are the attention backward's own, not the statistics pass's: "bwd_fused_bf16_cast" is not on this route.)
        // The backward checks again (BwdRun::need16): a switch may change behind this forward
        if (!g_bwd_dual_cast) return false;
        AttnDesc f = ad;
        f.in = Elem::BF16;
        f.o_cast = reinterpret_cast<void*>(1); f.cast = Elem::BF16;  // (what attention() below hands the launch)
        if (!attention_in_bf16_supported(f) && !attention_bf16_mfma_supported(f)) return false;
        // the backward's own record of the site (the chunked launch of site 2 gets its scratch there)
        return attention_bwd_bf16_supported(attn_bwd_site_desc(c, p, rs ? &rt : nullptr, a, reinterpret_cast<float*>(1)));
    };
    // The attention output's operand cast for the out-projection is written by the attention kernel itself where its shape can
    // (AttnDesc::o_cast, round 4; sola_tune "train_attn_cast" 0 = always the separate cast launch)
    const float* ac_src = nullptr;
    float* ac_dst = nullptr;
    void* ac_side = nullptr;
    bool ac_done = false;
    SolaCtx::SiteKeep* o16_site = nullptr;  // set by the layer loop in front of a site's attention() call: the site's record
    auto attention = [&](AttnDesc& ad) -> int {
        ac_src = nullptr; ac_done = false;
        // measured on the 64-sample ragged mix (same box): f16 operands 22.67 -> 22.55 ms per step (attention +0.10 ms, cast launches -0.26 ms);
        // split pairs + side copy (10 instead of 4 bytes per element out of a latency-bound kernel) 31.76 -> 31.78 ms: no gain, so the
        // split-f16 step keeps its cast launches unless the key is 2
        if (split && (op16 ? g_train_attn_cast != 0 : g_train_attn_cast == 2) && ad.ldo == D) {
            ac_src = ad.o;
            ac_dst = slot16(0, ad.o, M, D);
            ac_side = side16(ad.o, M, D);
            ad.o_cast = ac_dst; ad.o_side = ac_side; ad.cast = opfmt; ad.o_cast_done = &ac_done;
            // bf16 steps (train_bf16_store 3): where the bf16-MFMA kernel writes the out-projection's operand rows itself and they have an arena
            // slot of their own, the f32 rows are not written at all - the out-projection, its weight gradient and the attention backward
            // (D = dO . O) read the bfloat16 rows (4 of the launch's 12 bytes per element)
            if (o16_site && ad.in == Elem::BF16 && g_train_bf16_store >= 3 && ac_dst != sp_a && ac_dst != sp_b && ad.cast == Elem::BF16 &&
                attention_bf16_mfma_supported(ad) && attention_bwd_dout_bf16_enabled()) {
                ad.o = nullptr;
                o16_site->o16 = true;
            }
        }
        o16_site = nullptr;
        return launch_attention(ad, s);
    };
    // r16 != null (bf16 steps, sola_tune "train_bf16_store" 2): the residual is read from the sub-block input's bfloat16 operand copy and
    // the pre-norm rows are written as bfloat16 - 4 instead of 8 bytes per element through the epilogue of a K = 1024 GEMM that its f32
    // epilogue traffic bounds (profiles/r06_train_ragged_bf16.txt)
    auto out_proj = [&](const std::string& attn, const float* ao, const float* resid, float* res, const void* r16 = nullptr) -> int {
        GemmDesc gd{};
        gd.nprob = 1;
        gd.p[0] = GemmProblem{ao, W(attn + ".out_proj.weight"), W(attn + ".out_proj.bias"), resid, res};
        gd.M = M; gd.N = D; gd.K = D; gd.lda = D; gd.ldr = D; gd.ldc = D;
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        if (split && r16) { gd.p[0].R = static_cast<const float*>(r16); gd.r = gd.c = Elem::BF16; }
        if (split) {
            float* dst;
            if (ac_src == ao) {  // attention() reserved the operand's place; the attention kernel wrote it unless its shape cannot
                dst = ac_dst;
                if (!ac_done) SOLA_TRY(cast_fixed(ao, D, dst, M, D, 1.f, ac_side));
            } else {
                dst = slot16(0, ao, M, D);
                SOLA_TRY(cast_fixed(ao, D, dst, M, D, 1.f, side16(ao, M, D)));
            }
            ac_src = nullptr;
            gd.p[0].A = dst; gd.p[0].W = lin16(attn, 3); gd.p[0].scale_dev = lin_inv(attn, 3);
            gd.ab = opfmt; gd.out_scale = 1.f;
        }
        return launch_gemm(gd, s);
    };
    // next_src0 / next_src1: the FIRST / SECOND distinct input of the projection launch that follows (linear3 casts them into sp_a / sp_b in
    // that order): when one of them is this norm's y or y2, the norm writes the cast itself
    auto gn = [&](const std::string& lp, int l, int idx, const float* res, float* y, float* y2, const RowFamily& units, const float* next_src0,
                  const float* next_src1, bool res_bf16) -> int {
        GroupNormDesc nd{};
        nd.in = res_bf16 ? Elem::BF16 : Elem::F32;
        if (gn_fmt != Elem::F32) {
            const float* nxt[2] = {next_src0, next_src1};
            const long long y_rows = std::max<long long>(M, text_rows);  // the norm's token rows, bounded from above
            for (int e = 0; e < 2; ++e) {
                if (!nxt[e]) continue;
                if (nxt[e] == y) { float* dst = slot16(e, y, y_rows, D); nd.y_cast = dst; pc_src[e] = y; pc_dst[e] = dst; }
                else if (nxt[e] == y2) { float* dst = slot16(e, y2, y_rows, D); nd.y2_cast = dst; pc_src[e] = y2; pc_dst[e] = dst; }
            }
            nd.cast = gn_fmt;
        }
        nd.slice_ws = buf("gn_slots"); nd.slice_ws_bytes = (size_t)p.bufs.at("gn_slots").rows * p.bufs.at("gn_slots").cols * sizeof(float);
        nd.x = res; nd.y = y; nd.y2 = y2; nd.pe = y2 ? buf("pe") : nullptr;
        nd.gamma = W(lp + "norm." + std::to_string(idx) + ".weight");
        nd.beta = W(lp + "norm." + std::to_string(idx) + ".bias");
        site_fill_norm(nd, units);
        nd.C = D; nd.groups = c->cfg.n_groups_module;
        nd.eps = 1e-5f; nd.slope = 0.f; nd.leaky = 0;
        if (idx == 2 && g_train_gn_stats) {
            int wrote = 0;
            nd.stats_out = buf("l" + std::to_string(l) + "_gn2st");
            nd.stats_written = &wrote;
            SOLA_TRY(launch_group_norm(nd, s));
            c->gn2_stats[l] = (char)wrote;
            return SOLA_OK;
        }
        return launch_group_norm(nd, s);
    };
    // the bf16 operand copy of a sub-block's input, if it sits in the kept-operand arena (a shared cast buffer is overwritten before the
    // out-projection runs) - then the sub-block's pre-norm rows are bfloat16 (out_proj / gn above)
    auto resid16 = [&](const float* resid) -> const void* {
        if (!(split && is_bf && g_train_bf16_store >= 2 && keep16 && D % 8 == 0)) return nullptr;
        return c->x16_find(resid, D, Elem::BF16);
    };
    const SiteShape shape = rs ? site_shape_samples(rt) : site_shape_uniform(B, N, Tp, Wn);
    const float* xin = buf("conv5");
    for (int l = 0; l < c->cfg.n_layers; ++l) {
        const std::string lp = "object_lang_align_layers." + std::to_string(l) + ".";
        const std::string ls = "l" + std::to_string(l);
        auto ab = [&](int a, const char* what) { return buf(abuf(true, l, kAttnShort[a], what)); };
        float* x_obj = buf(ls + "_obj");
        float* x_pe = buf(ls + "_xpe");
        float* x_mot = buf(ls + "_motion");
        float* x_o2l = buf(ls + "_o2l");
        // What differs per site - the projections' inputs, the residual, the norm's outputs y / y2 = y + PE and the inputs of the NEXT
        // projection launch whose operand cast the norm may write (gn above): (i) inter-object attention over the N tracks of each (b, t'),
        // module.py:31-35; (ii) motion attention over T' per track, PE on q and k only, :38-43; (iii) object -> language cross attention,
        // :46-50 - the next layer's q / k / v projections read x_o2l (nothing reads its cast behind the last layer)
        const float* nxt_in = l + 1 < c->cfg.n_layers ? x_o2l : nullptr;
        const struct { const float *xq, *xk, *xv, *resid; float *y, *y2; const float *next_src0, *next_src1; } io[3] = {
            {xin, xin, xin, xin, x_obj, x_pe, x_pe, x_obj},
            {x_pe, x_pe, x_obj, x_obj, x_mot, nullptr, x_mot, nullptr},
            {x_mot, nullptr, nullptr, x_mot, x_o2l, nullptr, nxt_in, nullptr}};
        for (int a = 0; a < 3; ++a) {
            const SiteGeom g = site_geom(shape, a);
            const std::string an = lp + kAttnLong[a];
            float *const k = ab(a, a == 2 ? "lk" : "k"), *const v = ab(a, a == 2 ? "lv" : "v");
            AttnDesc ad{};
            ad.q = ab(a, "q"); ad.k = k; ad.v = v; ad.o = ab(a, "attn");
            ad.ldq = ad.ldk = ad.ldv = ad.ldo = D;
            ad.H = H; ad.DH = DH; ad.scale = scale; ad.lse = ab(a, "lse");
            site_fill_attn(ad, g);
            ad.drop = c->attn_drop(l, a);
            const bool s16 = site16(ad, a);
            if (a < 2) {
                SOLA_TRY(linear3(io[a].xq, io[a].xk, io[a].xv, an, 3, M, ab(a, "q"), k, v, 0, nullptr, s16));
            } else {  // q over the layer rows, k / v over the text rows (their data-dependent scale: scal_pair(1))
                SOLA_TRY(linear3(io[a].xq, nullptr, nullptr, an, 1, M, ab(a, "q"), nullptr, nullptr, 0, nullptr, s16));
                SOLA_TRY(linear3(buf("lang"), buf("lang"), nullptr, an, 2, (int)text_rows, k, v, nullptr, 1, split ? c->scal_pair(1) : nullptr, s16));
            }
            ad.in = s16 ? Elem::BF16 : Elem::F32;
            c->site(l, a).qkv16 = s16;
            o16_site = &c->site(l, a);
            SOLA_TRY(attention(ad));
            const void* r16 = resid16(io[a].resid);
            c->site(l, a).res16 = r16 != nullptr;
            SOLA_TRY(out_proj(an, ab(a, "attn"), io[a].resid, ab(a, "res"), r16));
            SOLA_TRY(gn(lp, l, a, ab(a, "res"), io[a].y, io[a].y2, g.q, io[a].next_src0, io[a].next_src1, r16 != nullptr));
        }
        xin = x_o2l;
    }

    // a6: score head (module/module.py:152-160)
    HeadDesc hd{xin, buf("lbar"), score_map, score_tokens};
    hd.D = D;
    site_fill_head(hd, shape);
    SOLA_TRY(launch_score_head(hd, s));
    c->last = p;
    c->last_rag = rt;
    c->last_ws = workspace;
    c->last_obj = obj;
    return SOLA_OK;
}
