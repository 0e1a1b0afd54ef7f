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

namespace {

// Operand casts that the PRODUCING GroupNorm already wrote (GroupNormDesc::y_cast; sola_tune "train_gn_cast" 0 = separate cast launches):
// the cast of a GEMM input was a launch of its own reading the f32 activation back - 24 of them per step.  Entry e belongs to the e-th
// distinct input of the projection launch that follows (the encoder uses entry 0); the GEMM that reads `src` takes it.
struct NormCasts {
    const float* src[2] = {nullptr, nullptr};
    float* dst[2] = {nullptr, nullptr};
    void offer(int e, const float* s, float* d) { src[e] = s; dst[e] = d; }
    float* take(int e, const float* s) {  // where the operand cast of `s`, the e-th distinct input, sits, or null; the entry is spent
        if (!s || src[e] != s) return nullptr;
        src[e] = nullptr;
        return dst[e];
    }
    void drop(int e) { src[e] = nullptr; }
};

// The out-projection's operand slot that attention() reserved for the attention kernel to write (AttnDesc::o_cast, round 4; sola_tune
// "train_attn_cast" 0 = always the separate cast launch).  dst null: none reserved; done: the kernel's shape could, the rows are there.
struct AttnCast { float* dst = nullptr; void* side = nullptr; bool done = false; };

// What differs between the three sub-blocks of a layer: the projections' inputs, the residual, the norm's outputs y / y2 = y + PE and the
// FIRST / SECOND distinct input of the projection launch that follows (linear3 casts them into sp_a / sp_b in that order): when one of
// them is this norm's y or y2, the norm writes the cast itself (gn)
struct SiteIO { const float *xq, *xk, *xv, *resid; float *y, *y2; const float *next_src0, *next_src1; };

// One training forward: what sola_forward_train_impl validated, the plan, the modes it runs in, and the stages it is made of.
struct FwdRun {
    SolaCtx* const c;
    const float *const obj, *const lang;
    float *const score_map, *const score_tokens;
    char* const base;          // the caller's workspace
    const hipStream_t s;
    const RagShape* const rs;  // null = a uniform batch; else the token rows of all samples concatenated, every shape-dependent kernel
                               // reads the unit tables of begin() (ragged.h) and B / N / T / L hold the largest extents
    const Plan p;
    const int B = p.B, N = p.N, T = p.T, L = p.L, Tp = p.Tp, M = p.M, Wn = p.W;
    const int D = c->cfg.lang_token_dim, H = c->cfg.num_heads, DH = D / H;
    const int R = rs ? rs->NT : B * N;  // tracks
    const long long text_rows = rs ? rs->LW : (long long)B * Wn;
    const float scale = 1.0f / sqrtf((float)DH);
    // ---- modes
    // training forward in the split-f16 mode (sola_set_precision 1): the same GEMM kernels as the inference forward on casts of
    // the f32 activations, everything the backward reads stays f32
    // (from ~1024 token rows on: below that the step is launch-bound and the extra cast launches cost more than the GEMMs gain)
    // precisions 2 / 3: the same structure with plain 16-bit GEMM operands, ONE MFMA per product - mixed-precision training:
    // activations, statistics, softmax, accumulation and everything the backward reads stay f32
    const Elem opfmt = operand_format(c->precision);  // the step's GEMM operand format (BF16: training only; BASELINE config C2)
    const bool op16 = is_row16(opfmt), is_bf = opfmt == Elem::BF16;
    const OperandCast ocast{opfmt, s};  // the row-major casts into that format (ctx.h)
    const int k_unit = op16 ? 64 : 32;  // reduction lengths are whole k-tiles of the operands' kernels
    const bool split = opfmt != Elem::F32 && D % k_unit == 0 && c->cfg.object_token_dim % k_unit == 0 && M >= g_train_split_min_rows;
    // 16-bit operand modes: every fixed-scale operand cast gets its own slot of the ctx's arena and is listed by its f32 source - the
    // backward's dW products read it instead of casting the activation again (ctx.h; data-dependent scales keep the shared buffers)
    // The split-f16 step ("f16x3") keeps nothing of its split pairs (fetching their hi halves with every other 16-byte chunk slowed the
    // dW kernel's DMA by what the saved casts had cost); its operand casts instead write the hi halves ONCE MORE as plain f16 rows
    // into the arena (side16 below): 2 more bytes per value written here, 6 fewer moved by the backward's X cast.
    const bool keep16 = split && op16 && g_train_x16_keep != 0;
    const bool side16_on = split && !op16 && g_train_x16_keep != 0 && g_train_dw_f16 != 0;
    const Elem gn_fmt = (split && op16 && g_train_gn_cast) ? opfmt : Elem::F32;  // the norms' operand casts (NormCasts; split pairs: no gain, kernels.h)
    // ---- pieces of the workspace
    float* const splitk_ws = p.bufs.count("splitk") ? buf("splitk") : nullptr;
    const size_t splitk_bytes = splitk_ws ? buf_bytes("splitk") : 0;
    float* const gn_slots = buf("gn_slots");
    const size_t gn_slots_bytes = buf_bytes("gn_slots");
    // split: every GEMM input is cast into one of these two right before its launch, unless it has an arena slot (slot16)
    float *const sp_a = split ? buf("sp_a") : nullptr, *const sp_b = split ? buf("sp_b") : nullptr;
    RagTables rt;     // ragged: unit tables in the workspace (they stay valid for sola_backward_ragged)
    SiteShape shape;  // the layers' units (sites.h)
    NormCasts pc;

    FwdRun(SolaCtx* c_, const float* obj_, const float* lang_, Plan&& plan, float* sm, float* st, void* workspace, hipStream_t s_, const RagShape* rs_)
        : c(c_), obj(obj_), lang(lang_), score_map(sm), score_tokens(st), base(static_cast<char*>(workspace)), s(s_), rs(rs_), p(std::move(plan)) {}

    float* buf(const std::string& name) const { return reinterpret_cast<float*>(base + p.bufs.at(name).off); }
    size_t buf_bytes(const std::string& name) const { return (size_t)p.bufs.at(name).rows * p.bufs.at(name).cols * sizeof(float); }
    float* ab(int l, int a, const char* what) const { return buf(abuf(true, l, kAttnShort[a], what)); }
    const float* W(const std::string& name) const { return ctx_weight(c, name); }
    long long level_rows(int lvl) const { return rs ? rs->rows[lvl] : (long long)R * (lvl == 0 ? T : p.Tl[lvl - 1]); }
    const float* layer_in(int l) const { return l ? buf("l" + std::to_string(l - 1) + "_o2l") : buf("conv5"); }  // l = n_layers: the head's input

    int begin(size_t ws_bytes) {
        SOLA_TRY(sola_check_forward_args(c, "forward", p.total, base, ws_bytes));
        if (rs) SOLA_TRY(rag_build_tables(c, *rs, base + p.bufs.at("tables").off, true, &rt, s));
        shape = rs ? site_shape_samples(rt) : site_shape_uniform(B, N, Tp, Wn);
        // the arena is the CALLER's (sola_set_x16_arena, round 4: an allocation of its own - half of the free device memory at most, grown with a
        // stream sync and a device-wide free inside the training forward - was memory torch's allocator could neither see nor reclaim);
        // what a forward asked for in total is read with sola_x16_arena_info; what does not fit is cast again by the backward as before
        c->x16.clear();
        c->x16_used = c->x16_need = 0;
        c->reset_sites();
        return SOLA_OK;
    }

    // ---- kept operand casts
    void* side16(const float* src, long long rows, int cols) const {  // f16x3: where the plain-f16 side copy of `src` goes
        return side16_on ? c->x16_keep(src, rows, cols, Elem::F16) : nullptr;
    }
    float* slot16(int which, const float* src, long long rows, int cols) const {  // the operand cast of `src` goes here
        void* const q = keep16 ? c->x16_keep(src, rows, cols, opfmt) : nullptr;  // else, or without room: the shared buffers
        return q ? static_cast<float*>(q) : which ? sp_b : sp_a;
    }
    // The separate cast launch of a GEMM input: `src` at the fixed scale 1 into its arena slot or shared buffer `which` (-> dst), with the
    // f16x3 side copy.  An error code like every launch, so the place comes back through `dst`.
    int cast_operand(int which, const float* src, long long rows, int cols, float*& dst) const {
        dst = slot16(which, src, rows, cols);
        return ocast.fixed(src, cols, dst, rows, cols, 1.f, side16(src, rows, cols));
    }

    // a1: weight standardisation (module/ws.py:9-13), every training forward; the projections' 16-bit copies where they are stale
    int weights() const {
        SOLA_TRY(sola_refresh_conv_weights(c, split ? opfmt : Elem::F32, true, s));
        return split ? sola_refresh_lin16(c, s) : SOLA_OK;
    }

    // a2: encoder (module/module.py:74-96,137-140)
    int encoder() {
        const float* x = obj;
        for (int i = 0; i < 6; ++i) {
            const ConvGeom& g = c->conv[i];
            float* const out = buf("conv" + std::to_string(i));
            GemmDesc gd{};
            gd.nprob = 1;
            gd.p[0] = GemmProblem{x, c->ws_buf + c->ws_off[i], W(enc_name(kConvIdx[i]) + ".bias"), nullptr, out};
            gd.M = (int)level_rows(i + 1); gd.N = g.cout; gd.K = g.k * g.cin;
            gd.lda = g.cin; gd.ldr = 0; gd.ldc = g.cout;
            gd.conv = g.k > 1 ? 1 : 0;
            gd.T_in = i ? p.Tl[i - 1] : T; gd.T_out = p.Tl[i]; gd.stride = g.stride; gd.pad = g.pad; gd.Cin = g.cin;
            if (rs && gd.conv) { gd.rowmap = rt.rowmap[i]; gd.T_in = 1; gd.T_out = 1; }
            gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
            if (split && g.cin % k_unit == 0) {
                float* a16 = sp_a;
                if (i == 0 && !is_bf) {  // the caller's tokens: data-dependent power-of-two scale (forward_fast.hip); bfloat16 has f32's range -
                                         // its cast is the fixed-scale one below, kept for the backward's dW product like every other operand
                    SOLA_TRY(ocast.auto_scale(x, g.cin, a16, level_rows(i), g.cin, c->scal_pair(0)));
                    gd.out_scale_dev = c->scal_pair(0) + 1;
                } else if (float* const cast = pc.take(0, x)) a16 = cast;  // the producing GroupNorm wrote this operand
                else SOLA_TRY(cast_operand(0, x, level_rows(i), g.cin, a16));  // nobody wrote it: a cast launch of its own, a16 = where
                pc.drop(0);
                gd.p[0].A = a16;
                gd.p[0].W = ws16_weight(c, opfmt, i);
                gd.ab = opfmt; gd.out_scale = 1.f;
            }
            SOLA_TRY(launch_gemm(gd, s));
            x = out;  // (conv5, no norm behind it, feeds layer 0)
            if (i < 5) {
                const std::string np = enc_name(kNormIdx[i]);
                GroupNormDesc nd{};
                nd.slice_ws = gn_slots; nd.slice_ws_bytes = gn_slots_bytes;
                nd.x = out; nd.y = buf("act" + std::to_string(i)); nd.y2 = nullptr; nd.pe = nullptr;
                nd.gamma = W(np + ".weight"); nd.beta = W(np + ".bias");
                site_fill_norm(nd, rs ? site_tracks(rt, i + 1) : site_tracks(R, p.Tl[i]));
                nd.C = g.cout; nd.groups = c->cfg.n_groups; nd.eps = 1e-5f; nd.slope = 0.01f; nd.leaky = 1;
                nd.drop = c->enc_drop(i);
                if (gn_fmt != Elem::F32 && c->conv[i + 1].cin % 64 == 0) {  // conv i+1 takes the cast from here
                    nd.y_cast = slot16(0, nd.y, level_rows(i + 1), g.cout); nd.cast = gn_fmt;
                    pc.offer(0, nd.y, static_cast<float*>(nd.y_cast));
                }
                SOLA_TRY(launch_group_norm(nd, s));
                x = nd.y;
            }
        }
        return SOLA_OK;
    }

    // a3: positional table; text tokens ++ negative tokens and their mean (module/module.py:143-147)
    int text() const {
        SOLA_TRY(launch_pos_encoding(W("positional_encoding_gaussian_matrix"), D, Tp, c->cfg.max_temporal_length, buf("pe"), s));
        if (rs) return launch_lang_concat_ragged(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, rt.u_lang, c->cfg.n_negative, D, s);
        return launch_lang_concat(lang, W("negative_token.weight"), buf("lang"), buf("lbar"), B, L, c->cfg.n_negative, D, s);
    }

    // ---- a5: alignment layers (module/module.py:22-52)
    // nprob projections first_proj.. of site `a` in layer `l`, one launch.  a_scal: the inputs' data-dependent scale pair.
    // c16: the outputs are written as BFLOAT16 rows (bf16 steps, sites whose attention kernels read them: site16 below)
    int linear3(const float* a0, const float* a1, const float* a2, int l, int a, int nprob, int rows, float* o0, float* o1, float* o2,
                int first_proj, float* a_scal = nullptr, bool c16 = false) {
        const float* as[3] = {a0, a1, a2};
        float* os[3] = {o0, o1, o2};
        GemmDesc gd{};
        gd.nprob = nprob;
        for (int j = 0; j < nprob; ++j) {
            const std::string nm = lin_name(l, a, first_proj + j);
            gd.p[j] = GemmProblem{as[j], W(nm + ".weight"), W(nm + ".bias"), nullptr, os[j]};
        }
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
                    if (float* const cast = pc.take(at, as[j])) dst[at] = cast;  // the producing GroupNorm wrote this operand
                    else if (a_scal) SOLA_TRY(ocast.auto_scale(as[j], D, dst[at], rows, D, a_scal));
                    else SOLA_TRY(cast_operand(at, as[j], rows, D, dst[at]));  // a cast launch of its own, dst[at] = where
                }
                gd.p[j].A = dst[at];
                gd.p[j].W = lin16_weight(c, opfmt, l, a, first_proj + j);
                gd.p[j].scale_dev = c->lin_inv_scale(l, a, first_proj + j);
            }
            gd.ab = opfmt; gd.out_scale = 1.f;
            if (a_scal) gd.out_scale_dev = a_scal + 1;
            if (c16) gd.c = opfmt;
            pc.drop(0); pc.drop(1);
        }
        return launch_gemm(gd, s);
    }
    // bf16 steps: does attention site `a` keep q / k / v (forward) and dq / dk / dv (backward) as bfloat16 rows?  Both kernels must take
    // the shape (attn_simple.hip's training instantiation; attn_bwd.hip's one-pass kernel)
    bool site16(const AttnDesc& ad, int a) const {
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
    }
    // The attention output's operand cast for the out-projection is written by the attention kernel itself where its shape can: the slot
    // is reserved here and handed to out_proj in `ac`.  `keep`: the site's record for the backward.
    int attention(AttnDesc& ad, SolaCtx::SiteKeep& keep, AttnCast& ac) const {
        // measured on the 64-sample ragged mix (same box): f16 operands 22.67 -> 22.55 ms per step (attention +0.10 ms, cast launches -0.26 ms);
        // split pairs + side copy (10 instead of 4 bytes per element out of a latency-bound kernel) 31.76 -> 31.78 ms: no gain, so the
        // split-f16 step keeps its cast launches unless the key is 2
        if (split && (op16 ? g_train_attn_cast != 0 : g_train_attn_cast == 2) && ad.ldo == D) {
            ac.dst = slot16(0, ad.o, M, D);
            ac.side = side16(ad.o, M, D);
            ad.o_cast = ac.dst; ad.o_side = ac.side; ad.cast = opfmt; ad.o_cast_done = &ac.done;
            // bf16 steps (train_bf16_store 3): where the bf16-MFMA kernel writes the out-projection's operand rows itself and they have an arena
            // slot of their own, the f32 rows are not written at all - the out-projection, its weight gradient and the attention backward
            // (D = dO . O) read the bfloat16 rows (4 of the launch's 12 bytes per element)
            if (ad.in == Elem::BF16 && g_train_bf16_store >= 3 && ac.dst != sp_a && ac.dst != sp_b && ad.cast == Elem::BF16 &&
                attention_bf16_mfma_supported(ad) && attention_bwd_dout_bf16_enabled()) {
                ad.o = nullptr;
                keep.o16 = true;
            }
        }
        return launch_attention(ad, s);
    }
    // res = ao * W_out^T + bias + resid; `ac`: what attention() reserved for the operand cast of ao.
    // r16 != null (bf16 steps, sola_tune "train_bf16_store" 2): the residual is read from the sub-block input's bfloat16 operand copy and
    // the pre-norm rows are written as bfloat16 - 4 instead of 8 bytes per element through the epilogue of a K = 1024 GEMM that its f32
    // epilogue traffic bounds (profiles/r06_train_ragged_bf16.txt)
    int out_proj(int l, int a, const float* ao, const float* resid, float* res, const void* r16, const AttnCast& ac) const {
        const std::string nm = lin_name(l, a, 3);
        GemmDesc gd{};
        gd.nprob = 1;
        gd.p[0] = GemmProblem{ao, W(nm + ".weight"), W(nm + ".bias"), resid, res};
        gd.M = M; gd.N = D; gd.K = D; gd.lda = D; gd.ldr = D; gd.ldc = D;
        gd.splitk_ws = splitk_ws; gd.splitk_bytes = splitk_bytes;
        if (split && r16) { gd.p[0].R = static_cast<const float*>(r16); gd.r = gd.c = Elem::BF16; }
        if (split) {
            float* dst = ac.dst;
            if (!dst) SOLA_TRY(cast_operand(0, ao, M, D, dst));  // nothing reserved: a cast launch of its own, dst = where
            else if (!ac.done) SOLA_TRY(ocast.fixed(ao, D, dst, M, D, 1.f, ac.side));  // the attention kernel's shape could not write it
            gd.p[0].A = dst; gd.p[0].W = lin16_weight(c, opfmt, l, a, 3); gd.p[0].scale_dev = c->lin_inv_scale(l, a, 3);
            gd.ab = opfmt; gd.out_scale = 1.f;
        }
        return launch_gemm(gd, s);
    }
    // norm `a` of layer `l` over `units`: res -> y (y2 = y + PE); offers the operand casts of next_src0 / next_src1 (SiteIO)
    int gn(int l, int a, const float* res, float* y, float* y2, const RowFamily& units, const float* next_src0, const float* next_src1,
           bool res_bf16) {
        const std::string np = norm_name(l, a);
        GroupNormDesc nd{};
        nd.in = res_bf16 ? Elem::BF16 : Elem::F32;
        if (gn_fmt != Elem::F32) {
            const float* nxt[2] = {next_src0, next_src1};
            const long long y_rows = std::max<long long>(M, text_rows);  // the norm's token rows, bounded from above
            for (int e = 0; e < 2; ++e) {
                if (!nxt[e]) continue;
                if (nxt[e] == y) { nd.y_cast = slot16(e, y, y_rows, D); pc.offer(e, y, static_cast<float*>(nd.y_cast)); }
                else if (nxt[e] == y2) { nd.y2_cast = slot16(e, y2, y_rows, D); pc.offer(e, y2, static_cast<float*>(nd.y2_cast)); }
            }
            nd.cast = gn_fmt;
        }
        nd.slice_ws = gn_slots; nd.slice_ws_bytes = gn_slots_bytes;
        nd.x = res; nd.y = y; nd.y2 = y2; nd.pe = y2 ? buf("pe") : nullptr;
        nd.gamma = W(np + ".weight"); nd.beta = W(np + ".bias");
        site_fill_norm(nd, units);
        nd.C = D; nd.groups = c->cfg.n_groups_module;
        nd.eps = 1e-5f; nd.slope = 0.f; nd.leaky = 0;
        int wrote = 0;  // the object -> language norm: (mean, rstd) kept for the backward where the sliced shape computes them
        if (a == 2 && g_train_gn_stats) { nd.stats_out = buf("l" + std::to_string(l) + "_gn2st"); nd.stats_written = &wrote; }
        SOLA_TRY(launch_group_norm(nd, s));
        if (nd.stats_out) c->gn2_stats[l] = (char)wrote;
        return SOLA_OK;
    }
    // the bf16 operand copy of a sub-block's input, if it sits in the kept-operand arena (a shared cast buffer is overwritten before the
    // out-projection runs) - then the sub-block's pre-norm rows are bfloat16 (out_proj / gn above)
    const void* resid16(const float* resid) const {
        if (!(split && is_bf && g_train_bf16_store >= 2 && keep16 && D % 8 == 0)) return nullptr;
        return c->x16_find(resid, D, Elem::BF16);
    }
    // site `a` of layer `l`: projections -> attention -> out-projection + residual -> norm
    int sub_block(int l, int a, const SiteIO& io) {
        const SiteGeom g = site_geom(shape, a);
        float *const q = ab(l, a, "q"), *const k = ab(l, a, a == 2 ? "lk" : "k"), *const v = ab(l, a, a == 2 ? "lv" : "v");
        float *const attn = ab(l, a, "attn"), *const res = ab(l, a, "res");
        SolaCtx::SiteKeep& keep = c->site(l, a);
        AttnDesc ad{};
        ad.q = q; ad.k = k; ad.v = v; ad.o = attn;
        ad.ldq = ad.ldk = ad.ldv = ad.ldo = D;
        ad.H = H; ad.DH = DH; ad.scale = scale; ad.lse = ab(l, a, "lse");
        site_fill_attn(ad, g);
        ad.drop = c->attn_drop(l, a);
        keep.qkv16 = site16(ad, a);
        if (a < 2) {
            SOLA_TRY(linear3(io.xq, io.xk, io.xv, l, a, 3, M, q, k, v, 0, nullptr, keep.qkv16));
        } else {  // q over the layer rows, k / v over the text rows (their data-dependent scale: scal_pair(1))
            SOLA_TRY(linear3(io.xq, nullptr, nullptr, l, a, 1, M, q, nullptr, nullptr, 0, nullptr, keep.qkv16));
            SOLA_TRY(linear3(buf("lang"), buf("lang"), nullptr, l, a, 2, (int)text_rows, k, v, nullptr, 1, split ? c->scal_pair(1) : nullptr, keep.qkv16));
        }
        ad.in = keep.qkv16 ? Elem::BF16 : Elem::F32;
        AttnCast ac;
        SOLA_TRY(attention(ad, keep, ac));
        const void* r16 = resid16(io.resid);
        keep.res16 = r16 != nullptr;
        SOLA_TRY(out_proj(l, a, attn, io.resid, res, r16, ac));
        return gn(l, a, res, io.y, io.y2, g.q, io.next_src0, io.next_src1, r16 != nullptr);
    }
    int layer(int l) {
        const std::string ls = "l" + std::to_string(l);
        const float* const xin = layer_in(l);
        float *const x_obj = buf(ls + "_obj"), *const x_pe = buf(ls + "_xpe"), *const x_mot = buf(ls + "_motion"), *const x_o2l = buf(ls + "_o2l");
        // (i) inter-object attention over the N tracks of each (b, t'), module.py:31-35; (ii) motion attention over T' per track, PE on q
        // and k only, :38-43; (iii) object -> language cross attention, :46-50 - the next layer's q / k / v projections read x_o2l
        // (nothing reads its cast behind the last layer)
        const float* nxt_in = l + 1 < c->cfg.n_layers ? x_o2l : nullptr;
        const SiteIO io[3] = {{xin, xin, xin, xin, x_obj, x_pe, x_pe, x_obj},
                              {x_pe, x_pe, x_obj, x_obj, x_mot, nullptr, x_mot, nullptr},
                              {x_mot, nullptr, nullptr, x_mot, x_o2l, nullptr, nxt_in, nullptr}};
        for (int a = 0; a < 3; ++a) SOLA_TRY(sub_block(l, a, io[a]));
        return SOLA_OK;
    }

    // a6: score head (module/module.py:152-160)
    int head() const {
        HeadDesc hd{layer_in(c->cfg.n_layers), buf("lbar"), score_map, score_tokens};
        hd.D = D;
        site_fill_head(hd, shape);
        return launch_score_head(hd, s);
    }
    void record() const {  // what the backward and the taps read of this forward
        c->last = p; c->last_rag = rt;
        c->last_ws = base; c->last_obj = obj;
    }
};

}  // namespace

// rs != null: a ragged batch (sola_forward_train_ragged); B, N, T, L are then ignored.
int sola_forward_train_impl(SolaCtx* c, const float* obj, const float* lang, int B, int N, int T, int L, float* score_map,
                            float* score_tokens, void* workspace, size_t ws_bytes, hipStream_t s, const RagShape* rs) {
    SOLA_ARG(c && obj && lang && score_map && score_tokens && workspace, "forward: null argument");
    if (rs) SOLA_ARG(rs->identity, "forward: a ragged training batch has one sample per video (sample_video[i] == i)");
    else SOLA_ARG(B > 0 && N > 0 && T > 0 && L >= 1, "forward: bad sizes B=%d N=%d T=%d L=%d", B, N, T, L);
    FwdRun r(c, obj, lang, rs ? make_plan_ragged(c, *rs) : make_plan(c, B, N, T, L, true), score_map, score_tokens, workspace, s, rs);
    SOLA_TRY(r.begin(ws_bytes));
    SOLA_TRY(r.weights());
    SOLA_TRY(r.encoder());
    SOLA_TRY(r.text());
    for (int l = 0; l < c->cfg.n_layers; ++l) SOLA_TRY(r.layer(l));
    SOLA_TRY(r.head());
    r.record();
    return SOLA_OK;
}
