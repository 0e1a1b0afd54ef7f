// Backward orchestration of the track-selection network (autograd of module/module.py:130-162): host code sequencing
// gemm.hip (dX via the NT kernel on transposed weights / the transposed-conv gather), gemm_tn.hip (dW, db),
// attn_bwd.hip, bwd.hip over the activations saved by sola_forward_train_impl.  Gradients of all 83
// parameters are written to the borrowed buffers registered with sola_set_grad (overwrite semantics).
// backward_impl validates the call and builds one BwdRun (context, plan, arena slots by enum, mode flags, the state the helpers share);
// its stages run in order: begin, score_head, layer (site_o2l, site_motion, site_obj over site_head = site_gn_bwd + out_proj_bwd +
// site_attention_bwd, and stats_dw), negative_tokens, encoder_stage (enc_dw, enc_dx, the norm's backward), ws_backward.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "ragged.h"
#include "sites.h"

int g_bwd_dual_cast = 1;  // sola_tune "bwd_dual_cast": the transposing cast of a gradient matrix also writes its row-major cast (A/B)
int g_bwd_fused_bf16_cast = 1;  // sola_tune "bwd_fused_bf16_cast": bf16 storage - the gradient statistics pass is the cast as well (A/B)

// sola_tune "train_dw_f16" (default 1, round 3): in the split-f16 training step (precision 1) the weight-gradient products
// dW = dY^T X run on PLAIN f16 casts of dY and X (one MFMA per product, f32 accumulation) instead of split pairs (three); forward and
// dX keep the split pairs.  A weight gradient is a sum over all token rows (>= 1024 here) in which the 2^-11 operand roundings
// average out: measured against the exact-f32 step (tools/train_dw_f16_errors.py) the median per-matrix error goes 5e-6 -> 1.2e-4
// (64 samples; 1.1e-5 -> 2.3e-4 at 8), the worst tensor (1.9e-3 / 4.9e-3: the forward's softmax near-ties) and the cosine of the
// whole gradient (0.999999) do not move; the step is 14 % faster on the ragged mix.  0 = split pairs everywhere.
int g_train_dw_f16 = 1;
// sola_tune "bwd_side_rows" (round 4): exact-f32 backward of at most this many token rows (the few-sample regime; the reference trains at
// batch size 1) runs its weight-gradient products dW = dY^T X - leaves of the graph, a third of the step's kernel time there - on a side
// stream beside the dX chain.  Kernels of 64-512 blocks leave most of the chip idle, so the two streams really overlap.  0 = off.
// Same kernels, same per-gradient order: results are bit-identical (tests/test_gpu_backward.py).  OFF by default: measured at one sample
// per step (tools/train_one_probe.py, profiles/r04_train_one_sample.txt) the step is bound by the HOST's enqueue rate as much as by the GPU
// (2.2 ms of host time per 2.7 ms step), and the ~60 event records / waits of the lane cost more host time (+0.5 ms) than the overlap saves.
int g_bwd_side_rows = 0;
// sola_tune "bwd_group_rows" (round 4): an exact-f32 backward of at most this many token rows DEFERS the weight-gradient products of its
// linear layers - every dY keeps a buffer of its own - and runs them all in ONE grouped launch behind the layers (gemm_tn.hip:
// gemm_tn_f32_group_kernel; 24 products + 48 slab reductions -> 1 launch), and transposes the weights its dX GEMMs read in one launch in
// front of them (36 -> 1).  At one sample per step (the reference's batch size) that is a third of the step's launches.  0 = off.
// Same products, a different (still fixed) summation order over the rows: deterministic, not bit-identical to the slab form.
int g_bwd_group_rows = 2048;

namespace {

// Slots of the backward's scratch arena, in the order make_arena lays them out.
enum Slot {
    S_G0, S_G1, S_E, S_DRES, S_DATTN, S_DQKV, S_DLKV, S_DLANG, S_DVEC, S_ATTN_PART, S_DLBAR_PART, S_DLBAR, S_ENC0, S_ENC1, S_DWSTD, S_WT, S_TN,
    S_GPART, S_BPART, S_COLSUM, S_SPLITK, S_DWKEEP, S_GNKEEP, S_ZCOL, S_DY_SP, S_WT_SP, S_SCAL, S_CPART, S_TNS, S_COUNT
};

struct Arena {
    char* base = nullptr;
    size_t total = 0;
    size_t off[S_COUNT] = {}, size[S_COUNT] = {};
    bool has[S_COUNT] = {};
    void add(Slot s, size_t floats) {
        off[s] = total;
        size[s] = floats * sizeof(float);
        has[s] = true;
        total += (floats * sizeof(float) + 255) & ~(size_t)255;
    }
    bool present(Slot s) const { return has[s]; }
    float* get(Slot s) const {
        if (!has[s]) throw std::out_of_range("scratch slot " + std::to_string((int)s) + " is not part of this step's arena");
        return reinterpret_cast<float*>(base + off[s]);
    }
    size_t bytes(Slot s) const { return has[s] ? size[s] : 0; }
    size_t bytes_from(Slot s) const { return total - off[s]; }  // upper bound to the end of the arena; the launchers check their own need
};

// row counts the arena is sized by: a uniform (B, N, T, L) batch or the concatenated rows of a ragged one
struct BwdSizes {
    size_t M, BW, R, S, inst_bt;  // layer rows, text ++ negative rows, tracks, samples, inter-object GroupNorm instances (sum of T')
    size_t rows[7];               // token rows per encoder level (0 = the object tokens)
    bool rag;
};
BwdSizes sizes_of(const Plan& p) {
    BwdSizes z{};
    z.M = p.M; z.BW = (size_t)p.B * p.W; z.R = (size_t)p.B * p.N; z.S = p.B; z.inst_bt = (size_t)p.B * p.Tp;
    z.rows[0] = z.R * p.T;
    for (int i = 0; i < 6; ++i) z.rows[i + 1] = z.R * p.Tl[i];
    z.rag = false;
    return z;
}
template <class RagLike>  // RagShape (before the forward) or RagTables (after it): the same extent fields
BwdSizes sizes_of_ragged(const RagLike& r) {
    BwdSizes z{};
    z.M = (size_t)r.Ms; z.BW = (size_t)r.LW; z.R = (size_t)r.NT; z.S = (size_t)r.S; z.inst_bt = (size_t)r.sumTpS;
    for (int j = 0; j < 7; ++j) z.rows[j] = (size_t)r.rows[j];
    z.rag = true;
    return z;
}

constexpr size_t kSplitkFloats = (size_t)8192 * 4096;
// 16 fixed scale slots + one pair per statistics pass of a step (6 convs, <= 8 per layer)
size_t scal_floats_of(const SolaCtx* c) { return 16 + 2 * (6 + 8 * (size_t)c->cfg.n_layers); }

Arena make_arena(const SolaCtx* c, const BwdSizes& z) {
    Arena a;
    const size_t D = c->cfg.lang_token_dim, H = c->cfg.num_heads, M = z.M, BW = z.BW;
    const size_t R = z.R;
    a.add(S_G0, M * D);
    a.add(S_G1, M * D);
    a.add(S_E, M * D);  // d(x + pe)
    a.add(S_DRES, M * D);
    a.add(S_DATTN, M * D);
    a.add(S_DQKV, M * 3 * D);
    a.add(S_DLKV, BW * 2 * D);
    a.add(S_DLANG, BW * D);
    a.add(S_DVEC, M * H);
    // object -> language attention backward in one pass: dK / dV partial sums per 256-query chunk of a sample (attn_bwd.hip); sized
    // for the most keys a text can have against the 64 the chunked launch takes (0 floats otherwise: the two-pass kernels run)
    a.add(S_ATTN_PART, attention_bwd_part_floats((long long)M, (int)z.S, (int)H, 64));
    a.add(S_DLBAR_PART, R * D);
    a.add(S_DLBAR, z.S * D);
    // GroupNorm partials are [n_inst][C]; n_inst is B*N (per track), B*T' (per time step) or B
    size_t enc_max = 0, ws_total = 0, wt_max = 3 * D * D, tn_max = 0, inst_c_max = std::max(R, z.inst_bt) * D;
    for (int i = 0; i < 6; ++i) {
        const ConvGeom& g = c->conv[i];
        enc_max = std::max(enc_max, z.rows[i + 1] * (size_t)g.cout);
        enc_max = std::max(enc_max, z.rows[i] * (size_t)g.cin);
        ws_total += (size_t)g.cout * g.cin * g.k;
        wt_max = std::max(wt_max, (size_t)g.cout * g.cin * g.k);
        tn_max = std::max(tn_max, gemm_tn_scratch_bytes((int)z.rows[i + 1], g.cout, g.k * g.cin));
        inst_c_max = std::max(inst_c_max, R * (size_t)g.cout);
    }
    tn_max = std::max(tn_max, gemm_tn_scratch_bytes((int)M, (int)D, (int)D));
    tn_max = std::max(tn_max, gemm_tn_scratch_bytes((int)BW, (int)D, (int)D));
    a.add(S_ENC0, enc_max);
    a.add(S_ENC1, enc_max);
    a.add(S_DWSTD, ws_total);
    a.add(S_WT, wt_max);
    a.add(S_TN, tn_max / sizeof(float) + 64);
    a.add(S_GPART, inst_c_max);
    a.add(S_BPART, inst_c_max);
    a.add(S_COLSUM, colsum_scratch_bytes(2, (int)std::max(M, std::max(R, z.inst_bt)), (int)D) / sizeof(float) + 64);
    // few-sample regime (the reference trains at batch size 1): the dX GEMMs have fewer 64x64 tiles than the chip has CUs; scratch
    // for their deterministic two-pass split-K, as the forward has (42-136 us per dX GEMM without it, 64 blocks on 256 CUs)
    if (M <= 8192) a.add(S_SPLITK, kSplitkFloats);
    const bool lowp = c->precision >= 1 && (long long)M >= g_train_split_min_rows;
    const bool few = !lowp && g_bwd_group_rows > 0 && M <= (size_t)g_bwd_group_rows;  // few-sample exact-f32 backward: deferred grouped dW (see g_bwd_group_rows)
    if (few) {
        size_t enc_keep = 0;  // + the encoder stages' dY (GroupNorm backward outputs) for the deferred conv weight gradients
        for (int i = 0; i < 5; ++i) enc_keep += z.rows[i + 1] * (size_t)c->conv[i].cout + 64;
        a.add(S_DWKEEP, (size_t)c->cfg.n_layers * (12 * M * D + 2 * BW * D + 7 * 64) + enc_keep);  // per layer: 3 dres + 3 dqkv (3D wide) + dlkv
        a.add(S_GNKEEP, (size_t)(3 * c->cfg.n_layers + 5) * 2 * (inst_c_max + 64));     // private (dgamma, dbeta) partials of every GroupNorm backward: one grouped column-sum launch per bucket
    }
    {   // conv dX as one GEMM z = dY W (every tap's contribution) + a col2im gather: the split-f16 / f16 modes, every ragged batch (the f32
        // path's transposed-conv gather needs one sequence length) and the few-sample backward (weights read where they lie)
        size_t zmax = 0;
        for (int i = 1; i < 6; ++i) zmax = std::max(zmax, z.rows[i + 1] * (size_t)c->conv[i].k * c->conv[i].cin);
        if (lowp || z.rag || few) a.add(S_ZCOL, zmax);
    }
    if (lowp) {  // split-f16 / f16-operand dX GEMMs (same size gate as the training forward): casts of dY and of the transposed weights, the data-dependent scale
        a.add(S_DY_SP, std::max(M, BW) * 3 * D);
        a.add(S_WT_SP, wt_max);
        a.add(S_SCAL, scal_floats_of(c));
        {   // per-64-row-slab column sums of a gradient matrix (launch_amax_colsum): bias gradients without a second read
            size_t cp = std::max((M / 64 + 1) * 3 * D, (BW / 64 + 1) * 2 * D);
            for (int i = 0; i < 6; ++i) cp = std::max(cp, (z.rows[i + 1] / 64 + 1) * (size_t)c->conv[i].cout);
            // round 6: every statistics pass of a step keeps its own slab table (the bias sums of a gradient bucket leave in one grouped
            // launch, flush_bias): per layer 3 out-projection tables, two [.., 3D] and one [.., D] for the q / k / v gradients, one text table
            size_t all = (size_t)c->cfg.n_layers * ((M / 64 + 1) * 10 * D + (BW / 64 + 1) * 2 * D + 7 * 64);
            for (int i = 0; i < 6; ++i) all += (z.rows[i + 1] / 64 + 1) * (size_t)c->conv[i].cout + 64;
            a.add(S_CPART, std::max(cp, all));
        }
        // split-f16 weight gradients of the projections (gemm_tn_split.hip): transposed operands + partial sums
        if (gemm_tn_split_supported((int)M, (int)D, (int)D)) {
            size_t need = gemm_tn_split_scratch_bytes((int)M, (int)D, (int)D, 3);
            if (gemm_tn_split_supported((int)BW, (int)D, (int)D)) need = std::max(need, gemm_tn_split_scratch_bytes((int)BW, (int)D, (int)D, 2));
            for (int i = 0; i < 6; ++i)
                if (gemm_tn_split_supported((int)z.rows[i + 1], c->conv[i].cout, c->conv[i].k * c->conv[i].cin))
                    need = std::max(need, gemm_tn_split_scratch_bytes((int)z.rows[i + 1], c->conv[i].cout, c->conv[i].k * c->conv[i].cin, 1));
            a.add(S_TNS, need / sizeof(float) + 64);
        }
    }
    return a;
}

}  // namespace

size_t sola_backward_scratch_bytes(const SolaCtx* c, const Plan& p) { return make_arena(c, sizes_of(p)).total; }

extern "C" size_t sola_backward_workspace_bytes(const SolaCtx* c, int B, int N, int T, int L) {
    if (!c || B <= 0 || N <= 0 || T <= 0 || L < 1) return 0;
    return sola_backward_scratch_bytes(c, make_plan(c, B, N, T, L, true));
}

extern "C" size_t sola_backward_ragged_workspace_bytes(const SolaCtx* c, const SolaRaggedBatch* batch) {
    if (!c || !batch) return 0;
    try {
        RagShape r;
        if (rag_shape(c, batch, r) != SOLA_OK) return 0;
        return make_arena(c, sizes_of_ragged(r)).total;
    } catch (const std::exception& e) {
        sola_set_error("backward_ragged_workspace_bytes: %s", e.what());
        return 0;
    }
}

AttnBwdDesc attn_bwd_site_desc(const SolaCtx* c, const Plan& p, const RagTables* rt, int a, float* part) {
    const int D = c->cfg.lang_token_dim, H = c->cfg.num_heads;
    AttnBwdDesc d{};
    d.ldq = d.ldk = d.ldv = d.ldo = D;
    d.ld_dq = 3 * D;
    d.ld_dk = d.ld_dv = a == 2 ? 2 * D : 3 * D;
    d.H = H; d.DH = D / H;
    d.scale = 1.0f / sqrtf((float)d.DH);
    site_fill_attn(d, site_geom(rt ? site_shape_samples(*rt) : site_shape_uniform(p.B, p.N, p.Tp, p.W), a));
    if (a == 2) {  // a sample's query rows are consecutive and the samples follow each other: the chunked one-pass launch applies
        d.part = part;
        d.part_floats = attention_bwd_part_floats((long long)p.M, p.B, H, 64);
        d.part_rows = (long long)p.M;
    }
    return d;
}

namespace {

struct WG { const float* dY; const float* X; float* dW; float* db; };  // one weight-gradient product dW = dY^T X (+ db = colsum(dY))

// One backward call: what backward_impl validated, the modes it runs in, and the state its stages share.
struct BwdRun {
    SolaCtx* const c;
    const RagTables* const rt;  // null = a uniform batch
    const Arena& ar;
    const char* const fbase;    // the forward's workspace
    const hipStream_t s;
    hipStream_t s2 = s;         // the side lane's stream (lane_on, set by begin()), else s
    const Plan& p = c->last;
    const int B = p.B, N = p.N, Tp = p.Tp, M = p.M, Wn = p.W, L = p.L, D = c->cfg.lang_token_dim, H = c->cfg.num_heads;
    const int R = rt ? rt->NT : B * N;                    // tracks
    const int BW = rt ? (int)rt->LW : B * Wn;             // text ++ negative rows
    const SiteShape shape = rt ? site_shape_samples(*rt) : site_shape_uniform(B, N, Tp, Wn);  // the layers' units (sites.h)
    // ---- modes
    // split: every GEMM of the backward on 16-bit MFMAs - (hi, lo) operand pairs, three products (SP16), or plain f16 / bf16
    // operands, one product (mixed precision - activations, gradients and accumulation stay f32)
    const Elem opfmt = operand_format(c->precision);  // the step's GEMM operand format: forward and dX products
    const bool op16 = is_row16(opfmt), is_bf = opfmt == Elem::BF16;
    const OperandCast ocast{opfmt, s};  // the row-major casts into that format (ctx.h)
    const int k_unit = op16 ? 64 : 32;  // reduction lengths are whole k-tiles of the operands' kernels
    const bool split = opfmt != Elem::F32 && ar.present(S_DY_SP);
    // sola_tune "train_dw_f16": in the split-f16 step the weight-gradient products dW = dY^T X take PLAIN f16 operands (one MFMA per
    // product; a sum over all token rows, where the operand rounding averages out) while forward and dX keep the split pairs
    const bool dw16 = !op16 && g_train_dw_f16 != 0;
    const Elem dw_fmt = dw16 ? Elem::F16 : opfmt;  // the dW products' operand format (split steps only)
    const bool lane_on = !split && g_bwd_side_rows > 0 && M <= g_bwd_side_rows;  // dW products on c->side_stream (g_bwd_side_rows)
    const bool group = !split && !lane_on && ar.present(S_DWKEEP);  // deferred, grouped dW of the linear layers (g_bwd_group_rows)
    const bool gn16 = split && is_bf && g_train_bf16_store && g_bwd_fused_bf16_cast && g_bwd_dual_cast && D % 8 == 0;  // norms write their bf16 dx
    // ---- fixed scratch
    float* const tn = ar.get(S_TN);  // the dW kernels' slab scratch: touched by the side stream only (lane_on)
    float* const wt = ar.get(S_WT);
    float* const splitk_ws = ar.present(S_SPLITK) ? ar.get(S_SPLITK) : nullptr;
    const size_t tn_bytes = ar.bytes_from(S_TN), splitk_bytes = splitk_ws ? kSplitkFloats * sizeof(float) : 0;
    float *const dattn = ar.get(S_DATTN), *const dlang = ar.get(S_DLANG), *const dvec = ar.get(S_DVEC), *const egrad = ar.get(S_E), *const dwstd = ar.get(S_DWSTD);
    float* const gbuf[2] = {ar.get(S_G0), ar.get(S_G1)};
    float* enc[2] = {ar.get(S_ENC0), ar.get(S_ENC1)};
    // round 6 (SiteKeep::qkv16): a site whose attention backward wrote dq / dk / dv as bfloat16 rows itself.  [M][3D] lands at the start of
    // "dy_sp" - exactly where the fused statistics pass would have put its cast, so everything downstream of it is unchanged - and the
    // object -> language site's [BW][2D] key / value gradients in the buffer's second half (kv16: their own record in the cast cache, the dX
    // GEMM of dq still reads the first half when they are consumed)
    const size_t dy_sp_halfs = split ? 2 * (size_t)std::max(M, BW) * 3 * D : 0;
    unsigned short* const dy16 = split ? reinterpret_cast<unsigned short*>(ar.get(S_DY_SP)) : nullptr;
    unsigned short* const kv16 = split ? dy16 + dy_sp_halfs / 2 : nullptr;
    // ---- gradient chain
    int cur = 0;                                                                 // gbuf[cur]: the gradient wrt the current sub-block's output
    float *dres = ar.get(S_DRES), *dqkv = ar.get(S_DQKV), *dlkv = ar.get(S_DLKV);  // the arena's, or (group) what keep() hands every sub-block
    bool egrad_bf16 = false;    // the motion sub-block's backward left d(x_obj + pe) in `egrad` as bfloat16 rows (bf16 steps)
    bool dlang_init = false;
    const float* dy = nullptr;  // encoder: the current stage's output gradient
    bool enc_dy16 = false;      // ... which also sits in "dy_sp" as bfloat16 rows (written by the norm backward that produced it)
    // ---- operand-cast cache: what the shared cast buffers "dy_sp" / "wt_sp" hold for the next consumer.
    //   src / ld / cols  the f32 matrix whose row-major 16-bit rows start "dy_sp".  Filled by stats() (the fused bf16 cast, or rows a producer -
    //                    a norm or attention backward - wrote there); cleared by stats(may_cast), by grad_x when it casts another matrix
    //                    into "dy_sp", and by site_attention_bwd when the attention backward writes its bf16 gradients there.
    //   kv_src           the [BW][2D] matrix whose bf16 rows kv16 holds.  Filled by stats() over rows the attention backward wrote; cleared
    //                    by site_attention_bwd (site 2) in front of the launch and by site_o2l behind the text side's dX.
    //   wt_sp_ready      "wt_sp" holds the cast of the transposed weights of the next grad_x call.  Filled by transpose_into, cleared by grad_x.
    struct CastCache {
        const float* src = nullptr;
        int ld = 0, cols = 0;
        const float* kv_src = nullptr;
        bool wt_sp_ready = false;
        bool holds(const float* m, int ld_, int cols_) const { return src == m && ld == ld_ && cols == cols_; }
    } cast;
    // ---- statistics passes (split mode): every gradient matrix is read ONCE for its scale (max|dY|, shared by the dW and dX GEMMs that
    //      consume it) and its bias gradients (per-slab column sums, folded by a tiny second pass): stats() -> scale slot, bias_from_stats()
    float* const cpart_base = split ? ar.get(S_CPART) : nullptr;
    float *cpart = cpart_base, *cpart_next = cpart_base;  // the CURRENT pass's slab table (bumped per pass: they all stay until flush_bias)
    const size_t cpart_bytes = ar.bytes(S_CPART);
    int cpart_cols = 0, cpart_slabs = 0, stat_calls = 0;
    float* const scal = split ? ar.get(S_SCAL) : nullptr;
    const int scal_floats = split ? (int)scal_floats_of(c) : 0;
    ColsumJobsDesc bias_q{};  // deferred bias gradients of the current bucket
    // ---- few-sample backward
    float* keep_ptr = group ? ar.get(S_DWKEEP) : nullptr;  // keep(): the next private buffer for a gradient matrix a deferred product reads at the end
    float* gn_keep = (group && ar.present(S_GNKEEP)) ? ar.get(S_GNKEEP) : nullptr;  // ... and for the partials of a deferred GroupNorm backward
    GemmTnGroupDesc gq{};
    ColsumPairGroupDesc gn_q{};
    // round 5: the dX GEMMs read the weight matrices in their own row-major layout (GemmDesc::w_nn, the few-row kernel's NN form: the same
    // products in the same order as on a transposed copy) - the step's 49 weight transpositions (one grouped launch, 264 MB of traffic)
    // are gone.  transpose_into() records the matrices of the next product, grad_x() hands them over.
    const float* nn_w[3] = {nullptr, nullptr, nullptr};
    int nn_rows = 0;
    bool side_pending[4] = {false, false, false, false};
    // bf16 steps: operands of the current site's products that exist as bfloat16 rows ONLY - the forward's contract (SiteKeep), decided under
    // the switches of the forward.  dy16_only: dq / dk / dv of a qkv16 site (set by site_attention_bwd, cleared by the next site_head);
    // x16_only: the attention output of an o16 site (out_proj_bwd, around its weight gradient).  A product that would read their f32 rows
    // fails (need16) instead of reading a buffer nothing wrote.
    bool dy16_only = false, x16_only = false;

    BwdRun(SolaCtx* c_, const RagTables* rt_, const Arena& ar_, const void* fwd_workspace, hipStream_t s_)
        : c(c_), rt(rt_), ar(ar_), fbase(static_cast<const char*>(fwd_workspace)), s(s_) {}

    const float* fb(const std::string& name) const { return reinterpret_cast<const float*>(fbase + p.bufs.at(name).off); }
    const float* W(const std::string& name) const { return ctx_weight(c, name); }
    float* G(const std::string& name) const { return ctx_grad(c, name); }
    const float* ab(int l, int a, const char* what) const { return fb(abuf(true, l, kAttnShort[a], what)); }
    WG wg(const std::string& an, const char* proj, const float* dY, const float* X) const {
        return WG{dY, X, G(an + "." + proj + ".weight"), G(an + "." + proj + ".bias")};
    }

    // the 16-bit dW kernel takes the product and its scratch fits
    bool tns_fits(int rows, int n_out, int k_in, int nprob) const {
        return split && ar.present(S_TNS) && gemm_tn_split_supported(rows, n_out, k_in) &&
               ar.bytes_from(S_TNS) >= gemm_tn_split_scratch_bytes(rows, n_out, k_in, nprob);
    }

    int need16(bool ok, const char* what) const {
        SOLA_ARG(ok, "backward: %s exist as bf16 rows only, but this backward reads their f32 rows (a switch changed between the forward and the backward)", what);
        return SOLA_OK;
    }

    // ---- side lane.  dw_begin(): the side stream waits for everything the main stream has enqueued (the dY it reads); dw_end(slot): marks
    //      the side stream's progress for the buffer class `slot` (0 = dres, 1 = dqkv / dlkv, 2 = the encoder's dy, 3 = everything);
    //      wait_side(slot): the main stream waits for that mark before it overwrites the buffer.  `tn` (the dW kernels' slab scratch) is
    //      touched by the side stream only.
    int dw_begin() {
        if (!lane_on) return SOLA_OK;
        SOLA_HIP(hipEventRecord(c->ev_fork, s));
        SOLA_HIP(hipStreamWaitEvent(s2, c->ev_fork, 0));
        return SOLA_OK;
    }
    int dw_end(int slot) {
        if (!lane_on) return SOLA_OK;
        SOLA_HIP(hipEventRecord(c->ev_side[slot], s2));
        side_pending[slot] = true;
        return SOLA_OK;
    }
    int wait_side(int slot) {
        if (!lane_on || !side_pending[slot]) return SOLA_OK;
        SOLA_HIP(hipStreamWaitEvent(s, c->ev_side[slot], 0));
        side_pending[slot] = false;
        return SOLA_OK;
    }
    int join_side() {  // every gradient the side stream has been given is final for the main stream's next operation
        if (!lane_on) return SOLA_OK;
        SOLA_TRY(dw_end(3));
        SOLA_TRY(wait_side(3));
        side_pending[0] = side_pending[1] = side_pending[2] = false;
        return SOLA_OK;
    }

    // ---- deferred launches of the few-sample backward and of the bias sums
    float* keep(size_t floats) {
        float* q = keep_ptr;
        keep_ptr += (floats + 63) & ~(size_t)63;
        return q;
    }
    int flush_group() {
        if (gq.nprob == 0) return SOLA_OK;
        SOLA_TRY(launch_gemm_tn_group(gq, s));
        gq.nprob = 0;
        return SOLA_OK;
    }
    int next_group_prob(GemmTnGroupDesc::Prob** q) {  // a cleared entry of the grouped launch (a full table leaves first)
        if (gq.nprob == 32) SOLA_TRY(flush_group());
        *q = &gq.p[gq.nprob++];
        **q = GemmTnGroupDesc::Prob{};
        return SOLA_OK;
    }
    int flush_bias() {
        if (bias_q.n == 0) return SOLA_OK;
        SOLA_TRY(launch_colsum_jobs(bias_q, s));
        bias_q.n = 0;
        return SOLA_OK;
    }
    int flush_gn() {
        if (gn_q.n == 0) return SOLA_OK;
        SOLA_TRY(launch_colsum_pair_group(gn_q, s));
        gn_q.n = 0;
        return SOLA_OK;
    }

    // One statistics pass over dY[rows][cols] (pitch ld): *sc_out = its scale slot, or null when the mode or the shape takes none.
    // bf16 storage: the pass is the CAST as well (launch_cast_bf16_colsum: bfloat16 needs no scale, so no max|x| in front of the cast) -
    // "dy_sp" then holds the row-major bf16 copy at pitch ld, and the dW / dX GEMMs of the matrix skip theirs.
    // ready16: the producer already wrote dY's bfloat16 rows (same pitch) there - only the slab column sums are taken, from the 2-byte rows
    int stats(const float* dY, int ld, int rows, int cols, float** sc_out, bool may_cast = true, const void* ready16 = nullptr) {
        *sc_out = nullptr;
        if (may_cast) cast.src = nullptr;
        if (!split || cols % 4 || ld % 4) return SOLA_OK;
        cpart = cpart_next;  // this pass's own table
        cpart_next += (((size_t)((rows + 63) / 64) * cols) + 63) & ~(size_t)63;
        SOLA_ARG((size_t)(cpart_next - cpart_base) * sizeof(float) <= cpart_bytes, "backward: the slab tables of the step's statistics passes exceed their arena");
        // every call takes the next pair of the slots behind the 16 fixed ones: they were zeroed by ONE memset when the call began (a
        // memset of 8 bytes per gradient matrix was 20 launches of ~5 us per step)
        SOLA_ARG(16 + 2 * (stat_calls + 1) <= scal_floats, "backward: more gradient-statistics passes (%d) than scale slots", stat_calls + 1);
        float* sc = scal + 16 + 2 * stat_calls++;
        if (ready16) {
            SOLA_TRY(launch_colsum_slabs_bf16(ready16, ld, rows, cols, sc, cpart, s));
            if (ready16 == dy16) { cast.src = dY; cast.ld = ld; cast.cols = cols; }
            else cast.kv_src = dY;
        } else if (may_cast && is_bf && g_bwd_fused_bf16_cast && g_bwd_dual_cast && ld % 8 == 0 && (size_t)rows * ld <= dy_sp_halfs) {
            SOLA_TRY(launch_cast_bf16_colsum(dY, ld, ar.get(S_DY_SP), ld, rows, cols, sc, cpart, s));
            cast.src = dY; cast.ld = ld; cast.cols = cols;
        } else {
            SOLA_TRY(launch_amax_colsum(dY, ld, rows, cols, sc, cpart, s));
        }
        cpart_cols = cols;
        cpart_slabs = (rows + 63) / 64;
        *sc_out = sc;
        return SOLA_OK;
    }
    // deferred (round 6): the sums of a bucket's bias gradients leave in ONE launch in front of the bucket's event (flush_bias) - the same
    // per-column arithmetic as the per-gradient launch_colsum they replace
    int bias_from_stats(int col_off, int ncols, float* db) {
        if (bias_q.n == 48) SOLA_TRY(flush_bias());
        const int e = bias_q.n++;
        bias_q.in[e] = cpart + col_off; bias_q.out[e] = db; bias_q.rows[e] = cpart_slabs; bias_q.cols[e] = ncols; bias_q.ld[e] = cpart_cols;
        return SOLA_OK;
    }

    // dW[N_out, K_in] = dY^T X, db = colsum(dY): up to three weight gradients sharing rows / sizes / pitches (q, k, v of one attention): one launch on the split-f16
    // path (gemm_tn_split.hip) + the bias gradients as column sums, or the f32 kernel per problem
    // sc: scale slot from stats() over a matrix containing every dY of the call; db_done: the bias gradients were taken from it
    // dy_rm_done (optional, out): the call also left the ROW-MAJOR cast of the whole [rows][ldy] gradient matrix behind g[0].dY in
    // "dy_sp" (same scale): the dX GEMMs of the same matrix then skip their own cast (grad_x's `cast_done`)
    int grad_w_many(const WG* g, int n, int ldy, int ldx, int rows, int n_out, int k_in, float* sc = nullptr, bool db_done = false,
                    bool* dy_rm_done = nullptr) {
        if (dy_rm_done) *dy_rm_done = false;
        if (dy16_only || x16_only)  // neither the grouped nor the exact-f32 launch below reads bf16 rows
            SOLA_TRY(need16(!group && tns_fits(rows, n_out, k_in, n), "operands of a weight gradient"));
        if (group && n_out == D && k_in == D) {  // deferred: one grouped launch behind the layers (the dY buffers are private: keep())
            for (int j = 0; j < n; ++j) {
                GemmTnGroupDesc::Prob* q;
                SOLA_TRY(next_group_prob(&q));
                q->A = g[j].dY; q->B = g[j].X; q->C = g[j].dW; q->bias_grad = db_done ? nullptr : g[j].db;
                q->M = rows; q->N = n_out; q->K = k_in; q->lda = ldy; q->ldb = ldx;
            }
            return SOLA_OK;
        }
        if (!tns_fits(rows, n_out, k_in, n)) {
            GemmTnDesc d{};
            d.M = rows; d.N = n_out; d.K = k_in; d.lda = ldy; d.ldb = ldx; d.scratch = tn; d.scratch_bytes = tn_bytes;
            for (int j = 0; j < n; ++j) {
                d.A = g[j].dY; d.B = g[j].X; d.C = g[j].dW; d.bias_grad = g[j].db;
                SOLA_TRY(launch_gemm_tn(d, s2));
            }
            return SOLA_OK;
        }
        GemmTnSplitDesc d{};
        d.scal = sc; d.ab = d.b16_fmt = dw_fmt; d.rm_fmt = opfmt;
        if (dy_rm_done && sc && g_bwd_dual_cast) {
            d.a_rm = ar.get(S_DY_SP); d.a_rm_ld = ldy;
            d.a_rm_ready = cast.src && cast.src == g[0].dY && cast.ld == ldy && (g[n - 1].dY - g[0].dY) + n_out <= cast.cols;
        }
        if (cast.kv_src && cast.kv_src == g[0].dY && sc) {  // the attention backward's own bf16 rows of the key / value gradients
            d.a_rm = reinterpret_cast<float*>(kv16); d.a_rm_ld = ldy; d.a_rm_ready = 1;
        }
        d.nprob = n; d.M = rows; d.N = n_out; d.K = k_in; d.lda = ldy; d.ldb = ldx;
        for (int j = 0; j < n; ++j) {
            d.A[j] = g[j].dY; d.B[j] = g[j].X; d.C[j] = g[j].dW;
            if (is_row16(dw_fmt) && ldx == k_in) d.B16[j] = c->x16_find(g[j].X, k_in, dw_fmt);
        }
        d.scratch = ar.get(S_TNS); d.scratch_bytes = ar.bytes_from(S_TNS);
        // ... and of launch_gemm_tn_split's two routes only the row-major 16-bit kernel does
        if (dy16_only || x16_only) SOLA_TRY(need16(gemm_tn_split_takes_tr(d), "operands of a weight gradient"));
        if (dy16_only) SOLA_TRY(need16(d.a_rm_ready && gemm_tn_split_writes_rm(d), "the gradient rows of a weight gradient"));
        for (int j = 0; j < n && x16_only; ++j) SOLA_TRY(need16(d.B16[j] != nullptr, "the activation rows of a weight gradient"));
        if (dy_rm_done) *dy_rm_done = gemm_tn_split_writes_rm(d);
        SOLA_TRY(launch_gemm_tn_split(d, s));
        for (int j = 0; j < n && !db_done; ++j)
            if (g[j].db) SOLA_TRY(launch_colsum(g[j].dY, g[j].db, 1, rows, n_out, ldy, 1.f, 0, ar.get(S_COLSUM), ar.bytes_from(S_COLSUM), s));
        return SOLA_OK;
    }

    // dX[rows, k_in] = dY[rows, n_cat] * Wcat (+ Radd), where wt holds Wcat^T as [k_in][n_cat]
    // cast_done: "dy_sp" already holds the row-major cast of the [rows][ldy] matrix that dY - col_off starts (grad_w_many)
    // c16: dX leaves as bfloat16 rows (pitch k_in values)
    int grad_x(const float* dY, int ldy, int rows, int n_cat, int k_in, const float* Radd, float* dX, float* sc = nullptr,
               bool cast_done = false, int col_off = 0, bool c16 = false) {
        GemmDesc d{};
        d.nprob = 1;
        d.p[0] = GemmProblem{dY, wt, nullptr, Radd, dX};
        d.M = rows; d.N = k_in; d.K = n_cat; d.lda = ldy; d.ldr = k_in; d.ldc = k_in;
        d.splitk_ws = splitk_ws; d.splitk_bytes = splitk_bytes;
        if (group) {
            SOLA_ARG(nn_rows > 0 && n_cat % nn_rows == 0 && n_cat / nn_rows <= 3, "backward: dX product over %d columns of %d-row weight matrices", n_cat, nn_rows);
            for (int j = 0; j < n_cat / nn_rows; ++j) d.w_nn[j] = nn_w[j];
            d.w_nn_rows = nn_rows;
            d.p[0].W = nullptr;
            if (!gemm_nn_supported(d)) {  // outside the few-row shape: the transposed copy, as the many-row path
                d.w_nn_rows = 0;
                for (int j = 0; j < n_cat / nn_rows; ++j) SOLA_TRY(launch_transpose(nn_w[j], wt, nn_rows, k_in, k_in, n_cat, j * nn_rows, s));
                d.p[0].W = wt;
            }
        }
        if (split && n_cat % k_unit == 0 && ldy % 4 == 0) {
            // dY is cast with a data-dependent power-of-two scale (gradients sit mostly below the f16 normal range), the
            // transposed weights with the fixed 2^6; the epilogue undoes both
            float* sl = sc ? sc : scal;
            float* const dy_sp = ar.get(S_DY_SP);
            if (cast.kv_src && cast.kv_src == dY - col_off && sc) {
                d.p[0].A = reinterpret_cast<const float*>(kv16 + col_off);
                d.lda = ldy;
            } else if (cast_done && sc) {
                d.p[0].A = op16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(dy_sp) + col_off) : dy_sp + col_off;
                d.lda = ldy;
            } else {
                SOLA_TRY(need16(!dy16_only, "the gradient rows of an input gradient"));
                cast.src = nullptr;  // "dy_sp" is rewritten
                if (sc) SOLA_TRY(ocast.scaled(dY, ldy, dy_sp, rows, n_cat, sl));
                else SOLA_TRY(ocast.auto_scale(dY, ldy, dy_sp, rows, n_cat, sl));
                d.p[0].A = dy_sp;
                d.lda = n_cat;
            }
            if (!cast.wt_sp_ready) SOLA_TRY(ocast.fixed(wt, n_cat, ar.get(S_WT_SP), k_in, n_cat, kLinScale));  // else transpose_into wrote the operand itself
            cast.wt_sp_ready = false;
            d.p[0].W = ar.get(S_WT_SP);
            d.ab = opfmt; d.out_scale = 1.f / kLinScale; d.out_scale_dev = sl + 1;
            if (c16) d.c = opfmt;
        } else {
            SOLA_TRY(need16(!dy16_only, "the gradient rows of an input gradient"));
            SOLA_ARG(!c16, "backward: a bf16 input gradient needs the 16-bit GEMM");
        }
        return launch_gemm(d, s);
    }
    // block col_off of the [k_in][n_cat] transposed weights that the next grad_x reads: wt[k][col_off + n] = w[n][k]
    int transpose_into(const float* w, int n_out, int k_in, int n_cat, int col_off) {
        if (group) {  // no copy: grad_x reads the matrix where it lies
            SOLA_ARG(col_off % n_out == 0 && col_off / n_out < 3, "backward: weight block at column %d of %d-row matrices", col_off, n_out);
            nn_w[col_off / n_out] = w;
            nn_rows = n_out;
            return SOLA_OK;
        }
        if (split && n_cat % k_unit == 0) {  // grad_x's condition for the reduced-precision GEMM: the operand is written directly
            cast.wt_sp_ready = true;
            return launch_transpose_cast(w, ar.get(S_WT_SP), n_out, k_in, k_in, n_cat, col_off, kLinScale, opfmt, s);
        }
        return launch_transpose(w, wt, n_out, k_in, k_in, n_cat, col_off, s);
    }

    // GroupNorm backward: the caller fills x, dy, dy2, dx, the unit geometry and the flags; parameters, partials and their sums are added here
    int gn_bwd(GroupNormBwdDesc d, const std::string& wname) {
        d.gamma = W(wname + ".weight"); d.beta = W(wname + ".bias");
        d.dgamma_part = ar.get(S_GPART); d.dbeta_part = ar.get(S_BPART);
        d.eps = 1e-5f; d.slope = 0.01f;
        SOLA_TRY(wait_side(0));  // a GroupNorm backward writes dres (layers) or the encoder's next dy: the side stream's readers are done
        SOLA_TRY(wait_side(2));
        // round 5, few-sample backward: private partial buffers; the column sums of all norms of a bucket leave in ONE launch (flush_gn)
        const bool defer = group && d.n_inst <= 256 && gn_q.n < 16 && ar.present(S_GNKEEP);
        if (defer) {
            d.dgamma_part = gn_keep; gn_keep += ((size_t)d.n_inst * d.C + 63) & ~(size_t)63;
            d.dbeta_part = gn_keep; gn_keep += ((size_t)d.n_inst * d.C + 63) & ~(size_t)63;
        }
        SOLA_TRY(launch_group_norm_bwd(d, s));
        if (defer) {
            const int e = gn_q.n++;
            gn_q.in0[e] = d.dgamma_part; gn_q.in1[e] = d.dbeta_part; gn_q.out0[e] = G(wname + ".weight"); gn_q.out1[e] = G(wname + ".bias");
            gn_q.rows[e] = d.n_inst; gn_q.cols[e] = d.C;
            return SOLA_OK;
        }
        return launch_colsum_pair(d.dgamma_part, d.dbeta_part, G(wname + ".weight"), G(wname + ".bias"), d.n_inst, d.C, d.C, ar.get(S_COLSUM),
                                  ar.bytes_from(S_COLSUM), s);
    }

    // side lane and bucket events exist, the scale slots are zero
    int begin() {
        if (lane_on && !c->side_stream) {
            SOLA_HIP(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
            SOLA_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
            for (hipEvent_t& e : c->ev_side) SOLA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        if (lane_on) s2 = c->side_stream;
        if (split) SOLA_HIP(hipMemsetAsync(scal, 0, scal_floats * sizeof(float), s));
        // gradient-bucket events (ctx.h): created once, recorded as each bucket's last gradient kernel is enqueued
        if ((int)c->bucket_ev.size() != c->n_buckets()) {
            for (hipEvent_t e : c->bucket_ev) (void)hipEventDestroy(e);
            c->bucket_ev.assign(c->n_buckets(), nullptr);
            for (hipEvent_t& e : c->bucket_ev) SOLA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        c->bucket_recorded = false;
        return SOLA_OK;
    }

    int score_head(const float* d_score_map, const float* d_score_tokens) {
        HeadBwdDesc d{fb("l" + std::to_string(c->cfg.n_layers - 1) + "_o2l"), fb("lbar"), d_score_map, d_score_tokens, gbuf[cur],
                      ar.get(S_DLBAR_PART)};
        d.D = D;
        site_fill_head(d, shape);
        SOLA_TRY(launch_score_head_bwd(d, s));
        if (rt) return launch_segsum_rows(ar.get(S_DLBAR_PART), ar.get(S_DLBAR), rt->trk_off, B, D, s);
        return launch_colsum(ar.get(S_DLBAR_PART), ar.get(S_DLBAR), B, N, D, D, 1.f, 0, nullptr, 0, s);
    }

    // ---- what the three sites of a layer share -------------------------------------------------------------------------------------------------

    // GroupNorm backward of sub-block a: dres = d(pre-norm rows) from gbuf[cur] (site 0: + the d(x_obj + pe) the motion site left in egrad)
    int site_gn_bwd(int l, int a) {
        GroupNormBwdDesc d{};
        d.x = ab(l, a, "res"); d.dy = gbuf[cur]; d.dx = dres;
        d.C = D; d.groups = c->cfg.n_groups_module;
        site_fill_norm(d, shape.fam[a]);
        if (a == 2 && c->gn2_stats[l]) d.stats_in = fb("l" + std::to_string(l) + "_gn2st");
        if (a == 0) { d.dy2 = egrad; d.dy2_fmt = egrad_bf16 ? Elem::BF16 : Elem::F32; }
        // dx16 (round 6, bf16 steps): the norm's input gradient once more as bfloat16 rows - the consumer GEMMs' operand, written here instead of
        // by a statistics-and-cast pass that read the f32 matrix back (launch_cast_bf16_colsum); the f32 rows stay (residual stream)
        if (gn16) d.dx16 = dy16;
        d.x_fmt = c->site(l, a).res16 ? Elem::BF16 : Elem::F32;
        return gn_bwd(d, norm_name(l, a));
    }

    // common tail of every sub-block: out_proj backward  (res = resid + attn * Wo^T + bo): dWo, dbo, dattn = dres Wo
    // *g16_out (bf16 steps, train_bf16_store 3): d(attention output) left the GEMM as bfloat16 rows, which the attention backward reads - the
    // site's q / k / v are bf16 rows, its backward kernels take a bf16 dO, and the GEMM can write it
    int out_proj_bwd(int l, int a, bool* g16_out) {
        const bool g16 = *g16_out = split && is_bf && g_train_bf16_store >= 3 && c->site(l, a).qkv16 && attention_bwd_dout_bf16_enabled() &&
                                    D % 8 == 0 && D % k_unit == 0;
        SOLA_ARG(g16 || !c->site(l, a).o16,
                 "backward: attention output %d of layer %d exists as bf16 rows only, but this backward takes the f32 rows (a switch changed between the forward and the backward)", a, l);
        const std::string an = layer_prefix(l) + kAttnLong[a];
        const WG wo[1] = {wg(an, "out_proj", dres, ab(l, a, "attn"))};
        float* sc;
        bool rm;
        SOLA_TRY(dw_begin());
        x16_only = c->site(l, a).o16;  // the weight gradient's X: the kept bf16 rows (grad_w_many: x16_find)
        SOLA_TRY(stats_dw(wo, 1, D, M, gn16 ? dy16 : nullptr, true, &sc, &rm));  // gn16: the norm's backward in front of this wrote the bf16 rows
        x16_only = false;
        SOLA_TRY(dw_end(0));
        SOLA_TRY(transpose_into(W(an + ".out_proj.weight"), D, D, D, 0));
        return grad_x(dres, D, M, D, D, nullptr, dattn, sc, rm, 0, g16);
    }

    // the site's attention backward: dattn -> dq | dk | dv in dqkv (site 2: dq in dqkv, dk | dv in dlkv).  *s16_out: they left as bfloat16 rows
    // in "dy_sp" (the statistics passes behind this take them from there)
    int site_attention_bwd(int l, int a, bool g16, bool* s16_out) {
        AttnBwdDesc ad = attn_bwd_site_desc(c, p, rt, a, ar.get(S_ATTN_PART));
        ad.q = ab(l, a, "q"); ad.k = ab(l, a, a == 2 ? "lk" : "k"); ad.v = ab(l, a, a == 2 ? "lv" : "v");
        ad.o = ab(l, a, "attn"); ad.dout = dattn; ad.lse = ab(l, a, "lse");
        ad.dq = dqkv; ad.dk = a == 2 ? dlkv : dqkv + D; ad.dv = a == 2 ? dlkv + D : dqkv + 2 * D; ad.dvec = dvec;
        ad.drop = c->attn_drop(l, a);
        const bool s16 = *s16_out = split && c->site(l, a).qkv16;
        if (s16) {
            ad.io_fmt = Elem::BF16; ad.dq16 = dy16;
            if (a == 2) { ad.dk16 = kv16; ad.dv16 = kv16 + D; cast.kv_src = nullptr; }
            else { ad.dk16 = dy16 + D; ad.dv16 = dy16 + 2 * D; }
            cast.src = nullptr;
            ad.dout_fmt = g16 ? Elem::BF16 : Elem::F32;
            // the forward asked this of the same record (site16); "attn_bwd_fused" / "attn_bwd_small" may have changed since
            SOLA_TRY(need16(attention_bwd_bf16_supported(ad), "q / k / v of an attention site (the attention backward now takes another kernel)"));
            if (g16 && c->site(l, a).o16) {
                ad.o = static_cast<const float*>(c->x16_find(ab(l, a, "attn"), D, Elem::BF16));
                ad.o_fmt = Elem::BF16;
                SOLA_ARG(ad.o, "backward: the forward kept only the bf16 rows of attention output %d of layer %d, and they are not in the arena", a, l);
            }
        }
        SOLA_TRY(wait_side(1));  // dqkv / dlkv: the previous sub-block's weight gradients have read them
        dy16_only = s16;
        return launch_attention_bwd(ad, s);
    }

    // What every projection gradient of the layers goes through: ONE statistics pass over the n column blocks of D that g[0].dY starts (pitch
    // ld), their bias gradients from its slab sums, then the n weight gradients.  *sc: the matrix's scale slot (null: none was taken, and the
    // weight gradients' launch sums the biases itself); rm (optional): grad_w_many's dy_rm_done.  may_cast / ready16: as stats().
    int stats_dw(const WG* g, int n, int ld, int rows, const void* ready16, bool may_cast, float** sc, bool* rm) {
        SOLA_TRY(stats(g[0].dY, ld, rows, n * D, sc, may_cast, ready16));
        for (int j = 0; j < n && *sc; ++j) SOLA_TRY(bias_from_stats(j * D, D, g[j].db));
        return grad_w_many(g, n, ld, D, rows, D, D, *sc, *sc != nullptr, rm);
    }

    // in front of a site's projection gradients: private gradient buffers (group), then the backward of its norm, out-projection and attention
    int site_head(int l, int a, bool* s16) {
        if (group) { dres = keep((size_t)M * D); dqkv = keep((size_t)M * 3 * D); }
        if (group && a == 2) dlkv = keep((size_t)BW * 2 * D);
        bool g16;
        dy16_only = false;
        SOLA_TRY(site_gn_bwd(l, a));
        SOLA_TRY(out_proj_bwd(l, a, &g16));
        return site_attention_bwd(l, a, g16, s16);
    }

    // ---- the sites' own parts: operands of the weight gradients and the dX plan ----------------------------------------------------------

    // (iii) object -> language: x_o2l = GN2(x_mot + attn(q(x_mot), k(lang), v(lang)) Wo)
    int site_o2l(int l) {
        const std::string an = layer_prefix(l) + kAttnLong[2];
        bool s16, rmq;
        SOLA_TRY(site_head(l, 2, &s16));
        const WG wq[1] = {wg(an, "q_proj", dqkv, fb("l" + std::to_string(l) + "_motion"))};
        const WG wkv[2] = {wg(an, "k_proj", dlkv, fb("lang")), wg(an, "v_proj", dlkv + D, fb("lang"))};
        float *scq, *sckv;
        SOLA_TRY(dw_begin());
        SOLA_TRY(stats_dw(wq, 1, 3 * D, M, s16 ? dy16 : nullptr, true, &scq, &rmq));
        SOLA_TRY(stats_dw(wkv, 2, 2 * D, BW, s16 ? kv16 : nullptr, false, &sckv, nullptr));  // no fused cast: "dy_sp" holds dq's for the dX GEMM below
        SOLA_TRY(dw_end(1));
        SOLA_TRY(transpose_into(W(an + ".q_proj.weight"), D, D, D, 0));
        SOLA_TRY(grad_x(dqkv, 3 * D, M, D, D, dres, gbuf[1 - cur], scq, rmq));  // d x_mot = dres + dq Wq
        SOLA_TRY(transpose_into(W(an + ".k_proj.weight"), D, D, 2 * D, 0));
        SOLA_TRY(transpose_into(W(an + ".v_proj.weight"), D, D, 2 * D, D));
        SOLA_TRY(grad_x(dlkv, 2 * D, BW, 2 * D, D, dlang_init ? dlang : nullptr, dlang, sckv));  // the text side's [BW][2D]; accumulated over the layers
        cast.kv_src = nullptr;
        dlang_init = true;
        cur = 1 - cur;
        return SOLA_OK;
    }

    // (ii) motion: x_mot = GN1(x_obj + attn(q(x_obj+pe), k(x_obj+pe), v(x_obj)) Wo)
    int site_motion(int l) {
        const std::string an = layer_prefix(l) + kAttnLong[1], ls = "l" + std::to_string(l);
        bool s16, rm3;
        SOLA_TRY(site_head(l, 1, &s16));
        const float *x_pe = fb(ls + "_xpe"), *x_obj = fb(ls + "_obj");
        const WG w3[3] = {wg(an, "q_proj", dqkv, x_pe), wg(an, "k_proj", dqkv + D, x_pe), wg(an, "v_proj", dqkv + 2 * D, x_obj)};
        float* sc3;
        SOLA_TRY(dw_begin());
        SOLA_TRY(stats_dw(w3, 3, 3 * D, M, s16 ? dy16 : nullptr, true, &sc3, &rm3));
        SOLA_TRY(dw_end(1));
        SOLA_TRY(transpose_into(W(an + ".q_proj.weight"), D, D, 2 * D, 0));
        SOLA_TRY(transpose_into(W(an + ".k_proj.weight"), D, D, 2 * D, D));
        // (bf16 steps, train_bf16_store 3: this branch gradient leaves its GEMM as bfloat16 rows; the inter-object norm's backward adds it as dy2)
        egrad_bf16 = split && is_bf && g_train_bf16_store >= 3 && D % 8 == 0 && group_norm_bwd_dy2_bf16_supported(N, D, c->cfg.n_groups_module);
        SOLA_TRY(grad_x(dqkv, 3 * D, M, 2 * D, D, nullptr, egrad, sc3, rm3, 0, egrad_bf16));  // d(x_obj + pe) = dq Wq + dk Wk
        SOLA_TRY(transpose_into(W(an + ".v_proj.weight"), D, D, D, 0));
        SOLA_TRY(grad_x(dqkv + 2 * D, 3 * D, M, D, D, dres, gbuf[1 - cur], sc3, rm3, 2 * D));  // d x_obj (direct) = dres + dv Wv
        cur = 1 - cur;
        return SOLA_OK;
    }

    // (i) inter-object: x_obj = GN0(xin + attn(q,k,v(xin)) Wo); x_obj also feeds x_obj + pe
    int site_obj(int l) {
        const std::string an = layer_prefix(l) + kAttnLong[0];
        bool s16, rm3;
        SOLA_TRY(site_head(l, 0, &s16));
        const float* xin = l == 0 ? fb("conv5") : fb("l" + std::to_string(l - 1) + "_o2l");
        const WG w3[3] = {wg(an, "q_proj", dqkv, xin), wg(an, "k_proj", dqkv + D, xin), wg(an, "v_proj", dqkv + 2 * D, xin)};
        float* sc3;
        SOLA_TRY(dw_begin());
        SOLA_TRY(stats_dw(w3, 3, 3 * D, M, s16 ? dy16 : nullptr, true, &sc3, &rm3));
        SOLA_TRY(dw_end(1));
        SOLA_TRY(transpose_into(W(an + ".q_proj.weight"), D, D, 3 * D, 0));
        SOLA_TRY(transpose_into(W(an + ".k_proj.weight"), D, D, 3 * D, D));
        SOLA_TRY(transpose_into(W(an + ".v_proj.weight"), D, D, 3 * D, 2 * D));
        SOLA_TRY(grad_x(dqkv, 3 * D, M, 3 * D, D, dres, gbuf[1 - cur], sc3, rm3, 0));  // d xin = dres + [dq|dk|dv] [Wq;Wk;Wv]
        cur = 1 - cur;
        return SOLA_OK;
    }

    int layer(int l) {
        SOLA_TRY(site_o2l(l));
        SOLA_TRY(site_motion(l));
        SOLA_TRY(site_obj(l));
        dy16_only = false;
        if (l > 0) {
            SOLA_TRY(join_side());
            SOLA_TRY(flush_bias());  // the layer's deferred bias sums
            if (!group) SOLA_HIP(hipEventRecord(c->bucket_ev[c->cfg.n_layers - 1 - l], s));  // layer l's 30 gradients are final
        }
        return SOLA_OK;
    }

    // rows L.. of d(lang ++ neg) from the k/v projections + the mean-over-W of the score head
    int negative_tokens() {
        SOLA_TRY(launch_neg_token_grad(dlang, ar.get(S_DLBAR), nullptr, G("negative_token.weight"), B, L, c->cfg.n_negative, D, s,
                                       rt ? rt->u_lang : nullptr));
        SOLA_TRY(join_side());
        SOLA_TRY(flush_bias());
        SOLA_HIP(hipEventRecord(c->bucket_ev[c->cfg.n_layers - 1], s));  // layer 0 + negative tokens
        return SOLA_OK;
    }

    // ---- encoder -------------------------------------------------------------------------------------------------------------------------------

    struct EncStage {
        int i;
        const ConvGeom& g;
        int t_in, rows;      // input steps (the longest sequence's, ragged), output token rows
        long long rows_in;
        const int2* rowmap;  // ragged conv: per output row (ragged.h)
        const float* x;      // the conv's input rows
        float* scc;          // scale slot of this stage's dY (shared by its dW and dX GEMMs), null = none taken
    };

    // the conv as the dW product sees it: dW_std[cout][k*cin] = dY^T im2col(x)
    template <class Desc>
    static void conv_dw_geom(Desc& d, const EncStage& e, int t_out) {
        const ConvGeom& g = e.g;
        d.M = e.rows; d.N = g.cout; d.K = g.k * g.cin; d.lda = g.cout; d.ldb = g.cin;
        d.conv = g.k > 1 ? 1 : 0; d.T_in = e.t_in; d.T_out = t_out; d.stride = g.stride; d.pad = g.pad; d.Cin = g.cin;
        d.rowmap = e.rowmap;
    }

    // weight and bias gradient of conv i from dy
    int enc_dw(EncStage& e) {
        const ConvGeom& g = e.g;
        const int i = e.i;
        float* const dW = dwstd + c->ws_off[i];  // dwstd is laid out as the context's standardised weights
        float* const db = G(enc_name(kConvIdx[i]) + ".bias");
        if (tns_fits(e.rows, g.cout, g.k * g.cin, 1)) {
            SOLA_TRY(stats(dy, g.cout, e.rows, g.cout, &e.scc, true, enc_dy16 ? dy16 : nullptr));
            GemmTnSplitDesc d{};
            d.scal = e.scc; d.ab = d.b16_fmt = dw_fmt; d.rm_fmt = opfmt;
            d.nprob = 1; d.A[0] = dy; d.B[0] = e.x; d.C[0] = dW;
            conv_dw_geom(d, e, p.Tl[i]);
            d.B_rows = e.rows_in;
            if (cast.holds(dy, g.cout, g.cout)) { d.a_rm = ar.get(S_DY_SP); d.a_rm_ld = g.cout; d.a_rm_ready = 1; }
            if (is_row16(dw_fmt) && (i > 0 || is_bf)) d.B16[0] = c->x16_find(e.x, g.cin, dw_fmt);
            d.scratch = ar.get(S_TNS); d.scratch_bytes = ar.bytes_from(S_TNS);
            SOLA_TRY(launch_gemm_tn_split(d, s));
            if (e.scc) return bias_from_stats(0, g.cout, db);
            return launch_colsum(dy, db, 1, e.rows, g.cout, g.cout, 1.f, 0, ar.get(S_COLSUM), ar.bytes_from(S_COLSUM), s);
        }
        if (group) {  // deferred with the other few-sample weight gradients: dy stays intact (keep() in encoder_stage)
            GemmTnGroupDesc::Prob* q;
            SOLA_TRY(next_group_prob(&q));
            q->A = dy; q->B = e.x; q->C = dW; q->bias_grad = db;
            conv_dw_geom(*q, e, p.Tl[i]);
            return SOLA_OK;
        }
        GemmTnDesc d{};
        d.A = dy; d.B = e.x; d.C = dW; d.bias_grad = db;
        conv_dw_geom(d, e, p.Tl[i]);
        d.scratch = tn; d.scratch_bytes = tn_bytes;
        SOLA_TRY(dw_begin());
        SOLA_TRY(launch_gemm_tn(d, s2));
        return dw_end(2);
    }

    // input gradient of conv i (i >= 1) into dact: d act_{i-1}[(r, ti)][ci] = sum_{kk, co} dY[(r, to)][co] w_std[co][kk][ci]
    int enc_dx(const EncStage& e, float* dact) {
        const ConvGeom& g = e.g;
        const int i = e.i, rows = e.rows;
        const float* const w_std = c->ws_buf + c->ws_off[i];  // [cout][k*cin], where the forward left them
        auto col2im = [&](const float* zc, Elem z_fmt) -> int {
            if (rt) return launch_col2im_ragged(zc, dact, e.rows_in, rt->imap[i - 1], g.cin, g.k, g.stride, g.pad, z_fmt, s);
            return launch_col2im(zc, dact, R, e.t_in, p.Tl[i], g.cin, g.k, g.stride, g.pad, z_fmt, s);
        };
        // z = dY W over the OUTPUT rows in one GEMM (every tap's contribution; a strided conv's gather form would multiply zeros for every
        // skipped step), then the k taps are gathered into dX; a k = 1 conv's z is dX
        float* const zcol = ar.present(S_ZCOL) ? ar.get(S_ZCOL) : nullptr;
        GemmDesc zd{};
        zd.nprob = 1;
        zd.p[0] = GemmProblem{dy, nullptr, nullptr, nullptr, g.k > 1 ? zcol : dact};
        zd.M = rows; zd.N = g.k * g.cin; zd.K = g.cout; zd.lda = g.cout; zd.ldc = g.k * g.cin;
        // few-sample exact-f32 backward: the standardised weights are read where they lie ([cout][k*cin] row-major = the few-row kernel's NN
        // form: no transposed copy) - uniform batches too (their transposed-conv gather form multiplies twice the products for the stride-2
        // convs and ran on the 64x64 + split-K pair)
        GemmDesc nn = zd;
        nn.w_nn[0] = w_std; nn.w_nn_rows = g.cout;
        if (group && gemm_nn_supported(nn)) {
            SOLA_TRY(launch_gemm(nn, s));
            return g.k > 1 ? col2im(zcol, Elem::F32) : SOLA_OK;
        }
        if (split && g.cout % 128 == 0 && g.cin % 8 == 0 && (size_t)rows * g.cout <= std::max((size_t)M, (size_t)BW) * 3 * D) {
            float* sl = e.scc ? e.scc : scal;
            if (e.scc && cast.holds(dy, g.cout, g.cout)) {}  // the statistics pass left the cast (bf16)
            else if (e.scc) SOLA_TRY(ocast.scaled(dy, g.cout, ar.get(S_DY_SP), rows, g.cout, sl));
            else SOLA_TRY(ocast.auto_scale(dy, g.cout, ar.get(S_DY_SP), rows, g.cout, sl));
            if (op16) SOLA_TRY(launch_cast_f16_t(w_std, g.k * g.cin, ar.get(S_WT_SP), g.cout, g.cout, g.k * g.cin, nullptr, opfmt, s));
            else SOLA_TRY(launch_cast_sp16_t(w_std, g.k * g.cin, ar.get(S_WT_SP), g.cout, g.cout, g.k * g.cin, nullptr, s));
            zd.p[0].A = ar.get(S_DY_SP); zd.p[0].W = ar.get(S_WT_SP);
            zd.ab = opfmt; zd.out_scale = 1.f; zd.out_scale_dev = sl + 1;
            // bf16 steps (train_bf16_store): the per-tap contributions leave the GEMM as bfloat16 rows - the input gradient of a bf16 conv as
            // autocast computes it - and the gather sums the taps in f32: half the bytes written and read between the two launches
            zd.c = (is_bf && g_train_bf16_store >= 3 && g.k > 1 && (g.k * g.cin) % 8 == 0) ? Elem::BF16 : Elem::F32;
            SOLA_TRY(launch_gemm(zd, s));
            return g.k > 1 ? col2im(zcol, zd.c) : SOLA_OK;
        }
        if (rt) {  // ragged, exact f32: a plain GEMM on the concatenated rows, then the taps are gathered per sequence
            SOLA_TRY(launch_transpose(w_std, wt, g.cout, g.k * g.cin, g.k * g.cin, g.cout, 0, s));  // wt [k*cin][cout]
            zd.p[0].W = wt;
            zd.splitk_ws = splitk_ws; zd.splitk_bytes = splitk_bytes;
            SOLA_TRY(launch_gemm(zd, s));
            return g.k > 1 ? col2im(zcol, Elem::F32) : SOLA_OK;
        }
        // uniform, exact f32: the NT kernel with the transposed-conv gather over dY and the weights re-laid-out to [cin][kk*cout + co]
        for (int kk = 0; kk < g.k; ++kk)
            SOLA_TRY(launch_transpose(w_std + (size_t)kk * g.cin, wt, g.cout, g.cin, g.k * g.cin, g.k * g.cout, kk * g.cout, s));
        GemmDesc d{};
        d.nprob = 1;
        d.p[0] = GemmProblem{dy, wt, nullptr, nullptr, dact};
        d.M = R * e.t_in; d.N = g.cin; d.K = g.k * g.cout; d.lda = g.cout; d.ldc = g.cin;
        d.conv = g.k > 1 ? 2 : 0; d.T_in = p.Tl[i]; d.T_out = e.t_in; d.stride = g.stride; d.pad = g.pad; d.Cin = g.cout;
        d.splitk_ws = splitk_ws; d.splitk_bytes = splitk_bytes;
        return launch_gemm(d, s);
    }

    // conv i from dy (the gradient wrt its output): dW and db, then - above the first conv - dX and the GroupNorm + LeakyReLU backward of
    // stage i - 1, which leaves the next stage's dy
    int encoder_stage(int i) {
        const int t_in = i == 0 ? p.T : p.Tl[i - 1];
        EncStage e{i, c->conv[i], t_in, rt ? (int)rt->rows[i + 1] : R * p.Tl[i], rt ? rt->rows[i] : (long long)R * t_in,
                   (rt && c->conv[i].k > 1) ? rt->rowmap[i] : nullptr, i == 0 ? c->last_obj : fb("act" + std::to_string(i - 1)), nullptr};
        const ConvGeom& g = e.g;
        SOLA_TRY(enc_dw(e));
        if (i == 0) return SOLA_OK;
        float* dact = enc[0];
        SOLA_TRY(enc_dx(e, dact));
        if (group) enc[1] = keep((size_t)e.rows_in * g.cin);  // conv i-1's dY: read again by its deferred weight gradient
        // the next stage's statistics pass finds the bf16 rows ready when they fit "dy_sp", the pitch is 16-byte aligned and that stage takes
        // the 16-bit dW route (enc_dw's condition)
        enc_dy16 = gn16 && g.cin % 8 == 0 && (size_t)e.rows_in * g.cin <= dy_sp_halfs &&
                   tns_fits((int)e.rows_in, g.cin, c->conv[i - 1].k * c->conv[i - 1].cin, 1);
        GroupNormBwdDesc d{};
        d.x = fb("conv" + std::to_string(i - 1)); d.dy = dact; d.dx = enc[1];
        site_fill_norm(d, rt ? site_tracks(*rt, i) : site_tracks(R, t_in));
        d.C = g.cin; d.groups = c->cfg.n_groups; d.leaky = 1;
        d.drop = c->enc_drop(i - 1);
        if (enc_dy16) d.dx16 = dy16;
        SOLA_TRY(gn_bwd(d, enc_name(kNormIdx[i - 1])));
        dy = enc[1];  // dact (enc[0]) is consumed; the next stage's dX may overwrite it, its GN backward overwrites enc[1]
        return SOLA_OK;
    }

    // weight-standardisation backward for all six convs
    int ws_backward() {
        if (group) SOLA_TRY(flush_group());  // the encoder's deferred weight gradients
        SOLA_TRY(flush_gn());                // ... and its norms' parameter gradients
        SOLA_TRY(join_side());               // dwstd is the side stream's
        WsBwdLayer layers[6];
        for (int i = 0; i < 6; ++i) {
            const std::string cp = enc_name(kConvIdx[i]);
            layers[i] = WsBwdLayer{W(cp + ".weight"), dwstd + c->ws_off[i], G(cp + ".weight"), c->conv[i].cout, c->conv[i].cin, c->conv[i].k};
        }
        SOLA_TRY(launch_ws_backward(layers, 6, s));
        SOLA_TRY(flush_bias());
        SOLA_HIP(hipEventRecord(c->bucket_ev[c->cfg.n_layers], s));  // encoder
        c->bucket_recorded = true;
        return SOLA_OK;
    }

    int run(const float* d_score_map, const float* d_score_tokens) {
        SOLA_TRY(begin());
        SOLA_TRY(score_head(d_score_map, d_score_tokens));
        for (int l = c->cfg.n_layers - 1; l >= 0; --l) SOLA_TRY(layer(l));
        if (group) {  // the deferred weight gradients of every layer: one launch; all layer buckets are final behind it
            SOLA_TRY(flush_group());
            SOLA_TRY(flush_gn());  // the layers' norm parameter gradients
            for (int l = c->cfg.n_layers - 1; l > 0; --l) SOLA_HIP(hipEventRecord(c->bucket_ev[c->cfg.n_layers - 1 - l], s));
        }
        SOLA_TRY(negative_tokens());
        dy = gbuf[cur];  // gradient wrt conv5 output [R*T', D]
        for (int i = 5; i >= 0; --i) SOLA_TRY(encoder_stage(i));
        return ws_backward();
    }
};

}  // namespace

// want_rag: the caller is sola_backward_ragged (the last forward must have been sola_forward_train_ragged, in this workspace)
static int backward_impl(SolaCtx* c, const float* d_score_map, const float* d_score_tokens, const void* fwd_workspace,
                         void* scratch, size_t scratch_bytes, void* stream_, bool want_rag) {
    SOLA_ARG(c && d_score_map && d_score_tokens && fwd_workspace && scratch, "backward: null argument");
    const Plan& p = c->last;
    if (!p.train || p.M == 0) {
        sola_set_error("backward: the last forward on this context was not sola_forward_train%s", want_rag ? "_ragged" : "");
        return SOLA_ERR_STATE;
    }
    if (p.rag != want_rag) {
        sola_set_error("backward: the last training forward was %s - call %s", p.rag ? "ragged" : "uniform", p.rag ? "sola_backward_ragged" : "sola_backward");
        return SOLA_ERR_STATE;
    }
    if (p.rag && fwd_workspace != c->last_ws) {
        sola_set_error("backward_ragged: not the workspace of the last sola_forward_train_ragged (its unit tables live there)");
        return SOLA_ERR_STATE;
    }
    const RagTables* const rt = p.rag ? &c->last_rag : nullptr;
    for (const Weight& w : c->weights)
        if (!w.grad && w.name != "positional_encoding_gaussian_matrix") {
            sola_set_error("backward: no gradient buffer registered for '%s'", w.name.c_str());
            return SOLA_ERR_WEIGHT;
        }
    Arena ar = make_arena(c, rt ? sizes_of_ragged(*rt) : sizes_of(p));
    if (scratch_bytes < ar.total) {
        sola_set_error("backward: scratch %zu bytes < required %zu", scratch_bytes, ar.total);
        return SOLA_ERR_WORKSPACE;
    }
    SOLA_ARG((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "backward: scratch must be 256-byte aligned");
    ar.base = static_cast<char*>(scratch);
    return BwdRun(c, rt, ar, fwd_workspace, as_stream(stream_)).run(d_score_map, d_score_tokens);
}

extern "C" int sola_backward(SolaCtx* c, const float* d_score_map, const float* d_score_tokens, const void* fwd_workspace,
                             void* scratch, size_t scratch_bytes, void* stream_) {
    try {
        return backward_impl(c, d_score_map, d_score_tokens, fwd_workspace, scratch, scratch_bytes, stream_, false);
    } catch (const std::exception& e) {
        sola_set_error("backward: %s", e.what());
        return SOLA_ERR_ARG;
    }
}

extern "C" int sola_backward_ragged(SolaCtx* c, const float* d_score_map, const float* d_score_tokens, const void* fwd_workspace,
                                    void* scratch, size_t scratch_bytes, void* stream_) {
    try {
        return backward_impl(c, d_score_map, d_score_tokens, fwd_workspace, scratch, scratch_bytes, stream_, true);
    } catch (const std::exception& e) {
        sola_set_error("backward_ragged: %s", e.what());
        return SOLA_ERR_ARG;
    }
}

extern "C" int sola_grad_bucket_count(const SolaCtx* c) { return c ? c->n_buckets() : 0; }

// bucket of a parameter: layers in reverse order, then layer 0 together with the negative tokens, then the encoder
extern "C" int sola_grad_bucket_of(const SolaCtx* c, const char* name) {
    SOLA_ARG(c && name, "grad_bucket_of: null argument");
    const std::string n(name);
    if (c->index.find(n) == c->index.end() || n == "positional_encoding_gaussian_matrix") {
        sola_set_error("grad_bucket_of: '%s' is not a parameter", name);
        return SOLA_ERR_WEIGHT;
    }
    const std::string lp = "object_lang_align_layers.";
    if (n.compare(0, lp.size(), lp) == 0) return c->cfg.n_layers - 1 - atoi(n.c_str() + lp.size());
    if (n == "negative_token.weight") return c->cfg.n_layers - 1;
    return c->cfg.n_layers;
}

extern "C" int sola_backward_wait_bucket(SolaCtx* c, int bucket, void* stream_) {
    SOLA_ARG(c && bucket >= 0 && bucket < c->n_buckets(), "backward_wait_bucket: bucket %d out of range", bucket);
    if (!c->bucket_recorded) {
        sola_set_error("backward_wait_bucket: no completed sola_backward on this context");
        return SOLA_ERR_STATE;
    }
    SOLA_HIP(hipStreamWaitEvent(as_stream(stream_), c->bucket_ev[bucket], 0));
    return SOLA_OK;
}
