// A uniform channels-last conv over few output frames as plain GEMMs, one problem per frame (kernels.h: ConvFramePlan).  Host code
// only: the launches are ordinary launch_gemm calls on pitched operands.
//
// Why: the implicit-im2col launch gives every output row all k taps and reads zeros for those in the padding.  Over T' = 4 frames
// of a k = 3 / pad 1 conv that is 2 of 12 tap products - a sixth of the launch - and because a 256-row tile mixes the frames of many
// tracks, no k-tile of it can be dropped inside the kernel.  Per frame the inside taps are one contiguous window, so the padding
// taps vanish as whole k-tiles of whole launches.
//
// Same bits: both forms add the same non-zero k-chunks to an accumulator in the same order (three MFMAs per 16-wide chunk, f32).
// What the per-frame form leaves out are whole taps - Cin is a multiple of the 32-wide k-tile - in which every product of the row
// is weight x (+0): an exact zero for FINITE weights, added to an accumulator that is +0 at the start (a leading tap) or unchanged
// by it (a trailing tap).  A NaN or infinite weight in a padding tap would reach the output of the conv launch only.  It holds
// where neither form splits K: the launches here carry no split-K scratch, and the forward takes the form only where every launch
// runs on the persistent direct-to-LDS kernel (conv_frames_pays).
#include <algorithm>

#include "kernels.h"

extern int g_gemm_glds, g_gemm_glds_force, g_gemm_persist;
bool gemm_split_glds_supported(const GemmDesc& d);
int gemm_split_glds_shape(const GemmDesc& d);

namespace {

constexpr int KTILE = 32;  // the direct-to-LDS kernels' k-tile (gemm_glds.h: GBK)

// frame t of the plan's launch li, problem j, as a plain GEMM problem of `g`
GemmDesc frame_launch(const GemmDesc& conv, const ConvFrameLaunch& L, const ConvTapWeights* w) {
    const int taps_all = conv.K / conv.Cin;
    const int tracks = conv.M / conv.T_out;
    GemmDesc g = conv;
    g.conv = 0; g.T_in = g.T_out = g.stride = g.pad = g.Cin = 0;
    g.rowmap = nullptr;
    g.nprob = L.nprob;
    g.M = tracks;
    g.K = L.taps * conv.Cin;
    g.lda = conv.T_in * conv.Cin;
    g.ldc = conv.T_out * conv.ldc;
    g.splitk_ws = nullptr; g.splitk_bytes = 0;  // never split K: the accumulation order is the conv launch's
    for (int j = 0; j < L.nprob; ++j) {
        const int t = L.frame[j], lo = L.lo[j];
        GemmProblem p = conv.p[0];
        p.A = conv.p[0].A + ((long long)t * conv.stride - conv.pad + lo) * conv.Cin;
        p.W = L.taps == taps_all ? conv.p[0].W : (w ? w->find(lo, lo + L.taps - 1) : nullptr);
        p.C = conv.p[0].C + (long long)t * conv.ldc;
        g.p[j] = p;
    }
    return g;
}

// launch_gemm's routing (gemm.hip), restated for one question: does this split-f16 launch run on the persistent 256x256 kernel
bool takes_persist256(const GemmDesc& d) {
    const long long t128 = (long long)((d.M + 127) / 128) * ((d.N + 127) / 128) * d.nprob;
    const bool big = t128 >= 512;
    return d.ab == Elem::SP16 && d.ksplit <= 1 && (big || g_gemm_glds_force) && g_gemm_glds && gemm_split_glds_supported(d) &&
           gemm_split_glds_shape(d) == 4 && g_gemm_persist && d.K / KTILE >= 2;
}

long long rounds_256(const GemmDesc& d) {
    const long long tiles = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256) * d.nprob;
    const int cus = sola_cu_count();
    return (tiles + cus - 1) / cus;
}

}  // namespace

bool conv_frames_plan(const GemmDesc& conv, ConvFramePlan& plan) {
    plan.n = 0;
    if (conv.conv != 1 || conv.rowmap || conv.ab != Elem::SP16 || conv.nprob != 1 || conv.p[0].R || conv.ksplit > 1 || conv.gn_gamma) return false;
    if (conv.Cin <= 0 || conv.Cin % KTILE != 0 || conv.K % conv.Cin != 0) return false;
    if (conv.T_out < 1 || conv.T_out > 5 || conv.T_in < 1 || conv.stride < 1 || conv.M % conv.T_out != 0) return false;
    const int k = conv.K / conv.Cin;
    int lo[5], taps[5];
    for (int t = 0; t < conv.T_out; ++t) {
        const int t0 = t * conv.stride - conv.pad;
        lo[t] = std::max(0, -t0);
        const int hi = std::min(k - 1, conv.T_in - 1 - t0);
        if (hi < lo[t]) return false;  // a frame that sees padding only: bias rows, no GEMM
        taps[t] = hi - lo[t] + 1;
    }
    // classes by tap count, fewest launches: frames in ascending order, three per launch
    for (int n_taps = k; n_taps >= 1; --n_taps) {
        ConvFrameLaunch* L = nullptr;
        for (int t = 0; t < conv.T_out; ++t) {
            if (taps[t] != n_taps) continue;
            if (!L || L->nprob == 3) {
                L = &plan.l[plan.n++];
                L->nprob = 0;
                L->taps = n_taps;
            }
            L->frame[L->nprob] = t;
            L->lo[L->nprob] = lo[t];
            ++L->nprob;
        }
    }
    return true;
}

bool conv_frames_pays(const GemmDesc& conv, const ConvFramePlan& plan) {
    if (plan.n == 0 || !takes_persist256(conv)) return false;
    long long cost = 0;
    for (int i = 0; i < plan.n; ++i) {
        const GemmDesc g = frame_launch(conv, plan.l[i], nullptr);
        if (!takes_persist256(g)) return false;
        cost += rounds_256(g) * g.K;
    }
    return 16 * cost <= 15 * rounds_256(conv) * conv.K;
}

bool conv_frames_has_weights(const GemmDesc& conv, const ConvFramePlan& plan, const ConvTapWeights& w) {
    for (int i = 0; i < plan.n; ++i) {
        const GemmDesc g = frame_launch(conv, plan.l[i], &w);
        for (int j = 0; j < g.nprob; ++j)
            if (!g.p[j].W) return false;
    }
    return plan.n > 0;
}

int launch_conv_frames(const GemmDesc& conv, const ConvFramePlan& plan, const ConvTapWeights& w, hipStream_t s) {
    SOLA_ARG(conv_frames_has_weights(conv, plan, w), "conv_frames: no per-frame form, or a tap range without its packed weights");
    for (int i = 0; i < plan.n; ++i) SOLA_TRY(launch_gemm(frame_launch(conv, plan.l[i], &w), s));
    return SOLA_OK;
}
