// Multi-scale deformable attention, forward (Deformable-DETR's operator; GroundingDINO's one custom op,
// groundingdino._C.ms_deform_attn_forward; Mask2Former's pixel decoder).  The contract is in sola_hip.h.
//
// One thread owns 4 consecutive channels of one (batch, query, head) output: D / 4 lanes (4, 8 or 16) share a unit, read the
// same locations and weights (one address for the whole group) and together fetch one head's row of a corner, D * 4 bytes
// - at D = 32 one 128-byte line per 8 lanes, 8 corners of 8 units per 16-byte load instruction of a wave.  The sum is kept in
// registers in the fixed (level, point, corner) order and stored once, 16 bytes per lane: no atomics, no LDS, no workspace.
//
// Blocks: head-major.  The N * chunks blocks of head 0 come first, each 256 / (D / 4) consecutive queries of one batch element,
// then head 1's: consecutive blocks are neighbouring queries of ONE head and, dealt round-robin over the 8 XCDs (observed, not
// promised), every XCD works on every head.  The other order (head = block % M: with M = 8 the blocks of a head share an XCD,
// whose L2 then holds that head's maps alone, S * 128 bytes = 2.8 MB for an 800 x 1333 image) was measured and lost on the
// encoder shape: 103 against 88 us with locations near the query's own pixel, 106 against 98 us with uniform ones; it won
// 2 us of 25 on the 900-query decoder shape (profiles/msda_bench.txt).  Nothing depends on the placement.
//
// Bounds.  The level table lives on the device and is not trusted.  A level counts only with 1 <= H, W <= 2^30 and a start in
// (-2^62, S); the integer corner is taken from a float clamped to [-2, 2^30], so the conversion is defined for every
// location (NaN included) and a clamped corner is outside its map.  A corner counts when it is inside the map AND its row
// start + y * W + x (64-bit) is in [0, S).  Rows are fetched through a buffer descriptor of exactly one batch element's
// S * M * D * 4 bytes (< 2^31, the host refuses more); a corner that does not count gets the offset 2^31, which the
// descriptor's range check answers with zeros without touching memory - a second fence behind the explicit test.
#include "kernels.h"

namespace {

constexpr int MSDA_THREADS = 256;
constexpr unsigned MSDA_NO_ROW = 0x80000000u;  // past every descriptor: num_records < 2^31
constexpr long long MSDA_MAX_SIDE = 1ll << 30;

struct MsdaArgs {
    const float* value;
    const long long* shapes;  // [L, 2] = (H, W)
    const long long* start;   // [L]
    const float* loc;
    const float* weight;
    float* out;
    int N, S, M, Lq, L, P;
    int chunks;  // query chunks of a (batch, head)
};

struct MsdaLevel {
    int H, W;
    long long start;
    float Hf, Wf;
    bool ok;
};

__device__ __forceinline__ MsdaLevel msda_level(const MsdaArgs& a, int l) {
    const long long H = a.shapes[2 * l], W = a.shapes[2 * l + 1], st = a.start[l];
    MsdaLevel v;
    v.ok = H >= 1 && W >= 1 && H <= MSDA_MAX_SIDE && W <= MSDA_MAX_SIDE && st < (long long)a.S && st > -(1ll << 62);
    v.H = (int)H; v.W = (int)W; v.start = st;
    v.Hf = (float)v.H; v.Wf = (float)v.W;
    return v;
}

// The four corners of one sampling point: byte offsets into the batch element's value (MSDA_NO_ROW where the corner does not
// count) and the bilinear weights, in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1).
struct MsdaPoint {
    unsigned off[4];
    float c[4];
};

__device__ __forceinline__ MsdaPoint msda_point(const MsdaLevel& lv, float loc_x, float loc_y, int S, unsigned row_bytes, unsigned lane_bytes) {
    const float x = __builtin_fmaf(loc_x, lv.Wf, -0.5f), y = __builtin_fmaf(loc_y, lv.Hf, -0.5f);
    const float x0f = floorf(x), y0f = floorf(y);
    const float lx = x - x0f, ly = y - y0f, hx = 1.f - lx, hy = 1.f - ly;
    // fmaxf drops a NaN operand: the conversion below is defined for every input
    const int x0 = (int)fminf(fmaxf(x0f, -2.f), (float)MSDA_MAX_SIDE), y0 = (int)fminf(fmaxf(y0f, -2.f), (float)MSDA_MAX_SIDE);
    MsdaPoint pt;
    pt.c[0] = hy * hx; pt.c[1] = hy * lx; pt.c[2] = ly * hx; pt.c[3] = ly * lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
        const long long row = lv.start + (long long)yy * lv.W + xx;  // |yy * W + xx| < 2^61
        const bool in = (unsigned)yy < (unsigned)lv.H && (unsigned)xx < (unsigned)lv.W && (unsigned long long)row < (unsigned long long)S;
        pt.off[k] = in ? (unsigned)row * row_bytes + lane_bytes : MSDA_NO_ROW;
    }
    return pt;
}

__device__ __forceinline__ f32x4 msda_row(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
}

// acc += w * (c0 v0 + c1 v1 + c2 v2 + c3 v3), every step one fused multiply-add, in this order
__device__ __forceinline__ f32x4 msda_add(f32x4 acc, float w, const MsdaPoint& pt, const f32x4 (&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s = pt.c[0] * v[0][e];
        s = __builtin_fmaf(pt.c[1], v[1][e], s);
        s = __builtin_fmaf(pt.c[2], v[2][e], s);
        s = __builtin_fmaf(pt.c[3], v[3][e], s);
        acc[e] = __builtin_fmaf(w, s, acc[e]);
    }
    return acc;
}

// P4: P == 4 with 16-byte aligned weights - a level's locations are two 16-byte loads and its weights one, and the 16 row
// loads of a level are in flight together.  Otherwise any P: 8-byte location loads, one point at a time.
template <int D, bool P4>
__global__ __launch_bounds__(MSDA_THREADS) void msda_fwd_kernel(const MsdaArgs a) {
    constexpr int LANES = D / 4, UNITS = MSDA_THREADS / LANES;
    const unsigned b = blockIdx.x;
    const unsigned per_head = (unsigned)a.N * (unsigned)a.chunks;
    const int m = (int)(b / per_head);
    const unsigned r = b - (unsigned)m * per_head;
    const int chunk = (int)(r % (unsigned)a.chunks), n = (int)(r / (unsigned)a.chunks);
    const int tid = threadIdx.x;
    const int q = chunk * UNITS + tid / LANES;
    const unsigned row_bytes = (unsigned)a.M * D * 4u;
    const unsigned lane_bytes = ((unsigned)m * D + (unsigned)(tid % LANES) * 4u) * 4u;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.value) + (long long)n * a.S * a.M * D, 0, a.S * (int)row_bytes, 0x00020000);
    if (q >= a.Lq) return;
    const int unit = (n * a.Lq + q) * a.M + m;  // < 2^31 / (2 L P)
    const float* loc = a.loc + (long long)unit * (a.L * a.P * 2);
    const float* wgt = a.weight + (long long)unit * (a.L * a.P);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < a.L; ++l) {
        const MsdaLevel lv = msda_level(a, l);
        if (!lv.ok) continue;  // uniform
        if constexpr (P4) {
            const float4 xy01 = reinterpret_cast<const float4*>(loc)[2 * l], xy23 = reinterpret_cast<const float4*>(loc)[2 * l + 1];
            const float4 w4 = reinterpret_cast<const float4*>(wgt)[l];
            const float px[4] = {xy01.x, xy01.z, xy23.x, xy23.z}, py[4] = {xy01.y, xy01.w, xy23.y, xy23.w};
            const float pw[4] = {w4.x, w4.y, w4.z, w4.w};
            MsdaPoint pt[4];
            f32x4 v[4][4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                pt[p] = msda_point(lv, px[p], py[p], a.S, row_bytes, lane_bytes);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[p][k] = msda_row(rs, pt[p].off[k]);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) acc = msda_add(acc, pw[p], pt[p], v[p]);
        } else {
            for (int p = 0; p < a.P; ++p) {
                const float2 xy = reinterpret_cast<const float2*>(loc)[l * a.P + p];
                const float w = wgt[l * a.P + p];
                const MsdaPoint pt = msda_point(lv, xy.x, xy.y, a.S, row_bytes, lane_bytes);
                f32x4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = msda_row(rs, pt.off[k]);
                acc = msda_add(acc, w, pt, v);
            }
        }
    }
    *reinterpret_cast<f32x4*>(a.out + (long long)unit * D + (tid % LANES) * 4) = acc;
}

template <int D>
void msda_launch(const MsdaArgs& a, bool p4, unsigned blocks, hipStream_t s) {
    if (p4) hipLaunchKernelGGL((msda_fwd_kernel<D, true>), dim3(blocks), dim3(MSDA_THREADS), 0, s, a);
    else hipLaunchKernelGGL((msda_fwd_kernel<D, false>), dim3(blocks), dim3(MSDA_THREADS), 0, s, a);
}

}  // namespace

int launch_ms_deform_attn(const float* value, const int64_t* shapes, const int64_t* start, const float* loc, const float* weight, int N,
                          int S, int M, int D, int Lq, int L, int P, float* out, hipStream_t s) {
    SOLA_ARG(N >= 1 && S >= 1 && M >= 1 && Lq >= 1, "ms_deform_attn: N %d, S %d, M %d, Lq %d must all be >= 1", N, S, M, Lq);
    SOLA_ARG(D == 16 || D == 32 || D == 64, "ms_deform_attn: D = %d channels per head, supported are 16, 32 and 64", D);
    SOLA_ARG(L >= 1 && L <= SOLA_MSDA_MAX_LEVELS, "ms_deform_attn: L = %d levels, supported are 1 to %d", L, SOLA_MSDA_MAX_LEVELS);
    SOLA_ARG(P >= 1 && P <= SOLA_MSDA_MAX_POINTS, "ms_deform_attn: P = %d points, supported are 1 to %d", P, SOLA_MSDA_MAX_POINTS);
    SOLA_ARG(value && shapes && start && loc && weight && out, "ms_deform_attn: null argument");
    const long long lim = 1ll << 31;
    const long long row = (long long)M * D;
    SOLA_ARG(row * 4 < lim && (long long)S * row * 4 < lim,
             "ms_deform_attn: one batch element's value is S*M*D*4 = %lld bytes, the 32-bit row offsets take fewer than 2^31", (long long)S * row * 4);
    SOLA_ARG((long long)N * S * row < lim, "ms_deform_attn: value has N*S*M*D = %lld elements, at most 2^31 - 1", (long long)N * S * row);
    const long long units = (long long)N * Lq * M;
    SOLA_ARG(units < lim && units * L * P * 2 < lim, "ms_deform_attn: sampling_locations has N*Lq*M*L*P*2 = %lld elements, at most 2^31 - 1",
             units * L * P * 2);
    SOLA_ARG(units * D < lim, "ms_deform_attn: the output has N*Lq*M*D = %lld elements, at most 2^31 - 1", units * D);
    SOLA_ARG(((reinterpret_cast<uintptr_t>(value) | reinterpret_cast<uintptr_t>(loc) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
             "ms_deform_attn: value, sampling_locations and the output must be 16-byte aligned");
    SOLA_ARG((reinterpret_cast<uintptr_t>(weight) & 3) == 0 && ((reinterpret_cast<uintptr_t>(shapes) | reinterpret_cast<uintptr_t>(start)) & 7) == 0,
             "ms_deform_attn: attention_weights must be 4-byte aligned, the level tables 8-byte aligned");
    MsdaArgs a{};
    a.value = value; a.shapes = reinterpret_cast<const long long*>(shapes); a.start = reinterpret_cast<const long long*>(start);
    a.loc = loc; a.weight = weight; a.out = out;
    a.N = N; a.S = S; a.M = M; a.Lq = Lq; a.L = L; a.P = P;
    const int units_per_block = MSDA_THREADS / (D / 4);
    a.chunks = (Lq + units_per_block - 1) / units_per_block;
    const long long blocks = (long long)N * M * a.chunks;  // <= units
    const bool p4 = P == 4 && (reinterpret_cast<uintptr_t>(weight) & 15) == 0;
    if (D == 16) msda_launch<16>(a, p4, (unsigned)blocks, s);
    else if (D == 32) msda_launch<32>(a, p4, (unsigned)blocks, s);
    else msda_launch<64>(a, p4, (unsigned)blocks, s);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
