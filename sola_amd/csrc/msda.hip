// Multi-scale deformable attention, forward and backward (Deformable-DETR's operator; GroundingDINO's one custom op,
// groundingdino._C.ms_deform_attn_forward / _backward; Mask2Former's pixel decoder).  The contracts are in sola_hip.h.
//
// Forward.  One thread owns 4 consecutive channels of one (batch, query, head) output: D / 4 lanes (4, 8 or 16) share a unit, read the
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

// ---- backward -----------------------------------------------------------------------------------------------------------------
// One lane owns ONE channel of a (batch, query, head) unit: D lanes (16, 32 or 64) share a unit, 256 / D units a block, blocks in the
// forward's order.  Not the forward's 4 channels per lane: the scatter into grad_value is float32 atomic adds, which run at one
// chip-wide byte rate when a wave-instruction is one dword per lane over whole rows (256 contiguous bytes at D = 64, two 128-byte
// rows at D = 32, four 64-byte rows at D = 16) - and on the encoder shape they are 1.46 GB, 13 times the forward's whole runtime at
// that rate, so the lane layout follows the atomics.  Measured (profiles/msda_bwd_bench.txt): 1.15 - 1.19 TB/s of adds on the encoder
// shape, 89 - 92 % of the chip's rate, at D = 16 and 64 the same within a tenth; the forward's layout (four adds per lane, lanes 16
// bytes apart) 0.30 TB/s.
//
// grad_loc and grad_weight: the unit that owns the element sums its D per-channel terms with the xor butterfly of common.h in the
// fixed order (32, 16, 8, 4, 2, 1 from D down) and its first lane stores it once; a dead level's entries are stored as zeros.
// Same bits on every run and stream, and with or without the other outputs (no multiply-add is left to the compiler to fuse).
// grad_value: one add per counting corner and channel, w * g_d first, then times the corner's coefficient; arrival order is
// the hardware's, so its last bits are NOT repeatable.  The explicit row test of msda_point guards every add; rows are read
// through the forward's range-checked descriptor.
struct MsdaBwdArgs {
    MsdaArgs f;  // out unused
    const float* grad_out;
    float* grad_value;   // zeroed by the launcher; null = not wanted, like the next two
    float* grad_loc;
    float* grad_weight;
};

// Sum over the D lanes of a unit (aligned groups of a wave), the same bits in each of them.
template <int D>
__device__ __forceinline__ float msda_unit_sum(float v) {
#pragma clang fp contract(off)
    if constexpr (D == 64) v = sum_xor32(v);
    if constexpr (D >= 32) v = sum_xor16(v);
    return sum_xor1(sum_xor2(sum_xor4(sum_xor8(v))));
}

template <int D, bool GV>
__global__ __launch_bounds__(MSDA_THREADS) void msda_bwd_kernel(const MsdaBwdArgs b) {
#pragma clang fp contract(off)
    constexpr int UNITS = MSDA_THREADS / D;
    const MsdaArgs& a = b.f;
    const unsigned blk = blockIdx.x;
    const unsigned per_head = (unsigned)a.N * (unsigned)a.chunks;
    const int m = (int)(blk / per_head);
    const unsigned r = blk - (unsigned)m * per_head;
    const int chunk = (int)(r % (unsigned)a.chunks), n = (int)(r / (unsigned)a.chunks);
    const int tid = threadIdx.x, d = tid % D;
    const int q = chunk * UNITS + tid / D;
    const unsigned row_bytes = (unsigned)a.M * D * 4u;
    const unsigned lane_bytes = ((unsigned)m * D + (unsigned)d) * 4u;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.value) + (long long)n * a.S * a.M * D, 0, a.S * (int)row_bytes, 0x00020000);
    if (q >= a.Lq) return;  // whole units leave: every butterfly partner of a lane that stays, stays
    const int unit = (n * a.Lq + q) * a.M + m;
    const int LP = a.L * a.P;
    const float* loc = a.loc + (long long)unit * (LP * 2);
    const float* wgt = a.weight + (long long)unit * LP;
    const float g = b.grad_out[(long long)unit * D + d];
    char* gv = GV ? reinterpret_cast<char*>(b.grad_value + (long long)n * a.S * a.M * D) : nullptr;
    float* gl = b.grad_loc ? b.grad_loc + (long long)unit * (LP * 2) : nullptr;
    float* gw = b.grad_weight ? b.grad_weight + (long long)unit * LP : nullptr;
    const bool sums = gl || gw;  // uniform
    for (int l = 0; l < a.L; ++l) {
        const MsdaLevel lv = msda_level(a, l);
        if (!lv.ok) {  // uniform
            if (d == 0)
                for (int p = 0; p < a.P; ++p) {
                    if (gl) reinterpret_cast<float2*>(gl)[l * a.P + p] = make_float2(0.f, 0.f);
                    if (gw) gw[l * a.P + p] = 0.f;
                }
            continue;
        }
        for (int p = 0; p < a.P; ++p) {
            const float2 xy = reinterpret_cast<const float2*>(loc)[l * a.P + p];
            const float w = wgt[l * a.P + p];
            const MsdaPoint pt = msda_point(lv, xy.x, xy.y, a.S, row_bytes, lane_bytes);
            if (sums) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)pt.off[k], 0, 0));
                // the fractions msda_point took its coefficients from (same expressions, same bits)
                const float x = __builtin_fmaf(xy.x, lv.Wf, -0.5f), y = __builtin_fmaf(xy.y, lv.Hf, -0.5f);
                const float lx = x - floorf(x), ly = y - floorf(y), hx = 1.f - lx, hy = 1.f - ly;
                float sw = pt.c[0] * v[0];
                sw = __builtin_fmaf(pt.c[1], v[1], sw);
                sw = __builtin_fmaf(pt.c[2], v[2], sw);
                sw = __builtin_fmaf(pt.c[3], v[3], sw);
                const float sx = __builtin_fmaf(ly, v[3] - v[2], hy * (v[1] - v[0]));
                const float sy = __builtin_fmaf(lx, v[3] - v[1], hx * (v[2] - v[0]));
                const float tw = msda_unit_sum<D>(g * sw), tx = msda_unit_sum<D>(g * sx), ty = msda_unit_sum<D>(g * sy);
                if (d == 0) {
                    if (gl) reinterpret_cast<float2*>(gl)[l * a.P + p] = make_float2((lv.Wf * w) * tx, (lv.Hf * w) * ty);
                    if (gw) gw[l * a.P + p] = tw;
                }
            }
            if constexpr (GV) {
                const float t = w * g;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (pt.off[k] != MSDA_NO_ROW) atomicAdd(reinterpret_cast<float*>(gv + pt.off[k]), t * pt.c[k]);
            }
        }
    }
}

template <int D>
void msda_launch(const MsdaArgs& a, bool p4, unsigned blocks, hipStream_t s) {
    if (p4) hipLaunchKernelGGL((msda_fwd_kernel<D, true>), dim3(blocks), dim3(MSDA_THREADS), 0, s, a);
    else hipLaunchKernelGGL((msda_fwd_kernel<D, false>), dim3(blocks), dim3(MSDA_THREADS), 0, s, a);
}

template <int D>
void msda_bwd_launch(const MsdaBwdArgs& b, unsigned blocks, hipStream_t s) {
    if (b.grad_value) hipLaunchKernelGGL((msda_bwd_kernel<D, true>), dim3(blocks), dim3(MSDA_THREADS), 0, s, b);
    else hipLaunchKernelGGL((msda_bwd_kernel<D, false>), dim3(blocks), dim3(MSDA_THREADS), 0, s, b);
}

// What the forward and the backward refuse alike; io is the [N,Lq,M*D] tensor of the call (the output / grad_out).
int msda_check(const char* who, const float* value, const int64_t* shapes, const int64_t* start, const float* loc, const float* weight,
               const float* io, int N, int S, int M, int D, int Lq, int L, int P) {
    SOLA_ARG(N >= 1 && S >= 1 && M >= 1 && Lq >= 1, "%s: N %d, S %d, M %d, Lq %d must all be >= 1", who, N, S, M, Lq);
    SOLA_ARG(D == 16 || D == 32 || D == 64, "%s: D = %d channels per head, supported are 16, 32 and 64", who, D);
    SOLA_ARG(L >= 1 && L <= SOLA_MSDA_MAX_LEVELS, "%s: L = %d levels, supported are 1 to %d", who, L, SOLA_MSDA_MAX_LEVELS);
    SOLA_ARG(P >= 1 && P <= SOLA_MSDA_MAX_POINTS, "%s: P = %d points, supported are 1 to %d", who, P, SOLA_MSDA_MAX_POINTS);
    SOLA_ARG(value && shapes && start && loc && weight && io, "%s: null argument", who);
    const long long lim = 1ll << 31;
    const long long row = (long long)M * D;
    SOLA_ARG(row * 4 < lim && (long long)S * row * 4 < lim,
             "%s: one batch element's value is S*M*D*4 = %lld bytes, the 32-bit row offsets take fewer than 2^31", who, (long long)S * row * 4);
    SOLA_ARG((long long)N * S * row < lim, "%s: value has N*S*M*D = %lld elements, at most 2^31 - 1", who, (long long)N * S * row);
    const long long units = (long long)N * Lq * M;
    SOLA_ARG(units < lim && units * L * P * 2 < lim, "%s: sampling_locations has N*Lq*M*L*P*2 = %lld elements, at most 2^31 - 1", who,
             units * L * P * 2);
    SOLA_ARG(units * D < lim, "%s: the output has N*Lq*M*D = %lld elements, at most 2^31 - 1", who, units * D);
    return SOLA_OK;
}

MsdaArgs msda_args(const float* value, const int64_t* shapes, const int64_t* start, const float* loc, const float* weight, float* out, int N,
                   int S, int M, int Lq, int L, int P, int units_per_block) {
    MsdaArgs a{};
    a.value = value; a.shapes = reinterpret_cast<const long long*>(shapes); a.start = reinterpret_cast<const long long*>(start);
    a.loc = loc; a.weight = weight; a.out = out;
    a.N = N; a.S = S; a.M = M; a.Lq = Lq; a.L = L; a.P = P;
    a.chunks = (Lq + units_per_block - 1) / units_per_block;
    return a;
}

uintptr_t msda_bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

int launch_ms_deform_attn(const float* value, const int64_t* shapes, const int64_t* start, const float* loc, const float* weight, int N,
                          int S, int M, int D, int Lq, int L, int P, float* out, hipStream_t s) {
    SOLA_TRY(msda_check("ms_deform_attn", value, shapes, start, loc, weight, out, N, S, M, D, Lq, L, P));
    SOLA_ARG(((msda_bits(value) | msda_bits(loc) | msda_bits(out)) & 15) == 0,
             "ms_deform_attn: value, sampling_locations and the output must be 16-byte aligned");
    SOLA_ARG((msda_bits(weight) & 3) == 0 && ((msda_bits(shapes) | msda_bits(start)) & 7) == 0,
             "ms_deform_attn: attention_weights must be 4-byte aligned, the level tables 8-byte aligned");
    const MsdaArgs a = msda_args(value, shapes, start, loc, weight, out, N, S, M, Lq, L, P, MSDA_THREADS / (D / 4));
    const long long blocks = (long long)N * M * a.chunks;  // <= units
    const bool p4 = P == 4 && (msda_bits(weight) & 15) == 0;
    if (D == 16) msda_launch<16>(a, p4, (unsigned)blocks, s);
    else if (D == 32) msda_launch<32>(a, p4, (unsigned)blocks, s);
    else msda_launch<64>(a, p4, (unsigned)blocks, s);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_ms_deform_attn_backward(const float* value, const int64_t* shapes, const int64_t* start, const float* loc, const float* weight,
                                   const float* grad_out, int N, int S, int M, int D, int Lq, int L, int P, float* grad_value, float* grad_loc,
                                   float* grad_weight, hipStream_t s) {
    const char* who = "ms_deform_attn_backward";
    SOLA_TRY(msda_check(who, value, shapes, start, loc, weight, grad_out, N, S, M, D, Lq, L, P));
    SOLA_ARG(grad_value || grad_loc || grad_weight, "%s: grad_value, grad_loc and grad_weight are all null, at least one output must be given", who);
    SOLA_ARG(((msda_bits(value) | msda_bits(loc)) & 15) == 0, "%s: value and sampling_locations must be 16-byte aligned", who);
    SOLA_ARG((msda_bits(weight) & 3) == 0 && ((msda_bits(shapes) | msda_bits(start)) & 7) == 0,
             "%s: attention_weights must be 4-byte aligned, the level tables 8-byte aligned", who);
    SOLA_ARG(((msda_bits(grad_out) | msda_bits(grad_value) | msda_bits(grad_weight)) & 3) == 0 && (msda_bits(grad_loc) & 7) == 0,
             "%s: grad_out, grad_value and grad_weight must be 4-byte aligned, grad_loc 8-byte aligned", who);
    MsdaBwdArgs b{};
    b.f = msda_args(value, shapes, start, loc, weight, nullptr, N, S, M, Lq, L, P, MSDA_THREADS / D);
    b.grad_out = grad_out; b.grad_value = grad_value; b.grad_loc = grad_loc; b.grad_weight = grad_weight;
    const long long blocks = (long long)N * M * b.f.chunks;  // <= units
    if (grad_value) SOLA_HIP(hipMemsetAsync(grad_value, 0, (size_t)N * S * M * D * sizeof(float), s));
    if (D == 16) msda_bwd_launch<16>(b, (unsigned)blocks, s);
    else if (D == 32) msda_bwd_launch<32>(b, (unsigned)blocks, s);
    else msda_bwd_launch<64>(b, (unsigned)blocks, s);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
