// What the GroupNorm kernels of both directions (norm.hip forward, bwd.hip backward) share, stated once: which kernel shape a unit takes
// (host, both ladders pinned by static_asserts), the token set of an instance and the block sum; bfloat16 rows widen through common.h's
// bf16x4_to_f32.  A unit is one (instance, group): ntok tokens x cg channels, normalised together.  The kernels' prologues, row loads,
// statistics and per-quad steps stay written out in the kernels: through shared helpers the compiler pairs other multiplies and adds
// into fused / packed instructions and results move in the last bit (profiles/gn_common_check.txt).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// Kernel shapes (host).  Pure functions of the unit's size, the formats and the sola_tune switches; the launchers switch on the result.
//   Wave      one wave per unit, four units per 256-thread block, R token slots per lane (units of <= 64 * 4 * R floats)
//   Block     one block of nthr threads per unit, R token slots per lane
//   Sliced    forward only: (unit, slice) blocks of GN_SLICE_R slots per lane, a statistics launch and an apply launch
//   ThreePass one block of nthr threads per unit walks it out of L2 (any token count, any channel count that is a multiple of 4)
// cpl = channels per lane (4; 8 in the forward's 16-bit storage mode), slices = slices per unit (Sliced only).
// ---------------------------------------------------------------------------------------------------------------
enum class GnKind : int { Wave, Block, Sliced, ThreePass };
struct GnShape { GnKind kind; int R, nthr, cpl, slices; };
constexpr bool operator==(const GnShape& a, const GnShape& b) {
    return a.kind == b.kind && a.R == b.R && a.nthr == b.nthr && a.cpl == b.cpl && a.slices == b.slices;
}
constexpr int GN_SLICE_R = 32;  // float4 per thread and slice of the sliced shape: 256 tokens at 128 channels per group, a FIXED size
// token slots per lane when `lanes` lanes of `lpt` lanes per token share a unit (none where the lanes do not divide into tokens)
constexpr int gn_slots(int ntok, int lanes, int lpt) { return lanes % lpt == 0 ? (ntok + lanes / lpt - 1) / (lanes / lpt) : 1 << 30; }

// Forward.  in / out / dropout select the eight-channel form (f16 rows in, f16 rows out, inference); gn_variant, gn_wide, gn_slices and
// gn_h8 are the sola_tune switches of the same names.  A Sliced result still needs its scratch: the launcher falls back to ThreePass.
constexpr GnShape gn_fwd_shape(int ntok, int cg, Elem in, Elem out, bool dropout, int gn_variant, int gn_wide, int gn_slices, int gn_h8) {
    const GnShape three_pass{GnKind::ThreePass, 0, 256, 4, 0};
    if (!gn_variant) return three_pass;
    const int f4 = cg / 4;
    // (f16 rows only: the eight-channel kernel widens its loads as _Float16; bfloat16 rows take the four-channel shapes, which widen them)
    if (gn_h8 && in == Elem::F16 && out == Elem::F16 && !dropout && cg % 8 == 0) {
        const int f8 = cg / 8;
        const int rw8 = gn_slots(ntok, 64, f8), rb8 = gn_slots(ntok, 256, f8), rk8 = gn_slots(ntok, 1024, f8);
        if (rw8 <= 2) return {GnKind::Wave, rw8, 256, 8, 0};
        if (rb8 <= 4) return {GnKind::Block, rb8 <= 2 ? 2 : 4, 256, 8, 0};
        if (rk8 <= 4) return {GnKind::Block, 4, 1024, 8, 0};
    }
    const int rw = gn_slots(ntok, 64, f4), rb = gn_slots(ntok, 256, f4);
    if (rw <= 4) return {GnKind::Wave, rw == 3 ? 4 : rw, 256, 4, 0};
    if (rb <= 16) return {GnKind::Block, rb <= 2 ? 2 : rb <= 4 ? 4 : rb <= 8 ? 8 : 16, 256, 4, 0};
    if (rb <= 32) return gn_wide && 1024 % f4 == 0 ? GnShape{GnKind::Block, 8, 1024, 4, 0}  // 8 per lane at 1024 threads
                                                   : GnShape{GnKind::Block, 32, 256, 4, 0};
    // units of more than 32 float4 per thread
    if (gn_slices && 256 % f4 == 0) return {GnKind::Sliced, GN_SLICE_R, 256, 4, gn_slots(ntok, 256 * GN_SLICE_R, f4)};
    return three_pass;
}

// Backward.  gn_bwd_reg is the sola_tune switch.  The register shapes shuffle across token lanes: f4 must be a power of two.
constexpr GnShape gn_bwd_shape(int ntok, int cg, int gn_bwd_reg) {
    const int f4 = cg / 4;
    if (!gn_bwd_reg || f4 > 256) return {GnKind::ThreePass, 0, 256, 4, 0};
    if ((f4 & (f4 - 1)) == 0) {
        const int rw = f4 <= 64 ? gn_slots(ntok, 64, f4) : 1 << 30, rb = gn_slots(ntok, 256, f4);
        if (rw <= 4) return {GnKind::Wave, rw == 3 ? 4 : rw, 256, 4, 0};
        if (rb <= 8) return {GnKind::Block, rb <= 2 ? 2 : rb <= 4 ? 4 : 8, 256, 4, 0};
        // units of up to twice the 256-thread shape (ragged batches: the inter-object norm over up to 128 tracks): 512 threads at 8
        // float4 per lane and tensor - the 1024-thread shape leaves most of its lanes idle on them (407 -> ~220 us per launch)
        if (rb <= 16) return {GnKind::Block, 8, 512, 4, 0};
        if (rb <= 32) return {GnKind::Block, 8, 1024, 4, 0};
    }
    return {GnKind::ThreePass, 0, 1024 % f4 == 0 ? 1024 : 256, 4, 0};
}
// the 1024-thread register shape (the object->language norm's, which never has a second gradient) has no bfloat16-dy2 code
constexpr bool gn_bwd_reads_bf16_dy2(const GnShape& sh) { return !(sh.kind == GnKind::Block && sh.nthr == 1024); }

// Both ladders at their edges (the values of the ladders as they stood in launch_group_norm / launch_group_norm_bwd).
namespace gn_shape_checks {
constexpr GnShape fwd(int ntok, int cg, int variant = 1, int wide = 1, int slices = 1) { return gn_fwd_shape(ntok, cg, Elem::F32, Elem::F32, false, variant, wide, slices, 1); }
constexpr GnShape fwd8(int ntok, int cg, int h8 = 1) { return gn_fwd_shape(ntok, cg, Elem::F16, Elem::F16, false, 1, 1, 1, h8); }
constexpr GnShape bwd(int ntok, int cg, int reg = 1) { return gn_bwd_shape(ntok, cg, reg); }
constexpr GnShape wave(int R, int cpl = 4) { return {GnKind::Wave, R, 256, cpl, 0}; }
constexpr GnShape block(int R, int nthr = 256, int cpl = 4) { return {GnKind::Block, R, nthr, cpl, 0}; }
constexpr GnShape sliced(int S) { return {GnKind::Sliced, GN_SLICE_R, 256, 4, S}; }
constexpr GnShape three(int nthr = 256) { return {GnKind::ThreePass, 0, nthr, 4, 0}; }
// forward, f32 in and out, 16 channels per group
static_assert(fwd(1, 16) == wave(1) && fwd(16, 16) == wave(1) && fwd(17, 16) == wave(2) && fwd(32, 16) == wave(2));
static_assert(fwd(33, 16) == wave(4) && fwd(64, 16) == wave(4) && fwd(65, 16) == block(2) && fwd(128, 16) == block(2));
static_assert(fwd(129, 16) == block(4) && fwd(256, 16) == block(4) && fwd(257, 16) == block(8) && fwd(512, 16) == block(8));
static_assert(fwd(513, 16) == block(16) && fwd(1024, 16) == block(16) && fwd(1025, 16) == block(8, 1024) && fwd(2048, 16) == block(8, 1024));
static_assert(fwd(1025, 16, 1, 0) == block(32) && fwd(2048, 16, 1, 0) == block(32));
static_assert(fwd(2049, 16) == sliced(2) && fwd(2049, 16, 1, 1, 0) == three() && fwd(2049, 16, 0) == three() && fwd(1, 16, 0) == three());
// ... 128 channels per group
static_assert(fwd(2, 128) == wave(1) && fwd(4, 128) == wave(2) && fwd(8, 128) == wave(4) && fwd(9, 128) == block(2));
static_assert(fwd(32, 128) == block(4) && fwd(64, 128) == block(8) && fwd(128, 128) == block(16));
static_assert(fwd(129, 128) == block(8, 1024) && fwd(256, 128) == block(8, 1024) && fwd(257, 128) == sliced(2));
// ... channel counts whose float4 do not divide a block: three passes at any token count
static_assert(fwd(1, 48) == three() && fwd(14, 48) == three() && fwd(5000, 48) == three());
// ... 1024 channels per group: one token per 256-thread pass, four per 1024-thread pass (1024 % 256 == 0: the wide shape takes 32 tokens)
static_assert(fwd(16, 1024) == block(16) && fwd(32, 1024) == block(8, 1024) && fwd(32, 1024, 1, 0) == block(32) && fwd(33, 1024) == sliced(2));
// forward, eight channels per lane (16-bit rows in, f16 rows out, no dropout), 128 channels per group
static_assert(fwd8(4, 128) == wave(1, 8) && fwd8(8, 128) == wave(2, 8) && fwd8(32, 128) == block(2, 256, 8) && fwd8(64, 128) == block(4, 256, 8));
static_assert(fwd8(65, 128) == block(4, 1024, 8) && fwd8(256, 128) == block(4, 1024, 8) && fwd8(257, 128) == sliced(2));
static_assert(fwd8(4, 128, 0) == wave(2) && fwd8(8, 128, 0) == wave(4) && fwd8(32, 128, 0) == block(4) && fwd8(64, 128, 0) == block(8));
static_assert(fwd8(65, 128, 0) == block(16) && fwd8(256, 128, 0) == block(8, 1024) && fwd8(257, 128, 0) == sliced(2));
static_assert(gn_fwd_shape(4, 128, Elem::F16, Elem::F16, true, 1, 1, 1, 1) == wave(2) && gn_fwd_shape(4, 128, Elem::F32, Elem::F16, false, 1, 1, 1, 1) == wave(2));
static_assert(gn_fwd_shape(4, 128, Elem::BF16, Elem::F16, false, 1, 1, 1, 1) == wave(2) && gn_fwd_shape(65, 128, Elem::BF16, Elem::F16, false, 1, 1, 1, 1) == block(16));
// backward, 16 channels per group
static_assert(bwd(16, 16) == wave(1) && bwd(32, 16) == wave(2) && bwd(64, 16) == wave(4) && bwd(65, 16) == block(2) && bwd(128, 16) == block(2));
static_assert(bwd(256, 16) == block(4) && bwd(512, 16) == block(8) && bwd(513, 16) == block(8, 512) && bwd(1024, 16) == block(8, 512));
static_assert(bwd(1025, 16) == block(8, 1024) && bwd(2048, 16) == block(8, 1024) && bwd(2049, 16) == three(1024));
static_assert(!gn_bwd_reads_bf16_dy2(bwd(1025, 16)) && !gn_bwd_reads_bf16_dy2(bwd(2048, 16)));
static_assert(gn_bwd_reads_bf16_dy2(bwd(1024, 16)) && gn_bwd_reads_bf16_dy2(bwd(2049, 16)) && gn_bwd_reads_bf16_dy2(bwd(16, 16)));
static_assert(bwd(16, 16, 0) == three() && bwd(2049, 16, 0) == three() && bwd(1025, 16, 0) == three());
static_assert(bwd(1, 48) == three() && bwd(5000, 48) == three() && bwd(1, 24) == three() && bwd(5000, 24) == three());
}  // namespace gn_shape_checks

// ---------------------------------------------------------------------------------------------------------------
// The token set of instance `inst`: first row, row stride, token count and the positional-encoding row of the forward's y + pe
// output (unused by the backward).  Args is GnArgs or GnBwdArgs: both carry units, inner, the three strides and ntok.
// ---------------------------------------------------------------------------------------------------------------
struct GnUnit { long long row0, tok_stride; int ntok, pe_row; };
template <class Args>
__device__ __forceinline__ GnUnit gn_unit(const Args& a, int inst) {
    GnUnit u;
    if (a.units) {
        const int4 d = a.units[inst];
        u.row0 = d.x; u.tok_stride = d.y; u.ntok = d.z; u.pe_row = d.w;
    } else {
        u.row0 = (long long)(inst / a.inner) * a.outer_stride + (long long)(inst % a.inner) * a.inner_stride;
        u.tok_stride = a.tok_stride; u.ntok = a.ntok; u.pe_row = inst % a.inner;
    }
    return u;
}

// Sum over a block of NTHR threads (NTHR / 64 waves); every thread gets the result; fixed combination order.
template <int NTHR>
__device__ __forceinline__ float block_sum_n(float v, float* red) {
    if (NTHR == 256) return block_sum_256(v, red);
    v = wave_sum(v);
    __syncthreads();  // protect `red` from a previous use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NTHR / 64; ++i) t += red[i];
    return t;
}

typedef _Float16 half4n __attribute__((ext_vector_type(4)));
enum : int { GN_F32 = 0, GN_F16 = 1, GN_BF16 = 2 };  // the row format codes of GnArgs::in_f16
