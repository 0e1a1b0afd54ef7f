// What the attention kernels (attn.hip, attn_simple.hip, attn_reg.hip, attn_res.hip, attn_f16.hip, attn_bwd.hip, lab/attn_ring.hip) share,
// stated once: where a (group) unit's rows are, how a 16-query output tile leaves a wave, the split-f16 register helpers, and on the
// host the AttnDesc -> kernel-argument fill, the profiler scope, the grid check, the head-dim dispatch and the entry points the files call
// across.  Every args struct keeps its own members and order (the kernarg layout is the kernel's); the templates below only rely on the
// shared member NAMES.  profiles/attn_common_isa.txt: kernel by kernel, what the compiler makes of these helpers against the written-out forms.
#pragma once
#include <type_traits>
#include <utility>

#include "kernels.h"

typedef half4 half4v;  // common.h's 16-bit vectors under the names the attention files use
typedef half8 half8v;

// ---- device: where a unit's rows are ---------------------------------------------------------------------------------------
// Group grp attends rows q0 + i * q_rs (i < Sq) over rows k0 + j * k_rs (j < Sk) of the one [B, N, T', D] token-major layout.
struct AttnUnit { long long q0, k0, q_rs, k_rs; int Sq, Sk; };

// strided groups: (outer, inner) index pair -> first rows; strides and lengths are the launch's
template <class A>
__device__ __forceinline__ AttnUnit attn_unit_strided(const A& a, int grp) {
    AttnUnit u;
    u.q0 = (long long)(grp / a.inner) * a.q_outer + (long long)(grp % a.inner) * a.q_inner;
    u.k0 = (long long)(grp / a.inner) * a.k_outer + (long long)(grp % a.inner) * a.k_inner;
    u.q_rs = a.q_rs; u.k_rs = a.k_rs; u.Sq = a.Sq; u.Sk = a.Sk;
    return u;
}
// Strided groups or, with unit tables (ragged batches), q_units[grp] / k_units[grp] = (first row, row stride, length, -).
// The rule for UNIFORM: where grp is wave-uniform (a block or a wave serves ONE unit) the table values are passed through readfirstlane -
// the compiler cannot know a table entry is the same for all lanes, and scalar values keep the address arithmetic behind them on the
// scalar unit.  Where the lanes of a wave serve different units (attn.hip's packed mode, attn_fwd_small_kernel and its f16 twin, every
// backward kernel) UNIFORM must be false: the scalarised form would hand every lane lane 0's unit.  No default, so every call says which.
template <bool UNIFORM, class A>
__device__ __forceinline__ AttnUnit attn_unit(const A& a, int grp) {
    AttnUnit u;
    if (a.q_units) {
        const int4 qu = a.q_units[grp], ku = a.k_units[grp];
        if constexpr (UNIFORM) {
            u.q0 = __builtin_amdgcn_readfirstlane(qu.x); u.q_rs = __builtin_amdgcn_readfirstlane(qu.y); u.Sq = __builtin_amdgcn_readfirstlane(qu.z);
            u.k0 = __builtin_amdgcn_readfirstlane(ku.x); u.k_rs = __builtin_amdgcn_readfirstlane(ku.y); u.Sk = __builtin_amdgcn_readfirstlane(ku.z);
        } else {
            u.q0 = qu.x; u.q_rs = qu.y; u.Sq = qu.z;
            u.k0 = ku.x; u.k_rs = ku.y; u.Sk = ku.z;
        }
    } else {
        u = attn_unit_strided(a, grp);
    }
    return u;
}

// ---- device: small helpers ---------------------------------------------------------------------------------------------------
// the two LDS-crossbar shuffles that finish a softmax row's max / sum: a row lives in one 16-lane column, its key slots in lanes 16 / 32 apart
__device__ __forceinline__ float xor16_32_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xor16_32_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// (the bf16 converters bf16x4_to_f32 / f32x4_to_bf16 and the f16 range guard f16_range_guard are common.h's: the GEMMs and the norms use them too)

// Split-f16 operands: four consecutive values as (hi4, lo4) (cast.hip: every 8 values = 32 bytes [hi8 | lo8]); a product runs as
// lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x16_f16 with f32 accumulation (~22-bit products, as in gemm_glds.hip).
struct HL4 { half4v hi, lo; };
// amax: the largest magnitude that went through (attn_res.hip's range guard covers q, k, v and the output pairs)
__device__ __forceinline__ HL4 split4(float x, float y, float z, float w, float& amax) {
    HL4 r;
    const float in[4] = {x, y, z, w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        _Float16 h1, l1;
        split_f16(in[j], h1, l1);
        r.hi[j] = h1; r.lo[j] = l1;
        amax = fmaxf(amax, fabsf(in[j]));
    }
    return r;
}
__device__ __forceinline__ HL4 split4(float x, float y, float z, float w) {
    float unused = 0.f;
    return split4(x, y, z, w, unused);
}
__device__ __forceinline__ f32x4 mfma3(const HL4& a, const HL4& b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x16f16(a.lo, b.hi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.lo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a.hi, b.hi, c, 0, 0, 0);
}

// ---- device: how an output tile leaves a wave ----------------------------------------------------------------------------------
// Store one query row's output tile.  op points at o[row][h*DH]; this lane holds d = 16c + 4*g4 + {0..3} of every chunk c (the
// O^T = V^T P^T register layout), scaled by inv on the way out.  f32: one float4 per chunk.  split-f16 (sp16): an 8-wide block
// [hi8 | lo8] is held by the lane pair (g4, g4 ^ 1); each lane writes the hi and the lo halves of its OWN four values as two 8-byte
// stores (block offset 8 * (g4 & 1), lo 16 bytes behind) - no cross-lane traffic (the lanes of a pair are 16 apart, a shuffle between
// them goes through the LDS crossbar), and the largest magnitude written goes to the range guard.
template <int NC>
__device__ __forceinline__ void attn_store_tile(float* op, int g4, const f32x4 (&oacc)[NC], float inv, int sp16, int* guard) {
    if (!sp16) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
            *reinterpret_cast<float4*>(op + 4 * g4 + c * 16) =
                make_float4(oacc[c][0] * inv, oacc[c][1] * inv, oacc[c][2] * inv, oacc[c][3] * inv);
        return;
    }
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        half4v hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = oacc[c][j] * inv;
            _Float16 h1, l1;
            split_f16(v, h1, l1);
            hi[j] = h1; lo[j] = l1;
            m = fmaxf(m, fabsf(v));
        }
        char* dst = reinterpret_cast<char*>(op + c * 16 + 8 * (g4 >> 1)) + 8 * (g4 & 1);
        *reinterpret_cast<half4v*>(dst) = hi;
        *reinterpret_cast<half4v*>(dst + 16) = lo;
    }
    f16_range_guard(guard, m);
}

// ---- host: AttnDesc / AttnBwdDesc -> kernel arguments ---------------------------------------------------------------------------
template <class A, class = void> struct attn_has_o_sp16 : std::false_type {};
template <class A> struct attn_has_o_sp16<A, std::void_t<decltype(std::declval<A&>().o_sp16)>> : std::true_type {};

// The fields every args struct has under the same name: pitches, sizes, the six strides, the scale and the unit tables (k_units falls
// back to q_units: self-attention over ragged units).  Structs with a split-f16 output also get o_sp16 and its guard rule: the guard
// word is only looked at where split pairs are written.
template <class A, class D>
void attn_fill_common(A& a, const D& d) {
    a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.ldo = d.ldo;
    a.G = d.G; a.H = d.H; a.Sq = d.Sq; a.Sk = d.Sk; a.inner = d.inner;
    a.q_outer = d.q_outer; a.q_inner = d.q_inner; a.q_rs = d.q_rs;
    a.k_outer = d.k_outer; a.k_inner = d.k_inner; a.k_rs = d.k_rs;
    a.scale = d.scale;
    a.q_units = d.q_units; a.k_units = d.q_units ? (d.k_units ? d.k_units : d.q_units) : nullptr;
    if constexpr (attn_has_o_sp16<A>::value) {
        a.o_sp16 = d.out == Elem::SP16; a.guard = d.out == Elem::SP16 ? d.guard : nullptr;
    }
}

// the forward's profiler scope: 4 flops per (query, key, head dim), q + o and k + v rows of bytes_per_elem bytes moved once
inline SolaProfScope attn_prof_scope(const AttnDesc& d, hipStream_t s, double bytes_per_elem = 4.0) {
    const double elems = (double)d.G * d.H * d.DH;
    return SolaProfScope(SOLA_PROF_ATTN, s, 4.0 * elems * d.Sq * d.Sk, bytes_per_elem * elems * (2.0 * d.Sq + 2.0 * d.Sk));
}

// a grid's x dimension, for SOLA_TRY; what = the error text's prefix ("attention", "attention (f16)", ...)
inline int attn_grid_ok(long long blocks, const char* what) {
    if (blocks < (1ll << 31)) return SOLA_OK;
    sola_set_error("%s: grid too large", what);
    return SOLA_ERR_ARG;
}

// f(std::integral_constant<int, DH>) for the head dims the MFMA shapes are compiled for; err_fmt takes the head dim
template <class F>
int attn_dispatch_dh(int DH, const char* err_fmt, F&& f) {
    switch (DH) {
        case 128: return f(std::integral_constant<int, 128>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: sola_set_error(err_fmt, DH); return SOLA_ERR_ARG;
    }
}

// ---- the shapes launch_attention (attn.hip) routes to, each declared once for its definition and its user -------------------------
bool attention_simple_supported(const AttnDesc& d);   // attn_simple.hip
int launch_attention_simple(const AttnDesc& d, hipStream_t s);
bool attention_small_supported(const AttnDesc& d);
int launch_attention_small(const AttnDesc& d, hipStream_t s);
bool attention_splitm_supported(const AttnDesc& d);
int launch_attention_splitm(const AttnDesc& d, hipStream_t s);
bool attention_spin_supported(const AttnDesc& d);
int launch_attention_spin(const AttnDesc& d, hipStream_t s);
bool attention_reg_supported(const AttnDesc& d);      // attn_reg.hip
int launch_attention_reg(const AttnDesc& d, hipStream_t s);
bool attention_res_supported(const AttnDesc& d);      // attn_res.hip
int launch_attention_res(const AttnDesc& d, hipStream_t s);
int launch_attention_bf16_train(const AttnDesc& d, hipStream_t s);  // attn_f16.hip (attention_bf16_mfma_supported: kernels.h)
extern int g_attn_splitm;
#ifdef SOLA_EXPERIMENTS  // closed experiment (lab/attn_ring.hip): EXPERIMENTS=1 builds with sola_tune "attn_ring" only
bool attention_ring_supported(const AttnDesc& d);
int launch_attention_ring(const AttnDesc& d, hipStream_t s);
extern int g_attn_ring;
#endif
