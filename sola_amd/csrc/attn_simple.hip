// High-occupancy shape of the exact-f32 attention core (inference; sola_tune "attn_variant" 2).
//
// attn.hip's shared mode keeps a whole 64-key K/V tile pair in LDS (68 KB) and 256 VGPRs per lane for its register
// prefetch of the next unit: two 4-wave blocks per CU, and a unit's phases (stage, QK^T, softmax, PV, store) largely
// serialise - it reaches 3.5 TB/s where a plain copy with the same access pattern reaches 5.3-5.9 (tools/micro/strided_bw).
// This shape trades the hand-rolled pipeline for occupancy: K/V tiles of TK = 32 keys (34 KB), no cross-unit state, ~100
// VGPRs, so four to five blocks share a CU and cover each other's latency; longer key sequences take further tiles with
// the online softmax.  Same arithmetic (v_mfma_f32_16x16x4_f32, S^T = K Q^T / O^T = V^T P^T register layout), same
// addressing (strided groups or unit tables), f32 or split-f16 output.
#include "attn_fwd_steps.h"

namespace {

struct AttnSArgs {
    const float *q, *k, *v;
    float* o;
    int ldq, ldk, ldv, ldo;
    int G, H, Sq, Sk, inner, nqb;
    long long q_outer, q_inner, q_rs;
    long long k_outer, k_inner, k_rs;
    float scale;
    int o_sp16;
    int in_bf16;  // q / k / v are bfloat16 rows (IN16 instantiation)
    int* guard;
    const int4 *q_units, *k_units;
    int xcd_remap;
    float* lse;       // TR instantiation: optional [q rows][H] log-sum-exp of the scaled scores (saved for the backward)
    DropoutCfg drop;  // TR instantiation: dropout on the probabilities (tools/attention.py:71), same counter-based mask as attn.hip
    void* o_cast;     // TR instantiation: AttnDesc::o_cast / o_side / cast
    void* o_side;
    int o_cast_fmt;
    int o_skip_f32;   // TR + IN16: the f32 output is not written (the bf16 o_cast is the only copy: AttnDesc::in BF16 with o == nullptr)
};

// DB: two LDS stages of TK keys; the next tile's K/V rows travel in registers while the current tile is multiplied and there
// is ONE barrier per tile (the shape that took the attention backward from 460 to 299 us, attn_bwd.hip).
// TR (round 3): the training forward - log-sum-exp output and dropout on the probabilities - so that sola_forward_train[_ragged]
// takes this shape too (its q-blocks are independent blocks: units of very different lengths balance over the chip, where
// attn.hip's shared mode walks a ragged unit's q-blocks inside one block).  A separate instantiation: the inference kernel's
// registers (126 at four blocks per CU) are untouched.
// IN16 (round 6, the training step's bf16 storage): q / k / v are BFLOAT16 rows (pitches in values) - 8-byte q loads, 16-byte K / V
// prefetch pieces of eight values, widened on their way into the f32 LDS stages; everything behind the loads is the f32 kernel.
template <int DH, int TK, bool DB = false, bool TR = false, bool IN16 = false>
__global__ __launch_bounds__(256, 4) void attn_fwd_f32_simple_kernel(const AttnSArgs a) {
    static_assert(!IN16 || (DB && TR), "bf16 inputs: the double-buffered training instantiation");
    constexpr int NC = DH / 16;
    constexpr int LDK = DH + 4, LDV = DH + 4;
    extern __shared__ __attribute__((aligned(16))) float smem_s[];
    float* Ks = smem_s;
    float* Vs = smem_s + TK * LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    // a.xcd_remap (grid % 8 == 0): consecutive logical blocks - the heads of a group, the q-blocks of a unit - share an XCD's L2
    const unsigned lb = a.xcd_remap ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const long long unit = lb / a.nqb;
    const int qb = (int)(lb - unit * a.nqb);
    const int grp = (int)(unit / a.H), h = (int)(unit - (long long)grp * a.H);
    const AttnUnit u = attn_unit<true>(a, grp);  // a block serves one unit
    const long long q0 = u.q0, k0 = u.k0, q_rs = u.q_rs, k_rs = u.k_rs;
    const int Sq = u.Sq, Sk = u.Sk;
    if (qb * 64 >= Sq) return;  // ragged: fewer q-blocks than the largest unit (block-uniform)
    const int qi = qb * 64 + wave * 16 + c16;
    const bool q_ok = qi < Sq;
    float4 qf[NC];
    if constexpr (IN16) {
        const unsigned short* qp = reinterpret_cast<const unsigned short*>(a.q) + (q0 + (long long)(q_ok ? qi : 0) * q_rs) * a.ldq + h * DH + 4 * g4;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 v = bf16x4_to_f32(*reinterpret_cast<const uint2*>(qp + c * 16));
            qf[c] = q_ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const float* qp = a.q + (q0 + (long long)qi * q_rs) * a.ldq + h * DH + 4 * g4;
#pragma unroll
        for (int c = 0; c < NC; ++c) qf[c] = q_ok ? *reinterpret_cast<const float4*>(qp + c * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    // pieces per thread and tile (K + V) of the prefetch: 16 bytes each - four f32 values, or eight bf16 ones (IN16)
    constexpr int VPP = IN16 ? 8 : 4, PPR = DH / VPP;  // values per piece, pieces per row
    constexpr int PT = DB ? 2 * TK * PPR / 256 : 1;
    float4 st[PT];
    // round 5: this kernel's time is its SIMD issue time - PMC: the f32 MFMA busy 50 % of the SIMD cycles and 1 066 VALU instructions per
    // wave, which do not overlap it on gfx950 (profiles/r05_attention_ring.txt) - so the prefetch keeps a pointer per piece and advances it
    // by the tile's stride (the 64-bit row products, quarter-rate multiplies, left the loop) and whole tiles load without the row test
    const char* fp[PT];
    int fr[PT];
    constexpr int ES = IN16 ? 2 : 4;  // bytes per stored value
    if constexpr (DB) {
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int e = tid + 256 * j, which = e / (TK * PPR), r = (e % (TK * PPR)) / PPR, cp = e % PPR;
            fr[j] = r;
            fp[j] = reinterpret_cast<const char*>(which ? a.v : a.k) + ((k0 + (long long)r * k_rs) * (which ? a.ldv : a.ldk) + h * DH + cp * VPP) * ES;
        }
    }
    const long long fstep_k = (long long)TK * k_rs * a.ldk * ES, fstep_v = (long long)TK * k_rs * a.ldv * ES;  // wave-uniform, bytes
    auto fetch = [&](int kt0) {
        if (kt0 + TK <= Sk) {  // a whole tile (block-uniform)
#pragma unroll
            for (int j = 0; j < PT; ++j) st[j] = *reinterpret_cast<const float4*>(fp[j]);
        } else {
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                st[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kt0 + fr[j] < Sk) st[j] = *reinterpret_cast<const float4*>(fp[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < PT; ++j) fp[j] += (tid + 256 * j) / (TK * PPR) ? fstep_v : fstep_k;
    };
    if (DB) fetch(0);
    int it = 0;
    for (int kt0 = 0; kt0 < Sk; kt0 += TK, ++it) {
        const int nrows = min(TK, Sk - kt0);
        const int nrows16 = (nrows + 15) & ~15;
        if (DB) {
            Ks = smem_s + (it & 1) * 2 * TK * LDK;
            Vs = Ks + TK * LDK;
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int e = tid + 256 * j, which = e / (TK * PPR), r = (e % (TK * PPR)) / PPR, cp = e % PPR;
                float* dst = &(which ? Vs : Ks)[r * LDK + cp * VPP];
                if constexpr (IN16) {
                    const uint4 w = __builtin_bit_cast(uint4, st[j]);
                    *reinterpret_cast<float4*>(dst) = bf16x4_to_f32(make_uint2(w.x, w.y));
                    *reinterpret_cast<float4*>(dst + 4) = bf16x4_to_f32(make_uint2(w.z, w.w));
                } else {
                    *reinterpret_cast<float4*>(dst) = st[j];
                }
            }
            __syncthreads();
            if (kt0 + TK < Sk) fetch(kt0 + TK);
        } else {
        if (kt0 > 0) __syncthreads();
        attn_stage_rows<float4, DH, 256>(a.k, a.v, a.ldk, a.ldv, k0, k_rs, kt0, h, nrows, nrows16, tid, Ks, Vs, LDK, LDV);
        __syncthreads();
        }
        const int ntile = nrows16 >> 4;
        f32x4 sc[TK / 16];
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
                attn_qk_f32<NC>(&Ks[(t * 16 + c16) * LDK + 4 * g4], qf, a0, a1);
                const int key0 = kt0 + t * 16 + 4 * g4;
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[t][r] = (key0 + r < Sk) ? (a0[r] + a1[r]) * a.scale : -INFINITY;
            } else {
                sc[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        // mask-and-scale, the softmax step and the PV loop stay written out: profiles/attn_fwd_bodies_isa.txt, attn_fwd_bodies_bench.txt
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[t][r]);
        mx = max_xor32(max_xor16(mx));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[t][r] = __expf(sc[t][r] - m_new);
                rs += sc[t][r];
            }
        rs = sum_xor32(sum_xor16(rs));
        l_run = l_run * alpha + rs;
        m_run = m_new;
        // the accumulators are rescaled only where some row's running maximum moved (x * 1 = x: the same bits; 32 multiplies of the SIMD's
        // issue time saved on every other tile or so)
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) oacc[c] *= alpha;
        }
        if constexpr (TR) {
            if (a.drop.enabled) {  // dropout acts on the normalised probabilities: the row sum above stays undropped (attn.hip)
                const unsigned long long rbase = ((unsigned long long)(grp * a.H + h) * Sq + qi) * Sk;
#pragma unroll
                for (int t = 0; t < TK / 16; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sc[t][r] = dropout_keep(a.drop, rbase + kt0 + t * 16 + 4 * g4 + r) ? sc[t][r] * a.drop.scale : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vp = &Vs[(t * 16 + 4 * g4 + r) * LDV + c16];
#pragma unroll
                    for (int c = 0; c < NC; ++c) oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[c * 16], sc[t][r], oacc[c], 0, 0, 0);
                }
            }
        }
    }
    if (!q_ok) return;
    const float inv = 1.f / l_run;
    if constexpr (TR) {
        if (a.lse && g4 == 0) a.lse[(q0 + (long long)qi * q_rs) * a.H + h] = m_run + logf(l_run);
    }
    float* op = a.o + (q0 + (long long)qi * q_rs) * a.ldo + h * DH;
    if constexpr (TR) {  // the f32 output may be skipped, and the out-projection's operand cast is written next to it
        if (!a.o_sp16) {
            if (!a.o_skip_f32) attn_store_tile<NC>(op, g4, oacc, inv, 0, nullptr);
            if (a.o_cast) {  // the out-projection's operand cast of the same values (uniform branch)
                const long long eo = (q0 + (long long)qi * q_rs) * a.ldo + h * DH;  // element offset of this row's head slice
                if (a.o_cast_fmt == 1) {
                    float* pp = static_cast<float*>(a.o_cast) + eo;
                    _Float16* sd = a.o_side ? static_cast<_Float16*>(a.o_side) + eo : nullptr;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        half4v hi, lo;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            _Float16 h1, l1;
                            split_f16(oacc[c][j] * inv, h1, l1);
                            hi[j] = h1; lo[j] = l1;
                        }
                        char* dst = reinterpret_cast<char*>(pp + c * 16 + 8 * (g4 >> 1)) + 8 * (g4 & 1);
                        *reinterpret_cast<half4v*>(dst) = hi;
                        *reinterpret_cast<half4v*>(dst + 16) = lo;
                        if (sd) *reinterpret_cast<half4v*>(sd + c * 16 + 4 * g4) = hi;
                    }
                } else {
                    _Float16* cp = static_cast<_Float16*>(a.o_cast) + eo;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        half4v hv;
                        if (a.o_cast_fmt == 3) {
                            typedef __bf16 bf16x4s __attribute__((ext_vector_type(4)));
                            bf16x4s b;
#pragma unroll
                            for (int j = 0; j < 4; ++j) b[j] = (__bf16)(oacc[c][j] * inv);
                            hv = __builtin_bit_cast(half4v, b);
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j) hv[j] = (_Float16)(oacc[c][j] * inv);
                        }
                        *reinterpret_cast<half4v*>(cp + c * 16 + 4 * g4) = hv;
                    }
                }
            }
            return;
        }
    }
    attn_store_tile<NC>(op, g4, oacc, inv, a.o_sp16, a.guard);
}

// ---- sequences of at most 4 steps (motion attention over T' = ceil(T/8): 4 at the headline shape) -----------------------
// A (track, head) unit is 4 rows of q, k, v in and 4 rows of o out - 8 KB of traffic for 4 K multiply-adds: pure streaming.
// The packed MFMA shape of attn.hip stages K/V through 67 KB of LDS (two blocks per CU) and reaches 45 % of the HBM peak
// where a copy with this access pattern reaches 66-74 % (tools/micro/strided_bw).  Here half a wave owns a unit: lane c holds
// float4 chunk c of every row (rows are 32 chunks = one 512-byte head slice, so every load and store is a coalesced 512
// bytes), the TT x TT scores are per-lane partial dot products all-reduced over the 32 lanes, softmax and P V run in
// registers.  No LDS, ~100 VGPRs, any occupancy the registers allow.
template <int TT>
__global__ __launch_bounds__(256) void attn_fwd_small_kernel(const AttnSArgs a) {
    constexpr int DH = 128;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, hw = lane >> 5;
    const long long unit = ((long long)blockIdx.x * 4 + wave) * 2 + hw;
    const long long n_units = (long long)a.G * a.H;
    const bool live = unit < n_units;
    const long long uu = live ? unit : 0;
    const int grp = (int)(uu / a.H), h = (int)(uu - (long long)grp * a.H);
    const AttnUnit u = attn_unit<false>(a, grp);  // the two halves of a wave serve different units
    const long long q0 = u.q0, k0 = u.k0, q_rs = u.q_rs, k_rs = u.k_rs;
    int Sq = u.Sq, Sk = u.Sk;
    if (!live) { Sq = 0; Sk = 0; }
    float4 qv[TT], kv[TT], vv[TT];
    // Rows past the unit's length: load a CLAMPED row and zero the VALUE.  `t < Sq ? *p : z` made the compiler select between the
    // global pointer and the address of a zero constant it had put into scratch memory, then load through a FLAT address: a
    // 16-byte scratch store per lane and row (366 MiB of WRITE_SIZE per launch for 256 MiB of output, profiles/r02_summary.md -
    // WRITE_SIZE itself is exact on this access pattern: profiles/r03_write_size_calibration.txt) and flat instead of global loads.
    auto ld = [&](const float* base, long long row0, long long rs, int ld_, int t, int n) {
        const float4 v = *reinterpret_cast<const float4*>(base + (row0 + (long long)(t < n ? t : 0) * rs) * ld_ + h * DH + 4 * c);
        const bool ok = t < n;
        return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
    };
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        qv[t] = ld(a.q, q0, q_rs, a.ldq, t, Sq);
        kv[t] = ld(a.k, k0, k_rs, a.ldk, t, Sk);
        vv[t] = ld(a.v, k0, k_rs, a.ldv, t, Sk);
    }
    float sc[TT][TT];
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const float p = (qv[i].x * kv[j].x + qv[i].y * kv[j].y) + (qv[i].z * kv[j].z + qv[i].w * kv[j].w);
            sc[i][j] = half_sum32(p) * a.scale;  // DPP + one permlane swap; stays inside the 32-lane half
        }
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        if (i >= Sq) break;
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < TT; ++j) mx = j < Sk ? fmaxf(mx, sc[i][j]) : mx;
        float den = 0.f, pj[TT];
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            pj[j] = j < Sk ? __expf(sc[i][j] - mx) : 0.f;
            den += pj[j];
        }
        const float inv = 1.f / den;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const float w = pj[j] * inv;
            o.x += w * vv[j].x; o.y += w * vv[j].y; o.z += w * vv[j].z; o.w += w * vv[j].w;
        }
        float* op = a.o + (q0 + (long long)i * q_rs) * a.ldo + h * DH;
        if (!a.o_sp16) {
            *reinterpret_cast<float4*>(op + 4 * c) = o;
        } else {
            // floats 4c .. 4c+3 are one half of the 8-wide block c >> 1 = 32 bytes [hi8 | lo8].  The lane pair (c, c ^ 1) trades
            // halves (two DPP moves each way) so that the even lane writes the 16 bytes of hi8 and the odd lane the 16 bytes of
            // lo8 - one 16-byte store per lane instead of two 8-byte ones (which reached HBM as 366 MiB of WRITE_SIZE per launch
            // for 256 MiB of output: half-written 32-byte sectors)
            const float v4[4] = {o.x, o.y, o.z, o.w};
            half4v hi, lo;
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                _Float16 h1, l1;
                split_f16(v4[j], h1, l1);
                hi[j] = h1; lo[j] = l1;
                m = fmaxf(m, fabsf(v4[j]));
            }
            const int2 hw2 = __builtin_bit_cast(int2, hi), lw2 = __builtin_bit_cast(int2, lo);
            const bool odd = c & 1;
            const int sx = odd ? hw2.x : lw2.x, sy = odd ? hw2.y : lw2.y;  // what the partner needs: its lo8 needs my lo4, its hi8 my hi4
            const int rx = __builtin_amdgcn_update_dpp(0, sx, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]: lane c <- lane c ^ 1
            const int ry = __builtin_amdgcn_update_dpp(0, sy, 0xB1, 0xF, 0xF, false);
            // even lane: [my hi4 | partner's hi4] at block + 0;  odd lane: [partner's lo4 | my lo4] at block + 16
            const int4 piece = odd ? make_int4(rx, ry, lw2.x, lw2.y) : make_int4(hw2.x, hw2.y, rx, ry);
            *reinterpret_cast<int4*>(reinterpret_cast<char*>(op + 8 * (c >> 1)) + (odd ? 16 : 0)) = piece;
            f16_range_guard(a.guard, m);
        }
    }
}

// ---- split-f16 products on f32 inputs (the split precision mode) -----------------------------------------------------------
// The exact-f32 MFMA (v_mfma_f32_16x16x4_f32: 32 cycles for 2 K flops) makes the shapes above co-bound by the matrix pipe:
// the object -> language attention needs 94 us of it per launch next to 114 us of HBM time at the practical rate, and the two
// do not overlap well at two to four waves per SIMD (measured 204 us = their sum).  In the split precision mode every other
// contraction already runs as hi*hi + hi*lo + lo*hi on f16 MFMAs (22-bit products), and so can these: the K/V tile is
// converted to (hi, lo) halfs while it is staged - K row-major, V TRANSPOSED ([d][key]) so that both MFMA A-fragments are
// single 8-byte LDS reads - Q and P are split in registers, and a product costs 3 x 8 cycles instead of 4 x 32.  The halved
// tile (38 KB for 32 keys) keeps four blocks per CU.  Same block decomposition, addressing and online softmax as above.
// block -> (unit, 64-query block) -> (group, head) for the two split kernels below.  The f32 kernel keeps its own lines (with the XCD
// remap), and the unit's rows and the lane's query stay in the kernels: either way moved a register row (profiles/attn_fwd_bodies_isa.txt).
struct SimpleBlock { int grp, h, qb; };
__device__ __forceinline__ SimpleBlock simple_block(const AttnSArgs& a) {
    SimpleBlock b;
    const long long unit = blockIdx.x / a.nqb;
    b.qb = (int)(blockIdx.x - unit * a.nqb);
    b.grp = (int)(unit / a.H); b.h = (int)(unit - (long long)b.grp * a.H);
    return b;
}
template <int DH, int TK>
__global__ __launch_bounds__(256, 4) void attn_fwd_splitm_kernel(const AttnSArgs a) {
    constexpr int NC = DH / 16;
    constexpr int LDK = DH + 8;   // halfs: K rows, 8-byte fragment reads conflict-free (row pitch = 4 banks mod 64)
    constexpr int LDT = TK + 8;   // halfs: V^T rows (one per head dim), pitch 20 dwords at TK = 32
    constexpr int F4 = DH / 4;
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_m[];
    _Float16* Kh = smem_m;
    _Float16* Kl = Kh + TK * LDK;
    _Float16* Vh = Kl + TK * LDK;   // [DH][LDT]
    _Float16* Vl = Vh + DH * LDT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const SimpleBlock b = simple_block(a);
    const int qb = b.qb, grp = b.grp, h = b.h;
    const AttnUnit u = attn_unit<true>(a, grp);  // a block serves one unit
    const long long q0 = u.q0, k0 = u.k0, q_rs = u.q_rs, k_rs = u.k_rs;
    const int Sq = u.Sq, Sk = u.Sk;
    if (qb * 64 >= Sq) return;
    const int qi = qb * 64 + wave * 16 + c16;
    const bool q_ok = qi < Sq;
    HL4 qs[NC];
    {
        const float* qp = a.q + (q0 + (long long)qi * q_rs) * a.ldq + h * DH + 4 * g4;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 v = q_ok ? *reinterpret_cast<const float4*>(qp + c * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            qs[c] = split4(v.x, v.y, v.z, v.w);
        }
    }
    f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    for (int kt0 = 0; kt0 < Sk; kt0 += TK) {
        const int nrows = min(TK, Sk - kt0);
        const int nrows16 = (nrows + 15) & ~15;
        if (kt0 > 0) __syncthreads();
        for (int idx = tid; idx < nrows16 * F4; idx += 256) {
            const int r = idx / F4, c4 = idx - r * F4;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (r < nrows) {
                const long long row = k0 + (long long)(kt0 + r) * k_rs;
                kv = *reinterpret_cast<const float4*>(a.k + row * a.ldk + h * DH + c4 * 4);
                vv = *reinterpret_cast<const float4*>(a.v + row * a.ldv + h * DH + c4 * 4);
            }
            const HL4 ks = split4(kv.x, kv.y, kv.z, kv.w), vs = split4(vv.x, vv.y, vv.z, vv.w);
            *reinterpret_cast<half4v*>(&Kh[r * LDK + c4 * 4]) = ks.hi;
            *reinterpret_cast<half4v*>(&Kl[r * LDK + c4 * 4]) = ks.lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Vh[(c4 * 4 + j) * LDT + r] = vs.hi[j];
                Vl[(c4 * 4 + j) * LDT + r] = vs.lo[j];
            }
        }
        __syncthreads();
        const int ntile = nrows16 >> 4;
        f32x4 sc[TK / 16];
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
                const int ko = (t * 16 + c16) * LDK + 4 * g4;
                attn_qk_split<NC>(reinterpret_cast<const char*>(&Kh[ko]), reinterpret_cast<const char*>(&Kl[ko]), 32, qs, a0, a1);
                const int key0 = kt0 + t * 16 + 4 * g4;
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[t][r] = (key0 + r < Sk) ? (a0[r] + a1[r]) * a.scale : -INFINITY;
            } else {
                sc[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        // mask-and-scale and the softmax step stay written out: either shared form costs the single-buffered shape 2 - 4 SGPRs
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[t][r]);
        mx = max_xor32(max_xor16(mx));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[t][r] = __expf(sc[t][r] - m_new);
                rs += sc[t][r];
            }
        rs = sum_xor32(sum_xor16(rs));
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int c = 0; c < NC; ++c) oacc[c] *= alpha;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
                const HL4 ps = split4(sc[t][0], sc[t][1], sc[t][2], sc[t][3]);
                const int vo = c16 * LDT + t * 16 + 4 * g4;  // V^T row d = 16c + c16, keys 16t + 4*g4 .. +3
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const HL4 vf = {*reinterpret_cast<const half4v*>(&Vh[vo + c * 16 * LDT]), *reinterpret_cast<const half4v*>(&Vl[vo + c * 16 * LDT])};
                    oacc[c] = mfma3(vf, ps, oacc[c]);
                }
            }
        }
    }
    if (!q_ok) return;
    const float inv = 1.f / l_run;
    attn_store_tile<NC>(a.o + (q0 + (long long)qi * q_rs) * a.ldo + h * DH, g4, oacc, inv, a.o_sp16, a.guard);
}

// ---- split-f16 q / k / v (written as split pairs by the projection GEMMs, GemmDesc::c SP16), high-occupancy shape (round 3) -----
// From ~48 keys per unit on, the exact-f32 products above take as long at the matrix pipe's peak as the traffic takes at the HBM
// peak (object -> language at the headline shape: 82 us against 115 us; inter-object attention over 128 tracks: 219 against 134),
// and the two do not overlap at four waves per SIMD.  attn.hip's kernel for split inputs is the round-1 shape (8 waves, 68 KB of
// LDS: 401 us where the f32 shape above takes 280-324).  Here the split rows go through the SAME block decomposition as the
// f32 shape: a row of 128 values is 16 blocks of [hi8 | lo8] = 512 bytes, K / V tiles are staged with plain 16-byte copies
// (no conversion: the GEMM epilogue did it), and
//   S^T = K Q^T : A = the key's (hi4, lo4) of a 16-wide head-dim chunk - two 8-byte LDS reads - B = Q's, loaded once;
//   O^T = V^T P^T: A = V^T fragments through ds_read_b64_tr_b16 (the 4 x 16 block of four keys x sixteen head dims, each lane
//                 supplying the address of one 8-byte piece of the split row: no transposed copy of V anywhere), B = P split
//                 in registers;
// each product hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x16_f16: 3 x 16 cycles where the f32 shape spends 4 x 32.
// Row pitch 560 bytes: both read patterns conflict-free on the 64-bank LDS.
typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));
// DB: two LDS stages of TK keys, the next tile's rows travel in registers under the current tile's products, one barrier per tile
// (as the f32 shape above).
template <int TK, bool DB = false>
__global__ __launch_bounds__(256, 4) void attn_fwd_spin_kernel(const AttnSArgs a) {
    constexpr int DH = 128, NC = DH / 16;
    constexpr int RB = 560;  // LDS row pitch, bytes (512 + 48)
    constexpr int P16 = DH / 4;  // 16-byte pieces per split row (DH values x 4 bytes)
    extern __shared__ __attribute__((aligned(16))) char smem_p[];
    char* Ks = smem_p;
    char* Vs = smem_p + TK * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const SimpleBlock b = simple_block(a);
    const int qb = b.qb, grp = b.grp, h = b.h;
    const AttnUnit u = attn_unit<true>(a, grp);  // a block serves one unit
    const long long q0 = u.q0, k0 = u.k0, q_rs = u.q_rs, k_rs = u.k_rs;
    const int Sq = u.Sq, Sk = u.Sk;
    if (qb * 64 >= Sq) return;
    const int qi = qb * 64 + wave * 16 + c16;
    const bool q_ok = qi < Sq;
    // byte offset, inside a split row, of the hi4 this lane's 4 head dims of chunk 0 (16c + 4*g4 .. +3); lo4 sits 16 bytes on
    const int frag = (g4 >> 1) * 32 + (g4 & 1) * 8;
    HL4 qs[NC];
    {
        const char* qp = reinterpret_cast<const char*>(a.q + (q0 + (long long)(q_ok ? qi : 0) * q_rs) * a.ldq + h * DH) + frag;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const half4v hv = *reinterpret_cast<const half4v*>(qp + c * 64);
            const half4v lv = *reinterpret_cast<const half4v*>(qp + c * 64 + 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                qs[c].hi[j] = q_ok ? hv[j] : (_Float16)0.f;
                qs[c].lo[j] = q_ok ? lv[j] : (_Float16)0.f;
            }
        }
    }
    f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    // V^T fragment addresses (ds_read_b64_tr_b16): lane p of a 16-lane group supplies the piece (key 4*g4 + (p >> 2), head dims
    // 4 * (p & 3) .. +3 of the chunk) and receives head dim p of the four keys
    const int vfrag = (4 * g4 + (c16 >> 2)) * RB + ((c16 & 3) >> 1) * 32 + (c16 & 1) * 8;
    constexpr int PT = DB ? 2 * TK * P16 / 256 : 1;  // 16-byte pieces per thread and tile (K + V) of the prefetch
    float4 st[PT];
    auto fetch = [&](int kt0) {
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int e = tid + 256 * j, which = e / (TK * P16), r = (e % (TK * P16)) / P16, c4 = e % P16;
            st[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kt0 + r < Sk) {
                const long long row = k0 + (long long)(kt0 + r) * k_rs;
                st[j] = which ? *reinterpret_cast<const float4*>(a.v + row * a.ldv + h * DH + c4 * 4)
                              : *reinterpret_cast<const float4*>(a.k + row * a.ldk + h * DH + c4 * 4);
            }
        }
    };
    if (DB) fetch(0);
    int it = 0;
    for (int kt0 = 0; kt0 < Sk; kt0 += TK, ++it) {
        const int nrows = min(TK, Sk - kt0);
        const int nrows16 = (nrows + 15) & ~15;
        if (DB) {
            Ks = smem_p + (it & 1) * 2 * TK * RB;
            Vs = Ks + TK * RB;
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int e = tid + 256 * j, which = e / (TK * P16), r = (e % (TK * P16)) / P16, c4 = e % P16;
                *reinterpret_cast<float4*>((which ? Vs : Ks) + r * RB + c4 * 16) = st[j];
            }
            __syncthreads();
            if (kt0 + TK < Sk) fetch(kt0 + TK);
        } else {
        if (kt0 > 0) __syncthreads();
        attn_stage_rows<float4, DH, 256>(a.k, a.v, a.ldk, a.ldv, k0, k_rs, kt0, h, nrows, nrows16, tid, reinterpret_cast<float*>(Ks),
                                         reinterpret_cast<float*>(Vs), RB / 4, RB / 4);
        __syncthreads();
        }
        const int ntile = nrows16 >> 4;
        f32x4 sc[TK / 16];
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
                const char* kp = Ks + (t * 16 + c16) * RB + frag;
                attn_qk_split<NC>(kp, kp + 16, 64, qs, a0, a1);
                const int key0 = kt0 + t * 16 + 4 * g4;
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[t][r] = (key0 + r < Sk) ? (a0[r] + a1[r]) * a.scale : -INFINITY;
            } else {
                sc[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        // mask-and-scale and the softmax step stay written out: either shared form costs the single-buffered shape 2 - 4 SGPRs
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[t][r]);
        mx = max_xor32(max_xor16(mx));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[t][r] = __expf(sc[t][r] - m_new);
                rs += sc[t][r];
            }
        rs = sum_xor32(sum_xor16(rs));
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int c = 0; c < NC; ++c) oacc[c] *= alpha;
#pragma unroll
        for (int t = 0; t < TK / 16; ++t) {
            if (t < ntile) {
                const HL4 ps = split4(sc[t][0], sc[t][1], sc[t][2], sc[t][3]);
                const char* vp = Vs + t * 16 * RB + vfrag;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    typedef __attribute__((address_space(3))) short4v lds_s4;
                    const short4v vh4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(vp + c * 64));
                    const short4v vl4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(vp + c * 64 + 16));
                    oacc[c] = mfma3(HL4{__builtin_bit_cast(half4v, vh4), __builtin_bit_cast(half4v, vl4)}, ps, oacc[c]);
                }
            }
        }
    }
    if (!q_ok) return;
    const float inv = 1.f / l_run;
    attn_store_tile<NC>(a.o + (q0 + (long long)qi * q_rs) * a.ldo + h * DH, g4, oacc, inv, a.o_sp16, a.guard);
}

}  // namespace: sola_tune switches are extern (tune.h)
int g_attn_spin_db = 1;  // sola_tune "attn_spin" 2 = single-buffered 32-key stages (A/B)
int g_attn_simple_db = 1;  // sola_tune "attn_simple_db": 1 = double-buffered 16-key stages with register prefetch
int g_attn_simple_remap = 0;  // sola_tune "attn_simple_remap": XCD-contiguous block order; measured no gain (273.8 vs 275.8 us at 64 tracks, 392 vs 400 at 128)
namespace {

// the grid of the three MFMA kernels: one block per (group, head, 64-query block)
int simple_grid(AttnSArgs& a, long long* blocks) {
    a.nqb = (a.Sq + 63) / 64;
    *blocks = (long long)a.G * a.H * a.nqb;
    return attn_grid_ok(*blocks, "attention");
}

template <int DH>
int launch_s(const AttnSArgs& a0, hipStream_t s) {
    AttnSArgs a = a0;
    constexpr int TK = 32;
    long long blocks;
    SOLA_TRY(simple_grid(a, &blocks));
    a.xcd_remap = (g_attn_simple_remap && blocks % 8 == 0) ? 1 : 0;
    // two stages of 16 keys: the LDS footprint of one 32-key stage (34 KB), the next tile prefetched in registers
    const size_t lds_db = (size_t)2 * 2 * 16 * (DH + 4) * sizeof(float);
    const dim3 grid((unsigned)blocks), block(256);
    if (a.in_bf16)  // training forward on bf16 q / k / v
        hipLaunchKernelGGL((attn_fwd_f32_simple_kernel<DH, 16, true, true, true>), grid, block, lds_db, s, a);
    else if (a.lse || a.drop.enabled)  // training forward
        hipLaunchKernelGGL((attn_fwd_f32_simple_kernel<DH, 16, true, true>), grid, block, lds_db, s, a);
    else if (g_attn_simple_db)
        hipLaunchKernelGGL((attn_fwd_f32_simple_kernel<DH, 16, true>), grid, block, lds_db, s, a);
    else
        hipLaunchKernelGGL((attn_fwd_f32_simple_kernel<DH, TK>), grid, block, (size_t)2 * TK * (DH + 4) * sizeof(float), s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

}  // namespace


// sequences of <= 4 steps at head_dim 128, inference (no log-sum-exp, no dropout), f32 q / k / v
bool attention_small_supported(const AttnDesc& d) {
    return !d.lse && !d.drop.enabled && d.in != Elem::SP16 && d.Sq <= 4 && d.Sk <= 4 && d.DH == 128;
}

static AttnSArgs make_sargs(const AttnDesc& d) {
    AttnSArgs a;
    a.q = d.q; a.k = d.k; a.v = d.v; a.o = d.o;
    attn_fill_common(a, d);
    a.lse = d.lse;
    a.drop = d.drop;
    a.nqb = 1; a.xcd_remap = 0;  // the launchers of the MFMA kernels set them (simple_grid, launch_s)
    a.in_bf16 = 0; a.o_skip_f32 = 0;  // f32 rows in, f32 rows out ...
    a.o_cast = nullptr; a.o_side = nullptr; a.o_cast_fmt = 0;  // ... and no operand cast: launch_attention_simple decides otherwise
    return a;
}

int launch_attention_small(const AttnDesc& d, hipStream_t s) {
    const AttnSArgs a = make_sargs(d);
    const SolaProfScope prof = attn_prof_scope(d, s);
    const unsigned blocks = (unsigned)(((long long)d.G * d.H + 7) / 8);  // half a wave per (group, head) unit
    const int need = d.Sq > d.Sk ? d.Sq : d.Sk;                          // steps the instantiation holds: 1, 2 or 4
    if (need <= 1) hipLaunchKernelGGL((attn_fwd_small_kernel<1>), dim3(blocks), dim3(256), 0, s, a);
    else if (need <= 2) hipLaunchKernelGGL((attn_fwd_small_kernel<2>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_fwd_small_kernel<4>), dim3(blocks), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

// f32 q / k / v, more than 16 keys or queries; with a log-sum-exp output / dropout (training) the TR instantiation, f32 output only
int g_attn_simple_train = 1;  // sola_tune "attn_simple_train": 0 = the training forward keeps attn.hip's kernels (A/B)
bool attention_simple_supported(const AttnDesc& d) {
    if ((d.lse || d.drop.enabled) && (!g_attn_simple_train || d.out == Elem::SP16)) return false;
    return d.in != Elem::SP16 && (d.Sq > 16 || d.Sk > 16) && (d.DH == 128 || d.DH == 64);
}
// bfloat16 q / k / v (AttnDesc::in BF16): this file's training instantiation takes them - f32 output or bf16 cast only, 8-value-aligned rows
bool attention_in_bf16_supported(const AttnDesc& d) {
    return g_attn_simple_train && d.out != Elem::SP16 && !d.k_private && (d.Sq > 16 || d.Sk > 16) && (d.DH == 128 || d.DH == 64) &&
           d.ldq % 8 == 0 && d.ldk % 8 == 0 && d.ldv % 8 == 0 && d.ldo % 8 == 0;
}

int launch_attention_simple(const AttnDesc& d, hipStream_t s) {
    AttnSArgs a = make_sargs(d);
    if (d.o_cast && d.o_cast_done && (d.lse || d.drop.enabled || d.in == Elem::BF16) && d.out != Elem::SP16 && d.ldo % 8 == 0) {  // the TR instantiation runs (launch_s)
        a.o_cast = d.o_cast; a.o_side = d.cast == Elem::SP16 ? d.o_side : nullptr; a.o_cast_fmt = (int)d.cast;  // (the kernel reads Elem's values)
        *d.o_cast_done = true;
    }
    a.in_bf16 = d.in == Elem::BF16;
    if (d.in == Elem::BF16) {
        SOLA_ARG(attention_in_bf16_supported(d), "attention: bf16 q / k / v need the high-occupancy training shape (more than 16 queries or keys, head_dim 64 / 128, pitches %% 8 == 0)");
        a.o_skip_f32 = d.o == nullptr;
        SOLA_ARG(d.o || a.o_cast, "attention: no output");
    }
    const SolaProfScope prof = attn_prof_scope(d, s);
    return d.DH == 128 ? launch_s<128>(a, s) : launch_s<64>(a, s);
}

// split-f16 q / k / v (GEMM outputs written as split pairs), head_dim 128, inference: the high-occupancy shape for split inputs
int g_attn_spin = 1;  // sola_tune "attn_spin": 0 = attn.hip's round-1 kernel for split inputs (A/B)
void sola_attn_set_spin(int v) { g_attn_spin = v != 0; g_attn_spin_db = v != 2; }
bool attention_spin_supported(const AttnDesc& d) {
    // units of at most two 64-query blocks (the inter-object attention): with many q-blocks per unit (object -> language) every
    // block re-stages the unit's K / V and attn.hip's resident-K/V loop wins (158 vs 184 us at the headline shape)
    return g_attn_spin && d.in == Elem::SP16 && !d.lse && !d.drop.enabled && d.DH == 128 && (d.Sq > 16 || d.Sk > 16) && (d.Sq <= 128 || d.q_units) &&
           d.ldq % 8 == 0 && d.ldk % 8 == 0 && d.ldv % 8 == 0;
}
int launch_attention_spin(const AttnDesc& d, hipStream_t s) {
    AttnSArgs a = make_sargs(d);
    const SolaProfScope prof = attn_prof_scope(d, s);
    long long blocks;
    SOLA_TRY(simple_grid(a, &blocks));
    // two stages of 16 keys with the next tile prefetched in registers, or one stage of 32 (sola_tune "attn_spin" 2): 35.8 KB either way
    const size_t lds = (size_t)2 * 32 * 560;
    if (g_attn_spin_db) hipLaunchKernelGGL((attn_fwd_spin_kernel<16, true>), dim3((unsigned)blocks), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((attn_fwd_spin_kernel<32>), dim3((unsigned)blocks), dim3(256), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

// f32 q / k / v with the products evaluated as split-f16 triples (AttnDesc::split_math; head_dim 128, inference)
bool attention_splitm_supported(const AttnDesc& d) {
    return d.split_math && !d.lse && !d.drop.enabled && d.in != Elem::SP16 && (d.Sq > 4 || d.Sk > 4) && d.DH == 128;
}
int launch_attention_splitm(const AttnDesc& d, hipStream_t s) {
    AttnSArgs a = make_sargs(d);
    const SolaProfScope prof = attn_prof_scope(d, s);
    long long blocks;
    SOLA_TRY(simple_grid(a, &blocks));
    constexpr int DH = 128, TK = 32;  // K rows as (hi, lo) halfs at pitch DH + 8, V^T rows at pitch TK + 8
    const size_t lds = ((size_t)2 * TK * (DH + 8) + (size_t)2 * DH * (TK + 8)) * sizeof(_Float16);
    hipLaunchKernelGGL((attn_fwd_splitm_kernel<DH, TK>), dim3((unsigned)blocks), dim3(256), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
