// The tile steps of the attention forward kernels (attn.hip, attn_simple.hip, attn_f16.hip, lab/attn_ring.hip), each stated once: score
// mask-and-scale, the online-softmax step, the exact-f32 and split-f16 score products, dropout on a tile's probabilities and plain K/V
// row staging.  All of them work on the S^T = K Q^T / O^T = V^T P^T register layout: lane (c16, g4) holds the scores of query c16
// against keys 16 t + 4 g4 + {0..3} of every 16-key tile t.  A kernel keeps a step written out where the shared form changed its register
// row or its measured time; profiles/attn_fwd_bodies_isa.txt has the table.
#pragma once
#include "attn_common.h"

// ---- scores of one 16-key tile -------------------------------------------------------------------------------------------------
// the two accumulator halves summed and scaled; key0 = the tile's first key of this lane, keys from Sk on are masked
__device__ __forceinline__ f32x4 attn_mask_scale(const f32x4 a0, const f32x4 a1, int key0, int Sk, float scale) {
    f32x4 s;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = (key0 + r < Sk) ? (a0[r] + a1[r]) * scale : -INFINITY;
    return s;
}
// a tile past the staged rows (t >= ntile): no keys
__device__ __forceinline__ f32x4 attn_mask_scale() { return f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}; }

// ---- online softmax over NT score tiles: sc becomes exp(sc - m_new), m_run / l_run move on; returns alpha = exp(m_old - m_new),
// which the caller applies to its accumulators by its own policy.  SWAP: the two lane steps (16, then 32) on common.h's v_permlane swaps
// (lab/attn_ring.hip) or on attn_common.h's __shfl_xor pair (attn.hip) - the same values from different instructions, so a kernel keeps
// the form it was measured with.
template <int NT, bool SWAP>
__device__ __forceinline__ float attn_softmax_tile(f32x4 (&sc)[NT], float& m_run, float& l_run) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[t][r]);
    if constexpr (SWAP) mx = max_xor32(max_xor16(mx));
    else mx = xor16_32_max(mx);
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);  // exp(-inf) = 0 on the first tile
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sc[t][r] = __expf(sc[t][r] - m_new);
            rs += sc[t][r];
        }
    if constexpr (SWAP) rs = sum_xor32(sum_xor16(rs));
    else rs = xor16_32_sum(rs);
    l_run = l_run * alpha + rs;
    m_run = m_new;
    return alpha;
}

// ---- exact-f32 chunk products (v_mfma_f32_16x16x4_f32) from LDS rows ------------------------------------------------------------
// S^T += K Q^T: kp = this lane's key row at head dim 4 g4; chunk c goes to a0 (even) or a1 (odd), four MFMAs each
template <int NC>
__device__ __forceinline__ void attn_qk_f32(const float* kp, const float4 (&qf)[NC], f32x4& a0, f32x4& a1) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float4 kf = *reinterpret_cast<const float4*>(kp + c * 16);
        f32x4& acc = (c & 1) ? a1 : a0;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[c].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[c].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[c].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[c].w, acc, 0, 0, 0);
    }
}
// (O^T += V^T P^T has no shared body: one function over the V row pointer and a tile's probabilities made other kernels of attn.hip's
// shared mode - lower rows, never timed: worth another look with timings - and each kernel keeps its loop.  profiles/attn_fwd_bodies_isa.txt)

// ---- split-f16 chunk products (mfma3) ------------------------------------------------------------------------------------------
// S^T += K Q^T: hi / lo = this lane's (hi4, lo4) pieces of chunk 0 of its key row, chunk c sits `step` bytes further in both
template <int NC>
__device__ __forceinline__ void attn_qk_split(const char* hi, const char* lo, int step, const HL4 (&qs)[NC], f32x4& a0, f32x4& a1) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const HL4 kf = {*reinterpret_cast<const half4v*>(hi + c * step), *reinterpret_cast<const half4v*>(lo + c * step)};
        if (c & 1) a1 = mfma3(kf, qs[c], a1);
        else a0 = mfma3(kf, qs[c], a0);
    }
}

// ---- dropout on the probabilities of NT tiles: element index rbase + kt0 + 16 t + 4 g4 + r of the counter-based mask -------------
// (the normalised probabilities are dropped: the row sum is taken before this)
template <int NT>
__device__ __forceinline__ void attn_dropout_tile(f32x4 (&sc)[NT], const DropoutCfg& drop, unsigned long long rbase, int kt0, int g4) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] = dropout_keep(drop, rbase + kt0 + t * 16 + 4 * g4 + r) ? sc[t][r] * drop.scale : 0.f;
}

// ---- plain K/V staging: nrows16 rows of K and V of head h into LDS, rows from nrows on zero-filled ------------------------------
// P = the 16-byte piece (float4, or half8v of 16-bit values), E = the stored value; pitches in values; t0 / NTHR = the copying threads
template <class P, int DH, int NTHR, class E>
__device__ __forceinline__ void attn_stage_rows(const E* k, const E* v, int ldk, int ldv, long long k0, long long k_rs, int kt0, int h,
                                                int nrows, int nrows16, int t0, E* Ks, E* Vs, int pk, int pv) {
    constexpr int VPP = sizeof(P) / sizeof(E), PPR = DH / VPP;
    for (int idx = t0; idx < nrows16 * PPR; idx += NTHR) {
        const int r = idx / PPR, cp = idx - r * PPR;
        P kv = {}, vv = {};
        if (r < nrows) {
            const long long row = k0 + (long long)(kt0 + r) * k_rs;
            kv = *reinterpret_cast<const P*>(k + row * ldk + h * DH + cp * VPP);
            vv = *reinterpret_cast<const P*>(v + row * ldv + h * DH + cp * VPP);
        }
        *reinterpret_cast<P*>(&Ks[r * pk + cp * VPP]) = kv;
        *reinterpret_cast<P*>(&Vs[r * pv + cp * VPP]) = vv;
    }
}
