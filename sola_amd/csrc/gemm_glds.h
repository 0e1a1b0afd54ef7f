// What the direct-to-LDS split-f16 / 16-bit GEMM kernels share across their files (gemm_glds.hip: the one-tile and persistent NT kernels;
// gemm_tn_tr.hip: the weight-gradient product, which leaves through the same epilogue; lab/gemm_k16.hip and lab/gemm_pp.hip: two closed
// experiments): the kernel arguments, the k-tile constants and the epilogue of the one-tile-per-block kernels.
#pragma once
#include "gemm_common.h"

struct GldsArgs {
    GemmProblem p[3];
    int M, N, K, lda, ldr, ldc;
    int conv, T_in, T_out, stride, pad, Cin;
    const int2* rowmap;  // conv, ragged batches: (source row of tap 0, tap-validity bits) per output row (GemmDesc::rowmap)
    int tiles_m, tiles_n, xcd_remap, nprob;
    int ksplit, kper;  // persistent kernel: > 1 = the reduction dim is cut into ksplit ranges of kper k-tiles, each an own work item
    float* part;       // ... writing raw partial sums to part[(problem * ksplit + range)][M][N] (gemm.hip reduces them)
    float out_scale;
    const float* out_scale_dev;
    int r_sp16, c_sp16;
    int r_f16, c_f16;  // PURE kernels: residual / output stored as _Float16 (ldr / ldc in halfs)
    int bf16;          // PURE kernels: the 16-bit operands are bfloat16 (launch-time selection of the PURE = 2 instantiations)
    const float* bias_scale_dev;  // optional device multiplier of the bias (GemmDesc::bias_scale_dev)
    int ablate;  // measurement only (sola_tune "gemm_ablate"): 4 = no epilogue
    int* guard;  // c_sp16: range guard word (GemmDesc::guard), null = unchecked
    // GNF instantiation of the persistent kernel: GroupNorm (64 channels per group = a wave's 64 output columns, instances of
    // gn_tokens = 4 / 8 / 16 consecutive rows) + LeakyReLU applied to the tile in the epilogue (GemmDesc::gn_gamma)
    const float *gn_gamma, *gn_beta;
    int gn_tokens;
    float gn_eps, gn_slope, gn_icnt;  // gn_icnt = 1 / (gn_tokens * 64)
    // persistent kernel, measurement (sola_tune "gemm_stagger" / "gemm_order" / "gemm_trace"; all 0 in production)
    int stagger;  // > 0: block b sleeps ((b >> 3) % 4) * stagger * 64 clocks before its first tile (de-synchronises the CUs' epilogues)
    // round 6, 16-bit launches whose tiles are not whole rounds of the CUs: the blocks that get one tile FEWER than the others start late, at
    // phases spread over most of a tile's time (slack * 64 clocks per k-tile at phase 1; 0 = off).  Their delay is free - they would idle at
    // the end instead - and their epilogues (and k-loops) no longer coincide with those of the full-count blocks: the HBM bursts of the
    // synchronised epilogues had every CU's matrix pipe waiting at once (sola_tune "gemm_slack_stagger"; profiles/r06_train_ragged_bf16.txt)
    // (carried as a NEGATIVE `stagger`: one more kernel argument cost the f16 conv instantiation a spilled register)
    int order;    // tile order variant (decode())
    unsigned long long* trace;  // TRACE instantiation: per (block, wave) record, see gemm_trace_words
};
constexpr int gemm_trace_words = 8 + 2 * 64;  // 64-bit words per (block, wave): sums, then the tiles' stamps (lane t = tile t of the block)

constexpr int GBK = 32;
constexpr int ROWB = 128;  // bytes per tile row (32 elements x 4 B)

// Epilogue of the one-tile-per-block kernels: shared by the 32-deep and the 16-deep (two blocks per CU) k-loops.
template <int MI, int WAVES_N>
__device__ __forceinline__ void glds_tile_epilogue(const GldsArgs& a, const GemmProblem& pr, f32x16 (&acc)[MI][2], char* lds, int wave, int lane,
                                                   int wr, int wc, int m0, int n0) {
    // ---- epilogue: the accumulators (one column per lane, 16 scattered rows) go through this wave's 16 KiB of the
    //      now idle stage buffers, 64 rows at a time, and leave as whole 16-byte row pieces (16 lanes cover one 256-byte
    //      row segment) instead of 64 strided dword stores per lane.  Bias, output scale and the residual are applied on
    //      the way out.
    if (a.ablate & 4) return;
    const float osc = (a.out_scale_dev ? a.out_scale * *a.out_scale_dev : a.out_scale) * (pr.scale_dev ? *pr.scale_dev : 1.f);
    float* tile = reinterpret_cast<float*>(lds) + wave * (64 * 64);  // [64 rows][64 cols] f32 (256-B rows: b32 writes and b128 reads are conflict-free)
    const int col_l = lane & 31, row_l = (lane >> 5) << 2;
    const int c4 = lane & 15;    // 16-byte column piece
    const int rsub = lane >> 4;  // 4 rows per pass
    const int n = n0 + wc * 64 + c4 * 4;
    const bool vec_ok = (a.ldc & 3) == 0 && n + 3 < a.N && (!pr.R || a.r_sp16 || (a.ldr & 3) == 0);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pr.bias) {
        const float bsc = a.bias_scale_dev ? *a.bias_scale_dev : 1.f;
        bv.x = n < a.N ? pr.bias[n] * bsc : 0.f;
        bv.y = n + 1 < a.N ? pr.bias[n + 1] * bsc : 0.f;
        bv.z = n + 2 < a.N ? pr.bias[n + 2] * bsc : 0.f;
        bv.w = n + 3 < a.N ? pr.bias[n + 3] * bsc : 0.f;
    }
#pragma unroll
    for (int h = 0; h < MI / 2; ++h) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i * 32 + (r & 3) + 8 * (r >> 2) + row_l;
                    const int col = j * 32 + col_l;
                    tile[row * 64 + col] = acc[h * 2 + i][j][r];
                }
        __syncthreads();
#pragma unroll 4
        for (int pass = 0; pass < 16; ++pass) {
            const int row = pass * 4 + rsub;
            const int m = m0 + wr * MI * 32 + h * 64 + row;
            const float4 t = *reinterpret_cast<const float4*>(&tile[row * 64 + c4 * 4]);
            if (m >= a.M) continue;
            float v[4] = {t.x * osc + bv.x, t.y * osc + bv.y, t.z * osc + bv.z, t.w * osc + bv.w};
            if (pr.R) {
                if (a.r_f16) {
                    const _Float16* rb = reinterpret_cast<const _Float16*>(pr.R) + (long long)m * a.ldr + n;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < a.N) v[e] += cvt16_in(rb[e], a.bf16 != 0);
                } else if (a.r_sp16) {
                    // 4 consecutive columns sit in one 8-wide block: hi[4] and lo[4] are two aligned 8-byte loads
                    const _Float16* rb = reinterpret_cast<const _Float16*>(pr.R + (long long)m * a.ldr + (n & ~7)) + (n & 4);
                    if (n + 3 < a.N) {
                        const half4 hh = *reinterpret_cast<const half4*>(rb), ll = *reinterpret_cast<const half4*>(rb + 8);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)hh[e] + (float)ll[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < a.N) v[e] += (float)rb[e] + (float)rb[8 + e];
                    }
                } else if (vec_ok) {
                    const float4 rv = *reinterpret_cast<const float4*>(pr.R + (long long)m * a.ldr + n);
                    v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < a.N) v[e] += pr.R[(long long)m * a.ldr + n + e];
                }
            }
            if (a.c_f16) {
                if (n >= a.N) continue;  // N % 4 == 0: the four columns are in range together
                *reinterpret_cast<half4*>(reinterpret_cast<_Float16*>(pr.C) + (long long)m * a.ldc + n) = cvt16x4_out(v, a.bf16 != 0);
                if (!a.bf16) f16_range_guard4(a.guard, v);
            } else if (a.c_sp16) {
                if (n >= a.N) continue;  // N % 8 == 0 and n % 4 == 0: the four columns are in range together
                // 4 consecutive columns of one 8-wide block: hi[4] and lo[4] leave as two aligned 8-byte stores
                _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * a.ldc + (n & ~7)) + (n & 4);
                half4 hh, ll;
#pragma unroll
                for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                *reinterpret_cast<half4*>(cb) = hh;
                *reinterpret_cast<half4*>(cb + 8) = ll;
                f16_range_guard4(a.guard, v);
            } else if (vec_ok) {
                *reinterpret_cast<float4*>(pr.C + (long long)m * a.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < a.N) pr.C[(long long)m * a.ldc + n + e] = v[e];
            }
        }
        if (h + 1 < MI / 2) __syncthreads();  // this wave's reads of the staging rows are done before they are rewritten
    }
}

#ifdef SOLA_EXPERIMENTS  // closed experiments: EXPERIMENTS=1 builds with sola_tune "gemm_k16" / "gemm_pp" only
int launch_gemm_k16(GldsArgs& a, bool conv, int M, int N, int nprob, hipStream_t s);  // lab/gemm_k16.hip
bool gemm_pp_applies(const GldsArgs& a, int M, int N);                                 // lab/gemm_pp.hip
int launch_gemm_pp(GldsArgs& a, bool conv, int M, int N, int nprob, hipStream_t s);
extern int g_gemm_k16, g_gemm_pp;
#endif
