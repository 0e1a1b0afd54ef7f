// Split-f16 NT GEMM with direct-to-LDS staging (global_load_lds_dwordx4): the staging-bound variant of gemm.hip's
// ARITH 1 kernel.  Same math (three v_mfma_f32_32x32x16_f16 per product on (hi, lo) f16 pairs, f32 accumulate); what
// changes is how a k-tile reaches LDS:
//   * every wave issues eight (or six) 1-KiB LDS-DMA pieces per k-tile: no VGPR round trip, no ds_write, and the source
//     pointers just advance 128 B per k-tile (also for the implicit-im2col conv, see below);
//   * the DMA writes LDS linearly (wave-uniform base + lane * 16 B), so tile rows are 128 contiguous bytes (8 lanes
//     per row, 8 rows per piece) and bank conflicts are removed by an XOR swizzle of the 16-byte chunks,
//     chunk' = chunk ^ ((row >> 1) & 7), applied on the SOURCE address when loading and on the fragment address when
//     reading (the same involution on both sides).  gfx950's LDS has 64 banks (256 B/clk): a ds_read_b128 is served 16
//     lanes at a time, and 16 consecutive rows reading the same logical chunk must land in 16 different 16-byte slots of
//     the 256-byte bank line - (row & 1) picks the half, the key the slot.  (A key of row & 7, right for a 32-bank LDS,
//     measured exactly half the read rate: tools/micro/lds_bw.hip, 69 vs 116 TB/s aggregate.)
//   * conv zero-padding rows read a 16-byte zero page instead (the DMA cannot predicate data); rows beyond M / N are
//     clamped to the last valid row (their products only reach outputs the epilogue never stores).
//
// Schedule: two LDS stages, ONE barrier per k-tile placed between its two 16-wide halves.  By then every wave holds both
// halves' fragments of tile kt in registers (so its stage can take the DMA of tile kt+2) and tile kt+1 has had a whole
// tile time to land, so its first fragments are fetched under the second half's MFMAs: no LDS latency is exposed behind
// a barrier and the DMA always has one full tile of MFMA work (~1.4 us) to cover its latency.
//
// Block shapes <MI, WAVES_M, WAVES_N>:
//   <2,2,2>  128x128, 4 waves of 64x64, 64 KiB LDS, two blocks per CU   - general shape
//   <4,2,4>  256x256, 8 waves of 128x64, 128 KiB, one block per CU      - 25 % fewer fragment bytes and half the DMA
//                                                                         bytes per MFMA; used when its grid fills
//                                                                         whole rounds of one block per CU
// Measured (tools/gemm_ablate.py, tools/pmc_gemm.sh, tools/pmc_clock.sh; M=16384 N=K=1024, 2.05 GHz effective clock):
// 256x256: 107 us total = 63-66 us MFMA+LDS loop alone (matrix pipe busy 68 % of cycles) + ~15 us of imperfect DMA
// overlap + ~28 us epilogue (HBM-bound: C once, residual once; with one round of blocks nothing overlaps it).  Also
// tried and dropped: a 256x128 / 3-stage shape (DMA two tiles ahead: no faster, latency was not the bound) and
// sched_group_barrier interleaving of fragment reads (+2-5 % on 64x64 wave tiles only, subsumed by this schedule).
// Also in this file (round 3): gemm_nt_split_glds_k16_kernel - an experiment, 16-deep k-tiles and two four-wave blocks per CU (slower:
// DESIGN.md Appendix A) - and gemm_tn_tr_kernel, the weight-gradient product on ROW-MAJOR 16-bit operands (transposing LDS reads
// instead of transposed copies; the training modes' default dW route).
#include "kernels.h"
#include <algorithm>
#include <type_traits>

namespace {

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

__device__ __forceinline__ void guard_sp16x4(int* guard, const float (&v)[4]) {
    const float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    if (guard && !(m < 65000.f)) atomicOr(guard, 1);  // NaN fails the comparison too
}

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
// 16-bit outputs / residuals of the PURE kernels: _Float16, or bfloat16 when the operands are (GemmDesc::bf16 with c_f16 / r_f16: the bf16
// STORAGE of the training step, round 6).  Four values as one 8-byte word.
typedef __bf16 bf16x4g __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half4 cvt16x4_out(const float (&v)[4], bool bf) {
    if (bf) {
        bf16x4g b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (__bf16)v[e];
        return __builtin_bit_cast(half4, b);
    }
    half4 hh;
#pragma unroll
    for (int e = 0; e < 4; ++e) hh[e] = (_Float16)v[e];
    return hh;
}
__device__ __forceinline__ float cvt16_in(_Float16 h, bool bf) {
    if (bf) return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned short, h) << 16);
    return (float)h;
}

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __attribute__((aligned(16))) float g_zero_page[4] = {0.f, 0.f, 0.f, 0.f};

constexpr int GBK = 32;
constexpr int ROWB = 128;  // bytes per tile row (32 elements x 4 B)

// bit kk set <=> 0 <= t0 + kk < T_in, for the (at most 8) taps of a conv window starting at time t0
__device__ __forceinline__ int conv_tap_bits(int t0, int T_in) {
    int bits = 0;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) bits |= ((unsigned)(t0 + kk) < (unsigned)T_in) ? (1 << kk) : 0;
    return bits;
}

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
                if (!a.bf16) guard_sp16x4(a.guard, v);
            } else if (a.c_sp16) {
                if (n >= a.N) continue;  // N % 8 == 0 and n % 4 == 0: the four columns are in range together
                // 4 consecutive columns of one 8-wide block: hi[4] and lo[4] leave as two aligned 8-byte stores
                _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * a.ldc + (n & ~7)) + (n & 4);
                half4 hh, ll;
#pragma unroll
                for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                *reinterpret_cast<half4*>(cb) = hh;
                *reinterpret_cast<half4*>(cb + 8) = ll;
                guard_sp16x4(a.guard, v);
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

// PURE = plain f16 operands (GemmDesc::arith 2): the same 128-byte tile rows now hold 64 consecutive halfs instead of 32
// (hi, lo) pairs, so nothing about the DMA, the swizzle or the fragment reads changes - a "hi" chunk is simply halfs
// 16j..16j+7 of the row and the "lo" chunk halfs 16j+8..16j+15 - and a product is hi*hi + lo*lo (two consecutive k-chunks,
// the same permutation of k on both operands) instead of lo*hi + hi*lo + hi*hi: a third of the MFMAs for twice the k.
template <int MI, int WAVES_M, int WAVES_N, bool CONV, int PURE = 0>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64) void gemm_nt_split_glds_kernel(const GldsArgs a) {
    constexpr int GBM = MI * 32 * WAVES_M, GBN = 64 * WAVES_N;
    constexpr int STAGES = 2;
    constexpr int STAGE_BYTES = (GBM + GBN) * ROWB;
    constexpr int NWAVE = WAVES_M * WAVES_N;
    constexpr int APW = GBM / 8 / NWAVE, WPW = GBN / 8 / NWAVE;  // 8-row DMA pieces per wave per k-tile
    static_assert(APW * NWAVE * 8 == GBM && WPW * NWAVE * 8 == GBN, "tile rows must split evenly over the waves");
    static_assert(NWAVE * 64 * 64 * 4 <= STAGES * STAGE_BYTES, "epilogue staging must fit in the stage buffers");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const GemmProblem pr = a.p[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    int rt, ct;
    {
        const int bid = blockIdx.x;
        if (a.xcd_remap) {
            const int x = bid & 7, j = bid >> 3;
            rt = x + 8 * (j / a.tiles_n);
            ct = j % a.tiles_n;
        } else {
            rt = bid / a.tiles_n;
            ct = bid % a.tiles_n;
        }
    }
    const int m0 = rt * GBM, n0 = ct * GBN;

    // ---- DMA coordinates: this wave owns row groups wave*APW + i (8 rows each) of the A tile and wave*WPW + i of the
    //      W tile; lane -> (row = rg*8 + lane/8, physical 16-byte chunk = lane%8).  Each piece keeps a running source
    //      pointer that advances 128 B per k-tile: also for the implicit-im2col conv, where the receptive field of an
    //      output row is (t0*Cin + k) contiguous floats of the channels-last input, so only the zero-padding test
    //      depends on k.
    const int lrow = lane >> 3, chunk = lane & 7;
    const char* a_ptr[APW];
    const char* w_ptr[WPW];
    int a_t0[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = (wave * APW + i) * 8 + lrow;     // tile-local A row
        const int col_bytes = (chunk ^ ((r >> 1) & 7)) * 16;  // logical 16-byte chunk that must land in this physical slot
        const int m = min(m0 + r, a.M - 1);
        if (CONV) {
            // a_t0 = validity bits of the window's taps (bit kk: tap kk lies inside the sequence)
            if (a.rowmap) {
                const int2 rm = a.rowmap[m];
                a_t0[i] = rm.y;
                a_ptr[i] = reinterpret_cast<const char*>(pr.A) + (long long)rm.x * a.Cin * 4 + col_bytes;
            } else {
                const int rr = m / a.T_out, to = m - rr * a.T_out;
                const int t0 = to * a.stride - a.pad;
                a_t0[i] = conv_tap_bits(t0, a.T_in);
                a_ptr[i] = reinterpret_cast<const char*>(pr.A) + ((long long)rr * a.T_in + t0) * a.Cin * 4 + col_bytes;
            }
        } else {
            a_t0[i] = 0;
            a_ptr[i] = reinterpret_cast<const char*>(pr.A + (long long)m * a.lda) + col_bytes;
        }
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int r = (wave * WPW + i) * 8 + lrow;  // tile-local W row
        const int n = min(n0 + r, a.N - 1);
        w_ptr[i] = reinterpret_cast<const char*>(pr.W + (long long)n * a.K) + (chunk ^ ((r >> 1) & 7)) * 16;
    }
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int nk = a.K / GBK;
    int conv_kk = 0, conv_c = 0;  // CONV: tap index and channel offset of the next k-tile to issue (uniform)
    int dma_kt = 0;               // index of the next k-tile to issue

    // Issues k-tiles in increasing order, one per call.  It is called once per loop iteration without a condition (the
    // eight pieces are interleaved with the MFMAs by sched_group_barrier, which needs one basic block): past the last
    // k-tile the pointers stop advancing, so the surplus calls re-read the last k-tile into a stage nobody reads.
    auto issue = [&](int stage) {
        char* sbase = lds + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const char* src = a_ptr[i];
            if (CONV) src = ((a_t0[i] >> conv_kk) & 1) ? src : zero;  // zero padding in time
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + (wave * APW + i) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)w_ptr[i], (lptr_t)(sbase + GBM * ROWB + (wave * WPW + i) * 1024), 16, 0, 0);
        }
        const bool more = dma_kt + 1 < nk;
        const int adv = more ? GBK * 4 : 0;
#pragma unroll
        for (int i = 0; i < APW; ++i) a_ptr[i] += adv;
#pragma unroll
        for (int i = 0; i < WPW; ++i) w_ptr[i] += adv;
        if (CONV) {  // branch-free: a branch here would split the basic block the DMA is interleaved in
            conv_c += more ? GBK : 0;
            const bool wrap = conv_c == a.Cin;
            conv_c = wrap ? 0 : conv_c;
            conv_kk += wrap ? 1 : 0;
        }
        ++dma_kt;
    };

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment addresses of this lane; the swizzle key (row >> 1) & 7 is the same for all its rows (they differ by multiples of 32)
    const int fr = lane & 31, fh = lane >> 5, key = (lane >> 1) & 7;
    const int a_frag = (wr * MI * 32 + fr) * ROWB, w_frag = GBM * ROWB + (wc * 64 + fr) * ROWB;

    struct Frags { half8 ah[MI], al[MI], bh[2], bl[2]; };
    auto load_frags = [&](const char* sbase, int s16, Frags& f) {
        const int hi_off = (((s16 * 2 + fh) * 2) ^ key) << 4;  // physical slot of the block's hi chunk
        const int lo_off = hi_off ^ 16;                           // ... and of its lo chunk (logical chunk + 1)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* q = sbase + w_frag + j * 32 * ROWB;
            f.bh[j] = *reinterpret_cast<const half8*>(q + hi_off);
            f.bl[j] = *reinterpret_cast<const half8*>(q + lo_off);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const char* p = sbase + a_frag + i * 32 * ROWB;
            f.ah[i] = *reinterpret_cast<const half8*>(p + hi_off);
            f.al[i] = *reinterpret_cast<const half8*>(p + lo_off);
        }
    };
    auto mfmas = [&](const Frags& f) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (PURE == 2) {  // bf16 operands: the same 16-byte chunks, v_mfma_f32_32x32x16_bf16
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.al[i]), __builtin_bit_cast(bf16x8, f.bl[j]), acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.ah[i]), __builtin_bit_cast(bf16x8, f.bh[j]), acc[i][j], 0, 0, 0);
                } else if constexpr (PURE == 1) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
                } else {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
                }
            }
    };

    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int stage = 0;
    Frags f0, f1;
    load_frags(lds, 0, f0);
    issue(1);
    constexpr int NRD = 2 * MI + 4, NMF = (PURE ? 4 : 6) * MI;  // fragment reads and MFMAs of one half
    constexpr int NDMA = APW + WPW, DMA_GAP = (NMF - 1) / NDMA;  // one DMA piece behind every DMA_GAP MFMAs of the second half
    for (int kt = 0; kt < nk; ++kt) {
        // Each half = one MFMA batch with the NEXT half's fragment reads issued right behind its first MFMA.  The compiler
        // waits lgkmcnt(0) in front of a batch (scalar loads in the loop keep it from counting LDS returns), so reads
        // issued just before a batch - where the scheduler puts them on its own, to shorten live ranges - stall that
        // batch for the whole LDS latency of 8 waves reading at once; behind the first MFMA they have a batch to land.
        load_frags(lds + stage * STAGE_BYTES, 1, f1);
        mfmas(f0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile kt+1 has landed (issued one tile time ago)
        __syncthreads();                                   // ... and nobody reads this stage any more
        __builtin_amdgcn_sched_barrier(0);
        // The eight DMA pieces of k-tile kt+2 are spread over this half's MFMAs: issued back to back behind the barrier
        // by all eight waves at once they queue in the CU's one texture-address unit (1 KiB per instruction = 16 clocks),
        // and a wave stuck at a full memory queue issues no MFMAs either (measured: +800 clocks per k-tile).
        load_frags(lds + (stage ^ 1) * STAGE_BYTES, 0, f0);  // past the last tile this reads stale LDS and is never used
        issue(stage);  // after the reads in program order: the compiler cannot tell the two stages apart and keeps LDS accesses ordered
        mfmas(f1);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
#pragma unroll
        for (int g = 0; g < NDMA; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, DMA_GAP, 0);
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - NDMA * DMA_GAP, 0);
        __builtin_amdgcn_sched_barrier(0);
        stage ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the surplus DMA of the last iterations must not land in the epilogue's staging
    __syncthreads();

    glds_tile_epilogue<MI, WAVES_N>(a, pr, acc, lds, wave, lane, wr, wc, m0, n0);
}


// ---- 16-deep k-tiles, two blocks per CU (experiment, sola_tune "gemm_k16") ------------------------------------------
// What the persistent kernel cannot hide is its epilogue: one block owns the CU, so while its eight waves drain a tile the
// matrix pipes idle.  Here a block is FOUR waves (one per SIMD) on a 256x128 tile with the same 128x64 wave tiles, and its
// LDS is small enough for TWO blocks per CU (3 stages x 24 KiB): the second block's k-loop runs under the first one's
// epilogue and prologue, and in the loop the two blocks give every SIMD its two waves back.  That needs k-tiles of 16:
//   * tile rows are 64 bytes (4 chunks of 16 B: hi/lo of two 8-wide k-blocks), a 1-KiB DMA piece is 16 rows; the chunk
//     swizzle key is (row >> 2) & 3 (16 consecutive rows x one logical chunk = 16 distinct slots of the 256-byte bank line);
//   * one k-tile is ONE MFMA batch (24 MFMAs, 16 with plain 16-bit operands); the next tile's 12 fragment reads go behind
//     its first MFMA and the 6 DMA pieces of the tile three ahead are spread over the rest;
//   * three stages: tile kt+1 is read, kt+2 is landing, kt+3 is issued into the stage tile kt's fragments came from (every
//     wave has them in registers behind the barrier).  One barrier per k-tile; the DMA has two batches to land.
template <bool CONV, int PURE = 0>
__global__ __launch_bounds__(256, 2) void gemm_nt_split_glds_k16_kernel(const GldsArgs a) {
    constexpr int MI = 4, WAVES_N = 2, NWAVE = 4;
    constexpr int GBM = 256, GBN = 128, KB = 16, RB = 64;
    constexpr int STAGES = 3, STAGE_BYTES = (GBM + GBN) * RB;
    constexpr int APW = GBM / 16 / NWAVE, WPW = GBN / 16 / NWAVE;  // 16-row DMA pieces per wave per k-tile
    static_assert(NWAVE * 64 * 64 * 4 <= STAGES * STAGE_BYTES, "epilogue staging must fit in the stage buffers");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const GemmProblem pr = a.p[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    int rt, ct;
    {
        const int bid = blockIdx.x;
        if (a.xcd_remap) {
            const int x = bid & 7, j = bid >> 3;
            rt = x + 8 * (j / a.tiles_n);
            ct = j % a.tiles_n;
        } else {
            rt = bid / a.tiles_n;
            ct = bid % a.tiles_n;
        }
    }
    const int m0 = rt * GBM, n0 = ct * GBN;

    // DMA coordinates: lane -> (row = piece * 16 + lane / 4, physical chunk = lane % 4)
    const int lrow = lane >> 2, chunk = lane & 3;
    const char* a_ptr[APW];
    const char* w_ptr[WPW];
    int a_t0[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = (wave * APW + i) * 16 + lrow;
        const int col_bytes = (chunk ^ ((r >> 2) & 3)) * 16;
        const int m = min(m0 + r, a.M - 1);
        if (CONV) {
            if (a.rowmap) {
                const int2 rm = a.rowmap[m];
                a_t0[i] = rm.y;
                a_ptr[i] = reinterpret_cast<const char*>(pr.A) + (long long)rm.x * a.Cin * 4 + col_bytes;
            } else {
                const int rr = m / a.T_out, to = m - rr * a.T_out;
                const int t0 = to * a.stride - a.pad;
                a_t0[i] = conv_tap_bits(t0, a.T_in);
                a_ptr[i] = reinterpret_cast<const char*>(pr.A) + ((long long)rr * a.T_in + t0) * a.Cin * 4 + col_bytes;
            }
        } else {
            a_t0[i] = 0;
            a_ptr[i] = reinterpret_cast<const char*>(pr.A + (long long)m * a.lda) + col_bytes;
        }
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int r = (wave * WPW + i) * 16 + lrow;
        const int n = min(n0 + r, a.N - 1);
        w_ptr[i] = reinterpret_cast<const char*>(pr.W + (long long)n * a.K) + (chunk ^ ((r >> 2) & 3)) * 16;
    }
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int nk = a.K / KB;
    int conv_kk = 0, conv_c = 0;
    int dma_kt = 0;

    auto issue = [&](int stage) {  // k-tiles in increasing order, one per call; past the last one the pointers stop (see the kernel above)
        char* sbase = lds + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const char* src = a_ptr[i];
            if (CONV) src = ((a_t0[i] >> conv_kk) & 1) ? src : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + (wave * APW + i) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)w_ptr[i], (lptr_t)(sbase + GBM * RB + (wave * WPW + i) * 1024), 16, 0, 0);
        }
        const bool more = dma_kt + 1 < nk;
        const int adv = more ? KB * 4 : 0;
#pragma unroll
        for (int i = 0; i < APW; ++i) a_ptr[i] += adv;
#pragma unroll
        for (int i = 0; i < WPW; ++i) w_ptr[i] += adv;
        if (CONV) {
            conv_c += more ? KB : 0;
            const bool wrap = conv_c == a.Cin;
            conv_c = wrap ? 0 : conv_c;
            conv_kk += wrap ? 1 : 0;
        }
        ++dma_kt;
    };

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5, key = (lane >> 2) & 3;  // the key is the same for all of a lane's rows (they differ by multiples of 32)
    const int a_frag = (wr * MI * 32 + fr) * RB, w_frag = GBM * RB + (wc * 64 + fr) * RB;
    const int hi_off = ((fh * 2) ^ key) << 4, lo_off = hi_off ^ 16;

    // The fragment reads are inline asm: in front of a compiler-visible LDS read the waitcnt pass puts vmcnt(0) (LDS-DMA pieces are in
    // flight, and it cannot tell the stages apart), which would cut the DMA's two batches of cover to none.  land() is their wait: it
    // names the fragments as in/out operands, so every use of them is ordered behind it.
    struct Frags { half8 ah[MI], al[MI], bh[2], bl[2]; };
    const unsigned a_hi = (unsigned)(a_frag + hi_off), a_lo = (unsigned)(a_frag + lo_off);
    const unsigned w_hi = (unsigned)(w_frag + hi_off), w_lo = (unsigned)(w_frag + lo_off);
#define K16_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr) : "memory")
    auto load_frags = [&](int stage, Frags& f) {
        const unsigned sb = (unsigned)(uintptr_t)(lptr_t)lds + (unsigned)(stage * STAGE_BYTES);
        const unsigned wh = sb + w_hi, wl = sb + w_lo, ah = sb + a_hi, al = sb + a_lo;
        K16_RD(f.bh[0], wh, 0);
        K16_RD(f.bl[0], wl, 0);
        K16_RD(f.bh[1], wh, 2048);
        K16_RD(f.bl[1], wl, 2048);
        K16_RD(f.ah[0], ah, 0);
        K16_RD(f.al[0], al, 0);
        K16_RD(f.ah[1], ah, 2048);
        K16_RD(f.al[1], al, 2048);
        K16_RD(f.ah[2], ah, 4096);
        K16_RD(f.al[2], al, 4096);
        K16_RD(f.ah[3], ah, 6144);
        K16_RD(f.al[3], al, 6144);
    };
#undef K16_RD
    static_assert(MI == 4 && 32 * RB == 2048, "the offsets above");
    auto land = [&](Frags& f, auto vm) {  // the DMA of the next k-tile and this wave's fragment reads are complete
        asm volatile("s_waitcnt vmcnt(%12) lgkmcnt(0)"
                     : "+v"(f.ah[0]), "+v"(f.ah[1]), "+v"(f.ah[2]), "+v"(f.ah[3]), "+v"(f.al[0]), "+v"(f.al[1]), "+v"(f.al[2]), "+v"(f.al[3]),
                       "+v"(f.bh[0]), "+v"(f.bh[1]), "+v"(f.bl[0]), "+v"(f.bl[1])
                     : "n"(decltype(vm)::value)
                     : "memory");
    };
    auto mfma1 = [&](const Frags& f, int i, int j, int which) {
        if constexpr (PURE == 2) {
            if (which == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.al[i]), __builtin_bit_cast(bf16x8, f.bl[j]), acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.ah[i]), __builtin_bit_cast(bf16x8, f.bh[j]), acc[i][j], 0, 0, 0);
        } else if constexpr (PURE == 1) {
            if (which == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bl[j], acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
        } else {
            if (which == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
            else if (which == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
        }
    };
    constexpr int PER = PURE ? 2 : 3;  // MFMAs per accumulator and k-tile, in the order lo terms first (as in the kernels above)
    auto mfmas_rest = [&](const Frags& f) {  // everything but (0, 0, term 0), which the step issues in front of the fragment reads
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int w = 0; w < PER; ++w)
                    if (i || j || w) mfma1(f, i, j, w);
    };

    constexpr int NMF = PER * 2 * MI;
    constexpr int NDMA = APW + WPW, DMA_GAP = (NMF - 1) / NDMA;
    issue(0);
    issue(1);
    issue(2);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NDMA) : "memory");  // k-tile 0 is the oldest third of what is in flight
    __builtin_amdgcn_s_barrier();
    Frags f0, f1;
    load_frags(0, f0);
    int s0 = 0;  // stage of k-tile kt (whose fragments are in registers): it takes the DMA of k-tile kt + 3
    auto step = [&](Frags& cur, Frags& nx) {
        land(cur, std::integral_constant<int, NDMA>());  // k-tile kt+1 has landed (kt+2 may still be in flight); cur is in registers
        __builtin_amdgcn_s_barrier();                    // ... for every wave, and nobody reads stage s0 any more
        __builtin_amdgcn_sched_barrier(0);
        const int s1 = s0 == 2 ? 0 : s0 + 1;
        mfma1(cur, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(s1, nx);  // behind the first MFMA: a batch to land
        __builtin_amdgcn_sched_barrier(0);
        issue(s0);
        mfmas_rest(cur);
#pragma unroll
        for (int g = 0; g < NDMA; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, DMA_GAP, 0);
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - NDMA * DMA_GAP, 0);
        __builtin_amdgcn_sched_barrier(0);
        s0 = s1;
    };
    for (int kt = 0; kt < nk; kt += 2) {  // K is a multiple of 32: an even number of 16-deep k-tiles
        step(f0, f1);
        step(f1, f0);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the surplus DMA and fragment reads of the last iteration must not reach the epilogue's staging
    __syncthreads();

    glds_tile_epilogue<MI, WAVES_N>(a, pr, acc, lds, wave, lane, wr, wc, m0, n0);
}


// ---- weight gradients without transposed copies: dW[n][k] = sum_m dY[m][n] X[m][k] on ROW-MAJOR 16-bit operands -------------------
// The reduction runs over the rows of both operands.  gemm_tn_split.hip's first route writes both matrices transposed (a streaming
// pass of its own per operand, 12 % of a ragged training step) and runs the NT kernel above; this kernel reads the row-major 16-bit
// casts the step has anyway (dY's is the dX GEMM's operand, X's the forward GEMM's) and transposes on the way from LDS to the
// matrix pipe with gfx950's ds_read_b64_tr_b16: a k-tile is 64 rows x 256 columns of each operand (512-byte rows, two rows per 1-KiB
// DMA piece), and a 4 (rows) x 16 (columns) block read by sixteen lanes - each supplying the address of one 8-byte piece - comes
// back with lane j holding column j's four row values, i.e. half of a 32x32x16 MFMA operand.  The 16-byte chunks of a row are
// XOR-swizzled by 4 * (row & 3): the eight rows one instruction touches (r..r+3 and r+8..r+11, 64 bytes each) then spread over all
// sixteen 16-byte slots of the 256-byte bank line, two each - the minimum for a 512-byte read.
// Same block shape, stages, halves and accumulator layout as the 256x256 NT kernel; split over the reduction like its ksplit mode:
// work item = (tile, row range), partial sums to `part` for gemm.hip's ordered reduce.  Rows beyond M read the zero page.
struct TnTrArgs {
    GldsArgs e;  // the epilogue's view: M x N = the dW tile grid (N_out x K_out), ldc, part, ksplit, tiles_m / tiles_n
    const char* A[3];      // dY as 16-bit rows [Mred][lda]
    const char* B[3];      // X as 16-bit rows [Mred][ldb]
    long long lda, ldb;    // row pitch in BYTES
    int a_sp, b_sp;        // 1: the operand is a SPLIT-f16 row-major matrix (8-value blocks [hi8 | lo8], 4 bytes per value) and the
                           // kernel takes its hi halves - exactly the plain f16 cast of the same values - by fetching every other
                           // 16-byte chunk (the split-f16 step's dX operand doubles as the dW operand: no second cast of dY)
    int Mred, kper, nkt;   // rows of the reduction; 64-row k-tiles per range / in total
    // CONV kernels: B is the channels-last conv input [rows_in][Cin] and the product's column k = tap * Cin + ci (implicit im2col; a
    // 256-column tile lies inside one tap: Cin % 256 == 0).  Reduction row m = (sequence r, output step to) reads source row
    // r * T_in + to * stride + tap - pad, zeros outside [0, T_in); or, with rowmap (ragged batches), row rowmap[m].x + tap where bit
    // `tap` of rowmap[m].y is set (GemmDesc::rowmap).
    int Cin, T_in, T_out, stride, pad;
    const int2* rowmap;
};

typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));

template <int BF, int CONV = 0>  // CONV: 0 = plain rows, 1 = conv taps by geometry, 2 = conv taps by rowmap
__global__ __launch_bounds__(512) void gemm_tn_tr_kernel(const TnTrArgs t) {
    constexpr int MI = 4, WAVES_N = 4, NWAVE = 8, KT = 64;
    constexpr int OPB = KT * 512, STAGE_BYTES = 2 * OPB;  // one operand's k-tile, one stage (A then B)
    constexpr int PPW = KT / 2 / NWAVE;                   // two-row DMA pieces per wave, operand and k-tile
    static_assert(NWAVE * 64 * 64 * 4 <= 2 * STAGE_BYTES, "epilogue staging must fit in the stage buffers");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const GldsArgs& a = t.e;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int tiles = a.tiles_m * a.tiles_n;
    int range, tile;
    {   // consecutive block ids go to different XCDs: the tiles of one row range (they share its rows) stay on one XCD's L2
        const int bid = blockIdx.x;
        if ((a.ksplit & 7) == 0) {
            const int x = bid & 7, q = bid >> 3;
            range = x + 8 * (q / tiles);
            tile = q % tiles;
        } else {
            range = bid / tiles;
            tile = bid % tiles;
        }
    }
    const int m0 = (tile / a.tiles_n) * 256, n0 = (tile % a.tiles_n) * 256;  // origin of the dW tile: row (dY column), column (X column)
    const int kt0 = range * t.kper;
    const int nk = min(t.nkt, kt0 + t.kper) - kt0;
    const long long mstart = (long long)kt0 * KT;

    // DMA coordinates: piece P = wave * PPW + i holds rows 2P, 2P+1 (lane / 32) of the k-tile; row & 3 = 2 * (i & 1) + lane / 32, so the
    // swizzled source column is the same for pieces i and i + 2 (four rows apart): one pointer per parity and operand
    const int prow = lane >> 5, pch = lane & 31;
    const char* Ab = t.A[blockIdx.z];
    const char* Bb = t.B[blockIdx.z];
    const int row0 = wave * PPW * 2 + prow;
    const char* a_ptr[2];
    const char* b_ptr[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int row = row0 + 2 * e;
        const int logical = pch ^ (4 * (row & 3));
        a_ptr[e] = Ab + (mstart + row) * t.lda + ((long long)(m0 * 2 + logical * 16) << t.a_sp);
        b_ptr[e] = Bb + (mstart + row) * t.ldb + ((long long)(n0 * 2 + logical * 16) << t.b_sp);
    }
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int rem0 = (int)min((long long)t.Mred - mstart, 1LL << 30);
    int rem_a = rem0, rem_b = rem0;  // rows left from the start of the next k-tile to issue, per operand
    const long long a_adv = (long long)KT * t.lda, b_adv = (long long)KT * t.ldb;
    const long long a_r4 = 4 * t.lda, b_r4 = 4 * t.ldb;  // four rows further
    // one operand's k-tile per call, in order; surplus calls behind the range fill a stage nobody reads; rows beyond M read zeros
    auto issue_a = [&](int stage) {
        char* sbase = lds + stage * STAGE_BYTES + wave * PPW * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const char* src = a_ptr[i & 1] + (i >> 1) * a_r4;
            __builtin_amdgcn_global_load_lds((gptr_t)(row0 + 2 * i < rem_a ? src : zero), (lptr_t)(sbase + i * 1024), 16, 0, 0);
        }
        a_ptr[0] += a_adv;
        a_ptr[1] += a_adv;
        rem_a -= KT;
    };
    // CONV: the tile's tap and first channel; per piece the (sequence, step) of its row (geometry) or the prefetched rowmap entry
    const int tap = CONV ? n0 / t.Cin : 0;
    const int bcol = CONV ? ((n0 - tap * t.Cin) * 2 + (pch ^ (4 * (row0 & 3))) * 16) << t.b_sp : 0;  // even pieces; odd ones flip chunk bit 3
    const int bcol_odd = CONV ? ((n0 - tap * t.Cin) * 2 + (pch ^ (4 * ((row0 + 2) & 3))) * 16) << t.b_sp : 0;
    int c_rr[PPW], c_to[PPW];
    int2 c_rm[PPW];
    const int q64 = CONV == 1 ? KT / t.T_out : 0, r64 = CONV == 1 ? KT % t.T_out : 0;
    long long m_b = mstart;  // first row of the next B k-tile to issue
    if constexpr (CONV == 1) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const long long m = mstart + row0 + 2 * i;
            c_rr[i] = (int)(m / t.T_out);
            c_to[i] = (int)(m - (long long)c_rr[i] * t.T_out);
        }
    }
    if constexpr (CONV == 2) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) c_rm[i] = t.rowmap[min(mstart + row0 + 2 * i, (long long)t.Mred - 1)];
    }
    auto issue_b = [&](int stage) {
        char* sbase = lds + stage * STAGE_BYTES + OPB + wave * PPW * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const char* src;
            bool ok = row0 + 2 * i < rem_b;
            if constexpr (CONV == 0) {
                src = b_ptr[i & 1] + (i >> 1) * b_r4;
            } else {
                long long srow;
                if constexpr (CONV == 1) {
                    const int ti = c_to[i] * t.stride + tap - t.pad;
                    ok = ok && (unsigned)ti < (unsigned)t.T_in;
                    srow = (long long)c_rr[i] * t.T_in + ti;
                    c_rr[i] += q64;
                    c_to[i] += r64;
                    const bool wrap = c_to[i] >= t.T_out;
                    c_to[i] -= wrap ? t.T_out : 0;
                    c_rr[i] += wrap ? 1 : 0;
                } else {
                    ok = ok && ((c_rm[i].y >> tap) & 1);
                    srow = (long long)c_rm[i].x + tap;
                }
                src = Bb + srow * t.ldb + ((i & 1) ? bcol_odd : bcol);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)(ok ? src : zero), (lptr_t)(sbase + i * 1024), 16, 0, 0);
        }
        if constexpr (CONV == 0) {
            b_ptr[0] += b_adv;
            b_ptr[1] += b_adv;
        }
        rem_b -= KT;
        if constexpr (CONV == 2) {  // the next k-tile's entries: a k-tile (and its barrier's vmcnt(0)) ahead of their use
            m_b += KT;
#pragma unroll
            for (int i = 0; i < PPW; ++i) c_rm[i] = t.rowmap[min(m_b + row0 + 2 * i, (long long)t.Mred - 1)];
        }
    };

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposing fragment reads: sixteen-lane group (g2, g1) = (k half of the operand, 16-column half of the 32-wide fragment);
    // lane j of the group addresses row j >> 2 of the group's four rows, 8-byte piece j & 3 of its 16 columns
    const int j16 = lane & 15, g1 = (lane >> 4) & 1, g2 = lane >> 5;
    const int q = j16 >> 2;  // = row & 3 of every row this lane addresses: the swizzle key
    const int lane_off = (8 * g2 + q) * 512 + (2 * g1 + ((j16 & 3) >> 1)) * 16 + 8 * (j16 & 1);
    int a_off[MI], b_off[2];
#pragma unroll
    for (int i = 0; i < MI; ++i) a_off[i] = lane_off + ((wr * 4 + (i ^ q)) << 6);
#pragma unroll
    for (int j = 0; j < 2; ++j) b_off[j] = OPB + lane_off + (((wc * 2 + j) ^ q) << 6);

    // The fragment reads are inline asm (as in the k16 kernel above): in front of a compiler-visible LDS read the waitcnt pass puts
    // vmcnt(0) while LDS-DMA pieces are in flight, which would expose the whole DMA latency once per k-tile.  land() is their wait.
    struct Frags { half8 a[MI], b[2]; };  // one 16-row step
    const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)lds;
#define TR_RD(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:" #off : "=v"(dst) : "v"(addr) : "memory")
#define TR_STEP(f, base, OFF)                                                                                                        \
    {                                                                                                                                \
        short4v l_, h_;                                                                                                              \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                              \
            TR_RD(l_, base + b_off[j], OFF); TR_RD(h_, base + b_off[j], OFF + 2048);                                                 \
            f.b[j] = __builtin_bit_cast(half8, __builtin_shufflevector(l_, h_, 0, 1, 2, 3, 4, 5, 6, 7));                             \
        }                                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < MI; ++i) {                                                                             \
            TR_RD(l_, base + a_off[i], OFF); TR_RD(h_, base + a_off[i], OFF + 2048);                                                 \
            f.a[i] = __builtin_bit_cast(half8, __builtin_shufflevector(l_, h_, 0, 1, 2, 3, 4, 5, 6, 7));                             \
        }                                                                                                                            \
    }
    auto land = [&](Frags& f) {  // this wave's fragment reads are complete; every use of f is ordered behind this
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]), "+v"(f.b[1])::"memory");
    };
    auto mfma1 = [&](const Frags& f, int i, int j) {
        if constexpr (BF) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.a[i]), __builtin_bit_cast(bf16x8, f.b[j]), acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[i], f.b[j], acc[i][j], 0, 0, 0);
    };
    auto mfmas_rest = [&](const Frags& f) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (i || j) mfma1(f, i, j);
    };
    constexpr int NMF = 2 * MI;  // MFMAs of one 16-row step
    auto spread_dma = [&]() {    // the PPW DMA pieces of one operand, one behind each of the step's following MFMAs
#pragma unroll
        for (int g = 0; g < PPW; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - PPW, 0);
    };

    // A k-tile is four 16-row steps on two alternating fragment sets; the next step's reads go right behind a step's first MFMA.
    // ONE barrier per k-tile, in front of its last step: by then every wave has its last fragments of the stage in registers (so the
    // stage can take the DMA of k-tile kt+2: A during that last step, B during the next k-tile's first) and k-tile kt+1 has had three
    // steps to land, so its first fragments are fetched under the last step's MFMAs.
    issue_a(0);
    issue_b(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int stage = 0;
    Frags f0, f1;
    TR_STEP(f0, lds0, 0);
    issue_a(1);
    for (int kt = 0; kt < nk; ++kt) {
        const unsigned cur = lds0 + (unsigned)(stage * STAGE_BYTES), nxt = lds0 + (unsigned)((stage ^ 1) * STAGE_BYTES);
        // step 0
        land(f0);
        __builtin_amdgcn_sched_barrier(0);
        mfma1(f0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        TR_STEP(f1, cur, 8192);
        __builtin_amdgcn_sched_barrier(0);
        issue_b(stage ^ 1);
        mfmas_rest(f0);
        spread_dma();
        __builtin_amdgcn_sched_barrier(0);
        // step 1
        land(f1);
        __builtin_amdgcn_sched_barrier(0);
        mfma1(f1, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        TR_STEP(f0, cur, 16384);
        __builtin_amdgcn_sched_barrier(0);
        mfmas_rest(f1);
        __builtin_amdgcn_sched_barrier(0);
        // step 2
        land(f0);
        __builtin_amdgcn_sched_barrier(0);
        mfma1(f0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        TR_STEP(f1, cur, 24576);
        __builtin_amdgcn_sched_barrier(0);
        mfmas_rest(f0);
        __builtin_amdgcn_sched_barrier(0);
        // step 3, behind the barrier
        land(f1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // k-tile kt+1 has landed
        __builtin_amdgcn_s_barrier();                      // ... for every wave, and nobody reads this stage any more
        __builtin_amdgcn_sched_barrier(0);
        mfma1(f1, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        TR_STEP(f0, nxt, 0);  // past the last k-tile this reads stale LDS and is never used
        __builtin_amdgcn_sched_barrier(0);
        issue_a(stage);
        mfmas_rest(f1);
        spread_dma();
        __builtin_amdgcn_sched_barrier(0);
        stage ^= 1;
    }
#undef TR_STEP
#undef TR_RD
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the surplus DMA and reads must not reach the epilogue's staging
    __syncthreads();

    GemmProblem pr{};
    const long long slab = ((long long)blockIdx.z * a.ksplit + range) * a.M * a.N;
    // (c_f16: the partial sums leave as 16-bit rows - bfloat16 in the bf16 step: GemmTnTrDesc::part_bf16)
    pr.C = a.c_f16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(a.part) + slab) : a.part + slab;
    glds_tile_epilogue<MI, WAVES_N>(a, pr, acc, lds, wave, lane, wr, wc, m0, n0);
}

// the ordered reduce of bfloat16 partial sums: C = scales * (sum over the slabs, in index order), four columns per thread
__global__ __launch_bounds__(256) void splitk_reduce_bf16_kernel(const unsigned short* __restrict__ part, int ksplit, long long mn, int N, int ldc,
                                                                 float* c0, float* c1, float* c2, const float* __restrict__ s0,
                                                                 const float* __restrict__ s1) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // quad index within one problem
    if (i * 4 >= mn) return;
    const int z = blockIdx.z;
    const unsigned short* p = part + (long long)z * ksplit * mn + i * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < ksplit; ++k) {
        const uint2 w = *reinterpret_cast<const uint2*>(p + (long long)k * mn);
        acc.x += __builtin_bit_cast(float, w.x << 16); acc.y += __builtin_bit_cast(float, w.x & 0xffff0000u);
        acc.z += __builtin_bit_cast(float, w.y << 16); acc.w += __builtin_bit_cast(float, w.y & 0xffff0000u);
    }
    const float osc = (s0 ? *s0 : 1.f) * (s1 ? *s1 : 1.f);
    float* c = z == 0 ? c0 : (z == 1 ? c1 : c2);
    const long long e = i * 4, m = e / N, n = e - m * N;
    *reinterpret_cast<float4*>(c + m * ldc + n) = make_float4(acc.x * osc, acc.y * osc, acc.z * osc, acc.w * osc);
}


// ---- persistent 256x256 variant ----------------------------------------------------------------------------------
// One block per CU walks tiles blockIdx.x, +gridDim.x, ...  What the one-tile-per-block kernel above loses between
// tiles (measured, M=65536 N=K=1024: loop 70 us per tile, + ~12 us of DMA start-up and block turnover, + 20 us
// epilogue, 30 us with a residual) is removed by treating the k-tiles of ALL the block's tiles as one DMA stream:
//   * while tile t runs its last two k-tiles the DMA already fetches k-tiles 0 and 1 of tile t+1 (the source pointers
//     are switched to the next tile's rows when the stream crosses the boundary), so a tile starts with its
//     fragments in LDS and no pipeline fill;
//   * the epilogue does not touch the stage buffers: each wave transposes its accumulators through a private 4-KiB
//     strip (16 rows x 64 columns) in the 32 KiB of LDS above the stages, eight strips per wave tile, with no block
//     barrier (LDS executes one wave's instructions in order), and its stores drain under the next tile's MFMAs.
// gfx950 counts loads and stores in one in-order vmcnt, so the first k-tile wait of a tile would also wait for the
// store acknowledgements of the epilogue before it; that wait names the number of stores instead (the DMA of k-tile 1
// is older than every one of them).
// Split-K (GldsArgs::ksplit > 1; weight gradients: 16 output tiles, reduction over ~16 K rows): every (tile, k-range) pair is a
// work item of its own, ordered like further problems of the launch, and leaves raw partial sums for gemm.hip's ordered reduce.
// RMODE: 0 = no residual, 1 = f32 residual, 2 = split-f16 residual; CSP: the output is written as split-f16 pairs.  They are
// compile-time so that the epilogue is straight-line code (with run-time flags the residual registers of the fast path
// flow through phi nodes the register allocator keeps - and spills - across the whole tile loop).
// PURE (see above): RMODE 3 = f16 residual, CSP = 2 writes C as plain f16.
// GNT != 0 (with CSP = 1, RMODE = 0, every tile interior): the norm that follows an encoder conv is applied HERE.  A GroupNorm
// instance of conv0-2 is GNT = 16 / 8 / 4 consecutive token rows x 64 channels, and a 16-row epilogue strip of a wave is 16 rows x
// its 64 output columns: whole instances, already in the wave's registers.  Per strip: shifted sums and sums of squares per
// instance, reduced over the wave (DPP + permlane swaps, no LDS), then (v - mean) * rstd * gamma + beta, LeakyReLU, split-f16
// store - the GroupNorm launch and its read of the f32 conv output disappear (norm.hip's register shapes moved 8 bytes per
// element for them).  GNT is a template parameter: the eight unrolled strips carry one variant of the statistics, not three.
// LD != 0 (round 4, plain rows): ONE wave of each SIMD's pair issues the whole DMA stream - LD = 1 the first-dispatched waves 0..3, LD = 2
// waves 4..7 - 16 pieces per k-tile instead of 8 per wave, as buffer loads (32-bit per-lane offsets + scalar row offsets, rows beyond M / N
// come back as zeros from the descriptor's bounds check).  Why: the SIMD arbitrates its two waves oldest-first, so the waves do not interleave
// their MFMAs - the older one runs ahead and parks at the k-tile barrier (45 % of its k-loop time, tools/gemm_trace.py) while the younger one
// finishes alone, with nobody to cover the ~100 cycles each of its DMA issues costs.  With the DMA on one wave of the pair, that wave's issue
// stalls are covered by the partner's MFMAs and the partner's stream has no stalls to cover.
template <bool CONV, int RMODE, int CSP, int PURE = 0, int GNT = 0, int NW = 8, int TRACE = 0, int LD = 0>
__global__ __launch_bounds__(NW * 64) void gemm_nt_split_glds_persist_kernel(const GldsArgs a) {
    static_assert(LD == 0 || (!CONV && NW == 8), "the loader-wave DMA stream is built for plain rows and eight waves");
    // NW = 8: 256x256 tiles, 2 x 4 waves, two waves per SIMD.  NW = 4 (experiment, sola_tune "gemm_nw4"): 256x128 tiles, 2 x 2 waves, one
    // wave per SIMD and up to 512 registers each
    constexpr int MI = 4, WAVES_N = NW / 2, GBM = 256, GBN = WAVES_N * 64, NWAVE = NW;
    constexpr int STAGE_BYTES = (GBM + GBN) * ROWB;
    constexpr int APW = GBM / 8 / NWAVE, WPW = GBN / 8 / NWAVE;
    constexpr int STRIP_ROWS = 16;
    constexpr bool GNF = GNT != 0;  // GNT = rows per GroupNorm instance (4 / 8 / 16), 0 = no norm in the epilogue
    constexpr int RB = 4;  // strips per residual batch (16 registers each)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    // the thread id re-derived where a tile's set-up or epilogue needs it (scalar wave index + lane count): no register holds it across the k-loops
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto fresh_tid = [&](int salt) {  // `salt`: a value of the current tile, so that the lane count is not computed once and kept (spilled)
        int l;
        asm("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l) : "s"(salt));
        return wave_s * 64 + l;
    };
    const int ks_n = a.ksplit > 1 ? a.ksplit : 1;
    const int nk = a.ksplit > 1 ? a.kper : a.K / GBK;

    // Tile order: the problems of a launch (q/k/v projections of the same rows) are the innermost index next to the column
    // tile, so the nprob * tiles_n tiles that read one 256-row block of A run back to back on one XCD and A comes from HBM once.
    // The k ranges of a split-K launch are further "problems" in that order.
    const int tiles_row = a.tiles_n * a.nprob * ks_n;
    const int total = a.tiles_m * tiles_row;
    auto decode = [&](int tile, int& z, int& ks, int& m0, int& n0) {
        int rt, c;
        if (a.xcd_remap && a.order == 1 && (tiles_row & 3) == 0 && (a.tiles_m & 63) == 0) {
            // measurement: an XCD's 32 CUs share 8 row panels x 4 column tiles per round (W tile re-read by 8 CUs instead of 32 / tiles_row)
            const int x = tile & 7, j = tile >> 3;         // j = index within the XCD
            const int g = j >> 5, l = j & 31;              // round group of 32 tiles, slot
            const int cg = tiles_row >> 2;                 // column groups of 4 tiles
            const int rg = g / cg;                         // row-panel group (8 panels) of this XCD
            c = (g - rg * cg) * 4 + (l & 3);
            rt = x + 8 * (rg * 8 + (l >> 2));
        } else if (a.xcd_remap) {
            const int x = tile & 7, j = tile >> 3;
            rt = x + 8 * (j / tiles_row);
            c = j % tiles_row;
        } else {
            rt = tile / tiles_row;
            c = tile % tiles_row;
        }
        const int zz = c / a.tiles_n;
        z = zz / ks_n;
        ks = zz - z * ks_n;
        m0 = rt * GBM;
        n0 = (c - zz * a.tiles_n) * GBN;
    };

    // ---- DMA stream state (same piece layout as the kernel above)
    const int lrow = lane >> 3, chunk = lane & 7;
    const char* a_ptr0;  // piece 0's running source pointer; pieces 1.. are a_ptr0 + a_d[i] (rows of a tile ascend in memory)
    const char* w_ptr0;
    int a_d[APW], w_d[WPW];
    int a_t0[APW];
    int conv_kk = 0, conv_c = 0;
    int dma_kt = 0;  // next k-tile of the DMA stream within its tile
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    auto setup_dma = [&](int tile) {
        int z, ks, m0, n0;
        decode(tile, z, ks, m0, n0);
        const int k0 = ks * nk * GBK;  // first reduction index of this work item
        const float* A = a.p[z].A + k0;
        const float* Wt = a.p[z].W + k0;
        // lane coordinates from an opaque, tile-dependent copy of the thread id: derived once per kernel, everything this set-up computes from
        // them (row offsets, swizzled columns) is hoisted out of the tile loop and kept - spilled - across the k-loops (round 4)
        const int lt = fresh_tid(tile);
        const int wave = lt >> 6, lrow = (lt >> 3) & 7, chunk = lt & 7;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int r = (wave * APW + i) * 8 + lrow;
            const int col_bytes = (chunk ^ ((r >> 1) & 7)) * 16;
            const int m = min(m0 + r, a.M - 1);
            const char* p;
            if (CONV) {
                if (a.rowmap) {
                    const int2 rm = a.rowmap[m];
                    a_t0[i] = rm.y;
                    p = reinterpret_cast<const char*>(A) + (long long)rm.x * a.Cin * 4 + col_bytes;
                } else {
                    const int rr = m / a.T_out, to = m - rr * a.T_out;
                    const int t0 = to * a.stride - a.pad;
                    a_t0[i] = conv_tap_bits(t0, a.T_in);
                    p = reinterpret_cast<const char*>(A) + ((long long)rr * a.T_in + t0) * a.Cin * 4 + col_bytes;
                }
            } else {
                a_t0[i] = 0;
                p = reinterpret_cast<const char*>(A + (long long)m * a.lda) + col_bytes;
            }
            if (i == 0) a_ptr0 = p;
            a_d[i] = (int)(p - a_ptr0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int r = (wave * WPW + i) * 8 + lrow;
            const int n = min(n0 + r, a.N - 1);
            const char* p = reinterpret_cast<const char*>(Wt + (long long)n * a.K) + (chunk ^ ((r >> 1) & 7)) * 16;
            if (i == 0) w_ptr0 = p;
            w_d[i] = (int)(p - w_ptr0);
        }
        conv_kk = CONV ? k0 / a.Cin : 0;
        conv_c = CONV ? k0 - conv_kk * a.Cin : 0;
        dma_kt = 0;
    };
    // piece q of this wave's share of a k-tile: q < APW = A piece q, else W piece q - APW
    auto issue_piece = [&](int stage, int q) {
        char* sbase = lds + stage * STAGE_BYTES;
        if (q < APW) {
            const char* src = a_ptr0 + a_d[q];
            if (CONV) src = ((a_t0[q] >> conv_kk) & 1) ? src : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + (wave * APW + q) * 1024), 16, 0, 0);
        } else {
            __builtin_amdgcn_global_load_lds((gptr_t)(w_ptr0 + w_d[q - APW]), (lptr_t)(sbase + GBM * ROWB + (wave * WPW + q - APW) * 1024), 16, 0, 0);
        }
    };
    auto issue_advance = [&]() {
        // past the last k-tile of the last tile the stream re-reads that k-tile (see the one-tile kernel)
        const bool more = dma_kt + 1 < nk;
        const int adv = more ? GBK * 4 : 0;
        a_ptr0 += adv;
        w_ptr0 += adv;
        if (CONV) {  // branch-free: a branch here would split the basic block the DMA is interleaved in
            conv_c += more ? GBK : 0;
            const bool wrap = conv_c == a.Cin;
            conv_c = wrap ? 0 : conv_c;
            conv_kk += wrap ? 1 : 0;
        }
        ++dma_kt;
    };
    auto issue = [&](int stage) {
#pragma unroll
        for (int q = 0; q < APW + WPW; ++q) issue_piece(stage, q);
        issue_advance();
    };
    // ---- LD: the loader waves' stream.  Loader l (0..3) owns pieces l * 8 .. l * 8 + 7 of the A tile and of the W tile; a piece's source =
    //      descriptor base (the tile's first row) + per-lane offset (row within the piece, swizzled chunk: the key's bit 2 is the piece's
    //      parity, so two offsets per operand) + scalar offset (k position + the piece's first row)
    constexpr int APL = GBM / 8 / 4, WPL = GBN / 8 / 4;
    const bool loader = LD == 0 || (LD == 1 ? wave_s < 4 : wave_s >= 4);
    const int lw = LD == 2 ? wave_s - 4 : wave_s;
    __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(zero), 0, 0, 0x00020000), rs_w = rs_a;
    int a_so = 0, w_so = 0;
    int a_vo[2] = {0, 0}, w_vo[2] = {0, 0};
    const int a_pitch8 = a.lda * 32, w_pitch8 = a.K * 32;  // bytes between pieces (8 rows)
    if constexpr (LD != 0) {
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            const int cb = (chunk ^ (lrow >> 1) ^ (par << 2)) << 4;
            a_vo[par] = lrow * a.lda * 4 + cb;
            w_vo[par] = lrow * a.K * 4 + cb;
        }
    }
    auto setup_dma_ld = [&](int tile) {
        int z, ks, m0, n0;
        decode(tile, z, ks, m0, n0);
        const int k0 = ks * nk * GBK;
        const float* Ab = a.p[z].A + (long long)m0 * a.lda;
        const float* Wb = a.p[z].W + (long long)n0 * a.K;
        rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Ab), 0, min(GBM, a.M - m0) * a.lda * 4, 0x00020000);
        rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wb), 0, min(GBN, a.N - n0) * a.K * 4, 0x00020000);
        a_so = k0 * 4 + lw * APL * a_pitch8;
        w_so = k0 * 4 + lw * WPL * w_pitch8;
        dma_kt = 0;
    };
    auto issue_piece_ld = [&](int stage, int q) {
        char* sbase = lds + stage * STAGE_BYTES;
        if (q < APL) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lptr_t)(sbase + (lw * APL + q) * 1024), 16, a_vo[q & 1], a_so + q * a_pitch8, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lptr_t)(sbase + GBM * ROWB + (lw * WPL + q - APL) * 1024), 16, w_vo[(q - APL) & 1], w_so + (q - APL) * w_pitch8, 0, 0);
    };
    auto issue_advance_ld = [&]() {
        const int adv = dma_kt + 1 < nk ? GBK * 4 : 0;
        a_so += adv;
        w_so += adv;
        ++dma_kt;
    };
    auto issue_ld = [&](int stage) {
#pragma unroll
        for (int q = 0; q < APL + WPL; ++q) issue_piece_ld(stage, q);
        issue_advance_ld();
    };

    const int fr = lane & 31, fh = lane >> 5, key = (lane >> 1) & 7;
    const int a_frag = (wr * MI * 32 + fr) * ROWB, w_frag = GBM * ROWB + (wc * 64 + fr) * ROWB;
    struct Frags { half8 ah[MI], al[MI], bh[2], bl[2]; };
    auto load_frags = [&](const char* sbase, int s16, Frags& f) {
        const int hi_off = (((s16 * 2 + fh) * 2) ^ key) << 4;
        const int lo_off = hi_off ^ 16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* q = sbase + w_frag + j * 32 * ROWB;
            f.bh[j] = *reinterpret_cast<const half8*>(q + hi_off);
            f.bl[j] = *reinterpret_cast<const half8*>(q + lo_off);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const char* p = sbase + a_frag + i * 32 * ROWB;
            f.ah[i] = *reinterpret_cast<const half8*>(p + hi_off);
            f.al[i] = *reinterpret_cast<const half8*>(p + lo_off);
        }
    };
    f32x16 acc[MI][2];
    // The same fragments and products in four GROUPS per half (one A row block each): the next half's fragments are fetched group by
    // group - B and A block 0 behind group 0's first MFMA, A block g behind group g's - so that a half holds at most 72 fragment
    // registers instead of two whole sets (96): the kernel stays inside its 256 registers without scratch (round 4).
    auto load_b = [&](const char* sbase, int s16, Frags& f) {
        const int hi_off = (((s16 * 2 + fh) * 2) ^ key) << 4, lo_off = hi_off ^ 16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* q = sbase + w_frag + j * 32 * ROWB;
            f.bh[j] = *reinterpret_cast<const half8*>(q + hi_off);
            f.bl[j] = *reinterpret_cast<const half8*>(q + lo_off);
        }
    };
    auto load_a = [&](const char* sbase, int s16, Frags& f, int i) {
        const int hi_off = (((s16 * 2 + fh) * 2) ^ key) << 4, lo_off = hi_off ^ 16;
        const char* p = sbase + a_frag + i * 32 * ROWB;
        f.ah[i] = *reinterpret_cast<const half8*>(p + hi_off);
        f.al[i] = *reinterpret_cast<const half8*>(p + lo_off);
    };
    auto for_groups = [&](auto&& fn) {
        static_assert(MI == 4, "four A row blocks per wave tile");
        fn(std::integral_constant<int, 0>{}); fn(std::integral_constant<int, 1>{}); fn(std::integral_constant<int, 2>{}); fn(std::integral_constant<int, 3>{});
    };
    auto mfma_group = [&](const Frags& f, int i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (PURE == 2) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.al[i]), __builtin_bit_cast(bf16x8, f.bl[j]), acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.ah[i]), __builtin_bit_cast(bf16x8, f.bh[j]), acc[i][j], 0, 0, 0);
            } else if constexpr (PURE == 1) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
            } else {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
            }
        }
    };

    int tile = blockIdx.x;
    if (tile >= total) return;
    if (a.stagger > 0) {  // measurement: four start phases, neighbouring CUs of an XCD in different ones
        const int ph = (blockIdx.x >> 3) & 3;
        for (int q = 0; q < ph * a.stagger; ++q) __builtin_amdgcn_s_sleep(1);  // 64 clocks each
    }
    if constexpr (PURE == 2)  // bf16 instantiations only (the training step's): the conv instantiations of the other modes have no register left for it
    if (a.stagger < 0) {
        const int slack = -a.stagger;
        const int grid = (int)gridDim.x, first = total % grid;  // blocks first.. have one tile fewer (first == 0: whole rounds, nobody has slack)
        if (first != 0 && (int)blockIdx.x >= first) {
            const int nsl = grid - first, idx = (int)blockIdx.x - first;
            const int n = (int)((long long)idx * slack * nk * 7 / (8LL * nsl));  // phases 0 .. 7/8 of a tile's time
            for (int q = 0; q < n; ++q) __builtin_amdgcn_s_sleep(1);
        }
    }
    // TRACE: cycles this wave spent at the k-tile wait + barrier, in the k-loops and in the epilogues; per tile the real-time stamps
    // (100 MHz, low 32 bits) of the end of its k-loop and of its epilogue, lane t of two registers = tile t of this block
    unsigned long long tr_wait = 0, tr_loop = 0, tr_epi = 0, tr_t0 = 0, tr_t1 = 0, tr_first = 0;
    int tr_kend = 0, tr_eend = 0, tr_n = 0;
    if constexpr (TRACE) tr_first = wall_clock64();
    bool prev_fast = false;  // the previous tile of this block left through the interior epilogue
    if constexpr (LD == 0) {
        setup_dma(tile);
        issue(0);
        issue(1);  // nk >= 2 (checked by the launcher)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APW + WPW) : "memory");  // k-tile 0 is the older half of what is in flight
    } else if (loader) {
        setup_dma_ld(tile);
        issue_ld(0);
        issue_ld(1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APL + WPL) : "memory");
    }
    __syncthreads();
    int stage = 0;
    constexpr int NMF = (PURE ? 4 : 6) * MI;
    constexpr int NDMA = APW + WPW;
    constexpr int NDMA_L = APL + WPL, DMA_GAP_L = NDMA_L > 0 ? (NMF - 1) / NDMA_L : 1;  // loader waves: one piece behind every MFMA of the second half
    static_assert(LD == 0 || DMA_GAP_L >= 1, "the loader's pieces must fit behind the second half's MFMAs");
    for (; tile < total; tile += gridDim.x) {
        int z, ks, m0, n0;
        decode(tile, z, ks, m0, n0);
        const int next = tile + gridDim.x;
        const bool has_next = next < total;
        unsigned long long tr_ls = 0;
        if constexpr (TRACE) tr_ls = clock64();
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // k-tile 0 of this tile is in LDS (waited for and published by the barrier of the previous tile's last k-tile, or by
        // the prologue).  Its first fragments are fetched here rather than kept in registers across the epilogue.
        Frags f0, f1;
        // One k-tile.  The k-loop itself must stay free of conditions: a scalar branch in front of the barrier (the relaxed
        // wait below) or behind it (switching the DMA stream to the next tile) cost 10 % and 2 % of the loop (measured,
        // one tile per CU), so the first k-tile is peeled for the wait and the last two for the stream switch.
        auto ktile = [&](auto first, auto rolec) {
            constexpr int ROLE = decltype(rolec)::value;  // 0: every wave loads its share (LD = 0); 1: loader wave; 2: its partner (no DMA)
            constexpr int MPG = NMF / MI;                  // MFMAs of one group (one A row block): 6 split, 4 plain 16-bit
            constexpr int NP = ROLE == 0 ? NDMA : (ROLE == 1 ? NDMA_L : 0), PPG = NP / MI;  // DMA pieces of this wave per k-tile / per group
            constexpr int GAP = (MPG - 1) / (PPG > 0 ? PPG : 1) * (PPG > 0 ? 1 : 0);          // MFMAs in front of each of a group's pieces (0: no pieces)
            static_assert(NP % MI == 0 && (PPG == 0 || GAP >= 1), "a group's DMA pieces must fit between its MFMAs");
            if constexpr (TRACE) tr_wait += tr_t1 - tr_t0;  // the previous k-tile's wait (both stamps have long returned)
            // ---- first half: products of k 0..15 (f0); the fragments of k 16..31 of the same stage arrive group by group
            {
                const char* sb = lds + stage * STAGE_BYTES;
                for_groups([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    if (g == 0) load_b(sb, 1, f1);
                    load_a(sb, 1, f1, g);
                    mfma_group(f0, g);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, g == 0 ? 6 : 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, MPG - 1, 0);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
            if constexpr (TRACE) tr_t0 = clock64();
            // k-tile kt+1 has landed.  At kt == 0 behind an interior tile's epilogue that is k-tile 1, issued BEFORE the
            // epilogue's stores: naming the store count (32 float4 or 64 half4 stores per wave; the counter is in order)
            // waits for the DMA without waiting for the stores to be acknowledged.
            if constexpr (ROLE != 2) {  // the partner of a loader wave has no DMA in flight: its stores need no wait
                if (decltype(first)::value && prev_fast) {
                    if (CSP == 1) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            __syncthreads();
            if constexpr (TRACE) tr_t1 = clock64();
            __builtin_amdgcn_sched_barrier(0);
            // ---- second half: products of k 16..31 (f1); the next k-tile's first fragments (the other stage) arrive group by group and
            //      the DMA pieces of k-tile kt+2 go into the stage every wave has just left, spread over the MFMAs (issued back to back they
            //      queue in the CU's one texture-address path and a wave stuck at a full memory queue issues no MFMAs: tools/micro/lds_dma.hip)
            {
                const char* sb = lds + (stage ^ 1) * STAGE_BYTES;  // after the last k-tile: read, never used
                for_groups([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    if (g == 0) load_b(sb, 0, f0);
                    load_a(sb, 0, f0, g);
#pragma unroll
                    for (int q = 0; q < PPG; ++q) {
                        if constexpr (ROLE == 0) issue_piece(stage, g * PPG + q);
                        if constexpr (ROLE == 1) issue_piece_ld(stage, g * PPG + q);
                    }
                    if (g == MI - 1) {
                        if constexpr (ROLE == 0) issue_advance();
                        if constexpr (ROLE == 1) issue_advance_ld();
                    }
                    mfma_group(f1, g);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, g == 0 ? 6 : 2, 0);
#pragma unroll
                    for (int q = 0; q < PPG; ++q) {
                        __builtin_amdgcn_sched_group_barrier(0x008, GAP, 0);
                        __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, MPG - 1 - PPG * GAP, 0);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
            stage ^= 1;
        };
        // k-tile kt issues the DMA of k-tile kt+2; from kt = nk-2 on that is the next tile's stream
        auto kloop = [&](auto rolec) {
            constexpr int ROLE = decltype(rolec)::value;
            auto switch_stream = [&]() {
                if constexpr (ROLE == 0) setup_dma(next);
                if constexpr (ROLE == 1) setup_dma_ld(next);
            };
            // k-tile 0 of this tile is in LDS (see above).  Its first fragments are fetched here, inside the role's own loop: fetched in front of
            // the role branch they stayed live - spilled - across the other role's code (LD != 0)
            load_frags(lds + stage * STAGE_BYTES, 0, f0);
            int kt = 1;
            if (nk == 2 && has_next) switch_stream();
            ktile(std::true_type{}, rolec);
            for (; kt < nk - 2; ++kt) ktile(std::false_type{}, rolec);
            if (nk > 2 && has_next) switch_stream();
            for (; kt < nk; ++kt) ktile(std::false_type{}, rolec);
        };
        if constexpr (LD == 0) kloop(std::integral_constant<int, 0>{});
        else if (loader) kloop(std::integral_constant<int, 1>{});
        else kloop(std::integral_constant<int, 2>{});
        unsigned long long tr_es = 0;
        if constexpr (TRACE) {
            tr_wait += tr_t1 - tr_t0;
            tr_t0 = tr_t1 = 0;
            tr_es = clock64();
            tr_loop += tr_es - tr_ls;
            tr_kend = lane == (tr_n & 63) ? (int)wall_clock64() : tr_kend;
        }
        auto trace_tile_end = [&]() {
            if constexpr (TRACE) {
                tr_epi += clock64() - tr_es;
                tr_eend = lane == (tr_n & 63) ? (int)wall_clock64() : tr_eend;
                ++tr_n;
            }
        };
        if (a.ablate & 4) {
            prev_fast = false;  // no stores went out: the next tile's first wait must be the full one
            trace_tile_end();
            continue;
        }

        // ---- epilogue: eight 16-row strips per wave tile through this wave's private LDS strip
        GemmProblem pr = a.p[z];
        float osc = (a.out_scale_dev ? a.out_scale * *a.out_scale_dev : a.out_scale) * (pr.scale_dev ? *pr.scale_dev : 1.f);
        int ldc = a.ldc;
        if (a.ksplit > 1) {  // raw partial sums; scale, bias, residual and the output format are the reduce pass's
            pr.C = a.part + (long long)(z * a.ksplit + ks) * a.M * a.N;
            pr.bias = nullptr;
            ldc = a.N;
            osc = 1.f;
        }
        // Everything the epilogue derives from the lane id goes through an opaque copy made here: otherwise the row
        // offsets of all 32 passes (64-bit, tile-invariant) are hoisted out of the tile loop and live - spilled - across
        // the k-loop.
        int le = fresh_tid(tile);
        asm volatile("" : "+v"(le));
        const int lane_e = le & 63, wave_e = le >> 6;
        const int fh_e = lane_e >> 5;
        float* strip = reinterpret_cast<float*>(lds + 2 * STAGE_BYTES) + wave_e * (STRIP_ROWS * 64);
        const int col_l = lane_e & 31;
        const int c4 = lane_e & 15, rsub = lane_e >> 4;
        const int wr_e = wave_e / WAVES_N, wc_e = wave_e % WAVES_N;
        const int n = n0 + wc_e * 64 + c4 * 4;
        const bool vec_ok = (ldc & 3) == 0 && n + 3 < a.N && (RMODE != 1 || (a.ldr & 3) == 0);
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pr.bias) {
            const float bsc = a.bias_scale_dev ? *a.bias_scale_dev : 1.f;
            bv.x = n < a.N ? pr.bias[n] * bsc : 0.f;
            bv.y = n + 1 < a.N ? pr.bias[n + 1] * bsc : 0.f;
            bv.z = n + 2 < a.N ? pr.bias[n + 2] * bsc : 0.f;
            bv.w = n + 3 < a.N ? pr.bias[n + 3] * bsc : 0.f;
        }
        float4 gnw = make_float4(1.f, 1.f, 1.f, 1.f), gnb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (GNF) {
            gnw = *reinterpret_cast<const float4*>(a.gn_gamma + n);
            gnb = *reinterpret_cast<const float4*>(a.gn_beta + n);
        }
        // Interior tiles (every row and column in range, 16-byte aligned rows) take a straight-line path: no per-lane
        // predicates, so the number of stores a wave issues is known (see the relaxed wait at the next tile's first
        // k-tile), and the residual is fetched four strips ahead (64 registers; the fragment registers are dead here).
        // vmcnt is one in-order counter for loads and stores: a residual load issued between stores would have to wait for
        // the acknowledgement of every store before it, so the loads of a batch are issued together, in front of its stores.
        const bool interior = m0 + GBM <= a.M && n0 + GBN <= a.N && (ldc & 3) == 0 && (RMODE != 1 || (a.ldr & 3) == 0);
        prev_fast = interior && !(a.ablate & 24);
        if (interior) {
            // Range guard of the split / f16 outputs: one flag per lane for the whole tile, checked once behind the last strip.  A
            // check per store (an exec-masked region in front of every pass) cost 32 branches per tile, and the packed-f32
            // subtract that followed the exec restore lost its low half in lanes 48..63 about five times per 65536 strips
            // (measured on the fused-norm epilogue: the element left the epilogue uncentred).
            unsigned long long out_of_range = 0;  // lane mask, kept in scalar registers
            auto note_range = [&](const float (&v)[4]) {
                const float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));  // drops NaNs
                out_of_range |= __builtin_amdgcn_ballot_w64(!(m < 65000.f) || __builtin_isunordered(v[0], v[1]) || __builtin_isunordered(v[2], v[3]));
            };
#pragma unroll
            for (int b = 0; b < 8 / RB; ++b) {
                f32x4 rbuf[RB * 4];
                if (RMODE) {
#pragma unroll
                    for (int sp = 0; sp < RB * 4; ++sp) {
                        const int st = b * RB + (sp >> 2), pass = sp & 3;  // strip 0..7 = (i, hf)
                        const int m = m0 + wr_e * 128 + (st >> 1) * 32 + (st & 1) * 16 + pass * 4 + rsub;
                        if (RMODE == 3) {  // four halfs = 8 bytes
                            const float2 h = *reinterpret_cast<const float2*>(reinterpret_cast<const _Float16*>(pr.R) + (long long)m * a.ldr + n);
                            rbuf[sp] = f32x4{h.x, h.y, 0.f, 0.f};
                        } else if (RMODE == 2) {
                            const char* rb = reinterpret_cast<const char*>(pr.R + (long long)m * a.ldr + (n & ~7)) + (n & 4) * 2;
                            const float2 h = *reinterpret_cast<const float2*>(rb), l = *reinterpret_cast<const float2*>(rb + 16);
                            rbuf[sp] = f32x4{h.x, h.y, l.x, l.y};
                        } else {
                            rbuf[sp] = *reinterpret_cast<const f32x4*>(pr.R + (long long)m * a.ldr + n);
                        }
                    }
                }
#pragma unroll
                for (int sl = 0; sl < RB; ++sl) {
                    const int st = b * RB + sl, i = st >> 1, hf = st & 1;
                    if (!(a.ablate & 16))
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int row = (q & 3) + 8 * (q >> 2) + 4 * fh_e;
                            const int col = (j * 32 + col_l) ^ (fh_e << 5);
                            strip[row * 64 + col] = acc[i][j][hf * 8 + q];
                        }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if constexpr (GNF) {
                        // instances of GNT rows: NI per strip, PPI passes each.  One pass over the values: sums of (v - k) and
                        // (v - k)^2 with k = a value of the instance itself (lane 0's first element: mean - k is a few standard
                        // deviations at most, so s2 / n - (s1 / n)^2 loses a digit, not the result), two INDEPENDENT wave
                        // reductions per instance - the two-pass form was one dependent chain of reduce, divide, reduce, sqrt,
                        // divide per strip with two waves per SIMD to hide it.
                        constexpr int NI = 16 / GNT, PPI = 4 / NI;
                        float d[4][4], s1[NI], s2[NI], mu[NI], rs[NI];
#pragma unroll
                        for (int u = 0; u < NI; ++u) s1[u] = s2[u] = 0.f;
                        float kk = 0.f;
#pragma unroll
                        for (int pass = 0; pass < 4; ++pass) {
                            const int row = pass * 4 + rsub, u = pass / PPI;
                            const float4 t = *reinterpret_cast<const float4*>(&strip[row * 64 + ((c4 ^ ((pass & 1) << 3)) << 2)]);
                            const float v0 = t.x * osc + bv.x, v1 = t.y * osc + bv.y, v2 = t.z * osc + bv.z, v3 = t.w * osc + bv.w;
                            if (pass % PPI == 0) kk = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v0)));
                            d[pass][0] = v0 - kk; d[pass][1] = v1 - kk; d[pass][2] = v2 - kk; d[pass][3] = v3 - kk;
                            s1[u] += (d[pass][0] + d[pass][1]) + (d[pass][2] + d[pass][3]);
                            s2[u] += (d[pass][0] * d[pass][0] + d[pass][1] * d[pass][1]) + (d[pass][2] * d[pass][2] + d[pass][3] * d[pass][3]);
                        }
#pragma unroll
                        for (int u = 0; u < NI; ++u) {
                            const float m1 = wave_sum_dpp(s1[u]) * a.gn_icnt, m2 = wave_sum_dpp(s2[u]) * a.gn_icnt;  // 1 / (GNT * 64): a power of two
                            mu[u] = m1;
                            rs[u] = __builtin_amdgcn_rsqf(fmaxf(m2 - m1 * m1, 0.f) + a.gn_eps);
                        }
                        const float gw[4] = {gnw.x, gnw.y, gnw.z, gnw.w}, gb[4] = {gnb.x, gnb.y, gnb.z, gnb.w};
#pragma unroll
                        for (int pass = 0; pass < 4; ++pass) {
                            const int row = pass * 4 + rsub;
                            const int m = m0 + wr_e * 128 + i * 32 + hf * 16 + row;
                            float v[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float y = (d[pass][e] - mu[pass / PPI]) * rs[pass / PPI] * gw[e] + gb[e];
                                v[e] = y >= 0.f ? y : y * a.gn_slope;
                            }
                            _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * ldc + (n & ~7)) + (n & 4);
                            half4 hh, ll;
#pragma unroll
                            for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                            *reinterpret_cast<half4*>(cb) = hh;
                            *reinterpret_cast<half4*>(cb + 8) = ll;
                            note_range(v);
                        }
                    } else
#pragma unroll
                    for (int pass = 0; pass < 4; ++pass) {
                        const int row = pass * 4 + rsub;
                        const int m = m0 + wr_e * 128 + i * 32 + hf * 16 + row;
                        float4 t;
                        if (a.ablate & 16) t = make_float4(acc[i][0][hf * 8 + pass], acc[i][0][hf * 8 + 4 + pass], acc[i][1][hf * 8 + pass], acc[i][1][hf * 8 + 4 + pass]);
                        else t = *reinterpret_cast<const float4*>(&strip[row * 64 + ((c4 ^ ((pass & 1) << 3)) << 2)]);
                        float v[4] = {t.x * osc + bv.x, t.y * osc + bv.y, t.z * osc + bv.z, t.w * osc + bv.w};
                        if (RMODE) {
                            const f32x4 rv = rbuf[sl * 4 + pass];
                            if (RMODE == 3) {
                                const half4 hh = __builtin_bit_cast(half4, float2{rv[0], rv[1]});
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] += cvt16_in(hh[e], PURE == 2);
                            } else if (RMODE == 2) {
                                const half4 hh = __builtin_bit_cast(half4, float2{rv[0], rv[1]}), ll = __builtin_bit_cast(half4, float2{rv[2], rv[3]});
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] += (float)hh[e] + (float)ll[e];
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] += rv[e];
                            }
                        }
                        if (CSP == 2) {
                            const half4 hh = cvt16x4_out(v, PURE == 2);
                            if (a.ablate & 8) asm volatile("" ::"v"(hh)); else
                            *reinterpret_cast<half4*>(reinterpret_cast<_Float16*>(pr.C) + (long long)m * ldc + n) = hh;
                            if (PURE != 2) note_range(v);
                        } else if (CSP == 1) {
                            _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * ldc + (n & ~7)) + (n & 4);
                            half4 hh, ll;
#pragma unroll
                            for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                            if (a.ablate & 8) asm volatile("" ::"v"(hh), "v"(ll)); else {
                            *reinterpret_cast<half4*>(cb) = hh;
                            *reinterpret_cast<half4*>(cb + 8) = ll; }
                            note_range(v);
                        } else {
                            if (a.ablate & 8) asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3])); else
                            *reinterpret_cast<float4*>(pr.C + (long long)m * ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if (CSP != 0 && a.guard && out_of_range != 0 && lane_e == 0) atomicOr(a.guard, 1);
            trace_tile_end();
            continue;
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                // rows of a 32x32 accumulator block held by this lane: (r & 3) + 8 * (r >> 2) + 4 * fh_e; r = hf*8 .. hf*8+7
                // are strip rows (q & 3) + 8 * (q >> 2) + 4 * fh.  Bit 2 of the strip row (= fh) flips the column's bit 5
                // so the two half waves write different banks.
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int row = (q & 3) + 8 * (q >> 2) + 4 * fh_e;
                        const int col = (j * 32 + col_l) ^ (fh_e << 5);
                        strip[row * 64 + col] = acc[i][j][hf * 8 + q];
                    }
                asm volatile("" ::: "memory");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int row = pass * 4 + rsub;
                    const int m = m0 + wr_e * 128 + i * 32 + hf * 16 + row;
                    const float4 t = *reinterpret_cast<const float4*>(&strip[row * 64 + ((c4 ^ ((pass & 1) << 3)) << 2)]);
                    if (m >= a.M) continue;
                    float v[4] = {t.x * osc + bv.x, t.y * osc + bv.y, t.z * osc + bv.z, t.w * osc + bv.w};
                    if (RMODE) {
                        if (RMODE == 3) {
                            const _Float16* rb = reinterpret_cast<const _Float16*>(pr.R) + (long long)m * a.ldr + n;
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (n + e < a.N) v[e] += cvt16_in(rb[e], PURE == 2);
                        } else if (RMODE == 2) {
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
                    if (CSP == 2) {
                        if (n >= a.N) continue;  // N % 4 == 0: the four columns are in range together
                        *reinterpret_cast<half4*>(reinterpret_cast<_Float16*>(pr.C) + (long long)m * ldc + n) = cvt16x4_out(v, PURE == 2);
                        if (PURE != 2) guard_sp16x4(a.guard, v);
                    } else if (CSP == 1) {
                        if (n >= a.N) continue;  // N % 8 == 0 and n % 4 == 0: the four columns are in range together
                        _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * ldc + (n & ~7)) + (n & 4);
                        half4 hh, ll;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                        *reinterpret_cast<half4*>(cb) = hh;
                        *reinterpret_cast<half4*>(cb + 8) = ll;
                        guard_sp16x4(a.guard, v);
                    } else if (vec_ok) {
                        *reinterpret_cast<float4*>(pr.C + (long long)m * ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < a.N) pr.C[(long long)m * ldc + n + e] = v[e];
                    }
                }
                asm volatile("" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
        }
        trace_tile_end();
    }
    if constexpr (TRACE) {
        if (a.trace) {
            unsigned long long* rec = a.trace + ((long long)blockIdx.x * NWAVE + wave) * gemm_trace_words;
            if (lane == 0) {
                rec[0] = tr_wait; rec[1] = tr_loop; rec[2] = tr_epi; rec[3] = (unsigned long long)tr_n;
                rec[4] = tr_first; rec[5] = wall_clock64(); rec[6] = (unsigned long long)nk; rec[7] = 0;
            }
            rec[8 + lane] = (unsigned)tr_kend;
            rec[8 + 64 + lane] = (unsigned)tr_eend;
        }
    }
}

}  // namespace

bool gemm_split_glds_supported(const GemmDesc& d) {
    if (d.arith == 2) {  // plain f16 rows: sizes in halfs, two per 4-byte unit
        if (d.K % (2 * GBK) != 0 || d.conv == 2) return false;
        return d.conv == 1 ? d.Cin % (2 * GBK) == 0 : d.lda % 16 == 0;
    }
    if (d.arith != 1 || d.K % GBK != 0 || d.conv == 2) return false;
    if (d.conv == 1) return d.Cin % GBK == 0;
    return d.lda % 8 == 0;
}

// Ping-pong variant (sola_tune "gemm_pp"; plain launches without residual whose tiles are all interior and K >= 352): 256x128
// tiles, four waves = ONE per SIMD with up to 512 registers, TWO accumulator sets.  The epilogue of a tile does not run behind
// its k-loop: its eight strips are drained one per k-tile under the first eight k-tiles of the block's NEXT tile (LDS transpose
// and conversion between that k-tile's MFMAs, the strip's stores behind the k-tile's last DMA piece, so the next k-tile's wait
// names them - vmcnt(stores per strip) - instead of waiting for their acknowledgement).  Same fragments, same accumulation
// order and the same epilogue arithmetic as the kernel above: results are bit-identical.
template <bool CONV, int CSP>
__global__ __launch_bounds__(256) void gemm_nt_split_glds_pp_kernel(const GldsArgs a) {
    constexpr int NW = 4;
    constexpr bool PURE = false;
    constexpr int MI = 4, WAVES_N = NW / 2, GBM = 256, GBN = WAVES_N * 64, NWAVE = NW;
    constexpr int STAGE_BYTES = (GBM + GBN) * ROWB;
    constexpr int APW = GBM / 8 / NWAVE, WPW = GBN / 8 / NWAVE;
    constexpr int STRIP_ROWS = 16;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int ks_n = a.ksplit > 1 ? a.ksplit : 1;
    const int nk = a.ksplit > 1 ? a.kper : a.K / GBK;

    // Tile order: the problems of a launch (q/k/v projections of the same rows) are the innermost index next to the column
    // tile, so the nprob * tiles_n tiles that read one 256-row block of A run back to back on one XCD and A comes from HBM once.
    // The k ranges of a split-K launch are further "problems" in that order.
    const int tiles_row = a.tiles_n * a.nprob * ks_n;
    const int total = a.tiles_m * tiles_row;
    auto decode = [&](int tile, int& z, int& ks, int& m0, int& n0) {
        int rt, c;
        if (a.xcd_remap) {
            const int x = tile & 7, j = tile >> 3;
            rt = x + 8 * (j / tiles_row);
            c = j % tiles_row;
        } else {
            rt = tile / tiles_row;
            c = tile % tiles_row;
        }
        const int zz = c / a.tiles_n;
        z = zz / ks_n;
        ks = zz - z * ks_n;
        m0 = rt * GBM;
        n0 = (c - zz * a.tiles_n) * GBN;
    };

    // ---- DMA stream state (same piece layout as the kernel above)
    const int lrow = lane >> 3, chunk = lane & 7;
    const char* a_ptr0;  // piece 0's running source pointer; pieces 1.. are a_ptr0 + a_d[i] (rows of a tile ascend in memory)
    const char* w_ptr0;
    int a_d[APW], w_d[WPW];
    int a_t0[APW];
    int conv_kk = 0, conv_c = 0;
    int dma_kt = 0;  // next k-tile of the DMA stream within its tile
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    auto setup_dma = [&](int tile) {
        int z, ks, m0, n0;
        decode(tile, z, ks, m0, n0);
        const int k0 = ks * nk * GBK;  // first reduction index of this work item
        const float* A = a.p[z].A + k0;
        const float* Wt = a.p[z].W + k0;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int r = (wave * APW + i) * 8 + lrow;
            const int col_bytes = (chunk ^ ((r >> 1) & 7)) * 16;
            const int m = min(m0 + r, a.M - 1);
            const char* p;
            if (CONV) {
                if (a.rowmap) {
                    const int2 rm = a.rowmap[m];
                    a_t0[i] = rm.y;
                    p = reinterpret_cast<const char*>(A) + (long long)rm.x * a.Cin * 4 + col_bytes;
                } else {
                    const int rr = m / a.T_out, to = m - rr * a.T_out;
                    const int t0 = to * a.stride - a.pad;
                    a_t0[i] = conv_tap_bits(t0, a.T_in);
                    p = reinterpret_cast<const char*>(A) + ((long long)rr * a.T_in + t0) * a.Cin * 4 + col_bytes;
                }
            } else {
                a_t0[i] = 0;
                p = reinterpret_cast<const char*>(A + (long long)m * a.lda) + col_bytes;
            }
            if (i == 0) a_ptr0 = p;
            a_d[i] = (int)(p - a_ptr0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            const int r = (wave * WPW + i) * 8 + lrow;
            const int n = min(n0 + r, a.N - 1);
            const char* p = reinterpret_cast<const char*>(Wt + (long long)n * a.K) + (chunk ^ ((r >> 1) & 7)) * 16;
            if (i == 0) w_ptr0 = p;
            w_d[i] = (int)(p - w_ptr0);
        }
        conv_kk = CONV ? k0 / a.Cin : 0;
        conv_c = CONV ? k0 - conv_kk * a.Cin : 0;
        dma_kt = 0;
    };
    auto issue = [&](int stage) {
        char* sbase = lds + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const char* src = a_ptr0 + a_d[i];
            if (CONV) src = ((a_t0[i] >> conv_kk) & 1) ? src : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + (wave * APW + i) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WPW; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)(w_ptr0 + w_d[i]), (lptr_t)(sbase + GBM * ROWB + (wave * WPW + i) * 1024), 16, 0, 0);
        }
        // past the last k-tile of the last tile the stream re-reads that k-tile (see the one-tile kernel)
        const bool more = dma_kt + 1 < nk;
        const int adv = more ? GBK * 4 : 0;
        a_ptr0 += adv;
        w_ptr0 += adv;
        if (CONV) {  // branch-free: a branch here would split the basic block the DMA is interleaved in
            conv_c += more ? GBK : 0;
            const bool wrap = conv_c == a.Cin;
            conv_c = wrap ? 0 : conv_c;
            conv_kk += wrap ? 1 : 0;
        }
        ++dma_kt;
    };

    const int fr = lane & 31, fh = lane >> 5, key = (lane >> 1) & 7;
    const int a_frag = (wr * MI * 32 + fr) * ROWB, w_frag = GBM * ROWB + (wc * 64 + fr) * ROWB;
    struct Frags { half8 ah[MI], al[MI], bh[2], bl[2]; };
    auto load_frags = [&](const char* sbase, int s16, Frags& f) {
        const int hi_off = (((s16 * 2 + fh) * 2) ^ key) << 4;
        const int lo_off = hi_off ^ 16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* q = sbase + w_frag + j * 32 * ROWB;
            f.bh[j] = *reinterpret_cast<const half8*>(q + hi_off);
            f.bl[j] = *reinterpret_cast<const half8*>(q + lo_off);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const char* p = sbase + a_frag + i * 32 * ROWB;
            f.ah[i] = *reinterpret_cast<const half8*>(p + hi_off);
            f.al[i] = *reinterpret_cast<const half8*>(p + lo_off);
        }
    };
    f32x16 acc[2][MI][2];  // accumulator sets of the tile in flight and of the tile being drained
    auto mfmas = [&](auto pc, const Frags& f) {
        constexpr int P = decltype(pc)::value;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (PURE) {
                    acc[P][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bl[j], acc[P][i][j], 0, 0, 0);
                    acc[P][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[P][i][j], 0, 0, 0);
                } else {
                    acc[P][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[j], acc[P][i][j], 0, 0, 0);
                    acc[P][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[j], acc[P][i][j], 0, 0, 0);
                    acc[P][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[j], acc[P][i][j], 0, 0, 0);
                }
            }
    };


    int tile = blockIdx.x;
    if (tile >= total) return;
    setup_dma(tile);
    issue(0);
    issue(1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APW + WPW) : "memory");
    __syncthreads();
    int stage = 0;
    constexpr int NRD = 2 * MI + 4, NMF = 6 * MI;
    constexpr int NDMA = APW + WPW, DMA_GAP = (NMF - 1) / NDMA;
    constexpr int NST = CSP == 1 ? 8 : 4;  // global stores per strip and wave

    // Lane coordinates of the epilogue are re-derived from an opaque copy of the thread id inside every strip: derived once, the
    // compiler hoists the addresses of all eight strips out of the tile loop and keeps them - spilled - across the k-loops.
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: costs no vector register across the k-loops
#define PP_LANE_COORDS                                                                                   \
    int le = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));                    \
    asm volatile("" : "+v"(le));                                                                         \
    const int lane_e = le, wave_e = wave_s;                                                              \
    const int fh_e = lane_e >> 5;                                                                        \
    float* strip = reinterpret_cast<float*>(lds + 2 * STAGE_BYTES) + wave_e * (STRIP_ROWS * 64);         \
    const int col_l = lane_e & 31;                                                                       \
    const int c4 = lane_e & 15, rsub = lane_e >> 4;                                                      \
    const int wr_e = wave_e / WAVES_N, wc_e = wave_e % WAVES_N;                                          \
    (void)fh_e; (void)strip; (void)col_l; (void)c4; (void)rsub; (void)wr_e; (void)wc_e;

    // the tile whose accumulators wait to be drained
    float* pend_C = nullptr;
    float pend_osc = 1.f;
    float4 pend_bv = make_float4(0.f, 0.f, 0.f, 0.f);
    int pend_m0 = 0, pend_n = 0;
    unsigned long long out_of_range = 0;

    // one strip (16 rows x this wave's 64 columns) of accumulator set Q: LDS transpose + conversion (part 1), stores (part 2)
    f32x4 sv[4];
    auto strip_compute = [&](auto qc, auto stc) {
        constexpr int Q = decltype(qc)::value, st = decltype(stc)::value, i = st >> 1, hf = st & 1;
        PP_LANE_COORDS
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int row = (q & 3) + 8 * (q >> 2) + 4 * fh_e;
                const int col = (j * 32 + col_l) ^ (fh_e << 5);
                strip[row * 64 + col] = acc[Q][i][j][hf * 8 + q];
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the strip is written (in-order LDS queue; wave-private region)
        __builtin_amdgcn_wave_barrier();
        // The four reads go through inline asm with their own lgkmcnt wait: in front of a compiler-visible LDS read the waitcnt pass
        // puts vmcnt(0) here (LDS-DMA pieces and the previous strip's stores are in flight) - exactly the wait this kernel avoids.
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int row = pass * 4 + rsub;
            const unsigned addr = (unsigned)(uintptr_t)(lptr_t)&strip[row * 64 + ((c4 ^ ((pass & 1) << 3)) << 2)];
            asm volatile("ds_read_b128 %0, %1" : "=v"(sv[pass]) : "v"(addr) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3])::"memory");
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            sv[pass][0] = sv[pass][0] * pend_osc + pend_bv.x; sv[pass][1] = sv[pass][1] * pend_osc + pend_bv.y;
            sv[pass][2] = sv[pass][2] * pend_osc + pend_bv.z; sv[pass][3] = sv[pass][3] * pend_osc + pend_bv.w;
        }
        __builtin_amdgcn_wave_barrier();
    };
    auto strip_store = [&](auto stc) {
        constexpr int st = decltype(stc)::value, i = st >> 1, hf = st & 1;
        PP_LANE_COORDS
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int m = pend_m0 + wr_e * 128 + i * 32 + hf * 16 + pass * 4 + rsub;
            if (CSP == 1) {
                _Float16* cb = reinterpret_cast<_Float16*>(pend_C + (long long)m * a.ldc + (pend_n & ~7)) + (pend_n & 4);
                half4 hh, ll;
#pragma unroll
                for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(sv[pass][e], h1, l1); hh[e] = h1; ll[e] = l1; }
                *reinterpret_cast<half4*>(cb) = hh;
                *reinterpret_cast<half4*>(cb + 8) = ll;
                const float mx = fmaxf(fmaxf(fabsf(sv[pass][0]), fabsf(sv[pass][1])), fmaxf(fabsf(sv[pass][2]), fabsf(sv[pass][3])));
                out_of_range |= __builtin_amdgcn_ballot_w64(!(mx < 65000.f) || __builtin_isunordered(sv[pass][0], sv[pass][1]) || __builtin_isunordered(sv[pass][2], sv[pass][3]));
            } else {
                *reinterpret_cast<float4*>(pend_C + (long long)m * a.ldc + pend_n) = make_float4(sv[pass][0], sv[pass][1], sv[pass][2], sv[pass][3]);
            }
        }
    };
    auto flush_guard = [&]() {
        if (CSP == 1 && a.guard && out_of_range != 0 && (tid & 63) == 0) atomicOr(a.guard, 1);
        out_of_range = 0;
    };

    Frags f0, f1;
    // one k-tile of the tile accumulating into set P; ST >= 0: strip ST of set P ^ 1 is drained under it; RELAX: the previous
    // k-tile ended with NST stores, which the wait for this k-tile's DMA may leave in flight
    auto ktile = [&](auto pc, auto stc, auto relaxc) {
        constexpr int P = decltype(pc)::value, ST = decltype(stc)::value;  // ST = 0..8: stores of strip ST - 1, transpose of strip ST
        constexpr bool STORES = ST >= 1 && ST <= 8, COMPUTE = ST >= 0 && ST <= 7;
        load_frags(lds + stage * STAGE_BYTES, 1, f1);
        mfmas(pc, f0);
        if constexpr (STORES) strip_store(std::integral_constant<int, STORES ? ST - 1 : 0>{});
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
        if constexpr (STORES) {  // the previous strip's stores, one per two MFMAs (a wave stuck at a full memory queue issues no MFMAs)
#pragma unroll
            for (int g = 0; g < NST; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - 2 * NST, 0);
        } else {
            __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // this strip's transpose through LDS behind the half's last MFMA issue (it runs under that MFMA and the barrier wait)
        if constexpr (COMPUTE) strip_compute(std::integral_constant<int, P ^ 1>{}, std::integral_constant<int, COMPUTE ? ST : 0>{});
        if constexpr (decltype(relaxc)::value) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        load_frags(lds + (stage ^ 1) * STAGE_BYTES, 0, f0);
        issue(stage);
        mfmas(pc, f1);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
#pragma unroll
        for (int g = 0; g < NDMA; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, DMA_GAP, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - NDMA * DMA_GAP, 0);
        __builtin_amdgcn_sched_barrier(0);
        stage ^= 1;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using NoStrip = std::integral_constant<int, -1>;
    // one tile into accumulator set P; DRAIN: the other set holds the previous tile (strips under k-tiles 0..7)
    auto run_tile = [&](auto pc, auto drainc) {
        constexpr int P = decltype(pc)::value;
        constexpr bool DRAIN = decltype(drainc)::value;
        int z, ks, m0, n0;
        decode(tile, z, ks, m0, n0);
        const int next = tile + gridDim.x;
        const bool has_next = next < total;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[P][i][j][r] = 0.f;
        load_frags(lds + stage * STAGE_BYTES, 0, f0);
        if constexpr (DRAIN) {
            ktile(pc, std::integral_constant<int, 0>{}, std::false_type{});
            ktile(pc, std::integral_constant<int, 1>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 2>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 3>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 4>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 5>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 6>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 7>{}, std::true_type{});
            ktile(pc, std::integral_constant<int, 8>{}, std::true_type{});
            flush_guard();
        } else {
            for (int q = 0; q < 9; ++q) ktile(pc, NoStrip{}, std::false_type{});
        }
        int kt = 9;  // nk >= 11 (checked by the launcher)
        for (; kt < nk - 2; ++kt) ktile(pc, NoStrip{}, std::false_type{});
        if (has_next) setup_dma(next);
        for (; kt < nk; ++kt) ktile(pc, NoStrip{}, std::false_type{});
        // this tile's accumulators now wait for the next tile's k-loop (or the drain below)
        const GemmProblem pr = a.p[z];
        pend_C = pr.C;
        pend_osc = (a.out_scale_dev ? a.out_scale * *a.out_scale_dev : a.out_scale) * (pr.scale_dev ? *pr.scale_dev : 1.f);
        pend_m0 = m0;
        {
            PP_LANE_COORDS
            pend_n = n0 + wc_e * 64 + c4 * 4;
        }
        pend_bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pr.bias) {
            const float bsc = a.bias_scale_dev ? *a.bias_scale_dev : 1.f;
            const float4 b4 = *reinterpret_cast<const float4*>(pr.bias + pend_n);
            pend_bv = make_float4(b4.x * bsc, b4.y * bsc, b4.z * bsc, b4.w * bsc);
        }
    };
    auto drain = [&](auto qc) {  // behind the block's last tile
        strip_compute(qc, std::integral_constant<int, 0>{}); strip_store(std::integral_constant<int, 0>{});
        strip_compute(qc, std::integral_constant<int, 1>{}); strip_store(std::integral_constant<int, 1>{});
        strip_compute(qc, std::integral_constant<int, 2>{}); strip_store(std::integral_constant<int, 2>{});
        strip_compute(qc, std::integral_constant<int, 3>{}); strip_store(std::integral_constant<int, 3>{});
        strip_compute(qc, std::integral_constant<int, 4>{}); strip_store(std::integral_constant<int, 4>{});
        strip_compute(qc, std::integral_constant<int, 5>{}); strip_store(std::integral_constant<int, 5>{});
        strip_compute(qc, std::integral_constant<int, 6>{}); strip_store(std::integral_constant<int, 6>{});
        strip_compute(qc, std::integral_constant<int, 7>{}); strip_store(std::integral_constant<int, 7>{});
        flush_guard();
    };
    if (a.ablate & 4) {  // measurement: k-loops only, nothing is drained or stored
        for (; tile < total; tile += gridDim.x) run_tile(I0{}, std::false_type{});
        float keep = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) keep += acc[0][i][j][r];
        if (keep == 12345.678f) a.p[0].C[tid] = keep;  // keeps the MFMAs alive
        return;
    }
#undef PP_LANE_COORDS_UNUSED
    run_tile(I0{}, std::false_type{});
    tile += gridDim.x;
    for (;;) {
        if (tile >= total) { drain(I0{}); return; }
        run_tile(I1{}, std::true_type{});
        tile += gridDim.x;
        if (tile >= total) { drain(I1{}); return; }
        run_tile(I0{}, std::true_type{});
        tile += gridDim.x;
    }
}

template <int MI, int WAVES_M, int WAVES_N, bool CONV, int PURE = 0>
static int launch_glds(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    constexpr int GBM = MI * 32 * WAVES_M, GBN = 64 * WAVES_N;
    a.tiles_m = (M + GBM - 1) / GBM;
    a.tiles_n = (N + GBN - 1) / GBN;
    a.xcd_remap = (a.tiles_m % 8 == 0) ? 1 : 0;
    constexpr size_t lds = (size_t)2 * (GBM + GBN) * ROWB;
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_split_glds_kernel<MI, WAVES_M, WAVES_N, CONV, PURE>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.done(dev);
    }
    hipLaunchKernelGGL((gemm_nt_split_glds_kernel<MI, WAVES_M, WAVES_N, CONV, PURE>), dim3(a.tiles_m * a.tiles_n, 1, nprob),
                       dim3(WAVES_M * WAVES_N * 64), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

// sola_tune "gemm_gn_fuse" (EXPERIMENTS builds): 1 = encoder conv0-2 apply their GroupNorm + LeakyReLU in the GEMM epilogue.  Round 5 decision: CLOSED.
// 500 fused forwards were bit-repeatable, but the headline did not move (18.73 K against 18.80 K samples/s: GroupNorm -0.36 ms, GEMM +0.17 ms, the
// rest in the launches around them - on a launch that sits at the board's power limit the epilogue's arithmetic is paid in clock).  History (round 3): the
// fused epilogue showed two nondeterministic corruption faults during development whose cause was never pinned to an instruction
// (DESIGN.md 5); they are contained (no packed-f32 code: -fno-slp-vectorize + tests/test_host_cpu.py's disassembly check; no exec
// change in the interior epilogue; the repeatability stress in the GPU suite), but a ~2 % step-time gain does not justify shipping an
// unexplained fault's containment as the default.
int g_gemm_gn_fuse = 0;
int g_gemm_pp = 0;  // experiment (sola_tune "gemm_pp"): 1 = ping-pong kernel where it applies
int g_gemm_nw4 = 0;  // experiment (sola_tune "gemm_nw4"): plain f32-output launches on 256x128 tiles with four waves, one per SIMD
int g_gemm_k16 = 0;  // experiment (sola_tune "gemm_k16"): 256x128 tiles, 16-deep k-tiles, two four-wave blocks per CU
int g_gemm_persist = 1;  // 256x256 shape: 1 = persistent kernel (one block per CU walks the tiles), 0 = one tile per block
// measurement switches of the persistent kernel (sola_tune "gemm_stagger" / "gemm_order" / "gemm_trace"), all off in production
int g_gemm_stagger = 0, g_gemm_order = 0, g_gemm_trace = 0, g_gemm_ld = 0;
int g_gemm_slack_stagger = 40;  // sola_tune "gemm_slack_stagger": s_sleep(1) periods per k-tile at phase 1 for the blocks with a tile of slack (16-bit launches; 0 = off;
                                // A/B on one box, ragged bf16 step: 0 -> 17.64-17.73 ms, 40 -> 17.46-17.51, 75 -> 17.54)
static unsigned long long* g_trace_buf = nullptr;  // [1024 blocks][8 waves][gemm_trace_words], allocated on first use
constexpr size_t TRACE_BYTES = (size_t)1024 * 8 * gemm_trace_words * 8;
// copies the trace of the LAST traced launch to the host (synchronises the device); returns the number of bytes written, < 0 on error
extern "C" long long sola_gemm_trace_read(void* host, long long bytes) {
    if (!g_trace_buf) return 0;
    const size_t n = (size_t)bytes < TRACE_BYTES ? (size_t)bytes : TRACE_BYTES;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, g_trace_buf, n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long long)n;
}

#ifdef SOLA_EXPERIMENTS
template <bool CONV, int PURE>
static int launch_k16(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    a.tiles_m = (M + 255) / 256;
    a.tiles_n = (N + 127) / 128;
    a.xcd_remap = (a.tiles_m % 8 == 0) ? 1 : 0;
    constexpr size_t lds = (size_t)3 * (256 + 128) * 64;
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_split_glds_k16_kernel<CONV, PURE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.done(dev);
    }
    hipLaunchKernelGGL((gemm_nt_split_glds_k16_kernel<CONV, PURE>), dim3(a.tiles_m * a.tiles_n, 1, nprob), dim3(256), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
#endif

template <bool CONV, int RMODE, int CSP, int PURE = 0, int GNT = 0, int NW = 8, int TRACE = 0, int LD = 0>
static int launch_persist_t(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    constexpr int GBN = NW / 2 * 64;
    a.tiles_m = (M + 255) / 256;
    a.tiles_n = (N + GBN - 1) / GBN;
    a.xcd_remap = (a.tiles_m % 8 == 0) ? 1 : 0;
    a.nprob = nprob;
    constexpr size_t lds = (size_t)2 * (256 + GBN) * ROWB + NW * 16 * 64 * 4;  // two stages + one epilogue strip per wave (160 KiB at NW = 8)
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_split_glds_persist_kernel<CONV, RMODE, CSP, PURE, GNT, NW, TRACE, LD>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.done(dev);
    }
    const int n_cu = sola_cu_count();
    const int total = a.tiles_m * a.tiles_n * nprob * (a.ksplit > 1 ? a.ksplit : 1);
    const int grid = total < n_cu ? total : n_cu;
    hipLaunchKernelGGL((gemm_nt_split_glds_persist_kernel<CONV, RMODE, CSP, PURE, GNT, NW, TRACE, LD>), dim3(grid), dim3(NW * 64), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}


#ifdef SOLA_EXPERIMENTS
template <bool CONV, int CSP>
static int launch_pp_t(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    a.tiles_m = M / 256;
    a.tiles_n = N / 128;
    a.xcd_remap = (a.tiles_m % 8 == 0) ? 1 : 0;
    a.nprob = nprob;
    constexpr size_t lds = (size_t)2 * (256 + 128) * ROWB + 4 * 16 * 64 * 4;
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_split_glds_pp_kernel<CONV, CSP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        once.done(dev);
    }
    const int n_cu = sola_cu_count();
    const int total = a.tiles_m * a.tiles_n * nprob;
    const int grid = total < n_cu ? total : n_cu;
    hipLaunchKernelGGL((gemm_nt_split_glds_pp_kernel<CONV, CSP>), dim3(grid), dim3(256), lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
// the ping-pong kernel takes launches without residual / norm / split-K whose tiles are all interior and whose k-loop is long
// enough to drain eight strips under it
static bool pp_applies(const GldsArgs& a, int M, int N) {
    return g_gemm_pp && !a.p[0].R && !a.gn_gamma && a.ksplit <= 1 && M % 256 == 0 && N % 128 == 0 && (a.ldc & 3) == 0 && a.K / GBK >= 11 &&
           (!a.p[0].bias || (reinterpret_cast<uintptr_t>(a.p[0].bias) & 15) == 0);
}
#endif

template <bool CONV>
static int launch_persist(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
#ifdef SOLA_EXPERIMENTS
    if (pp_applies(a, M, N)) return a.c_sp16 ? launch_pp_t<CONV, 1>(a, M, N, nprob, s) : launch_pp_t<CONV, 0>(a, M, N, nprob, s);
#endif
    if (a.ksplit > 1) return launch_persist_t<CONV, 0, 0>(a, M, N, nprob, s);  // partial sums: f32, no residual
#ifdef SOLA_EXPERIMENTS
    if (a.gn_gamma) {  // conditions checked by gemm_gn_fusable()
        if (a.gn_tokens == 16) return launch_persist_t<CONV, 0, 1, false, 16>(a, M, N, nprob, s);
        if (a.gn_tokens == 8) return launch_persist_t<CONV, 0, 1, false, 8>(a, M, N, nprob, s);
        return launch_persist_t<CONV, 0, 1, false, 4>(a, M, N, nprob, s);
    }
#else
    SOLA_ARG(!a.gn_gamma, "gemm: the fused GroupNorm epilogue is compiled in EXPERIMENTS builds only (closed in round 5: no gain on the power-bound kernel)");
#endif
    const int rmode = !a.p[0].R ? 0 : (a.r_sp16 ? 2 : 1);
    if (a.c_sp16) {
        if (CONV || rmode == 0) return launch_persist_t<CONV, 0, 1>(a, M, N, nprob, s);
        return rmode == 2 ? launch_persist_t<false, 2, 1>(a, M, N, nprob, s) : launch_persist_t<false, 1, 1>(a, M, N, nprob, s);
    }
#ifdef SOLA_EXPERIMENTS
    if (g_gemm_nw4 && !CONV && rmode == 0 && a.ksplit <= 1) return launch_persist_t<false, 0, 0, false, 0, 4>(a, M, N, nprob, s);  // experiment
    // experiment (sola_tune "gemm_ld"): one wave of each SIMD's pair issues the whole DMA stream; 32-bit buffer offsets: rows within 2 GiB
    const int ld = (!CONV && g_gemm_ld && (long long)256 * a.lda * 4 < (1LL << 31) && (long long)256 * a.K * 4 < (1LL << 31)) ? g_gemm_ld : 0;
    if (g_gemm_trace && !CONV && rmode == 0) {  // measurement: the plain instantiation with cycle stamps
        if (!g_trace_buf && hipMalloc(&g_trace_buf, TRACE_BYTES) != hipSuccess) g_trace_buf = nullptr;
        if (g_trace_buf) {
            (void)hipMemsetAsync(g_trace_buf, 0, TRACE_BYTES, s);
            a.trace = g_trace_buf;
            if constexpr (!CONV) {
                if (ld == 1) return launch_persist_t<false, 0, 0, 0, 0, 8, 1, 1>(a, M, N, nprob, s);
                if (ld == 2) return launch_persist_t<false, 0, 0, 0, 0, 8, 1, 2>(a, M, N, nprob, s);
            }
            return launch_persist_t<false, 0, 0, 0, 0, 8, 1>(a, M, N, nprob, s);
        }
    }
    if constexpr (!CONV) {
        if (ld && rmode == 0) return ld == 1 ? launch_persist_t<false, 0, 0, 0, 0, 8, 0, 1>(a, M, N, nprob, s) : launch_persist_t<false, 0, 0, 0, 0, 8, 0, 2>(a, M, N, nprob, s);
    }
#endif
    if (CONV || rmode == 0) return launch_persist_t<CONV, 0, 0>(a, M, N, nprob, s);
    return rmode == 2 ? launch_persist_t<false, 2, 0>(a, M, N, nprob, s) : launch_persist_t<false, 1, 0>(a, M, N, nprob, s);
}
// plain f16 operands: C and the residual f16 (16-bit storage mode, inference) or both f32 (f16-operand training: the
// activations stay f32, only the GEMM inputs are cast); split-K partial sums are always f32 without residual
template <bool CONV>
static int launch_persist_pure(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    const bool has_r = a.p[0].R != nullptr;
    if (a.bf16) {  // bf16 operands (training with bf16 GEMM operands, BASELINE config C2): f32 outputs / residuals, or - round 6, the
        // step's 16-bit storage - bf16 outputs (with a bf16 residual)
        if (a.ksplit > 1) return launch_persist_t<CONV, 0, 0, 2>(a, M, N, nprob, s);
        if (a.c_f16) {
            if (CONV || !has_r) return launch_persist_t<CONV, 0, 2, 2>(a, M, N, nprob, s);
            return launch_persist_t<false, 3, 2, 2>(a, M, N, nprob, s);
        }
        if (has_r && !CONV) return launch_persist_t<false, 1, 0, 2>(a, M, N, nprob, s);
        return launch_persist_t<CONV, 0, 0, 2>(a, M, N, nprob, s);
    }
    if (a.ksplit > 1) return launch_persist_t<CONV, 0, 0, true>(a, M, N, nprob, s);
    if (a.c_f16) {
        if (CONV || !has_r) return launch_persist_t<CONV, 0, 2, true>(a, M, N, nprob, s);
        return launch_persist_t<false, 3, 2, true>(a, M, N, nprob, s);
    }
    if (has_r && !CONV) return launch_persist_t<false, 1, 0, true>(a, M, N, nprob, s);
    return launch_persist_t<CONV, 0, 0, true>(a, M, N, nprob, s);
}

// the persistent kernel takes residual / no residual from the launch, so every problem of the launch must agree
static bool persist_uniform(const GldsArgs& a, int conv) {
    for (int i = 1; i < a.nprob; ++i)
        if ((a.p[i].R != nullptr) != (a.p[0].R != nullptr)) return false;
    return !(conv && a.p[0].R);
}

template <bool CONV>
static int launch_shape_pure(GldsArgs& a, int shape, int M, int N, int nprob, hipStream_t s) {
    if (a.ksplit > 1) return launch_persist_pure<CONV>(a, M, N, nprob, s);
    // the persistent kernel's residual modes of this arithmetic: f16 residual into an f16 output, f32 into f32
    const bool r_ok = !a.p[0].R || (!CONV && ((a.r_f16 && a.c_f16) || (!a.r_f16 && !a.c_f16)));
    if (shape == 4 && g_gemm_persist && a.K / GBK >= 2 && persist_uniform(a, CONV) && r_ok) return launch_persist_pure<CONV>(a, M, N, nprob, s);
    if (a.bf16) return shape == 4 ? launch_glds<4, 2, 4, CONV, 2>(a, M, N, nprob, s) : launch_glds<2, 2, 2, CONV, 2>(a, M, N, nprob, s);
    if (shape == 4) return launch_glds<4, 2, 4, CONV, true>(a, M, N, nprob, s);
    return launch_glds<2, 2, 2, CONV, true>(a, M, N, nprob, s);
}

template <bool CONV>
static int launch_shape(GldsArgs& a, int shape, int M, int N, int nprob, hipStream_t s) {
    if (a.ksplit > 1) return launch_persist<CONV>(a, M, N, nprob, s);
#ifdef SOLA_EXPERIMENTS
    if (shape == 4 && g_gemm_k16 && !a.gn_gamma) return launch_k16<CONV, 0>(a, M, N, nprob, s);
#endif
    if (shape == 4 && g_gemm_persist && a.K / GBK >= 2 && persist_uniform(a, CONV)) return launch_persist<CONV>(a, M, N, nprob, s);
    if (shape == 4) return launch_glds<4, 2, 4, CONV>(a, M, N, nprob, s);
    return launch_glds<2, 2, 2, CONV>(a, M, N, nprob, s);
}

int g_gemm_ablate = 0;

extern int g_gemm_glds;
int gemm_split_glds_shape(const GemmDesc& d);
// The fused-GroupNorm epilogue exists for the persistent 256x256 kernel only, on interior tiles: split-f16 arithmetic and
// output, one problem, no residual, M and N multiples of 256, 64 channels per group (a wave's columns), 4 / 8 / 16 tokens.
bool gemm_gn_fusable(const GemmDesc& d, int channels_per_group, int tokens) {
#ifndef SOLA_EXPERIMENTS
    return false;  // round 5: closed (bit-repeatable over 500 forwards, but no gain: the epilogue's arithmetic costs the power-bound launch what the norm's pass saved - profiles/r05_gnf_decision.txt)
#endif
    return g_gemm_gn_fuse && g_gemm_persist && d.arith == 1 && d.nprob == 1 && !d.p[0].R && d.ksplit <= 1 && d.M % 256 == 0 && d.N % 256 == 0 &&
           d.K / GBK >= 2 && channels_per_group == 64 && (tokens == 4 || tokens == 8 || tokens == 16) && (d.ldc & 7) == 0 &&
           gemm_split_glds_supported(d) && gemm_split_glds_shape(d) == 4;
}

int launch_gemm_split_glds(const GemmDesc& d, hipStream_t s) {
    GldsArgs a;
    for (int i = 0; i < 3; ++i) a.p[i] = d.p[i < d.nprob ? i : 0];
    a.M = d.M; a.N = d.N; a.K = d.K; a.lda = d.lda; a.ldr = d.ldr; a.ldc = d.ldc;
    a.conv = d.conv; a.T_in = d.T_in; a.T_out = d.T_out; a.stride = d.stride; a.pad = d.pad; a.Cin = d.Cin;
    a.r_f16 = a.c_f16 = 0;
    a.bf16 = 0;
    a.bias_scale_dev = d.bias_scale_dev;
    if (d.arith == 2) {  // plain f16 (or bf16) operand rows: the kernels address A and W in 4-byte units of two 16-bit values
        a.K = d.K / 2; a.lda = d.lda / 2; a.Cin = d.Cin / 2;
        a.r_f16 = d.r_f16; a.c_f16 = d.c_f16;
        a.bf16 = d.bf16 ? 1 : 0;
        SOLA_ARG(!(a.bf16 && a.r_f16 && !a.c_f16), "gemm: a bf16 residual goes with a bf16 output");
    }
    a.rowmap = d.conv == 1 ? d.rowmap : nullptr;
    a.out_scale = d.out_scale != 0.f ? d.out_scale : 1.f;
    a.out_scale_dev = d.out_scale_dev;
    a.r_sp16 = d.r_sp16;
    a.c_sp16 = d.c_sp16;
    a.nprob = d.nprob;
    a.ablate = g_gemm_ablate;
    a.stagger = g_gemm_stagger; a.order = g_gemm_order; a.trace = nullptr;
    if (a.stagger == 0 && d.arith == 2 && d.bf16 && g_gemm_slack_stagger > 0) a.stagger = -g_gemm_slack_stagger;
    a.guard = (d.c_sp16 || d.c_f16) ? d.guard : nullptr;
    a.gn_gamma = d.gn_gamma; a.gn_beta = d.gn_beta; a.gn_tokens = d.gn_tokens; a.gn_eps = d.gn_eps; a.gn_slope = d.gn_slope;
    a.gn_icnt = d.gn_tokens > 0 ? 1.0f / (64.0f * (float)d.gn_tokens) : 0.f;
    a.ksplit = d.ksplit > 1 ? d.ksplit : 1;
    a.kper = a.K / GBK / a.ksplit;
    a.part = d.splitk_ws;
    const int shape = gemm_split_glds_shape(d);
    if (d.arith == 2) return d.conv == 1 ? launch_shape_pure<true>(a, shape, d.M, d.N, d.nprob, s) : launch_shape_pure<false>(a, shape, d.M, d.N, d.nprob, s);
    return d.conv == 1 ? launch_shape<true>(a, shape, d.M, d.N, d.nprob, s) : launch_shape<false>(a, shape, d.M, d.N, d.nprob, s);
}

// g_gemm_glds: 1 = 128x128 blocks, 4 = 256x256, anything else = auto: 256x256 when its tiles keep at least 3/4 of the
// CUs busy over its whole rounds of one block per CU (the 256x256 kernel is 15-25 % faster per flop than the 128x128
// one, so a last round down to half full still wins; below that the idle CUs cost more than the shape gains)
int gemm_split_glds_shape(const GemmDesc& d) {
    if (g_gemm_glds == 1 || g_gemm_glds == 4) return g_gemm_glds;
    const long long t = (long long)((d.M + 255) / 256) * ((d.N + 255) / 256) * d.nprob;
    const long long rounds = (t + 255) / 256;
    return (t >= 256 && 4 * t >= 3 * rounds * 256) ? 4 : 1;
}

// ---- weight gradients on row-major 16-bit operands (gemm_tn_tr_kernel) -------------------------------------------------------------
int g_train_tn_tr = 1;  // sola_tune "train_tn_tr": 0 = always the transposed-copy route of gemm_tn_split.hip
bool gemm_tn_tr_supported(int M, int N, int K, long long lda, long long ldb) {
    return g_train_tn_tr && N % 256 == 0 && K % 256 == 0 && lda % 8 == 0 && ldb % 8 == 0 && M >= 128;
}
// the number of row ranges: about one work item per CU, every range at least two 64-row k-tiles, at most max_ranges (the scratch)
void gemm_tn_tr_geometry(int M, int N, int K, int nprob, int max_ranges, int& ksplit, int& kper) {
    const int nkt = (M + 63) / 64;
    const int tiles = (N / 256) * (K / 256) * nprob;
    int ks = std::max(1, sola_cu_count() / std::max(1, tiles));
    ks = std::min(ks, std::min(max_ranges, std::max(1, nkt / 2)));
    if (ks >= 8) ks &= ~7;  // whole XCD groups (the kernel's work-item order)
    kper = (nkt + ks - 1) / ks;
    ksplit = (nkt + kper - 1) / kper;  // no empty range
}
int launch_splitk_reduce_bf16(const void* part, int ksplit, int nprob, float* const* C, int M, int N, int ldc, const float* out_scale_dev,
                              const float* scale_dev, hipStream_t s) {
    SOLA_ARG(part && ksplit >= 1 && nprob >= 1 && nprob <= 3 && N % 4 == 0 && ldc % 4 == 0, "splitk_reduce_bf16: ksplit %d nprob %d N %d", ksplit, nprob, N);
    const long long mn = (long long)M * N;
    hipLaunchKernelGGL(splitk_reduce_bf16_kernel, dim3((unsigned)((mn / 4 + 255) / 256), 1, nprob), dim3(256), 0, s, static_cast<const unsigned short*>(part),
                       ksplit, mn, N, ldc, C[0], C[nprob > 1 ? 1 : 0], C[nprob > 2 ? 2 : 0], out_scale_dev, scale_dev);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_gemm_tn_tr(const GemmTnTrDesc& d, hipStream_t s) {
    SOLA_ARG(d.nprob >= 1 && d.nprob <= 3 && d.part && d.ksplit >= 1 && d.kper >= 1, "gemm_tn_tr: nprob %d ksplit %d", d.nprob, d.ksplit);
    SOLA_ARG(gemm_tn_tr_supported(d.M, d.N, d.K, d.lda, d.ldb), "gemm_tn_tr: M=%d N=%d K=%d", d.M, d.N, d.K);
    SolaProfScope prof(SOLA_PROF_GEMM_SPLIT256, s, 2.0 * d.M * d.N * (double)d.K * d.nprob,
                       2.0 * d.nprob * ((double)d.M * d.N + (double)d.M * d.K) + 4.0 * d.nprob * d.ksplit * (double)d.N * d.K);
    TnTrArgs t{};
    GldsArgs& a = t.e;
    a.M = d.N; a.N = d.K; a.ldc = d.K; a.K = 0;
    a.tiles_m = d.N / 256; a.tiles_n = d.K / 256;
    a.out_scale = 1.f;
    a.ksplit = d.ksplit; a.part = d.part; a.nprob = d.nprob;
    a.ablate = g_gemm_ablate;
    if (d.part_bf16) { SOLA_ARG(d.bf16 && d.K % 4 == 0, "gemm_tn_tr: bfloat16 partial sums go with bfloat16 operands"); a.c_f16 = 1; a.bf16 = 1; }
    for (int j = 0; j < 3; ++j) {
        t.A[j] = static_cast<const char*>(d.A[j < d.nprob ? j : 0]);
        t.B[j] = static_cast<const char*>(d.B[j < d.nprob ? j : 0]);
        SOLA_ARG((reinterpret_cast<uintptr_t>(t.A[j]) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.B[j]) & 15) == 0, "gemm_tn_tr: operands must be 16-byte aligned");
    }
    t.a_sp = d.a_split ? 1 : 0; t.b_sp = d.b_split ? 1 : 0;
    t.lda = d.lda * (d.a_split ? 4 : 2); t.ldb = d.ldb * (d.b_split ? 4 : 2); t.Mred = d.M; t.kper = d.kper; t.nkt = (d.M + 63) / 64;
    SOLA_ARG((long long)d.ksplit * d.kper >= t.nkt && (long long)(d.ksplit - 1) * d.kper < t.nkt, "gemm_tn_tr: ranges %d x %d k-tiles do not cover %d", d.ksplit, d.kper, t.nkt);
    constexpr size_t lds = 2 * 2 * 64 * 512;
    t.Cin = d.Cin; t.T_in = d.T_in; t.T_out = d.T_out; t.stride = d.stride; t.pad = d.pad; t.rowmap = d.rowmap;
    const int conv = !d.conv ? 0 : (d.rowmap ? 2 : 1);
    SOLA_ARG(!conv || (d.Cin % 256 == 0 && d.K % d.Cin == 0 && d.K / d.Cin <= 8 && (d.rowmap || (d.T_out > 0 && d.T_in > 0 && d.stride >= 1))),
             "gemm_tn_tr: conv geometry Cin=%d K=%d", d.Cin, d.K);
    SOLA_ARG(!(d.bf16 && (d.a_split || d.b_split)), "gemm_tn_tr: split-f16 operands are f16");
    if (conv) t.ldb = (long long)d.Cin * (d.b_split ? 4 : 2);
    static DeviceOnce once[2][3];
    int dev;
    const dim3 grid(a.tiles_m * a.tiles_n * d.ksplit, 1, d.nprob);
    const void* fn = nullptr;
#define TN_TR_PICK(BFV, CV) if ((d.bf16 ? 1 : 0) == BFV && conv == CV) fn = reinterpret_cast<const void*>(&gemm_tn_tr_kernel<BFV, CV>);
    TN_TR_PICK(0, 0) TN_TR_PICK(0, 1) TN_TR_PICK(0, 2) TN_TR_PICK(1, 0) TN_TR_PICK(1, 1) TN_TR_PICK(1, 2)
#undef TN_TR_PICK
    DeviceOnce& o = once[d.bf16 ? 1 : 0][conv];
    if (o.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        o.done(dev);
    }
    void* kargs[] = {&t};
    SOLA_HIP(hipLaunchKernel(fn, grid, dim3(512), kargs, lds, s));
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
