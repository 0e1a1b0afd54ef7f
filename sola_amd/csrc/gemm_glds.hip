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
// This file: the one-tile-per-block kernel, the persistent kernel and the shape routing.  The kernel arguments and the one-tile epilogue
// are in gemm_glds.h: gemm_tn_tr.hip (the weight-gradient product on row-major 16-bit operands) and the two closed experiments of this
// family, lab/gemm_k16.hip and lab/gemm_pp.hip (EXPERIMENTS=1 builds), share them.
#include <algorithm>
#include <type_traits>

#include "gemm_glds.h"

namespace {

// PURE = plain 16-bit operands (GemmDesc::ab F16 / BF16): the same 128-byte tile rows now hold 64 consecutive halfs instead of 32
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
    tile_decode(a, blockIdx.x, rt, ct);
    const int m0 = rt * GBM, n0 = ct * GBN;

    // ---- DMA coordinates: this wave owns row groups wave*APW + i (8 rows each) of the A tile and wave*WPW + i of the
    //      W tile; lane -> (row = rg*8 + lane/8, physical 16-byte chunk = lane%8).  Each piece keeps a running source
    //      pointer that advances 128 B per k-tile: also for the implicit-im2col conv, where the receptive field of an
    //      output row is (t0*Cin + k) contiguous floats of the channels-last input, so only the zero-padding test
    //      depends on k.
    const int lrow = dma_lane_row(lane), chunk = dma_lane_chunk(lane);
    const char* a_ptr[APW];
    const char* w_ptr[WPW];
    int a_t0[APW];  // CONV: validity bits of the window's taps
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = (wave * APW + i) * 8 + lrow;     // tile-local A row
        const int col_bytes = dma_src_chunk_bytes(chunk, r);
        const int m = dma_clamp_row(m0 + r, a.M);
        if (CONV) {
            long long row0;
            conv_window(a, m, row0, a_t0[i]);
            a_ptr[i] = reinterpret_cast<const char*>(pr.A) + row0 * a.Cin * 4 + col_bytes;
        } else {
            a_t0[i] = 0;
            a_ptr[i] = reinterpret_cast<const char*>(pr.A + (long long)m * a.lda) + col_bytes;
        }
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        const int r = (wave * WPW + i) * 8 + lrow;  // tile-local W row
        const int n = dma_clamp_row(n0 + r, a.N);
        w_ptr[i] = reinterpret_cast<const char*>(pr.W + (long long)n * a.K) + dma_src_chunk_bytes(chunk, r);
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
    // LOCAL FORMS: this kernel sits at a spill boundary.  Its decode and the row / window / swizzle arithmetic of setup_dma are
    // gemm_common.h's tile_decode and composite-column rule, conv_window and dma_* helpers written out: taken through the helpers, every
    // instantiation's register row moves and the conv ones spill vector registers (profiles/gemm_common_isa.txt).  a.order == 1 is
    // a measurement order of this kernel alone.
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
        } else if (a.xcd_remap) {  // gemm_common.h's tile_decode and composite-column rule, written out (below)
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
            auto note_range = [&](const float (&v)[4]) { out_of_range |= f16_range_ballot4(v); };
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
                        if (PURE != 2) f16_range_guard4(a.guard, v);
                    } else if (CSP == 1) {
                        if (n >= a.N) continue;  // N % 8 == 0 and n % 4 == 0: the four columns are in range together
                        _Float16* cb = reinterpret_cast<_Float16*>(pr.C + (long long)m * ldc + (n & ~7)) + (n & 4);
                        half4 hh, ll;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { _Float16 h1, l1; split_f16(v[e], h1, l1); hh[e] = h1; ll[e] = l1; }
                        *reinterpret_cast<half4*>(cb) = hh;
                        *reinterpret_cast<half4*>(cb + 8) = ll;
                        f16_range_guard4(a.guard, v);
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
    if (is_row16(d.ab)) {  // plain 16-bit rows: sizes in halfs, two per 4-byte unit
        if (d.K % (2 * GBK) != 0 || d.conv == 2) return false;
        return d.conv == 1 ? d.Cin % (2 * GBK) == 0 : d.lda % 16 == 0;
    }
    if (d.ab != Elem::SP16 || d.K % GBK != 0 || d.conv == 2) return false;
    if (d.conv == 1) return d.Cin % GBK == 0;
    return d.lda % 8 == 0;
}

template <int MI, int WAVES_M, int WAVES_N, bool CONV, int PURE = 0>
static int launch_glds(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    constexpr int GBM = MI * 32 * WAVES_M, GBN = 64 * WAVES_N;
    a.tiles_m = (M + GBM - 1) / GBM;
    a.tiles_n = (N + GBN - 1) / GBN;
    a.xcd_remap = xcd_remap_rows(a.tiles_m);
    constexpr size_t lds = (size_t)2 * (GBM + GBN) * ROWB;
    return launch_lds<gemm_nt_split_glds_kernel<MI, WAVES_M, WAVES_N, CONV, PURE>>(dim3(a.tiles_m * a.tiles_n, 1, nprob), dim3(WAVES_M * WAVES_N * 64), lds, s, a);
}

// sola_tune "gemm_gn_fuse" (EXPERIMENTS builds): 1 = encoder conv0-2 apply their GroupNorm + LeakyReLU in the GEMM epilogue.  Round 5 decision: CLOSED.
// 500 fused forwards were bit-repeatable, but the headline did not move (18.73 K against 18.80 K samples/s: GroupNorm -0.36 ms, GEMM +0.17 ms, the
// rest in the launches around them - on a launch that sits at the board's power limit the epilogue's arithmetic is paid in clock).  History (round 3): the
// fused epilogue showed two nondeterministic corruption faults during development whose cause was never pinned to an instruction
// (DESIGN.md 5); they are contained (no packed-f32 code: -fno-slp-vectorize + tests/test_host_cpu.py's disassembly check; no exec
// change in the interior epilogue; the repeatability stress in the GPU suite), but a ~2 % step-time gain does not justify shipping an
// unexplained fault's containment as the default.
int g_gemm_gn_fuse = 0;
int g_gemm_nw4 = 0;  // experiment (sola_tune "gemm_nw4"): plain f32-output launches on 256x128 tiles with four waves, one per SIMD
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

template <bool CONV, int RMODE, int CSP, int PURE = 0, int GNT = 0, int NW = 8, int TRACE = 0, int LD = 0>
static int launch_persist_t(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    constexpr int GBN = NW / 2 * 64;
    a.tiles_m = (M + 255) / 256;
    a.tiles_n = (N + GBN - 1) / GBN;
    a.xcd_remap = xcd_remap_rows(a.tiles_m);
    a.nprob = nprob;
    constexpr size_t lds = (size_t)2 * (256 + GBN) * ROWB + NW * 16 * 64 * 4;  // two stages + one epilogue strip per wave (160 KiB at NW = 8)
    const int total = a.tiles_m * a.tiles_n * nprob * (a.ksplit > 1 ? a.ksplit : 1);
    const int grid = std::min(total, sola_cu_count());  // one block per CU walks the tiles
    return launch_lds<gemm_nt_split_glds_persist_kernel<CONV, RMODE, CSP, PURE, GNT, NW, TRACE, LD>>(dim3(grid), dim3(NW * 64), lds, s, a);
}


template <bool CONV>
static int launch_persist(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
#ifdef SOLA_EXPERIMENTS
    if (gemm_pp_applies(a, M, N)) return launch_gemm_pp(a, CONV, M, N, nprob, s);
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
template <bool CONV, int PURE>
static int launch_persist_pure_t(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    const bool has_r = a.p[0].R != nullptr;
    if (a.ksplit > 1) return launch_persist_t<CONV, 0, 0, PURE>(a, M, N, nprob, s);
    if (a.c_f16) {  // 16-bit outputs (with a 16-bit residual)
        if (CONV || !has_r) return launch_persist_t<CONV, 0, 2, PURE>(a, M, N, nprob, s);
        return launch_persist_t<false, 3, 2, PURE>(a, M, N, nprob, s);
    }
    if (has_r && !CONV) return launch_persist_t<false, 1, 0, PURE>(a, M, N, nprob, s);
    return launch_persist_t<CONV, 0, 0, PURE>(a, M, N, nprob, s);
}
// PURE = 2: bf16 operands (training with bf16 GEMM operands, BASELINE config C2): f32 outputs / residuals, or - round 6, the step's 16-bit
// storage - bf16 outputs; PURE = 1: f16
template <bool CONV>
static int launch_persist_pure(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    return a.bf16 ? launch_persist_pure_t<CONV, 2>(a, M, N, nprob, s) : launch_persist_pure_t<CONV, 1>(a, M, N, nprob, s);
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
    if (shape == 4 && g_gemm_k16 && !a.gn_gamma) return launch_gemm_k16(a, CONV, M, N, nprob, s);
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
    return g_gemm_gn_fuse && g_gemm_persist && d.ab == Elem::SP16 && d.nprob == 1 && !d.p[0].R && d.ksplit <= 1 && d.M % 256 == 0 && d.N % 256 == 0 &&
           d.K / GBK >= 2 && channels_per_group == 64 && (tokens == 4 || tokens == 8 || tokens == 16) && (d.ldc & 7) == 0 &&
           gemm_split_glds_supported(d) && gemm_split_glds_shape(d) == 4;
}

int launch_gemm_split_glds(const GemmDesc& d, hipStream_t s) {
    GldsArgs a;
    gemm_fill_common(a, d);
    a.r_f16 = a.c_f16 = 0;
    a.bf16 = 0;
    a.bias_scale_dev = d.bias_scale_dev;
    if (is_row16(d.ab)) {  // plain f16 (or bf16) operand rows: the kernels address A and W in 4-byte units of two 16-bit values
        a.K = d.K / 2; a.lda = d.lda / 2; a.Cin = d.Cin / 2;
        a.r_f16 = is_row16(d.r); a.c_f16 = is_row16(d.c);  // (the operands' format: gemm_formats_ok)
        a.bf16 = d.ab == Elem::BF16;
    }
    a.out_scale = d.out_scale != 0.f ? d.out_scale : 1.f;
    a.out_scale_dev = d.out_scale_dev;
    a.r_sp16 = d.r == Elem::SP16;
    a.c_sp16 = d.c == Elem::SP16;
    a.nprob = d.nprob;
    a.ablate = g_gemm_ablate;
    a.stagger = g_gemm_stagger; a.order = g_gemm_order; a.trace = nullptr;
    if (a.stagger == 0 && d.ab == Elem::BF16 && g_gemm_slack_stagger > 0) a.stagger = -g_gemm_slack_stagger;
    a.guard = d.c != Elem::F32 ? d.guard : nullptr;
    a.gn_gamma = d.gn_gamma; a.gn_beta = d.gn_beta; a.gn_tokens = d.gn_tokens; a.gn_eps = d.gn_eps; a.gn_slope = d.gn_slope;
    a.gn_icnt = d.gn_tokens > 0 ? 1.0f / (64.0f * (float)d.gn_tokens) : 0.f;
    a.ksplit = d.ksplit > 1 ? d.ksplit : 1;
    a.kper = a.K / GBK / a.ksplit;
    a.part = d.splitk_ws;
    const int shape = gemm_split_glds_shape(d);
    if (is_row16(d.ab)) return d.conv == 1 ? launch_shape_pure<true>(a, shape, d.M, d.N, d.nprob, s) : launch_shape_pure<false>(a, shape, d.M, d.N, d.nprob, s);
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

