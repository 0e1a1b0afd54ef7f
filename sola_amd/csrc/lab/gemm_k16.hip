// 16-deep k-tiles, two four-wave blocks per CU: a CLOSED EXPERIMENT of the split-f16 NT GEMM (round 3; slower: DESIGN.md Appendix A,
// profiles/r03_gemm_k16.txt).  Compiled in SOLA_EXPERIMENTS builds only (make EXPERIMENTS=1; sola_tune "gemm_k16" 1, default 0); routed
// to from gemm_glds.hip's launch_shape.
#include <type_traits>

#include "../gemm_glds.h"

#ifdef SOLA_EXPERIMENTS
namespace {

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
    tile_decode(a, blockIdx.x, rt, ct);
    const int m0 = rt * GBM, n0 = ct * GBN;

    // DMA coordinates of the 64-byte rows (not gemm_common.h's 128-byte layout): lane -> (row = piece * 16 + lane / 4, physical chunk = lane % 4)
    const int lrow = lane >> 2, chunk = lane & 3;
    const char* a_ptr[APW];
    const char* w_ptr[WPW];
    int a_t0[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = (wave * APW + i) * 16 + lrow;
        const int col_bytes = (chunk ^ ((r >> 2) & 3)) * 16;
        const int m = dma_clamp_row(m0 + r, a.M);
        if (CONV) {  // gemm_common.h's conv_window, written out: the experiment stays the kernel profiles/r03_gemm_k16.txt timed (gemm_common_isa.txt)
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
        const int n = dma_clamp_row(n0 + r, a.N);
        w_ptr[i] = reinterpret_cast<const char*>(pr.W + (long long)n * a.K) + (chunk ^ ((r >> 2) & 3)) * 16;
    }
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int nk = a.K / KB;
    int conv_kk = 0, conv_c = 0;
    int dma_kt = 0;

    auto issue = [&](int stage) {  // k-tiles in increasing order, one per call; past the last one the pointers stop (see gemm_glds.hip's one-tile kernel)
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
    constexpr int PER = PURE ? 2 : 3;  // MFMAs per accumulator and k-tile, in the order lo terms first (as in gemm_glds.hip's kernels)
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

template <bool CONV, int PURE>
static int launch_k16(GldsArgs& a, int M, int N, int nprob, hipStream_t s) {
    a.tiles_m = (M + 255) / 256;
    a.tiles_n = (N + 127) / 128;
    a.xcd_remap = xcd_remap_rows(a.tiles_m);
    constexpr size_t lds = (size_t)3 * (256 + 128) * 64;
    return launch_lds<gemm_nt_split_glds_k16_kernel<CONV, PURE>>(dim3(a.tiles_m * a.tiles_n, 1, nprob), dim3(256), lds, s, a);
}

}  // namespace

int g_gemm_k16 = 0;  // experiment (sola_tune "gemm_k16"): 256x128 tiles, 16-deep k-tiles, two four-wave blocks per CU

int launch_gemm_k16(GldsArgs& a, bool conv, int M, int N, int nprob, hipStream_t s) {
    return conv ? launch_k16<true, 0>(a, M, N, nprob, s) : launch_k16<false, 0>(a, M, N, nprob, s);
}
#endif
