// Exact-f32 weight-gradient GEMM (backward of F.linear / F.conv1d at tools/attention.py:63-73, module/ws.py:14-22):
//   gemm_tn_f32_kernel : P[s][n][k] = sum_{m in split s} A[m][n] * B[m][k]   ("TN": both operands reduce over ROWS)
//                        A = dY [M, N]; B = X [M, K] or the implicit im2col of the channels-last conv input.
//   gemm_tn_f32_group_kernel : the same tile for up to 32 problems in one launch, every block over all rows of its problem
// The splits' partial sums are folded in index order by reduce.hip's sum_slabs_kernel (deterministic, no float atomics).
// Exact f32 on v_mfma_f32_32x32x2_f32.  The reduction index m is the slow (row) index of both operands, so tiles are
// staged [32 m][128 cols] with coalesced float4 row loads and the MFMA fragments are ds_read_b32 across the columns
// (lanes 0-31 take row m, lanes 32-63 row m+1: consecutive addresses, conflict-free).
#include <algorithm>

#include "gemm_common.h"

namespace {

struct TnArgs {
    const float* A;  // [M, N]
    const float* B;  // [M, K] or conv source
    float* P;        // [splits][N][K]
    float* Pb;       // optional [splits][N]: column sums of A (bias gradient), written by the tk == 0 blocks
    int M, N, K, lda, ldb;
    int conv, T_in, T_out, stride, pad, Cin;  // conv gather on B (same convention as the NT kernel's mode 1)
    const int2* rowmap;  // conv, ragged batches: row m reads tap kk from source row rowmap[m].x + kk when bit kk of rowmap[m].y is set
    int tiles_n, tiles_k, m_per_split;
};

constexpr int TB = 128;       // output tile (n and k)
constexpr int TM = 32;        // rows of the reduction per LDS stage
constexpr int TP = TB + 4;    // LDS pitch (floats), 16-byte aligned rows

// one (tile, row split) work item: tile = tn * tiles_k + tk
// NW = 4: 2 x 2 waves of 64 x 64; NW = 8 (round 4): 4 x 2 waves of 32 x 64 - the CU's two blocks (LDS) put four waves on every SIMD instead of
// two, as in the NT kernel (gemm.hip); the same reduction order per output element: bit-identical.  (The bias gradient Pb is not: a
// thread sums rows 16 apart there and 8 apart at NW = 4, another fixed order - tests/test_gpu_gemm_tn.py holds it to float64 under both.)
template <int NW>
__device__ __forceinline__ void tn_tile(const TnArgs& a, int tile, int split, float* smem) {
    constexpr int TMW = NW == 8 ? 1 : 2;     // 32-row MFMA tiles per wave along n
    constexpr int LP = NW == 8 ? 2 : 4;      // load passes: 8 rows per pass at 256 threads, 16 at 512
    constexpr int LR = NW == 8 ? 16 : 8;
    float* As = smem;                 // [2][TM][TP]
    float* Bs = smem + 2 * TM * TP;   // [2][TM][TP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int tn = tile / a.tiles_k, tk = tile % a.tiles_k;
    const int n0 = tn * TB, k0 = tk * TB;
    const int m_begin = split * a.m_per_split;
    const int m_end = min(a.M, m_begin + a.m_per_split);

    // loads: 32 lanes cover one 128-float row; LR rows per pass, LP passes
    const int lrow = tid >> 5;         // 0..LR-1
    const int lcol = (tid & 31) << 2;  // 0..124
    float4 ra[LP], rb[LP];
    auto load_stage = [&](int mbase) {
        int kk = 0, ci = k0 + lcol;
        if (a.conv) {
            kk = ci / a.Cin;
            ci -= kk * a.Cin;
        }
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            const int m = mbase + lrow + LR * i;
            const bool mok = m < m_end;
            ra[i] = (mok && n0 + lcol < a.N) ? *reinterpret_cast<const float4*>(a.A + (long long)m * a.lda + n0 + lcol)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = mok && k0 + lcol < a.K;
            const float* src;
            if (a.conv && a.rowmap) {
                const int2 rm = a.rowmap[mok ? m : 0];
                ok = ok && ((rm.y >> kk) & 1);
                src = a.B + ((long long)rm.x + kk) * a.Cin + ci;
            } else if (a.conv) {
                const int r = m / a.T_out;
                const int to = m - r * a.T_out;
                const int ti = to * a.stride - a.pad + kk;
                ok = ok && ti >= 0 && ti < a.T_in;
                src = a.B + ((long long)r * a.T_in + ti) * a.Cin + ci;
            } else {
                src = a.B + (long long)m * a.ldb + k0 + lcol;
            }
            rb[i] = ok ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LP; ++i) {
            *reinterpret_cast<float4*>(&As[(buf * TM + lrow + LR * i) * TP + lcol]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[(buf * TM + lrow + LR * i) * TP + lcol]) = rb[i];
        }
    };

    f32x16 acc[TMW][2];
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool want_bias = a.Pb != nullptr && tk == 0;

    const int fcol = lane & 31, fm = lane >> 5;
    const int nstage = (m_end - m_begin + TM - 1) / TM;
    if (nstage > 0) {
        load_stage(m_begin);
        if (want_bias) {
#pragma unroll
            for (int i = 0; i < LP; ++i) { bsum.x += ra[i].x; bsum.y += ra[i].y; bsum.z += ra[i].z; bsum.w += ra[i].w; }
        }
        store_stage(0);
    }
    __syncthreads();
    for (int st = 0; st < nstage; ++st) {
        const int buf = st & 1;
        if (st + 1 < nstage) load_stage(m_begin + (st + 1) * TM);
        const float* Ab = &As[(buf * TM + fm) * TP + wr * (32 * TMW) + fcol];
        const float* Bb = &Bs[(buf * TM + fm) * TP + wc * 64 + fcol];
        // fragments of four row pairs at a time, the next four requested before the current four's MFMAs (as one unrolled loop the compiler
        // issued read -> full wait -> two MFMAs per row pair: the LDS latency sat between every pair of MFMAs)
        constexpr int CHK = 4, NCH = TM / 2 / CHK;
        float fa0[2][CHK], fa1[2][CHK], fb0[2][CHK], fb1[2][CHK];
        auto frag = [&](int cidx, int slot) {
#pragma unroll
            for (int e = 0; e < CHK; ++e) {
                const int mm = (cidx * CHK + e) * 2;
                fa0[slot][e] = Ab[mm * TP];
                if constexpr (TMW == 2) fa1[slot][e] = Ab[mm * TP + 32];
                fb0[slot][e] = Bb[mm * TP];
                fb1[slot][e] = Bb[mm * TP + 32];
            }
        };
        frag(0, 0);
#pragma unroll
        for (int cidx = 0; cidx < NCH; ++cidx) {
            const int slot = cidx & 1;
            if (cidx + 1 < NCH) frag(cidx + 1, slot ^ 1);
            __builtin_amdgcn_sched_barrier(0);  // keep the next chunk's reads in front of this chunk's MFMAs (the scheduler sinks loads to their uses)
#pragma unroll
            for (int e = 0; e < CHK; ++e) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[slot][e], fb0[slot][e], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[slot][e], fb1[slot][e], acc[0][1], 0, 0, 0);
                if constexpr (TMW == 2) {
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[slot][e], fb0[slot][e], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[slot][e], fb1[slot][e], acc[1][1], 0, 0, 0);
                }
            }
        }
        if (st + 1 < nstage) {
            if (want_bias) {
#pragma unroll
                for (int i = 0; i < LP; ++i) { bsum.x += ra[i].x; bsum.y += ra[i].y; bsum.z += ra[i].z; bsum.w += ra[i].w; }
            }
            store_stage(buf ^ 1);
        }
        __syncthreads();
    }
    if (want_bias) {
        float* red = smem;  // [LR][TB]: reduce the LR row lanes (the stage buffers are free after the last barrier)
        *reinterpret_cast<float4*>(&red[lrow * TB + lcol]) = bsum;
        __syncthreads();
        if (tid < TB && n0 + tid < a.N) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < LR; ++r) v += red[r * TB + tid];
            a.Pb[(long long)split * a.N + n0 + tid] = v;
        }
    }
    float* P = a.P + (long long)split * a.N * a.K;
    const int col_l = lane & 31, row_l = (lane >> 5) << 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = k0 + wc * 64 + j * 32 + col_l;
        if (k >= a.K) continue;
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wr * (32 * TMW) + i * 32 + (r & 3) + 8 * (r >> 2) + row_l;
                if (n < a.N) P[(long long)n * a.K + k] = acc[i][j][r];
            }
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void gemm_tn_f32_kernel(const TnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    tn_tile<NW>(a, (int)blockIdx.x, (int)blockIdx.y, smem);
}

// ---- grouped form (round 4): the weight gradients of ALL linear layers of a few-sample step in ONE launch --------------------------
// One sample per optimizer step (the reference's batch size) has 256-2000 token rows: a [1024 x 1024] weight gradient is 64 tiles
// whose reduction over the rows is 8-60 stages.  Per matrix the launch above cut the rows into slabs to fill the chip (16 MB of
// partial sums written and read back per matrix) and two sum_slabs launches folded them: 24 + 48 launches of 5-17 us per step, 0.63
// ms of a 2.7 ms step.  The backward now defers these products (backward.hip): each dY keeps a buffer of its own until the end, and
// this kernel takes them all - blockIdx.x = (problem, tile), every block reduces over ALL rows of its problem and writes its dW tile
// and bias gradient directly (no partial sums, no second pass, fixed summation order).
constexpr int TN_GROUP_MAX = 32;
struct TnGroupProb {
    const float* A;
    const float* B;
    float* C;
    float* db;
    const int2* rowmap;
    int M, N, K, lda, ldb;
    int conv, T_in, T_out, stride, pad, Cin;
    int tiles_k, tile_begin;  // this problem's tiles are [tile_begin, next problem's tile_begin)
};
struct TnGroupArgs {
    TnGroupProb p[TN_GROUP_MAX];
    int nprob;
};
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void gemm_tn_f32_group_kernel(const TnGroupArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int pi = 0;
    for (int j = 1; j < g.nprob; ++j)  // block-uniform, at most 32 entries
        if ((int)blockIdx.x >= g.p[j].tile_begin) pi = j;
    const TnGroupProb& q = g.p[pi];
    TnArgs a;
    a.A = q.A; a.B = q.B; a.P = q.C; a.Pb = q.db;
    a.M = q.M; a.N = q.N; a.K = q.K; a.lda = q.lda; a.ldb = q.ldb;
    a.conv = q.conv; a.T_in = q.T_in; a.T_out = q.T_out; a.stride = q.stride; a.pad = q.pad; a.Cin = q.Cin; a.rowmap = q.rowmap;
    a.tiles_n = 0; a.tiles_k = q.tiles_k;
    a.m_per_split = (a.M + TM - 1) / TM * TM;  // one split: every row
    tn_tile<NW>(a, (int)blockIdx.x - q.tile_begin, 0, smem);
}

// (round 4's grouped weight transposition - W -> W^T for the dX GEMMs of a few-sample backward, 49 matrices in one launch - left with round 5:
// those GEMMs read the weights where they lie, gemm.hip's NN form)

}  // namespace

int g_gemm_tn_nw8 = 1;  // sola_tune "gemm_tn_nw8": the exact-f32 weight-gradient kernels with eight waves per block (0 = four; A/B)
static int tn_splits(int M, int N, int K) {
    const long long tiles = (long long)((N + TB - 1) / TB) * ((K + TB - 1) / TB);
    int splits = (int)((768 + tiles - 1) / tiles);
    const int max_splits = (M + 4 * TM - 1) / (4 * TM);
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    return splits;
}

size_t gemm_tn_scratch_bytes(int M, int N, int K) {
    const int splits = tn_splits(M, N, K);
    const size_t one_tile = (size_t)splits * ((size_t)N * K + N) * sizeof(float);
    const int ps = gemm_tn_persist_plan(M, N, K);  // the persistent kernel's partial sums + the bias gradient's column-sum pass behind them
    const size_t persist = ps > 0 ? (size_t)ps * N * K * sizeof(float) + colsum_scratch_bytes(1, M, N) : 0;
    return std::max(one_tile, persist);
}

int launch_gemm_tn(const GemmTnDesc& d, hipStream_t s) {
    SOLA_ARG(d.M > 0 && d.N > 0 && d.K > 0 && d.N % 4 == 0 && d.K % 4 == 0, "gemm_tn: bad dims M=%d N=%d K=%d", d.M, d.N, d.K);
    SOLA_ARG(d.lda % 4 == 0 && (d.conv || d.ldb % 4 == 0), "gemm_tn: leading dims must be multiples of 4");
    if (d.conv) SOLA_ARG(d.Cin % 4 == 0 && d.K % d.Cin == 0, "gemm_tn conv: Cin=%d K=%d", d.Cin, d.K);
    TnArgs a;
    a.A = d.A; a.B = d.B; a.P = d.scratch; a.Pb = nullptr; a.M = d.M; a.N = d.N; a.K = d.K; a.lda = d.lda; a.ldb = d.ldb;
    gemm_fill_conv(a, d);
    a.tiles_n = (d.N + TB - 1) / TB;
    a.tiles_k = (d.K + TB - 1) / TB;
    const size_t need = gemm_tn_scratch_bytes(d.M, d.N, d.K);
    if (d.scratch_bytes < need) {
        sola_set_error("gemm_tn: scratch %zu < %zu", d.scratch_bytes, need);
        return SOLA_ERR_WORKSPACE;
    }
    const int splits = tn_splits(d.M, d.N, d.K);
    // round 5: the persistent kernel where the shape is its own (N % 256, K % 128, a grid that fills whole rounds).  Its partial sums stay
    // inside the scratch sized for `splits`; the bias gradient (column sums of dY) is a pass of its own there - launch_colsum in the
    // slab a split less leaves free (the one-tile kernel sums the rows it stages, in registers: vector adds the f32 MFMA cannot hide)
    {
        const size_t cs_need = d.bias_grad ? colsum_scratch_bytes(1, d.M, d.N) : 0;
        const int room = (int)std::min<size_t>(64, (d.scratch_bytes - std::min(d.scratch_bytes, cs_need)) / ((size_t)d.N * d.K * sizeof(float)));
        const int ps = room >= 1 ? gemm_tn_persist_splits(d, room) : 0;
        if (ps > 0) {
            int used = 0;
            {
                SolaProfScope prof(SOLA_PROF_GEMM_TN, s, 2.0 * d.M * d.N * (double)d.K, 4.0 * ((double)d.M * (d.N + d.K) + (double)ps * d.N * d.K));
                SOLA_TRY(launch_gemm_tn_f32_persist(d, ps, d.scratch, &used, s));
            }
            const long long n4 = (long long)d.N * d.K / 4;
            {
                SolaProfScope prof(SOLA_PROF_MISC, s, 0, 4.0 * (used + 1.0) * d.N * d.K);
                SOLA_TRY(sum_slabs(d.scratch, d.C, n4, used, s));
            }
            if (d.bias_grad) {
                float* cs = d.scratch + (size_t)used * d.N * d.K;
                SOLA_TRY(launch_colsum(d.A, d.bias_grad, 1, d.M, d.N, d.lda, 1.0f, 0, cs, d.scratch_bytes - (size_t)used * d.N * d.K * sizeof(float), s));
            }
            return SOLA_OK;
        }
    }
    if (d.bias_grad) a.Pb = d.scratch + (size_t)splits * d.N * d.K;
    int mps = (d.M + splits - 1) / splits;
    mps = (mps + TM - 1) / TM * TM;
    a.m_per_split = mps;
    constexpr size_t lds = (size_t)4 * TM * TP * sizeof(float);
    {
        SolaProfScope prof(SOLA_PROF_GEMM_TN, s, 2.0 * d.M * d.N * (double)d.K, 4.0 * ((double)d.M * (d.N + d.K) + (double)splits * d.N * d.K));
        const dim3 grid(a.tiles_n * a.tiles_k, splits);
        SOLA_TRY(g_gemm_tn_nw8 ? launch_lds<gemm_tn_f32_kernel<8>>(grid, dim3(512), lds, s, a) : launch_lds<gemm_tn_f32_kernel<4>>(grid, dim3(256), lds, s, a));
    }
    {
        const long long n4 = (long long)d.N * d.K / 4;
        SolaProfScope prof(SOLA_PROF_MISC, s, 0, 4.0 * (splits + 1.0) * d.N * d.K);
        SOLA_TRY(sum_slabs(d.scratch, d.C, n4, splits, s));
        if (d.bias_grad) SOLA_TRY(sum_slabs(a.Pb, d.bias_grad, d.N / 4, splits, s));
    }
    return SOLA_OK;
}

int launch_gemm_tn_group(const GemmTnGroupDesc& d, hipStream_t s) {
    SOLA_ARG(d.nprob >= 1 && d.nprob <= TN_GROUP_MAX, "gemm_tn_group: nprob=%d", d.nprob);
    TnGroupArgs g;
    g.nprob = d.nprob;
    double flops = 0, bytes = 0;
    int tiles = 0;
    for (int j = 0; j < d.nprob; ++j) {
        const GemmTnGroupDesc::Prob& q = d.p[j];
        SOLA_ARG(q.A && q.B && q.C && q.M > 0 && q.N > 0 && q.K > 0 && q.N % 4 == 0 && q.K % 4 == 0 && q.lda % 4 == 0 && (q.conv || q.ldb % 4 == 0),
                 "gemm_tn_group: problem %d (M=%d N=%d K=%d)", j, q.M, q.N, q.K);
        if (q.conv) SOLA_ARG(q.Cin % 4 == 0 && q.K % q.Cin == 0, "gemm_tn_group conv: Cin=%d K=%d", q.Cin, q.K);
        TnGroupProb& o = g.p[j];
        o.A = q.A; o.B = q.B; o.C = q.C; o.db = q.bias_grad; o.rowmap = q.conv ? q.rowmap : nullptr;
        o.M = q.M; o.N = q.N; o.K = q.K; o.lda = q.lda; o.ldb = q.ldb;
        o.conv = q.conv; o.T_in = q.T_in; o.T_out = q.T_out; o.stride = q.stride; o.pad = q.pad; o.Cin = q.Cin;
        o.tiles_k = (q.K + TB - 1) / TB;
        o.tile_begin = tiles;
        tiles += ((q.N + TB - 1) / TB) * o.tiles_k;
        flops += 2.0 * q.M * q.N * (double)q.K;
        bytes += 4.0 * ((double)q.M * (q.N + q.K) + (double)q.N * q.K);
    }
    constexpr size_t lds = (size_t)4 * TM * TP * sizeof(float);
    SolaProfScope prof(SOLA_PROF_GEMM_TN, s, flops, bytes);
    if (g_gemm_tn_nw8) return launch_lds<gemm_tn_f32_group_kernel<8>>(dim3((unsigned)tiles), dim3(512), lds, s, g);
    return launch_lds<gemm_tn_f32_group_kernel<4>>(dim3((unsigned)tiles), dim3(256), lds, s, g);
}
