// DAVIS boundary (contour) F-measure counts on the column-major bit planes of jf.hip: for every (expression e, frame t)
//   fg = OR of e's selected track planes, gt = OR of its GT planes (the id lists of sola_mask_select_counts),
//   B(m)[y,x] = m[y,x] differs from an in-image neighbour among east, south, south-east,
//   dil(B)    = B dilated by the disk dy*dy + dx*dx <= r*r, nothing coming in from outside the image,
//   counts[e,t] = |B(fg)|, |B(gt)|, |B(fg) & dil(B(gt))|, |B(gt) & dil(B(fg))|   (int64, exact).
//
// boundary_counts_kernel: one block per (column strip, e*T + t).  A strip is C output columns plus a halo of r columns on
// each side for the disk and one more on the right for the east neighbour.  Everything lives in LDS as COLUMNS RE-ALIGNED
// TO WORDS: column c owns cw = ceil(h/32) words (bit j of word k = row 32k + j, tail bits zero) followed by NW zero guard
// words (NW more in front of column 0), so a vertical neighbour is a bit shift inside the column that reads zeros past
// either end, and the east / south-east neighbours are the same words of column c+1.
//   1. masks:    word (c,k) = 32 bits at COCO position x*h + 32k of the OR of the listed planes: two global words and a
//                funnel shift, cut to the rows of the column.  Columns outside the image are zero.
//   2. boundary: (m ^ east) | (m ^ south) | (m ^ south-east), south tests only in rows < h-1, east tests only for x < w-1.
//   3. counts:   popcounts of the boundary words of the C output columns; where a boundary word is not zero, the other
//                side's dilated boundary at that word.  The disk is, per dx, the column x+dx dilated vertically by
//                v(dx) = floor(sqrt(r*r - dx*dx)); v falls as |dx| grows and dilations compose, so one window of 2NW+1 words
//                takes the columns in from dx = 0 outwards (P |= B[x-dx] | B[x+dx]) and is dilated by v(dx-1) - v(dx)
//                before each step: r unit dilations in all, whatever the number of columns.  What is wrong at the window's
//                ends moves one bit inwards per unit dilation and never reaches the centre word (r <= 32 NW).
// The four block sums are added to counts with int64 atomics (exact in any order) after a memset on the same stream: no
// workspace, nothing shared between calls.
#include <algorithm>

#include "kernels.h"

namespace {

constexpr int BF_THREADS = 512;
constexpr int BF_MAX_RADIUS = 64;
// dynamic LDS of a block; 1 KiB of each share is left to the kernel's static arrays
constexpr size_t BF_LDS_TWO_BLOCKS = 79 * 1024;   // two blocks per CU
constexpr size_t BF_LDS_ONE_BLOCK = 159 * 1024;   // the whole LDS of a CU

__device__ __forceinline__ uint32_t low_bits(int n) {  // bits 0..n-1, any n
    return n >= 32 ? 0xffffffffu : n <= 0 ? 0u : (1u << n) - 1u;
}

struct BfArgs {
    const uint32_t* bits;
    long long stride;  // words per plane
    int M, T, h, w, r;
    int cw, cs;        // words per column, words from one column to the next (cw + NW)
    int C, ncols;      // output columns per strip, mask columns staged per strip (C + 2r + 1)
    const int *pred_off, *pred_idx, *gt_off, *gt_idx;
    unsigned long long* counts;
};

template <int NW>
__device__ __forceinline__ uint32_t dilated_word(const uint32_t* __restrict__ B, const int* __restrict__ vt, int r, int cs,
                                                 int at) {
    // `at` = the centre word in column x; column x+dx is dx*cs words further
    constexpr int N = 2 * NW + 1;
    uint32_t P[N];
#pragma unroll
    for (int j = 0; j < N; ++j) P[j] = B[at + j - NW];
    int v_prev = r;
    for (int dx = 1; dx <= r; ++dx) {
        const int v = vt[dx];
        for (int i = v; i < v_prev; ++i) {  // one unit dilation
            uint32_t Q[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const uint32_t below = j > 0 ? P[j - 1] >> 31 : 0u, above = j + 1 < N ? P[j + 1] << 31 : 0u;
                Q[j] = P[j] | (P[j] << 1) | below | (P[j] >> 1) | above;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) P[j] = Q[j];
        }
        v_prev = v;
        const int a = at + dx * cs, b = at - dx * cs;
#pragma unroll
        for (int j = 0; j < N; ++j) P[j] |= B[a + j - NW] | B[b + j - NW];
    }
    return P[NW];  // v(r) = 0: nothing left to dilate by
}

template <int NW>
__global__ __launch_bounds__(BF_THREADS) void boundary_counts_kernel(const BfArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bf_lds[];
    __shared__ int vt[BF_MAX_RADIUS + 1];
    __shared__ unsigned red[4][BF_THREADS / 64];
    const int arr = NW + a.ncols * a.cs;  // words of one staged array
    uint32_t* Mp = bf_lds;
    uint32_t* Mg = Mp + arr;
    uint32_t* Bp = Mg + arr;
    uint32_t* Bg = Bp + arr;
    const int tid = threadIdx.x;
    const long long et = blockIdx.x;
    const int e = (int)(et / a.T), t = (int)(et - (long long)e * a.T);
    const int x_first = (int)blockIdx.y * a.C - a.r;  // image column of staged column 0
    const int p0 = a.pred_off[e], p1 = a.pred_off[e + 1], g0 = a.gt_off[e], g1 = a.gt_off[e + 1];
    const int h = a.h, w = a.w, cw = a.cw, cs = a.cs;

    if (tid <= a.r) {  // v(dx) = floor(sqrt(r*r - dx*dx)), in integers
        const int left = a.r * a.r - tid * tid;
        int v = 0;
        while ((v + 1) * (v + 1) <= left) ++v;
        vt[tid] = v;
    }
    if (tid < NW) Mp[tid] = Mg[tid] = Bp[tid] = Bg[tid] = 0;  // the guard words in front of column 0

    // 1. the masks of the strip, columns re-aligned to words
    const int n_words = a.ncols * cs;
    for (int i = tid; i < n_words; i += BF_THREADS) {
        const int c = i / cs, k = i - c * cs;
        const int x = x_first + c;
        uint32_t mp = 0, mg = 0;
        if (k < cw && x >= 0 && x < w) {
            const long long pos = (long long)x * h + 32 * k;  // < h*w: 32k < h
            const long long wi = pos >> 5;
            const int sh = (int)(pos & 31);
            const bool two = sh != 0 && wi + 1 < a.stride;
            uint32_t plo = 0, phi = 0, glo = 0, ghi = 0;
            for (int j = p0; j < p1; ++j) {
                const int m = a.pred_idx[j];
                if ((unsigned)m >= (unsigned)a.M) continue;
                const uint32_t* pl = a.bits + ((long long)m * a.T + t) * a.stride;
                plo |= pl[wi];
                if (two) phi |= pl[wi + 1];
            }
            for (int j = g0; j < g1; ++j) {
                const int m = a.gt_idx[j];
                if ((unsigned)m >= (unsigned)a.M) continue;
                const uint32_t* pl = a.bits + ((long long)m * a.T + t) * a.stride;
                glo |= pl[wi];
                if (two) ghi |= pl[wi + 1];
            }
            const uint32_t rows = low_bits(h - 32 * k);
            mp = (sh ? (plo >> sh) | (phi << (32 - sh)) : plo) & rows;
            mg = (sh ? (glo >> sh) | (ghi << (32 - sh)) : glo) & rows;
        }
        Mp[NW + i] = mp;
        Mg[NW + i] = mg;
    }
    __syncthreads();

    // 2. boundary maps of the first ncols - 1 columns (the last one is only somebody's east neighbour)
    for (int i = tid; i < n_words; i += BF_THREADS) {
        const int c = i / cs, k = i - c * cs;
        const int x = x_first + c;
        uint32_t bp = 0, bg = 0;
        if (k < cw && x >= 0 && x < w && c + 1 < a.ncols) {
            const uint32_t south_rows = low_bits(h - 1 - 32 * k);
            const bool east = x + 1 < w;
            const int at = NW + i;
            {
                const uint32_t m = Mp[at], s = (m >> 1) | (Mp[at + 1] << 31);
                bp = (m ^ s) & south_rows;
                if (east) {
                    const uint32_t em = Mp[at + cs], es = (em >> 1) | (Mp[at + cs + 1] << 31);
                    bp |= (m ^ em) | ((m ^ es) & south_rows);
                }
            }
            {
                const uint32_t m = Mg[at], s = (m >> 1) | (Mg[at + 1] << 31);
                bg = (m ^ s) & south_rows;
                if (east) {
                    const uint32_t em = Mg[at + cs], es = (em >> 1) | (Mg[at + cs + 1] << 31);
                    bg |= (m ^ em) | ((m ^ es) & south_rows);
                }
            }
        }
        Bp[NW + i] = bp;
        Bg[NW + i] = bg;
    }
    __syncthreads();

    // 3. the C output columns
    unsigned n_fg = 0, n_gt = 0, fg_match = 0, gt_match = 0;  // a thread sees at most ncols*cs*32 / BF_THREADS pixels
    const int n_out = a.C * cw;
    for (int i = tid; i < n_out; i += BF_THREADS) {
        const int c = i / cw, k = i - c * cw;
        const int at = NW + (c + a.r) * cs + k;
        const uint32_t bp = Bp[at], bg = Bg[at];
        n_fg += __popc(bp);
        n_gt += __popc(bg);
        if (bp) fg_match += __popc(bp & dilated_word<NW>(Bg, vt, a.r, cs, at));
        if (bg) gt_match += __popc(bg & dilated_word<NW>(Bp, vt, a.r, cs, at));
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_fg += __shfl_xor(n_fg, o, 64);
        n_gt += __shfl_xor(n_gt, o, 64);
        fg_match += __shfl_xor(fg_match, o, 64);
        gt_match += __shfl_xor(gt_match, o, 64);
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
        red[0][wave] = n_fg; red[1][wave] = n_gt; red[2][wave] = fg_match; red[3][wave] = gt_match;
    }
    __syncthreads();
    if (tid < 4) {
        unsigned long long s = 0;
        for (int j = 0; j < BF_THREADS / 64; ++j) s += red[tid][j];
        if (s) atomicAdd(a.counts + et * 4 + tid, s);
    }
}

struct BfPlan {
    int nw, cw, cs, C, ncols, strips;
    size_t lds;
};

// Strip width: as many output columns as fit two blocks per CU; the whole LDS of a CU when that leaves fewer than 32
// columns (tall frames, large radii).  C == 0: the frame does not fit at all.
BfPlan bf_plan(int h, int w, int r) {
    BfPlan p{};
    p.nw = r > 32 ? 2 : 1;
    p.cw = (h + 31) / 32;
    p.cs = p.cw + p.nw;
    const long long halo = 2ll * r + 1;
    auto fit = [&](size_t budget) { return (long long)((budget / 16 - (size_t)p.nw) / (size_t)p.cs) - halo; };
    long long c = fit(BF_LDS_TWO_BLOCKS);
    if (c < std::min<long long>(w, 32)) c = fit(BF_LDS_ONE_BLOCK);
    if (c < 1) return p;
    c = std::min<long long>(c, w);
    p.strips = (int)((w + c - 1) / c);
    p.C = (w + p.strips - 1) / p.strips;  // even strips
    p.ncols = p.C + (int)halo;
    p.lds = 16 * ((size_t)p.nw + (size_t)p.ncols * p.cs);
    return p;
}

template <int NW>
int bf_launch(const BfArgs& a, const BfPlan& p, long long blocks, hipStream_t s) {
    static DeviceOnce once;
    int dev;
    if (once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&boundary_counts_kernel<NW>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_ONE_BLOCK));
        once.done(dev);
    }
    hipLaunchKernelGGL(boundary_counts_kernel<NW>, dim3((unsigned)blocks, (unsigned)p.strips), dim3(BF_THREADS), p.lds, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

}  // namespace

extern "C" size_t sola_boundary_counts_workspace_bytes(int h, int w, int radius, int E, int T) {
    (void)h; (void)w; (void)radius; (void)E; (void)T;
    return 0;  // the strips of a frame meet in int64 atomics on counts
}

extern "C" int sola_mask_select_boundary_counts(const uint32_t* bits, int64_t words_stride, int n_masks, int T, int h, int w, int radius,
                                                const int32_t* pred_off, const int32_t* pred_idx, const int32_t* gt_off,
                                                const int32_t* gt_idx, int E, int64_t* counts, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
    (void)workspace; (void)workspace_bytes;
    SOLA_ARG(bits && pred_off && gt_off && counts, "mask_select_boundary_counts: null argument");
    SOLA_ARG(n_masks >= 0 && T > 0 && E > 0 && h > 0 && w > 0, "mask_select_boundary_counts: bad sizes (n_masks %d, T %d, E %d, %dx%d)",
             n_masks, T, E, h, w);
    SOLA_ARG(radius >= 0 && radius <= BF_MAX_RADIUS, "mask_select_boundary_counts: radius %d outside 0..%d", radius, BF_MAX_RADIUS);
    SOLA_ARG((long long)h * w < (1ll << 31), "mask_select_boundary_counts: image too large");
    SOLA_ARG(words_stride >= sola_jf_plane_words(h, w) && words_stride % 4 == 0,
             "mask_select_boundary_counts: words_stride %lld must be a multiple of 4 and >= %lld", (long long)words_stride,
             (long long)sola_jf_plane_words(h, w));
    SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 15) == 0, "mask_select_boundary_counts: planes must be 16-byte aligned");
    SOLA_ARG((long long)E * T < (1ll << 31), "mask_select_boundary_counts: E*T too large");
    const BfPlan p = bf_plan(h, w, radius);
    SOLA_ARG(p.C >= 1 && p.strips <= 65535, "mask_select_boundary_counts: a %dx%d frame at radius %d does not fit the LDS strips", h, w,
             radius);
    hipStream_t s = as_stream(stream_);
    BfArgs a{};
    a.bits = bits;
    a.stride = words_stride;
    a.M = n_masks; a.T = T; a.h = h; a.w = w; a.r = radius;
    a.cw = p.cw; a.cs = p.cs; a.C = p.C; a.ncols = p.ncols;
    a.pred_off = pred_off; a.pred_idx = pred_idx; a.gt_off = gt_off; a.gt_idx = gt_idx;
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    const long long blocks = (long long)E * T;
    // like sola_mask_select_counts: the plane reads depend on the id lists on the device, only the counts are in the bytes
    SolaProfScope prof(SOLA_PROF_IOU_PACK, s, 0, 32.0 * (double)blocks);
    SOLA_HIP(hipMemsetAsync(counts, 0, (size_t)blocks * 32, s));
    return p.nw == 1 ? bf_launch<1>(a, p, blocks, s) : bf_launch<2>(a, p, blocks, s);
}
