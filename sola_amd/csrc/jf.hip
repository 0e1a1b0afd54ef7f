// Mask-level J&F of the evaluator (evaluator.py:174-247 with dataloader.py:251-369 feeding it) on one packed layout.
//
// Column-major bit planes: bit j of word i of a plane is the pixel at COCO position 32*i + j, position = x*h + y (the
// order of the run-length strings themselves).  A plane is `words_stride` words long, a multiple of 4, so every plane
// starts on 16 bytes and the counting kernel reads whole uint4s without a predicate; tail and pad bits are zero.  J and F
// are pixel counts, so the order of the pixels does not matter as long as both sides of a count use the same one.  This
// layout belongs to the J&F path alone: the row-major planes of mask_pack / mask_pair_counts (iou.hip) are a different one.
//
//   rle_pack_cm_kernel         COCO runs -> planes, one thread per output word: one upper-bound search in the mask's prefix
//                              sums at 32*i (its parity is the value there, rle_value() of masklet.hip), then a walk over
//                              the run ends inside the word.  One search per 32 pixels where rle_fill_or_kernel does one per
//                              pixel.  Runs that cover fewer than h*w pixels follow rle_fill_or_kernel's parity rule.
//   mask_nested_counts_kernel<NL>  one block per (expression e, frame t) for up to NL nested selections at once: e's candidate
//                              list is ordered so that the selection of level k is a prefix of it.  OR of e's GT planes into g once
//                              per quad (16 bytes per lane and load); p is carried over the levels in registers, each level ORs in
//                              only the planes that enter there, then adds popc(p & g), popc(p) to that level's per-lane counters;
//                              popc(g) once.  Reduced over the block and stored as int64 counts[e, k, t, 0..2]: no atomics, no
//                              memset, order-independent.  <1> is the plain selection of sola_mask_select_counts (one level that
//                              ends at the list's end), <SOLA_NESTED_MAX_LEVELS> the sweep (2*16 + 1 VGPRs of counters, the level
//                              loop unrolled to the compile-time bound): every plane of the largest selection and of the GT list
//                              is read once per (e, t), whatever the number of levels.
//   sola_rle_strings_to_cum_batch  host: every compressed string of a video -> prefix sums + run offsets in one call, with
//                              the parser of sola_rle_string_to_cum (api.hip).
#include <string.h>

#include <algorithm>

#include "kernels.h"

namespace {

__device__ __forceinline__ uint32_t bit_range(uint32_t a, uint32_t b) {  // bits a..b-1, 0 <= a <= b <= 32
    return (uint32_t)((1ull << b) - (1ull << a));
}

__global__ __launch_bounds__(256) void rle_pack_cm_kernel(const uint32_t* __restrict__ cum, const long long* __restrict__ off,
                                                          long long plane0, uint32_t hw, long long stride,
                                                          uint32_t* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // word of the plane
    if (i >= stride) return;
    const long long p = plane0 + blockIdx.y;
    uint32_t word = 0;
    const long long pos0 = i * 32;
    if (pos0 < (long long)hw) {
        const long long first = off[p], last = off[p + 1];  // an empty range is an absent frame: all zeros
        long long lo = first, hi = last;
        while (lo < hi) {  // first run end > pos0
            const long long mid = (lo + hi) >> 1;
            if ((long long)cum[mid] <= pos0) lo = mid + 1; else hi = mid;
        }
        uint32_t v = (uint32_t)((lo - first) & 1);
        const uint32_t span = (uint32_t)min(32ll, (long long)hw - pos0);
        uint32_t cur = 0;
        for (long long k = lo; k < last; ++k) {  // run ends inside the word (zero-length runs toggle twice at one place)
            const uint32_t e = (uint32_t)((long long)cum[k] - pos0);
            if (e >= span) break;
            if (v) word |= bit_range(cur, e);
            cur = e;
            v ^= 1u;
        }
        if (v) word |= bit_range(cur, span);
    }
    bits[p * stride + i] = word;
}

// One block per (expression e, frame t) for levels k0 .. k0 + nl - 1 of the K prefix ends of e's ordered list (nl <= NL): the first
// level of the launch ORs the whole prefix [0, end(e, k0)), the later ones what enters with them.  end(e, k) = min(max(level_end[e, k],
// end(e, k - 1)), len_e) is formed here, so a decreasing or too-long entry reads nothing outside e's list; a null level_end ends
// every level at len_e.  NL = 1 is the plain selection (sola_mask_select_counts), NL = SOLA_NESTED_MAX_LEVELS the sweep.  All list
// and level reads are block-uniform (scalar loads); the counters are indexed by unrolled constants only, so they stay in VGPRs.
template <int NL>
__global__ __launch_bounds__(256) void mask_nested_counts_kernel(const uint4* __restrict__ planes, long long quads, int M, int T,
                                                                 const int* __restrict__ pred_off, const int* __restrict__ pred_idx,
                                                                 const int* __restrict__ level_end, int K, int k0, int nl,
                                                                 const int* __restrict__ gt_off, const int* __restrict__ gt_idx,
                                                                 long long* __restrict__ counts) {
    __shared__ unsigned red[4][2 * NL + 1];
    const long long b = blockIdx.x;
    const int e = (int)(b / T), t = (int)(b - (long long)e * T);
    const int p0 = pred_off[e], len = max(pred_off[e + 1] - p0, 0), g0 = gt_off[e], g1 = gt_off[e + 1];
    const int* le = level_end + (long long)e * K;
    int prev = level_end ? 0 : len;
    for (int k = 0; level_end && k < k0; ++k) prev = min(max(le[k], prev), len);
    int ends[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (level_end && l < nl) prev = min(max(le[k0 + l], prev), len);
        ends[l] = p0 + prev;
    }
    unsigned ci[NL], cp[NL], cg = 0;  // per lane at most 128 * ceil(quads / 256) < 2^24 pixels
#pragma unroll
    for (int l = 0; l < NL; ++l) ci[l] = cp[l] = 0;
    for (long long q = threadIdx.x; q < quads; q += 256) {
        uint4 p = make_uint4(0, 0, 0, 0), g = make_uint4(0, 0, 0, 0);
#pragma unroll 4
        for (int k = g0; k < g1; ++k) {
            const int m = gt_idx[k];
            if ((unsigned)m >= (unsigned)M) continue;
            const uint4 v = planes[((long long)m * T + t) * quads + q];
            g.x |= v.x; g.y |= v.y; g.z |= v.z; g.w |= v.w;
        }
        cg += __popc(g.x) + __popc(g.y) + __popc(g.z) + __popc(g.w);
        int k = p0;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l < nl) {
#pragma unroll NL == 1 ? 4 : 1  // (more would spill SGPRs in the 16-level instance)
                for (; k < ends[l]; ++k) {
                    const int m = pred_idx[k];
                    if ((unsigned)m >= (unsigned)M) continue;
                    const uint4 v = planes[((long long)m * T + t) * quads + q];
                    p.x |= v.x; p.y |= v.y; p.z |= v.z; p.w |= v.w;
                }
                ci[l] += __popc(p.x & g.x) + __popc(p.y & g.y) + __popc(p.z & g.z) + __popc(p.w & g.w);
                cp[l] += __popc(p.x) + __popc(p.y) + __popc(p.z) + __popc(p.w);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            ci[l] += __shfl_xor(ci[l], o, 64);
            cp[l] += __shfl_xor(cp[l], o, 64);
        }
        cg += __shfl_xor(cg, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            red[wave][2 * l] = ci[l];
            red[wave][2 * l + 1] = cp[l];
        }
        red[wave][2 * NL] = cg;
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * nl) {  // one thread per entry of counts[e, k0 .. k0 + nl, t, 0..2]
        const int l = threadIdx.x / 3, c = threadIdx.x - 3 * l;
        const int j = c == 2 ? 2 * NL : 2 * l + c;
        counts[(((long long)e * K + k0 + l) * T + t) * 3 + c] =
            (long long)red[0][j] + (long long)red[1][j] + (long long)red[2][j] + (long long)red[3][j];
    }
}

}  // namespace

extern "C" int64_t sola_jf_plane_words(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    return (((int64_t)h * w + 31) / 32 + 3) & ~(int64_t)3;
}

extern "C" int sola_rle_pack_cm(const uint32_t* cum, const int64_t* off, int64_t n_planes, int h, int w, int64_t words_stride,
                                uint32_t* bits, void* stream_) {
    SOLA_ARG(cum && off && bits, "rle_pack_cm: null argument");
    SOLA_ARG(n_planes > 0 && h > 0 && w > 0, "rle_pack_cm: bad sizes");
    SOLA_ARG((long long)h * w < (1ll << 31), "rle_pack_cm: image too large");
    SOLA_ARG(words_stride >= sola_jf_plane_words(h, w) && words_stride % 4 == 0,
             "rle_pack_cm: words_stride %lld must be a multiple of 4 and >= %lld", (long long)words_stride,
             (long long)sola_jf_plane_words(h, w));
    SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 15) == 0, "rle_pack_cm: planes must be 16-byte aligned");
    hipStream_t s = as_stream(stream_);
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    const unsigned gx = (unsigned)((words_stride + 255) / 256);
    SolaProfScope prof(SOLA_PROF_IOU_PACK, s, 0, 4.0 * (double)n_planes * words_stride + 8.0 * (double)(n_planes + 1));
    for (int64_t p0 = 0; p0 < n_planes; p0 += 65535) {  // gridDim.y <= 65535
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n_planes - p0);
        hipLaunchKernelGGL(rle_pack_cm_kernel, dim3(gx, gy), dim3(256), 0, s, cum, reinterpret_cast<const long long*>(off),
                           (long long)p0, hw, (long long)words_stride, bits);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}

// The checks sola_mask_select_counts and sola_mask_nested_counts share (`who` is the name in front of the message), then the launches:
// one level (a null level_end included) runs the <1> instance, more levels the <SOLA_NESTED_MAX_LEVELS> one in chunks of 16.
static int nested_counts_launch(const char* who, const uint32_t* bits, int64_t words_stride, int n_masks, int T, const int32_t* pred_off,
                                const int32_t* pred_idx, const int32_t* level_end, int K, const int32_t* gt_off, const int32_t* gt_idx,
                                int E, int64_t* counts, void* stream_) {
    SOLA_ARG(words_stride < (1ll << 26), "%s: planes too large", who);
    SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 15) == 0, "%s: planes must be 16-byte aligned", who);
    SOLA_ARG((long long)E * T < (1ll << 31), "%s: E*T too large", who);
    hipStream_t s = as_stream(stream_);
    // the plane reads depend on the id lists, which live on the device: only the counts are in the profile's bytes
    SolaProfScope prof(SOLA_PROF_IOU_PACK, s, 0, 24.0 * (double)E * K * T);
    const auto kernel = K == 1 ? mask_nested_counts_kernel<1> : mask_nested_counts_kernel<SOLA_NESTED_MAX_LEVELS>;
    for (int k0 = 0; k0 < K; k0 += SOLA_NESTED_MAX_LEVELS) {  // a launch per 16 levels; its first level ORs the whole prefix again
        hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)E * T)), dim3(256), 0, s, reinterpret_cast<const uint4*>(bits),
                           (long long)(words_stride / 4), n_masks, T, pred_off, pred_idx, level_end, K, k0,
                           std::min(SOLA_NESTED_MAX_LEVELS, K - k0), gt_off, gt_idx, reinterpret_cast<long long*>(counts));
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}

extern "C" int sola_mask_select_counts(const uint32_t* bits, int64_t words_stride, int n_masks, int T, const int32_t* pred_off,
                                       const int32_t* pred_idx, const int32_t* gt_off, const int32_t* gt_idx, int E,
                                       int64_t* counts, void* stream_) {
    SOLA_ARG(bits && pred_off && gt_off && counts, "mask_select_counts: null argument");  // (null index lists: every list is empty)
    SOLA_ARG(n_masks >= 0 && T > 0 && E > 0, "mask_select_counts: bad sizes (n_masks %d, T %d, E %d)", n_masks, T, E);
    SOLA_ARG(words_stride > 0 && words_stride % 4 == 0, "mask_select_counts: words_stride %lld is not a multiple of 4",
             (long long)words_stride);
    return nested_counts_launch("mask_select_counts", bits, words_stride, n_masks, T, pred_off, pred_idx, nullptr, 1, gt_off, gt_idx, E,
                                counts, stream_);
}

extern "C" int sola_mask_nested_counts(const uint32_t* bits, int64_t words_stride, int n_masks, int T, const int32_t* pred_off,
                                       const int32_t* pred_idx, const int32_t* level_end, int K, const int32_t* gt_off,
                                       const int32_t* gt_idx, int E, int64_t* counts, void* stream_) {
    SOLA_ARG(bits && pred_off && pred_idx && level_end && gt_off && gt_idx && counts, "mask_nested_counts: null argument");
    SOLA_ARG(K > 0 && T > 0 && E > 0 && n_masks >= 0, "mask_nested_counts: bad sizes (n_masks %d, T %d, E %d, K %d)", n_masks, T, E, K);
    SOLA_ARG(words_stride > 0 && words_stride % 4 == 0, "mask_nested_counts: words_stride %lld is not a positive multiple of 4",
             (long long)words_stride);
    return nested_counts_launch("mask_nested_counts", bits, words_stride, n_masks, T, pred_off, pred_idx, level_end, K, gt_off, gt_idx, E,
                                counts, stream_);
}

extern "C" int64_t sola_rle_strings_to_cum_batch(const char* chars, const int64_t* str_off, int64_t n, uint32_t* cum, int64_t cap,
                                                 int64_t limit, int64_t* run_off) {
    if (!chars || !str_off || !cum || !run_off || n < 0 || cap < 0) {
        sola_set_error("rle_strings_to_cum_batch: bad arguments");
        return SOLA_ERR_ARG;
    }
    run_off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = str_off[i + 1] - str_off[i];
        if (str_off[i] < 0 || len < 0) {
            sola_set_error("rle_strings_to_cum_batch: string %lld has a negative length", (long long)i);
            return SOLA_ERR_ARG;
        }
        const int64_t r = sola_rle_string_to_cum(chars + str_off[i], len, cum + run_off[i], cap - run_off[i], limit);
        if (r < 0) {
            char why[256];
            strncpy(why, sola_last_error(), sizeof(why) - 1);
            why[sizeof(why) - 1] = 0;
            sola_set_error("rle_strings_to_cum_batch: string %lld: %s", (long long)i, why);
            return r;
        }
        run_off[i + 1] = run_off[i] + r;
    }
    return run_off[n];
}
