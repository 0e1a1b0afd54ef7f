// Column-major bit planes (jf.hip: bit x*h + y, what sola_rle_pack_cm and sola_index_pack decode into) -> the row-major planes of
// sola_mask_pack (iou.hip: bit y*w + x), so that masklets decoded once per video also feed the kernels that read row-major bits:
// the PNG writer's selection front-end (png_bitmap_select_kernel, png_encode.hip) and the IoU kernels, without a uint8 stage.
//
//   planes_cm_to_rm_kernel   a bit-matrix transpose.  One workgroup per (up to 64 image rows, plane).  Each lane of a wave loads the
//                            workgroup's rows of ONE column as a single piece of at most 64 bits (columns start at arbitrary bit
//                            offsets: two 8-byte loads and a funnel shift, png_select.h), 64 ballots turn the wave's 64 columns into 64
//                            row words, and the rows are kept in LDS.  The workgroup then writes the output words whose first bit lies
//                            in its rows: every word has one writer (no atomics, no memset), tail and pad words are written as zero
//                            by the plane's last workgroup.  A word that reaches past the workgroup's last row takes those at most 31
//                            bits from the source plane directly.
#include <algorithm>

#include "kernels.h"
#include "png_select.h"

namespace {

constexpr int CMRM_LDS_BUDGET = 48 * 1024;  // three workgroups in a CU's LDS; rows per workgroup shrink for very wide images

__global__ __launch_bounds__(256) void planes_cm_to_rm_kernel(const ps_u64* __restrict__ cm, long long nq_cm, long long plane0, int h,
                                                              int w, int rows, int pitch64, uint32_t* __restrict__ rm,
                                                              long long stride_rm) {
    extern __shared__ ps_u64 tile[];  // [rows][pitch64]: bit x of row r
    const long long p = plane0 + blockIdx.y;
    const ps_u64* src = cm + p * nq_cm;
    uint32_t* dst = rm + p * stride_rm;
    const int y0 = (int)blockIdx.x * rows, y1 = min(y0 + rows, h), ry = y1 - y0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nxt = (w + 63) >> 6;
    for (int xt = wave; xt < nxt; xt += 4) {
        const int x = xt * 64 + lane;
        const ps_u64 col = x < w ? ps_column(src, nq_cm, x, h, y0, ry) : 0ull;
        ps_u64 mine = 0;
        for (int r = 0; r < ry; ++r) {  // (uniform: ry and r are the wave's)
            const ps_u64 b = __ballot((int)((col >> r) & 1ull));
            if (lane == r) mine = b;
        }
        if (lane < ry) tile[lane * pitch64 + xt] = mine;
    }
    __syncthreads();
    const long long w0 = ps_first_word(y0, w), w1 = ps_first_word(y1, w);
    for (long long i = w0 + threadIdx.x; i < w1; i += 256) {
        uint32_t v = ps_rm_word(tile, pitch64, i, w, y0, y1);
        if (i == w1 - 1 && y1 < h) v |= ps_rm_rest(src, nq_cm, i, w, h, y1);
        dst[i] = v;
    }
    if (y1 == h)
        for (long long i = w1 + threadIdx.x; i < stride_rm; i += 256) dst[i] = 0u;
}

}  // namespace

extern "C" int sola_planes_cm_to_rm(const uint32_t* bits_cm, int64_t words_stride_cm, int64_t n_planes, int h, int w, uint32_t* bits_rm,
                                    int64_t words_stride_rm, void* stream_) {
    SOLA_ARG(bits_cm && bits_rm, "planes_cm_to_rm: null argument");
    SOLA_ARG(n_planes > 0 && h > 0 && w > 0, "planes_cm_to_rm: bad sizes (n_planes %lld, h %d, w %d)", (long long)n_planes, h, w);
    SOLA_ARG((long long)h * w < (1ll << 31), "planes_cm_to_rm: image too large (h*w must be < 2^31)");
    SOLA_ARG(words_stride_cm >= sola_jf_plane_words(h, w) && words_stride_cm % 4 == 0,
             "planes_cm_to_rm: words_stride_cm %lld must be a multiple of 4 and >= %lld", (long long)words_stride_cm,
             (long long)sola_jf_plane_words(h, w));
    SOLA_ARG(words_stride_rm >= sola_mask_words(h, w) && words_stride_rm % 4 == 0,
             "planes_cm_to_rm: words_stride_rm %lld must be a multiple of 4 and >= %lld", (long long)words_stride_rm,
             (long long)sola_mask_words(h, w));
    SOLA_ARG(((reinterpret_cast<uintptr_t>(bits_cm) | reinterpret_cast<uintptr_t>(bits_rm)) & 15) == 0,
             "planes_cm_to_rm: planes must be 16-byte aligned");
    const int pitch64 = (int)((((long long)w + 63) >> 6) | 1);  // odd: the lanes of a wave store one word of 64 different rows
    const int rows = std::min(PS_ROWS, CMRM_LDS_BUDGET / (pitch64 * 8));
    SOLA_ARG(rows >= 1, "planes_cm_to_rm: image too large (a row of %d pixels does not fit the LDS)", w);
    hipStream_t s = as_stream(stream_);
    const unsigned gx = (unsigned)((h + rows - 1) / rows);
    const size_t lds = (size_t)rows * pitch64 * 8;
    for (int64_t p0 = 0; p0 < n_planes; p0 += 65535) {  // gridDim.y <= 65535
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n_planes - p0);
        hipLaunchKernelGGL(planes_cm_to_rm_kernel, dim3(gx, gy), dim3(256), lds, s, reinterpret_cast<const ps_u64*>(bits_cm),
                           (long long)(words_stride_cm / 2), (long long)p0, h, w, rows, pitch64, bits_rm, (long long)words_stride_rm);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}
