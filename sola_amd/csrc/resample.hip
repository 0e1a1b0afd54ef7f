// Pillow's 8-bit two-pass resize (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
// Vertical_8bpc) and the byte -> float normalisation table behind it, on frames that arrive as uint8: what SAM2's init_state
// (`Image.open(p).convert("RGB").resize((1024, 1024))`, `/ 255.0`, `-= mean`, `/= std`) and GroundingDINO's RandomResize / ToTensor /
// Normalize do to every frame on the host.  Upstream details are from the public sources.
//
// sola_resample_taps / sola_resample_coeffs (host, double): the 22-bit integer coefficients of one axis.  This file is compiled with
//   -ffp-contract=off: a fused multiply-add in the weight arithmetic can move a coefficient by one.
//
// sola_resample_u8: src uint8 [T,H,W,C] (interleaved, any alignment) -> uint8 [T,h,w,C], or with a [C,256] float table the planar
//   float32 [T,C,h,w] = lut[c][byte].  Per pass a 32-bit accumulator starts at 1 << 21, adds pixel * k, is shifted right by 22
//   (arithmetic) and clamped to 0..255; the horizontal result is a BYTE before the vertical pass reads it.  sum |k| <= 1.18 * 2^22 for
//   the two filters, so 255 * sum |k| + 2^21 < 2^31.  A null table is the identity of that axis (Pillow skips the pass): one tap of
//   1 << 22, which the same arithmetic returns unchanged.
//
//   resample_fused_kernel<C, LUT>: one launch per batch.  A block of 512 threads owns RS_TW x RS_TH output pixels of one frame:
//     0. its columns' and rows' bounds and coefficients -> LDS (and the table);
//     1. the source rows y_lo .. y_hi of the columns x_lo .. x_hi it needs -> LDS as bytes, 16-byte loads wherever the ADDRESS is
//        16-byte aligned (a row sits at the same offset mod 16 as its address; the < 16 bytes at either end byte by byte);
//     2. horizontal pass LDS -> LDS, a thread keeps its output column and walks the rows, all C channels on one read of the coefficient;
//        the bytes land PLANAR, mid[c][row][column] (steps 1 and 2 take the rows rows_chunk at a time when a tall window does not
//        fit next to mid[], which holds them all: 1080p -> 1024 x 1024 takes one round, a 3 x reduction a dozen), so that
//     3. the vertical pass reads four neighbouring columns of a channel as one dword per tap, and the table epilogue stores them as
//        one float4 along w (w % 4 == 0 and a 16-byte-aligned output; dword stores otherwise).  uint8 output: a wave per output
//        row, consecutive lanes consecutive bytes.
//     Border rows are computed again by the tile above / below: the rounding is per (row, output column), the bytes are the same.
//     Bounds read from the tables are clamped to what the block staged: tables that are not sola_resample_coeffs' give wrong
//     pixels, never an access outside src, out or the LDS.
//   Geometries whose staging does not fit RS_LDS_BUDGET (very long reductions: rs_plan) take resample_pass_kernel twice - horizontal
//     into a byte intermediate [T,H,w,C] in the caller's scratch, then vertical + epilogue - one thread per output element, taps
//     read from memory; the same arithmetic, hence the same bytes.
// No atomics anywhere: the output bits do not depend on the run or the stream.
// The per-thread steps and the LDS plan live in resample_tile.h as host/device functions: tools/micro/resample_tile_host.hip runs them
// on the host, thread by thread, against Pillow-exact expectations and under AddressSanitizer.
#include <math.h>

#include <algorithm>

#include "kernels.h"
#include "resample_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ coefficients
double rs_bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}
double rs_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
bool rs_filter_ok(int filter) { return filter == SOLA_RESAMPLE_BILINEAR || filter == SOLA_RESAMPLE_BICUBIC; }
double rs_support(int filter) { return filter == SOLA_RESAMPLE_BILINEAR ? 1.0 : 2.0; }
int rs_taps(int in_size, int out_size, int filter) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(rs_support(filter) * fs) * 2 + 1;
}

// ------------------------------------------------------------------------------------------------------------------ kernels
// the steps are resample_tile.h's, one barrier between each
template <int C, bool LUT>
__global__ __launch_bounds__(RS_THREADS) void resample_fused_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
    __shared__ int2 bx[RS_TW], by[RS_TH];
    __shared__ float lut_s[LUT ? C * 256 : 1];
    const int tid = threadIdx.x;
    RsTile s;
    rs_tile_init(s, a, blockIdx.x, reinterpret_cast<uint8_t*>(rs_lds), bx, by, lut_s);
    rs_tile_load_tables<C, LUT>(s, a, tid);
    __syncthreads();
    rs_tile_window<C>(s, a);
    for (int r0 = 0; r0 < s.nrows; r0 += a.rows_chunk) {  // (uniform: every thread read the same bounds)
        const int nr = rs_min(a.rows_chunk, s.nrows - r0);
        rs_tile_stage<C>(s, a, tid, r0, nr);
        __syncthreads();
        rs_tile_horizontal<C>(s, a, tid, r0, nr);
        __syncthreads();
    }
    rs_tile_vertical<C, LUT>(s, a, tid);
}

template <bool VERT>
__global__ __launch_bounds__(256) void resample_pass_kernel(const PassArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < a.total) rs_pass_element<VERT>(a, idx);
}

int rs_check_geometry(const char* who, int T, int H, int W, int C, int h, int w, int taps_x, int taps_y) {
    SOLA_ARG(T >= 0, "%s: negative T %d", who, T);
    SOLA_ARG(C == 1 || C == 3, "%s: C = %d, only 1 (grey) and 3 (RGB) channels", who, C);
    SOLA_ARG(H >= 1 && W >= 1 && h >= 1 && w >= 1, "%s: empty axis (H %d, W %d, h %d, w %d)", who, H, W, h, w);
    SOLA_ARG(H <= SOLA_RESAMPLE_MAX_SIZE && W <= SOLA_RESAMPLE_MAX_SIZE && h <= SOLA_RESAMPLE_MAX_SIZE && w <= SOLA_RESAMPLE_MAX_SIZE,
             "%s: axis beyond %d (H %d, W %d, h %d, w %d)", who, SOLA_RESAMPLE_MAX_SIZE, H, W, h, w);
    SOLA_ARG(taps_x >= 0 && taps_x <= 4 * SOLA_RESAMPLE_MAX_SIZE + 1 && taps_y >= 0 && taps_y <= 4 * SOLA_RESAMPLE_MAX_SIZE + 1,
             "%s: taps_x %d / taps_y %d outside 0 .. %d", who, taps_x, taps_y, 4 * SOLA_RESAMPLE_MAX_SIZE + 1);
    return SOLA_OK;
}

}  // namespace

extern "C" int sola_resample_taps(int in_size, int out_size, int filter) {
    SOLA_ARG(rs_filter_ok(filter), "resample_taps: filter %d is neither %d (bilinear) nor %d (bicubic)", filter, SOLA_RESAMPLE_BILINEAR,
             SOLA_RESAMPLE_BICUBIC);
    SOLA_ARG(in_size >= 1 && out_size >= 1 && in_size <= SOLA_RESAMPLE_MAX_SIZE && out_size <= SOLA_RESAMPLE_MAX_SIZE,
             "resample_taps: sizes %d -> %d outside 1 .. %d", in_size, out_size, SOLA_RESAMPLE_MAX_SIZE);
    return rs_taps(in_size, out_size, filter);
}

extern "C" int sola_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* coeffs) {
    SOLA_ARG(rs_filter_ok(filter), "resample_coeffs: filter %d is neither %d (bilinear) nor %d (bicubic)", filter, SOLA_RESAMPLE_BILINEAR,
             SOLA_RESAMPLE_BICUBIC);
    SOLA_ARG(in_size >= 1 && out_size >= 1 && in_size <= SOLA_RESAMPLE_MAX_SIZE && out_size <= SOLA_RESAMPLE_MAX_SIZE,
             "resample_coeffs: sizes %d -> %d outside 1 .. %d", in_size, out_size, SOLA_RESAMPLE_MAX_SIZE);
    SOLA_ARG(bounds && coeffs, "resample_coeffs: null %s", bounds ? "coeffs" : "bounds");
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = rs_support(filter) * fs;
    const int taps = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    double* w = new double[taps];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            w[x] = filter == SOLA_RESAMPLE_BILINEAR ? rs_bilinear(arg) : rs_bicubic(arg);
            ww += w[x];
        }
        int32_t* k = coeffs + (long long)xx * taps;
        for (int x = 0; x < taps; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << RS_BITS)) : (int32_t)(0.5 + v * (1 << RS_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    delete[] w;
    return SOLA_OK;
}

extern "C" size_t sola_resample_u8_scratch_bytes(int T, int H, int W, int C, int h, int w, int taps_x, int taps_y) {
    if (rs_check_geometry("resample_u8_scratch_bytes", T, H, W, C, h, w, taps_x, taps_y) != SOLA_OK) return 0;
    if (T == 0 || taps_x == 0) return 0;  // no horizontal pass: nothing in between
    if (rs_plan(H, W, C, h, w, taps_x, std::max(taps_y, 1), false, taps_y == 0).fused) return 0;
    return ((size_t)T * H * w * C + 255) / 256 * 256;
}

extern "C" int sola_resample_u8(const uint8_t* src, int T, int H, int W, int C, int h, int w, const int32_t* table_x, int taps_x,
                                const int32_t* table_y, int taps_y, const float* lut, void* out, void* scratch, size_t scratch_bytes,
                                void* stream_) {
    SOLA_TRY(rs_check_geometry("resample_u8", T, H, W, C, h, w, taps_x, taps_y));
    SOLA_ARG((table_x != nullptr) == (taps_x > 0) && (table_y != nullptr) == (taps_y > 0),
             "resample_u8: a table and its taps go together (taps_x %d, taps_y %d; 0 taps = null table = the axis keeps its size)", taps_x, taps_y);
    SOLA_ARG(table_x || w == W, "resample_u8: null table_x but w %d != W %d", w, W);
    SOLA_ARG(table_y || h == H, "resample_u8: null table_y but h %d != H %d", h, H);
    SOLA_ARG(((reinterpret_cast<uintptr_t>(table_x) | reinterpret_cast<uintptr_t>(table_y) | reinterpret_cast<uintptr_t>(lut)) & 3) == 0,
             "resample_u8: tables must be 4-byte aligned");
    if (T == 0) return SOLA_OK;
    SOLA_ARG(src, "resample_u8: null src");
    SOLA_ARG(out, "resample_u8: null out");
    if (lut) SOLA_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "resample_u8: a float32 output must be 4-byte aligned");
    hipStream_t s = as_stream(stream_);
    const RsPlan p = rs_plan(H, W, C, h, w, std::max(taps_x, 1), std::max(taps_y, 1), !table_x, !table_y);
    if (p.fused) {
        const ResampleArgs a = rs_fused_args(p, src, T, H, W, h, w, table_x, taps_x, table_y, taps_y, lut, out);
        const long long blocks = (long long)a.tiles_x * a.tiles_y * T;
        SOLA_ARG(blocks < (1ll << 31), "resample_u8: %lld tiles, at most 2^31 - 1 in one call", blocks);
        const dim3 grid((unsigned)blocks), block(RS_THREADS);
        if (C == 1 && lut) hipLaunchKernelGGL((resample_fused_kernel<1, true>), grid, block, p.lds, s, a);
        else if (C == 1) hipLaunchKernelGGL((resample_fused_kernel<1, false>), grid, block, p.lds, s, a);
        else if (lut) hipLaunchKernelGGL((resample_fused_kernel<3, true>), grid, block, p.lds, s, a);
        else hipLaunchKernelGGL((resample_fused_kernel<3, false>), grid, block, p.lds, s, a);
        SOLA_LAUNCH_CHECK();
        return SOLA_OK;
    }
    const long long mid_total = (long long)T * H * w * C, out_total = (long long)T * h * w * C;
    SOLA_ARG(std::max(mid_total, out_total) < (1ll << 39), "resample_u8: %lld elements in one call of the two-launch route, at most 2^39 - 1",
             std::max(mid_total, out_total));
    const uint8_t* from = src;
    if (table_x) {
        SOLA_ARG(scratch && scratch_bytes >= (size_t)mid_total, "resample_u8: scratch of %zu bytes, sola_resample_u8_scratch_bytes asks for %zu",
                 scratch ? scratch_bytes : (size_t)0, sola_resample_u8_scratch_bytes(T, H, W, C, h, w, taps_x, taps_y));
        PassArgs a{src, table_x, nullptr, scratch, mid_total, H, W, C, w, taps_x};
        hipLaunchKernelGGL(resample_pass_kernel<false>, dim3((unsigned)((mid_total + 255) / 256)), dim3(256), 0, s, a);
        SOLA_LAUNCH_CHECK();
        from = reinterpret_cast<const uint8_t*>(scratch);
    }
    PassArgs a{from, table_y, lut, out, out_total, H, w, C, h, std::max(taps_y, 1)};
    hipLaunchKernelGGL(resample_pass_kernel<true>, dim3((unsigned)((out_total + 255) / 256)), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
