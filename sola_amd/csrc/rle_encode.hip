// Masks -> COCO compressed run-length strings on the GPU: the write side of the masklet rows (the reference's
// seg_utils.encode_rle_masklet_torch = pycocotools rleEncode + rleToString per frame, after a copy of the whole masklet to
// the host).  Byte-identical to pycocotools on {0,1} masks.
//
// Runs are taken over the column-major flattening p = x*h + y and alternate 0,1,0,... starting with zeros.  A frame's
// transition positions (v(p) != v(p-1), v(-1) = 0) followed by h*w are the inclusive prefix sums of its run lengths, the
// `cum` form rle_fill_or_kernel (masklet.hip) decodes.  Three phases on the caller's stream; kernel boundaries separate
// them, no workgroup hands data to another inside a launch:
//   1. count (launch_rle_encode_runs)  rle_rows_kernel<.., EMIT=false> reads the masks once, lanes along x with 16-byte
//      loads where the rows allow it (16 uint8 or 4 float32 columns per lane); a lane walks down a band of RLE_BAND rows
//      holding the row above as bits and counts the transitions of each of its columns: one count per (frame, column,
//      band), which are the frame's segments in column-major order.  The predecessor of (0,x) is (h-1,x-1), read once
//      per lane.  rle_seg_scan_kernel turns a frame's counts into exclusive offsets in place and writes its run count
//      (transitions + 1); rle_frame_scan_kernel scans the run counts into dev_run_off.
//   2. emit (launch_rle_encode_cum)  the same walk re-reads the masks and stores each transition's position at its
//      segment's offset in dev_cum; h*w ends each frame.  rle_char_count_kernel sums the characters of each run (local:
//      they depend on cum[i-3..i]) per frame, and the frame scan turns the sums into dev_char_off.
//   3. chars (launch_rle_encode_chars)  per frame, each run's characters are counted again, block-scanned and written at
//      their offsets.  Depends on cum alone, so it encodes a cum from the decoder side as well.
// Re-reading the masks in phase 2 (rather than a transition bitmap written in phase 1) keeps phase 1 a pure read; the
// measured phase times are in DESIGN.md.
#include <algorithm>

#include "kernels.h"
#include "mask_elems.h"

namespace {

constexpr int RLE_BAND = 64;            // rows per lane in the count / emit walk
constexpr int RLE_FRAMES = 65535;       // frames per launch (grid.y); larger n is chunked
constexpr int RLE_SCAN_ITEMS = 8;       // per thread and block iteration of the scans (256 threads)
constexpr int RLE_CHAR_ITEMS = 4;       // runs per thread and block iteration of the character kernels

struct RowsArgs {
    const void* masks;
    uint32_t* seg;              // [n, w*B]: counts (phase 1), exclusive offsets within the frame (after rle_seg_scan_kernel)
    const long long* run_off;   // [n+1] (emit)
    uint32_t* cum;              // (emit)
    int h, w, B, ncv;           // B bands per column, ncv lane columns (groups of VEC) per row
    int frame0;
};

// VEC consecutive pixels of one row -> bit c = pixel c is set
template <int KIND, int VEC>
__device__ __forceinline__ uint32_t load_bits(const typename mask_elem<KIND>::type* p) {
    if constexpr (VEC * mask_elem<KIND>::size == 16) {
        return vec_bits<KIND>(*reinterpret_cast<const typename mask_elem<KIND>::vec*>(p));
    } else if constexpr (KIND == MASK_U8 && VEC == 4) {
        return nz_byte_bits(*reinterpret_cast<const uint32_t*>(p));
    } else {
        static_assert(VEC == 1, "unsupported vector width");
        return mask_is_set<KIND>(*p);
    }
}

// One lane = VEC columns x0.. of one band of one frame.  EMIT=false: write the band's transition count of each column to
// seg; EMIT=true: write the transitions' positions into cum at the offsets seg now holds.
template <int KIND, int VEC, bool EMIT>
__global__ __launch_bounds__(256) void rle_rows_kernel(const RowsArgs a) {
    using T = typename mask_elem<KIND>::type;
    const int f = a.frame0 + blockIdx.y;
    const long long S = (long long)a.w * a.B;
    if (EMIT && blockIdx.x == 0 && threadIdx.x == 0) a.cum[a.run_off[f + 1] - 1] = (uint32_t)a.h * (uint32_t)a.w;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.ncv * a.B) return;
    const int b = t / a.ncv, x0 = (t - b * a.ncv) * VEC;
    const int y0 = b * RLE_BAND, y1 = min(a.h, y0 + RLE_BAND);
    const T* img = reinterpret_cast<const T*>(a.masks) + (long long)f * a.h * a.w + x0;
    uint32_t prev;
    if (y0 > 0) {
        prev = load_bits<KIND, VEC>(img + (long long)(y0 - 1) * a.w);
    } else {  // column x0+c follows (h-1, x0+c-1); column 0 follows the implicit 0
        const T* last = img + (long long)(a.h - 1) * a.w;
        prev = (load_bits<KIND, VEC>(last) << 1) & ((1u << VEC) - 1u);
        if (x0 > 0) prev |= mask_is_set<KIND>(last[-1]);
    }
    uint32_t* seg = a.seg + (long long)f * S + (long long)x0 * a.B + b;  // column x0+c: seg[c * B]
    uint32_t cnt[VEC];
    uint32_t* cum = nullptr;
    uint32_t lim = 0;  // the frame's transitions: masks that changed since phase 1 give wrong strings, never a stray store
    if constexpr (EMIT) {
        cum = a.cum + a.run_off[f];
        lim = (uint32_t)(a.run_off[f + 1] - a.run_off[f] - 1);
#pragma unroll
        for (int c = 0; c < VEC; ++c) cnt[c] = seg[(long long)c * a.B];
    } else {
#pragma unroll
        for (int c = 0; c < VEC; ++c) cnt[c] = 0;
    }
    const T* row = img + (long long)y0 * a.w;
    int y = y0;
    for (; y + 4 <= y1; y += 4, row += 4 * (long long)a.w) {  // four rows' loads in flight per lane
        uint32_t m[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = load_bits<KIND, VEC>(row + (long long)r * a.w);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t tr = m[r] ^ prev;
            prev = m[r];
            if constexpr (EMIT) {
                if (tr) {
#pragma unroll
                    for (int c = 0; c < VEC; ++c)
                        if (((tr >> c) & 1u) && cnt[c] < lim) cum[cnt[c]++] = (uint32_t)(x0 + c) * (uint32_t)a.h + (uint32_t)(y + r);
                }
            } else {
#pragma unroll
                for (int c = 0; c < VEC; ++c) cnt[c] += (tr >> c) & 1u;
            }
        }
    }
    for (; y < y1; ++y, row += a.w) {
        const uint32_t m = load_bits<KIND, VEC>(row);
        const uint32_t tr = m ^ prev;
        prev = m;
        if constexpr (EMIT) {
            if (tr) {
#pragma unroll
                for (int c = 0; c < VEC; ++c)
                    if (((tr >> c) & 1u) && cnt[c] < lim) cum[cnt[c]++] = (uint32_t)(x0 + c) * (uint32_t)a.h + (uint32_t)y;
            }
        } else {
#pragma unroll
            for (int c = 0; c < VEC; ++c) cnt[c] += (tr >> c) & 1u;
        }
    }
    if constexpr (!EMIT) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) seg[(long long)c * a.B] = cnt[c];
    }
}

// Exclusive scan over the 256 threads of the block; `total` = the block's sum.  Ends on a barrier, so `lds` may be reused.
template <typename V>
__device__ __forceinline__ V block_exclusive_scan(V v, V* lds, V& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    V before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const V s = lds[i];
        if (i < wave) before += s;
        total += s;
    }
    __syncthreads();
    return before + inc - v;
}

// One block per frame: the frame's segment counts -> exclusive offsets (in place); run_off[f+1] = transitions + 1.
__global__ __launch_bounds__(256) void rle_seg_scan_kernel(uint32_t* seg, long long S, long long* run_off, int frame0) {
    __shared__ uint32_t lds[4];
    const int f = frame0 + blockIdx.x;
    uint32_t* s = seg + (long long)f * S;
    uint32_t carry = 0;
    for (long long base = 0; base < S; base += 256 * RLE_SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * RLE_SCAN_ITEMS;
        uint32_t v[RLE_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int i = 0; i < RLE_SCAN_ITEMS; ++i) {
            v[i] = i0 + i < S ? s[i0 + i] : 0u;
            sum += v[i];
        }
        uint32_t total;
        uint32_t run = carry + block_exclusive_scan<uint32_t>(sum, lds, total);
#pragma unroll
        for (int i = 0; i < RLE_SCAN_ITEMS; ++i) {
            if (i0 + i < S) s[i0 + i] = run;
            run += v[i];
        }
        carry += total;
    }
    if (threadIdx.x == 0) run_off[f + 1] = (long long)carry + 1;
}

// One block: off[1..n] (per-frame sizes) -> inclusive prefix sums, off[0] = 0.
__global__ __launch_bounds__(256) void rle_frame_scan_kernel(long long* off, int n) {
    __shared__ long long lds[4];
    long long carry = 0;
    for (long long base = 0; base < n; base += 256 * RLE_SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * RLE_SCAN_ITEMS;
        long long v[RLE_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int i = 0; i < RLE_SCAN_ITEMS; ++i) {
            v[i] = i0 + i < n ? off[1 + i0 + i] : 0ll;
            sum += v[i];
        }
        long long total;
        long long run = carry + block_exclusive_scan<long long>(sum, lds, total);
#pragma unroll
        for (int i = 0; i < RLE_SCAN_ITEMS; ++i) {
            run += v[i];
            if (i0 + i < n) off[1 + i0 + i] = run;
        }
        carry += total;
    }
    if (threadIdx.x == 0) off[0] = 0;
}

// The value rleToString encodes for run i of a frame (cum = the frame's inclusive prefix sums): its length, or from the
// 4th run on the difference to the run two places back.
__device__ __forceinline__ long long run_delta(const uint32_t* __restrict__ cum, long long i) {
    const long long r = (long long)cum[i] - (i ? (long long)cum[i - 1] : 0ll);
    if (i < 3) return r;
    return r - ((long long)cum[i - 2] - (long long)cum[i - 3]);
}

// Characters of one value: 5-bit groups, least significant first, until the rest is the sign extension of the last group.
__device__ __forceinline__ int delta_chars(long long x) {
    int k = 0;
    bool more = true;
    while (more) {
        const long long c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++k;
    }
    return k;
}

// One block per frame: char_off[f+1] = characters of the frame's string.
__global__ __launch_bounds__(256) void rle_char_count_kernel(const uint32_t* __restrict__ cum, const long long* __restrict__ run_off,
                                                             long long* char_off, int frame0) {
    __shared__ long long lds[4];
    const int f = frame0 + blockIdx.x;
    const long long lo = run_off[f], R = run_off[f + 1] - lo;
    long long sum = 0;
    for (long long i = threadIdx.x; i < R; i += 256) sum += delta_chars(run_delta(cum + lo, i));
    long long total;
    block_exclusive_scan<long long>(sum, lds, total);
    if (threadIdx.x == 0) char_off[f + 1] = total;
}

// One block per frame: each thread takes RLE_CHAR_ITEMS consecutive runs per iteration, counts their characters, and
// writes them at the block-scanned offsets.
__global__ __launch_bounds__(256) void rle_chars_kernel(const uint32_t* __restrict__ cum, const long long* __restrict__ run_off,
                                                        const long long* __restrict__ char_off, char* __restrict__ chars, int frame0) {
    __shared__ long long lds[4];
    const int f = frame0 + blockIdx.x;
    const long long lo = run_off[f], R = run_off[f + 1] - lo;
    const uint32_t* c = cum + lo;
    char* out = chars + char_off[f];
    const char* end = chars + char_off[f + 1];  // offsets that do not match cum give wrong strings, never a stray store
    for (long long base = 0; base < R; base += 256 * RLE_CHAR_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * RLE_CHAR_ITEMS;
        long long x[RLE_CHAR_ITEMS];
        int k[RLE_CHAR_ITEMS];
        long long sum = 0;
#pragma unroll
        for (int i = 0; i < RLE_CHAR_ITEMS; ++i) {
            x[i] = i0 + i < R ? run_delta(c, i0 + i) : 0ll;
            k[i] = i0 + i < R ? delta_chars(x[i]) : 0;
            sum += k[i];
        }
        long long total;
        char* o = out + block_exclusive_scan<long long>(sum, lds, total);
#pragma unroll
        for (int i = 0; i < RLE_CHAR_ITEMS; ++i) {
            long long v = x[i];
            for (int j = 0; j < k[i]; ++j) {
                const int ch = (int)(v & 0x1f);
                v >>= 5;
                if (o < end) *o = (char)(48 + (ch | (j + 1 < k[i] ? 0x20 : 0)));
                ++o;
            }
        }
        out += total;
    }
}

// Lane width of the row walk: 16-byte loads when every row start is 16-byte aligned, else 4-byte (uint8), else scalar.
int rows_vec(const void* masks, int elem_type, int w) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(masks);
    if (elem_type == 0) return (w % 16 == 0 && p % 16 == 0) ? 16 : (w % 4 == 0 && p % 4 == 0) ? 4 : 1;
    return (w % 4 == 0 && p % 16 == 0) ? 4 : 1;
}

template <bool EMIT>
int launch_rows(const RowsArgs& base, int elem_type, int n, hipStream_t s) {
    const int vec = rows_vec(base.masks, elem_type, base.w);
    RowsArgs a = base;
    a.ncv = a.w / vec;
    const unsigned gx = (unsigned)(((long long)a.ncv * a.B + 255) / 256);
    for (int f0 = 0; f0 < n; f0 += RLE_FRAMES) {
        a.frame0 = f0;
        const dim3 grid(gx, (unsigned)std::min(RLE_FRAMES, n - f0)), block(256);
        with_mask_kind<MASK_LOGIT>(elem_type, [&](auto kind) {
            constexpr int KIND = decltype(kind)::value;
            constexpr int WIDE = 16 / mask_elem<KIND>::size;  // rows_vec gives 16 for uint8 alone
            if (vec == WIDE) hipLaunchKernelGGL((rle_rows_kernel<KIND, WIDE, EMIT>), grid, block, 0, s, a);
            else if (KIND == MASK_U8 && vec == 4) hipLaunchKernelGGL((rle_rows_kernel<MASK_U8, 4, EMIT>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((rle_rows_kernel<KIND, 1, EMIT>), grid, block, 0, s, a);
        });
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}

int check_sizes(const char* what, int elem_type, int n, int h, int w, size_t scratch_bytes) {
    SOLA_TRY(check_mask_sizes(what, elem_type, n, h, w));
    SOLA_ARG((long long)h * w < (1ll << 31), "%s: image too large (h*w must be < 2^31)", what);
    const size_t need = rle_encode_scratch_bytes(n, h, w);
    SOLA_ARG(scratch_bytes >= need, "%s: scratch %zu bytes < required %zu", what, scratch_bytes, need);
    return SOLA_OK;
}

}  // namespace

size_t rle_encode_scratch_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const size_t bands = ((size_t)h + RLE_BAND - 1) / RLE_BAND;
    return ((size_t)n * (size_t)w * bands * sizeof(uint32_t) + 255) & ~(size_t)255;
}

int launch_rle_encode_runs(const void* masks, int elem_type, int n, int h, int w, long long* run_off, void* scratch,
                           size_t scratch_bytes, hipStream_t s) {
    SOLA_TRY(check_sizes("rle_encode_runs", elem_type, n, h, w, scratch_bytes));
    RowsArgs a{};
    a.masks = masks; a.seg = static_cast<uint32_t*>(scratch);
    a.h = h; a.w = w; a.B = (h + RLE_BAND - 1) / RLE_BAND;
    SOLA_TRY(launch_rows<false>(a, elem_type, n, s));
    const long long S = (long long)w * a.B;
    for (int f0 = 0; f0 < n; f0 += RLE_FRAMES) {
        hipLaunchKernelGGL(rle_seg_scan_kernel, dim3((unsigned)std::min(RLE_FRAMES, n - f0)), dim3(256), 0, s, a.seg, S, run_off, f0);
        SOLA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rle_frame_scan_kernel, dim3(1), dim3(256), 0, s, run_off, n);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_rle_encode_cum(const void* masks, int elem_type, int n, int h, int w, const long long* run_off, uint32_t* cum,
                          long long* char_off, void* scratch, size_t scratch_bytes, hipStream_t s) {
    SOLA_TRY(check_sizes("rle_encode_cum", elem_type, n, h, w, scratch_bytes));
    RowsArgs a{};
    a.masks = masks; a.seg = static_cast<uint32_t*>(scratch); a.run_off = run_off; a.cum = cum;
    a.h = h; a.w = w; a.B = (h + RLE_BAND - 1) / RLE_BAND;
    SOLA_TRY(launch_rows<true>(a, elem_type, n, s));
    for (int f0 = 0; f0 < n; f0 += RLE_FRAMES) {
        hipLaunchKernelGGL(rle_char_count_kernel, dim3((unsigned)std::min(RLE_FRAMES, n - f0)), dim3(256), 0, s, cum, run_off, char_off, f0);
        SOLA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rle_frame_scan_kernel, dim3(1), dim3(256), 0, s, char_off, n);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_rle_encode_chars(const uint32_t* cum, const long long* run_off, const long long* char_off, int n, char* chars,
                            hipStream_t s) {
    SOLA_ARG(n > 0, "rle_encode_chars: bad sizes n=%d", n);
    for (int f0 = 0; f0 < n; f0 += RLE_FRAMES) {
        hipLaunchKernelGGL(rle_chars_kernel, dim3((unsigned)std::min(RLE_FRAMES, n - f0)), dim3(256), 0, s, cum, run_off, char_off, chars, f0);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}
