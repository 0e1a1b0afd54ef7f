// Baseline JPEG frames -> uint8 RGB on the device, the bytes of PIL's Image.open(f).convert("RGB") (include/sola_hip.h has the format
// contract, the refusals and the arithmetic).  The host parses (jpeg_plan.h: jpeg_parse), the device does the rest:
//
//   jpeg_layout_kernel    a block per frame: subsequences per restart segment, their prefix sums, and for every subsequence its byte
//                         range, its segment and the start a decoder that knows nothing would take (behind a stuffed 00).
//   jpeg_sync_kernel      a thread per subsequence, a block of JPEG_NT consecutive ones of a frame.  Thread i maps an in-state
//                         (bit position, block in the MCU, zigzag index) to the state behind the symbols that start in its bytes
//                         (jpeg_decode_subseq) and the number of blocks it completed.  In-states are known at segment starts and
//                         guessed elsewhere; round after round each thread takes its predecessor's out-state as its in-state and
//                         decodes again if that changed, behind barriers, until none did.  This is the self-synchronising decode of
//                         Weissenberger and Schmidt as a fixed-point iteration: "running on into the successor until the states
//                         meet" is the successor decoding again from the new state and finding its old out-state.  Across blocks the
//                         first thread takes the out-state its predecessor block left in the PREVIOUS launch (tail[], double
//                         buffered: no block reads what another writes in the same launch), and the host launches again while the
//                         change flag is set.  After round r the first r subsequences of a segment are final, so a block's loop ends
//                         within JPEG_NT + 1 rounds and the host's within the number of blocks per frame.  Nothing waits.
//   jpeg_prefix_kernel    exclusive scan of the completed-block counts of a frame.
//   jpeg_write_kernel     the decode once more from the final in-states, writing coefficient * quantiser as int16 in natural order
//                         into the zeroed buffer, DC as differences.  The first block of subsequence i is the first block of its
//                         segment + (prefix[i] - prefix[first subsequence of the segment]).
//   jpeg_dc_kernel        a block per (component, frame): segmented inclusive scan of the DC differences, reset at restart segments.
//   jpeg_idct_kernel      a thread per 8x8 block in plane order: islow IDCT into the component planes (padded to whole MCUs).
//   jpeg_colour_kernel    a thread per output pixel: fancy upsampling at the CROPPED plane sizes, YCbCr -> RGB, interleaved store.
//
// The sync and write kernels keep the frame's Huffman and quantisation tables in LDS (the index is per lane: scalar loads cannot
// serve it) and stage the block's contiguous range of the scan there with 16-byte loads; a block whose range does not fit (segment
// tables that no parser wrote) reads the scan from memory instead, same arithmetic.  All integer; the only atomics are ORs into the
// error words and the change flag.
#include <algorithm>

#include "kernels.h"
#include "jpeg_plan.h"

namespace {

#ifndef SOLA_JPEG_NT
#define SOLA_JPEG_NT 256  // (a -D builds the variants DESIGN.md row f17 compares)
#endif
constexpr int JPEG_NT = SOLA_JPEG_NT;  // subsequences (threads) per block of the sync / write kernels
constexpr int JPEG_SCAN_NT = 1024;     // threads of the prefix and DC scans
constexpr int JPEG_STAGE_MAX = 128 * 1024;  // dynamic LDS of the sync / write kernels at most (+ 8 KiB static, of a CU's 160 KiB)

struct JpegArgs {
    const uint8_t* scan;
    long long scan_bytes;
    const int32_t* segs;
    long long n_segs;
    const SolaJpegPlan* plans;  // device
    uint8_t* out;
    int T, S, W, H, ncomp, hs, vs, mcus_x, mcus_y, bpm, n_blocks;
    int sub_cap, seg_cap, wgs, stage_bytes;
    int yw, yh, cw, ch;  // padded plane sizes
    int16_t* coef;       // [T][n_blocks][64]
    uint8_t* planes;     // [T][yw*yh + 2*cw*ch]
    int4* info;          // [T][sub_cap]: lo, hi, segment | first-of-segment << 31, guessed start
    JpegState *sin, *sout, *tail;  // [T][sub_cap] x 2, [2][T][wgs]
    int32_t *cnt, *pref;           // [T][sub_cap]
    int32_t* seg_first;            // [T][seg_cap + 1]
    int32_t *nsub, *err, *flag;    // [T], [T], [1]
};

// what a frame's plan in device memory says, cut down to what the call's buffers hold
struct JpegFrame {
    const uint8_t* scan;
    int scan_len, nseg, ri;
    const int32_t* segs;
};
__device__ __forceinline__ JpegFrame jpeg_frame(const JpegArgs& a, int t) {
    const SolaJpegPlan* p = a.plans + t;
    JpegFrame f;
    long long off = p->scan_offset, len = p->scan_end - p->scan_begin;
    if (off < 0 || off > a.scan_bytes) off = a.scan_bytes;
    len = std::max(0ll, std::min(std::min(len, a.scan_bytes - off), (1ll << 28) - 1));
    f.scan = a.scan + off;
    f.scan_len = (int)len;
    long long so = p->seg_offset, ns = std::max(0, std::min(p->n_segments, a.seg_cap));
    if (so < 0 || so + ns > a.n_segs) ns = 0, so = 0;
    f.segs = a.segs + 2 * so;
    f.nseg = (int)ns;
    f.ri = std::max(0, p->restart_interval);
    return f;
}
__device__ __forceinline__ int2 jpeg_seg(const JpegFrame& f, int s) {
    const int lo = std::max(0, std::min(f.segs[2 * s], f.scan_len));
    return make_int2(lo, std::max(lo, std::min(f.segs[2 * s + 1], f.scan_len)));
}

// ------------------------------------------------------------------------------------------------------------------ layout
__global__ __launch_bounds__(JPEG_NT) void jpeg_layout_kernel(const JpegArgs a) {
    __shared__ int scan_s[JPEG_NT];
    __shared__ int carry_s;
    const int t = blockIdx.x, tid = threadIdx.x;
    const JpegFrame f = jpeg_frame(a, t);
    int32_t* seg_first = a.seg_first + (long long)t * (a.seg_cap + 1);
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < f.nseg; base += JPEG_NT) {
        const int s = base + tid;
        int n = 0;
        if (s < f.nseg) {
            const int2 r = jpeg_seg(f, s);
            n = std::max(1, (r.y - r.x + a.S - 1) / a.S);
        }
        scan_s[tid] = n;
        __syncthreads();
        for (int d = 1; d < JPEG_NT; d <<= 1) {
            const int v = tid >= d ? scan_s[tid - d] : 0;
            __syncthreads();
            scan_s[tid] += v;
            __syncthreads();
        }
        const int carry = carry_s;
        if (s < f.nseg) seg_first[s] = (int)std::min((long long)carry + scan_s[tid] - n, (long long)a.sub_cap);
        __syncthreads();
        if (tid == JPEG_NT - 1) carry_s = (int)std::min((long long)carry + scan_s[tid], (long long)a.sub_cap);
        __syncthreads();
    }
    const int nsub = carry_s;
    if (tid == 0) {
        seg_first[f.nseg] = nsub;
        a.nsub[t] = nsub;
    }
    __syncthreads();  // (the block's own writes to seg_first are visible to it behind the barrier)
    const JpegBytes bytes{f.scan, 0, f.scan_len};
    for (int i = tid; i < nsub; i += JPEG_NT) {
        int lo = 0, hi = f.nseg;  // the segment s with seg_first[s] <= i < seg_first[s + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_first[mid] <= i) lo = mid; else hi = mid;
        }
        const int2 r = jpeg_seg(f, lo);
        const int j = i - seg_first[lo];
        const int b = (int)std::min((long long)r.x + (long long)j * a.S, (long long)r.y);
        const int e = std::min(b + a.S, r.y);
        a.info[(long long)t * a.sub_cap + i] = make_int4(b, e, lo | (j == 0 ? (int)0x80000000 : 0), j == 0 ? b : jpeg_guess_start(bytes, b, r.x));
    }
}

// ------------------------------------------------------------------------------------------------------- sync and write
struct JpegBlockLds {
    SolaJpegHuff huff[6];
    uint16_t quant[192];
};
static_assert(sizeof(SolaJpegHuff) % 16 == 0 && sizeof(JpegBlockLds) % 16 == 0, "the tables are copied as 16-byte words");

// the frame's tables -> LDS
__device__ __forceinline__ void jpeg_load_tables(const JpegArgs& a, int t, JpegBlockLds* l, int tid) {
    const uint4* src = reinterpret_cast<const uint4*>(a.plans[t].huff);  // (hipMalloc'ed array of 16-byte-multiple structs: checked on the host)
    uint4* dst = reinterpret_cast<uint4*>(l->huff);
    for (int k = tid; k < (int)(sizeof(l->huff) / 16); k += JPEG_NT) dst[k] = src[k];
    for (int k = tid; k < 192; k += JPEG_NT) l->quant[k] = a.plans[t].quant[k / 64][k % 64];
}

// the bytes [lo, hi + 16) of the frame's scan -> LDS when they fit; else the scan in memory
__device__ __forceinline__ JpegBytes jpeg_stage(const JpegArgs& a, const JpegFrame& f, int lo, int hi, uint8_t* lds, int tid) {
    const long long base = f.scan - a.scan;  // the frame's first byte in a.scan (16-byte aligned: checked on the host)
    const long long g0 = (base + lo) & ~15ll, g1 = std::min((base + std::min(hi + 16, f.scan_len) + 15) & ~15ll, (a.scan_bytes + 15) & ~15ll);
    if (g1 - g0 > a.stage_bytes || a.stage_bytes == 0) return JpegBytes{f.scan, 0, f.scan_len};
    for (long long g = g0 + 16ll * tid; g < g1; g += 16ll * JPEG_NT) {
        if (g + 16 <= a.scan_bytes) {
            *reinterpret_cast<uint4*>(lds + (g - g0)) = *reinterpret_cast<const uint4*>(a.scan + g);
        } else {
            for (int k = 0; k < 16; ++k) lds[g - g0 + k] = g + k < a.scan_bytes ? a.scan[g + k] : 0;
        }
    }
    const int first = (int)std::max(g0 - base, 0ll);  // scan index of the first staged byte that is the frame's
    return JpegBytes{lds + (base + first - g0), first, (int)std::min(g1 - base, (long long)f.scan_len)};
}

__device__ __forceinline__ JpegTables jpeg_tables(const JpegArgs& a, const JpegBlockLds* l) {
    return JpegTables{l->huff, l->quant, a.ncomp, a.ncomp == 1 ? 1 : a.hs * a.vs, a.bpm};
}

__global__ __launch_bounds__(JPEG_NT) void jpeg_sync_kernel(const JpegArgs a, const int round) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage_s[];
    __shared__ JpegBlockLds lds;
    __shared__ JpegState out_s[JPEG_NT];
    const int t = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const int nsub = std::min(a.nsub[t], a.sub_cap);
    const int first = w * JPEG_NT;
    if (first >= nsub) return;
    const int last = std::min(first + JPEG_NT, nsub) - 1, i = first + tid;
    const bool active = i <= last;
    const long long row = (long long)t * a.sub_cap;
    const int4 info = a.info[row + std::min(i, last)];
    const bool seg_start = info.z < 0;
    JpegState* tail_new = a.tail + ((long long)(round & 1) * a.T + t) * a.wgs;
    const JpegState* tail_old = a.tail + ((long long)((round & 1) ^ 1) * a.T + t) * a.wgs;
    JpegState in, out = 0;
    int cnt = 0;
    bool dirty;
    if (round == 0) {
        in = jpeg_state((unsigned)info.w * 8u, 0, 0);
        dirty = active;
    } else {
        in = active ? a.sin[row + i] : 0;
        out = active ? a.sout[row + i] : 0;
        cnt = active ? a.cnt[row + i] : 0;
        dirty = false;
        if (tid == 0 && !seg_start && w > 0) {
            const JpegState cand = tail_old[w - 1];
            dirty = cand != in;
            in = cand;
        }
        if (!__syncthreads_or(dirty)) {  // the predecessor block left what it left before: this block's states stand
            if (tid == 0) tail_new[w] = tail_old[w];
            return;
        }
    }
    const JpegFrame f = jpeg_frame(a, t);
    jpeg_load_tables(a, t, &lds, tid);
    const JpegBytes bytes = jpeg_stage(a, f, a.info[row + first].x, a.info[row + last].y, stage_s, tid);
    __syncthreads();
    const JpegTables tab = jpeg_tables(a, &lds);
    const int2 seg = jpeg_seg(f, info.z & 0x7FFFFFFF);
    const JpegSubseq q{info.x, info.y, seg.x, seg.y};
    for (int iter = 0; iter <= JPEG_NT; ++iter) {  // after iteration k the block's first k + 1 states are final
        if (dirty) out = jpeg_decode_subseq<false>(bytes, q, tab, in, &cnt, nullptr, 0, 0, nullptr);
        out_s[tid] = out;
        __syncthreads();
        JpegState cand = in;
        if (active && tid > 0 && !seg_start) cand = out_s[tid - 1];
        dirty = cand != in;
        in = cand;
        if (!__syncthreads_or(dirty)) break;
    }
    if (active) {
        a.sin[row + i] = in;
        a.sout[row + i] = out;
        a.cnt[row + i] = cnt;
    }
    if (i == last) {
        tail_new[w] = out;
        // someone reads it only if the frame has a block behind this one; from round 1 on only a change matters
        if (last + 1 < nsub && (round == 0 || tail_old[w] != out)) atomicOr(a.flag, 1);
    }
}

__global__ __launch_bounds__(JPEG_SCAN_NT) void jpeg_prefix_kernel(const JpegArgs a) {
    __shared__ int scan_s[JPEG_SCAN_NT];
    __shared__ int carry_s;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int nsub = std::min(a.nsub[t], a.sub_cap);
    const long long row = (long long)t * a.sub_cap;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nsub; base += JPEG_SCAN_NT) {
        const int i = base + tid;
        const int n = i < nsub ? a.cnt[row + i] : 0;
        scan_s[tid] = n;
        __syncthreads();
        for (int d = 1; d < JPEG_SCAN_NT; d <<= 1) {
            const int v = tid >= d ? scan_s[tid - d] : 0;
            __syncthreads();
            scan_s[tid] += v;
            __syncthreads();
        }
        const int carry = carry_s;
        if (i < nsub) a.pref[row + i] = carry + scan_s[tid] - n;  // (wraps on rubbish counts: the write kernel checks every block index)
        __syncthreads();
        if (tid == JPEG_SCAN_NT - 1) carry_s = carry + scan_s[tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(JPEG_NT) void jpeg_write_kernel(const JpegArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage_s[];
    __shared__ JpegBlockLds lds;
    const int t = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const int nsub = std::min(a.nsub[t], a.sub_cap);
    const int first = w * JPEG_NT;
    if (first >= nsub) return;
    const int last = std::min(first + JPEG_NT, nsub) - 1, i = first + tid;
    const long long row = (long long)t * a.sub_cap;
    const JpegFrame f = jpeg_frame(a, t);
    jpeg_load_tables(a, t, &lds, tid);
    const JpegBytes bytes = jpeg_stage(a, f, a.info[row + first].x, a.info[row + last].y, stage_s, tid);
    __syncthreads();
    if (i > last) return;
    const JpegTables tab = jpeg_tables(a, &lds);
    const int4 info = a.info[row + i];
    const int s = info.z & 0x7FFFFFFF;
    const int2 seg = jpeg_seg(f, s);
    const JpegSubseq q{info.x, info.y, seg.x, seg.y};
    const int32_t* seg_first = a.seg_first + (long long)t * (a.seg_cap + 1);
    // the segment's blocks, and this subsequence's first among them
    const long long per_seg = f.ri ? (long long)f.ri * a.bpm : (long long)a.n_blocks;
    const long long blk_lo = std::min((long long)s * per_seg, (long long)a.n_blocks), blk_hi = std::min(blk_lo + per_seg, (long long)a.n_blocks);
    const long long rel = (long long)a.pref[row + i] - (long long)a.pref[row + std::min(std::max(seg_first[s], 0), nsub - 1)];
    const long long blk = blk_lo + std::max(0ll, std::min(rel, blk_hi - blk_lo));
    int cnt = 0, err = 0;
    jpeg_decode_subseq<true>(bytes, q, tab, a.sin[row + i], &cnt, a.coef + (long long)t * a.n_blocks * 64, blk, blk_hi, &err);
    const bool seg_last = i + 1 >= nsub || a.info[row + i + 1].z < 0;
    if (seg_last && blk + cnt < blk_hi) err |= JPEG_ERR_SHORT;
    if (err) atomicOr(a.err + t, err);
}

// ----------------------------------------------------------------------------------------------------------------- DC scan
// element e of component c: its e-th block in scan order
__device__ __forceinline__ int jpeg_comp_blocks(const JpegArgs& a, int c) { return (c == 0 && a.ncomp == 3) ? a.hs * a.vs : 1; }

__global__ __launch_bounds__(JPEG_SCAN_NT) void jpeg_dc_kernel(const JpegArgs a) {
    __shared__ int val_s[JPEG_SCAN_NT];
    __shared__ int head_s[JPEG_SCAN_NT];
    __shared__ int carry_s;
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int bc = jpeg_comp_blocks(a, c), ny = a.ncomp == 1 ? 1 : a.hs * a.vs;
    const int mcus = a.n_blocks / a.bpm, total = mcus * bc;
    const int ri = jpeg_frame(a, t).ri;
    int16_t* coef = a.coef + (long long)t * a.n_blocks * 64;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < total; base += JPEG_SCAN_NT) {
        const int e = base + tid;
        int v = 0, head = 0;
        long long at = 0;
        if (e < total) {
            const int mcu = e / bc, k = e - mcu * bc;
            at = ((long long)mcu * a.bpm + (c == 0 ? k : ny + c - 1)) * 64;
            v = coef[at];
            head = (ri > 0 && k == 0 && mcu % ri == 0) ? 1 : 0;
        }
        val_s[tid] = v;
        head_s[tid] = head;
        __syncthreads();
        for (int d = 1; d < JPEG_SCAN_NT; d <<= 1) {  // segmented inclusive scan: a head stops what comes from the left
            int add = 0, h = 0;
            if (tid >= d) {
                h = head_s[tid - d];
                if (!head_s[tid]) add = val_s[tid - d];
            }
            __syncthreads();
            val_s[tid] += add;
            head_s[tid] |= h;
            __syncthreads();
        }
        const int sum = val_s[tid] + (head_s[tid] ? 0 : carry_s);
        if (e < total) coef[at] = (int16_t)sum;
        __syncthreads();
        if (tid == JPEG_SCAN_NT - 1) carry_s = sum;
        __syncthreads();
    }
}

// -------------------------------------------------------------------------------------------------------------------- IDCT
__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one islow pass over (v0 .. v7), shared by columns and rows up to the descale
#define JPEG_IDCT_1D(v0, v1, v2, v3, v4, v5, v6, v7, SHIFT, o0, o1, o2, o3, o4, o5, o6, o7)     \
    {                                                                                           \
        int z2 = v2, z3 = v6;                                                                   \
        int z1 = (z2 + z3) * 4433;                                                              \
        int tmp2 = z1 + z3 * (-15137);                                                          \
        int tmp3 = z1 + z2 * 6270;                                                              \
        int tmp0 = (v0 + v4) << 13;                                                             \
        int tmp1 = (v0 - v4) << 13;                                                             \
        const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2; \
        tmp0 = v7; tmp1 = v5; tmp2 = v3; tmp3 = v1;                                             \
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;                                   \
        int z4 = tmp1 + tmp3;                                                                   \
        const int z5 = (z3 + z4) * 9633;                                                        \
        tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;                              \
        z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;                                   \
        z3 += z5; z4 += z5;                                                                     \
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;                     \
        o0 = jpeg_descale(tmp10 + tmp3, SHIFT); o7 = jpeg_descale(tmp10 - tmp3, SHIFT);         \
        o1 = jpeg_descale(tmp11 + tmp2, SHIFT); o6 = jpeg_descale(tmp11 - tmp2, SHIFT);         \
        o2 = jpeg_descale(tmp12 + tmp1, SHIFT); o5 = jpeg_descale(tmp12 - tmp1, SHIFT);         \
        o3 = jpeg_descale(tmp13 + tmp0, SHIFT); o4 = jpeg_descale(tmp13 - tmp0, SHIFT);         \
    }

__device__ __forceinline__ int jpeg_clamp8(int v) { return std::min(std::max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegArgs a) {
    const int t = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;  // block in plane order: luma rows, then Cb, then Cr
    if (e >= a.n_blocks) return;
    const int ybw = a.yw >> 3, ybh = a.yh >> 3, cbw = a.cw >> 3, cbh = a.ch >> 3;
    const int ny = a.ncomp == 1 ? 1 : a.hs * a.vs, nyb = ybw * ybh;
    int bx, by, blk, pitch;
    uint8_t* plane = a.planes + (long long)t * ((long long)a.yw * a.yh + 2ll * a.cw * a.ch);
    if (e < nyb) {
        by = e / ybw; bx = e - by * ybw;
        const int mx = bx / a.hs, my = by / a.vs;
        blk = (my * a.mcus_x + mx) * a.bpm + (by - my * a.vs) * a.hs + (bx - mx * a.hs);
        pitch = a.yw;
    } else {
        const int c = (e - nyb) / (cbw * cbh), r = (e - nyb) - c * cbw * cbh;
        by = r / cbw; bx = r - by * cbw;
        blk = (by * a.mcus_x + bx) * a.bpm + ny + c;
        pitch = a.cw;
        plane += (long long)a.yw * a.yh + (long long)c * a.cw * a.ch;
    }
    if (blk < 0 || blk >= a.n_blocks) return;
    const uint4* src = reinterpret_cast<const uint4*>(a.coef + ((long long)t * a.n_blocks + blk) * 64);
    int ws[64];
    union { uint4 q; int16_t h[8]; } rowv[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) rowv[r].q = src[r];
#pragma unroll
    for (int x = 0; x < 8; ++x)
        JPEG_IDCT_1D(rowv[0].h[x], rowv[1].h[x], rowv[2].h[x], rowv[3].h[x], rowv[4].h[x], rowv[5].h[x], rowv[6].h[x], rowv[7].h[x], 11,
                     ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x]);
    uint8_t* dst = plane + ((long long)by * 8) * pitch + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int o0, o1, o2, o3, o4, o5, o6, o7;
        JPEG_IDCT_1D(ws[8 * y], ws[8 * y + 1], ws[8 * y + 2], ws[8 * y + 3], ws[8 * y + 4], ws[8 * y + 5], ws[8 * y + 6], ws[8 * y + 7], 18,
                     o0, o1, o2, o3, o4, o5, o6, o7);
        uint2 px;
        px.x = jpeg_clamp8(o0 + 128) | (jpeg_clamp8(o1 + 128) << 8) | (jpeg_clamp8(o2 + 128) << 16) | (jpeg_clamp8(o3 + 128) << 24);
        px.y = jpeg_clamp8(o4 + 128) | (jpeg_clamp8(o5 + 128) << 8) | (jpeg_clamp8(o6 + 128) << 16) | (jpeg_clamp8(o7 + 128) << 24);
        *reinterpret_cast<uint2*>(dst + (long long)y * pitch) = px;  // (planes are 16-byte aligned, pitches multiples of 8)
    }
}

// ------------------------------------------------------------------------------------------------------ upsample + colour
// The chroma samples of the output pixels x0 .. x0 + 3 (x0 % 4 == 0) of row y from plane s (pitch a.cw), cropped to cw x ch samples.
__device__ __forceinline__ void jpeg_chroma4(const JpegArgs& a, const uint8_t* s, int x0, int y, int cw, int ch, int& c0, int& c1, int& c2, int& c3) {
    if (a.hs == 1) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(s + (long long)y * a.cw + x0);  // (pitch and x0 are multiples of 4)
        c0 = v & 255; c1 = (v >> 8) & 255; c2 = (v >> 16) & 255; c3 = v >> 24;
        return;
    }
    const int i0 = x0 >> 1, last = cw - 1;
    const int j = a.vs == 2 ? y >> 1 : y;
    const uint8_t* r0 = s + (long long)j * a.cw;
    // the four samples around the two the pixels sit on; an index outside the plane is only ever read where an edge rule replaces it
    const int k0 = max(i0 - 1, 0), k1 = min(i0, last), k2 = min(i0 + 1, last), k3 = min(i0 + 2, last);
    if (cw <= 2) {  // libjpeg replicates planes this narrow
        c0 = c1 = r0[k1];
        c2 = c3 = r0[k2];
        return;
    }
    if (a.vs == 1) {
        const int v0 = r0[k0], v1 = r0[k1], v2 = r0[k2], v3 = r0[k3];
        c0 = i0 == 0 ? v1 : (3 * v1 + v0 + 1) >> 2;
        c1 = i0 == last ? v1 : (3 * v1 + v2 + 2) >> 2;
        c2 = (3 * v2 + v1 + 1) >> 2;
        c3 = i0 + 1 == last ? v2 : (3 * v2 + v3 + 2) >> 2;
        return;
    }
    const uint8_t* r1 = s + (long long)((y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0)) * a.cw;
    const int v0 = 3 * r0[k0] + r1[k0], v1 = 3 * r0[k1] + r1[k1], v2 = 3 * r0[k2] + r1[k2], v3 = 3 * r0[k3] + r1[k3];
    c0 = i0 == 0 ? (4 * v1 + 8) >> 4 : (3 * v1 + v0 + 8) >> 4;
    c1 = i0 == last ? (4 * v1 + 7) >> 4 : (3 * v1 + v2 + 7) >> 4;
    c2 = (3 * v2 + v1 + 8) >> 4;
    c3 = i0 + 1 == last ? (4 * v2 + 7) >> 4 : (3 * v2 + v3 + 7) >> 4;
}

__device__ __forceinline__ uint32_t jpeg_rgb(int Y, int cb, int cr) {
    cb -= 128; cr -= 128;
    const int r = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
    const int g = jpeg_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const int b = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

// a thread per four pixels of a row
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegArgs a) {
    const int t = blockIdx.z, y = blockIdx.y, x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= a.W) return;
    const uint8_t* plane = a.planes + (long long)t * ((long long)a.yw * a.yh + 2ll * a.cw * a.ch);
    const uint32_t yy = *reinterpret_cast<const uint32_t*>(plane + (long long)y * a.yw + x0);  // (the padded pitch is a multiple of 8)
    uint32_t p0, p1, p2, p3;
    if (a.ncomp == 1) {
        p0 = (yy & 255) * 0x010101u; p1 = ((yy >> 8) & 255) * 0x010101u; p2 = ((yy >> 16) & 255) * 0x010101u; p3 = (yy >> 24) * 0x010101u;
    } else {
        const int cw = (a.W + a.hs - 1) / a.hs, ch = (a.H + a.vs - 1) / a.vs;
        const uint8_t* pcb = plane + (long long)a.yw * a.yh;
        int b0, b1, b2, b3, r0, r1, r2, r3;
        jpeg_chroma4(a, pcb, x0, y, cw, ch, b0, b1, b2, b3);
        jpeg_chroma4(a, pcb + (long long)a.cw * a.ch, x0, y, cw, ch, r0, r1, r2, r3);
        p0 = jpeg_rgb(yy & 255, b0, r0); p1 = jpeg_rgb((yy >> 8) & 255, b1, r1); p2 = jpeg_rgb((yy >> 16) & 255, b2, r2); p3 = jpeg_rgb(yy >> 24, b3, r3);
    }
    uint8_t* o = a.out + (((long long)t * a.H + y) * a.W + x0) * 3;
    if (x0 + 4 <= a.W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = p0 | (p1 << 24);
        o4[1] = (p1 >> 8) | (p2 << 16);
        o4[2] = (p2 >> 16) | (p3 << 8);
        return;
    }
    const int n = min(4, a.W - x0);
    const uint32_t px[4] = {p0, p1, p2, p3};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) {
            o[3 * k] = (uint8_t)px[k];
            o[3 * k + 1] = (uint8_t)(px[k] >> 8);
            o[3 * k + 2] = (uint8_t)(px[k] >> 16);
        }
}

// -------------------------------------------------------------------------------------------------------------------- host
size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct JpegLayout {
    JpegArgs a;
    size_t off_coef, off_planes, off_info, off_sin, off_sout, off_tail, off_cnt, off_pref, off_seg_first, off_words, total;
    size_t coef_bytes, words_bytes;
};

int jpeg_layout(const char* who, const SolaJpegPlan* plans, int T, int subseq_bytes, JpegLayout& L) {
    SOLA_ARG(plans, "%s: null plans", who);
    SOLA_ARG(T >= 1 && T <= 65535, "%s: T = %d, 1 .. 65535 frames in a call", who, T);
    const int S = subseq_bytes ? subseq_bytes : SOLA_JPEG_SUBSEQ_DEFAULT;
    SOLA_ARG(S >= SOLA_JPEG_SUBSEQ_MIN && S <= SOLA_JPEG_SUBSEQ_MAX && (S & (S - 1)) == 0, "%s: subseq_bytes %d: 0 or a power of two %d .. %d", who,
             subseq_bytes, SOLA_JPEG_SUBSEQ_MIN, SOLA_JPEG_SUBSEQ_MAX);
    const SolaJpegPlan& p0 = plans[0];
    SOLA_ARG(p0.width >= 1 && p0.height >= 1 && p0.width <= SOLA_JPEG_MAX_SIZE && p0.height <= SOLA_JPEG_MAX_SIZE, "%s: size %dx%d outside 1 .. %d", who,
             p0.width, p0.height, SOLA_JPEG_MAX_SIZE);
    SOLA_ARG((p0.ncomp == 1 && p0.hs == 1 && p0.vs == 1) || (p0.ncomp == 3 && (p0.hs == 1 || p0.hs == 2) && (p0.vs == 1 || p0.vs == 2) && p0.hs >= p0.vs),
             "%s: %d components with luma sampling %dx%d", who, p0.ncomp, p0.hs, p0.vs);
    const int bpm = p0.ncomp == 1 ? 1 : p0.hs * p0.vs + 2;
    const int mx = (p0.width + 8 * p0.hs - 1) / (8 * p0.hs), my = (p0.height + 8 * p0.vs - 1) / (8 * p0.vs);
    SOLA_ARG(p0.mcus_x == mx && p0.mcus_y == my && p0.blocks_per_mcu == bpm && (long long)p0.n_blocks == (long long)mx * my * bpm,
             "%s: plan 0 does not fit together (%d x %d MCUs of %d blocks, %d blocks)", who, p0.mcus_x, p0.mcus_y, p0.blocks_per_mcu, p0.n_blocks);
    long long sub_cap = 1, seg_cap = 1;
    for (int t = 0; t < T; ++t) {
        const SolaJpegPlan& p = plans[t];
        SOLA_ARG(p.width == p0.width && p.height == p0.height && p.ncomp == p0.ncomp && p.hs == p0.hs && p.vs == p0.vs && p.mcus_x == mx &&
                     p.mcus_y == my && p.blocks_per_mcu == bpm && p.n_blocks == p0.n_blocks,
                 "%s: frame %d (%dx%d, %d components, %dx%d) differs from frame 0 (%dx%d, %d, %dx%d)", who, t, p.width, p.height, p.ncomp, p.hs, p.vs,
                 p0.width, p0.height, p0.ncomp, p0.hs, p0.vs);
        const long long len = p.scan_end - p.scan_begin;
        SOLA_ARG(len >= 0 && len < (1ll << 28), "%s: frame %d: scan of %lld bytes", who, t, len);
        SOLA_ARG(p.n_segments >= 1 && p.n_segments <= (1 << 26) && p.restart_interval >= 0, "%s: frame %d: %d segments, restart interval %d", who, t,
                 p.n_segments, p.restart_interval);
        sub_cap = std::max(sub_cap, (len + S - 1) / S + p.n_segments);
        seg_cap = std::max(seg_cap, (long long)p.n_segments);
    }
    SOLA_ARG(sub_cap * T < (1ll << 30), "%s: %lld subsequences in a call", who, sub_cap * T);
    JpegArgs& a = L.a;
    memset(&a, 0, sizeof(a));
    a.T = T; a.S = S; a.W = p0.width; a.H = p0.height; a.ncomp = p0.ncomp; a.hs = p0.hs; a.vs = p0.vs;
    a.mcus_x = mx; a.mcus_y = my; a.bpm = bpm; a.n_blocks = p0.n_blocks;
    a.sub_cap = (int)sub_cap; a.seg_cap = (int)seg_cap;
    a.wgs = (a.sub_cap + JPEG_NT - 1) / JPEG_NT;
    const long long stage = ((long long)JPEG_NT * (S + 2) + 64 + 15) & ~15ll;
    a.stage_bytes = stage <= JPEG_STAGE_MAX ? (int)stage : 0;
    a.yw = mx * p0.hs * 8; a.yh = my * p0.vs * 8;
    a.cw = p0.ncomp == 1 ? 0 : mx * 8; a.ch = p0.ncomp == 1 ? 0 : my * 8;
    size_t o = 0;
    L.coef_bytes = (size_t)T * a.n_blocks * 128;
    L.off_coef = o; o += up256(L.coef_bytes);
    L.words_bytes = up256((size_t)(2 * T + 1) * 4);
    L.off_words = o; o += L.words_bytes;  // nsub, err, flag: zeroed with the coefficients
    L.off_planes = o; o += up256((size_t)T * ((size_t)a.yw * a.yh + 2 * (size_t)a.cw * a.ch));
    L.off_info = o; o += up256((size_t)T * a.sub_cap * 16);
    L.off_sin = o; o += up256((size_t)T * a.sub_cap * 8);
    L.off_sout = o; o += up256((size_t)T * a.sub_cap * 8);
    L.off_tail = o; o += up256((size_t)2 * T * a.wgs * 8);
    L.off_cnt = o; o += up256((size_t)T * a.sub_cap * 4);
    L.off_pref = o; o += up256((size_t)T * a.sub_cap * 4);
    L.off_seg_first = o; o += up256((size_t)T * (a.seg_cap + 1) * 4);
    L.total = o;
    return SOLA_OK;
}

void jpeg_bind(JpegLayout& L, void* scratch) {
    uint8_t* b = reinterpret_cast<uint8_t*>(scratch);
    JpegArgs& a = L.a;
    a.coef = reinterpret_cast<int16_t*>(b + L.off_coef);
    a.nsub = reinterpret_cast<int32_t*>(b + L.off_words);
    a.err = a.nsub + a.T;
    a.flag = a.err + a.T;
    a.planes = b + L.off_planes;
    a.info = reinterpret_cast<int4*>(b + L.off_info);
    a.sin = reinterpret_cast<JpegState*>(b + L.off_sin);
    a.sout = reinterpret_cast<JpegState*>(b + L.off_sout);
    a.tail = reinterpret_cast<JpegState*>(b + L.off_tail);
    a.cnt = reinterpret_cast<int32_t*>(b + L.off_cnt);
    a.pref = reinterpret_cast<int32_t*>(b + L.off_pref);
    a.seg_first = reinterpret_cast<int32_t*>(b + L.off_seg_first);
}

float* g_jpeg_profile = nullptr;

// times the stages of a call when sola_jpeg_profile asked for it: an event at every stage boundary, read at the end
struct JpegTimer {
    hipEvent_t ev[7];
    int n = 0;
    bool on;
    hipStream_t s;
    explicit JpegTimer(hipStream_t s_) : on(g_jpeg_profile != nullptr), s(s_) {
        if (on)
            for (auto& e : ev) (void)hipEventCreate(&e);
        mark();
    }
    void mark() {
        if (on && n < 7) (void)hipEventRecord(ev[n++], s);
    }
    void finish() {
        if (!on) return;
        (void)hipEventSynchronize(ev[n - 1]);
        for (int k = 0; k + 1 < n; ++k) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            g_jpeg_profile[k] += ms;
        }
        for (auto& e : ev) (void)hipEventDestroy(e);
        on = false;
    }
    ~JpegTimer() {
        if (on)
            for (auto& e : ev) (void)hipEventDestroy(e);
    }
};

}  // namespace

extern "C" int sola_jpeg_parse(const uint8_t* data, int64_t len, SolaJpegPlan* plan, int32_t* host_segs, int64_t seg_cap) {
    SOLA_ARG(data && plan, "jpeg_parse: null %s", data ? "plan" : "data");
    SOLA_ARG(len >= 0 && seg_cap >= 0 && (host_segs || seg_cap == 0), "jpeg_parse: len %lld, seg_cap %lld%s", (long long)len, (long long)seg_cap,
             host_segs ? "" : " with null host_segs");
    JpegParseError e;
    if (jpeg_parse(data, len, plan, host_segs, seg_cap, &e) != 0) {
        sola_set_error("jpeg_parse: %s", e.msg);
        return SOLA_ERR_ARG;
    }
    return SOLA_OK;
}

extern "C" size_t sola_jpeg_scratch_bytes(const SolaJpegPlan* plans, int T, int subseq_bytes) {
    JpegLayout L;
    if (jpeg_layout("jpeg_scratch_bytes", plans, T, subseq_bytes, L) != SOLA_OK) return 0;
    return L.total;
}

extern "C" int sola_jpeg_profile(float* host_ms) {
    g_jpeg_profile = host_ms;
    return SOLA_OK;
}

extern "C" int sola_jpeg_coefficients(const SolaJpegPlan* plans, int T, int subseq_bytes, const void* dev_scratch, int t, int16_t* host_coef,
                                      void* stream_) {
    JpegLayout L;
    SOLA_TRY(jpeg_layout("jpeg_coefficients", plans, T, subseq_bytes, L));
    SOLA_ARG(dev_scratch && host_coef && t >= 0 && t < T, "jpeg_coefficients: null pointer or frame %d of %d", t, T);
    hipStream_t s = as_stream(stream_);
    const size_t bytes = (size_t)L.a.n_blocks * 128;
    SOLA_HIP(hipMemcpyAsync(host_coef, reinterpret_cast<const uint8_t*>(dev_scratch) + L.off_coef + (size_t)t * bytes, bytes, hipMemcpyDeviceToHost, s));
    SOLA_HIP(hipStreamSynchronize(s));
    return SOLA_OK;
}

extern "C" int sola_jpeg_decode(const uint8_t* dev_scan, int64_t scan_bytes, const int32_t* dev_segs, int64_t n_segs, const SolaJpegPlan* plans,
                                const SolaJpegPlan* dev_plans, int T, int subseq_bytes, uint8_t* dev_out, void* dev_scratch, size_t scratch_bytes,
                                int32_t* host_err, int32_t* host_rounds, void* stream_) {
    JpegLayout L;
    SOLA_TRY(jpeg_layout("jpeg_decode", plans, T, subseq_bytes, L));
    SOLA_ARG(dev_scan && dev_segs && dev_plans && dev_out && dev_scratch && host_err, "jpeg_decode: null pointer");
    SOLA_ARG((reinterpret_cast<uintptr_t>(dev_scan) & 15) == 0 && (reinterpret_cast<uintptr_t>(dev_plans) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(dev_scratch) & 15) == 0 && (reinterpret_cast<uintptr_t>(dev_segs) & 3) == 0,
             "jpeg_decode: dev_scan, dev_plans and dev_scratch must be 16-byte aligned, dev_segs 4-byte");
    static_assert(sizeof(SolaJpegPlan) % 16 == 0 && offsetof(SolaJpegPlan, huff) % 16 == 0, "the kernels copy the tables of dev_plans[t] as 16-byte words");
    SOLA_ARG(scan_bytes >= 0 && n_segs >= 0, "jpeg_decode: scan_bytes %lld, n_segs %lld", (long long)scan_bytes, (long long)n_segs);
    SOLA_ARG(scratch_bytes >= L.total, "jpeg_decode: scratch of %zu bytes, sola_jpeg_scratch_bytes asks for %zu", scratch_bytes, L.total);
    for (int t = 0; t < T; ++t) {
        const SolaJpegPlan& p = plans[t];
        SOLA_ARG(p.scan_offset >= 0 && (p.scan_offset & 15) == 0 && p.scan_offset + (p.scan_end - p.scan_begin) <= scan_bytes,
                 "jpeg_decode: frame %d: scan of %lld bytes at offset %lld of %lld (offsets are multiples of 16)", t, (long long)(p.scan_end - p.scan_begin),
                 (long long)p.scan_offset, (long long)scan_bytes);
        SOLA_ARG(p.seg_offset >= 0 && p.seg_offset + p.n_segments <= n_segs, "jpeg_decode: frame %d: %d segments at row %lld of %lld", t, p.n_segments,
                 (long long)p.seg_offset, (long long)n_segs);
    }
    jpeg_bind(L, dev_scratch);
    JpegArgs& a = L.a;
    a.scan = dev_scan; a.scan_bytes = scan_bytes; a.segs = dev_segs; a.n_segs = n_segs; a.plans = dev_plans; a.out = dev_out;
    hipStream_t s = as_stream(stream_);
    static DeviceOnce once;  // the staging window may exceed the default dynamic LDS
    int dev;
    if (a.stage_bytes > 48 * 1024 && once.needed(&dev)) {
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(jpeg_sync_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, JPEG_STAGE_MAX));
        SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(jpeg_write_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, JPEG_STAGE_MAX));
        once.done(dev);
    }
    JpegTimer timer(s);
    SOLA_HIP(hipMemsetAsync(a.coef, 0, up256(L.coef_bytes) + L.words_bytes, s));  // coefficients, then nsub / err / flag
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3(T), dim3(JPEG_NT), 0, s, a);
    SOLA_LAUNCH_CHECK();
    timer.mark();
    const dim3 grid(a.wgs, T);
    int rounds = 0;
    for (;;) {
        hipLaunchKernelGGL(jpeg_sync_kernel, grid, dim3(JPEG_NT), a.stage_bytes, s, a, rounds);
        SOLA_LAUNCH_CHECK();
        ++rounds;
        if (a.wgs == 1) break;
        int flag = 0;
        SOLA_HIP(hipMemcpyAsync(&flag, a.flag, 4, hipMemcpyDeviceToHost, s));
        SOLA_HIP(hipStreamSynchronize(s));
        if (!flag) break;
        // after round r the first r blocks of every frame are final: wgs rounds settle everything, one more only confirms it
        if (rounds > a.wgs) break;
        SOLA_HIP(hipMemsetAsync(a.flag, 0, 4, s));
    }
    timer.mark();
    hipLaunchKernelGGL(jpeg_prefix_kernel, dim3(T), dim3(JPEG_SCAN_NT), 0, s, a);
    SOLA_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_write_kernel, grid, dim3(JPEG_NT), a.stage_bytes, s, a);
    SOLA_LAUNCH_CHECK();
    timer.mark();
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(a.ncomp, T), dim3(JPEG_SCAN_NT), 0, s, a);
    SOLA_LAUNCH_CHECK();
    timer.mark();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((a.n_blocks + 255) / 256, T), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    timer.mark();
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((a.W + 1023) / 1024, a.H, T), dim3(256), 0, s, a);
    SOLA_LAUNCH_CHECK();
    timer.mark();
    SOLA_HIP(hipMemcpyAsync(host_err, a.err, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    SOLA_HIP(hipStreamSynchronize(s));
    timer.finish();
    for (int t = 0; t < T; ++t) {  // restart segments the file does not have at all leave their blocks zero: a short frame too
        const long long mcus = (long long)a.mcus_x * a.mcus_y, ri = plans[t].restart_interval;
        if (plans[t].n_segments < (ri ? (mcus + ri - 1) / ri : 1)) host_err[t] |= JPEG_ERR_SHORT;
    }
    if (host_rounds) *host_rounds = rounds;
    return SOLA_OK;
}
