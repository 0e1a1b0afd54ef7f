// Binary masks -> the zlib streams of 8-bit greyscale PNG files on the GPU (pixel 255 where the mask is set): the write side
// of inference.py, which otherwise copies the masklet to the host and runs a general PNG encoder per frame.
//
// Format (include/sola_hip.h): filter type 0 on every scanline, so a frame's raw stream is R = h*(w+1) bytes of 0x00 / 0xFF;
// one DEFLATE block with the FIXED Huffman table and distance-1 matches only.  The stream is then a pure function of the
// maximal runs of equal raw bytes (taken across row ends): run [s, e) = literal, then L = e-s-1 bytes as matches of 258
// while L >= 261 or L == 258, L-3 then 3 for L in {259, 260}, L for 3..257, literals for 1 and 2.  The token that starts
// at raw position t is therefore known from s and min(e - t, 261) alone: at s, at s+1+258k, at s+2 (L == 2), at e-3.
//
// Work is divided by FIXED RAW SEGMENTS of 64 bytes = one 64-bit word of the raw stream's bitmap per thread, 256 words per
// workgroup, never by run: an empty 1080p frame is one run of ~8000 tokens, a noise frame ~2 M runs of one.  A token belongs
// to the segment that holds its first byte.  Kernel boundaries separate the phases; no workgroup waits for another.
//   sizes (launch_png_deflate_sizes)
//     1. png_bitmap_kernel   reads the masks ONCE (16-byte loads, shifted to the segment) and writes the raw bitmap to the
//        scratch; per workgroup the last run start and the two Adler-32 partial sums (sum of bytes, position-weighted sum).
//        (launch_png_deflate_sizes_select: png_bitmap_select_kernel instead - the bitmap of the OR of selected row-major bit
//        planes at nested prefixes, one stream per (expression, level, frame); everything after it is the same code.)
//     2. png_count_kernel    bitmap -> bits of each segment's tokens, summed per workgroup, and the workgroup's first 7 bits.
//        The start of the run that enters a segment is a max-scan of run starts: inside the workgroup by shuffles, across
//        workgroups by reading back through kernel 1's per-workgroup values (almost always one step).
//     3. png_frame_kernel    one workgroup per frame: exclusive scan of the workgroups' bit counts, the frame's byte count,
//        Adler-32 reduced mod 65521.   4. png_offsets_kernel   byte counts -> dev_byte_off.
//   write (launch_png_deflate_write)
//     5. png_write_kernel    the same walk, tokens OR-ed into a zeroed LDS image of the workgroup's bytes (LDS atomics), which
//        is then stored with plain stores.  Every output byte has ONE owner: the workgroup that holds the byte's first
//        bit.  The owner of a byte that straddles two workgroups takes the missing (at most 7) bits from the first-7-bits
//        values of phase 2, so no global atomics and no zeroing of the output are needed.  Workgroup 0 adds the zlib and
//        block headers, the last one the end-of-block code, the padding and the Adler-32.
#include <algorithm>

#include "kernels.h"
#include "mask_elems.h"
#include "png_select.h"

namespace {

typedef unsigned long long u64;

constexpr int PNG_FRAMES = 65535;                     // frames per launch (grid.y); larger n is chunked
constexpr int PNG_SEG = 64;                           // raw bytes per thread
constexpr int PNG_GROUP_RAW = 256 * PNG_SEG;          // raw bytes per workgroup
constexpr int PNG_AHEAD = 5;                          // following words a segment may read: 64 + 261 <= 64 * (1 + PNG_AHEAD)
constexpr int PNG_LDS_WORDS = (19 + 9 * PNG_GROUP_RAW + 7 + 7) / 32 + 3;  // header bits + 9 bits per byte + end-of-block + padding
constexpr uint32_t PNG_BITS_MASK = 0xffffffu;         // info word: bits of the workgroup | first 7 bits << 24

struct PngArgs {
    const void* masks;
    long long npix;             // n*h*w
    int h, w;
    uint32_t R, W, NB;          // raw bytes, bitmap words, workgroups per frame
    int frame0, vec;            // vec: masks is 16-byte aligned
    u64* bitmap;                // [n, W]
    u64* s2;                    // [n, NB] sum of (R - p) over set raw bytes
    u64* bitoff;                // [n, NB] first token bit of the workgroup within the frame
    uint32_t* lasttr;           // [n, NB] 1 + last run start in the workgroup, 0 = none
    uint32_t* s1;               // [n, NB] set raw bytes
    uint32_t* info;             // [n, NB]
    long long* byte_off;
    uint32_t* adler;
    uint8_t* out;
};

// Pixels [c*CP, c*CP + CP) of the whole tensor -> CP bits; CP = pixels per 16 bytes.  The vector load is taken when the
// chunk lies inside the tensor and the tensor is 16-byte aligned, else guarded scalar loads.
template <int KIND>
__device__ __forceinline__ uint32_t chunk_bits(const typename mask_elem<KIND>::type* base, long long c, long long npix, bool vec) {
    constexpr int CP = 16 / mask_elem<KIND>::size;
    if (vec && (c + 1) * CP <= npix) return vec_bits<KIND>(*reinterpret_cast<const typename mask_elem<KIND>::vec*>(base + c * CP));
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < CP; ++i)
        if (c * CP + i < npix) b |= (uint32_t)mask_is_set<KIND>(base[c * CP + i]) << i;
    return b;
}

// `len` (1..64) consecutive pixels from `start` -> bits
template <int KIND>
__device__ __forceinline__ u64 fetch_bits(const typename mask_elem<KIND>::type* base, long long start, int len, long long npix, bool vec) {
    constexpr int CP = 16 / mask_elem<KIND>::size;
    long long c = start / CP;
    const int o = (int)(start - c * CP);
    u64 acc = 0;
    for (int got = -o; got < len; got += CP, ++c) {
        const u64 b = chunk_bits<KIND>(base, c, npix, vec);
        acc |= got < 0 ? b >> o : b << got;
    }
    return len < 64 ? acc & ((1ull << len) - 1ull) : acc;
}

__device__ __forceinline__ uint32_t ctz64(u64 v) { return (uint32_t)__ffsll((long long)v) - 1u; }

// 256-thread inclusive scan; `excl` = the scan without the thread's own value, `total` = the workgroup's.  Ends on a barrier.
template <typename V, typename Op>
__device__ __forceinline__ V block_scan(V v, V ident, Op op, V* lds, V& excl, V& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = op(inc, o);
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    V before = ident;
    total = ident;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const V s = lds[i];
        if (i < wave) before = op(before, s);
        total = op(total, s);
    }
    __syncthreads();
    const V prev = __shfl_up(inc, 1, 64);
    excl = lane ? op(before, prev) : before;
    return op(before, inc);
}

struct OpAdd {
    template <typename V>
    __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};
struct OpMax {
    template <typename V>
    __device__ __forceinline__ V operator()(V a, V b) const { return a > b ? a : b; }
};

// 1 + position of the last run start inside the word (bit i starts a run when it differs from bit i-1; raw byte 0 always
// does), 0 = none.
__device__ __forceinline__ uint32_t last_start(u64 B, uint32_t prevbit, uint32_t k, uint32_t p0, uint32_t nv, u64& T) {
    T = B ^ ((B << 1) | prevbit);
    if (k == 0) T |= 1ull;
    if (nv < 64) T &= (1ull << nv) - 1ull;
    return T ? p0 + (63u - (uint32_t)__clzll((long long)T)) + 1u : 0u;
}

// The workgroup's records of frame f after its bitmap words: the last run start and the two Adler-32 partial sums.  `prevbit` is
// the raw bit in front of the thread's word (0 in front of the frame's first).  Ends on a barrier.
__device__ __forceinline__ void group_records(const PngArgs a, int f, uint32_t blk, uint32_t k, uint32_t p0, uint32_t nv, u64 B,
                                              uint32_t prevbit, uint32_t* r32, u64* r64) {
    u64 tr;
    const uint32_t lt = last_start(B, prevbit, k, p0, nv, tr);
    // Adler-32 partial sums in units of 255: set bytes, and the sum of (R - p) over them
    const uint32_t cnt = (uint32_t)__popcll(B);
    const uint32_t widx = (uint32_t)__popcll(B & 0xaaaaaaaaaaaaaaaaull) + ((uint32_t)__popcll(B & 0xccccccccccccccccull) << 1) +
                          ((uint32_t)__popcll(B & 0xf0f0f0f0f0f0f0f0ull) << 2) + ((uint32_t)__popcll(B & 0xff00ff00ff00ff00ull) << 3) +
                          ((uint32_t)__popcll(B & 0xffff0000ffff0000ull) << 4) + ((uint32_t)__popcll(B & 0xffffffff00000000ull) << 5);
    const u64 w2 = cnt ? (u64)cnt * (u64)(a.R - p0) - widx : 0ull;
    uint32_t e32, tmax, tcnt;
    u64 e64, tw2;
    block_scan<uint32_t>(lt, 0u, OpMax(), r32, e32, tmax);
    block_scan<uint32_t>(cnt, 0u, OpAdd(), r32, e32, tcnt);
    block_scan<u64>(w2, 0ull, OpAdd(), r64, e64, tw2);
    if (threadIdx.x == 0) {
        const size_t i = (size_t)f * a.NB + blk;
        a.lasttr[i] = tmax;
        a.s1[i] = tcnt;
        a.s2[i] = tw2;
    }
}

// ---- phase 1 ------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void png_bitmap_kernel(const PngArgs a) {
    using T = typename mask_elem<KIND>::type;
    __shared__ uint32_t top[256];
    __shared__ uint32_t r32[4];
    __shared__ u64 r64[4];
    const int f = a.frame0 + blockIdx.y;
    const uint32_t blk = blockIdx.x, k = blk * 256u + threadIdx.x, p0 = k * PNG_SEG;
    const T* base = reinterpret_cast<const T*>(a.masks);
    const long long fpix = (long long)f * a.h * a.w;
    const uint32_t row = (uint32_t)a.w + 1u;
    u64 B = 0;
    uint32_t nv = 0;
    if (k < a.W) {
        nv = min((uint32_t)PNG_SEG, a.R - p0);
        uint32_t y = p0 / row, c = p0 - y * row, filled = 0;
        while (filled < nv) {
            if (c == 0) {  // the filter byte
                ++filled;
                c = 1;
                continue;
            }
            const uint32_t len = min(nv - filled, row - c);
            B |= fetch_bits<KIND>(base, fpix + (long long)y * a.w + (c - 1), (int)len, a.npix, a.vec != 0) << filled;
            filled += len;
            c += len;
            if (c == row) {
                c = 0;
                ++y;
            }
        }
        a.bitmap[(size_t)f * a.W + k] = B;
    }
    top[threadIdx.x] = (uint32_t)(B >> 63);
    __syncthreads();
    uint32_t prevbit = 0;
    if (threadIdx.x) prevbit = top[threadIdx.x - 1];
    else if (k > 0 && k < a.W) {  // the raw byte before this workgroup's first
        const uint32_t p = p0 - 1u, y = p / row, c = p - y * row;
        if (c) prevbit = mask_is_set<KIND>(base[fpix + (long long)y * a.w + (c - 1)]);
    }
    group_records(a, f, blk, k, p0, nv, B, prevbit, r32, r64);
}

// ---- phase 1 from bit planes: the OR of a selection of row-major planes, at up to SOLA_NESTED_MAX_LEVELS nested prefixes ----------
// One thread per 64-bit raw word of one (expression e, frame t); the grid is (workgroup of 256 words, t, e).  e's list is ordered so
// that the selection of level l is its prefix of end(e, l) entries (the rules of mask_nested_counts_kernel, jf.hip: ends clamped
// here to non-decreasing values within the list, a null level_end = the whole list, ids outside [0, n_masks) skipped).  The thread
// gathers its 64 raw bits from every plane that ENTERS at a level (png_select.h) and carries the OR over the levels in one
// register; at the end of each level it stores the word into stream (e*K + l)*T + t's bitmap and the workgroup leaves that stream's
// records.  Every plane of the largest selection is read once per (e, t); list and level reads are block-uniform.
struct PngSelArgs {
    const ps_u64* planes;  // [n_masks * T][nq]
    long long nq;          // 64-bit words of a plane
    int n_masks, T, K, e0, t0;
    const int *sel_off, *sel_idx, *level_end;
};

__global__ __launch_bounds__(256) void png_bitmap_select_kernel(const PngArgs a, const PngSelArgs s) {
    __shared__ uint32_t top[256];
    __shared__ uint32_t r32[4];
    __shared__ u64 r64[4];
    const int e = s.e0 + blockIdx.z, t = s.t0 + blockIdx.y;
    const uint32_t blk = blockIdx.x, k = blk * 256u + threadIdx.x, p0 = k * PNG_SEG;
    const PsWord wd = ps_word(k, a.W, a.R, (uint32_t)a.w + 1u);
    // the raw byte before this workgroup's first: its flat position, -1 = a filter byte or not this thread's to fetch
    const long long before = (threadIdx.x == 0 && k > 0 && k < a.W) ? ps_raw_to_flat(p0 - 1u, (uint32_t)a.w) : -1ll;
    const int l0 = s.sel_off[e], len = max(s.sel_off[e + 1] - l0, 0);
    const int* le = s.level_end ? s.level_end + (long long)e * s.K : nullptr;
    u64 B = 0;
    uint32_t pb = 0;
    int j = 0, prev = 0;
    for (int l = 0; l < s.K; ++l) {
        const int end = le ? min(max(le[l], prev), len) : len;
        for (; j < end; ++j) {
            const int m = s.sel_idx[l0 + j];
            if ((unsigned)m >= (unsigned)s.n_masks) continue;
            const ps_u64* plane = s.planes + ((long long)m * s.T + t) * s.nq;
            if (wd.nv) B |= ps_gather(plane, s.nq, wd, (uint32_t)a.w);
            if (before >= 0) pb |= (uint32_t)ps_fetch(plane, s.nq, before, 1);
        }
        prev = end;
        const int f = (e * s.K + l) * s.T + t;
        if (wd.nv) a.bitmap[(size_t)f * a.W + k] = B;
        top[threadIdx.x] = (uint32_t)(B >> 63);
        __syncthreads();
        const uint32_t prevbit = threadIdx.x ? top[threadIdx.x - 1] : pb;
        group_records(a, f, blk, k, p0, wd.nv, B, prevbit, r32, r64);  // (ends on a barrier: top is free again)
    }
}

// ---- the token walk -------------------------------------------------------------------------------------------------------
struct CountSink {
    uint32_t bits = 0, head = 0;
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb) {
        if (bits < 7) head |= v << bits;
        bits += nb;
    }
};

struct WriteSink {
    uint32_t* lds;
    uint32_t wi, fill;
    u64 acc = 0;
    __device__ __forceinline__ WriteSink(uint32_t* l, uint32_t bit) : lds(l), wi(bit >> 5), fill(bit & 31u) {}
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb) {
        acc |= (u64)v << fill;
        fill += nb;
        if (fill >= 32) {
            if (wi < (uint32_t)PNG_LDS_WORDS) atomicOr(&lds[wi], (uint32_t)acc);
            acc >>= 32;
            fill -= 32;
            ++wi;
        }
    }
    __device__ __forceinline__ void flush() {
        if (fill && wi < (uint32_t)PNG_LDS_WORDS) atomicOr(&lds[wi], (uint32_t)acc);
    }
};

// Huffman codes go in most significant bit first, everything else least significant first: codes are bit-reversed here
template <class Sink>
__device__ __forceinline__ void put_literal(Sink& sink, uint32_t v) {
    if (v) sink.put(0x1ffu, 9);  // 0xFF: 9-bit code 110010000 + 111
    else sink.put(0x0cu, 8);     // 0x00: 8-bit code 00110000
}

template <class Sink>
__device__ __forceinline__ void put_match(Sink& sink, uint32_t len) {  // length 3..258 at distance 1 (5-bit code 00000)
    uint32_t sym, e = 0, extra = 0;
    if (len == 258) sym = 285;
    else if (len <= 10) sym = 254 + len;
    else {
        const uint32_t x = len - 3;
        e = 29u - (uint32_t)__clz((int)x);
        sym = 261 + 4 * e + ((x >> e) & 3u);
        extra = x & ((1u << e) - 1u);
    }
    const uint32_t nb = sym < 280 ? 7u : 8u;
    const uint32_t code = sym < 280 ? sym - 256 : 0xc0u + (sym - 280);
    sink.put((__brev(code) >> (32 - nb)) | extra << nb, nb + e + 5);
}

// Tokens that start in raw bytes [p0, p0 + nv) of a frame; B = those bytes as bits, s = start of the run that holds p0.
template <class Sink>
__device__ __forceinline__ void walk_word(Sink& sink, u64 B, uint32_t p0, uint32_t nv, uint32_t s, const u64* __restrict__ fw,
                                          uint32_t k, uint32_t W, uint32_t R) {
    uint32_t i = 0;
    while (i < nv) {
        const uint32_t v = (uint32_t)(B >> i) & 1u;
        const u64 diff = (v ? ~B : B) >> i;
        const uint32_t j = min(diff ? i + ctz64(diff) : 64u, nv);
        uint32_t e = p0 + j;
        bool open = false;  // the run's end lies beyond what was read: it is at least 261 past every token start here
        if (j == nv && p0 + nv < R) {
            open = true;
            for (uint32_t a = 1; a <= (uint32_t)PNG_AHEAD; ++a) {
                if (k + a >= W) {
                    open = false;
                    break;
                }
                const uint32_t q0 = p0 + a * PNG_SEG, valid = min((uint32_t)PNG_SEG, R - q0);
                const u64 word = fw[k + a];
                u64 d = v ? ~word : word;
                if (valid < 64) d |= ~0ull << valid;
                if (d) {
                    e = q0 + ctz64(d);
                    open = false;
                    break;
                }
                e = q0 + PNG_SEG;
            }
        }
        const uint32_t lo = p0 + i, hi = p0 + j;
        if (s >= lo) put_literal(sink, v);
        const uint32_t kk = s >= lo ? 0u : (lo - s - 1u + 257u) / 258u;
        const uint32_t t = s + 1u + 258u * kk;
        if (t < hi) {
            const uint32_t Lk = e - t;
            if (open || Lk >= 261 || Lk == 258) put_match(sink, 258);
            else if (Lk >= 259) put_match(sink, Lk - 3);
            else if (Lk >= 3) put_match(sink, Lk);
            else if (kk == 0) put_literal(sink, v);
        }
        if (!open) {
            const uint32_t L = e - s - 1u;
            if (L == 2 && s + 2 >= lo && s + 2 < hi) put_literal(sink, v);
            if (L >= 259) {
                const uint32_t m = L % 258u;
                if ((m == 1 || m == 2) && e - 3 >= lo && e - 3 < hi) put_match(sink, 3);
            }
        }
        i = j;
        s = p0 + j;
    }
}

// The thread's word of the bitmap and the start of the run that enters it.
__device__ __forceinline__ void load_word(const PngArgs& a, int f, uint32_t blk, uint32_t* r32, u64& B, uint32_t& p0, uint32_t& nv,
                                          uint32_t& s) {
    const u64* fw = a.bitmap + (size_t)f * a.W;
    const uint32_t k = blk * 256u + threadIdx.x;
    p0 = k * PNG_SEG;
    const bool in = k < a.W;
    B = in ? fw[k] : 0ull;
    nv = in ? min((uint32_t)PNG_SEG, a.R - p0) : 0u;
    const uint32_t prevbit = (in && k > 0) ? (uint32_t)(fw[k - 1] >> 63) : 0u;
    u64 tr;
    const uint32_t lt = last_start(B, prevbit, k, p0, nv, tr);
    uint32_t before, total;
    block_scan<uint32_t>(lt, 0u, OpMax(), r32, before, total);
    // earlier workgroups of the frame, nearest first; raw byte 0 starts a run, so the search ends
    uint32_t carry = 0;
    const uint32_t* lasttr = a.lasttr + (size_t)f * a.NB;
    for (uint32_t top = blk; top > 0 && carry == 0; top = top > 256 ? top - 256 : 0) {
        const uint32_t v = threadIdx.x < top ? lasttr[top - 1 - threadIdx.x] : 0u;
        uint32_t e;
        block_scan<uint32_t>(v, 0u, OpMax(), r32, e, carry);
    }
    s = (tr & 1ull) ? p0 : max(before, carry) - 1u;
}

// ---- phase 2 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_count_kernel(const PngArgs a) {
    __shared__ uint32_t r32[4];
    __shared__ uint32_t head7;
    const int f = a.frame0 + blockIdx.y;
    const uint32_t blk = blockIdx.x;
    if (threadIdx.x == 0) head7 = 0;
    u64 B;
    uint32_t p0, nv, s;
    load_word(a, f, blk, r32, B, p0, nv, s);  // (barriers inside: head7 is visible)
    CountSink sink;
    walk_word(sink, B, p0, nv, s, a.bitmap + (size_t)f * a.W, blk * 256u + threadIdx.x, a.W, a.R);
    uint32_t off, total;
    block_scan<uint32_t>(sink.bits, 0u, OpAdd(), r32, off, total);
    if (sink.bits && off < 7) atomicOr(&head7, (sink.head << off) & 0x7fu);
    __syncthreads();
    if (threadIdx.x == 0) a.info[(size_t)f * a.NB + blk] = total | head7 << 24;
}

// ---- phase 3: one workgroup per frame -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_frame_kernel(const PngArgs a) {
    __shared__ u64 r64[4];
    const int f = a.frame0 + blockIdx.x;
    const size_t o = (size_t)f * a.NB;
    u64 carry = 0, c1 = 0, c2 = 0;
    for (uint32_t base = 0; base < a.NB; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < a.NB;
        const u64 v = in ? (u64)(a.info[o + i] & PNG_BITS_MASK) : 0ull;
        u64 ex, total;
        block_scan<u64>(v, 0ull, OpAdd(), r64, ex, total);
        if (in) {
            a.bitoff[o + i] = carry + ex;
            c1 += a.s1[o + i];
            c2 += a.s2[o + i];
        }
        carry += total;
    }
    u64 ex, t1, t2;
    block_scan<u64>(c1, 0ull, OpAdd(), r64, ex, t1);
    block_scan<u64>(c2, 0ull, OpAdd(), r64, ex, t2);  // < R^2 / 2 + R < 2^63
    if (threadIdx.x == 0) {
        // 2 zlib header bytes; 3 block header bits, tokens, 7 end-of-block bits, padded to a byte; 4 Adler-32 bytes
        a.byte_off[f + 1] = (long long)((19ull + carry + 7ull + 7ull) >> 3) + 4ll;
        const u64 A = (1ull + 255ull * t1) % 65521ull;
        const u64 Bs = ((u64)a.R + 255ull * (t2 % 65521ull)) % 65521ull;
        a.adler[f] = (uint32_t)(Bs << 16 | A);
    }
}

// One workgroup: off[1..n] (per-frame sizes) -> inclusive prefix sums, off[0] = 0.
__global__ __launch_bounds__(256) void png_offsets_kernel(long long* off, int n) {
    __shared__ long long lds[4];
    long long carry = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long i = base + threadIdx.x;
        const long long v = i < n ? off[1 + i] : 0ll;
        long long ex, total;
        const long long inc = block_scan<long long>(v, 0ll, OpAdd(), lds, ex, total);
        if (i < n) off[1 + i] = carry + inc;
        carry += total;
    }
    if (threadIdx.x == 0) off[0] = 0;
}

// ---- phase 5 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_write_kernel(const PngArgs a) {
    __shared__ uint32_t buf[PNG_LDS_WORDS];
    __shared__ uint32_t r32[4];
    const int f = a.frame0 + blockIdx.y;
    const uint32_t blk = blockIdx.x;
    const size_t o = (size_t)f * a.NB;
    const bool last = blk + 1 == a.NB;
    const uint32_t nbits = a.info[o + blk] & PNG_BITS_MASK;
    const u64 Pb = 19ull + a.bitoff[o + blk], Pn = Pb + nbits;  // the workgroup's bits within the frame's stream
    const long long fbase = a.byte_off[f];
    long long fsize = a.byte_off[f + 1] - fbase;
    if (fsize < 6) return;  // offsets that do not belong to this bitmap: nothing is stored
    const u64 base_byte = blk ? Pb >> 3 : 0ull;          // frame byte of buf's byte 0
    const u64 first = blk ? (Pb + 7) >> 3 : 0ull;        // owned frame bytes [first, end)
    u64 end = last ? (u64)(fsize - 4) : (Pn + 7) >> 3;
    end = min(end, (u64)(fsize - 4));
    end = min(end, base_byte + 4ull * (PNG_LDS_WORDS - 1));
    const uint32_t bit0 = (uint32_t)(Pb - 8ull * base_byte);
    uint32_t nz = (bit0 + nbits + 31u) / 32u + 2u;
    if (end > base_byte) nz = max(nz, (uint32_t)((end - base_byte + 3) >> 2) + 1u);
    nz = min(nz, (uint32_t)PNG_LDS_WORDS);
    for (uint32_t i = threadIdx.x; i < nz; i += 256) buf[i] = (blk == 0 && i == 0) ? 0x030178u : 0u;  // 78 01, BFINAL=1 BTYPE=01
    u64 B;
    uint32_t p0, nv, s;
    load_word(a, f, blk, r32, B, p0, nv, s);  // (barriers inside: buf is zeroed)
    const u64* fw = a.bitmap + (size_t)f * a.W;
    const uint32_t k = blk * 256u + threadIdx.x;
    CountSink cnt;
    walk_word(cnt, B, p0, nv, s, fw, k, a.W, a.R);
    uint32_t off, total;
    block_scan<uint32_t>(cnt.bits, 0u, OpAdd(), r32, off, total);
    if (total != nbits) return;  // a scratch that changed since the sizes call (uniform): nothing is stored
    WriteSink sink(buf, bit0 + off);
    walk_word(sink, B, p0, nv, s, fw, k, a.W, a.R);
    sink.flush();
    if (threadIdx.x == 0 && !last && (Pn & 7ull) && end > first) {
        // the last owned byte ends in the following workgroups' bits (zeros after the frame's last: end-of-block)
        uint32_t need = 8u - (uint32_t)(Pn & 7ull), pos = 0, val = 0;
        for (uint32_t j = blk + 1; j < a.NB && need; ++j) {
            const uint32_t inf = a.info[o + j];
            const uint32_t take = min(need, inf & PNG_BITS_MASK);
            val |= ((inf >> 24) & ((1u << take) - 1u)) << pos;
            pos += take;
            need -= take;
        }
        const uint32_t bit = bit0 + nbits;
        if ((bit >> 5) < (uint32_t)PNG_LDS_WORDS) atomicOr(&buf[bit >> 5], val << (bit & 31u));  // (bit & 7) + 7 bits stay inside the word's byte
    }
    __syncthreads();
    if (end > first) {
        uint8_t* dst = a.out + fbase + (long long)first;
        const uint32_t lb0 = (uint32_t)(first - base_byte), nbytes = (uint32_t)(end - first);
        const uint32_t headb = min(nbytes, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
        const uint32_t nd = (nbytes - headb) >> 2, tailb = nbytes - headb - 4u * nd;
        if (threadIdx.x < headb) dst[threadIdx.x] = (uint8_t)(buf[(lb0 + threadIdx.x) >> 2] >> (((lb0 + threadIdx.x) & 3u) * 8u));
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst + headb);
        for (uint32_t j = threadIdx.x; j < nd; j += 256) {
            const uint32_t lb = lb0 + headb + 4u * j, wi = lb >> 2, sh = (lb & 3u) * 8u;
            dw[j] = sh ? (buf[wi] >> sh) | (buf[wi + 1] << (32u - sh)) : buf[wi];
        }
        if (threadIdx.x < tailb) {
            const uint32_t lb = lb0 + headb + 4u * nd + threadIdx.x;
            dst[headb + 4u * nd + threadIdx.x] = (uint8_t)(buf[lb >> 2] >> ((lb & 3u) * 8u));
        }
    }
    if (last && threadIdx.x < 4) a.out[fbase + fsize - 4 + threadIdx.x] = (uint8_t)(a.adler[f] >> (24u - 8u * threadIdx.x));
}

struct Layout {
    uint32_t R, W, NB;
    size_t bitmap, s2, bitoff, lasttr, s1, info, total;
};

Layout layout(int n, int h, int w) {
    Layout l{};
    l.R = (uint32_t)((long long)h * ((long long)w + 1));
    l.W = (l.R + PNG_SEG - 1) / PNG_SEG;
    l.NB = (l.W + 255) / 256;
    const size_t groups = (size_t)n * l.NB;
    size_t o = 0;
    l.bitmap = o; o += (size_t)n * l.W * 8;
    l.s2 = o; o += groups * 8;
    l.bitoff = o; o += groups * 8;
    l.lasttr = o; o += groups * 4;
    l.s1 = o; o += groups * 4;
    l.info = o; o += groups * 4;
    l.total = (o + 255) & ~(size_t)255;
    return l;
}

int check_sizes(const char* what, int elem_type, int n, int h, int w, size_t scratch_bytes) {
    SOLA_TRY(check_mask_sizes(what, elem_type, n, h, w));
    SOLA_ARG((long long)h * ((long long)w + 1) < (1ll << 31), "%s: image too large (h*(w+1) must be < 2^31)", what);
    const size_t need = png_deflate_scratch_bytes(n, h, w);
    SOLA_ARG(need > 0, "%s: sizes overflow n=%d h=%d w=%d", what, n, h, w);
    SOLA_ARG(scratch_bytes >= need, "%s: scratch %zu bytes < required %zu", what, scratch_bytes, need);
    return SOLA_OK;
}

PngArgs make_args(const void* masks, int n, int h, int w, void* scratch) {
    const Layout l = layout(n, h, w);
    char* sc = static_cast<char*>(scratch);
    PngArgs a{};
    a.masks = masks;
    a.npix = (long long)n * h * w;
    a.h = h; a.w = w; a.R = l.R; a.W = l.W; a.NB = l.NB;
    a.vec = (reinterpret_cast<uintptr_t>(masks) & 15) == 0;
    a.bitmap = reinterpret_cast<u64*>(sc + l.bitmap);
    a.s2 = reinterpret_cast<u64*>(sc + l.s2);
    a.bitoff = reinterpret_cast<u64*>(sc + l.bitoff);
    a.lasttr = reinterpret_cast<uint32_t*>(sc + l.lasttr);
    a.s1 = reinterpret_cast<uint32_t*>(sc + l.s1);
    a.info = reinterpret_cast<uint32_t*>(sc + l.info);
    return a;
}

}  // namespace

size_t png_deflate_scratch_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    if ((long long)h * ((long long)w + 1) >= (1ll << 31)) return 0;
    const Layout l = layout(n, h, w);
    if ((double)n * ((double)l.W * 8.0 + (double)l.NB * 28.0) > 9.0e18) return 0;
    return l.total;
}

int launch_png_deflate_sizes(const void* masks, int elem_type, int n, int h, int w, long long* byte_off, uint32_t* adler,
                             void* scratch, size_t scratch_bytes, hipStream_t s) {
    SOLA_TRY(check_sizes("png_deflate_sizes", elem_type, n, h, w, scratch_bytes));
    PngArgs a = make_args(masks, n, h, w, scratch);
    a.byte_off = byte_off;
    a.adler = adler;
    for (int f0 = 0; f0 < n; f0 += PNG_FRAMES) {
        a.frame0 = f0;
        const unsigned nf = (unsigned)std::min(PNG_FRAMES, n - f0);
        const dim3 grid(a.NB, nf), block(256);
        with_mask_kind<MASK_LOGIT>(elem_type, [&](auto kind) {
            hipLaunchKernelGGL(png_bitmap_kernel<decltype(kind)::value>, grid, block, 0, s, a);
        });
        SOLA_LAUNCH_CHECK();
        hipLaunchKernelGGL(png_count_kernel, grid, block, 0, s, a);
        SOLA_LAUNCH_CHECK();
        hipLaunchKernelGGL(png_frame_kernel, dim3(nf), block, 0, s, a);
        SOLA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, s, byte_off, n);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_png_deflate_sizes_select(const uint32_t* bits, long long words_stride, int n_masks, int T, int h, int w, const int* sel_off,
                                    const int* sel_idx, const int* level_end, int K, int E, long long* byte_off, uint32_t* adler,
                                    void* scratch, size_t scratch_bytes, hipStream_t s) {
    const char* what = "png_deflate_sizes_select";
    SOLA_ARG(K >= 1 && E >= 1 && T >= 1 && h >= 1 && w >= 1 && n_masks >= 0 && K <= SOLA_NESTED_MAX_LEVELS,
             "%s: bad sizes K=%d (1..%d) E=%d T=%d n_masks=%d h=%d w=%d", what, K, SOLA_NESTED_MAX_LEVELS, E, T, n_masks, h, w);
    SOLA_ARG(level_end || K == 1, "%s: null level_end needs K == 1", what);
    SOLA_ARG((long long)E * K * T < (1ll << 31), "%s: E*K*T too large (must be < 2^31)", what);
    const int n = E * K * T;
    SOLA_ARG((long long)h * ((long long)w + 1) < (1ll << 31), "%s: image too large (h*(w+1) must be < 2^31)", what);
    SOLA_ARG(words_stride % 4 == 0 && words_stride >= sola_mask_words(h, w), "%s: words_stride %lld must be a multiple of 4 and >= %lld", what,
             words_stride, (long long)sola_mask_words(h, w));
    SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 15) == 0, "%s: planes must be 16-byte aligned", what);
    SOLA_TRY(check_sizes(what, 0, n, h, w, scratch_bytes));
    PngArgs a = make_args(bits, n, h, w, scratch);
    a.byte_off = byte_off;
    a.adler = adler;
    PngSelArgs sel{};
    sel.planes = reinterpret_cast<const ps_u64*>(bits);
    sel.nq = words_stride / 2;
    sel.n_masks = n_masks; sel.T = T; sel.K = K;
    sel.sel_off = sel_off; sel.sel_idx = sel_idx; sel.level_end = level_end;
    for (int e0 = 0; e0 < E; e0 += PNG_FRAMES)  // gridDim.y, gridDim.z <= 65535
        for (int t0 = 0; t0 < T; t0 += PNG_FRAMES) {
            sel.e0 = e0; sel.t0 = t0;
            const dim3 grid(a.NB, (unsigned)std::min(PNG_FRAMES, T - t0), (unsigned)std::min(PNG_FRAMES, E - e0));
            hipLaunchKernelGGL(png_bitmap_select_kernel, grid, dim3(256), 0, s, a, sel);
            SOLA_LAUNCH_CHECK();
        }
    for (int f0 = 0; f0 < n; f0 += PNG_FRAMES) {
        a.frame0 = f0;
        const unsigned nf = (unsigned)std::min(PNG_FRAMES, n - f0);
        hipLaunchKernelGGL(png_count_kernel, dim3(a.NB, nf), dim3(256), 0, s, a);
        SOLA_LAUNCH_CHECK();
        hipLaunchKernelGGL(png_frame_kernel, dim3(nf), dim3(256), 0, s, a);
        SOLA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, s, byte_off, n);
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

int launch_png_deflate_write(const void* masks, int elem_type, int n, int h, int w, const long long* byte_off,
                             const uint32_t* adler, uint8_t* bytes, void* scratch, size_t scratch_bytes, hipStream_t s) {
    SOLA_TRY(check_sizes("png_deflate_write", elem_type, n, h, w, scratch_bytes));
    PngArgs a = make_args(masks, n, h, w, scratch);
    a.byte_off = const_cast<long long*>(byte_off);
    a.adler = const_cast<uint32_t*>(adler);
    a.out = bytes;
    for (int f0 = 0; f0 < n; f0 += PNG_FRAMES) {
        a.frame0 = f0;
        const dim3 grid(a.NB, (unsigned)std::min(PNG_FRAMES, n - f0)), block(256);
        hipLaunchKernelGGL(png_write_kernel, grid, block, 0, s, a);
        SOLA_LAUNCH_CHECK();
    }
    return SOLA_OK;
}
