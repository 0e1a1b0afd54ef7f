// Index maps (one byte per pixel, the value is the object id: the palette PNGs of Ref-DAVIS / Ref-YouTube-VOS) -> the packed
// layouts of the rest of the library, from ONE read of the maps (dataloader.py:260-276 load_gt_masklet and
// track_generation/seg_utils.py:29-49 get_masklets_ytbvos do up to 255 `masks == obj_id` passes on the host).
//
// sola_index_hist: idx [T,h,w] uint8 -> counts int64 [T,256].  hipMemsetAsync of the table, then index_hist_kernel: one block
//   of 256 threads per IH_CHUNK_BYTES (64 KiB) piece of ONE frame.  16-byte loads wherever the absolute ADDRESS is 16-byte
//   aligned (any w, any base: only the < 16 bytes at either end of a piece are read byte by byte, mask_elems.h's mask_piece).  A
//   lane counts RUNS of equal bytes and carries the open run from vector to vector, so a frame of one value costs a lane one
//   LDS atomic, not one per pixel.  One LDS histogram per wave (4 x 256 uint32; a block sees at most 65536 pixels), folded by
//   thread b = bin b into the table with one 64-bit integer atomicAdd per non-zero bin.
//
// sola_index_pack: plane (first_plane ? first_plane[k] : k*T) + t = (idx[t] == ids[k]).  Both layouts stage their piece of
//   frame t as BYTES in LDS so that a plane word is 32 CONSECUTIVE LDS bytes, and share everything after that:
//     layout 0 (row-major, iou.hip's mask_pack format): a block owns IPR_WORDS = 256 words = 8192 pixels of the raster.  The
//       piece is copied with 16-byte loads and ds_write_b128 at the same offset mod 16 as its address (edges byte by byte).
//     layout 1 (column-major, jf.hip's format, position = x*h + y): a block owns a strip of `cw` whole columns of frame t and
//       stages them TRANSPOSED, LDS byte (x - x0)*h + y: 8 lanes per row read the row's 16-byte-aligned blocks (coalesced,
//       edges byte by byte) and each scatters its 16 bytes with ds_write_b8.  A column is not word-aligned when h % 32 != 0,
//       so a word may run into the next column(s): every word has exactly ONE owner, the strip that holds its first bit
//       (png_write_kernel's rule for straddling bytes), and a strip also stages the ceil(31 / h) columns after its own that
//       its last word can reach.  No global atomics on the planes, no memset of them.  cw = 64 while (64 + extra) * h fits
//       IPC_LDS_BUDGET (80 KiB: h <= 1259 keeps 64 columns and two blocks per CU), halved until it fits for taller frames
//       (the slower path: shorter row segments), down to one column at SOLA_INDEX_MAX_H.
//   Then, for every chunk of SOLA_INDEX_ID_CHUNK ids (held in SGPRs, the loop over them unrolled): a thread takes the words it
//   owns, reads the 9 LDS dwords around a word's 32 bytes, aligns them with v_alignbit, and for each id turns the 8 dwords
//   into 32 bits (xor with the id in every byte, zero-byte test, 4 flag bits gathered per dword) and stores the word.  The
//   maps are read from memory once for all K ids; a further chunk re-reads LDS only.  The last block of a frame also writes
//   the pad words up to words_stride as zeros; tail bits are masked.  area (optional): a kernel zeroes the addressed entries,
//   then the waves add their popcounts with 64-bit integer atomics.  Identical from run to run.
#include <algorithm>

#include "kernels.h"
#include "mask_elems.h"

namespace {

typedef unsigned long long u64;

// ----------------------------------------------------------------------------------------------------------- histogram
constexpr int IH_THREADS = 256;
constexpr int IH_CHUNK_BYTES = 64 * 1024;
constexpr int IH_BATCH = 4;  // 16-byte loads in flight per lane

struct HistRun {
    uint32_t value = 0, n = 0;
    __device__ __forceinline__ void byte(uint32_t b, uint32_t* hist) {
        if (b == value) { ++n; return; }
        if (n) atomicAdd(&hist[value], n);
        value = b;
        n = 1;
    }
    __device__ __forceinline__ void dword(uint32_t d, uint32_t* hist) {
        byte(d & 255u, hist); byte((d >> 8) & 255u, hist); byte((d >> 16) & 255u, hist); byte(d >> 24, hist);
    }
    __device__ __forceinline__ void flush(uint32_t* hist) {
        if (n) atomicAdd(&hist[value], n);
        n = 0;
    }
};

__global__ __launch_bounds__(IH_THREADS) void index_hist_kernel(const uint8_t* __restrict__ idx, long long hw, int chunks, int base_mod,
                                                                u64* __restrict__ counts) {
    __shared__ uint32_t hist[IH_THREADS / 64][256];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < (IH_THREADS / 64) * 256; i += IH_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int m = (int)(blockIdx.x / (unsigned)chunks);
    const int c = (int)(blockIdx.x - (unsigned)m * (unsigned)chunks);
    const long long first = (long long)m * hw;
    const int lo = c * IH_CHUNK_BYTES;  // < hw < 2^31
    const int hi = (int)min((long long)lo + IH_CHUNK_BYTES, hw);
    const MaskPiece pc = mask_piece<16>(base_mod, first, lo, hi);
    const int v_lo = pc.v_lo, n_vec = pc.n_vec;
    uint32_t* mine = hist[wave];
    HistRun run;

    if (tid < pc.n_edge) run.byte(idx[first + (tid < pc.n_head ? lo + tid : pc.v_hi + (tid - pc.n_head))], mine);

    if (tid < n_vec) {
        const uint4* src = reinterpret_cast<const uint4*>(idx + first + v_lo) + tid;
        for (int k0 = 0; k0 * IH_THREADS < n_vec; k0 += IH_BATCH) {
            // a vector past the end re-reads the piece's last one and is not counted
            uint4 data[IH_BATCH];
#pragma unroll
            for (int j = 0; j < IH_BATCH; ++j) data[j] = src[(size_t)min((k0 + j) * IH_THREADS, n_vec - 1 - tid)];
#pragma unroll
            for (int j = 0; j < IH_BATCH; ++j) {
                if (tid + (k0 + j) * IH_THREADS < n_vec) {
                    run.dword(data[j].x, mine); run.dword(data[j].y, mine); run.dword(data[j].z, mine); run.dword(data[j].w, mine);
                }
            }
        }
    }
    run.flush(mine);
    __syncthreads();
    u64 total = 0;
#pragma unroll
    for (int j = 0; j < IH_THREADS / 64; ++j) total += hist[j][tid];
    if (total) atomicAdd(counts + (long long)m * 256 + tid, total);
}

// ---------------------------------------------------------------------------------------------------------------- pack
constexpr int IDC = SOLA_INDEX_ID_CHUNK;
constexpr int IPR_THREADS = 256;
constexpr int IPR_WORDS = 256;               // words of a row-major block
constexpr int IPR_BYTES = IPR_WORDS * 32;    // = its pixels
constexpr int IP_LDS_TAIL = 48;              // a word's 9 dwords may reach 35 bytes past the last staged byte
constexpr int IPC_THREADS = 512;
constexpr int IPC_COLS = 64;
constexpr int IPC_LDS_BUDGET = 80 * 1024;    // two blocks in a CU's 160 KiB
static_assert(2 * SOLA_INDEX_MAX_H + IP_LDS_TAIL + 16 <= IPC_LDS_BUDGET, "one column and the one after it fit at the height limit");

struct PackArgs {
    const uint8_t* idx;
    const int32_t* ids;
    const int32_t* first_plane;
    uint32_t* bits;
    u64* area;
    long long hw, stride, n_words;  // pixels of a frame, words of a plane, words that hold pixels
    int T, h, w, K;
    int parts;                      // blocks per frame: row-major pieces / column strips
    int cw, extra;                  // layout 1: columns a strip owns, columns after them it may need
};

// flags of the bytes of x that are ZERO, as 4 bits: the complement of mask_elems.h's nz_byte_bits, kept apart because
// nz_byte_bits(x) ^ 15 here makes the pack kernels 8 to 13 % longer (profiles/mask_elems_isa.txt)
__device__ __forceinline__ uint32_t ip_zero_bytes(uint32_t x) {
    uint32_t z = ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x)) & 0x80808080u;  // bit 7 of every zero byte
    z >>= 7;        // bits 0, 8, 16, 24
    z |= z >> 7;    // + 1, 9, 17
    z |= z >> 14;   // + 2, 3
    return z & 15u;
}

// The words i_lo + tid, + THREADS, ... < i_hi of frame t, for every id: word i is the 32 bytes at lds + off0 + 32 * (i - i_lo).
template <int THREADS, bool AREA>
__device__ __forceinline__ void ip_emit(const PackArgs& a, const uint32_t* lds32, int t, long long i_lo, long long i_hi, uint32_t off0) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < a.K; k0 += IDC) {
        uint32_t pat[IDC];
        long long plane[IDC];  // the id's plane of this frame, < 0: nothing to write
        bool none[IDC];        // an id no byte can hold: empty planes
#pragma unroll
        for (int j = 0; j < IDC; ++j) {
            const int k = min(k0 + j, a.K - 1);
            const int id = a.ids[k];
            const long long first = a.first_plane ? (long long)a.first_plane[k] : (long long)k * a.T;
            none[j] = (unsigned)id >= 256u;
            pat[j] = (uint32_t)(id & 255) * 0x01010101u;
            plane[j] = (k0 + j < a.K && first >= 0) ? first + t : -1;
        }
        uint32_t pop[IDC];
#pragma unroll
        for (int j = 0; j < IDC; ++j) pop[j] = 0;
        for (long long base = i_lo; base < i_hi; base += THREADS) {  // uniform trip count: the reduction below is wave-wide
            const long long i = base + tid;
            const bool live = i < i_hi;
            const long long left = a.hw - i * 32;  // pixels from the word's first bit on
            uint32_t d[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] = 0;
            uint32_t mask = 0;
            if (live && left > 0) {
                mask = left >= 32 ? 0xffffffffu : (1u << (int)left) - 1u;
                const uint32_t o = off0 + (uint32_t)(i - i_lo) * 32u;
                const uint32_t* p = lds32 + (o >> 2);
                const uint32_t sh = (o & 3u) * 8u;
                uint32_t r[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) r[q] = p[q];
#pragma unroll
                for (int q = 0; q < 8; ++q) d[q] = (uint32_t)((((u64)r[q + 1] << 32) | r[q]) >> sh);
            }
#pragma unroll
            for (int j = 0; j < IDC; ++j) {
                if (plane[j] < 0) continue;  // uniform
                uint32_t word = 0;
                if (!none[j]) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) word |= ip_zero_bytes(d[q] ^ pat[j]) << (4 * q);
                    word &= mask;
                }
                if (live) a.bits[plane[j] * a.stride + i] = word;
                if constexpr (AREA) pop[j] += __popc(word);
            }
        }
        if constexpr (AREA) {
#pragma unroll
            for (int j = 0; j < IDC; ++j) {
                if (plane[j] < 0) continue;
                uint32_t v = pop[j];  // a block holds fewer than 2^24 pixels
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if ((tid & 63) == 0 && v) atomicAdd(a.area + plane[j], (u64)v);
            }
        }
    }
}

template <bool AREA>
__global__ __launch_bounds__(IPR_THREADS) void index_pack_rm_kernel(const PackArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds32[(IPR_BYTES + 16 + IP_LDS_TAIL) / 4];
    uint8_t* lds8 = reinterpret_cast<uint8_t*>(lds32);
    const int tid = threadIdx.x;
    const int t = (int)(blockIdx.x / (unsigned)a.parts);
    const int part = (int)(blockIdx.x - (unsigned)t * (unsigned)a.parts);
    const long long lo = (long long)part * IPR_BYTES;
    const int len = (int)max(0ll, min((long long)IPR_BYTES, a.hw - lo));
    const uint8_t* src = a.idx + (long long)t * a.hw + lo;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    if (len > 0) {
        const int n_blk = (mis + len + 15) / 16;  // 16-byte-aligned blocks that hold bytes of the piece
        for (int b = tid; b < n_blk; b += IPR_THREADS) {
            const int c0 = 16 * b - mis;  // the block's first byte, counted from the piece's
            if (c0 >= 0 && c0 + 16 <= len) {
                reinterpret_cast<uint4*>(lds32)[b] = *reinterpret_cast<const uint4*>(src + c0);
            } else {
                for (int j = 0; j < 16; ++j)
                    if (c0 + j >= 0 && c0 + j < len) lds8[16 * b + j] = src[c0 + j];
            }
        }
    }
    __syncthreads();
    const long long i_lo = (long long)part * IPR_WORDS;
    const long long i_hi = part == a.parts - 1 ? a.stride : i_lo + IPR_WORDS;
    ip_emit<IPR_THREADS, AREA>(a, lds32, t, i_lo, i_hi, (uint32_t)mis);
}

template <bool AREA>
__global__ __launch_bounds__(IPC_THREADS) void index_pack_cm_kernel(const PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ipc_lds[];
    uint8_t* lds8 = reinterpret_cast<uint8_t*>(ipc_lds);
    const int tid = threadIdx.x;
    const int t = (int)(blockIdx.x / (unsigned)a.parts);
    const int strip = (int)(blockIdx.x - (unsigned)t * (unsigned)a.parts);
    const int h = a.h, w = a.w;
    const int x0 = strip * a.cw, x1 = min(w, x0 + a.cw);
    const int n = x1 - x0 + min(w - x1, a.extra);  // staged columns, <= cw + extra
    const uint8_t* frame = a.idx + (long long)t * a.hw;

    // 8 lanes per row: lane b of a row takes the b-th 16-byte-aligned block that holds bytes of the row's n
    constexpr int ROWS = IPC_THREADS / 8;
    constexpr int BATCH = 4;
    const int r = tid >> 3, b = tid & 7;
    for (int y0 = 0; y0 < h; y0 += ROWS * BATCH) {
        uint4 data[BATCH];
        int c0[BATCH], kind[BATCH];  // kind 0: nothing, 1: byte by byte, 2: data[] holds the block
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
            const int y = y0 + q * ROWS + r;
            kind[q] = 0;
            c0[q] = 0;
            data[q] = make_uint4(0, 0, 0, 0);
            if (y < h) {
                const uint8_t* src = frame + (long long)y * w + x0;
                c0[q] = 16 * b - (int)(reinterpret_cast<uintptr_t>(src) & 15);  // the block's first byte as a column of the strip
                if (c0[q] < n && c0[q] + 16 > 0) {
                    kind[q] = (c0[q] >= 0 && c0[q] + 16 <= n) ? 2 : 1;
                    if (kind[q] == 2) data[q] = *reinterpret_cast<const uint4*>(src + c0[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
            const int y = y0 + q * ROWS + r;
            if (kind[q] == 2) {
                uint8_t* dst = lds8 + c0[q] * h + y;
                const uint32_t dw[4] = {data[q].x, data[q].y, data[q].z, data[q].w};
#pragma unroll
                for (int j = 0; j < 16; ++j) dst[j * h] = (uint8_t)(dw[j >> 2] >> (8 * (j & 3)));
            } else if (kind[q] == 1) {
                const uint8_t* src = frame + (long long)y * w + x0;
                for (int j = 0; j < 16; ++j) {
                    const int c = c0[q] + j;
                    if (c >= 0 && c < n) lds8[c * h + y] = src[c];
                }
            }
        }
    }
    __syncthreads();
    const long long pos0 = (long long)x0 * h, pos1 = (long long)x1 * h;
    const long long i_lo = (pos0 + 31) / 32;  // the words whose first bit lies in columns x0 .. x1 - 1
    const long long i_hi = strip == a.parts - 1 ? a.stride : (pos1 + 31) / 32;
    ip_emit<IPC_THREADS, AREA>(a, ipc_lds, t, i_lo, i_hi, (uint32_t)(i_lo * 32 - pos0));
}

__global__ __launch_bounds__(256) void index_area_zero_kernel(const int32_t* __restrict__ first_plane, int K, int T, u64* __restrict__ area) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)K * T) return;
    const int k = (int)(i / T), t = (int)(i - (long long)k * T);
    const long long plane = first_plane ? (long long)first_plane[k] : (long long)k * T;
    if (plane >= 0) area[plane + t] = 0;
}

}  // namespace

extern "C" int sola_index_hist(const uint8_t* idx, int T, int h, int w, int64_t* counts, void* stream_) {
    SOLA_ARG(T >= 0 && h >= 0 && w >= 0, "index_hist: negative size (T %d, h %d, w %d)", T, h, w);
    if (T == 0) return SOLA_OK;
    const long long hw = (long long)h * w;
    SOLA_ARG(hw < (1ll << 31), "index_hist: h*w = %lld >= 2^31", hw);
    SOLA_ARG(counts, "index_hist: null counts");
    SOLA_ARG((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "index_hist: counts must be 8-byte aligned");
    const long long chunks = (hw + IH_CHUNK_BYTES - 1) / IH_CHUNK_BYTES;
    const long long blocks = chunks * T;
    SOLA_ARG(blocks < (1ll << 31), "index_hist: %lld pieces of %d bytes, at most 2^31 - 1 in one call", blocks, IH_CHUNK_BYTES);
    if (hw > 0) SOLA_ARG(idx, "index_hist: null idx");
    hipStream_t s = as_stream(stream_);
    SOLA_HIP(hipMemsetAsync(counts, 0, (size_t)T * 256 * sizeof(int64_t), s));
    if (hw == 0) return SOLA_OK;
    hipLaunchKernelGGL(index_hist_kernel, dim3((unsigned)blocks), dim3(IH_THREADS), 0, s, idx, hw, (int)chunks,
                       (int)(reinterpret_cast<uintptr_t>(idx) & 15), reinterpret_cast<u64*>(counts));
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}

extern "C" int sola_index_pack(const uint8_t* idx, int T, int h, int w, const int32_t* ids, int K, const int32_t* first_plane, int layout,
                               int64_t words_stride, uint32_t* bits, int64_t* area, void* stream_) {
    SOLA_ARG(T >= 0 && h >= 0 && w >= 0 && K >= 0, "index_pack: negative size (T %d, h %d, w %d, K %d)", T, h, w, K);
    SOLA_ARG(layout == 0 || layout == 1, "index_pack: layout %d is neither 0 (row-major) nor 1 (column-major)", layout);
    if (T == 0 || K == 0) return SOLA_OK;
    const long long hw = (long long)h * w;
    SOLA_ARG(hw < (1ll << 31), "index_pack: h*w = %lld >= 2^31", hw);
    SOLA_ARG(ids, "index_pack: null ids");
    SOLA_ARG(bits, "index_pack: null bits");
    if (hw > 0) SOLA_ARG(idx, "index_pack: null idx");
    const long long n_words = (hw + 31) / 32;
    if (layout == 0) {
        SOLA_ARG(words_stride >= n_words, "index_pack: words_stride %lld must be >= %lld", (long long)words_stride, n_words);
        SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 3) == 0, "index_pack: planes must be 4-byte aligned");
    } else {
        SOLA_ARG(h <= SOLA_INDEX_MAX_H, "index_pack: h = %d, at most %d rows in the column-major layout", h, SOLA_INDEX_MAX_H);
        SOLA_ARG(words_stride >= sola_jf_plane_words(h, w) && words_stride % 4 == 0,
                 "index_pack: words_stride %lld must be a multiple of 4 and >= %lld", (long long)words_stride,
                 (long long)sola_jf_plane_words(h, w));
        SOLA_ARG((reinterpret_cast<uintptr_t>(bits) & 15) == 0, "index_pack: planes must be 16-byte aligned");
    }
    SOLA_ARG(words_stride < (1ll << 40), "index_pack: words_stride %lld too large", (long long)words_stride);
    if (area) SOLA_ARG((reinterpret_cast<uintptr_t>(area) & 7) == 0, "index_pack: area must be 8-byte aligned");
    PackArgs a{};
    a.idx = idx; a.ids = ids; a.first_plane = first_plane; a.bits = bits; a.area = reinterpret_cast<u64*>(area);
    a.hw = hw; a.stride = words_stride; a.n_words = n_words;
    a.T = T; a.h = h; a.w = w; a.K = K;
    size_t lds = 0;
    const bool columns = layout == 1 && hw > 0;  // (an empty frame has no pixel order: its planes are pad words alone)
    if (columns) {
        a.extra = (31 + h - 1) / h;
        a.cw = IPC_COLS;
        auto need = [&](int cw) { return ((size_t)std::min(w, cw + a.extra) * h + IP_LDS_TAIL + 15) / 16 * 16; };
        while (a.cw > 1 && need(a.cw) > (size_t)IPC_LDS_BUDGET) a.cw >>= 1;
        lds = need(a.cw);
        a.parts = (w + a.cw - 1) / a.cw;
    } else {
        a.parts = (int)std::max(1ll, (n_words + IPR_WORDS - 1) / IPR_WORDS);
    }
    const long long blocks = (long long)a.parts * T;
    SOLA_ARG(blocks < (1ll << 31), "index_pack: %lld blocks, at most 2^31 - 1 in one call", blocks);
    hipStream_t s = as_stream(stream_);
    if (area) {
        const long long n = (long long)K * T;
        hipLaunchKernelGGL(index_area_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, first_plane, K, T, a.area);
        SOLA_LAUNCH_CHECK();
    }
    if (words_stride == 0) return SOLA_OK;  // (empty frames in planes without pad words)
    if (columns) {
        static DeviceOnce once;
        int dev;
        if (once.needed(&dev)) {
            SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&index_pack_cm_kernel<false>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, IPC_LDS_BUDGET));
            SOLA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&index_pack_cm_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, IPC_LDS_BUDGET));
            once.done(dev);
        }
        if (area) hipLaunchKernelGGL(index_pack_cm_kernel<true>, dim3((unsigned)blocks), dim3(IPC_THREADS), lds, s, a);
        else hipLaunchKernelGGL(index_pack_cm_kernel<false>, dim3((unsigned)blocks), dim3(IPC_THREADS), lds, s, a);
    } else {
        if (area) hipLaunchKernelGGL(index_pack_rm_kernel<true>, dim3((unsigned)blocks), dim3(IPR_THREADS), 0, s, a);
        else hipLaunchKernelGGL(index_pack_rm_kernel<false>, dim3((unsigned)blocks), dim3(IPR_THREADS), 0, s, a);
    }
    SOLA_LAUNCH_CHECK();
    return SOLA_OK;
}
