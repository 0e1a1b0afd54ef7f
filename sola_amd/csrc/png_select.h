// The bit-gather arithmetic of png_select.hip (column-major planes -> row-major planes) and of png_encode.hip's
// png_bitmap_select_kernel (row-major planes -> the raw-stream bitmap of a PNG frame) as host/device functions: the kernels call
// them, and tools/micro/png_select_host.hip runs the same code on the host over heap arrays of exactly the plane sizes (under
// AddressSanitizer: every index of every geometry is checked without a GPU).
//
// Every bit array here is read as 64-bit words, bit j of word i = position 64*i + j.  On a little-endian machine that is the
// layout of the 32-bit planes of include/sola_hip.h (bit j of uint32 word i = position 32*i + j) whenever the plane holds an even
// number of uint32 words and starts on 8 bytes; the planes' strides are multiples of 4 words and they start on 16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PS_HD __host__ __device__ __forceinline__

typedef unsigned long long ps_u64;

constexpr int PS_ROWS = 64;  // image rows a workgroup of the transpose stages: one bit of a lane's 64-bit column piece each

PS_HD long long ps_min(long long a, long long b) { return a < b ? a : b; }

// `len` (1..64) bits from position `start` of an array of nq words; positions behind the array read as 0, no word outside
// [0, nq) is touched, and the second word is loaded only when the piece reaches into it
PS_HD ps_u64 ps_fetch(const ps_u64* q, long long nq, long long start, int len) {
    const long long i = start >> 6;
    const int o = (int)(start & 63);
    ps_u64 v = i < nq ? q[i] >> o : 0ull;
    if (o + len > 64 && i + 1 < nq) v |= q[i + 1] << (64 - o);
    return len < 64 ? v & ((1ull << len) - 1ull) : v;
}

// ---- row-major plane -> raw stream of a PNG frame --------------------------------------------------------------------------------
// Raw byte p of an h x w frame, row = w + 1: y = p / row, c = p - y * row; c == 0 is the filter byte (always 0), else it is the
// pixel at flat position y*w + c - 1.  Word k of the frame's bitmap holds raw bytes [64k, 64k + nv).
struct PsWord {
    uint32_t y, c, nv;  // row and column-within-the-raw-row of the word's first byte, valid bytes (0: the word is outside the frame)
};

PS_HD PsWord ps_word(uint32_t k, uint32_t nwords, uint32_t R, uint32_t row) {
    PsWord wd{0u, 0u, 0u};
    if (k >= nwords) return wd;
    const uint32_t p0 = k * 64u;
    wd.nv = R - p0 < 64u ? R - p0 : 64u;
    wd.y = p0 / row;
    wd.c = p0 - wd.y * row;
    return wd;
}

// the word's raw bits from one plane: pieces of one or more image rows at shifted offsets, the filter bytes between them stay 0
PS_HD ps_u64 ps_gather(const ps_u64* plane, long long nq, PsWord wd, uint32_t w) {
    const uint32_t row = w + 1u;
    ps_u64 B = 0;
    uint32_t y = wd.y, c = wd.c, filled = 0;
    while (filled < wd.nv) {
        if (c == 0) {  // the filter byte
            ++filled;
            c = 1;
            continue;
        }
        const uint32_t len = wd.nv - filled < row - c ? wd.nv - filled : row - c;
        B |= ps_fetch(plane, nq, (long long)y * w + (c - 1), (int)len) << filled;
        filled += len;
        c += len;
        if (c == row) {
            c = 0;
            ++y;
        }
    }
    return B;
}

// flat position of raw byte p, -1 for a filter byte
PS_HD long long ps_raw_to_flat(uint32_t p, uint32_t w) {
    const uint32_t row = w + 1u, y = p / row, c = p - y * row;
    return c ? (long long)y * w + (c - 1) : -1ll;
}

// ---- column-major plane -> row-major plane -----------------------------------------------------------------------------------
// A workgroup takes image rows [y0, y1), y1 - y0 <= PS_ROWS.  Lane l of a wave loads rows y0.. of column x as one piece of the
// column-major plane (position x*h + y0: any bit offset, aligned by ps_fetch's funnel shift); 64 ballots turn 64 columns into 64
// row words, kept in a tile of (y1 - y0) rows x pitch64 words.  The workgroup then OWNS the output words whose first bit lies in its
// rows, [ps_first_word(y0), ps_first_word(y1)): one writer per word.  The last of them may reach up to 31 bits past row y1 - 1;
// those bits come one by one from the column-major plane (ps_rm_rest).
PS_HD ps_u64 ps_column(const ps_u64* cm, long long nq, int x, int h, int y0, int rows) {
    return ps_fetch(cm, nq, (long long)x * h + y0, rows);
}

PS_HD long long ps_first_word(int y, int w) { return ((long long)y * w + 31) >> 5; }

// bits [32*i, 32*i + 32) of the row-major plane that lie in rows [y0, y1), from the tile (32*i >= y0*w)
PS_HD uint32_t ps_rm_word(const ps_u64* tile, int pitch64, long long i, int w, int y0, int y1) {
    const long long first = 32 * i, end = ps_min(first + 32, (long long)y1 * w);
    long long pos = first;
    int y = (int)(pos / w), c = (int)(pos - (long long)y * w);
    uint32_t out = 0;
    while (pos < end) {
        const int len = (int)ps_min(end - pos, w - c);
        out |= (uint32_t)ps_fetch(tile, (long long)(y1 - y0) * pitch64, (long long)(y - y0) * pitch64 * 64 + c, len) << (int)(pos - first);
        pos += len;
        c = 0;
        ++y;
    }
    return out;
}

// ... and its bits at or behind row y1 (below h*w), from the column-major plane itself
PS_HD uint32_t ps_rm_rest(const ps_u64* cm, long long nq, long long i, int w, int h, int y1) {
    const long long first = 32 * i, end = ps_min(first + 32, (long long)h * w);
    uint32_t out = 0;
    for (long long pos = (long long)y1 * w > first ? (long long)y1 * w : first; pos < end; ++pos) {
        const int y = (int)(pos / w), x = (int)(pos - (long long)y * w);
        out |= (uint32_t)ps_fetch(cm, nq, (long long)x * h + y, 1) << (int)(pos - first);
    }
    return out;
}
