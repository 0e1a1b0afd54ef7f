// The per-thread steps of resample.hip's kernels as host/device functions of the thread index: the kernels call them between their
// barriers, and tools/micro/resample_tile_host.hip runs the same code on the host, thread by thread, over plain arrays in place of
// the LDS (under AddressSanitizer: every index of every geometry is checked without a GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sola_hip.h"

#define RS_HD __host__ __device__ __forceinline__

constexpr int RS_BITS = 22;
constexpr int RS_TW = SOLA_RESAMPLE_TILE_W, RS_TH = SOLA_RESAMPLE_TILE_H;
constexpr int RS_THREADS = 512;  // eight waves: the tap loops wait on LDS reads, a CU holds two blocks
constexpr int RS_LDS_BUDGET = 56 * 1024;  // dynamic; + 4 KiB static: two blocks in a CU's 160 KiB, no function attribute needed
constexpr int RS_MIN_CHUNK = 8;           // fewer source rows per staging round than this (or than the tile needs): two launches
static_assert(RS_TW == 64 && RS_TH == 64, "the planar rows of mid[] are 64 bytes and bx / by hold 64 entries");

RS_HD int rs_min(int a, int b) { return a < b ? a : b; }
RS_HD int rs_max(int a, int b) { return a > b ? a : b; }
RS_HD int rs_clip8(int acc) { return rs_min(rs_max(acc >> RS_BITS, 0), 255); }

// row `o` of an axis table [out][2 + taps]: (first source index, taps used, k...); a null table is the identity
RS_HD int2 rs_bounds(const int32_t* __restrict__ tab, int taps, int o) {
    if (!tab) return make_int2(o, 1);
    const int32_t* row = tab + (long long)o * (2 + taps);
    return make_int2(row[0], row[1]);
}

struct ResampleArgs {
    const uint8_t* src;
    const int32_t *tab_x, *tab_y;
    const float* lut;
    void* out;
    int T, H, W, h, w;
    int taps_x, taps_y;        // 1 for a null table
    int span_cap, rows_cap;    // source columns / rows a tile can need (rs_plan)
    int rows_chunk;            // source rows staged at a time (raw[] holds that many; mid[] holds all rows_cap)
    int tiles_x, tiles_y;
    int raw_pitch;             // bytes of a staged source row, a multiple of 16
    int vec;                   // LUT: float4 stores are aligned
    uint32_t off_ky, off_raw, off_mid;  // byte offsets into the dynamic LDS (kx at 0)
};

// a block's view of its LDS and of its tile
struct RsTile {
    int2 *bx, *by;   // [RS_TW], [RS_TH]: the table's bounds of the tile's columns / rows
    int32_t *kx, *ky;
    uint8_t *raw, *mid;
    float* lut_s;
    int t, ox0, oy0, ncols, nrows_out;
    // the source window, known after step 0
    int x_lo, span, y_lo, nrows, mis0, step;
    const uint8_t* src0;
};

RS_HD void rs_tile_init(RsTile& s, const ResampleArgs& a, unsigned block, uint8_t* lds8, int2* bx, int2* by, float* lut_s) {
    s.bx = bx; s.by = by; s.lut_s = lut_s;
    s.kx = reinterpret_cast<int32_t*>(lds8);
    s.ky = reinterpret_cast<int32_t*>(lds8 + a.off_ky);
    s.raw = lds8 + a.off_raw;
    s.mid = lds8 + a.off_mid;
    const int txi = (int)(block % (unsigned)a.tiles_x);
    const int rest = (int)(block / (unsigned)a.tiles_x);
    const int tyi = rest % a.tiles_y;
    s.t = rest / a.tiles_y;
    s.ox0 = txi * RS_TW; s.oy0 = tyi * RS_TH;
    s.ncols = rs_min(RS_TW, a.w - s.ox0); s.nrows_out = rs_min(RS_TH, a.h - s.oy0);
}

// ---- 0: bounds, coefficients, table -> LDS
template <int C, bool LUT>
RS_HD void rs_tile_load_tables(const RsTile& s, const ResampleArgs& a, int tid) {
    const int taps_x = a.taps_x, taps_y = a.taps_y;
    if (tid < s.ncols) s.bx[tid] = rs_bounds(a.tab_x, taps_x, s.ox0 + tid);
    if (tid >= 64 && tid - 64 < s.nrows_out) s.by[tid - 64] = rs_bounds(a.tab_y, taps_y, s.oy0 + tid - 64);
    for (int i = tid; i < s.ncols * taps_x; i += RS_THREADS) {
        const int o = i / taps_x, j = i - o * taps_x;
        s.kx[i] = a.tab_x ? a.tab_x[(long long)(s.ox0 + o) * (2 + taps_x) + 2 + j] : (1 << RS_BITS);
    }
    for (int i = tid; i < s.nrows_out * taps_y; i += RS_THREADS) {
        const int o = i / taps_y, j = i - o * taps_y;
        s.ky[i] = a.tab_y ? a.tab_y[(long long)(s.oy0 + o) * (2 + taps_y) + 2 + j] : (1 << RS_BITS);
    }
    if constexpr (LUT)
        for (int i = tid; i < C * 256; i += RS_THREADS) s.lut_s[i] = a.lut[i];
}

// (after a barrier) the source window of the tile: bounds ascend with the output index; never more than the launch sized the LDS
// for, never outside the source - whatever the tables hold
template <int C>
RS_HD void rs_tile_window(RsTile& s, const ResampleArgs& a) {
    const int2 x_last = s.bx[s.ncols - 1], y_last = s.by[s.nrows_out - 1];
    s.x_lo = rs_min(rs_max(s.bx[0].x, 0), a.W);
    s.span = rs_min(rs_min(rs_max(x_last.x + x_last.y, s.x_lo), a.W) - s.x_lo, a.span_cap);
    s.y_lo = rs_min(rs_max(s.by[0].x, 0), a.H);
    s.nrows = rs_min(rs_min(rs_max(y_last.x + y_last.y, s.y_lo), a.H) - s.y_lo, a.rows_cap);
    s.src0 = a.src + (((long long)s.t * a.H + s.y_lo) * a.W + s.x_lo) * C;
    s.mis0 = (int)(reinterpret_cast<uintptr_t>(s.src0) & 15);
    s.step = (int)(((long long)a.W * C) & 15);
}

// ---- 1: the source rows r0 .. r0 + nr of the window -> raw[(r - r0) * raw_pitch + mis_r + byte of the row piece]: a row sits at the
// same offset mod 16 as its address
template <int C>
RS_HD void rs_tile_stage(const RsTile& s, const ResampleArgs& a, int tid, int r0, int nr) {
    const int len = s.span * C;
    const long long row_bytes = (long long)a.W * C;
    const int nb = a.raw_pitch / 16;
    for (int it = tid; it < nr * nb; it += RS_THREADS) {
        const int rr = it / nb, b = it - rr * nb;
        const int r = r0 + rr;
        const int mis = (s.mis0 + r * s.step) & 15;
        if (b * 16 >= mis + len) continue;
        const uint8_t* srow = s.src0 + r * row_bytes;
        uint8_t* drow = s.raw + rr * a.raw_pitch;
        const int c0 = 16 * b - mis;  // the block's first byte, counted from the row piece's
        if (c0 >= 0 && c0 + 16 <= len) {
            *reinterpret_cast<uint4*>(drow + 16 * b) = *reinterpret_cast<const uint4*>(srow + c0);
        } else {
            for (int j = 0; j < 16; ++j)
                if (c0 + j >= 0 && c0 + j < len) drow[16 * b + j] = srow[c0 + j];
        }
    }
}

// ---- 2: horizontal pass of those rows, raw -> mid[(c * rows_cap + r) * RS_TW + column].  A thread keeps its output column (tid & 63:
// its window and its coefficient row are found once) and walks the source rows, all C channels on one read of the coefficient
template <int C>
RS_HD void rs_tile_horizontal(const RsTile& s, const ResampleArgs& a, int tid, int r0, int nr) {
    const int i = tid & (RS_TW - 1);
    if (i >= s.ncols) return;
    const int2 b = s.bx[i];
    const int start = rs_min(rs_max(b.x - s.x_lo, 0), s.span);
    const int n = rs_min(rs_max(b.y, 0), rs_min(a.taps_x, s.span - start));
    const int32_t* k = s.kx + i * a.taps_x;
    for (int rr = tid / RS_TW; rr < nr; rr += RS_THREADS / RS_TW) {
        const int r = r0 + rr;
        const uint8_t* p = s.raw + rr * a.raw_pitch + ((s.mis0 + r * s.step) & 15) + start * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_BITS - 1);
#pragma unroll 4
        for (int j = 0; j < n; ++j) {  // (four taps' LDS reads in flight)
            const int kk = k[j];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[j * C + c] * kk;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) s.mid[(c * a.rows_cap + r) * RS_TW + i] = (uint8_t)rs_clip8(acc[c]);
    }
}

// ---- 3: vertical pass and epilogue.  Table: four neighbouring columns of a channel are one dword of mid per tap and one float4 of
// the planar output; bytes: one thread per output byte, consecutive lanes consecutive bytes
template <int C, bool LUT>
RS_HD void rs_tile_vertical(const RsTile& s, const ResampleArgs& a, int tid) {
    if constexpr (LUT) {
        float* out = reinterpret_cast<float*>(a.out);
        for (int it = tid; it < s.nrows_out * C * (RS_TW / 4); it += RS_THREADS) {
            const int q = it & (RS_TW / 4 - 1), rc = it / (RS_TW / 4);
            const int oyi = rc / C, c = rc - oyi * C;
            const int ox = s.ox0 + 4 * q;
            if (ox >= a.w) continue;
            const int2 b = s.by[oyi];
            const int start = rs_min(rs_max(b.x - s.y_lo, 0), s.nrows);
            const int n = rs_min(rs_max(b.y, 0), rs_min(a.taps_y, s.nrows - start));
            const uint32_t* p = reinterpret_cast<const uint32_t*>(s.mid + (c * a.rows_cap + start) * RS_TW) + q;
            const int32_t* k = s.ky + oyi * a.taps_y;
            int acc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = 1 << (RS_BITS - 1);
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const int kk = k[j];
                const uint32_t d = p[j * (RS_TW / 4)];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (int)((d >> (8 * e)) & 255u) * kk;
            }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = s.lut_s[c * 256 + rs_clip8(acc[e])];
            float* dst = out + (((long long)s.t * C + c) * a.h + s.oy0 + oyi) * a.w + ox;
            if (a.vec) {  // w % 4 == 0: the four columns exist
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ox + e < a.w) dst[e] = v[e];
            }
        }
    } else {
        uint8_t* out = reinterpret_cast<uint8_t*>(a.out);
        const int rowb = s.ncols * C;
        for (int oyi = tid / 64; oyi < s.nrows_out; oyi += RS_THREADS / 64) {  // a wave per output row
            const int2 b = s.by[oyi];
            const int start = rs_min(rs_max(b.x - s.y_lo, 0), s.nrows);
            const int n = rs_min(rs_max(b.y, 0), rs_min(a.taps_y, s.nrows - start));
            const int32_t* k = s.ky + oyi * a.taps_y;
            uint8_t* dst = out + (((long long)s.t * a.h + s.oy0 + oyi) * a.w + s.ox0) * C;
            for (int jj = tid & 63; jj < rowb; jj += 64) {
                const int i = jj / C, c = jj - i * C;
                const uint8_t* p = s.mid + (c * a.rows_cap + start) * RS_TW + i;
                int acc = 1 << (RS_BITS - 1);
#pragma unroll 4
                for (int j = 0; j < n; ++j) acc += (int)p[j * RS_TW] * k[j];
                dst[jj] = (uint8_t)rs_clip8(acc);
            }
        }
    }
}

// One pass of the two-launch route, one thread per output element.  src [T,Hs,Ws,C] bytes; VERT = false resamples x into
// uint8 [T,Hs,n_out,C]; VERT = true resamples y into [T,n_out,Ws,C] bytes or, with a table, float32 planar [T,C,n_out,Ws].
struct PassArgs {
    const uint8_t* src;
    const int32_t* tab;
    const float* lut;
    void* out;
    long long total;  // output elements
    int Hs, Ws, C, n_out, taps;
};

template <bool VERT>
RS_HD void rs_pass_element(const PassArgs& a, long long idx) {
    const int C = a.C;
    const int ow = VERT ? a.Ws : a.n_out, oh = VERT ? a.n_out : a.Hs;
    const int c = (int)(idx % C);
    long long rest = idx / C;
    const int x = (int)(rest % ow);
    rest /= ow;
    const int y = (int)(rest % oh);
    const long long t = rest / oh;
    const int n_in = VERT ? a.Hs : a.Ws;
    const int o = VERT ? y : x;
    const int2 b = rs_bounds(a.tab, a.taps, o);
    const int first = rs_min(rs_max(b.x, 0), n_in);
    const int n = rs_min(rs_max(b.y, 0), rs_min(a.taps, n_in - first));
    const int32_t* k = a.tab ? a.tab + (long long)o * (2 + a.taps) + 2 : nullptr;
    const long long stride = VERT ? (long long)a.Ws * C : C;
    const uint8_t* p = a.src + ((t * a.Hs + (VERT ? first : y)) * a.Ws + (VERT ? x : first)) * C + c;
    int acc = 1 << (RS_BITS - 1);
    for (int j = 0; j < n; ++j) acc += (int)p[j * stride] * (k ? k[j] : (1 << RS_BITS));
    const int v = rs_clip8(acc);
    if (VERT && a.lut) reinterpret_cast<float*>(a.out)[((t * C + c) * oh + y) * ow + x] = a.lut[c * 256 + v];
    else reinterpret_cast<uint8_t*>(a.out)[idx] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------------------------- planning (host)
struct RsPlan {
    bool fused;
    int span_cap, rows_cap, raw_pitch, rows_chunk;
    uint32_t off_ky, off_raw, off_mid;
    size_t lds;
};
// source indices that `tile` consecutive outputs can touch: first(o + k) - first(o) <= k * in / out + 1, plus the taps of the last
inline long long rs_window(int tile, int in, int out, int taps, bool identity) {
    const int n = tile < out ? tile : out;
    if (identity) return n;
    const long long need = ((long long)(n - 1) * in + out - 1) / out + taps + 1;
    return need < in ? need : in;
}
inline RsPlan rs_plan(int H, int W, int C, int h, int w, int taps_x, int taps_y, bool id_x, bool id_y) {
    RsPlan p{};
    const long long span = rs_window(RS_TW, W, w, taps_x, id_x), rows = rs_window(RS_TH, H, h, taps_y, id_y);
    const long long pitch = (span * C + 30 + 15) / 16 * 16;  // a row piece starts up to 15 bytes in and ends inside a 16-byte block
    const long long kx = (long long)(RS_TW < w ? RS_TW : w) * taps_x * 4, ky = (long long)(RS_TH < h ? RS_TH : h) * taps_y * 4;
    const long long off_raw = (kx + ky + 15) / 16 * 16;
    // mid[] holds every source row of the tile (the vertical pass needs them all), raw[] as many as still fit: the rows are staged
    // and resampled horizontally RS_MIN_CHUNK or more at a time
    const long long mid = (long long)C * rows * RS_TW;
    const long long left = (long long)RS_LDS_BUDGET - off_raw - mid;
    const long long chunk = left < pitch ? 0 : (left / pitch < rows ? left / pitch : rows);
    const long long off_mid = off_raw + chunk * pitch;
    const long long total = off_mid + mid;
    p.fused = chunk >= (rows < RS_MIN_CHUNK ? rows : RS_MIN_CHUNK);
    if (p.fused) {
        p.span_cap = (int)span; p.rows_cap = (int)rows; p.raw_pitch = (int)pitch; p.rows_chunk = (int)chunk;
        p.off_ky = (uint32_t)kx; p.off_raw = (uint32_t)off_raw; p.off_mid = (uint32_t)off_mid;
        p.lds = (size_t)total;
    }
    return p;
}
// the launch arguments of the one-launch route
inline ResampleArgs rs_fused_args(const RsPlan& p, const uint8_t* src, int T, int H, int W, int h, int w, const int32_t* table_x, int taps_x,
                                  const int32_t* table_y, int taps_y, const float* lut, void* out) {
    ResampleArgs a{};
    a.src = src; a.tab_x = table_x; a.tab_y = table_y; a.lut = lut; a.out = out;
    a.T = T; a.H = H; a.W = W; a.h = h; a.w = w;
    a.taps_x = taps_x > 1 ? taps_x : 1; a.taps_y = taps_y > 1 ? taps_y : 1;
    a.span_cap = p.span_cap; a.rows_cap = p.rows_cap; a.raw_pitch = p.raw_pitch; a.rows_chunk = p.rows_chunk;
    a.off_ky = p.off_ky; a.off_raw = p.off_raw; a.off_mid = p.off_mid;
    a.tiles_x = (w + RS_TW - 1) / RS_TW; a.tiles_y = (h + RS_TH - 1) / RS_TH;
    a.vec = lut && w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    return a;
}
