// The bit-gather arithmetic of sola_amd/csrc/png_select.h on the HOST: the column-major -> row-major transpose (the ballots of
// planes_cm_to_rm_kernel restated bit by bit, everything else the kernel's own functions, workgroup by workgroup and word by word)
// and the raw-word gather of png_bitmap_select_kernel, over heap arrays of exactly the plane sizes, against a naive per-pixel
// restatement.  Built with AddressSanitizer on the host side, every index of every geometry is checked without a GPU:
//   make -C tools/micro png_select_host && tools/micro/png_select_host
// (runs no kernel and opens no device).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../sola_amd/csrc/png_select.h"

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static long long round4(long long x) { return (x + 3) & ~3ll; }

static int g_bad = 0;
static void fail(const char* what, int h, int w, long long at) {
    if (g_bad++ < 20) printf("MISMATCH %s h=%d w=%d at %lld\n", what, h, w, at);
}

// mode 0: noise, 1: all ones, 2: all zeros, 3: sparse
static void run(int h, int w, int mode, int rows_cap) {
    const long long hw = (long long)h * w;
    std::vector<uint8_t> pix((size_t)hw);
    for (long long i = 0; i < hw; ++i) pix[(size_t)i] = mode == 1 ? 1 : mode == 2 ? 0 : mode == 3 ? (rnd() % 97 == 0) : (rnd() & 1);
    // exactly the minimal strides of the two layouts, as uint32 words
    const long long stride_cm = round4((hw + 31) / 32), stride_rm = round4((hw + 31) / 32);
    const long long nq_cm = stride_cm / 2, nq_rm = stride_rm / 2;
    ps_u64* cm = (ps_u64*)calloc((size_t)nq_cm, 8);
    uint32_t* rm = (uint32_t*)malloc((size_t)stride_rm * 4);
    for (long long i = 0; i < stride_rm; ++i) rm[i] = 0xffffffffu;  // unwritten or dirty words show
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            if (pix[(size_t)y * w + x]) {
                const long long pos = (long long)x * h + y;
                cm[pos >> 6] |= 1ull << (pos & 63);
            }
    // ---- the transpose, workgroup by workgroup
    const int pitch64 = (int)((((long long)w + 63) >> 6) | 1);
    const int rows = rows_cap < PS_ROWS ? rows_cap : PS_ROWS;
    std::vector<int> writers((size_t)stride_rm, 0);
    for (int y0 = 0; y0 < h; y0 += rows) {
        const int y1 = y0 + rows < h ? y0 + rows : h, ry = y1 - y0;
        ps_u64* tile = (ps_u64*)malloc((size_t)ry * pitch64 * 8);  // exactly the rows in use; the pad column is never written
        for (int i = 0; i < ry * pitch64; ++i) tile[i] = 0xa5a5a5a5a5a5a5a5ull;
        for (int xt = 0; xt < (w + 63) / 64; ++xt) {
            ps_u64 col[64];
            for (int lane = 0; lane < 64; ++lane) col[lane] = xt * 64 + lane < w ? ps_column(cm, nq_cm, xt * 64 + lane, h, y0, ry) : 0ull;
            for (int r = 0; r < ry; ++r) {  // lane r keeps ballot r
                ps_u64 b = 0;
                for (int lane = 0; lane < 64; ++lane) b |= ((col[lane] >> r) & 1ull) << lane;
                tile[r * pitch64 + xt] = b;
            }
        }
        const long long w0 = ps_first_word(y0, w), w1 = ps_first_word(y1, w);
        for (long long i = w0; i < w1; ++i) {
            uint32_t v = ps_rm_word(tile, pitch64, i, w, y0, y1);
            if (i == w1 - 1 && y1 < h) v |= ps_rm_rest(cm, nq_cm, i, w, h, y1);
            rm[i] = v;
            ++writers[(size_t)i];
        }
        if (y1 == h)
            for (long long i = w1; i < stride_rm; ++i) {
                rm[i] = 0;
                ++writers[(size_t)i];
            }
        free(tile);
    }
    for (long long i = 0; i < stride_rm; ++i) {
        uint32_t want = 0;
        for (int j = 0; j < 32; ++j)
            if (32 * i + j < hw && pix[(size_t)(32 * i + j)]) want |= 1u << j;
        if (rm[i] != want) fail("rm word", h, w, i);
        if (writers[(size_t)i] != 1) fail("writers of a word", h, w, i);
    }
    // ---- the raw-word gather over the row-major plane just made
    const uint32_t row = (uint32_t)w + 1u, R = (uint32_t)((long long)h * row), W = (R + 63) / 64;
    const ps_u64* plane = (const ps_u64*)rm;
    for (uint32_t k = 0; k < W + 3; ++k) {  // (words behind the frame: nv = 0, nothing is read)
        const PsWord wd = ps_word(k, W, R, row);
        const ps_u64 got = wd.nv ? ps_gather(plane, nq_rm, wd, (uint32_t)w) : 0ull;
        ps_u64 want = 0;
        for (uint32_t j = 0; j < 64; ++j) {
            const unsigned long long p = 64ull * k + j;
            if (k >= W || p >= R) break;
            const uint32_t y = (uint32_t)(p / row), c = (uint32_t)(p % row);
            if (c && pix[(size_t)y * w + (c - 1)]) want |= 1ull << j;
        }
        if (got != want) fail("raw word", h, w, k);
        if (k > 0 && k < W) {  // the raw byte in front of a word
            const long long flat = ps_raw_to_flat(64u * k - 1u, (uint32_t)w);
            const uint32_t p = 64u * k - 1u, y = p / row, c = p % row;
            const uint32_t wantb = c ? pix[(size_t)y * w + (c - 1)] : 0u;
            const uint32_t gotb = flat >= 0 ? (uint32_t)ps_fetch(plane, nq_rm, flat, 1) : 0u;
            if ((flat < 0) != (c == 0) || gotb != wantb) fail("previous raw bit", h, w, k);
        }
    }
    free(cm);
    free(rm);
}

int main() {
    // w + 1 = 2, 32, 64, 65, 96, 130, 201; one-column and one-row images; more than one workgroup of rows and of raw words
    const int sizes[][2] = {{1, 1}, {1, 300}, {300, 1}, {64, 1}, {65, 1}, {7, 5}, {40, 64}, {33, 95}, {64, 63}, {130, 31}, {7, 200},
                            {100, 200}, {65, 129}, {129, 65}, {63, 64}, {64, 64}, {128, 128}, {200, 333}, {31, 2}, {97, 3}, {480, 854}};
    int n = 0;
    for (const auto& s : sizes)
        for (int mode = 0; mode < 4; ++mode)
            for (int rows : {64, 5, 1}) {  // (fewer rows per workgroup: the very wide images' path)
                if ((long long)s[0] * s[1] > 100000 && rows != 64) continue;
                run(s[0], s[1], mode, rows);
                ++n;
            }
    for (int i = 0; i < 300; ++i) run(1 + (int)(rnd() % 150), 1 + (int)(rnd() % 150), (int)(rnd() % 4), 1 + (int)(rnd() % 64)), ++n;
    printf("%d geometries, %d mismatches\n", n, g_bad);
    return g_bad ? 1 : 0;
}
