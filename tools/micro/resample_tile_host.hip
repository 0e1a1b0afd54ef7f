// resample.hip's kernels on the HOST, thread by thread: the steps of sola_amd/csrc/resample_tile.h run over plain heap arrays of
// exactly the planned sizes in place of the LDS, the source, the tables and the output, and the result is compared with a naive
// two-pass restatement.  Built with AddressSanitizer on the host side, every index of every geometry is checked without a GPU:
//   make -C tools/micro resample_tile_host && tools/micro/resample_tile_host
// (needs sola_amd/lib/libsola_hip.so for sola_resample_coeffs; runs no kernel and opens no device).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sola_amd/csrc/resample_tile.h"

static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

struct Axis {
    std::vector<int32_t> table;  // [out][2 + taps], empty: the axis keeps its size
    int taps = 0;
};
static Axis make_axis(int in, int out, int filter) {
    Axis ax;
    if (in == out) return ax;
    ax.taps = sola_resample_taps(in, out, filter);
    std::vector<int32_t> b(2 * (size_t)out), k((size_t)out * ax.taps);
    if (ax.taps <= 0 || sola_resample_coeffs(in, out, filter, b.data(), k.data()) != 0) { printf("coeffs failed: %s\n", sola_last_error()); exit(2); }
    ax.table.resize((size_t)out * (2 + ax.taps));
    for (int o = 0; o < out; ++o) {
        ax.table[(size_t)o * (2 + ax.taps)] = b[2 * o];
        ax.table[(size_t)o * (2 + ax.taps) + 1] = b[2 * o + 1];
        memcpy(&ax.table[(size_t)o * (2 + ax.taps) + 2], &k[(size_t)o * ax.taps], 4 * (size_t)ax.taps);
    }
    return ax;
}

// naive: horizontal pass into a byte image, then vertical
static std::vector<uint8_t> naive(const uint8_t* src, int T, int H, int W, int C, int h, int w, const Axis& ax, const Axis& ay) {
    std::vector<uint8_t> mid((size_t)T * H * w * C), out((size_t)T * h * w * C);
    for (int t = 0; t < T; ++t)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < w; ++x)
                for (int c = 0; c < C; ++c) {
                    int v;
                    if (ax.table.empty()) {
                        v = src[(((size_t)t * H + y) * W + x) * C + c];
                    } else {
                        const int32_t* row = &ax.table[(size_t)x * (2 + ax.taps)];
                        int acc = 1 << 21;
                        for (int j = 0; j < row[1]; ++j) acc += src[(((size_t)t * H + y) * W + row[0] + j) * C + c] * row[2 + j];
                        v = acc >> 22;
                        v = v < 0 ? 0 : v > 255 ? 255 : v;
                    }
                    mid[(((size_t)t * H + y) * w + x) * C + c] = (uint8_t)v;
                }
    for (int t = 0; t < T; ++t)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                for (int c = 0; c < C; ++c) {
                    int v;
                    if (ay.table.empty()) {
                        v = mid[(((size_t)t * H + y) * w + x) * C + c];
                    } else {
                        const int32_t* row = &ay.table[(size_t)y * (2 + ay.taps)];
                        int acc = 1 << 21;
                        for (int j = 0; j < row[1]; ++j) acc += mid[(((size_t)t * H + row[0] + j) * w + x) * C + c] * row[2 + j];
                        v = acc >> 22;
                        v = v < 0 ? 0 : v > 255 ? 255 : v;
                    }
                    out[(((size_t)t * h + y) * w + x) * C + c] = (uint8_t)v;
                }
    return out;
}

template <int C, bool LUT>
static void run_fused(const ResampleArgs& a, const RsPlan& p) {
    uint8_t* lds = (uint8_t*)malloc(p.lds);  // exactly the planned bytes (malloc's blocks are 16-byte aligned)
    std::vector<int2> bx(RS_TW), by(RS_TH);
    std::vector<float> lut_s(LUT ? C * 256 : 1);
    const unsigned blocks = (unsigned)a.tiles_x * a.tiles_y * a.T;
    for (unsigned blk = 0; blk < blocks; ++blk) {
        memset(lds, 0xEE, p.lds);
        RsTile s;
        rs_tile_init(s, a, blk, lds, bx.data(), by.data(), lut_s.data());
        for (int tid = 0; tid < RS_THREADS; ++tid) rs_tile_load_tables<C, LUT>(s, a, tid);
        rs_tile_window<C>(s, a);
        for (int r0 = 0; r0 < s.nrows; r0 += a.rows_chunk) {
            const int nr = rs_min(a.rows_chunk, s.nrows - r0);
            memset(s.raw, 0xDD, (size_t)a.rows_chunk * a.raw_pitch);
            for (int tid = 0; tid < RS_THREADS; ++tid) rs_tile_stage<C>(s, a, tid, r0, nr);
            for (int tid = 0; tid < RS_THREADS; ++tid) rs_tile_horizontal<C>(s, a, tid, r0, nr);
        }
        for (int tid = 0; tid < RS_THREADS; ++tid) rs_tile_vertical<C, LUT>(s, a, tid);
    }
    free(lds);
}

static int g_cases = 0, g_fused = 0;

// corrupt: the tables hold garbage bounds - the result is not compared, only the accesses are checked
static bool run_case(int T, int H, int W, int C, int h, int w, int filter, bool use_lut, int src_off, int out_off, bool corrupt = false) {
    Axis ax = make_axis(W, w, filter), ay = make_axis(H, h, filter);
    const size_t n_src = (size_t)T * H * W * C, n_out = (size_t)T * h * w * C;
    // src_off bytes past a 16-byte boundary, and the source ends where its allocation ends: a read past it is caught
    uint8_t* src_buf = (uint8_t*)malloc(n_src + src_off);
    uint8_t* src = src_buf + src_off;
    for (size_t i = 0; i < n_src; ++i) src[i] = (uint8_t)(rnd() % 3 == 0 ? (rnd() & 1) * 255 : rnd());
    std::vector<uint8_t> want = naive(src, T, H, W, C, h, w, ax, ay);
    if (corrupt) {
        for (Axis* a : {&ax, &ay})
            for (size_t o = 0; !a->table.empty() && o < a->table.size() / (2 + a->taps); ++o) {
                a->table[o * (2 + a->taps)] = (int32_t)(rnd() % 40000) - 20000;
                a->table[o * (2 + a->taps) + 1] = (int32_t)(rnd() % 80000) - 20000;
            }
    }
    std::vector<float> lut((size_t)C * 256);
    for (int i = 0; i < C * 256; ++i) lut[i] = (float)(i * 7 % 1021) * 0.125f - 3.f;
    const size_t out_bytes = n_out * (use_lut ? 4 : 1);
    uint8_t* out_buf = (uint8_t*)malloc(out_bytes + out_off);
    void* out = out_buf + out_off;
    const int32_t* tx = ax.table.empty() ? nullptr : ax.table.data();
    const int32_t* ty = ay.table.empty() ? nullptr : ay.table.data();
    const RsPlan p = rs_plan(H, W, C, h, w, ax.taps > 1 ? ax.taps : 1, ay.taps > 1 ? ay.taps : 1, !tx, !ty);
    std::vector<uint8_t> scratch;
    if (p.fused) {
        ++g_fused;
        const ResampleArgs a = rs_fused_args(p, src, T, H, W, h, w, tx, ax.taps, ty, ay.taps, use_lut ? lut.data() : nullptr, out);
        if (C == 1 && use_lut) run_fused<1, true>(a, p);
        else if (C == 1) run_fused<1, false>(a, p);
        else if (use_lut) run_fused<3, true>(a, p);
        else run_fused<3, false>(a, p);
    } else {
        const uint8_t* from = src;
        if (tx) {
            scratch.resize((size_t)T * H * w * C);
            PassArgs a{src, tx, nullptr, scratch.data(), (long long)scratch.size(), H, W, C, w, ax.taps};
            for (long long i = 0; i < a.total; ++i) rs_pass_element<false>(a, i);
            from = scratch.data();
        }
        PassArgs a{from, ty, use_lut ? lut.data() : nullptr, out, (long long)n_out, H, w, C, h, ay.taps > 1 ? ay.taps : 1};
        for (long long i = 0; i < a.total; ++i) rs_pass_element<true>(a, i);
    }
    bool ok = true;
    if (!corrupt) {
        for (int t = 0; t < T && ok; ++t)
            for (int y = 0; y < h && ok; ++y)
                for (int x = 0; x < w && ok; ++x)
                    for (int c = 0; c < C && ok; ++c) {
                        const uint8_t v = want[(((size_t)t * h + y) * w + x) * C + c];
                        if (use_lut) ok = ((const float*)out)[(((size_t)t * C + c) * h + y) * w + x] == lut[c * 256 + v];
                        else ok = ((const uint8_t*)out)[(((size_t)t * h + y) * w + x) * C + c] == v;
                        if (!ok) printf("MISMATCH at t %d y %d x %d c %d\n", t, y, x, c);
                    }
    }
    ++g_cases;
    if (!ok) printf("FAILED: T %d %dx%d C %d -> %dx%d filter %d lut %d offsets %d %d (%s)\n", T, H, W, C, h, w, filter, (int)use_lut, src_off, out_off,
                    p.fused ? "fused" : "two passes");
    free(src_buf); free(out_buf);
    return ok;
}

int main() {
    static const int geo[][4] = {
        {53, 37, 20, 16}, {53, 37, 64, 64}, {37, 53, 16, 20}, {480, 270, 256, 256}, {270, 480, 256, 256}, {480, 270, 333, 187},
        {7, 200, 200, 7}, {200, 7, 7, 200}, {5, 3, 41, 50}, {1, 1, 4, 4}, {64, 64, 1, 1}, {200, 33, 7, 33}, {33, 200, 33, 7},
        {48, 27, 30, 27}, {27, 48, 27, 30}, {29, 31, 29, 31}, {90, 70, 65, 63}, {70, 90, 63, 65}, {150, 140, 131, 130},
        {609, 600, 200, 200},  // 3 x down: the source rows of a tile are staged 14 at a time
        {3000, 40, 8, 24}, {2600, 9, 5, 9}, {48, 85, 64, 64}, {48, 85, 100, 100}, {160, 90, 64, 36},
    };
    bool ok = true;
    for (const auto& g : geo)
        for (int filter : {SOLA_RESAMPLE_BILINEAR, SOLA_RESAMPLE_BICUBIC})
            for (int C : {1, 3})
                for (int lut = 0; lut < 2; ++lut)
                    for (int off = 0; off < 4; ++off)
                        ok &= run_case(off == 3 ? 2 : 1, g[0], g[1], C, g[2], g[3], filter, lut != 0, off, lut ? (off & 1) * 4 : off);
    // the shapes of the benchmark, one frame each
    ok &= run_case(1, 1080, 1920, 3, 1024, 1024, SOLA_RESAMPLE_BICUBIC, true, 0, 0);
    ok &= run_case(1, 720, 1280, 3, 1024, 1024, SOLA_RESAMPLE_BICUBIC, true, 1, 0);
    ok &= run_case(1, 1080, 1920, 3, 750, 1333, SOLA_RESAMPLE_BILINEAR, true, 2, 0);
    ok &= run_case(1, 1080, 1920, 3, 1024, 1024, SOLA_RESAMPLE_BICUBIC, false, 3, 1);
    // tables that sola_resample_coeffs did not write: wrong pixels, no access outside the buffers
    for (const auto& g : geo)
        for (int C : {1, 3})
            for (int lut = 0; lut < 2; ++lut) ok &= run_case(2, g[0], g[1], C, g[2], g[3], SOLA_RESAMPLE_BICUBIC, lut != 0, 1, 0, true);
    printf("%s: %d cases (%d in one launch)\n", ok ? "ok" : "FAILED", g_cases, g_fused);
    return ok ? 0 : 1;
}
