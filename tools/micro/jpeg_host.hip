// jpeg.hip's host parser and the per-thread arithmetic of its entropy decode (sola_amd/csrc/jpeg_plan.h: bit reader over stuffed
// bytes, subsequence starts, decoder state, jpeg_decode_subseq) on the HOST, under AddressSanitizer, over heap buffers of exactly the
// file's and the scan's size:
//   make -C tools/micro jpeg_host && python tools/jpeg_host_cases.py        (writes Pillow-encoded files and runs this on them)
//   tools/micro/jpeg_host FILE...
// For every file, and for truncated and byte-flipped copies of it: parse; if the parser accepts, decode the scan (a) sequentially,
// one subsequence per restart segment, and (b) the way the kernels do - subsequences of 16 / 64 bytes, blocks of 4 / 256 threads, in-states
// guessed and replaced by the predecessor's out-state round after round, block tails double buffered, the same round bounds - and
// where (a) reports no error, (b) must give the same coefficients and no error.  Every coefficient write is checked against the
// buffer by the sanitizer and against the segment's block range by the code.  Runs no kernel, opens no device, needs no library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../sola_amd/csrc/jpeg_plan.h"

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }
static long g_parsed = 0, g_accepted = 0, g_compared = 0, g_rounds_max = 0;

struct Sub { int lo, hi, seg, first, guess; };

// (b): returns the error word; coef int16 [n_blocks][64] on the heap, exactly
static int decode_parallel(const SolaJpegPlan& plan, const std::vector<int32_t>& segs, const JpegBytes& bytes, int scan_len, int S, int NT,
                           std::vector<int16_t>& coef) {
    const JpegTables tab{plan.huff, &plan.quant[0][0], plan.ncomp, plan.ncomp == 1 ? 1 : plan.hs * plan.vs, plan.blocks_per_mcu};
    std::vector<Sub> sub;
    std::vector<int> seg_first;
    auto seg_range = [&](int s, int& lo, int& hi) {
        lo = std::max(0, std::min(segs[2 * s], scan_len));
        hi = std::max(lo, std::min(segs[2 * s + 1], scan_len));
    };
    for (int s = 0; s < plan.n_segments; ++s) {
        int lo, hi;
        seg_range(s, lo, hi);
        seg_first.push_back((int)sub.size());
        const int n = std::max(1, (hi - lo + S - 1) / S);
        for (int j = 0; j < n; ++j) {
            const int b = std::min(lo + j * S, hi);
            sub.push_back(Sub{b, std::min(b + S, hi), s, j == 0, j == 0 ? b : jpeg_guess_start(bytes, b, lo)});
        }
    }
    const int nsub = (int)sub.size(), wgs = (nsub + NT - 1) / NT;
    std::vector<JpegState> sin(nsub), sout(nsub), tail(2 * (size_t)wgs);
    std::vector<int> cnt(nsub);
    auto F = [&](int i, JpegState in, int* c) {
        int lo, hi;
        seg_range(sub[i].seg, lo, hi);
        const JpegSubseq q{sub[i].lo, sub[i].hi, lo, hi};
        return jpeg_decode_subseq<false>(bytes, q, tab, in, c, nullptr, 0, 0, nullptr);
    };
    int rounds = 0;
    for (;;) {
        bool flag = false;
        for (int w = 0; w < wgs; ++w) {
            const int first = w * NT, last = std::min(first + NT, nsub) - 1;
            std::vector<char> dirty(NT, 0);
            JpegState* tail_new = &tail[(size_t)(rounds & 1) * wgs];
            const JpegState* tail_old = &tail[(size_t)((rounds & 1) ^ 1) * wgs];
            if (rounds == 0) {
                for (int i = first; i <= last; ++i) { sin[i] = jpeg_state((unsigned)sub[i].guess * 8u, 0, 0); dirty[i - first] = 1; }
            } else {
                if (!sub[first].first && w > 0 && tail_old[w - 1] != sin[first]) { sin[first] = tail_old[w - 1]; dirty[0] = 1; }
                if (!dirty[0]) { tail_new[w] = tail_old[w]; continue; }
            }
            int iter = 0;
            for (; iter <= NT; ++iter) {
                for (int i = first; i <= last; ++i)
                    if (dirty[i - first]) sout[i] = F(i, sin[i], &cnt[i]);
                bool any = false;
                for (int i = last; i > first; --i) {  // every thread reads its predecessor's out-state of THIS iteration
                    dirty[i - first] = 0;
                    if (!sub[i].first && sout[i - 1] != sin[i]) { sin[i] = sout[i - 1]; dirty[i - first] = 1; any = true; }
                }
                dirty[0] = 0;
                if (!any) break;
            }
            if (iter > NT) { printf("FAIL: a block's loop did not end within its bound\n"); exit(1); }
            tail_new[w] = sout[last];
            if (last + 1 < nsub && (rounds == 0 || tail_old[w] != sout[last])) flag = true;
        }
        ++rounds;
        if (wgs == 1 || !flag) break;
        if (rounds > wgs) { printf("FAIL: the host loop did not end within its bound\n"); exit(1); }
    }
    g_rounds_max = std::max(g_rounds_max, (long)rounds);
    // prefix, write
    std::vector<long long> pref(nsub + 1, 0);
    for (int i = 0; i < nsub; ++i) pref[i + 1] = pref[i] + cnt[i];
    int err = 0;
    const long long per_seg = plan.restart_interval ? (long long)plan.restart_interval * plan.blocks_per_mcu : plan.n_blocks;
    for (int i = 0; i < nsub; ++i) {
        const int s = sub[i].seg;
        int lo, hi;
        seg_range(s, lo, hi);
        const long long blk_lo = std::min(s * per_seg, (long long)plan.n_blocks), blk_hi = std::min(blk_lo + per_seg, (long long)plan.n_blocks);
        const long long blk = blk_lo + std::max(0ll, std::min(pref[i] - pref[seg_first[s]], blk_hi - blk_lo));
        const JpegSubseq q{sub[i].lo, sub[i].hi, lo, hi};
        int c = 0, e = 0;
        jpeg_decode_subseq<true>(bytes, q, tab, sin[i], &c, coef.data(), blk, blk_hi, &e);
        if ((i + 1 == nsub || sub[i + 1].first) && blk + c < blk_hi) e |= JPEG_ERR_SHORT;
        err |= e;
    }
    return err;
}

static void check(const uint8_t* file, long long len, const char* what) {
    uint8_t* data = (uint8_t*)malloc((size_t)std::max(len, 1ll));  // exactly the file
    memcpy(data, file, (size_t)len);
    SolaJpegPlan plan;
    JpegParseError e;
    ++g_parsed;
    if (jpeg_parse(data, len, &plan, nullptr, 0, &e) != 0) { free(data); return; }
    std::vector<int32_t> segs(2 * (size_t)plan.n_segments);  // exactly the segments
    if (jpeg_parse(data, len, &plan, segs.data(), plan.n_segments, &e) != 0) { printf("FAIL %s: the second parse refused: %s\n", what, e.msg); exit(1); }
    ++g_accepted;
    if (plan.scan_begin < 0 || plan.scan_end < plan.scan_begin || plan.scan_end > len) { printf("FAIL %s: scan range outside the file\n", what); exit(1); }
    const int scan_len = (int)(plan.scan_end - plan.scan_begin);
    for (int s = 0; s < plan.n_segments; ++s)
        if (segs[2 * s] < 0 || segs[2 * s + 1] < segs[2 * s] || segs[2 * s + 1] > scan_len) { printf("FAIL %s: segment %d outside the scan\n", what, s); exit(1); }
    uint8_t* scan = (uint8_t*)malloc((size_t)std::max(scan_len, 1));  // exactly the scan
    memcpy(scan, data + plan.scan_begin, (size_t)scan_len);
    const JpegBytes bytes{scan, 0, scan_len};
    std::vector<int16_t> ref((size_t)plan.n_blocks * 64, 0);
    const int ref_err = decode_parallel(plan, segs, bytes, scan_len, 1 << 28, 256, ref);  // (a): one subsequence per segment
    const int cfg[3][2] = {{16, 4}, {64, 256}, {16, 256}};
    for (const auto& c : cfg) {
        std::vector<int16_t> coef((size_t)plan.n_blocks * 64, 0);
        const int err = decode_parallel(plan, segs, bytes, scan_len, c[0], c[1], coef);
        if (ref_err == 0) {
            ++g_compared;
            if (err != 0 || coef != ref) { printf("FAIL %s: subsequences of %d bytes, blocks of %d: error word %d, coefficients %s\n", what, c[0], c[1], err, coef == ref ? "equal" : "differ"); exit(1); }
        }
    }
    free(scan);
    free(data);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: jpeg_host FILE...\n"); return 2; }
    for (int f = 1; f < argc; ++f) {
        FILE* fp = fopen(argv[f], "rb");
        if (!fp) { printf("cannot open %s\n", argv[f]); return 2; }
        std::vector<uint8_t> file;
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + n);
        fclose(fp);
        const long accepted = g_accepted, compared = g_compared;
        check(file.data(), (long long)file.size(), argv[f]);
        if (g_accepted == accepted || g_compared == compared) { printf("FAIL %s: a valid file was refused or did not decode cleanly\n", argv[f]); return 1; }
        const long long len = (long long)file.size(), step = std::max(1ll, len / 97);
        for (long long cut = 0; cut < len; cut += (cut < 700 ? 1 : step)) check(file.data(), cut, "truncated");
        for (int k = 0; k < 64; ++k) {
            std::vector<uint8_t> copy = file;
            const int flips = 1 + (int)(rnd() % 3);
            for (int j = 0; j < flips; ++j) copy[rnd() % copy.size()] ^= (uint8_t)(1u << (rnd() % 8));
            check(copy.data(), len, "flipped");
        }
    }
    printf("jpeg_host ok: %ld buffers parsed, %ld accepted, %ld parallel decodes equal to the sequential one, at most %ld sync rounds\n", g_parsed, g_accepted,
           g_compared, g_rounds_max);
    return 0;
}
