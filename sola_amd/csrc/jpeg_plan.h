// Baseline JPEG on the GPU (jpeg.hip): the host parser and the per-thread arithmetic of the entropy decode - byte-stuffed bit reader,
// subsequence starts, decoder state, one subsequence's decode - as host/device functions.  jpeg.hip's kernels call them on the device
// and sola_jpeg_parse on the host; tools/micro/jpeg_host.hip runs the same code thread by thread over heap buffers of exactly the
// file's size under AddressSanitizer.  Nothing here trusts its input: every read of a file or a scan goes through a range check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sola_hip.h"

#define JPEG_HD __host__ __device__ __forceinline__

constexpr int JPEG_ERR_CODE = 1;     // a bit pattern with no Huffman code
constexpr int JPEG_ERR_ZIGZAG = 2;   // a run that leaves the block (zigzag index past 63)
constexpr int JPEG_ERR_OVERRUN = 4;  // entropy data left after the segment's last block
constexpr int JPEG_ERR_SHORT = 8;    // a restart segment that ends before its last block

JPEG_HD int jpeg_min(int a, int b) { return a < b ? a : b; }
JPEG_HD int jpeg_max(int a, int b) { return a > b ? a : b; }

// zigzag position -> natural (row-major) position
__device__ __constant__ const uint8_t jpeg_natural_dev[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t jpeg_natural_host[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
JPEG_HD int jpeg_natural(int z) {
#if defined(__HIP_DEVICE_COMPILE__)
    return jpeg_natural_dev[z & 63];
#else
    return jpeg_natural_host[z & 63];
#endif
}

// ------------------------------------------------------------------------------------------------------------------- bytes
// A window [lo, hi) of a scan held at p (global memory, LDS, or a heap block on the host): index k of the SCAN, zero outside.
struct JpegBytes {
    const uint8_t* p;
    int lo, hi;
    JPEG_HD int at(int k) const { return (k >= lo && k < hi) ? p[k - lo] : 0; }
};

// Where a decoder that knows nothing starts in a subsequence cut at byte b of a segment [seg_lo, seg_hi): at b, or behind it when b
// is the stuffed 00 of an FF 00 pair (an FF inside a segment is always followed by its 00).
JPEG_HD int jpeg_guess_start(const JpegBytes& s, int b, int seg_lo) {
    return (b > seg_lo && s.at(b - 1) == 0xFF && s.at(b) == 0x00) ? b + 1 : b;
}

// ------------------------------------------------------------------------------------------------------------------- state
// (bit position, block within the MCU, zigzag index) in one 64-bit word.  The position is byte * 8 + bit of the DATA byte that holds
// the next bit (never a stuffed 00); scans are below 2^28 bytes.
typedef unsigned long long JpegState;
JPEG_HD JpegState jpeg_state(unsigned pos, int n, int z) { return (JpegState)pos | ((JpegState)(unsigned)n << 32) | ((JpegState)(unsigned)z << 40); }
JPEG_HD unsigned jpeg_state_pos(JpegState s) { return (unsigned)s; }
JPEG_HD int jpeg_state_n(JpegState s) { return (int)((s >> 32) & 0xFF); }
JPEG_HD int jpeg_state_z(JpegState s) { return (int)((s >> 40) & 0xFF); }

// ------------------------------------------------------------------------------------------------------------------ reader
// 64-bit window, next bit at the top.  `next` is the scan index of the next byte to fetch, `ff` remembers which of the last bytes
// fetched were FF (each took its stuffed 00 with it), so that the position of the next unread bit can be told at any time.
struct JpegReader {
    JpegBytes s;
    int seg_hi;  // bytes at or beyond it read as zero bits
    unsigned long long acc;
    int nbits, next;
    unsigned ff;
    JPEG_HD void fill() {
        while (nbits <= 56) {
            int b = 0;
            if (next < seg_hi) {
                b = s.at(next++);
                if (b == 0xFF) ++next;  // its stuffed 00
            } else {
                ++next;  // zero bits behind the segment: the position keeps counting, one byte each
            }
            ff = (ff << 1) | (b == 0xFF ? 1u : 0u);
            acc |= (unsigned long long)b << (56 - nbits);
            nbits += 8;
        }
    }
    JPEG_HD void start(const JpegBytes& bytes, int seg_hi_, unsigned pos) {
        s = bytes; seg_hi = seg_hi_; acc = 0; nbits = 0; ff = 0;
        next = (int)(pos >> 3);
        fill();
        drop((int)(pos & 7));
    }
    JPEG_HD unsigned peek(int n) const { return (unsigned)(acc >> (64 - n)); }  // 1 <= n <= 32
    JPEG_HD void drop(int n) {  // n <= nbits
        if (n) { acc <<= n; nbits -= n; }
    }
    // scan index of the byte that holds the next unread bit, and that bit's index in it
    JPEG_HD int byte_pos() const {
        const int m = (nbits + 7) >> 3;  // bytes of the window not fully read, the last m fetched
        return next - m - __builtin_popcount(ff & ((1u << m) - 1u));
    }
    JPEG_HD unsigned pos() const { return (unsigned)byte_pos() * 8u + (unsigned)((8 - (nbits & 7)) & 7); }
};

// ----------------------------------------------------------------------------------------------------------------- Huffman
// One symbol of table h from the top of the window (>= 16 bits there): the symbol, or -1 for a bit pattern without a code.
JPEG_HD int jpeg_symbol(JpegReader& r, const SolaJpegHuff* h) {
    const unsigned v = r.peek(16);
    const unsigned e = h->look[v >> 8];
    if (e) {
        r.drop((int)(e >> 8));
        return (int)(e & 0xFF);
    }
    for (int l = 9; l <= 16; ++l)
        if (v < h->limit[l]) {
            r.drop(l);
            return h->vals[((int)(v >> (16 - l)) + h->valoff[l]) & 255];
        }
    return -1;
}
// the s-bit magnitude behind a symbol, sign-extended the JPEG way (s <= 15)
JPEG_HD int jpeg_extend(JpegReader& r, int s) {
    if (s == 0) return 0;
    const int v = (int)r.peek(s);
    r.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// -------------------------------------------------------------------------------------------------------- one subsequence
struct JpegSubseq {
    int lo, hi;          // its bytes [lo, hi) of the scan
    int seg_lo, seg_hi;  // its restart segment
};
struct JpegTables {
    const SolaJpegHuff* huff;  // [6]: component * 2 + (0 DC, 1 AC)
    const uint16_t* quant;     // [3][64], natural order
    int ncomp, ny, bpm;        // luma blocks per MCU, blocks per MCU
};
JPEG_HD int jpeg_block_comp(const JpegTables& t, int n) { return n < t.ny ? 0 : jpeg_min(n - t.ny + 1, t.ncomp - 1); }

// Decodes the symbols that START in q's bytes from state `in` and returns the state behind them; *count = blocks completed.
// A state that already lies behind the subsequence passes through.  WRITE: coefficients times their quantiser go to coef (int16
// [.][64], natural order, DC as the difference) from block `blk` on, never at or beyond blk_hi; *err collects JPEG_ERR_* bits.
// Without WRITE a bit pattern that cannot be decoded ends the subsequence at its successor's guess and reports nothing: a guessed
// state decodes rubbish as a matter of course.
template <bool WRITE>
JPEG_HD JpegState jpeg_decode_subseq(const JpegBytes& bytes, const JpegSubseq& q, const JpegTables& t, JpegState in, int* count, int16_t* coef,
                                     long long blk, long long blk_hi, int* err) {
    *count = 0;
    if ((int)(jpeg_state_pos(in) >> 3) >= q.hi) return in;
    JpegReader r;
    r.start(bytes, q.seg_hi, jpeg_state_pos(in));
    int n = jpeg_state_n(in) % t.bpm, z = jpeg_state_z(in) & 63, done = 0, bad = 0;
    while (r.byte_pos() < q.hi) {
        if (WRITE && blk >= blk_hi) {  // the segment is complete: what is left are the pad bits of its last byte, or an overrun
            if (r.byte_pos() + 2 < q.seg_hi) bad |= JPEG_ERR_OVERRUN;
            break;
        }
        r.fill();
        const int c = jpeg_block_comp(t, n);
        int v, at;
        if (z == 0) {
            const int s = jpeg_symbol(r, t.huff + 2 * c);
            if (s < 0) { bad |= JPEG_ERR_CODE; break; }
            v = jpeg_extend(r, s & 15);
            at = 0;
            z = 1;
        } else {
            const int rs = jpeg_symbol(r, t.huff + 2 * c + 1);
            if (rs < 0) { bad |= JPEG_ERR_CODE; break; }
            const int run = rs >> 4, s = rs & 15;
            if (s == 0) {
                if (run != 15) {
                    z = 64;  // end of block
                } else {
                    z += 16;
                    if (z > 63) { bad |= JPEG_ERR_ZIGZAG; break; }
                }
                v = 0;
                at = -1;
            } else {
                z += run;
                if (z > 63) { bad |= JPEG_ERR_ZIGZAG; break; }
                v = jpeg_extend(r, s);
                at = jpeg_natural(z);
                ++z;
            }
        }
        if (WRITE && at >= 0) coef[blk * 64 + at] = (int16_t)(v * (int)t.quant[c * 64 + at]);
        if (z >= 64) {
            z = 0;
            n = n + 1 == t.bpm ? 0 : n + 1;
            ++done;
            if (WRITE) ++blk;
        }
    }
    *count = done;
    if (bad) {
        if (WRITE) *err |= bad;
        return jpeg_state((unsigned)jpeg_guess_start(bytes, q.hi, q.seg_lo) * 8u, 0, 0);
    }
    return jpeg_state(r.pos(), n, z);
}

// ------------------------------------------------------------------------------------------------------------------ parser
struct JpegParseError {
    char msg[160];
};
#define JPEG_REFUSE(e, ...)                          \
    do {                                             \
        snprintf((e)->msg, sizeof((e)->msg), __VA_ARGS__); \
        return -1;                                   \
    } while (0)

// The lookup form of one DHT table; -1 for a table no decoder could use.
inline int jpeg_build_huff(const uint8_t counts[16], const uint8_t* vals, int nvals, bool dc, SolaJpegHuff* h) {
    memset(h, 0, sizeof(*h));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        h->valoff[l] = k - (int)code;
        for (int i = 0; i < cnt; ++i, ++k, ++code) {
            if (k >= nvals || k >= 256) return -1;
            if (dc && vals[k] > 15) return -1;
            h->vals[k] = vals[k];
            if (l <= 8)
                for (unsigned f = 0; f < (1u << (8 - l)); ++f) h->look[(code << (8 - l)) | f] = (uint16_t)((l << 8) | vals[k]);
        }
        if (code > (1u << l)) return -1;  // more codes of this length than the prefix leaves room for
        h->limit[l] = code << (16 - l);
        code <<= 1;
    }
    return k == nvals ? 0 : -1;
}

// One file's bytes -> plan (+ the restart segments' [begin, end) byte offsets from scan_begin, the first seg_cap of them).  0, or -1
// with the reason in e->msg.  Reads data[0 .. len) only.
inline int jpeg_parse(const uint8_t* data, long long len, SolaJpegPlan* plan, int32_t* segs, long long seg_cap, JpegParseError* e) {
    memset(plan, 0, sizeof(*plan));
    e->msg[0] = 0;
    if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) JPEG_REFUSE(e, "not a JPEG file (no SOI marker)");
    if (len >= (1ll << 31)) JPEG_REFUSE(e, "file of %lld bytes, at most 2^31 - 1", len);
    uint8_t qt[4][64];
    bool have_qt[4] = {false, false, false, false}, have_ht[8] = {false, false, false, false, false, false, false, false};
    static_assert(sizeof(SolaJpegHuff) % 4 == 0, "SolaJpegHuff is copied as a block");
    SolaJpegHuff* ht = new SolaJpegHuff[8];  // [class * 4 + id]
    struct Free { SolaJpegHuff* p; ~Free() { delete[] p; } } free_ht{ht};
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, cid[3] = {0, 0, 0}, ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, cq[3] = {0, 0, 0};
    int ri = 0;
    long long p = 2;
    for (;;) {
        if (p + 2 > len) JPEG_REFUSE(e, "file ends before the scan (at byte %lld)", p);
        if (data[p] != 0xFF) JPEG_REFUSE(e, "byte 0x%02X at %lld where a marker should be", data[p], p);
        int m = data[p + 1];
        if (m == 0xFF) { ++p; continue; }  // fill bytes before a marker are legal between segments
        p += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) JPEG_REFUSE(e, "marker 0x%02X in the header", m);
        if (m == 0xD9) JPEG_REFUSE(e, "EOI before any scan");
        if (p + 2 > len) JPEG_REFUSE(e, "segment 0x%02X: length field beyond the file", m);
        const long long sl = ((long long)data[p] << 8) | data[p + 1];
        if (sl < 2 || p + sl > len) JPEG_REFUSE(e, "segment 0x%02X: length %lld beyond the file", m, sl);
        const uint8_t* s = data + p + 2;
        const long long n = sl - 2;
        if (m == 0xC0) {
            if (sof) JPEG_REFUSE(e, "more than one SOF");
            if (n < 6) JPEG_REFUSE(e, "SOF0: short segment");
            if (s[0] == 12) JPEG_REFUSE(e, "12-bit samples");
            if (s[0] != 8) JPEG_REFUSE(e, "%d-bit samples", s[0]);
            plan->height = (s[1] << 8) | s[2];
            plan->width = (s[3] << 8) | s[4];
            plan->ncomp = s[5];
            if (plan->ncomp == 4) JPEG_REFUSE(e, "four components (CMYK / YCCK)");
            if (plan->ncomp != 1 && plan->ncomp != 3) JPEG_REFUSE(e, "%d components", plan->ncomp);
            if (plan->width < 1 || plan->height < 1 || plan->width > SOLA_JPEG_MAX_SIZE || plan->height > SOLA_JPEG_MAX_SIZE)
                JPEG_REFUSE(e, "size %dx%d: width and height must be 1 .. %d", plan->width, plan->height, SOLA_JPEG_MAX_SIZE);
            if (n != 6 + 3 * plan->ncomp) JPEG_REFUSE(e, "SOF0: length %lld for %d components", sl, plan->ncomp);
            for (int c = 0; c < plan->ncomp; ++c) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                cq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) JPEG_REFUSE(e, "sampling factors %dx%d of component %d", ch[c], cv[c], c);
                if (cq[c] > 3) JPEG_REFUSE(e, "quantisation table %d of component %d", cq[c], c);
            }
            if (plan->ncomp == 3) {
                if (ch[1] != ch[2] || cv[1] != cv[2]) JPEG_REFUSE(e, "sampling factors: chroma %dx%d and %dx%d", ch[1], cv[1], ch[2], cv[2]);
                if (ch[0] < ch[1] || cv[0] < cv[1]) JPEG_REFUSE(e, "sampling factors: subsampled luma (%dx%d against chroma %dx%d)", ch[0], cv[0], ch[1], cv[1]);
                if (ch[1] != 1 || cv[1] != 1) JPEG_REFUSE(e, "sampling factors: chroma %dx%d, only 1x1", ch[1], cv[1]);
                if (ch[0] == 1 && cv[0] == 2) JPEG_REFUSE(e, "sampling factors: 4:4:0 (luma 1x2)");
                if (ch[0] == 4 && cv[0] == 1) JPEG_REFUSE(e, "sampling factors: 4:1:1 (luma 4x1)");
                if (!((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2)))
                    JPEG_REFUSE(e, "sampling factors: luma %dx%d, only 1x1, 2x1 and 2x2", ch[0], cv[0]);
                plan->hs = ch[0];
                plan->vs = cv[0];
            } else {
                plan->hs = plan->vs = 1;  // a scan of one component is not interleaved: its factors do not matter
            }
            sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (n >= 1 && s[0] == 12 && m == 0xC1) JPEG_REFUSE(e, "12-bit samples (extended sequential SOF1)");
            JPEG_REFUSE(e, "%s (SOF%d), only baseline SOF0",
                        m == 0xC1 ? "extended sequential DCT" : m == 0xC2 ? "progressive DCT" : m == 0xC3 ? "lossless"
                        : m >= 0xC9 ? "arithmetic coding" : "differential (hierarchical) frame", m - 0xC0);
        } else if (m == 0xCC) {
            JPEG_REFUSE(e, "arithmetic coding (DAC segment)");
        } else if (m == 0xC4) {
            long long o = 0;
            while (o < n) {
                if (o + 17 > n) JPEG_REFUSE(e, "DHT: short segment");
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) JPEG_REFUSE(e, "DHT: table class %d id %d", tc, th);
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
                if (total > 256 || o + 17 + total > n) JPEG_REFUSE(e, "DHT: %d symbols beyond the segment", total);
                if (jpeg_build_huff(s + o + 1, s + o + 17, total, tc == 0, &ht[tc * 4 + th]) != 0)
                    JPEG_REFUSE(e, "DHT: table class %d id %d is no prefix code", tc, th);
                have_ht[tc * 4 + th] = true;
                o += 17 + total;
            }
        } else if (m == 0xDB) {
            long long o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq == 1) JPEG_REFUSE(e, "16-bit quantisation tables");
                if (pq != 0 || tq > 3) JPEG_REFUSE(e, "DQT: precision %d id %d", pq, tq);
                if (o + 65 > n) JPEG_REFUSE(e, "DQT: short segment");
                for (int z = 0; z < 64; ++z) qt[tq][jpeg_natural_host[z]] = s[o + 1 + z];
                have_qt[tq] = true;
                o += 65;
            }
        } else if (m == 0xDD) {
            if (n != 2) JPEG_REFUSE(e, "DRI: length %lld", sl);
            ri = (s[0] << 8) | s[1];
        } else if (m == 0xDC) {
            JPEG_REFUSE(e, "DNL marker");
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
            // APPn / COM: skipped (EXIF orientation included, as PIL ignores it)
        } else if (m == 0xDA) {
            if (!sof) JPEG_REFUSE(e, "SOS before SOF");
            if (n < 1 || s[0] != plan->ncomp) JPEG_REFUSE(e, "more than one scan (a scan of %d of the %d components)", n < 1 ? 0 : s[0], plan->ncomp);
            if (n != 4 + 2 * plan->ncomp) JPEG_REFUSE(e, "SOS: length %lld for %d components", sl, plan->ncomp);
            if (adobe && (adobe_transform == 0 || adobe_transform == 2) && plan->ncomp == 3)
                JPEG_REFUSE(e, "Adobe segment with transform %d (not YCbCr)", adobe_transform);
            if (adobe && adobe_transform != 1 && plan->ncomp == 3) JPEG_REFUSE(e, "Adobe segment with transform %d", adobe_transform);
            if (!jfif && !adobe && plan->ncomp == 3 && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')
                JPEG_REFUSE(e, "components named R, G, B without a JFIF or Adobe segment (read as RGB, not YCbCr)");
            for (int c = 0; c < plan->ncomp; ++c) {
                if (s[1 + 2 * c] != cid[c]) JPEG_REFUSE(e, "SOS: component %d where the frame has %d", s[1 + 2 * c], cid[c]);
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) JPEG_REFUSE(e, "SOS: Huffman tables %d / %d", td, ta);
                if (!have_ht[td]) JPEG_REFUSE(e, "missing table: DC Huffman table %d", td);
                if (!have_ht[4 + ta]) JPEG_REFUSE(e, "missing table: AC Huffman table %d", ta);
                if (!have_qt[cq[c]]) JPEG_REFUSE(e, "missing table: quantisation table %d", cq[c]);
                plan->huff[2 * c] = ht[td];
                plan->huff[2 * c + 1] = ht[4 + ta];
                for (int i = 0; i < 64; ++i) plan->quant[c][i] = qt[cq[c]][i];
            }
            const uint8_t* t = s + 1 + 2 * plan->ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) JPEG_REFUSE(e, "SOS: spectral selection %d..%d, approximation 0x%02X in a baseline scan", t[0], t[1], t[2]);
            p += sl;
            break;
        } else {
            JPEG_REFUSE(e, "marker 0x%02X", m);
        }
        p += sl;
    }
    const int mw = 8 * plan->hs, mh = 8 * plan->vs;
    plan->mcus_x = (plan->width + mw - 1) / mw;
    plan->mcus_y = (plan->height + mh - 1) / mh;
    plan->blocks_per_mcu = plan->ncomp == 1 ? 1 : plan->hs * plan->vs + 2;
    const long long mcus = (long long)plan->mcus_x * plan->mcus_y;
    plan->n_blocks = (int32_t)(mcus * plan->blocks_per_mcu);  // <= 2048 * 2048 * 3
    plan->restart_interval = ri;
    plan->scan_begin = p;
    // one pass over the scan for FF: stuffing, restart markers, the marker that ends it
    const long long max_segs = ri ? (mcus + ri - 1) / ri : 1;
    long long nseg = 0, seg_lo = p, q = p, end = -1;
    int expect = 0;
    while (end < 0) {
        const uint8_t* f = q < len ? (const uint8_t*)memchr(data + q, 0xFF, (size_t)(len - q)) : nullptr;
        if (!f) { end = len; break; }                     // no EOI: the file is cut short
        q = f - data;
        if (q + 1 >= len) { end = q; break; }             // a lone FF as the last byte
        const int m = data[q + 1];
        if (m == 0x00) { q += 2; continue; }
        if (m >= 0xD0 && m <= 0xD7) {
            if (!ri) JPEG_REFUSE(e, "restart marker in a scan without a restart interval");
            if (m != 0xD0 + expect) JPEG_REFUSE(e, "restart marker RST%d where RST%d is due", m - 0xD0, expect);
            expect = (expect + 1) & 7;
            if (nseg + 1 >= max_segs) JPEG_REFUSE(e, "more restart segments than the %lld intervals of the frame", max_segs);
            if (segs && nseg < seg_cap) { segs[2 * nseg] = (int32_t)(seg_lo - p); segs[2 * nseg + 1] = (int32_t)(q - p); }
            ++nseg;
            q += 2;
            seg_lo = q;
            continue;
        }
        if (m == 0xD9) { end = q; break; }
        if (m == 0xFF) JPEG_REFUSE(e, "0xFF fill byte inside the scan");
        if (m == 0xDC) JPEG_REFUSE(e, "DNL marker");
        if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) JPEG_REFUSE(e, "more than one scan (marker 0x%02X behind the first)", m);
        JPEG_REFUSE(e, "marker 0x%02X inside the scan", m);
    }
    if (segs && nseg < seg_cap) { segs[2 * nseg] = (int32_t)(seg_lo - p); segs[2 * nseg + 1] = (int32_t)(end - p); }
    ++nseg;
    plan->scan_end = end;
    plan->n_segments = (int32_t)nseg;
    if (end - p >= (1ll << 28)) JPEG_REFUSE(e, "scan of %lld bytes, at most 2^28 - 1", end - p);
    return 0;
}
