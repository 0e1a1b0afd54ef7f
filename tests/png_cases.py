"""The PNG format of sola_png_deflate_* (include/sola_hip.h) restated in numpy / pure Python, and the shared case list of
test_png_cpu.py (which pins this restatement against zlib and PIL) and test_gpu_png.py (which uses it as the yardstick).

8-bit greyscale, filter type 0 on every scanline, one IDAT holding a zlib stream ``78 01`` + ONE fixed-Huffman DEFLATE
block with distance-1 matches only + Adler-32.  The raw stream is cut into maximal runs of equal bytes across row ends; a run
of value v and length n is the literal v, then L = n-1 more bytes: while L > 0: L == 258 or L >= 261 -> match 258;
L in {259, 260} -> match L-3; 3 <= L <= 257 -> match L; L in {1, 2} -> L literals."""
import struct
import zlib

import numpy as np

import masklet_cases as mc

# RFC 1951 3.2.5: (symbol, extra bits, first length)
_LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10),
                 (265, 1, 11), (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31),
                 (273, 3, 35), (274, 3, 43), (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115),
                 (281, 5, 131), (282, 5, 163), (283, 5, 195), (284, 5, 227), (285, 0, 258)]


def _fixed_code(sym):
    """RFC 1951 3.2.6: (code, bits) of a literal/length symbol in the fixed table."""
    if sym <= 143:
        return 0b00110000 + sym, 8
    if sym <= 255:
        return 0b110010000 + (sym - 144), 9
    if sym <= 279:
        return sym - 256, 7
    return 0b11000000 + (sym - 280), 8


def _reversed(code, bits):
    return int(format(code, f"0{bits}b")[::-1], 2)


def _token_tables():
    """value / bit count of every token, everything already in stream order (least significant bit first): index 0 and 1 =
    the literals 0x00 and 0xFF, index 3..258 = a distance-1 match of that length (code, extra bits, 5-bit distance code 0)."""
    val, nb = np.zeros(259, np.int64), np.zeros(259, np.int64)
    for i, byte in enumerate((0x00, 0xFF)):
        c, b = _fixed_code(byte)
        val[i], nb[i] = _reversed(c, b), b
    for length in range(3, 259):
        sym, extra, first = [t for t in _LENGTH_TABLE if t[2] <= length][-1]
        if length == 258:
            sym, extra, first = 285, 0, 258
        c, b = _fixed_code(sym)
        val[length], nb[length] = _reversed(c, b) | (length - first) << b, b + extra + 5
    return val, nb


TOKEN_VAL, TOKEN_BITS = _token_tables()
EOB_BITS = 7  # symbol 256: seven zero bits


def run_tokens(n):
    """Tokens of one run of length n, the rule of the format word for word: 0 = literal, else a match length."""
    out = [0]
    L = n - 1
    while L > 0:
        if L == 258 or L >= 261:
            out.append(258)
            L -= 258
        elif L in (259, 260):
            out.append(L - 3)
            L = 3
        elif L >= 3:
            out.append(L)
            L = 0
        else:
            out.extend([0] * L)
            L = 0
    return out


def raw_stream(mask):
    """(h,w) mask -> bytes: per row one filter byte 0, then 255 where the mask is set."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = m * 255
    return raw.tobytes()


def _pack(vals, nbits):
    """tokens (value, bits) -> bytes, least significant bit first, zero padded."""
    out = []
    step = 1 << 20
    for i in range(0, len(vals), step):
        v, b = vals[i:i + step], nbits[i:i + step]
        start = np.cumsum(b) - b
        idx = np.repeat(np.arange(len(v)), b)
        within = np.arange(int(b.sum())) - np.repeat(start, b)
        out.append(((v[idx] >> within) & 1).astype(np.uint8))
    return np.packbits(np.concatenate(out), bitorder="little").tobytes()


def deflate_raw(raw):
    """bytes of 0x00 / 0xFF -> the zlib stream of the format (vectorised over the runs; run_tokens is the rule)."""
    r = np.frombuffer(raw, np.uint8)
    assert r.size and np.isin(r, (0, 255)).all()
    starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
    lens = np.diff(np.concatenate([starts, [r.size]]))
    vals = (r[starts] != 0).astype(np.int64)
    L = lens - 1
    q, rem = L // 258, L % 258
    late = (q >= 1) & ((rem == 1) | (rem == 2))  # ends in 259 / 260: L-3, then 3
    K = q - late
    rest = rem + 258 * late
    t1 = np.where(rest == 0, -1, np.where(rest <= 2, 0, np.where(rest <= 257, rest, rest - 3)))
    t2 = np.where(rest == 2, 0, np.where(rest >= 259, 3, -1))
    cnt = 1 + K + (t1 >= 0) + (t2 >= 0)
    first = np.cumsum(cnt) - cnt
    tok = np.full(int(cnt.sum()), 258, np.int64)
    tok[first] = 0
    tok[(first + 1 + K)[t1 >= 0]] = t1[t1 >= 0]
    tok[(first + 2 + K)[t2 >= 0]] = t2[t2 >= 0]
    tok = np.where(tok == 0, np.repeat(vals, cnt), tok)  # literal -> which literal
    v = np.concatenate([[0b011], TOKEN_VAL[tok], [0]])   # BFINAL=1, BTYPE=01 (least significant bit first) ... end of block
    b = np.concatenate([[3], TOKEN_BITS[tok], [EOB_BITS]])
    return b"\x78\x01" + _pack(v, b) + struct.pack(">I", zlib.adler32(raw))


def deflate_raw_by_rule(raw):
    """The same stream from run_tokens, run by run (slow; pins the vectorised form on small inputs)."""
    r = np.frombuffer(raw, np.uint8)
    v, b = [0b011], [3]
    i = 0
    while i < r.size:
        j = i
        while j < r.size and r[j] == r[i]:
            j += 1
        for t in run_tokens(j - i):
            t = t if t else int(r[i] != 0)
            v.append(int(TOKEN_VAL[t])), b.append(int(TOKEN_BITS[t]))
        i = j
    v.append(0), b.append(EOB_BITS)
    return b"\x78\x01" + _pack(np.array(v, np.int64), np.array(b, np.int64)) + struct.pack(">I", zlib.adler32(raw))


def zlib_stream(mask):
    return deflate_raw(raw_stream(mask))


def stream_bound(h, w):
    return 6 + (9 * h * (w + 1) + 17) // 8


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_wrap(stream, h, w):
    """signature, IHDR (8-bit greyscale, no interlace), one IDAT, IEND around a zlib stream."""
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", stream) +
            _chunk(b"IEND", b""))


def png_file(mask):
    h, w = np.asarray(mask).shape
    return png_wrap(zlib_stream(mask), h, w)


# ---- cases ------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 300), (300, 1), (7, 5), (64, 63), (65, 257), (480, 854), (720, 1280), (1080, 1920), (1920, 1080)]
STRIPES = [1, 2, 3, 257, 258, 259, 260, 261]


def frames(h, w, seed=0):
    """[(name, (h,w) uint8 {0,1})]: empty, full, one pixel in each corner, checkerboard, vertical and horizontal stripes of
    every width of STRIPES (runs of every branch of the match rule, also across row ends), noise at 0.5 and 0.01, blobs."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8))]
    for name, (y, x) in (("tl", (0, 0)), ("tr", (0, w - 1)), ("bl", (h - 1, 0)), ("br", (h - 1, w - 1))):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        out.append(("corner_" + name, m))
    out.append(("checker", ((yy + xx) % 2).astype(np.uint8)))
    for s in STRIPES:
        out.append((f"vstripe{s}", ((xx // s) % 2).astype(np.uint8)))
        out.append((f"hstripe{s}", ((yy // s) % 2 == 0).astype(np.uint8)))
    out.append(("noise0.5", (rng.random((h, w)) < 0.5).astype(np.uint8)))
    out.append(("noise0.01", (rng.random((h, w)) < 0.01).astype(np.uint8)))
    for i, m in enumerate(mc.blob_masklet(5, h, w, seed + 7)):
        out.append((f"blob{i}", (np.asarray(m) != 0).astype(np.uint8)))
    return out


def small_frames():
    """Every frame of the sizes below 100 000 pixels (the CPU suite's share of the cases, plus one mid-size blob set)."""
    out = []
    for h, w in SIZES:
        if h * w < 100000:
            out += [(f"{h}x{w}/{n}", m) for n, m in frames(h, w)]
    out += [(f"480x854/{n}", m) for n, m in frames(480, 854) if n in ("empty", "full", "blob1", "vstripe259", "hstripe1", "noise0.01")]
    return out
