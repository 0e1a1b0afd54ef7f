"""Baseline JPEG decode (include/sola_hip.h: sola_jpeg_parse / sola_jpeg_decode) restated in numpy and plain Python - parser,
sequential Huffman decode, islow IDCT, fancy upsampling, colour - and the case generator of tests/test_jpeg_cpu.py and
tests/test_gpu_jpeg.py.  Pillow's own encoder makes every file at test time; nothing is read from disk.

The restatement is written from the arithmetic the header states, not from the library's code: a sequential decoder with one
bit position per restart segment, no subsequences, no lookup form (except where `parse` derives the plan's tables so that the C
parser can be compared field for field)."""
import io

import numpy as np
from PIL import Image

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SUBSEQ_MIN, SUBSEQ_DEFAULT = 16, 128   # SOLA_JPEG_SUBSEQ_MIN / _DEFAULT
THREADS_PER_BLOCK = 256                # subsequences a workgroup of the sync kernel owns

SIZES = [(8, 8), (16, 16), (17, 13), (40, 52), (33, 47), (9, 65), (24, 31)]   # (width, height)
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITIES = [30, 75, 95, 100]
CONTENTS = ["noise", "smooth"]
MODES = ["plain", "optimize", "restart3"]


# ----------------------------------------------------------------------------------------------------------------- the files
def image(w, h, content, seed, grey=False):
    rng = np.random.default_rng(seed)
    c = 1 if grey else 3
    if content == "noise":
        a = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    else:
        y, x = np.mgrid[0:h, 0:w]
        ph = rng.uniform(0, 6.28, size=(c, 3))
        a = np.stack([127.5 + 70 * np.sin(x / 9.0 + ph[k, 0]) + 50 * np.cos(y / 7.0 + ph[k, 1]) + 0.4 * ((x * y) % 17) for k in range(c)], -1)
        a = np.clip(a + rng.normal(0, 2.0, size=a.shape), 0, 255).astype(np.uint8)
    return a[:, :, 0] if grey else a


def encode(arr, quality=75, sampling="4:2:0", mode="plain", **kw):
    """Pillow's encoder.  mode: "plain", "optimize", "restart<n>" (restart_marker_blocks = n), or several joined by '+'."""
    for m in mode.split("+"):
        if m == "optimize":
            kw["optimize"] = True
        elif m.startswith("restart"):
            kw["restart_marker_blocks"] = int(m[7:])
    if arr.ndim == 3:
        kw["subsampling"] = sampling
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def case(w, h, sampling="4:2:0", quality=75, content="noise", mode="plain", seed=0):
    return encode(image(w, h, content, seed, grey=sampling == "grey"), quality, sampling, mode)


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def grid():
    for (w, h) in SIZES:
        for s in SAMPLINGS:
            for q in QUALITIES:
                for c in CONTENTS:
                    for m in MODES:
                        yield (w, h, s, q, c, m)


# ---------------------------------------------------------------------------------------------------------------- the parser
def huff_lookup(counts, vals):
    """The plan's form of one table: look [256] u16, limit [18] u32, valoff [18] i32, vals [256] u8."""
    look, limit, valoff, v = np.zeros(256, np.uint16), np.zeros(18, np.uint32), np.zeros(18, np.int32), np.zeros(256, np.uint8)
    code = k = 0
    for l in range(1, 17):
        valoff[l] = k - code
        for _ in range(counts[l - 1]):
            v[k] = vals[k]
            if l <= 8:
                look[code << (8 - l):(code + 1) << (8 - l)] = (l << 8) | vals[k]
            k += 1
            code += 1
        limit[l] = code << (16 - l)
        code <<= 1
    return look, limit, valoff, v


def parse(data):
    """A valid baseline file -> dict with the fields of SolaJpegPlan, `segs` ([begin, end) from scan_begin) and the raw tables."""
    assert data[:2] == b"\xff\xd8"
    p, qt, ht, ri = 2, {}, {}, 0
    plan = {}
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        s = data[p + 4:p + 2 + n]
        if m == 0xC0:
            assert s[0] == 8
            plan["height"], plan["width"], plan["ncomp"] = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif m == 0xC4:
            o = 0
            while o < len(s):
                counts = list(s[o + 1:o + 17])
                ht[(s[o] >> 4, s[o] & 15)] = (counts, list(s[o + 17:o + 17 + sum(counts)]))
                o += 17 + sum(counts)
        elif m == 0xDB:
            o = 0
            while o < len(s):
                assert s[o] >> 4 == 0
                t = np.zeros(64, np.uint16)
                t[NATURAL] = np.frombuffer(s[o + 1:o + 65], np.uint8)
                qt[s[o] & 15] = t
                o += 65
        elif m == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            assert s[0] == plan["ncomp"]
            tabs = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            p += 2 + n
            break
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
        p += 2 + n
    nc = plan["ncomp"]
    plan["hs"], plan["vs"] = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    plan["mcus_x"] = -(-plan["width"] // (8 * plan["hs"]))
    plan["mcus_y"] = -(-plan["height"] // (8 * plan["vs"]))
    plan["blocks_per_mcu"] = 1 if nc == 1 else plan["hs"] * plan["vs"] + 2
    plan["n_blocks"] = plan["mcus_x"] * plan["mcus_y"] * plan["blocks_per_mcu"]
    plan["restart_interval"] = ri
    plan["scan_begin"] = p
    plan["quant"] = [qt[comps[c][3]] for c in range(nc)]
    plan["huff_raw"] = [ht[(cls, tabs[c][cls])] for c in range(nc) for cls in (0, 1)]
    plan["huff"] = [huff_lookup(*h) for h in plan["huff_raw"]]
    segs, lo, q = [], p, p
    while True:
        q = data.find(b"\xff", q)
        assert q >= 0 and q + 1 < len(data)
        m = data[q + 1]
        if m == 0:
            q += 2
        elif 0xD0 <= m <= 0xD7:
            segs.append((lo - p, q - p))
            q += 2
            lo = q
        else:
            assert m == 0xD9, hex(m)
            break
    segs.append((lo - p, q - p))
    plan["scan_end"], plan["segs"], plan["n_segments"] = q, segs, len(segs)
    return plan


# ------------------------------------------------------------------------------------------------------------ entropy decode
def _decode_table(counts, vals):
    """next 16 bits -> (code length, symbol); length 0 where no code matches."""
    length, sym = np.zeros(65536, np.uint8), np.zeros(65536, np.uint8)
    code = k = 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            length[code << (16 - l):(code + 1) << (16 - l)] = l
            sym[code << (16 - l):(code + 1) << (16 - l)] = vals[k]
            k += 1
            code += 1
        code <<= 1
    return length.tolist(), sym.tolist()


def decode_coefficients(data, plan=None):
    """int16 [n_blocks, 64]: coefficient times quantiser, natural order, DC as values; blocks in scan order."""
    plan = plan or parse(data)
    nc, bpm, ri = plan["ncomp"], plan["blocks_per_mcu"], plan["restart_interval"]
    ny = bpm - 2 if nc == 3 else 1
    tabs = [_decode_table(*h) for h in plan["huff_raw"]]
    quant = [q.astype(np.int64) for q in plan["quant"]]
    mcus = plan["mcus_x"] * plan["mcus_y"]
    coef = np.zeros((plan["n_blocks"], 64), np.int64)
    nat = NATURAL.tolist()
    for k, (lo, hi) in enumerate(plan["segs"]):
        raw = data[plan["scan_begin"] + lo:plan["scan_begin"] + hi].replace(b"\xff\x00", b"\xff") + b"\0" * 8
        pos = 0

        def bits(n):
            nonlocal pos
            i, o = pos >> 3, pos & 7
            v = (int.from_bytes(raw[i:i + 5], "big") >> (40 - o - n)) & ((1 << n) - 1) if n else 0
            pos += n
            return v

        def symbol(tab):
            nonlocal pos
            i, o = pos >> 3, pos & 7
            v = (int.from_bytes(raw[i:i + 3], "big") >> (8 - o)) & 0xFFFF
            assert tab[0][v], "no code"
            pos += tab[0][v]
            return tab[1][v]

        def extend(s):
            v = bits(s)
            return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

        pred = [0] * nc
        m0 = k * ri if ri else 0
        m1 = min(m0 + ri, mcus) if ri else mcus
        for mcu in range(m0, m1):
            for n in range(bpm):
                c = 0 if n < ny else n - ny + 1
                b = mcu * bpm + n
                pred[c] += extend(symbol(tabs[2 * c]))
                coef[b, 0] = pred[c] * quant[c][0]
                z = 1
                while z < 64:
                    rs = symbol(tabs[2 * c + 1])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        z += 16
                        continue
                    z += r
                    assert z < 64
                    coef[b, nat[z]] = extend(s) * quant[c][nat[z]]
                    z += 1
    return coef.astype(np.int16)


# --------------------------------------------------------------------------------------------------------------------- pixels
def _idct_1d(v, shift):
    """One islow pass over axis 0 of v [8, ...] (int64), descaled by `shift` with rounding."""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (v[0] + v[4]) << 13
    tmp1 = (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3])
    return (out + (1 << (shift - 1))) >> shift


def idct(coef):
    """int16 [n, 64] -> uint8 [n, 8, 8]."""
    v = coef.astype(np.int64).reshape(-1, 8, 8)
    ws = _idct_1d(v.transpose(1, 0, 2), 11)              # columns: axis 0 = row index of the block -> ws [8 (row), n, 8 (col)]
    out = _idct_1d(ws.transpose(2, 1, 0), 18)            # rows: axis 0 = column index -> out [8 (col), n, 8 (row)]
    return np.clip(out.transpose(1, 2, 0) + 128, 0, 255).astype(np.uint8)


def component_planes(plan, pix):
    """The component planes cropped to ceil(W*h_i/h_max) x ceil(H*v_i/v_max)."""
    nc, hs, vs, bpm = plan["ncomp"], plan["hs"], plan["vs"], plan["blocks_per_mcu"]
    mx, my, W, H = plan["mcus_x"], plan["mcus_y"], plan["width"], plan["height"]
    b = pix.reshape(my, mx, bpm, 8, 8)
    if nc == 1:
        return [b[:, :, 0].transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:H, :W]]
    y = b[:, :, :hs * vs].reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)[:H, :W]
    cw, ch = -(-W // hs), -(-H // vs)
    return [y] + [b[:, :, hs * vs + c].transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:ch, :cw] for c in range(2)]


def upsample_h2v1(s):
    h, w = s.shape
    s = s.astype(np.int32)
    if w <= 2:                     # libjpeg takes plain replication for planes this narrow
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((h, 2 * w), np.int32)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out


def upsample_h2v2(s):
    h, w = s.shape
    s = s.astype(np.int32)
    if w <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], s[-1:]], 0)
    out = np.empty((2 * h, 2 * w), np.int32)
    for r, other in ((0, above), (1, below)):
        cs = 3 * s + other
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[r::2, 0::2], out[r::2, 1::2] = even, odd
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """uint8 [H, W, 3]: what Image.open(data).convert("RGB") holds."""
    plan = parse(data)
    planes = component_planes(plan, idct(decode_coefficients(data, plan)))
    H, W = plan["height"], plan["width"]
    if plan["ncomp"] == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2)
    up = {(1, 1): lambda s: s, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(plan["hs"], plan["vs"])]
    return colour(planes[0], up(planes[1])[:H, :W], up(planes[2])[:H, :W])


# ------------------------------------------------------------------------------------------------- subsequences (host side)
def subsequence_starts(plan, subseq_bytes):
    """The first byte (from scan_begin) of every subsequence, segment by segment: what sola_jpeg_decode cuts."""
    out = []
    for lo, hi in plan["segs"]:
        out += list(range(lo, max(hi, lo + 1), subseq_bytes))
    return out


def stuffed_case(subseq_bytes=SUBSEQ_MIN):
    """A quality-100 noise file whose scan holds stuffed FF 00 pairs, one of them with its 00 on a subsequence boundary: the first
    of a fixed list of seeds that has both (searched, so the generator does not depend on one encoder version's bytes)."""
    for seed in range(64):
        data = case(48, 40, "4:2:0", 100, "noise", "plain", seed=1000 + seed)
        plan = parse(data)
        scan = data[plan["scan_begin"]:plan["scan_end"]]
        starts = set(subsequence_starts(plan, subseq_bytes))
        hits = [i + 1 for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] == 0x00 and (i + 1) in starts]
        if hits:
            return data, plan, hits
    raise AssertionError("no seed puts a stuffed 00 on a subsequence boundary")
