"""Baseline JPEG decode without a GPU: tests/jpeg_cases.py's numpy restatement against Pillow in every byte over the grid of sizes,
samplings, qualities, contents and encoder modes; sola_jpeg_parse against the restatement's parse field for field; every refusal with
its message; every truncation point of a small file; the symbols declared, exported and bound."""
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import jpeg_cases as jc  # noqa: E402
from sola_amd import _lib, frames  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

SYMBOLS = ["sola_jpeg_parse", "sola_jpeg_scratch_bytes", "sola_jpeg_decode", "sola_jpeg_coefficients", "sola_jpeg_profile"]


def test_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["sola_jpeg_scratch_bytes"][0] is C.c_size_t
    # the ctypes mirror of the plan has the header's layout: the kernels copy its tables as 16-byte words
    assert C.sizeof(frames.SolaJpegHuff) == 912 and C.sizeof(frames.SolaJpegPlan) == 80 + 384 + 6 * 912
    assert frames.SolaJpegPlan.huff.offset % 16 == 0 and C.sizeof(frames.SolaJpegPlan) % 16 == 0
    assert "jpeg.hip" in open(os.path.join(ROOT, "sola_amd", "csrc", "Makefile")).read()
    assert frames.load_video_frames.__kwdefaults__ is None and frames.load_video_frames.__defaults__[-1] == "pil"


@pytest.mark.parametrize("size", jc.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_is_pillow(size):
    n = 0
    for (w, h, s, q, c, m) in jc.grid():
        if (w, h) != size:
            continue
        data = jc.case(w, h, s, q, c, m)
        assert np.array_equal(jc.decode(data), jc.pillow_rgb(data)), (w, h, s, q, c, m)
        n += 1
    assert n == len(jc.SAMPLINGS) * len(jc.QUALITIES) * len(jc.CONTENTS) * len(jc.MODES)


def test_restatement_on_narrow_planes():
    for (w, h) in [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (6, 9), (2, 17), (16, 1), (1, 16)]:
        for s in jc.SAMPLINGS:
            data = jc.case(w, h, s, 90, "noise")
            assert np.array_equal(jc.decode(data), jc.pillow_rgb(data)), (w, h, s)


def same_plan(data):
    want = jc.parse(data)
    plan, segs = frames.jpeg_parse(data)
    for f in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "blocks_per_mcu", "n_blocks", "restart_interval", "n_segments", "scan_begin",
              "scan_end"):
        assert getattr(plan, f) == want[f], f
    assert (plan.scan_offset, plan.seg_offset) == (0, 0)
    assert segs.tolist() == [list(s) for s in want["segs"]]
    for c in range(want["ncomp"]):
        assert np.array_equal(np.ctypeslib.as_array(plan.quant[c]), want["quant"][c]), c
        for k in range(2):
            look, limit, valoff, vals = want["huff"][2 * c + k]
            h = plan.huff[2 * c + k]
            assert np.array_equal(np.ctypeslib.as_array(h.look), look) and np.array_equal(np.ctypeslib.as_array(h.vals), vals)
            assert np.array_equal(np.ctypeslib.as_array(h.limit)[1:17], limit[1:17]) and np.array_equal(np.ctypeslib.as_array(h.valoff)[1:17], valoff[1:17])


def test_parse_is_the_restatements():
    for s in jc.SAMPLINGS:
        for m in jc.MODES + ["restart1", "restart2+optimize"]:
            for (w, h) in [(40, 52), (33, 47), (9, 65)]:
                same_plan(jc.case(w, h, s, 75, "noise", m))
    data = jc.case(256, 192, "4:2:0", 95, "noise", "restart1")  # more segments than the binding's first buffer holds
    assert jc.parse(data)["n_segments"] == 192
    same_plan(data)
    info = frames.jpeg_info(jc.case(33, 47, "4:2:2", 75, "noise", "restart3"))
    assert info == {"size": (33, 47), "mode": "RGB", "sampling": "4:2:2", "restart_interval": 3}
    assert frames.jpeg_info(jc.case(9, 65, "grey"))["mode"] == "L"


def test_skipped_segments_and_orientation():
    arr = jc.image(24, 31, "noise", 3)
    exif = Image.Exif()
    exif[0x0112] = 6  # orientation: PIL's convert("RGB") ignores it, so does the parser
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=80, exif=exif, comment=b"a comment segment", icc_profile=b"x" * 500)
    data = buf.getvalue()
    assert b"Exif" in data and b"a comment segment" in data
    same_plan(data)
    assert np.array_equal(jc.decode(data), jc.pillow_rgb(data))


# ------------------------------------------------------------------------------------------------------------------ refusals
def patched(data, marker, offset, value):
    """The file with byte `offset` of the payload of the first `marker` segment set to `value`."""
    at = data.index(bytes([0xFF, marker]))
    b = bytearray(data)
    b[at + 4 + offset] = value
    return bytes(b)


def with_segment(data, marker, payload, before=0xDA):
    at = data.index(bytes([0xFF, before]))
    n = len(payload) + 2
    return data[:at] + bytes([0xFF, marker, n >> 8, n & 255]) + payload + data[at:]


def refusals():
    base = jc.case(40, 52, "4:2:0", 75, "noise")
    plan = jc.parse(base)
    sb = plan["scan_begin"]
    cmyk = io.BytesIO()
    Image.fromarray(jc.image(16, 16, "noise", 0)).convert("CMYK").save(cmyk, "JPEG")
    adobe = lambda t: b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([t])
    sof = base.index(b"\xff\xc0")
    two_scans = base[:-2] + base[base.index(b"\xff\xda"):]
    no_dht = base[:base.index(b"\xff\xc4")] + base[base.index(b"\xff\xda"):]
    return [
        ("progressive", jc.encode(jc.image(16, 16, "noise", 0), progressive=True), "progressive"),
        ("cmyk", cmyk.getvalue(), "four components"),
        ("extended", base[:sof] + b"\xff\xc1" + base[sof + 2:], "extended sequential"),
        ("lossless", base[:sof] + b"\xff\xc3" + base[sof + 2:], "lossless"),
        ("arithmetic", base[:sof] + b"\xff\xc9" + base[sof + 2:], "arithmetic"),
        ("12-bit", patched(base, 0xC0, 0, 12), "12-bit samples"),
        ("16-bit-dqt", patched(base, 0xDB, 0, 0x10), "16-bit quantisation tables"),
        ("adobe-0", with_segment(base, 0xEE, adobe(0)), "Adobe segment with transform 0"),
        ("adobe-2", with_segment(base, 0xEE, adobe(2)), "Adobe segment with transform 2"),
        ("4:4:0", patched(base, 0xC0, 7, 0x12), "4:4:0"),
        ("4:1:1", patched(base, 0xC0, 7, 0x41), "4:1:1"),
        ("subsampled-luma", patched(patched(patched(base, 0xC0, 7, 0x11), 0xC0, 10, 0x22), 0xC0, 13, 0x22), "subsampled luma"),
        ("chroma-2x1", patched(patched(base, 0xC0, 10, 0x21), 0xC0, 13, 0x21), "chroma 2x1"),
        ("two-scans", two_scans, "more than one scan"),
        ("non-interleaved", patched(base, 0xDA, 0, 1), "more than one scan"),
        ("dnl", with_segment(base, 0xDC, b"\x00\x34"), "DNL marker"),
        ("dnl-in-scan", base[:sb + 40] + b"\xff\xdc\x00\x04\x00\x34" + base[sb + 40:], "DNL marker"),
        ("fill-byte", base[:sb + 40] + b"\xff\xff\x00" + base[sb + 40:], "fill byte inside the scan"),
        ("marker-in-scan", base[:sb + 40] + b"\xff\xe1" + base[sb + 40:], "marker 0xE1 inside the scan"),
        ("rst-without-dri", base[:sb + 40] + b"\xff\xd0" + base[sb + 40:], "restart marker in a scan without a restart interval"),
        ("missing-huffman", no_dht, "missing table: DC Huffman table 0"),
        ("missing-quant", patched(base, 0xC0, 8, 3), "missing table: quantisation table 3"),
        ("width-0", patched(patched(base, 0xC0, 3, 0), 0xC0, 4, 0), "width and height must be 1 .. 16384"),
        ("height-0", patched(patched(base, 0xC0, 1, 0), 0xC0, 2, 0), "width and height must be 1 .. 16384"),
        ("width-16385", patched(patched(base, 0xC0, 3, 0x40), 0xC0, 4, 0x01), "width and height must be 1 .. 16384"),
        ("length-past-the-end", patched(base, 0xDB, -2, 0xFF), "beyond the file"),
        ("not-jpeg", b"\x89PNG\r\n\x1a\n" + base, "not a JPEG file"),
    ]


@pytest.mark.parametrize("name,data,message", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_say_which(name, data, message):
    with pytest.raises(SolaError, match=re.escape(message)):
        frames.jpeg_info(data)


def test_restart_markers_out_of_order_are_refused():
    data = jc.case(33, 47, "4:2:0", 75, "noise", "restart1")
    at = data.index(b"\xff\xd1")
    with pytest.raises(SolaError, match="RST2 where RST1 is due"):
        frames.jpeg_info(data[:at] + b"\xff\xd2" + data[at + 2:])
    extra = data[:at] + b"\xff\xd1\x00\xff\xd2\x00\xff\xd3\x00" * 4 + data[at + 2:]
    with pytest.raises(SolaError, match="RST|more restart segments"):
        frames.jpeg_info(extra)


def test_every_truncation_point():
    data = jc.case(17, 13, "4:2:0", 75, "noise", "restart1")
    accepted = 0
    for cut in range(len(data)):
        buf = (C.c_uint8 * max(cut, 1)).from_buffer_copy(data[:cut] or b"\0")
        plan, segs = frames.SolaJpegPlan(), np.full((8, 2), -1, np.int32)
        status = _lib.lib().sola_jpeg_parse(buf, cut, C.byref(plan), C.c_void_p(segs.ctypes.data), 8)
        if status != 0:
            assert status == -1 and _lib.lib().sola_last_error()
            continue
        accepted += 1
        assert 0 <= plan.scan_begin <= plan.scan_end <= cut and 1 <= plan.n_segments <= 2
        for lo, hi in segs[:plan.n_segments]:
            assert 0 <= lo <= hi <= plan.scan_end - plan.scan_begin
    assert 0 < accepted < len(data)  # cuts inside the scan are accepted (the scan ends with the buffer), cuts in the header are not


def test_scratch_and_decode_refuse_before_any_launch():
    L = _lib.lib()
    plan, segs = frames.jpeg_parse(jc.case(40, 52))
    plans = (frames.SolaJpegPlan * 1)(plan)
    assert L.sola_jpeg_scratch_bytes(plans, 1, 0) > 0 and L.sola_jpeg_scratch_bytes(plans, 1, jc.SUBSEQ_MIN) > 0
    for bad in (8, 24, 8192, -16):
        assert L.sola_jpeg_scratch_bytes(plans, 1, bad) == 0 and b"subseq_bytes" in L.sola_last_error()
    assert L.sola_jpeg_scratch_bytes(plans, 0, 0) == 0
    other, _ = frames.jpeg_parse(jc.case(40, 52, "4:2:2"))
    assert L.sola_jpeg_scratch_bytes((frames.SolaJpegPlan * 2)(plan, other), 2, 0) == 0 and b"differs from frame 0" in L.sola_last_error()
    err = (C.c_int32 * 1)()
    assert L.sola_jpeg_decode(None, 0, None, 0, plans, None, 1, 0, None, None, 0, err, None, None) == -1 and b"null" in L.sola_last_error()
    with pytest.raises(SolaError, match="GPU only"):
        frames.decode_jpeg([jc.case(16, 16)], device="cpu")
