"""The COCO compressed-RLE encoder's host side (sola_rle_encode_*, seg_utils.encode_rle_*) without a GPU: scratch sizes,
argument checks that refuse before any launch, and the Python entry points."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before it launches anything
BIG = 1 << 62


def test_scratch_bytes_are_the_documented_sizes():
    h = _lib.lib()
    # n * w * ceil(h/64) * 4 bytes, rounded up to 256
    assert h.sola_rle_encode_scratch_bytes(64, 720, 1280) == 64 * 1280 * 12 * 4
    assert h.sola_rle_encode_scratch_bytes(200, 1080, 1920) == 200 * 1920 * 17 * 4
    assert h.sola_rle_encode_scratch_bytes(1, 1, 1) == 256
    assert h.sola_rle_encode_scratch_bytes(3, 65, 7) == 256  # 3 * 7 * 2 * 4 = 168
    assert h.sola_rle_encode_scratch_bytes(5, 129, 33) == 2048  # 5 * 33 * 3 * 4 = 1980
    for bad in [(0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0)]:
        assert h.sola_rle_encode_scratch_bytes(*bad) == 0


def _refused(status, *words):
    assert status == -1
    msg = _lib.lib().sola_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_bad_arguments_are_refused_without_a_gpu():
    h = _lib.lib()
    ok = h.sola_rle_encode_scratch_bytes(2, 8, 8)
    # null pointers
    _refused(h.sola_rle_encode_runs(None, 0, 2, 8, 8, FAKE, FAKE, ok, None), "null")
    _refused(h.sola_rle_encode_runs(FAKE, 0, 2, 8, 8, None, FAKE, ok, None), "null")
    _refused(h.sola_rle_encode_runs(FAKE, 0, 2, 8, 8, FAKE, None, ok, None), "null")
    for i in range(5):
        args = [FAKE] * 5
        args[i] = None
        m, ro, cum, co, sc = args
        _refused(h.sola_rle_encode_cum(m, 0, 2, 8, 8, ro, cum, co, sc, ok, None), "null")
    for i in range(4):
        args = [FAKE] * 4
        args[i] = None
        _refused(h.sola_rle_encode_chars(args[0], args[1], args[2], 2, args[3], None), "null")
    # elem_type outside 0..2
    _refused(h.sola_rle_encode_runs(FAKE, 3, 2, 8, 8, FAKE, FAKE, ok, None), "elem_type")
    _refused(h.sola_rle_encode_cum(FAKE, -1, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, ok, None), "elem_type")
    # h*w >= 2^31
    _refused(h.sola_rle_encode_runs(FAKE, 0, 1, 65536, 32768, FAKE, FAKE, BIG, None), "too large")
    _refused(h.sola_rle_encode_cum(FAKE, 1, 1, 1 << 16, 1 << 15, FAKE, FAKE, FAKE, FAKE, BIG, None), "too large")
    # n <= 0, h or w <= 0
    for n, hh, ww in [(0, 8, 8), (-3, 8, 8), (1, 0, 8), (1, 8, -1)]:
        _refused(h.sola_rle_encode_runs(FAKE, 0, n, hh, ww, FAKE, FAKE, BIG, None), "bad sizes")
        _refused(h.sola_rle_encode_cum(FAKE, 0, n, hh, ww, FAKE, FAKE, FAKE, FAKE, BIG, None), "bad sizes")
    _refused(h.sola_rle_encode_chars(FAKE, FAKE, FAKE, 0, FAKE, None), "bad sizes")
    # short or misaligned scratch
    _refused(h.sola_rle_encode_runs(FAKE, 0, 2, 8, 8, FAKE, FAKE, ok - 1, None), "scratch")
    _refused(h.sola_rle_encode_cum(FAKE, 2, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, 0, None), "scratch")
    _refused(h.sola_rle_encode_runs(FAKE, 0, 2, 8, 8, FAKE, ctypes.c_void_p((1 << 20) + 2), ok, None), "aligned")


def test_seg_utils_entry_points_exist_and_refuse_cpu_tensors():
    from sola_amd import seg_utils
    for name in ("encode_rle_masklet", "encode_rle_masklet_torch", "encode_rle_mask", "encode_rle_masklets"):
        assert callable(getattr(seg_utils, name))
    assert seg_utils.encode_rle_masklet_torch is seg_utils.encode_rle_masklet
    with pytest.raises(SolaError, match="GPU only"):
        seg_utils.encode_rle_masklet(torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(SolaError, match="GPU only"):
        seg_utils.encode_rle_mask(torch.zeros(4, 4))
    assert seg_utils.encode_rle_masklets([]) == []
