"""The GPU PNG writer's host side without a GPU: the restatement of the format (png_cases.py) pinned against Python's zlib
and PIL before test_gpu_png.py uses it as the yardstick; scratch sizes and the argument checks that refuse before any launch;
the Python entry points; the --gpu_png flag."""
import ctypes
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import png_cases as pc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before it launches anything
BIG = 1 << 62
CASES = pc.small_frames()


@pytest.mark.parametrize("name,m", CASES, ids=[n for n, _ in CASES])
def test_restatement_decodes_with_zlib_and_pil(name, m):
    raw, stream = pc.raw_stream(m), pc.zlib_stream(m)
    h, w = m.shape
    assert len(raw) == h * (w + 1)
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == raw
    assert struct.unpack(">I", stream[-4:])[0] == zlib.adler32(raw)
    assert len(stream) <= pc.stream_bound(h, w)
    img = Image.open(io.BytesIO(pc.png_file(m)))
    assert img.mode == "L" and img.size == (w, h)
    np.testing.assert_array_equal(np.array(img), m * 255)


def test_vectorised_restatement_equals_the_rule_run_by_run():
    for name, m in CASES:
        if m.size <= 20000:
            raw = pc.raw_stream(m)
            assert pc.deflate_raw(raw) == pc.deflate_raw_by_rule(raw), name


def test_runs_of_every_length_decompress_to_themselves():
    """259 / 260 is where a wrong split produces an illegal 1- or 2-byte match."""
    lengths = sorted(set(range(1, 601)) | {258 * k + d for k in range(1, 9) for d in range(-3, 6)})
    for byte in (0x00, 0xFF):
        other = bytes([byte ^ 0xFF])
        for n in lengths:
            toks = pc.run_tokens(n)
            assert toks[0] == 0 and all(t == 0 or 3 <= t <= 258 for t in toks)
            assert 1 + sum(t if t else 1 for t in toks[1:]) == n
            for raw in (bytes([byte]) * n, other * 2 + bytes([byte]) * n + other):
                stream = pc.deflate_raw(raw)
                assert zlib.decompress(stream) == raw, (byte, n)
                assert stream == pc.deflate_raw_by_rule(raw), (byte, n)
                assert len(stream) <= 6 + (9 * len(raw) + 17) // 8


def test_stream_length_never_exceeds_the_bound_on_random_small_frames():
    rng = np.random.default_rng(3)
    for _ in range(300):
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        m = (rng.random((h, w)) < rng.random()).astype(np.uint8)
        s = pc.zlib_stream(m)
        assert len(s) <= pc.stream_bound(h, w)
        assert zlib.decompress(s) == pc.raw_stream(m)
    # all-0xFF-literal worst case: a full frame of width 1 alternates filter byte and pixel
    m = np.ones((50, 1), np.uint8)
    assert len(pc.zlib_stream(m)) <= pc.stream_bound(50, 1)


def test_scratch_bytes_are_the_documented_sizes():
    h = _lib.lib()

    def want(n, hh, ww):
        raw = hh * (ww + 1)
        return (n * (-(-raw // 64) * 8 + -(-raw // 16384) * 28) + 255) // 256 * 256

    for n, hh, ww in [(1, 1, 1), (3, 7, 5), (100, 720, 1280), (200, 1080, 1920), (2, 1920, 1080), (1, 300, 1)]:
        assert h.sola_png_deflate_scratch_bytes(n, hh, ww) == want(n, hh, ww)
    for bad in [(0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 32768)]:
        assert h.sola_png_deflate_scratch_bytes(*bad) == 0


def _refused(status, *words):
    assert status == -1
    msg = _lib.lib().sola_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_bad_arguments_are_refused_without_a_gpu():
    h = _lib.lib()
    ok = h.sola_png_deflate_scratch_bytes(2, 8, 8)
    for i in range(4):  # null pointers
        m, off, ad, sc = [None if j == i else FAKE for j in range(4)]
        _refused(h.sola_png_deflate_sizes(m, 0, 2, 8, 8, off, ad, sc, ok, None), "null")
    for i in range(5):
        m, off, ad, out, sc = [None if j == i else FAKE for j in range(5)]
        _refused(h.sola_png_deflate_write(m, 0, 2, 8, 8, off, ad, out, sc, ok, None), "null")
    _refused(h.sola_png_deflate_sizes(FAKE, 3, 2, 8, 8, FAKE, FAKE, FAKE, ok, None), "elem_type")
    _refused(h.sola_png_deflate_write(FAKE, -1, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, ok, None), "elem_type")
    # h*(w+1) >= 2^31 (h*w alone is below it in the second pair)
    for hh, ww in [(65536, 32768), (32768, 65535)]:
        _refused(h.sola_png_deflate_sizes(FAKE, 0, 1, hh, ww, FAKE, FAKE, FAKE, BIG, None), "too large")
        _refused(h.sola_png_deflate_write(FAKE, 1, 1, hh, ww, FAKE, FAKE, FAKE, FAKE, BIG, None), "too large")
    for n, hh, ww in [(0, 8, 8), (-3, 8, 8), (1, 0, 8), (1, 8, -1)]:
        _refused(h.sola_png_deflate_sizes(FAKE, 0, n, hh, ww, FAKE, FAKE, FAKE, BIG, None), "bad sizes")
        _refused(h.sola_png_deflate_write(FAKE, 0, n, hh, ww, FAKE, FAKE, FAKE, FAKE, BIG, None), "bad sizes")
    # short or misaligned scratch
    _refused(h.sola_png_deflate_sizes(FAKE, 0, 2, 8, 8, FAKE, FAKE, FAKE, ok - 1, None), "scratch")
    _refused(h.sola_png_deflate_write(FAKE, 2, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, 0, None), "scratch")
    _refused(h.sola_png_deflate_sizes(FAKE, 0, 2, 8, 8, FAKE, FAKE, ctypes.c_void_p((1 << 20) + 4), ok, None), "aligned")
    _refused(h.sola_png_deflate_write(FAKE, 0, 2, 8, 8, FAKE, FAKE, FAKE, ctypes.c_void_p((1 << 20) + 4), ok, None), "aligned")


def test_seg_utils_entry_points_exist_and_refuse_cpu_tensors():
    from sola_amd import seg_utils
    for name in ("png_deflate_masklet", "encode_png_masklet", "encode_png_mask", "encode_png_masklets"):
        assert callable(getattr(seg_utils, name))
    with pytest.raises(SolaError, match="GPU only"):
        seg_utils.encode_png_masklet(torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(SolaError, match="GPU only"):
        seg_utils.encode_png_mask(torch.zeros(4, 4))
    with pytest.raises(SolaError, match="GPU only"):
        seg_utils.png_deflate_masklet(torch.zeros(1, 4, 4))
    assert seg_utils.encode_png_masklets([]) == []


def test_gpu_png_flag_reaches_the_config():
    from sola_amd.config import load_configs
    root = os.path.join(os.path.dirname(HERE), "configs")
    base = ["--config", "mevis/default", "--eval_weight_epoch", "1"]
    cfg = load_configs("inference", base + ["--gpu_png", "true"], config_root=root)
    assert cfg["gpu_png"] is True
    assert "gpu_png" not in load_configs("inference", base, config_root=root)
    assert load_configs("inference", base + ["--gpu_png", "false"], config_root=root)["gpu_png"] is False


def test_inference_has_the_writer_function():
    import inspect

    import inference
    sig = inspect.signature(inference.save_masklet)
    assert list(sig.parameters) == ["dataset", "vid", "eid", "pred", "frames", "out_dir", "device", "gpu_png"]
    assert sig.parameters["gpu_png"].default is False
