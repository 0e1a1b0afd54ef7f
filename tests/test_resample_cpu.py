"""Frame preprocessing without a GPU: the numpy restatement of tests/resample_cases.py against PIL itself, sola_resample_coeffs /
sola_resample_taps against the restatement, the normalisation tables against their recipes run on the host, GroundingDINO's size
rule, and the argument checks of sola_resample_u8 (refused before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import resample_cases as rc  # noqa: E402
from sola_amd import _lib, frames  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _err():
    return _lib.lib().sola_last_error().decode()


def test_symbols_are_declared_and_loadable():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    for name in ("sola_resample_taps", "sola_resample_coeffs", "sola_resample_u8_scratch_bytes", "sola_resample_u8"):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in hdr
    from PIL import Image
    assert frames.FILTERS == {"bilinear": int(Image.BILINEAR), "bicubic": int(Image.BICUBIC)}
    for k, v in (("BILINEAR", 2), ("BICUBIC", 3), ("MAX_SIZE", frames.MAX_SIZE), ("TILE_W", rc.TILE_W), ("TILE_H", rc.TILE_H)):
        assert f"#define SOLA_RESAMPLE_{k} {v}\n" in hdr
    assert (frames.TILE_W, frames.TILE_H) == (rc.TILE_W, rc.TILE_H)
    mk = open(os.path.join(ROOT, "sola_amd", "csrc", "Makefile")).read()
    assert "FLAGS_resample = -ffp-contract=off" in mk and " resample.hip " in mk


@pytest.mark.parametrize("geometry", rc.GEOMETRIES + rc.LONG_GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_restatement_equals_pil_on_every_pixel(geometry):
    (H, W), size, filters = geometry
    for filt in filters:
        for Cn in (1, 3):
            for kind in rc.CONTENTS:
                img = rc.content(kind, 1, H, W, Cn)[0]
                got, want = rc.resize(img, size, filt), rc.pil_resize(img, size, filt)
                assert got.shape == want.shape == size + (Cn,)
                np.testing.assert_array_equal(got, want, err_msg=f"{filt}, C {Cn}, {kind}")


def _axes():
    axes = set(rc.AXES)
    for (H, W), (h, w), _ in rc.GEOMETRIES + rc.LONG_GEOMETRIES:
        axes |= {(H, h), (W, w)}
    return sorted(axes)


def test_library_coefficients_equal_the_restatement():
    assert {(1920, 1024), (1080, 1024), (1920, 1333)} <= set(_axes())
    for n_in, n_out in _axes():
        for filt in rc.BOTH:
            bounds, k = frames.resample_coeffs(n_in, n_out, filt)
            want_b, want_k = rc.coeffs(n_in, n_out, filt)
            assert bounds.dtype == k.dtype == np.int32
            np.testing.assert_array_equal(bounds, want_b, err_msg=f"{n_in} -> {n_out} {filt}")
            np.testing.assert_array_equal(k, want_k, err_msg=f"{n_in} -> {n_out} {filt}")
            # what the kernels rely on: the windows ascend and stay inside the source, the accumulator cannot overflow
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= n_in).all()
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()
            assert 255 * int(np.abs(k).sum(axis=1).max()) + (1 << 21) < 1 << 31


def test_taps_values():
    L = _lib.lib()
    # ceil(support * max(in / out, 1)) * 2 + 1; support 1 (bilinear, PIL's filter 2) / 2 (bicubic, 3)
    for n_in, n_out, filt, want in ((1920, 1024, 3, 9), (1080, 1024, 3, 7), (1920, 1333, 2, 5), (200, 7, 3, 117), (200, 7, 2, 59),
                                    (3, 50, 3, 5), (3, 50, 2, 3), (1, 1, 2, 3), (64, 1, 3, 257), (16384, 1, 3, 65537), (1080, 750, 2, 5)):
        assert L.sola_resample_taps(n_in, n_out, filt) == want == rc.taps(n_in, n_out, "bilinear" if filt == 2 else "bicubic")
    for filt in (0, 1, 4, 5, -1):
        assert L.sola_resample_taps(10, 5, filt) == -1 and f"filter {filt}" in _err()
    for n_in, n_out in ((0, 5), (5, 0), (-1, 5), (16385, 5), (5, 16385)):
        assert L.sola_resample_taps(n_in, n_out, 3) == -1 and "outside 1 .. 16384" in _err()
    b, k = np.zeros((5, 2), np.int32), np.zeros((5, 9), np.int32)
    pb, pk = C.c_void_p(b.ctypes.data), C.c_void_p(k.ctypes.data)
    assert L.sola_resample_coeffs(10, 5, 1, pb, pk) == -1 and "filter 1" in _err()
    assert L.sola_resample_coeffs(10, 0, 3, pb, pk) == -1 and "outside" in _err()
    assert L.sola_resample_coeffs(10, 5, 3, None, pk) == -1 and "null bounds" in _err()
    assert L.sola_resample_coeffs(10, 5, 3, pb, None) == -1 and "null coeffs" in _err()
    with pytest.raises(SolaError):
        frames.resample_coeffs(10, 5, "lanczos")
    # a hand-worked axis: 4 -> 2 bilinear, scale 2, support 2, 5 taps; output 0 is centred on 1.0 and reaches sources 0..2
    bounds, k = frames.resample_coeffs(4, 2, "bilinear")
    assert bounds.tolist() == [[0, 3], [1, 3]]
    # weights (0.75, 0.75, 0.25) / 1.75 and its mirror image
    assert k.tolist() == [[1797559, 1797559, 599186, 0, 0], [599186, 1797559, 1797559, 0, 0]]
    bounds, k = frames.resample_coeffs(2, 4, "bilinear")  # upscale: 3 taps, plain linear interpolation weights
    assert bounds.tolist() == [[0, 1], [0, 2], [0, 2], [1, 1]]
    assert k.tolist() == [[1 << 22, 0, 0], [3 << 20, 1 << 20, 0], [1 << 20, 3 << 20, 0], [1 << 22, 0, 0]]


def _host_recipe(recipe, img, mean, std):
    """The recipe itself on a host uint8 [H,W,3] image -> float32 [3,H,W]."""
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    if recipe == "sam2_video":  # sam2/utils/misc.py _load_img_as_tensor + load_video_frames_from_jpg_images
        img_np = img / 255.0
        images = torch.zeros(1, 3, img.shape[0], img.shape[1], dtype=torch.float32)
        images[0] = torch.from_numpy(img_np).permute(2, 0, 1)
        images -= m
        images /= s
        return images[0]
    # torchvision ToTensor (uint8 HWC -> CHW, .to(float32).div(255)) and Normalize (tensor.sub_(mean).div_(std))
    t = torch.from_numpy(img).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(m).div_(s)


@pytest.mark.parametrize("recipe", ["sam2_video", "to_tensor"])
def test_normalise_table_equals_the_recipe_on_every_byte(recipe):
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # 256 x 1 x 3: byte v in every channel of row v
    for mean, std in ((MEAN, STD), ((0.5, 0.25, 0.1), (0.3, 1.0, 0.01))):
        table = frames.normalise_table(mean, std, recipe)
        assert table.dtype == torch.float32 and tuple(table.shape) == (3, 256) and not table.is_cuda
        assert torch.equal(table, _host_recipe(recipe, img, mean, std)[:, :, 0])
    assert tuple(frames.normalise_table((0.5,), (0.5,), recipe).shape) == (1, 256)
    with pytest.raises(SolaError):
        frames.normalise_table(MEAN, STD, "imagenet")
    with pytest.raises(SolaError):
        frames.normalise_table((0.5, 0.5), (0.5, 0.5), recipe)


def test_gdino_size_on_hand_worked_cases():
    assert frames.gdino_size(1920, 1080) == (1333, 750)   # 1920/1080 * 800 > 1333: short = round(1333 * 1080 / 1920) = 750
    assert frames.gdino_size(1080, 1920) == (750, 1333)
    assert frames.gdino_size(640, 480) == (1066, 800)     # int(800 * 640 / 480)
    assert frames.gdino_size(480, 640) == (800, 1066)
    assert frames.gdino_size(1200, 800) == (1200, 800)    # the short side is already 800
    assert frames.gdino_size(1333, 750) == (1333, 750)
    assert frames.gdino_size(500, 500) == (800, 800)
    assert frames.gdino_size(160, 90, 40, 64) == (64, 36)  # short = round(64 * 90 / 160) = 36
    for w, h, short, max_size in ((1920, 1080, 800, 1333), (333, 500, 800, 1333), (1000, 37, 40, 64), (90, 160, 40, 64), (640, 480, 800, None)):
        assert frames.gdino_size(w, h, short, max_size) == rc.gdino_size(w, h, short, max_size)


def _u8(src=0x10000, T=1, H=10, W=12, Cn=3, h=5, w=6, tx=0x20000, taps_x=5, ty=0x30000, taps_y=5, lut=None, out=0x40000, scratch=None,
        scratch_bytes=0):
    return _lib.lib().sola_resample_u8(src, T, H, W, Cn, h, w, tx, taps_x, ty, taps_y, lut, out, scratch, scratch_bytes, None)


def test_resample_u8_argument_errors_without_gpu():
    assert _u8(src=None) == -1 and "null src" in _err()
    assert _u8(out=None) == -1 and "null out" in _err()
    for Cn in (0, 2, 4):
        assert _u8(Cn=Cn) == -1 and f"C = {Cn}" in _err()
    assert _u8(T=-1) == -1 and "negative T" in _err()
    for kw in ({"H": 0}, {"W": 0}, {"h": 0}, {"w": 0}, {"h": -3}):
        assert _u8(**kw) == -1 and "empty axis" in _err()
    for kw in ({"H": 16385}, {"W": 16385}, {"h": 16385}, {"w": 16385}):
        assert _u8(**kw) == -1 and "beyond 16384" in _err()
    assert _u8(tx=None) == -1 and "go together" in _err()              # taps without a table
    assert _u8(taps_y=0) == -1 and "go together" in _err()             # a table without taps
    assert _u8(taps_x=-1) == -1 and "outside 0" in _err()
    assert _u8(tx=None, taps_x=0) == -1 and "null table_x but w 6 != W 12" in _err()
    assert _u8(ty=None, taps_y=0) == -1 and "null table_y but h 5 != H 10" in _err()
    assert _u8(tx=0x20002) == -1 and "4-byte aligned" in _err()
    assert _u8(lut=0x50000, out=0x40002) == -1 and "float32 output must be 4-byte aligned" in _err()
    # a long reduction takes the two-launch route: its scratch is checked before the first launch
    L = _lib.lib()
    long = dict(H=3000, W=40, h=8, w=24, taps_x=L.sola_resample_taps(40, 24, 3), taps_y=L.sola_resample_taps(3000, 8, 3))
    need = L.sola_resample_u8_scratch_bytes(2, 3000, 40, 3, 8, 24, long["taps_x"], long["taps_y"])
    assert need >= 2 * 3000 * 24 * 3 and need % 256 == 0
    assert _u8(T=2, **long) == -1 and f"scratch of 0 bytes, sola_resample_u8_scratch_bytes asks for {need}" in _err()
    assert _u8(T=2, scratch=0x60000, scratch_bytes=1000, **long) == -1 and "scratch of 1000 bytes" in _err()
    # the one-launch geometries need none; nothing to do: no pointer is looked at
    assert L.sola_resample_u8_scratch_bytes(64, 1080, 1920, 3, 1024, 1024, 9, 7) == 0
    assert L.sola_resample_u8_scratch_bytes(1, 1080, 1920, 3, 750, 1333, 5, 5) == 0
    assert L.sola_resample_u8_scratch_bytes(1, 200, 7, 3, 7, 200, 5, 117) == 0
    assert L.sola_resample_u8_scratch_bytes(2, 2600, 9, 3, 5, 9, 0, L.sola_resample_taps(2600, 5, 3)) == 0  # no horizontal pass: nothing in between
    assert _u8(T=0, src=None, out=None) == 0
    assert _u8(T=0, Cn=2) == -1  # but the arguments are still checked


def test_cpu_tensors_raise():
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    table = frames.normalise_table(MEAN, STD)
    for call in (lambda: frames.resize_u8(img, (4, 4)), lambda: frames.resize_u8(img[0], (4, 4), "bilinear"),
                 lambda: frames.preprocess(img, (4, 4), "bicubic", table), lambda: frames.gdino_image(img[0])):
        with pytest.raises(SolaError, match="GPU only"):
            call()


def test_load_video_frames_refusals_without_gpu(tmp_path):
    with pytest.raises(SolaError, match="async_loading_frames"):
        frames.load_video_frames(str(tmp_path), 64, False, async_loading_frames=True)
    with pytest.raises(SolaError, match="video files"):
        frames.load_video_frames(str(tmp_path / "clip.mp4"), 64, False)
    with pytest.raises(SolaError, match="no JPEG frames"):
        frames.load_video_frames(str(tmp_path), 64, False)
    with pytest.raises(SolaError, match="GPU only"):
        (tmp_path / "0.jpg").write_bytes(b"")
        frames.load_video_frames(str(tmp_path), 64, False, compute_device="cpu")
    assert 1 <= frames.READER_THREADS <= 16 and frames.CHUNK_FRAMES >= 1
    assert "cpu_count" not in open(os.path.join(ROOT, "sola_amd", "frames.py")).read()
