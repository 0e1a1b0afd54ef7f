"""Frame preprocessing on the GPU: frames.resize_u8 against PIL.Image.resize byte for byte (every geometry of
tests/resample_cases.py, both filters, every content kind, grey and RGB), frames.preprocess / load_video_frames / gdino_image
against the host recipes under torch.equal.  Everything is exact: there is no tolerance in this file."""
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

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = 0xA5
# the output pixels one block of the fused kernel owns (SOLA_RESAMPLE_TILE_W x SOLA_RESAMPLE_TILE_H); rc.GEOMETRIES holds outputs of
# TILE + 1 and TILE - 1 on either axis and one of 3 x 3 tiles
TILE_W, TILE_H = 64, 64

_PIL = {}


def pil_frames(kind, T, H, W, Cn, size, filt):
    """(source uint8 [T,H,W,C], PIL's resize of every frame [T,h,w,C]), computed once per case and never written to."""
    key = (kind, T, H, W, Cn, size, filt)
    if key not in _PIL:
        src = rc.content(kind, T, H, W, Cn)
        want = np.stack([rc.pil_resize(f, size, filt) for f in src])
        src.setflags(write=False)
        want.setflags(write=False)
        _PIL[key] = (src, want)
    return _PIL[key]


def on_device(arr, offset=0):
    """The array as a view that starts ``offset`` bytes into a 256-byte-aligned allocation."""
    buf = torch.empty(arr.size + offset + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(np.array(arr)))  # (a copy: the shared cases are read-only)
    assert view.data_ptr() % 16 == offset % 16
    return view


def test_tile_sides_are_the_librarys():
    assert (TILE_W, TILE_H) == (rc.TILE_W, rc.TILE_H) == (frames.TILE_W, frames.TILE_H)
    hdr = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert f"#define SOLA_RESAMPLE_TILE_W {TILE_W}\n" in hdr and f"#define SOLA_RESAMPLE_TILE_H {TILE_H}\n" in hdr
    outs = [size for _, size, _ in rc.GEOMETRIES]
    assert (TILE_H + 1, TILE_W - 1) in outs and (TILE_H - 1, TILE_W + 1) in outs


@pytest.mark.parametrize("geometry", rc.GEOMETRIES + rc.LONG_GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_resize_u8_equals_pil_byte_for_byte(geometry):
    (H, W), size, filters = geometry
    for filt in filters:
        for Cn in (1, 3):
            for kind in rc.CONTENTS:
                src, want = pil_frames(kind, 1, H, W, Cn, size, filt)
                got = frames.resize_u8(on_device(src), size, filt)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + size + (Cn,) and got.is_cuda
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{filt}, C {Cn}, {kind}")
    # rank 3 in, rank 3 out
    src, want = pil_frames("uniform", 1, H, W, 3, size, filters[0])
    got = frames.resize_u8(on_device(src[0]), size, filters[0])
    assert tuple(got.shape) == size + (3,)
    np.testing.assert_array_equal(got.cpu().numpy(), want[0])


def test_the_long_reductions_take_the_two_launch_route():
    L = _lib.lib()
    for (H, W), (h, w), _ in rc.GEOMETRIES:
        tx = 0 if W == w else L.sola_resample_taps(W, w, 3)
        ty = 0 if H == h else L.sola_resample_taps(H, h, 3)
        assert L.sola_resample_u8_scratch_bytes(3, H, W, 3, h, w, tx, ty) == 0
    (H, W), (h, w), _ = rc.LONG_GEOMETRIES[0]
    assert L.sola_resample_u8_scratch_bytes(3, H, W, 3, h, w, L.sola_resample_taps(W, w, 3), L.sola_resample_taps(H, h, 3)) >= 3 * H * w * 3


@pytest.mark.parametrize("filt", rc.BOTH)
@pytest.mark.parametrize("geometry", [((53, 37), (20, 16)), ((37, 53), (64, 64)), ((150, 140), (131, 130)), ((33, 200), (33, 7)),
                                      ((3000, 40), (8, 24))], ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_three_different_frames_at_every_source_alignment(geometry, filt):
    (H, W), size = geometry
    for Cn in (1, 3):
        src, want = pil_frames("uniform", 3, H, W, Cn, size, filt)
        # (37 and 53 pixels of 1 or 3 bytes: odd row lengths W * C, so every source row starts at another alignment)
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
        for offset in (0, 1, 2, 3):
            got = frames.resize_u8(on_device(src, offset), size, filt)
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"C {Cn}, offset {offset}")


def _call(src, size, filt, table, out):
    """sola_resample_u8 into ``out`` (any device buffer) through the wrapper's own tables."""
    T, H, W, Cn = src.shape
    h, w = size
    tx, taps_x = frames._axis_table(W, w, filt, src.device)
    ty, taps_y = frames._axis_table(H, h, filt, src.device)
    need = _lib.lib().sola_resample_u8_scratch_bytes(T, H, W, Cn, h, w, taps_x, taps_y)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().sola_resample_u8(_lib.ptr(src), T, H, W, Cn, h, w, _lib.ptr(tx), taps_x, _lib.ptr(ty), taps_y, _lib.ptr(table),
                                           _lib.ptr(out), _lib.ptr(scratch), need, _lib.current_stream()), "sola_resample_u8")


@pytest.mark.parametrize("geometry", [((53, 37), (20, 16)), ((90, 70), (65, 63)), ((150, 140), (131, 130)), ((48, 27), (30, 27)),
                                      ((3000, 40), (8, 24))], ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_nothing_outside_the_output_is_written(geometry):
    (H, W), (h, w) = geometry
    table = frames.normalise_table(MEAN, STD, "sam2_video").cuda()
    for filt in rc.BOTH:
        src, want = pil_frames("uniform", 2, H, W, 3, (h, w), filt)
        d = on_device(src, 1)
        # (a float output is 4-byte aligned; at 16 bytes and w % 4 == 0 - the first geometry - the kernel stores 16 bytes per lane)
        for lut, n_bytes, pad in ((None, 2 * h * w * 3, 509), (table, 2 * 3 * h * w * 4, 512), (table, 2 * 3 * h * w * 4, 516)):
            fenced = torch.full((pad + n_bytes + 512,), SENTINEL, dtype=torch.uint8, device="cuda")
            _call(d, (h, w), filt, lut, fenced[pad:])
            host = fenced.cpu().numpy()
            assert (host[:pad] == SENTINEL).all() and (host[pad + n_bytes:] == SENTINEL).all(), f"{filt}, lut {lut is not None}"
            body = host[pad:pad + n_bytes]
            if lut is None:
                np.testing.assert_array_equal(body.reshape(2, h, w, 3), want)
            else:
                got = torch.from_numpy(body.view(np.float32).reshape(2, 3, h, w).copy())
                assert torch.equal(got, table.cpu()[torch.arange(3)[None, :, None, None], torch.from_numpy(np.array(want)).permute(0, 3, 1, 2).long()])


def _host_recipe(recipe, frames_u8):
    """The recipe on host uint8 [T,H,W,3] frames -> float32 [T,3,H,W]: SAM2's load_video_frames arithmetic / torchvision's ToTensor + Normalize."""
    m = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    T, H, W, _ = frames_u8.shape
    if recipe == "sam2_video":
        images = torch.zeros(T, 3, H, W, dtype=torch.float32)
        for n in range(T):
            images[n] = torch.from_numpy(frames_u8[n] / 255.0).permute(2, 0, 1)
        images -= m
        images /= s
        return images
    return torch.stack([torch.from_numpy(np.array(f)).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(m).div_(s)
                        for f in frames_u8])


@pytest.mark.parametrize("recipe", ["sam2_video", "to_tensor"])
@pytest.mark.parametrize("geometry", [((270, 480), (256, 256), "bicubic"), ((480, 270), (333, 187), "bilinear"),
                                      ((150, 140), (131, 130), "bicubic"), ((33, 200), (33, 7), "bilinear"),
                                      ((3000, 40), (8, 24), "bicubic")], ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_preprocess_equals_the_host_recipe_on_pil_frames(geometry, recipe):
    (H, W), size, filt = geometry
    table = frames.normalise_table(MEAN, STD, recipe)
    for kind in ("uniform", "binary"):
        src, want_u8 = pil_frames(kind, 2, H, W, 3, size, filt)
        got = frames.preprocess(on_device(src, 3), size, filt, table)  # (256 is a multiple of 4: 16-byte stores; 187, 130, 7 are not)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3) + size and got.is_cuda
        assert torch.equal(got.cpu(), _host_recipe(recipe, want_u8)), kind
    grey = frames.normalise_table((0.5,), (0.25,), recipe)
    src, want_u8 = pil_frames("uniform", 2, H, W, 1, size, filt)
    got = frames.preprocess(on_device(src), size, filt, grey.cuda())
    assert torch.equal(got.cpu(), grey[0][torch.from_numpy(np.array(want_u8)).long()].permute(0, 3, 1, 2))
    with pytest.raises(SolaError, match=r"float32 \[3,256\]"):
        frames.preprocess(on_device(pil_frames("uniform", 2, H, W, 3, size, filt)[0]), size, filt, grey)


def test_two_runs_and_a_side_stream_give_identical_bits():
    table = frames.normalise_table(MEAN, STD, "sam2_video").cuda()
    for (H, W), size in (((270, 480), (256, 256)), ((150, 140), (131, 130)), ((3000, 40), (8, 24))):
        d = on_device(rc.content("uniform", 3, H, W, 3), 1)
        first_u8, first_f = frames.resize_u8(d, size), frames.preprocess(d, size, "bicubic", table)
        assert torch.equal(frames.resize_u8(d, size), first_u8) and torch.equal(frames.preprocess(d, size, "bicubic", table), first_f)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            side_u8, side_f = frames.resize_u8(d, size), frames.preprocess(d, size, "bicubic", table)
        side.synchronize()
        assert torch.equal(side_u8, first_u8) and torch.equal(side_f, first_f)


def test_tables_are_cached_per_axis_filter_and_device():
    d = on_device(rc.content("uniform", 1, 37, 53, 3))
    frames.resize_u8(d, (20, 16), "bicubic")
    a = frames._axis_table(53, 16, "bicubic", d.device)
    assert frames._axis_table(53, 16, "bicubic", d.device)[0] is a[0] and a[1] == 15 and tuple(a[0].shape) == (16, 2 + 15)
    assert frames._axis_table(53, 16, "bilinear", d.device)[0] is not a[0]
    assert frames._axis_table(53, 53, "bicubic", d.device) == (None, 0)


# ------------------------------------------------------------------------------------------------------- SAM2's video frames
@pytest.fixture(scope="module")
def jpeg_dir(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("video")
    # 48 x 85 (height x width) frames, written out of order and under both extensions: the order is the integer stem's
    for stem, ext in ((10, ".jpg"), (2, ".jpeg"), (0, ".jpg")):
        Image.fromarray(rc.content("ramp", 1, 48, 85, 3, seed=stem)[0] ^ np.uint8(stem * 9)).save(str(d / f"{stem}{ext}"), quality=92)
    (d / "notes.txt").write_text("not a frame")
    return d


def _sam2_host(video_path, image_size):
    """sam2/utils/misc.py load_video_frames_from_jpg_images + _load_img_as_tensor, restated with PIL on the same files."""
    from PIL import Image
    names = [p for p in os.listdir(video_path) if os.path.splitext(p)[-1] in (".jpg", ".jpeg", ".JPG", ".JPEG")]
    names.sort(key=lambda p: int(os.path.splitext(p)[0]))
    images = torch.zeros(len(names), 3, image_size, image_size, dtype=torch.float32)
    for n, name in enumerate(names):
        img_pil = Image.open(os.path.join(video_path, name))
        img_np = np.array(img_pil.convert("RGB").resize((image_size, image_size)))
        img_np = img_np / 255.0
        images[n] = torch.from_numpy(img_np).permute(2, 0, 1)
        video_width, video_height = img_pil.size
    images -= torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    images /= torch.tensor(STD, dtype=torch.float32)[:, None, None]
    return images, video_height, video_width


def test_load_video_frames_equals_sam2s_recipe(jpeg_dir):
    want, vh, vw = _sam2_host(str(jpeg_dir), 64)
    assert (vh, vw) == (48, 85) and not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    images, h, w = frames.load_video_frames(str(jpeg_dir), 64, False, compute_device=torch.device("cuda"))
    assert (h, w) == (48, 85) and images.is_cuda and images.dtype == torch.float32 and tuple(images.shape) == (3, 3, 64, 64)
    assert torch.equal(images.cpu(), want)
    host, h, w = frames.load_video_frames(str(jpeg_dir), 64, True, img_mean=MEAN, img_std=STD, compute_device="cuda")
    assert (h, w) == (48, 85) and not host.is_cuda and torch.equal(host, images.cpu())
    for size in (100, 31):  # and off the tile sides, in chunks of two frames and a last one
        old, frames.CHUNK_FRAMES = frames.CHUNK_FRAMES, 2
        try:
            got = frames.load_video_frames(str(jpeg_dir), size, False)[0]
        finally:
            frames.CHUNK_FRAMES = old
        assert torch.equal(got.cpu(), _sam2_host(str(jpeg_dir), size)[0])


def test_load_video_frames_refusals(jpeg_dir, tmp_path):
    from PIL import Image
    with pytest.raises(SolaError, match="async_loading_frames"):
        frames.load_video_frames(str(jpeg_dir), 64, False, async_loading_frames=True)
    clip = tmp_path / "clip.mp4"
    clip.write_bytes(b"\0" * 16)
    with pytest.raises(SolaError, match="video files"):
        frames.load_video_frames(str(clip), 64, False)
    for stem, hw in ((0, (48, 85)), (1, (48, 85)), (2, (40, 85))):
        Image.fromarray(np.zeros(hw + (3,), np.uint8)).save(str(tmp_path / f"{stem}.jpg"))
    with pytest.raises(SolaError, match=r"2\.jpg: frame of 85x40 in a video of 85x48"):
        frames.load_video_frames(str(tmp_path), 64, False)


# ------------------------------------------------------------------------------------------------------------ GroundingDINO
def test_gdino_image_equals_pil_bilinear_and_to_tensor_normalize():
    from PIL import Image
    img = rc.content("uniform", 1, 160, 90, 3)[0]  # 90 wide, 160 tall
    w, h = rc.gdino_size(90, 160, 40, 64)
    assert (w, h) == (36, 64) == frames.gdino_size(90, 160, 40, 64)
    pil = Image.fromarray(img, "RGB")
    resized = np.asarray(pil.resize((w, h), Image.BILINEAR))
    want = _host_recipe("to_tensor", resized[None])[0]
    got = frames.gdino_image(pil, short=40, max_size=64, mean=MEAN, std=STD)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 64, 36)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(frames.gdino_image(on_device(img, 1), short=40, max_size=64), got)
    wide = np.ascontiguousarray(np.swapaxes(img, 0, 1))  # 160 wide, 90 tall -> 64 x 36
    got = frames.gdino_image(Image.fromarray(wide, "RGB"), short=40, max_size=64)
    assert tuple(got.shape) == (3, 36, 64)
    assert torch.equal(got.cpu(), _host_recipe("to_tensor", np.asarray(Image.fromarray(wide, "RGB").resize((64, 36), Image.BILINEAR))[None])[0])
    keeps = rc.content("uniform", 1, 40, 50, 3)[0]  # the short side is already 40: only the table
    assert torch.equal(frames.gdino_image(on_device(keeps), short=40, max_size=64).cpu(), _host_recipe("to_tensor", keeps[None])[0])
