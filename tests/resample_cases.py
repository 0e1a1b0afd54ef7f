"""Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py: a numpy restatement of Pillow's 8-bit two-pass resize
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal and the vertical 8bpc pass) and of
GroundingDINO's size rule, the geometry list, and the content generators.  The restatement is checked against PIL itself on the
whole list (test_resample_cpu.py); the GPU tests compare with PIL directly."""
import math

import numpy as np

FILTER_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
PRECISION_BITS = 32 - 8 - 2
TILE_W = TILE_H = 64  # SOLA_RESAMPLE_TILE_W / _H: the output pixels one block of the fused kernel owns


def pil_filter(name):
    from PIL import Image
    return {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name]


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def taps(in_size, out_size, filt):
    return int(math.ceil(FILTER_SUPPORT[filt] * max(in_size / out_size, 1.0))) * 2 + 1


def coeffs(in_size, out_size, filt):
    """(bounds int32 [out,2], k int32 [out,taps]): python floats are C doubles, every operation is rounded on its own."""
    f = _bilinear if filt == "bilinear" else _bicubic
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filt] * fs
    n_taps = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, n_taps), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, k


def _pass_axis0(img, out_size, filt):
    """One 8-bit pass along axis 0 of a uint8 array: accumulator 1 << 21, + pixel * k, >> 22, clamp to a byte."""
    bounds, k = coeffs(img.shape[0], out_size, filt)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for o in range(out_size):
        lo, n = bounds[o]
        acc = np.tensordot(k[o, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, size, filt):
    """uint8 [H,W] or [H,W,C] -> (h, w): horizontal pass first, a byte image in between, an axis that keeps its size is skipped."""
    h, w = size
    if img.shape[1] != w:
        img = np.swapaxes(_pass_axis0(np.swapaxes(img, 0, 1), w, filt), 0, 1)
    if img.shape[0] != h:
        img = _pass_axis0(img, h, filt)
    return np.ascontiguousarray(img)


def pil_resize(img, size, filt):
    """The same through PIL: [H,W,C] with C 1 (mode "L") or 3 ("RGB")."""
    from PIL import Image
    h, w = size
    if img.shape[2] == 1:
        return np.asarray(Image.fromarray(img[:, :, 0], "L").resize((w, h), pil_filter(filt)))[:, :, None]
    return np.asarray(Image.fromarray(img, "RGB").resize((w, h), pil_filter(filt)))


def gdino_size(w, h, short=800, max_size=1333):
    """GroundingDINO datasets/transforms.py get_size_with_aspect_ratio, as (w, h)."""
    size = short
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


# (H, W) -> (h, w); the filters each runs with.  The issue's list, as heights x widths, and both orientations of the long ones.
BOTH = ("bicubic", "bilinear")
GEOMETRIES = [
    ((53, 37), (20, 16), BOTH),
    ((53, 37), (64, 64), BOTH),
    ((37, 53), (16, 20), BOTH),
    ((480, 270), (256, 256), BOTH),
    ((270, 480), (256, 256), BOTH),
    ((480, 270), (333, 187), ("bilinear",)),
    ((7, 200), (200, 7), BOTH),       # 200 -> 7: 117 bicubic taps
    ((200, 7), (7, 200), BOTH),
    ((5, 3), (41, 50), BOTH),
    ((1, 1), (4, 4), BOTH),
    ((64, 64), (1, 1), BOTH),
    ((200, 33), (7, 33), BOTH),       # one axis only: the horizontal pass is skipped
    ((33, 200), (33, 7), BOTH),       # ... the vertical one
    ((48, 27), (30, 27), BOTH),
    ((27, 48), (27, 30), BOTH),
    ((29, 31), (29, 31), BOTH),       # nothing changes
    ((90, 70), (TILE_H + 1, TILE_W - 1), BOTH),   # one more / one less than the fused kernel's tile sides
    ((70, 90), (TILE_H - 1, TILE_W + 1), BOTH),
    ((150, 140), (2 * TILE_H + 3, 2 * TILE_W + 2), BOTH),  # 3 x 3 tiles, upscale of one axis and downscale of the other
    ((609, 600), (200, 200), BOTH),   # 3 x down: the fused kernel stages a tile's source rows in several rounds
]
# a reduction whose staging does not fit the fused kernel's LDS: the two-launch route through scratch
LONG_GEOMETRIES = [((3000, 40), (8, 24), BOTH), ((2600, 9), (5, 9), BOTH)]
AXES = [(1920, 1024), (1080, 1024), (1920, 1333), (1080, 750), (1280, 1024), (720, 1024)]

CONTENTS = ("uniform", "binary", "ramp", "zeros", "full")


def content(kind, T, H, W, C, seed=0):
    """uint8 [T,H,W,C]: uniform noise, 0/255 noise (clips on both sides under bicubic), ramps, constant 0 and constant 255."""
    rng = np.random.default_rng(seed + 1000 * H + W + 7 * C)
    if kind == "uniform":
        return rng.integers(0, 256, size=(T, H, W, C), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, size=(T, H, W, C), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        base = [(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 255 // max(W + H - 2, 1))]
        img = np.stack([base[c % 3] for c in range(C)], axis=-1).astype(np.uint8)
        return np.stack([np.roll(img, t, axis=1) for t in range(T)])
    if kind == "zeros":
        return np.zeros((T, H, W, C), np.uint8)
    if kind == "full":
        return np.full((T, H, W, C), 255, np.uint8)
    raise ValueError(kind)
