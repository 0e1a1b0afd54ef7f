"""What csrc/mask_elems.h states once - which element values count as a set pixel - pinned at every entry point that reads
masks.  One numpy statement of the predicate (x != 0 for uint8 and float32 masks, x > 0 for float32 logits); every entry
point must give on x what it gives on the binary uint8 image pred(x), both computed on the device by the library.  The
values are the ones on which copies of the predicate could drift apart: 128 and 255 (the carry of the word-parallel byte
test), both zeros, both signs, denormals, infinities and NaN (set for `!= 0`, clear for `> 0`), each at every position
mod 16 of a row.  Two shapes: 16-byte vectors everywhere (aligned base, width a multiple of 16), and 5 x 19 one element into
its allocation (scalar and edge reads, rows that cross vectors, piece head and tail).  Integers throughout: equality."""
import functools

import numpy as np
import pytest
import torch

from sola_amd import seg_utils as su

pytestmark = pytest.mark.gpu

U8_VALUES = np.array([0, 1, 127, 128, 255], np.uint8)
F32_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1e-45, -1e-45, np.inf, -np.inf, np.nan], np.float32)
KINDS = {"uint8": (U8_VALUES, False), "float32": (F32_VALUES, False), "logits": (F32_VALUES, True)}
SHAPES = {"vector": (2, 4, 32, 0), "edges": (2, 5, 19, 1)}  # n, h, w, elements between the allocation and the view


def pred(x, logits):
    with np.errstate(invalid="ignore"):
        return ((x > 0) if logits else (x != 0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """(x on the device as laid out by `shape`, pred(x) as an aligned uint8 device tensor, logits)."""
    values, logits = KINDS[kind]
    n, h, w, shift = SHAPES[shape]
    r, c = np.divmod(np.arange(n * h * w), w)  # rows of all frames, one after the other
    which = (c % 16 + r + n * h * (c // 16)) % len(values)
    for v in range(len(values)):  # every value at every position mod 16 of a row
        assert set((c % 16)[which == v]) == set(range(min(w, 16))), (kind, shape, v)
    host = values[which].reshape(n, h, w)
    buf = torch.zeros(n * h * w + shift, dtype=torch.from_numpy(values).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[shift:].view(n, h, w)
    x.copy_(torch.from_numpy(host))
    assert x.data_ptr() == buf.data_ptr() + shift * buf.element_size() and x.is_contiguous()
    return x, torch.from_numpy(pred(host, logits)).cuda(), logits


def same(got, want, what):
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if torch.is_tensor(g):
            assert g.shape == w.shape and torch.equal(g, w), f"{what}: output {i} differs between x and pred(x)"
        else:
            assert g == w, f"{what}: output {i} differs between x and pred(x)"


CASES = [(k, s) for k in KINDS for s in SHAPES]
ids = [f"{k}-{s}" for k, s in CASES]


@pytest.mark.parametrize("kind,shape", [c for c in CASES if c[0] != "logits"], ids=[i for i in ids if "logits" not in i])
def test_pack_masks(kind, shape):
    x, b, _ = case(kind, shape)
    same(su.pack_masks(x), su.pack_masks(b), "pack_masks")


@pytest.mark.parametrize("kind,shape", CASES, ids=ids)
def test_encode_rle_masklet(kind, shape):
    x, b, logits = case(kind, shape)
    same(su.encode_rle_masklet(x, logits=logits, return_cum=True), su.encode_rle_masklet(b, return_cum=True), "encode_rle_masklet")


@pytest.mark.parametrize("kind,shape", CASES, ids=ids)
def test_png_deflate_masklet(kind, shape):
    x, b, logits = case(kind, shape)
    same(su.png_deflate_masklet(x, logits=logits), su.png_deflate_masklet(b), "png_deflate_masklet")


@pytest.mark.parametrize("kind,shape", CASES, ids=ids)
def test_mask_logit_stats(kind, shape):
    x, b, logits = case(kind, shape)
    got = su.mask_logit_stats(x, 0.0, 1.0, logits=logits)  # n_hi and n_lo of logits are counts at +1 and -1: not compared
    same(got[:, 2:], su.mask_logit_stats(b, logits=False)[:, 2:], "mask_logit_stats (area, box)")


@pytest.mark.parametrize("kind,shape", CASES, ids=ids)
def test_connected_components(kind, shape):
    x, b, logits = case(kind, shape)
    same(su.connected_components(x, logits=logits)[0], su.connected_components(b)[0], "connected_components labels")


@pytest.mark.parametrize("kind,shape", [c for c in CASES if c[0] != "float32"], ids=[i for i in ids if "float32" not in i])
def test_pack_masklet_bilinear(kind, shape):
    # at the source size; plain float32 is resampled as values there, not read through the predicate
    x, b, logits = case(kind, shape)
    hw = tuple(x.shape[1:])
    same(su.pack_masklet_bilinear(x, hw, logits=logits), su.pack_masklet_bilinear(b, hw), "pack_masklet_bilinear")
