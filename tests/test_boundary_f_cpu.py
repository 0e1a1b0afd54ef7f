"""Host side of the DAVIS boundary F (no GPU): the numpy restatement against hand-derived vectors, the radius, the
per-frame F from counts, and the argument checks of sola_mask_select_boundary_counts."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import boundary_cases as bc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402


def _set(b):
    return {(int(y), int(x)) for y, x in zip(*np.nonzero(b))}


def test_boundary_map_hand_vectors():
    h, w = 7, 9
    m = np.zeros((h, w), np.uint8)
    m[3, 4] = 1  # interior pixel: itself (differs from all three), north (south test), west (east test), north-west (south-east)
    assert _set(bc.boundary_map(m)) == {(3, 4), (2, 4), (3, 3), (2, 3)}
    m = np.zeros((h, w), np.uint8)
    m[h - 1, w - 1] = 1  # bottom-right corner: it has no neighbour to test, its west / north / north-west neighbours see it
    assert _set(bc.boundary_map(m)) == {(h - 1, w - 2), (h - 2, w - 1), (h - 2, w - 2)}
    assert not bc.boundary_map(np.ones((h, w), np.uint8)).any()
    assert not bc.boundary_map(np.zeros((h, w), np.uint8)).any()
    assert not bc.boundary_map(np.ones((1, 1), np.uint8)).any()
    row = np.zeros((h, w), np.uint8)
    row[h - 1] = 1  # the last row tests east only: a full last row is seen from the row above alone
    assert _set(bc.boundary_map(row)) == {(h - 2, x) for x in range(w)}


def test_f_hand_vectors():
    h, w = 23, 37
    ones, zeros = np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)
    pixel = zeros.copy()
    pixel[10, 20] = 1
    r = bc.radius(h, w)
    assert r == 1
    assert bc.f_from_counts(bc.boundary_counts(ones, ones, r)) == 1.0
    np.testing.assert_array_equal(bc.boundary_counts(ones, pixel, r), [0, 4, 0, 0])
    assert bc.f_from_counts(bc.boundary_counts(ones, pixel, r)) == 0.0
    assert bc.f_from_counts(bc.boundary_counts(pixel, ones, r)) == 0.0
    assert bc.f_from_counts(bc.boundary_counts(zeros, zeros, r)) == 1.0
    assert bc.f_from_counts(bc.boundary_counts(pixel, pixel, r)) == 1.0
    # two pixels 3 apart: their 2x2 boundaries are 2 columns apart; radius 1 matches nothing, radius 2 everything
    other = zeros.copy()
    other[10, 23] = 1
    np.testing.assert_array_equal(bc.boundary_counts(pixel, other, 1), [4, 4, 0, 0])
    np.testing.assert_array_equal(bc.boundary_counts(pixel, other, 2), [4, 4, 2, 2])
    np.testing.assert_array_equal(bc.boundary_counts(pixel, other, 3), [4, 4, 4, 4])


def test_disk_dilate():
    b = np.zeros((9, 11), bool)
    b[4, 5] = True
    for r in (0, 1, 2, 3):
        d = bc.disk_dilate(b, r)
        yy, xx = np.mgrid[0:9, 0:11]
        np.testing.assert_array_equal(d, (yy - 4) ** 2 + (xx - 5) ** 2 <= r * r)
    assert bc.disk(1).sum() == 5 and bc.disk(2).sum() == 13 and bc.disk(0).sum() == 1
    corner = np.zeros((3, 4), bool)
    corner[0, 0] = True  # nothing wraps round, a radius larger than the frame covers it
    np.testing.assert_array_equal(bc.disk_dilate(corner, 1), [[1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]])
    assert bc.disk_dilate(corner, 9).all()
    rng = np.random.default_rng(5)
    for h, w, r in [(23, 37, 1), (23, 37, 5), (40, 17, 9), (5, 3, 9), (1, 30, 2), (30, 1, 3)]:
        b = rng.random((h, w)) < 0.03
        np.testing.assert_array_equal(bc.disk_dilate_rows(b, r), bc.disk_dilate(b, r))


def test_disk_dilate_matches_cv2_and_skimage():
    cv2 = pytest.importorskip("cv2")
    morphology = pytest.importorskip("skimage.morphology")
    rng = np.random.default_rng(6)
    for h, w, r in [(23, 37, 1), (40, 33, 3), (50, 60, 9)]:
        b = (rng.random((h, w)) < 0.03).astype(np.uint8)
        want = cv2.dilate(b, morphology.disk(r).astype(np.uint8))
        np.testing.assert_array_equal(bc.disk_dilate(b, r), want != 0)


def test_boundary_radius():
    for (h, w), r in {(540, 960): 9, (720, 1280): 12, (1080, 1920): 18, (23, 37): 1}.items():
        assert seg_utils.boundary_radius(h, w) == r == bc.radius(h, w)
        assert isinstance(seg_utils.boundary_radius(h, w), int)
    assert seg_utils.boundary_radius(540, 960, 3) == 3
    assert seg_utils.boundary_radius(540, 960, bound_th=0.02) == 23  # ceil(22.03)
    assert seg_utils.boundary_radius(3, 4, 0.2) == 1  # 0.2 * 5 is 1.0 in float64: the ceiling stays


def test_F_boundary_from_counts():
    import torch
    special = {(0, 5, 0, 0): 0.0, (5, 0, 0, 0): 0.0, (0, 0, 0, 0): 1.0, (4, 8, 4, 8): 1.0, (4, 8, 0, 0): 0.0}
    for c, want in special.items():
        assert seg_utils.F_boundary_from_counts(torch.tensor([c])) == want == bc.f_from_counts(c)
    rng = np.random.default_rng(8)
    n = rng.integers(0, 40, size=(50, 2))
    table = np.concatenate([n, rng.integers(0, 41, size=(50, 2)) % (n + 1)], 1).astype(np.int64)  # matches <= boundary sizes
    table[:4] = list(special)[:4]
    got = seg_utils.F_boundary_from_counts(torch.from_numpy(table))
    assert got == np.mean([bc.f_from_counts(c) for c in table])
    p, r = 3 / 7, 2 / 9
    assert seg_utils.F_boundary_from_counts(torch.tensor([[7, 9, 3, 2]])) == 2 * p * r / (p + r)
    fg, gt = mc.blob_masklet(5, 23, 37, 3), mc.blob_masklet(5, 23, 37, 4)
    counts = np.stack([bc.boundary_counts(a, b, 1) for a, b in zip(fg, gt)])
    assert float(seg_utils.F_boundary_from_counts(torch.from_numpy(counts))) == bc.masklet_f(fg, gt)


def test_boundary_counts_argument_errors_without_gpu():
    L = _lib.lib()
    h, w = 23, 37
    stride = L.sola_jf_plane_words(h, w)
    buf = (ctypes.c_uint32 * (stride + 8))()
    base = ctypes.addressof(buf)
    bits = base + (-base) % 16
    lists = (ctypes.c_int32 * 4)()
    counts = (ctypes.c_int64 * 4)()
    good = dict(bits=bits, stride=stride, radius=1, counts=ctypes.addressof(counts))

    def call(**kw):
        a = dict(good, **kw)
        p = ctypes.addressof(lists)
        return L.sola_mask_select_boundary_counts(a["bits"], a["stride"], 1, 1, h, w, a["radius"], p, p, p, p, 1, a["counts"], None, 0, None)

    assert call(radius=65) == -1 and b"radius 65" in L.sola_last_error()
    assert call(radius=-1) == -1 and b"radius" in L.sola_last_error()
    assert call(counts=None) == -1 and b"null" in L.sola_last_error()
    assert call(bits=bits + 4) == -1 and b"16-byte aligned" in L.sola_last_error()
    assert call(stride=stride - 4) == -1 and b"words_stride" in L.sola_last_error()
    assert call(stride=stride + 1) == -1 and b"words_stride" in L.sola_last_error()
    assert L.sola_boundary_counts_workspace_bytes(1080, 1920, 18, 16, 100) == 0
