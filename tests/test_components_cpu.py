"""Connected components without a GPU: the restatement of the contract (components_cases.py) pinned against hand-written
arrays and scipy.ndimage.label before test_gpu_components.py uses it as the yardstick; the declared symbols; scratch sizes
and the argument checks that refuse before any launch; the Python entry points' own checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import components_cases as cc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused (or is a no-op) before it launches anything
SYMBOLS = ["sola_mask_components_scratch_bytes", "sola_mask_components", "sola_mask_fill_small"]


def test_label_hand_written_frame_both_connectivities():
    m = np.array([[1, 0, 0, 1, 1],
                  [0, 1, 0, 0, 1],
                  [0, 0, 0, 1, 0],
                  [1, 1, 0, 0, 0]], np.uint8)
    lab8, area8 = cc.label(m, 8)
    np.testing.assert_array_equal(lab8, [[1, 0, 0, 4, 4],
                                         [0, 1, 0, 0, 4],
                                         [0, 0, 0, 4, 0],
                                         [16, 16, 0, 0, 0]])
    np.testing.assert_array_equal(area8, [[2, 0, 0, 4, 4],
                                          [0, 2, 0, 0, 4],
                                          [0, 0, 0, 4, 0],
                                          [2, 2, 0, 0, 0]])
    lab4, area4 = cc.label(m, 4)
    np.testing.assert_array_equal(lab4, [[1, 0, 0, 4, 4],
                                         [0, 7, 0, 0, 4],
                                         [0, 0, 0, 14, 0],
                                         [16, 16, 0, 0, 0]])
    np.testing.assert_array_equal(area4, [[1, 0, 0, 3, 3],
                                          [0, 1, 0, 0, 3],
                                          [0, 0, 0, 1, 0],
                                          [2, 2, 0, 0, 0]])
    assert lab8.dtype == np.int32 and area8.dtype == np.int32


def test_label_u_shape_takes_the_first_pixel_in_raster_order():
    # the two arms meet only in the last row: the label is the left arm's first pixel, whichever arm a scan meets first
    m = np.array([[0, 1, 0, 1],
                  [1, 1, 0, 1],
                  [0, 1, 1, 1]], np.uint8)
    lab, area = cc.label(m, 4)
    np.testing.assert_array_equal(lab, m * 2)
    np.testing.assert_array_equal(area, m * 8)


def test_label_checkerboard():
    m = cc.frames(6, 7)[6][1]
    assert cc.frames(6, 7)[6][0] == "checkerboard"
    lab8, area8 = cc.label(m, 8)
    assert set(np.unique(lab8)) == {0, 2} and set(np.unique(area8)) == {0, int(m.sum())}
    lab4, area4 = cc.label(m, 4)
    np.testing.assert_array_equal(lab4, np.where(m != 0, np.arange(42).reshape(6, 7) + 1, 0))
    np.testing.assert_array_equal(area4, m)


def test_fill_holes_hand_written_scores():
    nan = np.float32(np.nan)
    s = np.array([[1, 1, 1, 1, 1, 1, -1],
                  [1, -2, 0, 1, 1, 1, 1],
                  [1, 1, 1, -0.0, 1, 1, 1],
                  [-3, 1, nan, 1, 1, -1, -1],
                  [-3, 1, 1, 1, 1, -1, -1]], np.float32)
    # 8-connectivity: {-2, 0, -0.0} is one hole of 3; the corner pixel a hole of 1 (the border does not exempt it); the left
    # pair a hole of 2; the 2x2 block a hole of 4; the NaN is neither background nor filled
    want3 = s.copy()
    for y, x in ((1, 1), (1, 2), (2, 3), (0, 6), (3, 0), (4, 0)):
        want3[y, x] = np.float32(0.1)
    got3 = cc.fill_holes(s, 3)
    np.testing.assert_array_equal(got3.view(np.int32), want3.view(np.int32))
    want1 = s.copy()
    want1[0, 6] = np.float32(0.1)
    np.testing.assert_array_equal(cc.fill_holes(s, 1).view(np.int32), want1.view(np.int32))
    # 4-connectivity: -0.0 at (2,3) is its own hole of 1
    want1[2, 3] = np.float32(0.1)
    np.testing.assert_array_equal(cc.fill_holes(s, 1, connectivity=4).view(np.int32), want1.view(np.int32))
    got4 = cc.fill_holes(s, 4, fill_value=0.5)
    assert np.all(got4[3:, 5:] == np.float32(0.5)) and np.isnan(got4[3, 2]) and got4[0, 0] == 1


def test_remove_small_hand_written_mask():
    m = np.array([[1, 0, 0, 0, 0, 0],
                  [0, 0, 1, 1, 1, 0],
                  [0, 0, 1, 0, 1, 0],
                  [0, 0, 1, 1, 1, 0]], np.uint8)
    isl = cc.remove_small(m, 1, "islands")
    want = m.copy()
    want[0, 0] = 0
    np.testing.assert_array_equal(isl, want)
    holes = cc.remove_small(m, 1, "holes")
    want = m.copy()
    want[2, 3] = 1
    np.testing.assert_array_equal(holes, want)
    np.testing.assert_array_equal(cc.remove_small(m, 8, "islands"), np.zeros_like(m))
    np.testing.assert_array_equal(cc.remove_small(m, 0, "holes"), m)


def test_rings_hold_holes_of_max_area_and_one_more():
    m = cc.rings(17, 33)
    _, areas = cc.label(m == 0, 4)
    inner = sorted(set(np.unique(areas)) - {0, int(areas.max())})
    assert inner == [cc.MAX_AREA, cc.MAX_AREA + 1]
    filled = cc.remove_small(m, cc.MAX_AREA, "holes")
    assert int(filled.sum()) - int(m.sum()) == cc.MAX_AREA


def _renumbered(lab):
    """labels -> numbered 1.. in raster order of first appearance (what scipy returns)."""
    flat = lab.ravel()
    vals, first = np.unique(flat[flat > 0], return_index=True)
    order = np.argsort(first)
    table = np.zeros(int(flat.max()) + 1, np.int64)
    table[vals[order]] = np.arange(1, len(vals) + 1)
    return table[lab]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h,w", [(1, 70), (17, 33), (65, 129)])
def test_label_equals_scipy_after_renumbering(h, w, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for name, m in cc.frames(h, w):
        lab, areas = cc.label(m, connectivity)
        ref, n = ndimage.label(m, structure=structure)
        np.testing.assert_array_equal(_renumbered(lab), ref, err_msg=name)
        sizes = np.bincount(ref.ravel(), minlength=n + 1)
        sizes[0] = 0
        np.testing.assert_array_equal(areas, sizes[ref], err_msg=name)
        # the label is the first pixel of its component
        vals, first = np.unique(lab.ravel(), return_index=True)
        np.testing.assert_array_equal(first[vals > 0], vals[vals > 0] - 1, err_msg=name)


def test_big_serpentine_is_one_component():
    h, w = cc.BIG
    for vertical in (False, True):
        m = cc.serpentine(h, w, vertical)
        lab, areas = cc.label(m, 4)
        assert set(np.unique(lab)) == {0, 1} and set(np.unique(areas)) == {0, int(m.sum())}


def test_tile_corner_frames_follow_the_library_tile():
    from sola_amd import seg_utils
    assert tuple(seg_utils.CC_TILE) == cc.TILE
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert int(re.search(r"#define SOLA_CC_TILE_H (\d+)", header).group(1)) == cc.TILE[0]
    assert int(re.search(r"#define SOLA_CC_TILE_W (\d+)", header).group(1)) == cc.TILE[1]
    m = cc.tile_corner_pairs(65, 129)
    assert int(m.sum()) == 2 * 4 * 2 and m[15, 63] == 1 and m[16, 64] == 1
    lab8, _ = cc.label(m, 8)
    lab4, _ = cc.label(m, 4)
    assert len(np.unique(lab8)) == 1 + 8 and len(np.unique(lab4)) == 1 + 16


def test_symbols_are_declared_and_in_the_header():
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
    assert _lib.SIGNATURES["sola_mask_components_scratch_bytes"][0] is ctypes.c_size_t


def test_scratch_bytes_and_refusals_before_any_launch():
    L = _lib.lib()
    assert L.sola_mask_components_scratch_bytes(2, 3, 5) == 256
    assert L.sola_mask_components_scratch_bytes(100, 1080, 1920) == 100 * 1080 * 1920 * 8
    for n, h, w in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 11, 1 << 10, 1 << 10)):
        assert L.sola_mask_components_scratch_bytes(n, h, w) == 0
    big = 1 << 40
    # any empty dimension: a successful no-op, nothing is read
    for n, h, w in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert L.sola_mask_components(None, 0, n, h, w, 8, None, None, None, 0, None) == 0
        assert L.sola_mask_fill_small(None, 3, n, h, w, 8, 8, 0.1, None, None, 0, None) == 0
    for conn in (0, 6, 9, -4):
        assert L.sola_mask_components(FAKE, 0, 1, 4, 4, conn, FAKE, FAKE, FAKE, big, None) == -1
        assert b"connectivity" in L.sola_last_error()
        assert L.sola_mask_fill_small(FAKE, 3, 1, 4, 4, conn, 8, 0.1, FAKE, FAKE, big, None) == -1
    assert L.sola_mask_fill_small(FAKE, 3, 1, 4, 4, 8, -1, 0.1, FAKE, FAKE, big, None) == -1
    assert b"max_area" in L.sola_last_error()
    need = L.sola_mask_components_scratch_bytes(1, 4, 4)
    assert L.sola_mask_components(FAKE, 0, 1, 4, 4, 8, FAKE, FAKE, FAKE, need - 1, None) == -1
    assert b"scratch" in L.sola_last_error()
    assert L.sola_mask_fill_small(FAKE, 3, 1, 4, 4, 8, 8, 0.1, FAKE, FAKE, need - 1, None) == -1
    assert L.sola_mask_components(FAKE, 0, 1 << 11, 1 << 10, 1 << 10, 8, FAKE, FAKE, FAKE, big, None) == -1
    assert b"2^31" in L.sola_last_error()
    assert L.sola_mask_components(FAKE, 6, 1, 4, 4, 8, FAKE, FAKE, FAKE, big, None) == -1
    assert L.sola_mask_components(FAKE, 0, 1, 4, 4, 8, None, FAKE, FAKE, big, None) == -1


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    from sola_amd import seg_utils as su
    s = torch.zeros(1, 1, 4, 4)
    with pytest.raises(SolaError, match="GPU only"):
        su.connected_components(s.to(torch.uint8))
    with pytest.raises(SolaError, match="GPU only"):
        su.fill_holes_in_mask_scores(s, 8)
    with pytest.raises(SolaError, match="GPU only"):
        su.remove_small_regions(s, 8, "holes")
    for bad in (0, -3):
        with pytest.raises(SolaError, match="max_area"):
            su.fill_holes_in_mask_scores(s, bad)
    with pytest.raises(SolaError, match="float32"):
        su.fill_holes_in_mask_scores(s.to(torch.uint8), 8)
    with pytest.raises(SolaError, match="mode"):
        su.remove_small_regions(s, 8, "both")
    with pytest.raises(SolaError, match=r"\(N,1,H,W\)"):
        su.connected_components(torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
