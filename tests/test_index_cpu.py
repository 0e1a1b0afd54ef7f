"""Index maps -> bit planes without a GPU: the symbols, the argument checks of sola_index_hist / sola_index_pack (refused before
any launch), the numpy restatement of tests/index_cases.py against hand-written cases, the object-id rules, and the Ref-DAVIS
annotation reader of TrackDataset."""
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

import index_cases as ic  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402
from sola_amd import data as sdata  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402


def test_symbols_are_declared_and_loadable():
    L = _lib.lib()
    for name in ("sola_index_hist", "sola_index_pack"):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert name in open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert seg_utils.INDEX_ID_CHUNK == ic.ID_CHUNK
    assert f"#define SOLA_INDEX_ID_CHUNK {ic.ID_CHUNK}\n" in open(os.path.join(ROOT, "include", "sola_hip.h")).read()


def _err():
    return _lib.lib().sola_last_error().decode()


def _pack(idx=0x1000, T=2, h=5, w=7, ids=0x2000, K=3, first=None, layout=1, stride=None, bits=0x4000, area=None):
    if stride is None:
        stride = ic.cm_words(h, w) if layout == 1 else ic.rm_words(h, w)
    return _lib.lib().sola_index_pack(idx, T, h, w, ids, K, first, layout, stride, bits, area, None)


def test_index_pack_argument_errors_without_gpu():
    assert _pack(layout=2) == -1 and "layout 2" in _err()
    assert _pack(layout=-1) == -1 and "layout -1" in _err()
    for kw in ({"T": -1}, {"h": -1}, {"w": -2}, {"K": -1}):
        assert _pack(**kw) == -1 and "negative size" in _err()
    assert _pack(stride=ic.cm_words(5, 7) - 4) == -1 and "words_stride 0 must be a multiple of 4 and >= 4" in _err()
    assert _pack(h=37, w=61, stride=ic.cm_words(37, 61) + 2) == -1 and "multiple of 4" in _err()
    assert _pack(layout=0, stride=ic.rm_words(5, 7) - 1) == -1 and "words_stride 1 must be >= 2" in _err()
    assert _pack(bits=0x4004) == -1 and "16-byte aligned" in _err()
    assert _pack(layout=0, bits=0x4002) == -1 and "4-byte aligned" in _err()
    assert _pack(area=0x8004, layout=0) == -1 and "area must be 8-byte aligned" in _err()
    assert _pack(h=1 << 16, w=1 << 15, layout=0) == -1 and "h*w = 2147483648 >= 2^31" in _err()
    assert _pack(h=16385, w=1) == -1 and "at most 16384 rows" in _err()
    assert _pack(bits=None) == -1 and "null bits" in _err()
    assert _pack(ids=None) == -1 and "null ids" in _err()
    assert _pack(idx=None) == -1 and "null idx" in _err()
    # nothing to do: no pointer is looked at
    assert _pack(T=0, idx=None, bits=None, ids=None) == 0
    assert _pack(K=0, idx=None, bits=None, ids=None) == 0
    assert _pack(T=0, layout=3) == -1  # but the arguments are still checked


def test_index_hist_argument_errors_without_gpu():
    L = _lib.lib()
    assert L.sola_index_hist(0x1000, -1, 4, 4, 0x2000, None) == -1 and "negative size" in _err()
    assert L.sola_index_hist(0x1000, 1, 4, -4, 0x2000, None) == -1 and "negative size" in _err()
    assert L.sola_index_hist(0x1000, 1, 1 << 16, 1 << 15, 0x2000, None) == -1 and ">= 2^31" in _err()
    assert L.sola_index_hist(0x1000, 1, 4, 4, None, None) == -1 and "null counts" in _err()
    assert L.sola_index_hist(0x1000, 1, 4, 4, 0x2004, None) == -1 and "8-byte aligned" in _err()
    assert L.sola_index_hist(None, 1, 4, 4, 0x2000, None) == -1 and "null idx" in _err()
    assert L.sola_index_hist(None, 0, 4, 4, None, None) == 0


def test_restatement_on_a_hand_written_3x5_case():
    m = np.array([[[1, 0, 2, 2, 0],
                   [1, 1, 0, 2, 255],
                   [0, 1, 0, 0, 255]]], np.uint8)
    # row-major: pixel p = y*5 + x; object 1 at p = 0, 5, 6, 11; object 2 at 2, 3, 8; 255 at 9, 14
    rm = ic.rm_planes(m, [1, 2, 255, 7])
    assert rm.shape == (4, 1) and rm.dtype == np.uint32
    assert rm[:, 0].tolist() == [1 | 1 << 5 | 1 << 6 | 1 << 11, 1 << 2 | 1 << 3 | 1 << 8, 1 << 9 | 1 << 14, 0]
    # column-major: position = x*3 + y; object 1 at (0,0) (1,0) (1,1) (2,1) -> 0, 1, 4, 5; object 2 at (0,2) (0,3) (1,3) -> 6, 9, 10
    cm = ic.cm_planes(m, [1, 2, 255, 7])
    assert cm.shape == (4, 4) and not cm[:, 1:].any()
    assert cm[:, 0].tolist() == [1 | 1 << 1 | 1 << 4 | 1 << 5, 1 << 6 | 1 << 9 | 1 << 10, 1 << 13 | 1 << 14, 0]
    assert ic.hist(m)[0, [0, 1, 2, 255, 7]].tolist() == [6, 4, 3, 2, 0] and ic.hist(m).sum() == 15


def test_restatement_on_a_hand_written_33x2_case():
    m = np.zeros((2, 33, 2), np.uint8)
    m[0, 32, 0] = 4   # raster pixel 64, column-major position 32
    m[0, 0, 1] = 4    # raster pixel 1, column-major position 33: word 1 of the column-major plane spans both columns
    m[1, 31, 1] = 4   # raster pixel 63, column-major position 64
    rm, cm = ic.rm_planes(m, [4]), ic.cm_planes(m, [4])
    assert rm.shape == (2, 3) and cm.shape == (2, 4)
    assert rm.tolist() == [[1 << 1, 0, 1], [0, 1 << 31, 0]]
    assert cm.tolist() == [[0, 1 | 1 << 1, 0, 0], [0, 0, 1, 0]]
    wide = ic.cm_planes(m, [4], stride=8)
    assert wide.shape == (2, 8) and np.array_equal(wide[:, :4], cm) and not wide[:, 4:].any()


def test_restatement_follows_pack_masks_documented_bit_order():
    # include/sola_hip.h: "words of 32 pixels, row-major over the H*W comparison grid"; bit j of word i is pixel 32*i + j
    maps = ic.random_maps(2, 7, 13, 0, values=[0, 3])
    planes = ic.rm_planes(maps, [3])
    for t in range(2):
        for p in np.flatnonzero(maps[t].reshape(-1) == 3):
            assert planes[t, p // 32] >> (p % 32) & 1
        assert sum(bin(int(x)).count("1") for x in planes[t]) == int((maps[t] == 3).sum())
    assert _lib.lib().sola_mask_words(7, 13) == ic.rm_words(7, 13) and _lib.lib().sola_jf_plane_words(7, 13) == ic.cm_words(7, 13)
    assert _lib.lib().sola_jf_plane_words(37, 61) == ic.cm_words(37, 61)


def test_object_id_rules_on_a_host_histogram():
    maps = np.zeros((3, 4, 4), np.uint8)
    maps[0, 0, :] = [0, 2, 255, 9]
    maps[1, 0, :] = [5, 5, 0, 254]
    maps[2, 1, 1] = 255
    h = ic.hist(maps)
    assert seg_utils.object_ids_from_hist(h, "davis") == [2, 9] == ic.object_ids(maps, "davis")
    assert seg_utils.object_ids_from_hist(h, "ytbvos") == [2, 5, 9, 254, 255] == ic.object_ids(maps, "ytbvos")
    assert seg_utils.object_ids_from_hist(torch.from_numpy(h), "ytbvos") == [2, 5, 9, 254, 255]
    assert seg_utils.object_ids_from_hist(np.zeros((0, 256), np.int64), "davis") == []
    with pytest.raises(ValueError):
        seg_utils.object_ids_from_hist(h, "coco")
    with pytest.raises(ValueError):
        seg_utils.object_ids_from_hist(h[:, :255], "davis")


def test_cpu_tensors_raise():
    maps = torch.zeros((2, 4, 4), dtype=torch.uint8)
    for call in (lambda: seg_utils.index_hist(maps), lambda: seg_utils.index_object_ids(maps, "davis"),
                 lambda: seg_utils.pack_index_masklets(maps, [1]), lambda: seg_utils.pack_index_masklets(maps, [1], "cm"),
                 lambda: seg_utils.index_masklets(maps), lambda: seg_utils.IndexMasklet(maps, 1)):
        with pytest.raises(SolaError, match="GPU only"):
            call()


def test_has_mask_gt_and_skip_reason(tmp_path):
    import eval as ev
    data_root, track_root, split = ic.make_davis_tree(str(tmp_path / "with"))
    ds = sdata.TrackDataset(split, data_root, track_root)
    assert ds.has_mask_gt
    assert ev.jf_skip_reason({}, ds) is None
    data_root, track_root, split = ic.make_davis_tree(str(tmp_path / "without"), with_annotations=False)
    bare = sdata.TrackDataset(split, data_root, track_root)
    assert not bare.has_mask_gt
    reason = ev.jf_skip_reason({}, bare)
    assert reason and "DAVIS" not in reason and "no mask ground truth" in reason
    with pytest.raises(ValueError):
        bare.gt_index_maps("bear")
    assert ev.jf_skip_reason({"jf": False}, ds) == "--jf false"


@pytest.mark.parametrize("mode", ["P", "L"])
def test_gt_index_maps_reads_palette_and_greyscale_frames(tmp_path, mode):
    from PIL import Image
    data_root, track_root, split = ic.make_davis_tree(str(tmp_path), mode=mode)
    ds = sdata.TrackDataset(split, data_root, track_root)
    adir = os.path.join(data_root, "ref-davis", "valid", "Annotations", "bear")
    assert Image.open(os.path.join(adir, "00000.png")).mode == mode
    maps = ds.gt_index_maps("bear")
    assert maps.dtype == np.uint8 and maps.shape == (ic.T, ic.H, ic.W)
    assert np.array_equal(maps, ic.annotation("bear"))  # sorted file names = frame order; indices, not colours
    assert ds.gt_index_maps("bear") is maps  # the last video is kept
    other = ds.gt_index_maps("camel")
    assert np.array_equal(other, ic.annotation("camel")) and ds.gt_index_maps("camel") is other
    again = ds.gt_index_maps("bear")
    assert again is not maps and np.array_equal(again, maps)


def test_gt_index_maps_refuses_colour_files_and_mixed_sizes(tmp_path):
    from PIL import Image
    data_root, track_root, split = ic.make_davis_tree(str(tmp_path))
    ds = sdata.TrackDataset(split, data_root, track_root)
    adir = os.path.join(data_root, "ref-davis", "valid", "Annotations")
    Image.fromarray(np.zeros((ic.H, ic.W, 3), np.uint8)).save(os.path.join(adir, "bear", "00002.png"))
    with pytest.raises(ValueError, match="00002.png.*RGB"):
        ds.gt_index_maps("bear")
    Image.fromarray(np.zeros((ic.H + 1, ic.W), np.uint8)).save(os.path.join(adir, "camel", "00003.png"))
    with pytest.raises(ValueError, match="00003.png.*frame size"):
        ds.gt_index_maps("camel")


def test_gt_masklets_is_gt_rles_for_mevis(tmp_path):
    import jf_cases as jc
    data_root, track_root, split = jc.make_tree(str(tmp_path))
    ds = sdata.TrackDataset(split, data_root, track_root)
    assert ds.gt_masklets("vidA", "1", "cpu") == ds.gt_rles("vidA", "1")
    assert ds.gt_masklets("vidA", "1", "cpu")[0] is ds.gt_rles("vidA", "1")[0]
