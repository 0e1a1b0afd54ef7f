"""Host side of the mask-level J&F path (no GPU): the batch RLE string parser, the dataset's track / GT masklet lists
and the mask-GT switch."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import jf_cases as jc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import SolaError, _lib, data as sdata, seg_utils  # noqa: E402


def test_batch_string_parser_matches_the_oracle():
    rng = np.random.default_rng(3)
    masks = list(mc.blob_masklet(8, 23, 37, 5)) + [np.zeros((23, 37), np.uint8), np.ones((23, 37), np.uint8),
                                                  (rng.random((23, 37)) < 0.5).astype(np.uint8)]
    strings = [mo.rle_counts_to_string(mo.mask_to_counts(m)) for m in masks]
    strings.insert(3, "")  # no runs
    cum, off = seg_utils.rle_strings_to_cum(strings, 23 * 37)
    assert off[0] == 0 and off[-1] == len(cum) and len(off) == len(strings) + 1
    for i, s in enumerate(strings):
        want = np.cumsum(np.asarray(mo.rle_string_to_counts(s), np.int64)).astype(np.uint32)
        np.testing.assert_array_equal(cum[off[i]:off[i + 1]], want)
    assert off[4] == off[3]


def test_batch_string_parser_rejects_what_the_single_parser_rejects():
    good = mo.rle_counts_to_string([3, 4, 5])
    with pytest.raises(SolaError, match="string 1.*truncated"):
        seg_utils.rle_strings_to_cum([good, "1o"])
    with pytest.raises(SolaError, match="string 0.*cover"):
        seg_utils.rle_strings_to_cum(["99"], 10)  # 18 pixels > 10
    L = _lib.lib()
    chars = np.frombuffer(b"11111" + good.encode(), np.uint8)
    str_off = np.array([0, 5, 5 + len(good)], np.int64)
    cum = np.empty(4, np.uint32)
    run_off = np.empty(3, np.int64)
    args = (chars.ctypes.data, str_off.ctypes.data, 2, cum.ctypes.data)
    assert L.sola_rle_strings_to_cum_batch(*args, 4, -1, run_off.ctypes.data) < 0  # 5 runs > 4
    assert b"more runs than the output holds" in L.sola_last_error()
    for s in (b"1o", b"11111", b"99"):  # the single-string helper rejects the same strings
        buf = np.empty(4, np.uint32)
        assert L.sola_rle_string_to_cum(s, len(s), ctypes.c_void_p(buf.ctypes.data), 4, 10) < 0
    cum = np.empty(16, np.uint32)
    assert L.sola_rle_strings_to_cum_batch(chars.ctypes.data, str_off.ctypes.data, 2, cum.ctypes.data, 16, -1, run_off.ctypes.data) == 8
    np.testing.assert_array_equal(run_off, [0, 5, 8])


def test_plane_stride_is_padded_to_16_bytes():
    L = _lib.lib()
    for h, w in [(1, 1), (1, 37), (29, 1), (23, 37), (32, 4), (720, 1280), (1080, 1920)]:
        s = L.sola_jf_plane_words(h, w)
        assert s % 4 == 0 and s >= (h * w + 31) // 32 and s - (h * w + 31) // 32 < 4


def test_track_and_gt_masklets_follow_the_sample_order(tmp_path):
    data_root, track_root, split = jc.make_tree(str(tmp_path))
    ds = sdata.TrackDataset(split, data_root, track_root)
    assert ds.has_mask_gt
    mask_dict = json.load(open(os.path.join(data_root, "mevis", "valid_u", "mask_dict.json")))
    for vid, (grid, exps) in jc.VIDEOS.items():
        for eid, (_, annos, gd) in exps.items():
            tracks = ds.track_rles(vid, eid)
            # roots in order, sorted file names: the order of __getitem__'s tokens and merged_masklet's predictions
            idx = [i for i, s in enumerate(ds.samples) if s["video_id"] == vid and s["expression_id"] == eid][0]
            assert ds[idx]["sam2_anno_id"] == sorted(grid) + sorted(gd)
            want = []
            for root, tail, ids in (("grid_tracks", (vid,), grid), ("gdino_tracks", (vid, eid), gd)):
                mdir = os.path.join(track_root, root, "mevis", "valid_u", "sam2_masklets", *tail)
                want += [json.load(open(os.path.join(mdir, f"{a:05d}.json")))["rle"] for a in sorted(ids)]
            assert tracks == want
            preds = np.array([(i * 7 + len(eid)) % 3 == 0 for i in range(len(tracks))], np.int64)
            preds[0] = 1
            np.testing.assert_array_equal(ds.merged_masklet(vid, eid, preds) != 0, mo.merge_selected(tracks, preds) != 0)
            assert ds.gt_rles(vid, eid) == [mask_dict[str(a)] for a in annos]
        # a video's grid tracks are read once and shared by its expressions
        first = ds.track_rles(vid, "0")
        for eid in exps:
            assert all(a is b for a, b in zip(ds.track_rles(vid, eid)[:len(grid)], first[:len(grid)]))


def test_no_mask_gt_without_mask_dict(tmp_path):
    data_root, track_root, split = jc.make_tree(str(tmp_path), with_mask_dict=False)
    ds = sdata.TrackDataset(split, data_root, track_root)
    assert not ds.has_mask_gt
    with pytest.raises(ValueError):
        ds.gt_rles("vidA", "0")
    # Ref-DAVIS: out of scope even with a mask_dict.json next to its metadata
    mdir = os.path.join(data_root, "ref-davis", "meta_expressions", "valid")
    os.makedirs(mdir)
    json.dump({"videos": {"v": {"frames": ["00000"], "expressions": {"0": {"exp": "x", "obj_id": "1"}}}}},
              open(os.path.join(mdir, "meta_expressions.json"), "w"))
    os.makedirs(os.path.join(data_root, "ref-davis", "valid"))
    json.dump({}, open(os.path.join(data_root, "ref-davis", "valid", "mask_dict.json"), "w"))
    dav = sdata.TrackDataset({"data_name": "ref-davis", "data_type": "valid", "sam2_output_dirs": "grid_tracks"}, data_root, track_root)
    assert not dav.has_mask_gt
