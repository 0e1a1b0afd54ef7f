"""The grid-prompt stage without a GPU: the numpy restatement of its contracts (amg_cases.py) pinned against hand-written
values and against torch on the CPU before test_gpu_amg.py uses it as the yardstick; the declared symbols; the scratch size
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

import amg_cases as ac  # noqa: E402
from oracle import masklet_oracle  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused (or is a no-op) before it launches anything
SYMBOLS = ["sola_mask_logit_stats", "sola_box_nms_scratch_bytes", "sola_box_nms", "sola_box_nms_profile"]
nan, inf = np.float32(np.nan), np.float32(np.inf)

HAND_LOGITS = np.array([[-2, -2, -2, -2, -2],
                        [-2, 0.0, -0.0, 1.0, -1.0],
                        [nan, inf, -inf, 0.5, -0.5],
                        [-2, -2, 2.0, nan, -2]], np.float32)

HAND_BOXES = np.array([[0, 0, 10, 10],      # 0
                       [0, 0, 10, 5],       # 1: IoU with 0 is exactly 0.5
                       [0, 0, 10, 4.5],     # 2: same score as 1, IoU with 1 is 0.9: the lower index wins the tie
                       [0, 4, 10, 10],      # 3: IoU with 0 is 0.6
                       [20, 20, 30, 30],    # 4
                       [20, 20, 30, 27]],   # 5: IoU with 4 is float32(7/10) = float32(0.7) exactly
                      np.float32)
HAND_SCORES = np.array([0.9, 0.8, 0.8, 0.7, 0.95, 0.1], np.float32)


def test_stats_hand_written_logit_map():
    # thr 0, thr_hi 1, thr_lo -1: values ON a threshold do not count for it, NaN and -inf never count, -0.0 is not > 0
    got = ac.stats(HAND_LOGITS[None], True, 0.0, 1.0, -1.0)
    #                      n_hi (inf, 2)  n_lo (0, -0, 1, inf, .5, -.5, 2)  area (1, inf, .5, 2)  box
    np.testing.assert_array_equal(got, [[2, 7, 4, 1, 1, 3, 3]])
    assert got.dtype == np.int64
    # the same map as a float32 MASK (!= 0): NaN and both infinities are set, both zeros are clear
    got = ac.stats(HAND_LOGITS[None], False)
    np.testing.assert_array_equal(got, [[18, 18, 18, 0, 0, 4, 3]])
    np.testing.assert_array_equal(ac.stats(np.zeros((2, 3, 4), np.uint8), False), np.zeros((2, 7), np.int64))
    one = np.zeros((1, 3, 4), np.uint8)
    one[0, 2, 3] = 7
    np.testing.assert_array_equal(ac.stats(one, False), [[1, 1, 1, 3, 2, 3, 2]])


def test_stats_equal_the_torch_expressions_of_the_contract():
    thr, off = 0.25, 0.5
    names, ms = ac.stat_masks(17, 63, seed=1)
    rng = np.random.default_rng(0)
    logit = np.where(ms != 0, 1.0, -1.0).astype(np.float32) * rng.uniform(0.01, 2.0, ms.shape).astype(np.float32) + np.float32(thr)
    logit = np.concatenate([logit, ac.threshold_logits(17, 63, thr, thr + off, thr - off)[None]])
    t = torch.from_numpy(logit)
    st = ac.stats(logit, True, thr, thr + off, thr - off)
    # sam2.utils.amg.calculate_stability_score, as a contract: counts of masks > (thr +- off), ratio in float32
    hi = (t > (thr + off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    lo = (t > (thr - off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    np.testing.assert_array_equal(st[:, 0], hi.numpy())
    np.testing.assert_array_equal(st[:, 1], lo.numpy())
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32), (hi / lo).numpy())
    # the box of a bool mask from max / min over both axes, empty masks -> zeros
    m = t > thr
    h, w = m.shape[-2:]
    in_h, _ = m.max(-1)
    hc = in_h * torch.arange(h)[None]
    bottom, _ = hc.max(-1)
    top, _ = (hc + h * (~in_h)).min(-1)
    in_w, _ = m.max(-2)
    wc = in_w * torch.arange(w)[None]
    right, _ = wc.max(-1)
    left, _ = (wc + w * (~in_w)).min(-1)
    box = torch.stack([left, top, right, bottom], -1) * (~((right < left) | (bottom < top))).unsqueeze(-1)
    np.testing.assert_array_equal(st[:, 3:], box.numpy())
    np.testing.assert_array_equal(st[:, 2], m.flatten(1).sum(1).numpy())
    assert not st[names.index("empty"), 2:].any()  # no pixel above thr: area 0, box (0, 0, 0, 0)


def test_nms_hand_boxes_tie_and_exact_threshold():
    order = ac.visiting_order(HAND_SCORES)
    np.testing.assert_array_equal(order, [4, 0, 1, 2, 3, 5])  # 1 before 2: equal scores, lower index first
    assert ac.box_iou_f32(HAND_BOXES[0], HAND_BOXES[1]) == np.float32(0.5)
    assert ac.box_iou_f32(HAND_BOXES[4], HAND_BOXES[5]) == np.float32(0.7)
    for fn in (lambda t: ac.box_nms_loop(HAND_BOXES, order, None, t), lambda t: ac.box_nms(HAND_BOXES, HAND_SCORES, None, t)):
        assert fn(0.5) == [4, 0, 1]           # 1 survives IoU == 0.5; 2 falls to 1, 3 to 0 (0.6), 5 to 4 (0.7)
        assert fn(0.7) == [4, 0, 1, 3, 5]     # 5 survives IoU == float32(0.7); 2 still falls to 1 (0.9)
    cats = np.array([0, 0, 1, 0, 0, 1], np.int64)  # 2 and 5 in a category of their own: nothing suppresses them
    assert ac.box_nms_loop(HAND_BOXES, order, cats, 0.5) == [4, 0, 1, 2, 5]
    assert ac.box_nms(HAND_BOXES, HAND_SCORES, cats, 0.5) == [4, 0, 1, 2, 5]
    # identical one-pixel (zero-area) boxes: 0/0 is NaN and does not suppress
    dots = np.array([[5, 5, 5, 5], [5, 5, 5, 5]], np.float32)
    assert ac.box_nms_loop(dots, np.array([0, 1]), None, 0.5) == [0, 1]
    assert ac.box_nms(dots, np.array([1.0, 1.0], np.float32), None, 0.5) == [0, 1]


@pytest.mark.parametrize("n,k", [(65, 1), (130, 3)])
def test_nms_array_form_equals_the_scalar_double_loop(n, k):
    for boxes in (ac.rect_boxes(n, n), ac.float_boxes(n, n)):
        scores = ac.tied_scores(n, n)
        idxs = None if k == 1 else ac.categories(n, k, n)
        for thr in (0.5, 0.7):
            want = ac.box_nms_loop(boxes, ac.visiting_order(scores), idxs, thr)
            assert ac.box_nms(boxes, scores, idxs, thr) == want
            assert 0 < len(want) < n


def test_part_filter_hand_masks_with_duplicate_and_empty():
    m = np.zeros((5, 4, 6), np.uint8)
    m[0, :, 0:4] = 1      # 16 pixels
    m[1] = m[0]           # its duplicate
    m[2, 0:2, 0:3] = 1    # 6 pixels, all inside 0
    m[3, 3, 3:6] = 1      # 3 pixels, one inside 0
    #                     4: empty, part-ness 0/0 = nan
    np.testing.assert_array_equal(ac.filter_part(m), [False, True, True, False, False])
    np.testing.assert_array_equal(ac.filter_part(m[:1]), [False])
    # the last mask is never `full`: a pair of duplicates marks only the second
    np.testing.assert_array_equal(ac.filter_part(m[:2]), [False, True])
    # exactly 7/10 is not a part at 0.7, and is one at 0.69
    pair = np.zeros((2, 4, 12), np.uint8)
    pair[0, :, 0:7] = 1
    pair[1, 0, 0:10] = 1
    np.testing.assert_array_equal(ac.filter_part(pair, 0.7), [False, False])
    np.testing.assert_array_equal(ac.filter_part(pair, 0.69), [False, True])


def test_part_filter_equals_the_literal_loop_over_the_oracle():
    for n in (2, 9, 40):
        masks = ac.part_masks(n, 45, 80, n)
        areas = masks.reshape(n, -1).sum(1, dtype=np.int64)
        assert np.all(np.diff(areas) <= 0)
        t = torch.from_numpy(masks).float()
        is_part = torch.tensor([False] * n)
        for idx in range(n - 1):
            if is_part[idx]:
                continue
            P = torch.from_numpy(masklet_oracle.compute_P(t.numpy(), t[idx].numpy()))
            is_part[P > 0.7] = True
            is_part[idx] = False
        np.testing.assert_array_equal(ac.filter_part(masks), is_part.numpy())
    assert ac.filter_part(ac.part_masks(40, 45, 80, 40)).sum() > 3


def test_rle_uncompressed_hand_masks_and_the_oracle():
    m = np.array([[0, 1, 1],
                  [0, 1, 0]], np.uint8)
    assert ac.rle_uncompressed(m) == {"size": [2, 3], "counts": [2, 3, 1]}
    assert ac.rle_uncompressed(np.ones((2, 3))) == {"size": [2, 3], "counts": [0, 6]}
    assert ac.rle_uncompressed(np.zeros((2, 3))) == {"size": [2, 3], "counts": [6]}
    for name, f in zip(*ac.stat_masks(17, 33)):
        assert ac.rle_uncompressed(f)["counts"] == masklet_oracle.mask_to_counts(f), name


def test_symbols_are_declared_and_in_the_header():
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
    assert _lib.SIGNATURES["sola_box_nms_scratch_bytes"][0] is ctypes.c_size_t
    from sola_amd import seg_utils
    assert int(re.search(r"#define SOLA_BOX_NMS_MAX_N (\d+)", header).group(1)) == seg_utils.NMS_MAX_BOXES >= 16384


def test_scratch_bytes_refusals_and_no_ops_before_any_launch():
    L = _lib.lib()
    from sola_amd.seg_utils import NMS_MAX_BOXES
    assert L.sola_box_nms_scratch_bytes(1) == 256
    assert L.sola_box_nms_scratch_bytes(64) == 512
    assert L.sola_box_nms_scratch_bytes(65) == 65 * 2 * 8 + 240
    assert L.sola_box_nms_scratch_bytes(3072) == 3072 * 48 * 8
    assert L.sola_box_nms_scratch_bytes(NMS_MAX_BOXES) == NMS_MAX_BOXES * (NMS_MAX_BOXES // 64) * 8
    for n in (0, -1, NMS_MAX_BOXES + 1):
        assert L.sola_box_nms_scratch_bytes(n) == 0
    big = 1 << 40
    # statistics: refused before anything is touched
    for n, h, w in ((-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert L.sola_mask_logit_stats(FAKE, 2, n, h, w, 0.0, 1.0, -1.0, FAKE, None) == -1
        assert b"negative" in L.sola_last_error()
    for et in (-1, 3, 5):
        assert L.sola_mask_logit_stats(FAKE, et, 1, 4, 4, 0.0, 1.0, -1.0, FAKE, None) == -1
        assert b"elem_type" in L.sola_last_error()
    assert L.sola_mask_logit_stats(FAKE, 2, 1, 1 << 16, 1 << 15, 0.0, 1.0, -1.0, FAKE, None) == -1
    assert b"2^31" in L.sola_last_error()
    assert L.sola_mask_logit_stats(FAKE, 0, (1 << 31) - 1, 1 << 15, 1 << 15, 0.0, 1.0, -1.0, FAKE, None) == -1
    assert b"pieces" in L.sola_last_error()
    assert L.sola_mask_logit_stats(ctypes.c_void_p((1 << 20) + 2), 2, 1, 4, 4, 0.0, 1.0, -1.0, FAKE, None) == -1
    assert b"aligned" in L.sola_last_error()
    assert L.sola_mask_logit_stats(FAKE, 2, 1, 4, 4, 0.0, 1.0, -1.0, None, None) == -1
    # n == 0: a successful no-op, nothing is read or written
    for h, w in ((4, 4), (0, 4), (4, 0), (1 << 16, 1 << 16)):
        assert L.sola_mask_logit_stats(None, 2, 0, h, w, 0.0, 1.0, -1.0, None, None) == 0
    # NMS
    assert L.sola_box_nms(FAKE, FAKE, None, -1, 0.5, FAKE, FAKE, FAKE, big, None) == -1
    assert b"negative" in L.sola_last_error()
    assert L.sola_box_nms(FAKE, FAKE, None, NMS_MAX_BOXES + 1, 0.5, FAKE, FAKE, FAKE, big, None) == -1
    assert b"at most" in L.sola_last_error()
    need = L.sola_box_nms_scratch_bytes(100)
    assert L.sola_box_nms(FAKE, FAKE, None, 100, 0.5, FAKE, FAKE, FAKE, need - 1, None) == -1
    assert b"scratch" in L.sola_last_error()
    for args in ((None, FAKE, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE, FAKE), (FAKE, FAKE, None, FAKE, FAKE),
                 (FAKE, FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, FAKE, None)):
        boxes, order, keep, n_keep, scratch = args
        assert L.sola_box_nms(boxes, order, None, 100, 0.5, keep, n_keep, scratch, big, None) == -1
        assert b"null" in L.sola_last_error()
    assert L.sola_box_nms(ctypes.c_void_p((1 << 20) + 4), FAKE, None, 100, 0.5, FAKE, FAKE, FAKE, big, None) == -1
    assert b"aligned" in L.sola_last_error()
    assert L.sola_box_nms_profile(FAKE, FAKE, None, 100, 0.5, FAKE, FAKE, FAKE, big, None, None) == -1


def test_python_entry_points_refuse_cpu_tensors_wrong_ranks_and_dtypes():
    from sola_amd import seg_utils as su
    logit = torch.zeros(2, 1, 4, 4)
    boxes, scores = torch.zeros(3, 4), torch.zeros(3)
    for call in (lambda: su.mask_logit_stats(logit), lambda: su.calculate_stability_score(logit, 0.0, 1.0),
                 lambda: su.batched_mask_to_box(logit.bool()), lambda: su.nms(boxes, scores, 0.5),
                 lambda: su.batched_nms(boxes, scores, torch.zeros(3, dtype=torch.int64), 0.5),
                 lambda: su.filter_part_masks(logit[:, 0]), lambda: su.mask_to_rle_uncompressed(logit[:, 0])):
        with pytest.raises(SolaError, match="GPU only"):
            call()
    with pytest.raises(SolaError, match=r"\(N,1,H,W\)"):
        su.mask_logit_stats(torch.zeros(2, 3, 4, 4))
    with pytest.raises(SolaError, match="float32"):
        su.mask_logit_stats(logit.to(torch.uint8))
    with pytest.raises(SolaError, match="float32"):
        su.calculate_stability_score(logit.double(), 0.0, 1.0)
    with pytest.raises(SolaError, match="uint8/bool or float32"):
        su.mask_logit_stats(logit.to(torch.int32), logits=False)
    with pytest.raises(SolaError, match="bool or uint8"):
        su.batched_mask_to_box(logit)
    with pytest.raises(SolaError, match=r"\[N,4\]"):
        su.nms(torch.zeros(3, 5), scores, 0.5)
    with pytest.raises(SolaError, match="float32"):
        su.nms(boxes.double(), scores, 0.5)
    with pytest.raises(SolaError, match="scores"):
        su.nms(boxes, torch.zeros(2), 0.5)
    with pytest.raises(SolaError, match="idxs"):
        su.batched_nms(boxes, scores, torch.zeros(2, dtype=torch.int64), 0.5)
    with pytest.raises(SolaError, match="integers"):
        su.batched_nms(boxes, scores, torch.zeros(3), 0.5)
    with pytest.raises(SolaError, match=r"\(N,H,W\)"):
        su.filter_part_masks(logit)
    with pytest.raises(SolaError, match="uint8/bool or float32"):
        su.filter_part_masks(torch.zeros(2, 4, 4, dtype=torch.int64))
    np.testing.assert_array_equal(su.box_area(torch.tensor([[1.0, 2.0, 4.0, 4.0], [0.0, 0.0, 0.0, 9.0]])).numpy(), [6.0, 0.0])
