"""The grid-prompt stage on the GPU against the numpy restatement of its contracts (amg_cases.py, pinned in test_amg_cpu.py):
per-mask statistics from one read (sola_mask_logit_stats), greedy box NMS (sola_box_nms), the part filter and uncompressed
RLE.  Everything here is integers or float32 decisions with a stated order of operations: equality, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases as ac  # noqa: E402
from sola_amd import seg_utils as su  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["uint8", "bool", "float32", "logits"]
SMALL_SIZES = [(1, 1), (3, 5), (17, 63), (64, 64), (65, 129), (270, 481)]


def as_kind(m, kind, thr=0.0, seed=0):
    """{0,1} uint8 -> a CUDA tensor of the kind whose counted pixels are m's; the float kinds carry both zeros and both signs
    (logits: set pixels above thr, clear ones below it or on it)."""
    t = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    if kind == "uint8":
        return t * 255 if seed % 2 else t
    if kind == "bool":
        return t.bool()
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand(t.shape, device="cuda", generator=g) + 0.01
    pick = torch.randint(0, 3, t.shape, device="cuda", generator=g)
    if kind == "float32":  # != 0: negative values are set, both zeros are clear
        on = torch.where(pick == 0, -r, r)
        off = torch.where(pick == 0, torch.full_like(r, -0.0), torch.zeros_like(r))
    else:  # logits: > thr; below thr, thr itself and (at thr = 0) -0.0 are clear
        on = r * 3 + thr
        zero = torch.full_like(r, -0.0 if thr == 0 else thr)  # -0.0 is not above a threshold of 0
        off = torch.where(pick == 0, thr - r * 3, torch.where(pick == 1, zero, torch.full_like(r, thr)))
    return torch.where(t != 0, on, off).float()


def check_stats(x, logits, thr=0.0, off=1.0, what=""):
    got = su.mask_logit_stats(x, thr, off, logits=logits)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (x.shape[0], 7)
    host = x.reshape(x.shape[0], x.shape[-2], x.shape[-1]).cpu().numpy()
    want = ac.stats(host, logits, thr, thr + off, thr - off)
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(1))
        raise AssertionError(f"{what}: maps {bad.tolist()} differ; map {bad[0]}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}")
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SMALL_SIZES)
def test_stats_every_kind_and_small_size(h, w, kind):
    names, ms = ac.stat_masks(h, w)
    x = as_kind(ms, kind, seed=h + w)
    got = check_stats(x, kind == "logits", what=f"{kind} {h}x{w}")
    assert got[names.index("full"), 2] == h * w and not got[names.index("empty"), 2:].any()
    if kind in ("uint8", "logits") and h * w <= 65 * 129:  # n up to 192, each map shifted off its neighbours' alignment
        many = np.concatenate([ms] * (192 // len(ms) + 1))[:192]
        check_stats(as_kind(many, kind, seed=1), kind == "logits", what=f"{kind} {h}x{w} n=192")


@pytest.mark.parametrize("h,w", SMALL_SIZES)
def test_stats_logits_on_the_thresholds_and_a_second_threshold_pair(h, w):
    for thr, off in ((0.0, 1.0), (0.25, 0.5)):
        _, ms = ac.stat_masks(h, w)
        x = torch.cat([as_kind(ms, "logits", thr=thr, seed=3), torch.from_numpy(ac.threshold_logits(h, w, thr, thr + off, thr - off))[None].cuda()])
        st = check_stats(x, True, thr, off, what=f"logits {h}x{w} thr {thr} off {off}")
        # the wrappers over the table
        score = su.calculate_stability_score(x.unsqueeze(1), thr, off)
        assert score.dtype == torch.float32 and score.is_cuda
        with np.errstate(invalid="ignore", divide="ignore"):
            np.testing.assert_array_equal(score.cpu().numpy(), st[:, 0].astype(np.float32) / st[:, 1].astype(np.float32))
        box = su.batched_mask_to_box(x > thr)
        assert box.dtype == torch.int64
        np.testing.assert_array_equal(box.cpu().numpy(), st[:, 3:])


def test_stats_unaligned_views_empty_shapes_and_four_dims():
    _, ms = ac.stat_masks(17, 63)
    for kind in ("uint8", "logits"):
        flat = as_kind(ms, kind, seed=2).reshape(-1)
        for shift in (1, 2, 3, 5):  # a contiguous tensor that starts 1..5 elements into an allocation
            buf = torch.zeros(flat.numel() + 8, device="cuda", dtype=flat.dtype)
            buf[shift:shift + flat.numel()] = flat
            x = buf[shift:shift + flat.numel()].view(ms.shape)
            assert x.is_contiguous() and x.data_ptr() % 16 != 0
            check_stats(x, kind == "logits", what=f"{kind} shifted by {shift}")
    z = su.mask_logit_stats(torch.zeros((3, 0, 7), device="cuda"))
    assert tuple(z.shape) == (3, 7) and not z.any()
    assert tuple(su.mask_logit_stats(torch.zeros((0, 4, 7), device="cuda")).shape) == (0, 7)
    x = as_kind(ms, "logits")
    assert torch.equal(su.mask_logit_stats(x.unsqueeze(1)), su.mask_logit_stats(x))


def test_stats_1080p_three_maps_repeat_and_side_stream():
    h, w = 1080, 1920
    names, ms = ac.stat_masks(h, w, n_random=1)
    pick = [names.index("blobs0"), names.index("noise"), names.index("bottom-right")]
    x = as_kind(ms[pick], "logits", seed=4)
    first = check_stats(x, True, what="1080p")
    again = su.mask_logit_stats(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = su.mask_logit_stats(x)
    side.synchronize()
    np.testing.assert_array_equal(again.cpu().numpy(), first)
    np.testing.assert_array_equal(other.cpu().numpy(), first)
    check_stats(torch.from_numpy(ms[pick]).cuda(), False, what="1080p uint8")


# -------------------------------------------------------------------------------------------------------------------- NMS
def run_nms(boxes, scores, idxs, thr, scratch=None):
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    if idxs is None and scratch is None:
        got = su.nms(b, s, thr)
    else:
        got = su.batched_nms(b, s, None if idxs is None else torch.from_numpy(idxs).cuda(), thr, scratch=scratch)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
    return got.cpu().tolist()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 130, 1000])
def test_nms_equals_the_restatement(n):
    for make in (ac.rect_boxes, ac.float_boxes):
        boxes = make(n, n + 1).reshape(n, 4)
        scores = ac.tied_scores(n, n)
        for k in (1, 3, n):
            idxs = None if k == 1 else ac.categories(n, max(k, 1), n)
            for thr in (0.5, 0.7):
                want = ac.box_nms(boxes, scores, idxs, thr)
                assert run_nms(boxes, scores, idxs, thr) == want, (make.__name__, n, k, thr)
                if k == n and n:
                    assert sorted(want) == list(range(n))  # a category each: nothing interacts
    if 2 <= n <= 130:  # and the array form of the restatement is the scalar double loop
        assert ac.box_nms(boxes, scores, None, 0.5) == ac.box_nms_loop(boxes, ac.visiting_order(scores), None, 0.5)


def test_nms_3072_boxes_and_prefilled_scratch():
    n = 3072
    boxes, scores = ac.rect_boxes(n, 7), ac.tied_scores(n, 7)
    idxs = ac.categories(n, 3, 7)
    want = ac.box_nms(boxes, scores, idxs, 0.7)
    assert 100 < len(want) < n
    assert run_nms(boxes, scores, idxs, 0.7) == want
    nb = su.lib().sola_box_nms_scratch_bytes(n)
    scratch = torch.full((nb,), 0xFF, device="cuda", dtype=torch.uint8)  # written before it is read
    assert run_nms(boxes, scores, idxs, 0.7, scratch=scratch) == want
    fb = ac.float_boxes(n, 8)
    assert run_nms(fb, scores, None, 0.5) == ac.box_nms(fb, scores, None, 0.5)


def test_nms_hand_boxes_ties_exact_threshold_and_box_area():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [0, 0, 10, 4.5], [0, 4, 10, 10], [20, 20, 30, 30], [20, 20, 30, 27]], np.float32)
    scores = np.array([0.9, 0.8, 0.8, 0.7, 0.95, 0.1], np.float32)
    assert run_nms(boxes, scores, None, 0.5) == [4, 0, 1]
    assert run_nms(boxes, scores, None, 0.7) == [4, 0, 1, 3, 5]
    assert run_nms(boxes, scores, np.array([0, 0, 1, 0, 0, 1], np.int64), 0.5) == [4, 0, 1, 2, 5]
    dots = np.array([[5, 5, 5, 5], [5, 5, 5, 5]], np.float32)
    assert run_nms(dots, np.ones(2, np.float32), None, 0.5) == [0, 1]
    np.testing.assert_array_equal(su.box_area(torch.from_numpy(boxes).cuda()).cpu().numpy(), [100, 50, 45, 60, 100, 70])


# ------------------------------------------------------------------------------------------------- part filter, plain RLE
@pytest.mark.parametrize("n", [1, 2, 40, 300])
def test_filter_part_masks_equals_the_loop(n):
    masks = ac.part_masks(n, 135, 240, n)
    want = ac.filter_part(masks)
    for t in (torch.from_numpy(masks).cuda(), torch.from_numpy(masks).cuda().float()):
        got = su.filter_part_masks(t)
        assert got.dtype == torch.bool and not got.is_cuda
        np.testing.assert_array_equal(got.numpy(), want)
    if n >= 40:
        assert want.any() and not want.all()
        np.testing.assert_array_equal(su.filter_part_masks(torch.from_numpy(masks).cuda(), 0.3).numpy(), ac.filter_part(masks, 0.3))


def test_mask_to_rle_uncompressed_equals_the_restatement():
    h, w = 17, 63
    names, ms = ac.stat_masks(h, w)
    for kind in ("uint8", "logits"):
        got = su.mask_to_rle_uncompressed(as_kind(ms, kind, seed=6), logits=kind == "logits")
        assert len(got) == len(ms)
        for name, g, m in zip(names, got, ms):
            assert g == ac.rle_uncompressed(m), name
            assert sum(g["counts"]) == h * w and all(isinstance(c, int) for c in g["counts"])
        assert got[names.index("empty")]["counts"] == [h * w]
        assert got[names.index("full")]["counts"] == [0, h * w]
    assert su.mask_to_rle_uncompressed(torch.zeros((0, 4, 4), device="cuda", dtype=torch.uint8)) == []
