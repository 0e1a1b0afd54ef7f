"""sola_mask_components / sola_mask_fill_small on the GPU against the restatement in components_cases.py (pinned on the CPU
by test_components_cpu.py): every element of labels, areas and the rewritten scores / masks, exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import components_cases as cc  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["uint8", "bool", "float32", "logits"]
_FRAMES, _WANT, _SCORES = {}, {}, {}


@pytest.fixture(scope="module")
def su():
    from sola_amd import seg_utils
    assert tuple(seg_utils.CC_TILE) == cc.TILE
    return seg_utils


def stack(h, w):
    """(names, (N,h,w) uint8 {0,1}) of a size, built once."""
    if (h, w) not in _FRAMES:
        fr = cc.big_frames(h, w) if (h, w) == cc.BIG else cc.frames(h, w)
        _FRAMES[(h, w)] = ([n for n, _ in fr], np.stack([m for _, m in fr]))
    return _FRAMES[(h, w)]


def want(h, w, connectivity):
    """The restatement's (labels, areas) of stack(h, w), computed once and left unchanged."""
    key = (h, w, connectivity)
    if key not in _WANT:
        _WANT[key] = cc.label_frames(stack(h, w)[1], connectivity)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def scores(h, w):
    if (h, w) not in _SCORES:
        _SCORES[(h, w)] = np.stack([cc.scores_from_mask(m, i) for i, m in enumerate(stack(h, w)[1])])
        _SCORES[(h, w)].setflags(write=False)
    return _SCORES[(h, w)]


def as_kind(m, kind, seed=0):
    """{0,1} uint8 -> a CUDA tensor of the kind whose set pixels are m's; the float kinds carry both zeros and both signs."""
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
    else:  # logits: > 0; negative, zero and -0.0 are clear
        on = r
        off = torch.where(pick == 0, -r, torch.where(pick == 1, torch.full_like(r, -0.0), torch.zeros_like(r)))
    return torch.where(t != 0, on, off).float()


def check_frames(got, wanted, names, what):
    got = got.cpu().numpy()
    if not np.array_equal(got, wanted):
        bad = [names[i] for i in range(len(names)) if not np.array_equal(got[i], wanted[i])]
        i = names.index(bad[0])
        at = np.argwhere(got[i] != wanted[i])[0]
        raise AssertionError(f"{what}: frames {bad} differ; {bad[0]} first at {tuple(at)}: got {got[i][tuple(at)]}, "
                             f"want {wanted[i][tuple(at)]} ({int((got[i] != wanted[i]).sum())} elements)")


ALL_SIZES = cc.SIZES + [cc.BIG]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("h,w", ALL_SIZES, ids=[f"{h}x{w}" for h, w in ALL_SIZES])
def test_labels_and_areas_equal_the_restatement(su, h, w, connectivity, kind):
    names, m = stack(h, w)
    wl, wa = want(h, w, connectivity)
    labels, areas = su.connected_components(as_kind(m, kind, seed=h + w), connectivity, logits=kind == "logits")
    assert labels.dtype == torch.int32 and areas.dtype == torch.int32 and labels.shape == m.shape
    check_frames(labels, wl, names, "labels")
    check_frames(areas, wa, names, "areas")


@pytest.mark.parametrize("h,w", [(17, 33), (65, 129)])
def test_sam2_layout_and_per_frame_calls_give_the_same(su, h, w):
    names, m = stack(h, w)
    t = torch.from_numpy(m).cuda()
    l3, a3 = su.connected_components(t)
    l4, a4 = su.connected_components(t.unsqueeze(1))
    assert l4.shape == (len(names), 1, h, w)
    assert torch.equal(l4[:, 0], l3) and torch.equal(a4[:, 0], a3)
    for i in range(len(names)):  # no label or count leaks between the frames of one call
        li, ai = su.connected_components(t[i:i + 1])
        assert torch.equal(li[0], l3[i]) and torch.equal(ai[0], a3[i]), names[i]


@pytest.mark.parametrize("max_area", [1, 8, 9, 100])
@pytest.mark.parametrize("h,w", [(1, 70), (70, 1), (17, 33), (65, 129), (128, 256)])
def test_fill_holes_equals_the_restatement_bit_for_bit(su, h, w, max_area):
    names, _ = stack(h, w)
    s = scores(h, w)
    wanted = np.stack([cc.fill_holes(f, max_area) for f in s]).view(np.int32)
    t = torch.from_numpy(s.copy()).cuda()
    before = t.clone()
    got = su.fill_holes_in_mask_scores(t.unsqueeze(1), max_area)
    assert got.shape == (len(names), 1, h, w) and got.dtype == torch.float32
    assert torch.equal(t.view(torch.int32), before.view(torch.int32))  # the input is left alone
    check_frames(got[:, 0].view(torch.int32), wanted, names, f"fill_holes max_area {max_area}")
    # in place: out aliasing in
    same = su.fill_holes_in_mask_scores(t, max_area, out=t)
    assert same.data_ptr() == t.data_ptr()
    check_frames(t.view(torch.int32), wanted, names, f"in-place fill_holes max_area {max_area}")


def test_fill_holes_fill_value_connectivity_and_bad_max_area(su):
    h, w = 65, 129
    names, _ = stack(h, w)
    s = scores(h, w)
    t = torch.from_numpy(s.copy()).cuda()
    wanted = np.stack([cc.fill_holes(f, 8, 0.75, 4) for f in s]).view(np.int32)
    check_frames(su.fill_holes_in_mask_scores(t, 8, fill_value=0.75, connectivity=4).view(torch.int32), wanted, names, "fill 4")
    for bad in (0, -1):
        with pytest.raises(SolaError, match="max_area"):
            su.fill_holes_in_mask_scores(t, bad)


@pytest.mark.parametrize("dtype", ["uint8", "bool", "float32"])
@pytest.mark.parametrize("mode", ["holes", "islands"])
def test_remove_small_regions_equals_the_restatement(su, mode, dtype):
    for h, w in ((17, 33), (65, 129)):
        names, m = stack(h, w)
        t = torch.from_numpy(m).cuda()
        t = t.bool() if dtype == "bool" else t.float() if dtype == "float32" else t
        for max_area in (0, 8, 9):
            wanted = np.stack([cc.remove_small(f, max_area, mode) for f in m])
            got = su.remove_small_regions(t.unsqueeze(1), max_area, mode)
            assert got.dtype == t.dtype and got.shape == (len(names), 1, h, w)
            check_frames(got[:, 0].to(torch.uint8), wanted, names, f"{mode} {max_area} {dtype}")


def test_views_go_through_prep(su):
    h, w = 65, 129
    names, m = stack(h, w)
    wl, wa = want(h, w, 8)
    # a 4-byte-offset view of float32 and a 1-byte-offset view of uint8: the frames start one element into a buffer
    for kind in ("float32", "uint8"):
        t = as_kind(m, kind)
        buf = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
        buf[1:] = t.reshape(-1)
        view = buf[1:].view(t.shape)
        assert view.data_ptr() % 8 != 0 or kind == "uint8"
        labels, areas = su.connected_components(view)
        check_frames(labels, wl, names, f"offset {kind} labels")
        check_frames(areas, wa, names, f"offset {kind} areas")
    # non-contiguous: every second column of a wider tensor, and a transposed one
    wide = torch.zeros((len(names), h, 2 * w), device="cuda", dtype=torch.uint8)
    wide[:, :, ::2] = torch.from_numpy(m).cuda()
    labels, areas = su.connected_components(wide[:, :, ::2])
    check_frames(labels, wl, names, "strided labels")
    tr = torch.from_numpy(np.ascontiguousarray(m.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not tr.is_contiguous()
    labels, areas = su.connected_components(tr)
    check_frames(areas, wa, names, "transposed areas")
    s = scores(h, w)
    sw = torch.zeros((len(names), h, 2 * w), device="cuda")
    sw[:, :, ::2] = torch.from_numpy(s.copy()).cuda()
    wanted = np.stack([cc.fill_holes(f, 8) for f in s]).view(np.int32)
    check_frames(su.fill_holes_in_mask_scores(sw[:, :, ::2], 8).view(torch.int32), wanted, names, "strided fill")


def test_nothing_relies_on_what_the_scratch_held(su):
    from sola_amd import _lib
    h, w = 65, 129
    names, m = stack(h, w)
    wl, wa = want(h, w, 8)
    nb = _lib.lib().sola_mask_components_scratch_bytes(len(names), h, w)
    t = torch.from_numpy(m).cuda()
    s = torch.from_numpy(scores(h, w).copy()).cuda()
    wanted = np.stack([cc.fill_holes(f, 8) for f in scores(h, w)]).view(np.int32)
    for fill in (0xFF, 0x00, 0x7F):
        scratch = torch.full((nb,), fill, device="cuda", dtype=torch.uint8)
        labels, areas = su.connected_components(t, scratch=scratch)
        check_frames(labels, wl, names, f"labels, scratch {fill:#x}")
        check_frames(areas, wa, names, f"areas, scratch {fill:#x}")
        scratch.fill_(fill)
        check_frames(su.fill_holes_in_mask_scores(s, 8, scratch=scratch).view(torch.int32), wanted, names, f"fill, scratch {fill:#x}")


def test_consecutive_sizes_and_two_streams_are_bit_identical(su):
    big_names, big = stack(128, 256)
    small_names, small = stack(17, 33)
    tb, ts = torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()
    sb = torch.from_numpy(scores(128, 256).copy()).cuda()
    # the cached scratch is shared by consecutive calls of different sizes on one stream
    lb, ab = su.connected_components(tb)
    lsm, asm = su.connected_components(ts)
    lb2, ab2 = su.connected_components(tb)
    fb = su.fill_holes_in_mask_scores(sb, 8)
    check_frames(lb, want(128, 256, 8)[0], big_names, "large, first")
    check_frames(lsm, want(17, 33, 8)[0], small_names, "small after large")
    check_frames(asm, want(17, 33, 8)[1], small_names, "small after large")
    assert torch.equal(lb, lb2) and torch.equal(ab, ab2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        l2, a2 = su.connected_components(tb)
        f2 = su.fill_holes_in_mask_scores(sb, 8)
    side.synchronize()
    assert torch.equal(l2, lb) and torch.equal(a2, ab) and torch.equal(f2.view(torch.int32), fb.view(torch.int32))


def test_error_paths(su):
    from sola_amd import _lib
    L = _lib.lib()
    t = torch.zeros((2, 1, 17, 33), device="cuda", dtype=torch.uint8)
    with pytest.raises(SolaError, match="connectivity"):
        su.connected_components(t, connectivity=6)
    with pytest.raises(SolaError, match="connectivity"):
        su.fill_holes_in_mask_scores(t.float(), 8, connectivity=0)
    with pytest.raises(SolaError, match="GPU only"):
        su.connected_components(t.cpu())
    with pytest.raises(SolaError, match="GPU only"):
        su.fill_holes_in_mask_scores(t.float().cpu(), 8)
    with pytest.raises(SolaError, match="uint8/bool or float32"):
        su.connected_components(t.to(torch.int32))
    # a short scratch through the raw ABI: refused before any launch, the outputs untouched
    need = L.sola_mask_components_scratch_bytes(2, 17, 33)
    scratch = torch.zeros(need, device="cuda", dtype=torch.uint8)
    out = torch.full((2, 2, 17, 33), -7, device="cuda", dtype=torch.int32)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    st = _lib.current_stream(t.device)
    assert L.sola_mask_components(p(t), 0, 2, 17, 33, 8, p(out[0]), p(out[1]), p(scratch), need - 1, st) == -1
    assert b"scratch" in L.sola_last_error()
    f = t.float()
    assert L.sola_mask_fill_small(p(f), 3, 2, 17, 33, 8, 8, 0.1, p(f), p(scratch), need - 1, st) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((f == 0).all())
    assert L.sola_mask_components(p(t), 0, 2, 17, 33, 8, p(out[0]), p(out[1]), p(scratch), need, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # empty calls are no-ops
    e = torch.zeros((0, 1, 17, 33), device="cuda", dtype=torch.uint8)
    labels, areas = su.connected_components(e)
    assert labels.shape == e.shape and areas.shape == e.shape
    assert su.fill_holes_in_mask_scores(e.float(), 8).shape == e.shape
