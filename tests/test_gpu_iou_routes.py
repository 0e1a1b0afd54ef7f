"""Mask IoU through the C ABI on every route of its launcher (iou_cases.py): exact counts on dirty scratch and dirty outputs, call
after call with DIFFERENT mask sets through the same scratch - a count row left by the previous call is then a wrong row, where
repeating one set (tests/test_gpu_iou.py) makes it the right one - and the route each call took read from the profiler's launch counts."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou_cases as ic  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402
from sola_amd._lib import check, current_stream, lib, ptr, tuned  # noqa: E402

FENCE = 64  # int64 words on each side of the outputs
SENTINEL = -0x5A5A5A5A5A5A5A5B
_DEV = {}


def device_set(case, which):
    """(A, B, inter, union) of the case's mask set on the device, uploaded once; B starts case.offset bytes into its storage."""
    key = (case.id, which)
    if key not in _DEV:
        A, B = ic.make_masks(case, which)
        a = torch.from_numpy(A.copy()).cuda()  # (the shared arrays are read-only)
        store = torch.empty(B.nbytes + case.offset, dtype=torch.uint8, device="cuda")
        b = store[case.offset:].view(a.dtype).view(B.shape)
        b.copy_(torch.from_numpy(B.copy()))
        assert b.data_ptr() % 16 == case.offset % 16 and a.data_ptr() % 16 == 0
        ri, ru = ic.reference(case, which)
        _DEV[key] = (a, b, torch.from_numpy(ri.copy()).cuda(), torch.from_numpy(ru.copy()).cuda())
    return _DEV[key]


def dirty_scratch(case):
    """The call's scratch, every byte 0xFF: the larger of the two restated sizes, or no more than the ABI asks for."""
    assert lib().sola_mask_iou_scratch_bytes(case.P, case.R, case.H, case.W) == ic.abi_scratch_bytes(case.P, case.R, case.H, case.W)
    return torch.full((ic.scratch_bytes(case),), 0xFF, dtype=torch.uint8, device="cuda")


def fenced_outputs(case):
    n = case.P * case.R
    buf = torch.full((2 * FENCE + 2 * n,), SENTINEL, dtype=torch.int64, device="cuda")
    return buf, buf[FENCE:FENCE + n].view(case.P, case.R), buf[FENCE + n:FENCE + 2 * n].view(case.P, case.R)


def call(case, a, b, inter, union, scratch):
    check(lib().sola_mask_iou_matrix(ptr(a), ptr(b), 0 if case.dtype == "u8" else 1, case.P, case.R, case.H, case.W, case.h, case.w,
                                     ptr(inter), ptr(union), ptr(scratch), scratch.numel(), current_stream(a.device)), "sola_mask_iou_matrix")


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_exact_counts_on_dirty_scratch_and_outputs_call_after_call(case):
    """The scratch starts as 0xFF bytes, the outputs as -1 inside a fenced buffer.  Three calls through that scratch, nothing cleared
    in between: the case's mask set, its complemented and shifted twin, the first set again.  Every call's counts are the exact
    reference's (so every element was written), and the fences stay as they were."""
    scratch = dirty_scratch(case)
    buf, inter, union = fenced_outputs(case)
    with tuned(**dict(case.switches)):
        for which in (0, 1, 0):
            a, b, ri, ru = device_set(case, which)
            inter.fill_(-1)
            union.fill_(-1)
            call(case, a, b, inter, union, scratch)
            assert torch.equal(inter, ri), (case.id, which, "inter", int((inter != ri).sum()))
            assert torch.equal(union, ru), (case.id, which, "union", int((union != ru).sum()))
            assert bool((buf[:FENCE] == SENTINEL).all()) and bool((buf[-FENCE:] == SENTINEL).all()), (case.id, which)


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_the_route_is_the_restated_one(case):
    """The profiler's launch counts of the call: a onepass/* case is ONE launch of the pack category and none of the pair kernel; a
    decline/* case is one pair launch behind one pack launch (both sets in one streaming launch) or two.  The counts cannot tell the
    packed form from the ticket form, nor the G of the instantiation: those rest on iou_cases.route, which test_iou_cpu.py holds
    to the launcher's limits."""
    scratch = dirty_scratch(case)
    buf, inter, union = fenced_outputs(case)
    a, b, ri, ru = device_set(case, 0)
    branch = ic.case_route(case)
    try:
        _lib.profile_enable(True, categories=["iou_pack", "iou_pair"])
        _lib.profile_read(reset=True)
        with tuned(**dict(case.switches)):
            call(case, a, b, inter, union, scratch)
        pr = _lib.profile_read(reset=True)
    finally:
        _lib.profile_enable(False)
    launches = (pr["iou_pack"]["launches"], pr["iou_pair"]["launches"])
    if branch.startswith("onepass/"):
        assert launches == (1, 0), (case.id, branch, launches)
    else:
        assert launches == ((1 if ic.case_fallback(case) == "pair-stream" else 2), 1), (case.id, branch, ic.case_fallback(case), launches)
    assert torch.equal(inter, ri) and torch.equal(union, ru)


def test_both_forms_agree_call_after_call_past_the_ends_of_the_rings():
    """The packed form's cases at 64 x 96 under iou_packed 1, 0, 1 in turn, the two mask sets alternating through one scratch per case.
    The library hands every call a range of its ticket ring (4096 tickets, a group each) and every packed call 4 R lines of its
    pair-word ring (16384): the ticket-form phase alone takes more than 4096 tickets and the packed phases more than 16384 lines, so both
    rings are walked past their ends and every ticket and word must have gone back to zero."""
    cases = [ic.BY_ID[i] for i in ic.RING_IDS]
    scratch = {c.id: dirty_scratch(c) for c in cases}
    outs, tickets, lines = [], 0, 0
    n = 0
    for packed, sweeps in ((1, 11), (0, 80), (1, 11)):
        with tuned(iou_packed=packed):
            for _ in range(sweeps):
                for c in cases:
                    assert ic.case_route(c, {"iou_packed": packed}).endswith("/pk" if packed else "/ticket")
                    a, b, ri, ru = device_set(c, n & 1)
                    out = torch.full((2, c.P, c.R), -1, dtype=torch.int64, device="cuda")
                    call(c, a, b, out[0], out[1], scratch[c.id])
                    outs.append((out, ri, ru))
                    if packed:
                        lines += 4 * c.R
                    else:
                        tickets += ic.launch_shape(c)[2]
                    n += 1
    assert tickets > ic.OP_TICKETS and lines > ic.OP_ACC_LINES
    torch.cuda.synchronize()
    for i, (out, ri, ru) in enumerate(outs):
        assert torch.equal(out[0], ri) and torch.equal(out[1], ru), i


def test_alternating_calls_at_the_ticket_forms_real_size():
    """P = 4 tracks x 33 prompts at 720 x 1280 (the ticket form, 513 blocks per call) through seg_utils.mask_iou_matrix and the scratch
    it caches per stream: 40 calls that alternate two mask sets on one stream, then 20 on each of two streams at once, the streams
    out of step with each other.  A block that took its group's last ticket before another block's row had landed would fold the other
    set's row.  This is a net, not a proof: such a race need not fire in any given run, so a pass shows little and only a failure
    means something; the deterministic half is the check of the built code object in test_iou_cpu.py."""
    case = ic.ALTERNATING
    assert ic.case_route(case) == "onepass/G2/ticket" and ic.launch_shape(case)[2] * ic.launch_shape(case)[3] == 513
    sets = [device_set(case, which) for which in (0, 1)]
    torch.cuda.synchronize()
    outs = []
    for i in range(40):
        outs.append((i & 1, seg_utils.mask_iou_matrix(sets[i & 1][0], sets[i & 1][1])))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(20):
        for k, st in enumerate(streams):
            with torch.cuda.stream(st):
                which = (i + k) & 1
                outs.append((which, seg_utils.mask_iou_matrix(sets[which][0], sets[which][1])))
    torch.cuda.synchronize()
    for i, (which, (inter, union)) in enumerate(outs):
        assert torch.equal(inter, sets[which][2]) and torch.equal(union, sets[which][3]), (i, which)
