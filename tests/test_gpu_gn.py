"""GroupNorm forward and backward against float64 (gn_cases.py, checked in test_gn_cpu.py) in every kernel shape, row format and unit layout
of launch_group_norm and launch_group_norm_bwd, through sola_group_norm_ex and sola_group_norm_backward_ex.  Every call runs on FENCED
memory: x, dy and dy2 inside NaN-filled buffers (fence rows in front and behind, NaN in every row no unit owns), gamma, beta and pe with NaN
behind them, outputs and casts inside sentinel-filled buffers, the slice scratch and the backward's scratch exactly as large as they must be
with a sentinel tail - so a read outside a unit or a write outside its rows shows as a wrong value, never as a fault.  With -s the module ends
with the worst error / bar of every shape (profiles/gn_parity.txt)."""
import collections
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_cases as gc  # noqa: E402
from sola_amd._lib import check, current_stream, lib, ptr, tuned  # noqa: E402

pytestmark = pytest.mark.gpu

FENCE = 8                                   # fence rows in front of and behind every matrix
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5         # NaN patterns (f32; f16 and bfloat16) no kernel produces from finite rows
TAIL, TAIL_FILL = 4096, 0xA5                # bytes behind a scratch buffer
SOLA_ERR_ARG, SOLA_ERR_WORKSPACE = -1, -4
WORST = collections.defaultdict(lambda: [0.0, 0])  # (direction, shape, formats) -> worst error / bar, runs


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    print("\nGroupNorm against float64: worst error / bar per kernel shape and row formats (in-out[+cast]; backward: x[,dy2])")
    print("bar of f32 rows = 8 x the float32 restatement's error, of max|reference|: " +
          ", ".join(f"{d} {v} {gc.F32_MEASURED[(d, v)]:.2e} -> {gc.F32_BAR[(d, v)]:.2e}" for d, v in sorted(gc.F32_MEASURED)))
    print(f"y, y2 and dx of cases whose largest unit has {gc.LARGE_UNIT} elements or more: at most {gc.LARGE_UNIT_BAR:.2e} (gn_cases.f32_bar)")
    print("16-bit rows: + 2^-11 (f16), 2^-21 (split pairs) of |reference| per element")
    print(f"{'direction':<10}{'shape':<18}{'formats':<16}{'worst':>8}{'runs':>6}")
    for (d, shape, fmts), (r, n) in sorted(WORST.items()):
        print(f"{d:<10}{shape:<18}{fmts:<16}{r:8.4f}{n:6d}")


def record(case, shape, r):
    fmts = gc.FMT_NAME[case.in_fmt]
    if case.direction == "fwd":
        fmts += "-" + gc.FMT_NAME[case.out_fmt] + ("+" + gc.FMT_NAME[case.cast_fmt] if case.cast_fmt else "")
    elif case.dy2_fmt is not None:
        fmts += "," + gc.FMT_NAME[case.dy2_fmt]
    w = WORST[(case.direction, gc.shape_name(shape), fmts)]
    w[0], w[1] = max(w[0], r), w[1] + 1


def fenced_in(t):
    """(buffer, view) on the device: ``t`` [rows, cols] (or [cols]) between FENCE rows of NaN."""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    buf = torch.full((t2.shape[0] + 2 * FENCE, t2.shape[1]), float("nan"), dtype=t.dtype)
    buf[FENCE:FENCE + t2.shape[0]] = t2
    buf = buf.cuda()
    return buf, buf[FENCE:FENCE + t2.shape[0]]


class Out:
    """One output matrix [rows, cols] of 4- or 2-byte elements between FENCE rows, everything sentinels before the call."""

    def __init__(self, rows, cols, wide=True):
        self.rows = rows
        self.buf = torch.full((rows + 2 * FENCE, cols), SENT32 if wide else SENT16, dtype=torch.int32 if wide else torch.int16, device="cuda")
        self.sent = SENT32 if wide else SENT16
        self.view = self.buf[FENCE:FENCE + rows]

    def assert_fence(self, owned, what):
        """owned: bool [rows] on the device, the rows that must be written - every other element must still be the sentinel."""
        held = self.buf == self.sent
        assert bool(held[:FENCE].all()) and bool(held[FENCE + self.rows:].all()), (what, "a write in front of or behind the matrix")
        inside = held[FENCE:FENCE + self.rows]
        assert bool(inside[~owned].all()), (what, "a write into a row no unit owns")
        assert not bool(inside[owned].any()), (what, "an element of a unit was not written")

    def assert_untouched(self, what):
        assert bool((self.buf == self.sent).all()), (what, "written by a call that must not write it")

    def to(self, dtype):
        return self.view.view(dtype)


def scratch(nbytes):
    buf = torch.full((nbytes + TAIL,), TAIL_FILL, dtype=torch.uint8, device="cuda")
    return buf


def assert_tail(buf, nbytes, what):
    assert bool((buf[nbytes:] == TAIL_FILL).all()), (what, "a write behind the scratch")


class Dropout:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        check(lib().sola_set_stage_dropout(gc.DROP_P if self.on else 0.0, gc.DROP_SEED), "sola_set_stage_dropout")

    def __exit__(self, *exc):
        check(lib().sola_set_stage_dropout(0.0, 0), "sola_set_stage_dropout")


def live_shape(case):
    out = (C.c_int * 5)()
    if case.direction == "fwd":
        check(lib().sola_group_norm_shape(0, gc.ntok(case), case.cg, case.in_fmt, case.out_fmt, int(case.dropout), out), "shape")
    else:
        check(lib().sola_group_norm_shape(1, gc.ntok(case), case.cg, 0, 0, 0, out), "shape")
    return tuple(out)


def units_dev(case):
    t = gc.units_table(case)
    return None if t is None else t.cuda()


Fwd = collections.namedtuple("Fwd", "status y y2 y_cast y2_cast guard stats stats_written raw")


def run_forward(case, inp, switches=None, stats=False, want_status=0):
    """One sola_group_norm_ex call of ``case`` on ``inp`` under the case's switches and ``switches``.  y / y2 come back on the host as the
    format's own dtype (split pairs decoded to float64), casts as their dtype, raw = the device buffers (for bit comparisons)."""
    geo = gc.geometry(case)
    Cn = gc.channels(case)
    what = (case.id, switches)
    owned = geo.owned.cuda()
    xb, xv = fenced_in(inp.x)
    gb, gv = fenced_in(inp.gamma)
    bb, bv = fenced_in(inp.beta)
    pb, pv = fenced_in(inp.pe)
    wide = case.out_fmt != gc.F16
    y = Out(geo.rows, Cn, wide)
    y2 = Out(geo.rows, Cn, wide) if case.y2 else None
    yc = Out(geo.rows, Cn, False) if case.cast_fmt else None
    y2c = Out(geo.rows, Cn, False) if case.cast_fmt and case.y2 else None
    guard = torch.tensor([SENT32, 0 if case.out_fmt != gc.F32 else 0x5A5A, SENT32], dtype=torch.int32, device="cuda")
    scale = torch.tensor([float("nan"), case.in_scale or 1.0, float("nan")], device="cuda") if case.in_scale else None
    n_units = len(geo.units) * case.groups
    st = Out(n_units, 2, True)
    written = C.c_int(0)
    ud = units_dev(case)
    n_inst, inner, outer_stride, inner_stride, tok_stride, ntok = geo.args
    with tuned(**dict(case.switches, **(switches or {}))), Dropout(case.dropout):
        shape = live_shape(case)
        assert shape == gc.expected_shape(case, switches), (what, shape)
        ws_bytes = n_units * shape[4] * 8 if shape[0] == gc.SLICED else 0
        ws = scratch(ws_bytes)
        status = lib().sola_group_norm_ex(
            ptr(xv), ptr(y.view), ptr(y2.view) if y2 else None, ptr(pv) if case.y2 else None, ptr(gv), ptr(bv), n_inst, inner, outer_stride,
            inner_stride, tok_stride, ntok, Cn, case.groups, gc.EPS, gc.SLOPE, int(case.leaky), case.in_fmt, case.out_fmt, ptr(ud),
            ptr(scale[1:]) if scale is not None else None, ptr(guard[1:]), ptr(yc.view) if yc else None, ptr(y2c.view) if y2c else None,
            case.cast_fmt, ptr(ws), ws_bytes, ptr(st.view) if stats else None, C.byref(written) if stats else None, current_stream(xb.device))
    torch.cuda.synchronize()
    assert status == want_status, (what, status, lib().sola_last_error())
    assert_tail(ws, ws_bytes, what)
    assert int(guard[0]) == SENT32 and int(guard[2]) == SENT32, (what, "a write beside the guard word")
    outs = [o for o in (y, y2, yc, y2c) if o is not None]
    if status != 0:
        for o in outs + [st]:
            o.assert_untouched(what)
        return Fwd(status, None, None, None, None, int(guard[1]), None, written.value, None)
    for o in outs:
        o.assert_fence(owned, what)

    def host(o):
        if o is None:
            return None
        if case.out_fmt == gc.F16:
            return o.to(torch.float16).cpu()
        return gc.decode_sp16(o.to(torch.float32).cpu()) if case.out_fmt == gc.SP16 else o.to(torch.float32).cpu()

    cast = lambda o: None if o is None else o.to(gc.TORCH16[case.cast_fmt]).cpu()  # noqa: E731
    if shape[0] == gc.SLICED and stats:
        assert written.value == 1, (what, "the sliced shape did not report its statistics")
        st.assert_fence(torch.ones(n_units, dtype=torch.bool, device="cuda"), what)
    else:
        assert written.value == 0, (what, "statistics reported by a shape that writes none")
        st.assert_untouched(what)
    return Fwd(status, host(y), host(y2), cast(yc), cast(y2c), int(guard[1]), st.to(torch.float32).cpu(), written.value,
               [o.buf for o in outs])


Bwd = collections.namedtuple("Bwd", "status dx dgamma dbeta dx16 raw")


def run_backward(case, inp, switches=None, short=0, stats_in=None, want_status=0):
    geo = gc.geometry(case)
    Cn = gc.channels(case)
    what = (case.id, switches)
    owned = geo.owned.cuda()
    xb, xv = fenced_in(inp.x)
    db, dv = fenced_in(inp.dy)
    d2b, d2v = fenced_in(inp.dy2) if inp.dy2 is not None else (None, None)
    gb, gv = fenced_in(inp.gamma)
    bb, bv = fenced_in(inp.beta)
    dx = Out(geo.rows, Cn)
    dg, dbt = Out(1, Cn), Out(1, Cn)
    dx16 = Out(geo.rows, Cn, False) if case.dx16 else None
    n_inst, inner, outer_stride, inner_stride, tok_stride, ntok = geo.args
    nb = 2 * n_inst * Cn * 4
    sc = scratch(nb)
    ud = units_dev(case)
    with tuned(**dict(case.switches, **(switches or {}))), Dropout(case.dropout):
        shape = live_shape(case)
        assert shape == gc.expected_shape(case, switches), (what, shape)
        status = lib().sola_group_norm_backward_ex(
            ptr(xv), ptr(dv), ptr(d2v), ptr(gv), ptr(bv), ptr(dx.view), ptr(dg.view), ptr(dbt.view), n_inst, inner, outer_stride, inner_stride,
            tok_stride, ntok, Cn, case.groups, gc.EPS, gc.SLOPE, int(case.leaky), ptr(ud), case.in_fmt, case.dy2_fmt or 0,
            ptr(dx16.view) if dx16 else None, ptr(stats_in), ptr(sc), nb - short, current_stream(xb.device))
    torch.cuda.synchronize()
    assert status == want_status, (what, status, lib().sola_last_error())
    assert_tail(sc, nb, what)
    outs = [o for o in (dx, dx16) if o is not None]
    if status != 0:
        for o in outs + [dg, dbt]:
            o.assert_untouched(what)
        assert bool((sc == TAIL_FILL).all()), (what, "the scratch was written by a refused call")
        return Bwd(status, None, None, None, None, None)
    for o in outs:
        o.assert_fence(owned, what)
    one = torch.ones(1, dtype=torch.bool, device="cuda")
    dg.assert_fence(one, what)
    dbt.assert_fence(one, what)
    return Bwd(status, dx.to(torch.float32).cpu(), dg.to(torch.float32).cpu().reshape(-1), dbt.to(torch.float32).cpu().reshape(-1),
               dx16.to(torch.bfloat16).cpu() if dx16 else None, [o.buf for o in outs + [dg, dbt]])


def same_bits(a, b, what):
    assert len(a.raw) == len(b.raw)
    for i, (p, q) in enumerate(zip(a.raw, b.raw)):
        assert torch.equal(p, q), (what, i, "two runs of one call differ")


def assert_finite(case, res, what):
    for (name, t), (_, r) in zip(gc.outputs(case, res), gc.outputs(case, gc.reference(case, what[1]))):
        assert bool(torch.isfinite(t.double()[~torch.isnan(r)]).all()), (what, name, "not finite: something read a fence or a row no unit owns")


def settings_of(case):
    """The case's own switches, and the three-pass switch on top where that changes the kernel."""
    three = gc.three_pass_switch(case)
    return [None] + ([three] if gc.expected_shape(case, three) != gc.expected_shape(case) else [])


# ---- 1: every case against float64, fences, the same bits twice, casts ----------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.FWD_CASES, ids=lambda c: c.id)
def test_forward_against_float64(case):
    assert gc.formats_ok(case.in_fmt, case.out_fmt, case.cast_fmt)
    for v in case.variants:
        inp, ref = gc.make_inputs(case, v), gc.reference(case, v)
        for sw in settings_of(case):
            what = (case.id, v, sw)
            got = run_forward(case, inp, sw)
            assert_finite(case, got, what)
            r = gc.worst_ratio(case, v, got, ref, case.out_fmt)
            print(f"{case.id} {v} [{gc.shape_name(gc.expected_shape(case, sw))}]: error / bar {r:.4f}")
            record(case, gc.expected_shape(case, sw), r)
            assert r <= 1.0, (what, r)
            # a clean input leaves the guard of 16-bit outputs 0; f32 outputs never touch theirs
            assert got.guard == (0 if case.out_fmt != gc.F32 else 0x5A5A), (what, got.guard)
            same_bits(got, run_forward(case, inp, sw), what)
            if case.cast_fmt:  # the casts are the casts of the f32 outputs of the same launch, bit for bit
                dt = gc.TORCH16[case.cast_fmt]
                have = ~torch.isnan(ref.y)
                assert torch.equal(got.y_cast[have].view(torch.int16), got.y.to(dt)[have].view(torch.int16)), (what, "y_cast")
                if case.y2:
                    assert torch.equal(got.y2_cast[have].view(torch.int16), got.y2.to(dt)[have].view(torch.int16)), (what, "y2_cast")


@pytest.mark.parametrize("case", gc.BWD_CASES, ids=lambda c: c.id)
def test_backward_against_float64(case):
    assert gc.bwd_formats_ok(case.in_fmt, case.dy2_fmt or gc.F32)
    for v in case.variants:
        inp, ref = gc.make_inputs(case, v), gc.reference(case, v)
        for sw in settings_of(case):
            what = (case.id, v, sw)
            got = run_backward(case, inp, sw)
            assert_finite(case, got, what)
            r = gc.worst_ratio(case, v, got, ref)
            print(f"{case.id} {v} [{gc.shape_name(gc.expected_shape(case, sw))}]: error / bar {r:.4f}")
            record(case, gc.expected_shape(case, sw), r)
            assert r <= 1.0, (what, r)
            same_bits(got, run_backward(case, inp, sw), what)
            if case.dx16:
                have = ~torch.isnan(ref.dx)
                assert torch.equal(got.dx16[have].view(torch.int16), got.dx.to(torch.bfloat16)[have].view(torch.int16)), (what, "dx16")


# ---- 2: dropout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in gc.FWD_CASES if c.dropout], ids=lambda c: c.id)
def test_forward_dropout_mask_and_scale(case):
    """The zeroed positions are the same set - the restated mask - under the case's shape and under gn_variant 0; a kept element is
    scale x the result without dropout (f32 rows out of the same kernel: the one multiplication, bit for bit)."""
    v = case.variants[0]
    inp = gc.make_inputs(case, v)
    geo = gc.geometry(case)
    keep = gc.dropout_keep(geo.rows, gc.channels(case))
    have = geo.owned[:, None].expand_as(keep)
    drops = [run_forward(case, inp, sw) for sw in (None, {"gn_variant": 0})]
    for got in drops:
        assert torch.equal((got.y.double() != 0)[have], keep[have]), (case.id, "the dropped set")
    plain = case._replace(dropout=False)
    if case.out_fmt == gc.F32 and gc.expected_shape(plain) == gc.expected_shape(case):
        base = run_forward(plain, inp)
        sel = have & keep
        assert torch.equal(drops[0].y[sel], (base.y * torch.tensor(gc.dropout_scale()))[sel]), (case.id, "kept elements are scale x the plain result")


@pytest.mark.parametrize("case", [c for c in gc.BWD_CASES if c.dropout], ids=lambda c: c.id)
def test_backward_drops_the_forward_positions(case):
    """A gradient that arrives at a position the forward zeroed counts for nothing: the same bits whatever dy holds there."""
    v = case.variants[0]
    inp = gc.make_inputs(case, v)
    geo = gc.geometry(case)
    dropped = ~gc.dropout_keep(geo.rows, gc.channels(case)) & geo.owned[:, None]
    for sw in settings_of(case):
        a = run_backward(case, inp, sw)
        b = run_backward(case, inp._replace(dy=torch.where(dropped, torch.full_like(inp.dy, 1e6), inp.dy)), sw)
        same_bits(a, b, (case.id, sw))


# ---- 3: the range guard -------------------------------------------------------------------------------------------------------------------
GUARDED = [c for c in gc.FWD_CASES if c.out_fmt in (gc.F16, gc.SP16) and not c.dropout and gc.ntok(c) * c.cg >= 16]


@pytest.mark.parametrize("case", GUARDED, ids=lambda c: c.id)
def test_one_value_past_the_limit_sets_the_guard(case):
    """One element of the largest unit's LAST token is made an outlier (x = 6e4: its normalised value is sqrt(n - 1) of the unit's n
    elements, every other one - 1 / sqrt(n - 1)) and its channel's gamma 2 x 65000 / sqrt(n - 1): that one output is 1.3e5, past
    F16_GUARD_LIMIT, every other one of the channel 1.3e5 / (n - 1).  The word must be set in every shape (a clean input left it 0 in
    test_forward_against_float64)."""
    v = case.variants[0]
    inp = gc.make_inputs(case, v)
    geo = gc.geometry(case)
    u = max(geo.units, key=lambda q: q[2])
    n = u[2] * case.cg
    row, ch = u[0] + (u[2] - 1) * u[1], gc.channels(case) - 3  # the last token, a channel of the last group
    x, gamma, beta = inp.x.clone(), inp.gamma.clone(), inp.beta.clone()
    x[row, ch] = min(6e4, 6e4 / (case.in_scale or 1.0))  # (f16 rows hold no more; 1.5e4 after the scale is an outlier all the same)
    gamma[ch], beta[ch] = 2 * gc.F16_GUARD_LIMIT / (n - 1) ** 0.5, 0.0
    assert 2 * gc.F16_GUARD_LIMIT / (n - 1) < 0.9 * gc.F16_GUARD_LIMIT
    for sw in settings_of(case):
        got = run_forward(case, inp._replace(x=x, gamma=gamma, beta=beta), sw)
        assert got.guard == 1, (case.id, sw, got.guard)


# ---- 4: statistics from the sliced forward to the three-pass backward -----------------------------------------------------------------------
SLICED_F32 = [c for c in gc.FWD_CASES if gc.expected_shape(c)[0] == gc.SLICED and c.out_fmt == gc.F32 and not c.dropout]
OTHER_F32 = [c for c in gc.FWD_CASES if gc.expected_shape(c)[0] != gc.SLICED and c.out_fmt == gc.F32 and not c.dropout][::6]


@pytest.mark.parametrize("case", SLICED_F32, ids=lambda c: c.id)
def test_sliced_forward_writes_its_statistics(case):
    for v in case.variants:
        inp, ref = gc.make_inputs(case, v), gc.reference(case, v)
        got = run_forward(case, inp, stats=True)  # (asserts *stats_written == 1 and every pair written)
        for col, name in ((0, "mean"), (1, "rstd")):
            r = gc.ratio(got.stats[:, col], ref.stats[:, col], gc.f32_bar(case, v, "y"))
            assert r <= 1.0, (case.id, v, name, r)
        # the shape switched off: neither the pairs nor the flag (asserted in run_forward)
        run_forward(case, inp, {"gn_slices": 0}, stats=True)


@pytest.mark.parametrize("case", OTHER_F32, ids=lambda c: c.id)
def test_other_shapes_leave_the_statistics_alone(case):
    run_forward(case, gc.make_inputs(case, case.variants[0]), stats=True)


def as_forward(case):
    return case._replace(direction="fwd", out_fmt=gc.F32, cast_fmt=gc.F32, y2=False, dy2_fmt=None, dx16=False, dropout=False)


THREE_BWD = [c for c in gc.BWD_CASES if gc.expected_shape(c)[0] == gc.THREE and gc.expected_shape(as_forward(c))[0] == gc.SLICED]
REG_BWD = [c for c in gc.BWD_CASES if gc.expected_shape(c)[0] != gc.THREE][::5]


@pytest.mark.parametrize("case", THREE_BWD, ids=lambda c: c.id)
def test_three_pass_backward_on_the_forward_statistics(case):
    assert THREE_BWD
    for v in case.variants:
        inp, ref = gc.make_inputs(case, v), gc.reference(case, v)
        fwd = run_forward(as_forward(case), inp, stats=True)
        got = run_backward(case, inp, stats_in=fwd.stats.cuda().contiguous())
        r = gc.worst_ratio(case, v, got, ref)
        record(case, gc.expected_shape(case), r)
        assert r <= 1.0, (case.id, v, r)


@pytest.mark.parametrize("case", REG_BWD, ids=lambda c: c.id)
def test_register_backward_ignores_the_statistics(case):
    v = case.variants[0]
    inp = gc.make_inputs(case, v)
    nan_stats = torch.full((len(gc.geometry(case).units) * case.groups, 2), float("nan"), device="cuda")
    same_bits(run_backward(case, inp), run_backward(case, inp, stats_in=nan_stats), case.id)


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------
WIDE_BWD = [c for c in gc.BWD_CASES if gc.expected_shape(c)[:3] == (gc.BLOCK, 8, 1024) and c.dy2_fmt == gc.F32]


@pytest.mark.parametrize("case", WIDE_BWD, ids=lambda c: c.id)
def test_bf16_dy2_is_refused_by_the_1024_thread_register_shape(case):
    assert not gc.bwd_reads_bf16_dy2(gc.expected_shape(case))
    inp = gc.make_inputs(case, case.variants[0])
    refused = case._replace(dy2_fmt=gc.BF16)
    run_backward(refused, inp._replace(dy2=inp.dy2.to(torch.bfloat16)), want_status=SOLA_ERR_ARG)  # (asserts that nothing was written)


@pytest.mark.parametrize("case", gc.BWD_CASES[::9], ids=lambda c: c.id)
def test_backward_scratch_one_byte_short_is_refused(case):
    run_backward(case, gc.make_inputs(case, case.variants[0]), short=1, want_status=SOLA_ERR_WORKSPACE)


def shapes_run(case):
    return {gc.expected_shape(case, sw)[:4] for sw in settings_of(case)}


def test_selections_are_not_empty():
    """What the sampled and filtered selections above must cover, whatever becomes of the case tables."""
    assert len(SLICED_F32) >= 4 and len(THREE_BWD) >= 3 and len(WIDE_BWD) >= 2 and len(GUARDED) >= 40
    # the guard: every kernel that writes 16-bit rows, in each format it writes (the h8 kernels write f16 only)
    pairs = {(k, c.out_fmt) for c in GUARDED for k in shapes_run(c)}
    want = {(k, f) for k in gc.FWD_KERNELS for f in (gc.F16, gc.SP16) if not (k[3] == 8 and f == gc.SP16)}
    assert pairs == want, pairs ^ want
    # the statistics are left alone by every forward shape but the sliced one; NaN statistics by every register shape of the backward
    assert {gc.expected_shape(c)[:4] for c in OTHER_F32} == {k for k in gc.FWD_KERNELS if k[0] != gc.SLICED and k[3] == 4}
    assert {gc.expected_shape(c)[:4] for c in REG_BWD} == {k for k in gc.BWD_KERNELS if k[0] != gc.THREE}
    assert {gc.expected_shape(c)[:4] for c in THREE_BWD} == {(gc.THREE, 0, 1024, 4)}  # (the 256-thread three-pass units have no sliced forward)
    # (the scratch size is checked by the entry point, in front of every shape: one case of each kind)
    assert {gc.expected_shape(c)[0] for c in gc.BWD_CASES[::9]} == {gc.WAVE, gc.BLOCK, gc.THREE}
