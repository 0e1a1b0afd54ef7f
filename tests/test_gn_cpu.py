"""gn_cases.py against the library and against itself, without a GPU: the restated shape ladders equal sola_group_norm_shape over a sweep of
sizes, formats and switches; refused format combinations are refused by the entry points before anything is launched; every kernel of both
launchers is the expected shape of some case; the float64 reference agrees with torch.nn.functional.group_norm and autograd; the bars are
what a float32 evaluation measures; and each mutated float64 model misses the bar on the cases written for it."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_cases as gc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import tuned  # noqa: E402

SOLA_ERR_ARG = -1
NTOKS = sorted(set(range(1, 70)) | {n + d for n in (128, 256, 512, 1024, 2048, 4096, 8192) for d in (-1, 0, 1, 2)} | {5000, 16384, 16385})
CGS = (4, 8, 16, 24, 32, 48, 64, 128, 256, 512, 1024)
SWITCH_SETS = [{}] + [{k: 0} for k in gc.SWITCHES] + [{"gn_wide": 0, "gn_slices": 0}, {"gn_h8": 0, "gn_wide": 0}]


def library_shape(direction, ntok, cg, in_fmt, out_fmt, dropout):
    out = (C.c_int * 5)()
    _lib.check(_lib.lib().sola_group_norm_shape(direction, ntok, cg, in_fmt, out_fmt, int(dropout), out), "sola_group_norm_shape")
    return tuple(out)


@pytest.mark.parametrize("sw", SWITCH_SETS, ids=lambda sw: ",".join(f"{k}={v}" for k, v in sw.items()) or "default")
def test_restated_ladders_equal_the_library(sw):
    with tuned(**sw):
        for cg in CGS:
            for ntok in NTOKS:
                assert library_shape(1, ntok, cg, gc.F32, gc.F32, False) == gc.bwd_shape(ntok, cg, sw), ("bwd", ntok, cg)
                for in_fmt in (gc.F32, gc.F16, gc.BF16):
                    for out_fmt in (gc.F32, gc.SP16, gc.F16):
                        for dropout in (False, True):
                            want = gc.fwd_shape(ntok, cg, in_fmt, out_fmt, dropout, sw)
                            assert library_shape(0, ntok, cg, in_fmt, out_fmt, dropout) == want, ("fwd", ntok, cg, in_fmt, out_fmt, dropout)
    for key, default in gc.SWITCHES.items():
        assert _lib.tune_query(key)[0] == default  # handed back


def test_ladder_edges_named_in_gn_common():
    """The static_asserts of gn_common.h, through the restatement (the sweep above holds it to the library)."""
    f, b = gc.fwd_shape, gc.bwd_shape
    wave = lambda R, cpl=4: (gc.WAVE, R, 256, cpl, 0)  # noqa: E731
    block = lambda R, nthr=256, cpl=4: (gc.BLOCK, R, nthr, cpl, 0)  # noqa: E731
    sliced = lambda S: (gc.SLICED, 32, 256, 4, S)  # noqa: E731
    three = lambda nthr=256: (gc.THREE, 0, nthr, 4, 0)  # noqa: E731
    assert [f(n, 16) for n in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)] == \
        [wave(1), wave(1), wave(2), wave(2), wave(4), wave(4), block(2), block(2), block(4), block(4), block(8), block(8), block(16), block(16),
         block(8, 1024), block(8, 1024), sliced(2)]
    assert f(1025, 16, sw={"gn_wide": 0}) == block(32) and f(2049, 16, sw={"gn_slices": 0}) == three() and f(1, 16, sw={"gn_variant": 0}) == three()
    assert [f(n, 128) for n in (2, 4, 8, 9, 32, 64, 128, 129, 256, 257)] == \
        [wave(1), wave(2), wave(4), block(2), block(4), block(8), block(16), block(8, 1024), block(8, 1024), sliced(2)]
    assert f(1, 48) == f(14, 48) == f(5000, 48) == three()
    assert f(16, 1024) == block(16) and f(32, 1024) == block(8, 1024) and f(32, 1024, sw={"gn_wide": 0}) == block(32) and f(33, 1024) == sliced(2)
    f8 = lambda n, **kw: f(n, 128, gc.F16, gc.F16, **kw)  # noqa: E731
    assert [f8(n) for n in (4, 8, 32, 64, 65, 256, 257)] == \
        [wave(1, 8), wave(2, 8), block(2, 256, 8), block(4, 256, 8), block(4, 1024, 8), block(4, 1024, 8), sliced(2)]
    assert [f8(n, sw={"gn_h8": 0}) for n in (4, 8, 32, 64, 65, 256)] == [wave(2), wave(4), block(4), block(8), block(16), block(8, 1024)]
    assert f8(4, dropout=True) == wave(2) and f(4, 128, gc.F32, gc.F16) == wave(2) and f(4, 128, gc.BF16, gc.F16) == wave(2)
    assert [b(n, 16) for n in (16, 32, 64, 65, 128, 256, 512, 513, 1024, 1025, 2048, 2049)] == \
        [wave(1), wave(2), wave(4), block(2), block(2), block(4), block(8), block(8, 512), block(8, 512), block(8, 1024), block(8, 1024), three(1024)]
    assert not gc.bwd_reads_bf16_dy2(b(1025, 16)) and gc.bwd_reads_bf16_dy2(b(1024, 16)) and gc.bwd_reads_bf16_dy2(b(2049, 16))
    assert b(16, 16, {"gn_bwd_reg": 0}) == three() and b(1, 48) == b(5000, 24) == three()


def _dummy():
    buf = (C.c_float * 4096)()  # as large as any size a call below states
    return C.cast(buf, C.c_void_p), buf


def test_refused_formats_are_refused_before_any_launch():
    """group_norm_formats_ok / group_norm_bwd_formats_ok and the bfloat16-dy2 rule as restated: a call the restatement refuses comes back
    with SOLA_ERR_ARG from the argument checks, which run before the device is touched - launch_group_norm and launch_group_norm_bwd state
    that order beside their checks (the accepted combinations run in test_gpu_gn.py)."""
    L = _lib.lib()
    p, keep = _dummy()
    refused = 0
    for in_fmt in range(4):
        for out_fmt in range(4):
            for cast_fmt in range(4):
                if gc.formats_ok(in_fmt, out_fmt, cast_fmt):
                    continue
                rc = L.sola_group_norm_ex(p, p, None, None, p, p, 1, 1, 1, 0, 1, 1, 8, 1, 1e-5, 0.01, 0, in_fmt, out_fmt, None, None, None,
                                          p if cast_fmt else None, None, cast_fmt, None, 0, None, None, None)
                assert rc == SOLA_ERR_ARG and b"no kernel for" in L.sola_last_error(), (in_fmt, out_fmt, cast_fmt, L.sola_last_error())
                refused += 1
    assert refused == 4 * 4 * 4 - sum(gc.formats_ok(i, o, c) for i in range(4) for o in range(4) for c in range(4)) and refused > 30
    for x_fmt in range(4):
        for dy2_fmt in range(4):
            if gc.bwd_formats_ok(x_fmt, dy2_fmt):
                continue
            rc = L.sola_group_norm_backward_ex(p, p, p, p, p, p, p, p, 1, 1, 1, 0, 1, 1, 8, 1, 1e-5, 0.01, 0, None, x_fmt, dy2_fmt, None, None, p, 64, None)
            assert rc == SOLA_ERR_ARG and b"f32 or bfloat16 rows" in L.sola_last_error(), (x_fmt, dy2_fmt)
    for ntok, cg in ((1025, 16), (2048, 16), (200, 128), (17, 1024), (32, 1024)):  # the 1024-thread register shape
        assert not gc.bwd_reads_bf16_dy2(gc.bwd_shape(ntok, cg))
        rc = L.sola_group_norm_backward_ex(p, p, p, p, p, p, p, p, 1, 1, ntok, 0, 1, ntok, cg, 1, 1e-5, 0.01, 0, None, gc.F32, gc.BF16, None, None,
                                           p, 8 * cg, None)
        assert rc == SOLA_ERR_ARG and b"bfloat16 dy2" in L.sola_last_error(), (ntok, cg)
    del keep


def test_every_kernel_is_the_expected_shape_of_a_case():
    fwd = {gc.expected_shape(c)[:4] for c in gc.FWD_CASES} | {gc.expected_shape(c, gc.three_pass_switch(c))[:4] for c in gc.FWD_CASES}
    bwd = {gc.expected_shape(c)[:4] for c in gc.BWD_CASES} | {gc.expected_shape(c, gc.three_pass_switch(c))[:4] for c in gc.BWD_CASES}
    assert fwd == gc.FWD_KERNELS, fwd ^ gc.FWD_KERNELS
    assert bwd == gc.BWD_KERNELS, bwd ^ gc.BWD_KERNELS
    # ... the h8 kernel's five, and each unit again leaving it: switched off, with dropout, with f32 and with bfloat16 rows in
    h8 = [c for c in gc.FWD_CASES if gc.expected_shape(c)[3] == 8]
    assert {gc.expected_shape(c)[:3] for c in h8} == {k[:3] for k in gc.FWD_KERNELS if k[3] == 8}
    for c in gc.FWD_CASES:
        if c.out_fmt == gc.F16 and (c.in_fmt != gc.F16 or c.dropout or dict(c.switches).get("gn_h8") == 0):
            assert gc.expected_shape(c)[3] == 4, c.id
    leaves = lambda pred: {gc.ntok(c) for c in gc.FWD_CASES if c.cg == 128 and c.out_fmt == gc.F16 and pred(c)}  # noqa: E731
    for pred in (lambda c: c.in_fmt == gc.F16 and dict(c.switches).get("gn_h8") == 0, lambda c: c.in_fmt == gc.F16 and c.dropout,
                 lambda c: c.in_fmt == gc.F32, lambda c: c.in_fmt == gc.BF16):
        assert set(gc.H8_LEAVES) <= leaves(pred)
    # ... sliced units of 2, 3 and 4 slices, one with a one-token last slice, and units of fewer slices than the launch's S beside them
    sliced = [c for c in gc.FWD_CASES if gc.expected_shape(c)[0] == gc.SLICED]
    assert {gc.expected_shape(c)[4] for c in sliced} >= {2, 3, 4}
    assert any(c.cg == 1024 and gc.ntok(c) == 33 for c in sliced) and any(c.layout == "units" for c in sliced)
    # ... wave shapes with a partly empty last block, every group count, every layout
    for cases in (gc.FWD_CASES, gc.BWD_CASES):
        wave_units = {len(gc.geometry(c).units) * c.groups for c in cases if gc.expected_shape(c)[0] == gc.WAVE}
        assert {1, 3, 5, 6} <= wave_units
        assert {c.groups for c in cases} == {1, 2, 3, 8} and {c.layout for c in cases} == set(gc.LAYOUTS)
    assert any(c.layout == "strided" and c.y2 and c.n_inst > c.inner for c in gc.FWD_CASES)


def test_geometry_of_the_three_layouts():
    for c in gc.CASES:
        geo = gc.geometry(c)
        n_inst, inner, outer_stride, inner_stride, tok_stride, ntok = geo.args
        assert n_inst == len(geo.units) and ntok == max(u[2] for u in geo.units)
        if c.layout != "units":  # the entry point's own addressing
            for i, (r0, st, n, pe_row) in enumerate(geo.units):
                assert (r0, st, n, pe_row) == ((i // inner) * outer_stride + (i % inner) * inner_stride, tok_stride, ntok, i % inner)
            assert bool(geo.owned.all())
        else:
            assert not bool(geo.owned.all()) and 1 in {u[2] for u in geo.units}  # rows that belong to no unit; a one-token unit
            assert len({u[2] for u in geo.units}) > 1 or ntok == 1
            assert any(u[3] != i % inner for i, u in enumerate(geo.units)) and {u[1] for u in geo.units} == {1, 2}


ROWS_CASES = [c for c in gc.CASES if c.layout == "rows" and not c.dropout][::3]


@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: c.id)
def test_reference_agrees_with_torch_group_norm(case):
    F = torch.nn.functional
    v = case.variants[0]
    inp, ref = gc.make_inputs(case, v), gc.reference(case, v)
    t, Cn = case.toks[0], gc.channels(case)
    x = gc.x64_of(case, inp).reshape(case.n_inst, t, Cn).transpose(1, 2).clone().requires_grad_(True)  # [instances, C, tokens]
    gamma, beta = inp.gamma.double().requires_grad_(True), inp.beta.double().requires_grad_(True)
    y = F.group_norm(x, case.groups, gamma, beta, gc.EPS)
    if case.leaky:
        y = F.leaky_relu(y, gc.SLOPE)
    back = lambda z: z.transpose(1, 2).reshape(case.n_inst * t, Cn)  # noqa: E731
    if case.direction == "fwd":
        assert gc.rel_error(back(y.detach()), ref.y) < 1e-12
        if case.y2:
            assert gc.rel_error(back(y.detach()) + inp.pe.double()[0], ref.y2) < 1e-12
        return
    dy = inp.dy.double() + (inp.dy2.double() if inp.dy2 is not None else 0.0)
    y.backward(dy.reshape(case.n_inst, t, Cn).transpose(1, 2))
    assert gc.rel_error(back(x.grad), ref.dx) < 1e-11
    assert gc.rel_error(gamma.grad, ref.dgamma) < 1e-11 and gc.rel_error(beta.grad, ref.dbeta) < 1e-11


def test_written_out_model_is_the_reference():
    """model64 without a mutation - the forward and the backward's formulas by hand - equals the oracle-and-autograd reference: what a
    mutant differs by is its mutation."""
    for c in gc.CASES:
        for v in c.variants:
            ref, got = gc.reference(c, v), gc.model64(c, v)
            for (name, g), (_, r) in zip(gc.outputs(c, got), gc.outputs(c, ref)):
                assert torch.equal(torch.isnan(g), torch.isnan(r)), (c.id, v, name)
                assert gc.rel_error(g, r) < 1e-11, (c.id, v, name)


def test_dropout_restatement():
    keep = gc.dropout_keep(512, 256)
    assert abs(float(keep.float().mean()) - (1 - gc.DROP_P)) < 0.01 and abs(gc.dropout_scale() - 1 / (1 - gc.DROP_P)) < 1e-6
    assert torch.equal(keep[:100], gc.dropout_keep(100, 256))  # a function of the element offset alone


def test_bars_are_eight_times_the_float32_restatement():
    worst = {k: 0.0 for k in gc.F32_MEASURED}
    for c in gc.CASES:
        for v in c.variants:
            ref, got = gc.reference(c, v), gc.model32(c, v)
            worst[(c.direction, v)] = max([worst[(c.direction, v)]] + [gc.rel_error(g, r) for (_, g), (_, r) in zip(gc.outputs(c, got), gc.outputs(c, ref))])
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for k, stated in gc.F32_MEASURED.items():
        # (numpy's pairwise sums differ a little between builds; the stated value is the measured one rounded up)
        assert 0.7 * stated <= worst[k] <= stated * 1.02, (k, worst[k], stated)
        assert gc.F32_BAR[k] == 8.0 * stated
    # what a variance over n - 1 needs: at units of 16k elements and more the bar of every per-unit output, in both directions and on every
    # variant, is under 1.2e-5 - and never under what the float32 evaluation itself reaches at those sizes
    assert gc.LARGE_UNIT_BAR < 1.2e-5
    large = [c for c in gc.CASES if gc.largest_unit(c) >= gc.LARGE_UNIT]
    assert {c.direction for c in large} == {"fwd", "bwd"} and {v for c in large for v in c.variants} == set(gc.VARIANTS)
    for c in large:
        for v in c.variants:
            ref, got = gc.reference(c, v), gc.model32(c, v)
            for (name, g), (_, r) in zip(gc.outputs(c, got), gc.outputs(c, ref)):
                if name in gc.PER_UNIT_OUTPUTS:
                    assert gc.f32_bar(c, v, name) < 1.2e-5, (c.id, v, name)
                    assert gc.rel_error(g, r) < 0.5 * gc.f32_bar(c, v, name), (c.id, v, name, gc.rel_error(g, r))
                else:
                    assert gc.f32_bar(c, v, name) == gc.F32_BAR[(c.direction, v)]
    for c in gc.CASES:  # the cap only ever narrows
        for v in c.variants:
            assert all(gc.f32_bar(c, v, name) <= gc.F32_BAR[(c.direction, v)] for name, _ in gc.outputs(c, gc.reference(c, v)))


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
def plain_f32(c):
    return c.in_fmt == gc.F32 and c.out_fmt == gc.F32 and not c.dropout


def mutant_cases(mutant):
    if mutant == "var_n_minus_1":
        # Units of 16k elements and more, on every variant.  The mutant moves a unit of n elements by 1 / 2n of its largest normalised
        # entries; it is held to miss the bar wherever that is 1.25 x the bar or more (the largest output entry need not be the largest
        # normalised one).  Under the cap that is every unit up to 33k elements on every variant.  Beyond - the 38k, 66k and 99k units - 1 / 2n
        # (1.3e-5 .. 5e-6) is under 8 x the float32 evaluation's own error on "offset" (1.7e-5 at these sizes): no bar with that margin sees
        # it there, the "wide" bar (1.9e-6) does at every size, and every large case is held on at least one variant (asserted below).
        large = [c for c in gc.FWD_CASES if plain_f32(c) and gc.largest_unit(c) >= gc.LARGE_UNIT]
        picked = [(c, v) for c in large for v in c.variants if 1.0 / (2 * gc.largest_unit(c)) >= 1.25 * gc.f32_bar(c, v, "y")]
        assert {c for c, _ in picked} == set(large) and sum(v == "offset" for _, v in picked) >= 8
        assert all((c, v) in picked for c in large for v in c.variants if gc.largest_unit(c) <= 33000)
        return picked
    if mutant == "eps_outside_sqrt":
        return [(c, "tight") for c in gc.FWD_CASES if "tight" in c.variants]
    if mutant == "last_slice_full":
        return [(c, v) for c in gc.FWD_CASES if plain_f32(c) and gc.expected_shape(c)[0] == gc.SLICED and
                gc.ntok(c) % (256 // (c.cg // 4) * gc.GN_SLICE_R) for v in c.variants]
    if mutant == "pe_row_inst":
        return [(c, v) for c in gc.FWD_CASES if plain_f32(c) and c.y2 and (c.layout == "units" or (c.layout == "strided" and c.n_inst > c.inner))
                for v in c.variants]
    if mutant == "last_token_dropped":
        return [(c, v) for c in gc.FWD_CASES if plain_f32(c) and gc.ntok(c) > 1 for v in c.variants]
    if mutant == "leaky_on_x":
        return [(c, v) for c in gc.BWD_CASES if c.leaky for v in c.variants]
    assert mutant == "no_dy2"
    return [(c, v) for c in gc.BWD_CASES if c.dy2_fmt is not None for v in c.variants]


@pytest.mark.parametrize("mutant", gc.FWD_MUTANTS + gc.BWD_MUTANTS)
def test_mutant_misses_the_bar(mutant):
    cases = mutant_cases(mutant)
    assert len(cases) >= 3, mutant
    for c, v in cases:
        ref, got = gc.reference(c, v), gc.model64(c, v, mutant)
        assert gc.worst_ratio(c, v, got, ref) > 1.0, (mutant, c.id, v, gc.worst_ratio(c, v, got, ref))
