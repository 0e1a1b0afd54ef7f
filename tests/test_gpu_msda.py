"""sola_ms_deform_attn on the GPU against the float64 restatement of its contract (msda_cases.py, pinned against the public
grid_sample statement in test_msda_cpu.py): parity inside a derived bound, the kernel's error next to the float32 statement's,
the exact properties, the guard against a level table that points outside value, and the GroundingDINO extension stand-in."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msda_cases as mc  # noqa: E402
from sola_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs on the CPU, float64 restatement) of a case: computed once, shared, never modified."""
    inputs = mc.make_case(case)
    return inputs, mc.restatement(*inputs, dtype=torch.float64)


def run(value, shapes, start, loc, w):
    return ops.ms_deform_attn(value.cuda(), shapes.cuda(), start.cuda(), loc.cuda(), w.cuda())


def assert_parity(out, out64, value, shapes, w, what):
    N, Lq = out64.shape[:2]
    M = w.shape[2]
    err = (out.double().cpu() - out64).abs().reshape(N, Lq, M, -1)
    bound = mc.parity_bound(value, shapes, w)
    worst = float((err / bound).max())
    print(f"{what}: max |out - out64| = {float(err.max()):.3e}, at most {worst:.3f} of its bound ({float(bound.max()):.3e})")
    assert worst <= 1.0, (what, worst)
    return float(err.max())


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_parity_against_the_float64_restatement(case):
    (value, shapes, start, loc, w), out64 = reference(case)
    out = run(value, shapes, start, loc, w)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == tuple(out64.shape)
    e_hip = assert_parity(out, out64, value, shapes, w, mc.case_id(case))
    e_torch = float((mc.statement(value, shapes, start, loc, w, torch.float32).double() - out64).abs().max())
    print(f"{mc.case_id(case)}: E_hip {e_hip:.3e}  E_torch(f32 grid_sample statement, CPU) {e_torch:.3e}  ratio {e_hip / e_torch:.2f}")


def test_any_p_kernel_on_misaligned_weights_gives_the_same_bits():
    """P = 4 with weights that are not 16-byte aligned take the any-P kernel: same arithmetic, same order."""
    (value, shapes, start, loc, w), out64 = reference(mc.SMALL)
    want = run(value, shapes, start, loc, w)
    buf = torch.zeros(w.numel() + 1, device="cuda")
    buf[1:] = w.flatten().cuda()
    w_off = buf[1:].view(w.shape)
    assert w_off.data_ptr() % 16 == 4 and w_off.is_contiguous()
    got = ops.ms_deform_attn(value.cuda(), shapes.cuda(), start.cuda(), loc.cuda(), w_off)
    assert torch.equal(got, want)


def test_error_next_to_the_float32_statement_on_the_decoder_shape():
    """900 queries: E_hip = max |out - out64| against E_torch = the same error of the public statement in float32, on the same
    inputs on the device.  E_hip <= 2 E_torch: the summation order over the 16 samples differs, nothing else may."""
    (value, shapes, start, loc, w), out64 = reference(mc.DECODER)
    e_hip = float((run(value, shapes, start, loc, w).double().cpu() - out64).abs().max())
    stmt = mc.statement(value.cuda(), shapes, start, loc.cuda(), w.cuda(), torch.float32)
    e_torch = float((stmt.double().cpu() - out64).abs().max())
    print(f"decoder shape: E_hip {e_hip:.3e}  E_torch {e_torch:.3e}  ratio {e_hip / e_torch:.3f}")
    assert e_hip <= 2 * e_torch, (e_hip, e_torch)


def test_locations_outside_every_map_give_exact_zeros():
    (value, shapes, start, loc, w), _ = reference(mc.SMALL)
    g = torch.Generator().manual_seed(5)
    # every sample at least one pixel outside on one axis (the smallest map is 1 x 1: a pixel is the whole range), on all four sides
    far = torch.rand(loc.shape, generator=g) * 3 + 1.6
    far = torch.where(torch.rand(loc.shape, generator=g) < 0.5, far, -far + 1)
    keep_one_inside = torch.rand(loc.shape[:-1], generator=g) < 0.5
    far[..., 1] = torch.where(keep_one_inside, loc[..., 1].clamp(0, 1), far[..., 1])
    out = run(value, shapes, start, far, w)
    assert torch.equal(out, torch.zeros_like(out))


def test_pixel_centres_with_one_hot_weights_return_the_value_row_bit_for_bit():
    N, M, D, L, P = 2, 3, 32, 2, 4
    shapes, start, S = mc.level_tables([(8, 8), (8, 8)])
    g = torch.Generator().manual_seed(7)
    value = torch.randn(N, S, M, D, generator=g)
    Lq = 64
    ys, xs = torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")
    centre = torch.stack([(xs.flatten() + 0.5) / 8, (ys.flatten() + 0.5) / 8], -1)  # query q addresses pixel (q // 8, q % 8)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15
    w = torch.zeros(N, Lq, M, L, P)
    want = torch.empty(N, Lq, M, D)
    for n in range(N):
        for m in range(M):
            hot_l, hot_p = (n + m) % L, (n + 2 * m) % P
            loc[n, :, m, hot_l, hot_p] = centre
            w[n, :, m, hot_l, hot_p] = 1
            want[n, :, m] = value[n, int(start[hot_l]):int(start[hot_l]) + 64, m]
    out = run(value, shapes, start, loc, w)
    assert torch.equal(out.cpu(), want.reshape(N, Lq, M * D))


def test_identical_bits_on_any_stream_and_every_element_written():
    (value, shapes, start, loc, w), _ = reference(mc.CASES[2])
    dev = [t.cuda() for t in (value, shapes, start, loc, w)]
    a = ops.ms_deform_attn(*dev)
    b = ops.ms_deform_attn(*dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.ms_deform_attn(*dev)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, b) and torch.equal(a, c)
    # the output over a buffer that held NaN: every element is written (the allocator hands the freed block back)
    N, Lq, MD = a.shape
    from sola_amd import _lib
    out = torch.full((N, Lq, MD), float("nan"), device="cuda")
    L, P = loc.shape[3], loc.shape[4]
    _lib.check(_lib.lib().sola_ms_deform_attn(_lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), _lib.ptr(dev[4]), N,
                                              value.shape[1], value.shape[2], value.shape[3], Lq, L, P, _lib.ptr(out),
                                              _lib.current_stream(out.device)), "sola_ms_deform_attn")
    assert not torch.isnan(out).any() and torch.equal(out, a)


def test_a_table_that_points_outside_value_reads_nothing_there():
    """value is S rows inside a larger ALLOCATED buffer whose other rows, before and after, hold 1e30.  The table describes maps that run
    into those rows, start before row 0, or are empty: rows outside [0, S) are absent, nothing of the 1e30 shows."""
    N, Lq, M, D, P = 1, 130, 8, 32, 4
    S, before, after = 60, 100, 400
    g = torch.Generator().manual_seed(11)
    big = torch.full((N, before + S + after, M, D), 1e30)
    big[:, before:before + S] = torch.randn(N, S, M, D, generator=g)
    #                 runs 40 rows past S   starts before row 0   empty      far past S (every row absent)
    shapes = torch.tensor([[10, 10], [6, 8], [0, 5], [4, 4]], dtype=torch.int64)
    start = torch.tensor([0, -20, 10, S + 100], dtype=torch.int64)
    # nothing the table addresses lies outside the allocation
    assert int(start[3]) + 16 <= S + after and int(shapes[0].prod()) <= S + after and -int(start[1]) <= before
    L = 4
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15
    w = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).reshape(N, Lq, M, L, P)
    big_dev = big.cuda()
    value_dev = big_dev[:, before:before + S]
    assert value_dev.is_contiguous() and value_dev.data_ptr() == big_dev.data_ptr() + before * M * D * 4
    out = ops.ms_deform_attn(value_dev, shapes.cuda(), start.cuda(), loc.cuda(), w.cuda())
    assert float(out.abs().max()) < 1e3
    value = big[:, before:before + S].contiguous()
    out64 = mc.restatement(value, shapes, start, loc, w, torch.float64, rows=S)
    assert float(out64.abs().max()) > 0.1  # the rows that are there do count
    assert_parity(out, out64, value, shapes, w, "guarded table")


def test_the_extension_stand_in_equals_the_operator():
    (value, shapes, start, loc, w), _ = reference(mc.SMALL)
    assert value.shape[0] == 2
    dev = [t.cuda() for t in (value, shapes, start, loc, w)]
    assert torch.equal(ops.gdino_ext.ms_deform_attn_forward(*dev, 64), ops.ms_deform_attn(*dev))
