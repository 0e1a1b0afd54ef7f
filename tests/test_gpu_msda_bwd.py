"""sola_ms_deform_attn_backward on the GPU against float64 autograd through the restatement of the forward's contract
(msda_bwd_cases.py, pinned and calibrated in test_msda_bwd_cpu.py): parity of the three gradients inside derived bounds, what is
bit-repeatable and what is not, every requested element written, the guard against a level table that points outside value,
autograd through ops.ms_deform_attn, and the error next to torch's own float32 backward on the decoder shape."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msda_bwd_cases as bc  # noqa: E402
import msda_cases as mc  # noqa: E402
from sola_amd import _lib, ops  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("grad_value", "grad_loc", "grad_weight")


def run(value, shapes, start, loc, w, grad_out, need=(True, True, True)):
    return ops.ms_deform_attn_backward(value.cuda(), shapes.cuda(), start.cuda(), loc.cuda(), w.cuda(), grad_out.cuda(), need)


def assert_inside_bounds(got, want, inputs, grad_out, what, rows=None):
    ratios, excluded = bc.worst_ratios(got, want, *inputs, grad_out, rows=rows)
    print(f"{what}: worst err / bound  grad_value {ratios[0]:.4f}  grad_loc {ratios[1]:.4f}  grad_weight {ratios[2]:.4f}; "
          f"{100 * excluded:.3f} % of the samples near a cell border")
    assert max(ratios) <= 1.0, (what, ratios)
    assert excluded <= bc.MAX_EXCLUDED, (what, excluded)


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_parity_of_the_three_gradients_against_float64(case):
    inputs, grad_out, want = bc.grad_reference(case)
    got = run(*inputs, grad_out)
    for g, ref in zip(got, want):
        assert g.dtype == torch.float32 and g.is_cuda and g.shape == ref.shape
    assert_inside_bounds(got, want, inputs, grad_out, mc.case_id(case))


def test_grad_loc_and_grad_weight_have_identical_bits_on_any_stream():
    inputs, grad_out, want = bc.grad_reference(mc.CASES[2])
    dev = [t.cuda() for t in (*inputs, grad_out)]
    a = ops.ms_deform_attn_backward(*dev)
    b = ops.ms_deform_attn_backward(*dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.ms_deform_attn_backward(*dev)
    torch.cuda.current_stream().wait_stream(side)
    for other in (b, c):
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
    # grad_value: float atomic adds, the order is the hardware's - inside its bound every time, equal bits not required
    for i, got in enumerate((a, b, c)):
        assert_inside_bounds(got, want, inputs, grad_out, f"run {i}")


def c_entry(value, shapes, start, loc, w, grad_out, grad_value, grad_loc, grad_weight):
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    p = _lib.ptr
    _lib.check(_lib.lib().sola_ms_deform_attn_backward(p(value), p(shapes), p(start), p(loc), p(w), p(grad_out), N, S, M, D, Lq, L, P,
                                                       p(grad_value), p(grad_loc), p(grad_weight), _lib.current_stream(value.device)),
               "sola_ms_deform_attn_backward")


def test_every_requested_element_is_written():
    """The C entry on NaN-filled outputs, every location outside every map: exact zeros everywhere (grad_value by the entry's own
    memset, the other two stored by the kernel)."""
    (value, shapes, start, loc, w), grad_out, _ = bc.grad_reference(mc.SMALL)
    g = torch.Generator().manual_seed(5)
    far = torch.rand(loc.shape, generator=g) * 3 + 1.6  # at least one pixel outside on both axes, on all four sides
    far = torch.where(torch.rand(loc.shape, generator=g) < 0.5, far, -far + 1)
    dev = [t.cuda() for t in (value, shapes, start, far, w, grad_out)]
    outs = [torch.full(t.shape, float("nan"), device="cuda") for t in (value, loc, w)]
    c_entry(*dev, *outs)
    for name, out in zip(NAMES, outs):
        assert torch.equal(out, torch.zeros_like(out)), name


def test_need_subsets_leave_out_what_is_not_wanted():
    inputs, grad_out, want = bc.grad_reference(mc.SMALL)
    full = run(*inputs, grad_out)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, False, True), (True, True, False)):
        got = run(*inputs, grad_out, need)
        for i in range(3):
            assert (got[i] is not None) == need[i], (need, NAMES[i])
        for i in (1, 2):
            if need[i]:
                assert torch.equal(got[i], full[i]), (need, NAMES[i])
        assert_inside_bounds(got, want, inputs, grad_out, f"need {need}")


def test_pixel_centres_with_one_hot_weights_scatter_the_grad_out_row_bit_for_bit():
    """Each query on its own pixel, coefficient exactly 1, weight exactly 1: one add of the grad_out row into a zeroed row."""
    N, M, D, L, P = 2, 3, 32, 2, 4
    shapes, start, S = mc.level_tables([(8, 8), (8, 8)])
    g = torch.Generator().manual_seed(7)
    value = torch.randn(N, S, M, D, generator=g)
    Lq = 64
    ys, xs = torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")
    centre = torch.stack([(xs.flatten() + 0.5) / 8, (ys.flatten() + 0.5) / 8], -1)  # query q addresses pixel (q // 8, q % 8)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15
    w = torch.zeros(N, Lq, M, L, P)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    want = torch.zeros(N, S, M, D)
    for n in range(N):
        for m in range(M):
            hot_l, hot_p = (n + m) % L, (n + 2 * m) % P
            loc[n, :, m, hot_l, hot_p] = centre
            w[n, :, m, hot_l, hot_p] = 1
            want[n, int(start[hot_l]):int(start[hot_l]) + 64, m] = grad_out.view(N, Lq, M, D)[n, :, m]
    grad_value = run(value, shapes, start, loc, w, grad_out, (True, False, False))[0]
    assert torch.equal(grad_value.cpu(), want)


def test_adds_from_different_blocks_meet_in_one_cell():
    """D = 32: a block holds 8 queries of a head; 17 queries (two blocks and one more) all sample the same cell of a 4 x 4 map."""
    N, M, D, P, Lq = 1, 2, 32, 2, 2 * (256 // 32) + 1
    shapes, start, S = mc.level_tables([(4, 4)])
    g = torch.Generator().manual_seed(13)
    value = torch.randn(N, S, M, D, generator=g)
    px = torch.rand(N, Lq, M, 1, P, 2, generator=g) * 0.6 + 1.2  # pixel coordinates in (1.2, 1.8): the cell of corners 1 and 2
    loc = (px + 0.5) / 4
    w = torch.softmax(torch.randn(N, Lq, M, P, generator=g), -1).reshape(N, Lq, M, 1, P)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    inputs = (value, shapes, start, loc, w)
    want = bc.autograd_grads(mc.restatement, *inputs, grad_out, torch.float64)
    hit = want[0].abs().sum((0, 2, 3)) > 0
    assert hit.nonzero().flatten().tolist() == [5, 6, 9, 10]
    assert_inside_bounds(run(*inputs, grad_out), want, inputs, grad_out, "17 queries on one cell")


def test_any_number_of_points_and_misaligned_weights():
    """One kernel serves every P (CASES[2] has P = 3) and needs 4-byte alignment of the weights only: weights one float off a
    16-byte boundary give the bits of the aligned call."""
    inputs, grad_out, want = bc.grad_reference(mc.CASES[2])
    assert inputs[3].shape[4] == 3
    full = run(*inputs, grad_out)
    assert_inside_bounds(full, want, inputs, grad_out, "P = 3")
    value, shapes, start, loc, w = inputs
    buf = torch.zeros(w.numel() + 1, device="cuda")
    buf[1:] = w.flatten().cuda()
    w_off = buf[1:].view(w.shape)
    assert w_off.data_ptr() % 16 == 4 and w_off.is_contiguous()
    got = ops.ms_deform_attn_backward(value.cuda(), shapes.cuda(), start.cuda(), loc.cuda(), w_off, grad_out.cuda())
    assert torch.equal(got[1], full[1]) and torch.equal(got[2], full[2])
    assert_inside_bounds(got, want, inputs, grad_out, "P = 3, weights off by 4 bytes")


def test_a_table_that_points_outside_value_writes_nothing_there():
    """value and grad_value are S rows inside larger ALLOCATED buffers whose other rows, before and after, hold sentinels.  The table
    describes maps that run into those rows, start before row 0, or are empty: rows outside [0, S) are absent - nothing is read
    from value's sentinels (1e30 would show), nothing is added to grad_value's."""
    N, Lq, M, D, P = 1, 130, 8, 32, 4
    S, before, after = 60, 100, 400
    g = torch.Generator().manual_seed(11)
    big = torch.full((N, before + S + after, M, D), 1e30)
    big[:, before:before + S] = torch.randn(N, S, M, D, generator=g)
    #                 runs 40 rows past S   starts before row 0   empty      far past S (every row absent)
    shapes = torch.tensor([[10, 10], [6, 8], [0, 5], [4, 4]], dtype=torch.int64)
    start = torch.tensor([0, -20, 10, S + 100], dtype=torch.int64)
    # nothing the table addresses lies outside the allocations
    assert int(start[3]) + 16 <= S + after and int(shapes[0].prod()) <= S + after and -int(start[1]) <= before
    L = 4
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15
    w = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).reshape(N, Lq, M, L, P)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    big_dev = big.cuda()
    value_dev = big_dev[:, before:before + S]
    sentinel = 12345.0
    big_grad = torch.full((N, before + S + after, M, D), sentinel, device="cuda")
    grad_value = big_grad[:, before:before + S]
    assert value_dev.is_contiguous() and grad_value.is_contiguous() and grad_value.data_ptr() == big_grad.data_ptr() + before * M * D * 4
    grad_loc, grad_weight = torch.empty(loc.shape, device="cuda"), torch.empty(w.shape, device="cuda")
    c_entry(value_dev, shapes.cuda(), start.cuda(), loc.cuda(), w.cuda(), grad_out.cuda(), grad_value, grad_loc, grad_weight)
    assert bool((big_grad[:, :before] == sentinel).all()) and bool((big_grad[:, before + S:] == sentinel).all())
    inputs = (big[:, before:before + S].contiguous(), shapes, start, loc, w)
    want = bc.autograd_grads(mc.restatement, *inputs, grad_out, torch.float64, rows=S)
    assert min(float(t.abs().max()) for t in want) > 0.1  # the rows that are there do count
    assert float(grad_loc.abs().max()) < 1e6 and float(grad_weight.abs().max()) < 1e6
    assert_inside_bounds((grad_value, grad_loc, grad_weight), want, inputs, grad_out, "guarded table", rows=S)


def test_autograd_through_the_operator_and_the_training_stand_in():
    inputs, grad_out, want = bc.grad_reference(mc.SMALL)
    value, shapes, start, loc, w = (t.cuda() for t in inputs)
    g = grad_out.cuda()
    direct = ops.ms_deform_attn_backward(value, shapes, start, loc, w, g)
    plain = ops.ms_deform_attn(value, shapes, start, loc, w)
    assert not plain.requires_grad and plain.grad_fn is None
    leaves = [t.clone().requires_grad_(True) for t in (value, loc, w)]
    out = ops.ms_deform_attn(leaves[0], shapes, start, leaves[1], leaves[2])
    assert out.requires_grad and torch.equal(out.detach(), plain)
    out.backward(g)
    assert torch.equal(leaves[1].grad, direct[1]) and torch.equal(leaves[2].grad, direct[2])
    assert_inside_bounds(tuple(t.grad for t in leaves), want, inputs, grad_out, "autograd")
    # only what requires grad is computed
    only_w = w.clone().requires_grad_(True)
    ops.ms_deform_attn(value, shapes, start, loc, only_w).backward(g)
    assert torch.equal(only_w.grad, direct[2])
    # no graph under no_grad, and today's bits
    with torch.no_grad():
        quiet = ops.ms_deform_attn(leaves[0], shapes, start, leaves[1], leaves[2])
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, plain)
    # the training stand-in: upstream's argument order, im2col_step ignored
    ext = ops.gdino_train_ext.ms_deform_attn_backward(value, shapes, start, loc, w, g, 64)
    assert torch.equal(ext[1], direct[1]) and torch.equal(ext[2], direct[2])
    assert_inside_bounds(ext, want, inputs, grad_out, "gdino_train_ext")
    assert torch.equal(ops.gdino_train_ext.ms_deform_attn_forward(value, shapes, start, loc, w, 64), plain)


def test_deterministic_algorithms_refuse_grad_value():
    inputs, grad_out, _ = bc.grad_reference(mc.SMALL)
    dev = [t.cuda() for t in (*inputs, grad_out)]
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(SolaError, match="not bit-repeatable"):
            ops.ms_deform_attn_backward(*dev)
        got = ops.ms_deform_attn_backward(*dev, need=(False, True, True))  # the repeatable two are served
        assert got[0] is None and got[1] is not None and got[2] is not None
        torch.use_deterministic_algorithms(True, warn_only=True)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = ops.ms_deform_attn_backward(*dev)
        assert got[0] is not None and any("not bit-repeatable" in str(x.message) for x in seen)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


def test_error_next_to_torch_float32_autograd_on_the_decoder_shape():
    """900 queries: E_hip = max |hip - f64| of each gradient against E_torch, the same error of float32 torch autograd through the
    grid_sample statement on the device; grad_loc over the samples that are not near a cell border, both sides.  E_hip <= 2 E_torch:
    the order of the sums differs, nothing else may."""
    inputs, grad_out, want = bc.grad_reference(mc.DECODER)
    value, shapes, start, loc, w = inputs
    hip = run(*inputs, grad_out)
    stmt = bc.autograd_grads(mc.statement, value.cuda(), shapes, start, loc.cuda(), w.cuda(), grad_out.cuda(), torch.float32)
    keep = ~bc.near_border(loc, shapes)

    def err(got, i):
        e = (got[i].double().cpu() - want[i]).abs()
        return float(e[keep].max()) if i == 1 else float(e.max())

    worst = []
    for i, name in enumerate(NAMES):
        e_hip, e_torch = err(hip, i), err(stmt, i)
        print(f"decoder shape {name}: E_hip {e_hip:.3e}  E_torch {e_torch:.3e}  ratio {e_hip / e_torch:.3f}")
        worst.append((name, e_hip, e_torch))
    for name, e_hip, e_torch in worst:
        assert e_hip <= 2 * e_torch, (name, e_hip, e_torch)
