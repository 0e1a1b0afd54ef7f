"""Multi-scale deformable attention, backward, without a GPU: the float64 yardstick of test_gpu_msda_bwd.py pinned (autograd through
the restatement against autograd through the public grid_sample statement), the bounds calibrated with the float32 CPU
autograd, the declared symbol, and the checks of the C entry and of the Python entry points that refuse before any launch."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import msda_bwd_cases as bc  # noqa: E402
import msda_cases as mc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before it launches anything


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_restatement_autograd_equals_statement_autograd_in_float64(case):
    inputs, grad_out, want = bc.grad_reference(case)
    stmt = bc.autograd_grads(mc.statement, *inputs, grad_out, torch.float64)
    for name, a, b in zip(("grad_value", "grad_loc", "grad_weight"), want, stmt):
        assert a.shape == b.shape and a.dtype == torch.float64
        err = float((a - b).abs().max())
        assert err <= 1e-11 * max(1.0, float(b.abs().max())), (name, err)
    assert float(want[0].abs().max()) > 0.1 and float(want[1].abs().max()) > 0.1 and float(want[2].abs().max()) > 0.1


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_float32_cpu_autograd_lies_inside_every_bound(case):
    """Calibration of the three bounds: the float32 autograd of the restatement, whose arithmetic the bounds describe, must sit
    well inside them, and near_border may leave out at most MAX_EXCLUDED of the samples."""
    inputs, grad_out, want = bc.grad_reference(case)
    f32 = bc.autograd_grads(mc.restatement, *inputs, grad_out, torch.float32)
    ratios, excluded = bc.worst_ratios(f32, want, *inputs, grad_out)
    print(f"{mc.case_id(case)}: float32 CPU autograd at {ratios[0]:.4f} / {ratios[1]:.4f} / {ratios[2]:.4f} of the grad_value / grad_loc / "
          f"grad_weight bounds; {100 * excluded:.3f} % of the samples near a cell border")
    assert max(ratios) <= 1.0, ratios
    assert excluded <= bc.MAX_EXCLUDED, excluded


def test_near_border_marks_the_samples_next_to_a_cell_border():
    shapes = torch.tensor([[4, 8]], dtype=torch.int64)
    # pixel x = loc_x * 8 - 0.5, y = loc_y * 4 - 0.5
    loc = torch.tensor([[0.3125, 0.5], [0.3125 + 1e-6, 0.5], [0.30, 0.375], [0.30, 0.375 + 1e-3], [0.30, 0.40]], dtype=torch.float64)
    got = bc.near_border(loc.view(1, 5, 1, 1, 1, 2), shapes).flatten().tolist()
    assert got == [True, True, True, False, False]


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert re.search(r"\bint sola_ms_deform_attn_backward\(const float\* dev_value, const int64_t\* dev_spatial_shapes", header)
    assert "Forward only" not in header
    res, args = _lib.SIGNATURES["sola_ms_deform_attn_backward"]
    assert res is ctypes.c_int and len(args) == 17
    fn = getattr(_lib.lib(), "sola_ms_deform_attn_backward")  # the built library exports it
    assert fn.argtypes == args


def test_c_entry_refuses_before_any_launch():
    L = _lib.lib()
    off = lambda n: ctypes.c_void_p((1 << 20) + n)  # noqa: E731

    def call(N=1, S=100, M=8, D=32, Lq=10, Lv=4, P=4, value=FAKE, loc=FAKE, w=FAKE, shapes=FAKE, start=FAKE, go=FAKE, gv=FAKE, gl=FAKE,
             gw=FAKE):
        return L.sola_ms_deform_attn_backward(value, shapes, start, loc, w, go, N, S, M, D, Lq, Lv, P, gv, gl, gw, None)

    for kw, text in (
            # the new conditions: grad_out, the three outputs
            ({"go": None}, b"null"), ({"gv": None, "gl": None, "gw": None}, b"all null"), ({"go": off(2)}, b"4-byte"),
            ({"gv": off(2)}, b"4-byte"), ({"gw": off(1)}, b"4-byte"), ({"gl": off(4)}, b"8-byte"), ({"gl": off(4), "gv": None, "gw": None}, b"8-byte"),
            # a sample of the forward's
            ({"D": 24}, b"D = 24"), ({"Lv": 0}, b"L = 0"), ({"Lv": 9}, b"L = 9"), ({"P": 9}, b"P = 9"), ({"N": 0}, b">= 1"),
            ({"Lq": 0}, b">= 1"), ({"value": None}, b"null"), ({"loc": None}, b"null"), ({"w": None}, b"null"), ({"shapes": None}, b"null"),
            ({"start": None}, b"null"), ({"value": off(8)}, b"16-byte"), ({"loc": off(4)}, b"16-byte"), ({"w": off(2)}, b"4-byte"),
            ({"start": off(4)}, b"8-byte"), ({"S": 1 << 21, "M": 8, "D": 32}, b"2^31"), ({"N": 64, "S": 1 << 17, "M": 8, "D": 32}, b"N*S*M*D"),
            ({"N": 4, "Lq": 1 << 20, "M": 8, "Lv": 8, "P": 8}, b"N*Lq*M*L*P*2"),
            ({"N": 16, "Lq": 1 << 20, "M": 8, "D": 64, "Lv": 1, "P": 1}, b"N*Lq*M*D")):
        assert call(**kw) == -1, kw
        assert text in L.sola_last_error() and b"ms_deform_attn_backward:" in L.sola_last_error(), (kw, L.sola_last_error())


def test_python_entry_points_refuse():
    from sola_amd import ops
    value, shapes, start, loc, w = mc.make_case(mc.SMALL)
    grad_out = bc.make_grad_out(mc.SMALL)
    for fn in (ops.ms_deform_attn_backward, lambda *a: ops.gdino_train_ext.ms_deform_attn_backward(*a, 64)):
        with pytest.raises(SolaError, match="GPU only"):
            fn(value, shapes, start, loc, w, grad_out)
    # a CPU tensor that requires grad is refused like any other: no graph is recorded around a call that cannot run
    with pytest.raises(SolaError, match="GPU only"):
        ops.ms_deform_attn(value.clone().requires_grad_(True), shapes, start, loc, w)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(SolaError, match="grad_output is .*float32 only"):
            ops.ms_deform_attn_backward(value, shapes, start, loc, w, grad_out.to(bad))
    with pytest.raises(SolaError, match="grad_output must be float32"):
        ops.ms_deform_attn_backward(value, shapes, start, loc, w, grad_out.double())
    N, Lq, MD = grad_out.shape
    for g in (grad_out[:1], grad_out[:, :5], grad_out[..., :32], grad_out.reshape(N, Lq, 3, 32), grad_out.flatten()):
        with pytest.raises(SolaError, match=r"grad_output must be \[N,Lq,M\*D\]"):
            ops.ms_deform_attn_backward(value, shapes, start, loc, w, g)
    with pytest.raises(SolaError, match="at least one"):
        ops.ms_deform_attn_backward(value, shapes, start, loc, w, grad_out, need=(False, False, False))
    # the forward's checks, factored out and shared: a sample
    with pytest.raises(SolaError, match="shapes disagree"):
        ops.ms_deform_attn_backward(value[:1], shapes, start, loc, w, grad_out)
    with pytest.raises(SolaError, match="int64"):
        ops.ms_deform_attn_backward(value, shapes.int(), start, loc, w, grad_out)
    with pytest.raises(SolaError, match="D = 24"):
        ops.ms_deform_attn_backward(torch.zeros(2, value.shape[1], 3, 24), shapes, start, loc, w, torch.zeros(2, Lq, 72))


def test_the_training_stand_in_has_both_names_and_the_inference_one_still_refuses():
    from sola_amd import ops
    assert callable(ops.gdino_train_ext.ms_deform_attn_forward) and callable(ops.gdino_train_ext.ms_deform_attn_backward)
    assert ops.gdino_train_ext is not ops.gdino_ext
    value, shapes, start, loc, w = mc.make_case(mc.SMALL)
    with pytest.raises(SolaError, match="inference only"):
        ops.gdino_ext.ms_deform_attn_backward(value, shapes, start, loc, w, value, 64)
    with pytest.raises(SolaError, match="GPU only"):
        ops.gdino_train_ext.ms_deform_attn_forward(value, shapes, start, loc, w, 64)
