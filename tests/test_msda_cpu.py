"""Multi-scale deformable attention without a GPU: the corner-by-corner restatement of the contract (msda_cases.py) pinned
against the public grid_sample statement before test_gpu_msda.py uses it as the yardstick; the declared symbol; the checks of
the C entry and of the Python entry points that refuse before any launch."""
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

import msda_cases as mc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before it launches anything


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_restatement_equals_the_grid_sample_statement_in_float64(case):
    value, shapes, start, loc, w = mc.make_case(case)
    outside = ((loc < 0) | (loc > 1)).any(-1).float().mean()
    if loc[..., 0].numel() >= 1000:
        assert 0.3 < outside < 0.5  # the outside-sample share the cases are built for
    a = mc.restatement(value, shapes, start, loc, w, torch.float64)
    b = mc.statement(value, shapes, start, loc, w, torch.float64)
    assert a.shape == b.shape == (case[1], case[2], case[3] * case[4]) and a.dtype == torch.float64
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), err


def test_restatement_drops_rows_outside_value_and_empty_levels():
    value, shapes, start, loc, w = mc.make_case(mc.SMALL)
    S = value.shape[1]
    full = mc.restatement(value, shapes, start, loc, w)
    # rows >= rows are absent: the same as zeros in their place
    cut = S - 5
    zeroed = value.clone()
    zeroed[:, cut:] = 0
    assert torch.equal(mc.restatement(value, shapes, start, loc, w, rows=cut), mc.restatement(zeroed, shapes, start, loc, w))
    # a level with H <= 0 contributes nothing: the same as zero weights on it
    dead = shapes.clone()
    dead[1, 0] = 0
    w0 = w.clone()
    w0[:, :, :, 1] = 0
    assert torch.equal(mc.restatement(value, dead, start, loc, w), mc.restatement(value, shapes, start, loc, w0))
    assert not torch.equal(full, mc.restatement(value, dead, start, loc, w))


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert re.search(r"\bint sola_ms_deform_attn\(const float\* dev_value, const int64_t\* dev_spatial_shapes", header)
    assert "sola_ms_deform_attn" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["sola_ms_deform_attn"]
    assert res is ctypes.c_int and len(args) == 14
    fn = getattr(_lib.lib(), "sola_ms_deform_attn")  # the built library exports it
    assert fn.argtypes == args
    from sola_amd import ops
    assert int(re.search(r"#define SOLA_MSDA_MAX_LEVELS (\d+)", header).group(1)) == ops.MSDA_MAX_LEVELS == 8
    assert int(re.search(r"#define SOLA_MSDA_MAX_POINTS (\d+)", header).group(1)) == ops.MSDA_MAX_POINTS == 8
    assert "msda.hip" in open(os.path.join(ROOT, "sola_amd", "csrc", "Makefile")).read()


def test_c_entry_refuses_before_any_launch():
    L = _lib.lib()

    def call(N=1, S=100, M=8, D=32, Lq=10, Lv=4, P=4, value=FAKE, loc=FAKE, out=FAKE, w=FAKE, shapes=FAKE, start=FAKE):
        return L.sola_ms_deform_attn(value, shapes, start, loc, w, N, S, M, D, Lq, Lv, P, out, None)

    for kw, text in (({"D": 24}, b"D = 24"), ({"D": 8}, b"D = 8"), ({"D": 128}, b"D = 128"), ({"Lv": 0}, b"L = 0"), ({"Lv": 9}, b"L = 9"),
                     ({"P": 0}, b"P = 0"), ({"P": 9}, b"P = 9"), ({"N": 0}, b">= 1"), ({"S": 0}, b">= 1"), ({"M": -1}, b">= 1"),
                     ({"Lq": 0}, b">= 1"), ({"value": None}, b"null"), ({"loc": None}, b"null"), ({"out": None}, b"null"),
                     ({"w": None}, b"null"), ({"shapes": None}, b"null"), ({"start": None}, b"null"),
                     ({"value": ctypes.c_void_p((1 << 20) + 8)}, b"16-byte"), ({"loc": ctypes.c_void_p((1 << 20) + 4)}, b"16-byte"),
                     ({"out": ctypes.c_void_p((1 << 20) + 8)}, b"16-byte"), ({"w": ctypes.c_void_p((1 << 20) + 2)}, b"4-byte"),
                     ({"shapes": ctypes.c_void_p((1 << 20) + 4)}, b"8-byte"),
                     # 32-bit indexing: one batch element's bytes, value's elements, the locations, the output
                     ({"S": 1 << 21, "M": 8, "D": 32}, b"2^31"), ({"N": 64, "S": 1 << 17, "M": 8, "D": 32}, b"N*S*M*D"),
                     ({"N": 4, "Lq": 1 << 20, "M": 8, "Lv": 8, "P": 8}, b"N*Lq*M*L*P*2"),
                     ({"N": 16, "Lq": 1 << 20, "M": 8, "D": 64, "Lv": 1, "P": 1}, b"N*Lq*M*D"),
                     ({"N": 1 << 16, "Lq": 1 << 16, "M": 2, "Lv": 1, "P": 1}, b"N*Lq*M*L*P*2")):
        assert call(**kw) == -1, kw
        assert text in L.sola_last_error(), (kw, L.sola_last_error())


def test_python_entry_points_refuse():
    from sola_amd import ops
    value, shapes, start, loc, w = mc.make_case(mc.SMALL)
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    with pytest.raises(SolaError, match="GPU only"):
        ops.ms_deform_attn(value, shapes, start, loc, w)
    with pytest.raises(SolaError, match="GPU only"):
        ops.gdino_ext.ms_deform_attn_forward(value, shapes, start, loc, w, 64)
    for bad in (torch.float16, torch.bfloat16):
        for args in ((value.to(bad), shapes, start, loc, w), (value, shapes, start, loc.to(bad), w), (value, shapes, start, loc, w.to(bad))):
            with pytest.raises(SolaError, match="float32 only.*GroundingDINO"):
                ops.ms_deform_attn(*args)
    with pytest.raises(SolaError, match="float32"):
        ops.ms_deform_attn(value.double(), shapes, start, loc, w)
    # shapes against each other: batch, heads, queries, levels, points; the tables' length and type
    for args in ((value[:1], shapes, start, loc, w), (value[:, :, :2], shapes, start, loc, w), (value, shapes, start, loc[:, :5], w),
                 (value, shapes, start, loc, w[:, :, :, :3]), (value, shapes, start, loc, w[..., :3]), (value.flatten(2), shapes, start, loc, w),
                 (value, shapes, start, loc[..., :1], w)):
        with pytest.raises(SolaError, match="shapes disagree|expected value"):
            ops.ms_deform_attn(*args)
    for args in ((value, shapes[:3], start, loc, w), (value, shapes, start[:3], loc, w), (value, shapes.int(), start, loc, w),
                 (value, shapes, start.float(), loc, w), (value, shapes.flatten(), start, loc, w)):
        with pytest.raises(SolaError, match="int64"):
            ops.ms_deform_attn(*args)
    # a value whose S disagrees with the maps the table describes cannot be told apart on the host (the table stays on the
    # device); what the host CAN see is an S that leaves no row at all
    with pytest.raises(SolaError, match="S 0"):
        ops.ms_deform_attn(value[:, :0], shapes, start, loc, w)
    with pytest.raises(SolaError, match="D = 24"):
        ops.ms_deform_attn(torch.zeros(N, S, M, 24), shapes, start, loc, w)
    nine = torch.ones(9, 2, dtype=torch.int64)
    with pytest.raises(SolaError, match="L = 9"):
        ops.ms_deform_attn(value, nine, nine[:, 0].clone(), torch.zeros(N, Lq, M, 9, P, 2), torch.zeros(N, Lq, M, 9, P))
    with pytest.raises(SolaError, match="P = 9"):
        ops.ms_deform_attn(value, shapes, start, torch.zeros(N, Lq, M, L, 9, 2), torch.zeros(N, Lq, M, L, 9))
    with pytest.raises(SolaError, match="inference only"):
        ops.gdino_ext.ms_deform_attn_backward(value, shapes, start, loc, w, value, 64)
