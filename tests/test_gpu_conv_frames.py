"""The encoder convs over few output frames as one plain GEMM per frame (sola_amd/csrc/conv_frames.hip): the taps in the zero padding are
not multiplied, and the result has the bits of the implicit-im2col launch - both forms add the same non-zero k-chunks in the same order,
and what the per-frame form leaves out are exact zeros.  Checked on the entry point (every frame class, ragged tiles, strided windows, on
NaN-fenced outputs), on the packed weight copies, and in the forward (bits and routing)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sola_amd import _lib, ops, synth  # noqa: E402
from sola_amd._lib import tuned  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

# the three direct-to-LDS kernels of tests/test_gpu_fast.py::test_split_gemm_block_shapes_bit_identical
KERNELS = [dict(gemm_glds=1, gemm_persist=0), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=4, gemm_persist=1)]
KERNEL_IDS = ["128x128", "256x256", "persistent"]

# (R, T_in, cin, cout, k, stride, pad).  k 3 / stride 1 / pad 1: T_out = T_in = 1..5 (one tap class; two; interior + edges with one, two
# and three interior frames); stride 2 at T_in 8 (only the first window leaves the sequence) and 7 (the last one too).  R 300 / 513: ragged
# last M tile of the 256-row and 128-row kernels; cout 72 / 264: ragged N tile; cin 32: one k-tile per tap (T_in 1: a one-k-tile launch).
CASES = [
    (300, 1, 96, 72, 3, 1, 1),
    (513, 1, 32, 264, 3, 1, 1),
    (513, 2, 32, 264, 3, 1, 1),
    (300, 3, 96, 264, 3, 1, 1),
    (513, 4, 32, 72, 3, 1, 1),
    (300, 4, 96, 264, 3, 1, 1),
    (300, 5, 32, 264, 3, 1, 1),
    (513, 5, 96, 72, 3, 1, 1),
    (300, 8, 32, 72, 3, 2, 1),
    (513, 7, 96, 264, 3, 2, 1),
]
F64_CASES = {(300, 1, 96, 72, 3, 1, 1), (513, 2, 32, 264, 3, 1, 1), (300, 3, 96, 264, 3, 1, 1), (513, 4, 32, 72, 3, 1, 1), (513, 5, 96, 72, 3, 1, 1)}
FENCE = 4096  # floats in front of and behind y


def _operands(case):
    R, T, cin, cout, k, stride, pad = case
    g = torch.Generator(device="cuda").manual_seed(R * 31 + T * 7 + cin + cout + stride)
    x = torch.randn((R * T, cin), device="cuda", generator=g)
    w = torch.randn((cout, k * cin), device="cuda", generator=g)  # standardised weights have unit variance: cast with scale 1
    b = torch.randn(cout, device="cuda", generator=g)
    return ops.cast_sp16(x).view(R, T, cin), ops.cast_sp16(w), b


def _fenced(R, t_out, cout):
    n = R * t_out * cout
    big = torch.full((2 * FENCE + n,), float("nan"), device="cuda", dtype=torch.float32)
    return big, big[FENCE:FENCE + n].view(R, t_out, cout)


def _float64(x_sp, w_sp, b, case):
    R, T, cin, cout, k, stride, pad = case
    t_out = (T + 2 * pad - k) // stride + 1
    x = ops.decode_sp16(x_sp.reshape(R * T, cin)).double().cpu().numpy().reshape(R, T, cin)
    w = ops.decode_sp16(w_sp).double().cpu().numpy().reshape(cout, k, cin)
    xp = np.zeros((R, T + 2 * pad, cin))
    xp[:, pad:pad + T] = x
    ref = np.empty((R, t_out, cout))
    for t in range(t_out):
        ref[:, t] = np.einsum("rkc,okc->ro", xp[:, t * stride:t * stride + k], w) + b.double().cpu().numpy()
    return ref


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "R%d-T%d-cin%d-cout%d-k%ds%dp%d" % c)
def test_per_frame_form_has_the_bits_of_the_conv_launch(case, kernel):
    R, T, cin, cout, k, stride, pad = case
    t_out = (T + 2 * pad - k) // stride + 1
    x_sp, w_sp, b = _operands(case)
    with tuned(gemm_glds_force=1), tuned(**kernel):
        conv = ops.conv1d_cl_split(x_sp, w_sp, b, k, stride, pad, mode=0)
        big, y = _fenced(R, t_out, cout)
        ops.conv1d_cl_split(x_sp, w_sp, b, k, stride, pad, mode=1, out=y)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), "an element of y was not written"
    assert torch.isnan(big[:FENCE]).all() and torch.isnan(big[-FENCE:]).all(), "a pitched store left y"
    assert torch.equal(conv.view(torch.int32), y.view(torch.int32))
    if case in F64_CASES:
        ref = _float64(x_sp, w_sp, b, case)
        err = np.abs(y.cpu().numpy() - ref).max()
        print(f"{case}: max |err| {err:.3e}, bound {2e-6 * max(1.0, np.abs(ref).max()):.3e}")
        assert err <= 2e-6 * max(1.0, np.abs(ref).max())


def test_forward_rule_keeps_the_conv_launch_for_a_small_conv():
    """mode -1 is the forward's rule: a conv of a few hundred tracks fills no round of 256x256 tiles, so it stays one launch."""
    case = (300, 4, 96, 264, 3, 1, 1)
    x_sp, w_sp, b = _operands(case)
    with tuned(gemm_glds_force=1):
        conv = ops.conv1d_cl_split(x_sp, w_sp, b, 3, 1, 1, mode=0)
        _lib.profile_enable(True)
        try:
            _lib.profile_read(reset=True)
            auto = ops.conv1d_cl_split(x_sp, w_sp, b, 3, 1, 1, mode=-1)
            pr = _lib.profile_read(reset=True)
        finally:
            _lib.profile_enable(False)
    assert pr["gemm_split"]["launches"] + pr["gemm_split256"]["launches"] == 1
    assert torch.equal(conv.view(torch.int32), auto.view(torch.int32))


def _module(cfg):
    m = LanguageAlignedTrackSelectionModule(cfg)
    sd = synth.make_state_dict(cfg, 42)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.precision = "f16x3"
    return m


def _forward(m, B, N, T, L, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    obj = torch.randn((B, N, T, m.object_token_dim), device="cuda", generator=g)
    lang = torch.randn((B, L, m.lang_token_dim), device="cuda", generator=g)
    with torch.no_grad():
        return m(obj, lang)


SMALL_CIN_CFG = dict(synth.SMALL_MODEL_CFG, object_token_dim=16, n_groups=4)  # conv3: 32 input channels


@pytest.mark.parametrize("cfg", [SMALL_CIN_CFG, synth.DEFAULT_MODEL_CFG], ids=["cin32", "cin512"])
def test_packed_tap_ranges_are_column_slices_of_the_full_cast(cfg):
    m = _module(cfg)
    _forward(m, 1, 8, 32, 4)
    cins = [cfg["object_token_dim"]] + [2 * cfg["object_token_dim"]] * 3 + [cfg["lang_token_dim"]] * 2
    for layer in range(6):
        full, lo, hi, n = m.conv_weights_split(layer)
        assert (lo, hi) == (0, 0 if layer == 5 else 2) and n == (2 if layer in (3, 4) else 0)
        seen = set()
        for r in range(n):
            packed, lo, hi, _ = m.conv_weights_split(layer, r)
            seen.add((lo, hi))
            cut = full[:, lo * cins[layer]:(hi + 1) * cins[layer]].contiguous()
            assert torch.equal(packed.view(torch.int32), cut.view(torch.int32)), (layer, lo, hi)
        assert seen == ({(1, 2), (0, 1)} if n else set())
    # ... and the full cast is the cast of the standardised weights, as before
    w3 = m.short_motion_encoder[12].weight.detach()
    assert torch.equal(m.conv_weights_split(3)[0].view(torch.int32), ops.cast_sp16(ops.ws_standardize(w3)).view(torch.int32))


GEMM_CATEGORIES = ["gemm128", "gemm64", "gemm_split", "gemm_split256", "gemm_split256_gn"]


@pytest.fixture(scope="module")
def default_module():
    return _module(synth.DEFAULT_MODEL_CFG)


def _profiled_forward(m, B):
    _lib.profile_enable(True)
    try:
        _lib.profile_read(reset=True)
        _forward(m, B, 64, 32, 16)
        torch.cuda.synchronize()
        return _lib.profile_read(reset=True)
    finally:
        _lib.profile_enable(False)


def test_forward_takes_the_per_frame_form_for_conv3_and_conv4_and_keeps_the_bits(default_module):
    """B 128 x N 64 x T 32 is the smallest batch at which the rule holds: 2 problems x 32 x 4 = 256 tiles per launch.  A forward has
    6 conv + 14 projection GEMM launches; conv3 and conv4 are two launches each in the per-frame form."""
    m = default_module
    pr = _profiled_forward(m, 128)
    assert sum(pr[c]["launches"] for c in GEMM_CATEGORIES) == 22, {c: pr[c]["launches"] for c in GEMM_CATEGORIES}
    R = 128 * 64
    for layer, src in ((3, "act2"), (4, "act3")):
        conv = m.short_motion_encoder[4 * layer]
        x_sp = m.workspace_tap(src).view(R, 4, conv.in_channels)
        w_sp = ops.cast_sp16(ops.ws_standardize(conv.weight.detach()))
        ref = ops.conv1d_cl_split(x_sp, w_sp, conv.bias.detach(), 3, 1, 1, mode=0)
        got = m.workspace_tap(f"conv{layer}").view(R, 4, conv.out_channels)
        assert torch.equal(ref.view(torch.int32), got.view(torch.int32)), layer


def test_forward_keeps_the_conv_launches_at_a_small_batch(default_module):
    pr = _profiled_forward(default_module, 8)
    assert sum(pr[c]["launches"] for c in GEMM_CATEGORIES) == 20, {c: pr[c]["launches"] for c in GEMM_CATEGORIES}
