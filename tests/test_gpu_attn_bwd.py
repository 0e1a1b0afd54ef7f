"""sola_attention_backward / sola_attention_backward_ws in f32 against float64 autograd (attn_bwd_cases.py, checked in
test_attn_bwd_cpu.py) on every branch of launch_attention_bwd at head dim 128: the register kernel, the one-pass kernel at one, two
and four waves, unchunked and in 64- and 256-query chunks, the block-shared and per-wave two-pass kernels and their two mixtures;
under the A/B switches still in the build; with gradients written into column blocks of a wider buffer; and with dropout, the mask
read out of the forward by the one-hot probe.  With -s the module ends with the worst error / bar of every branch
(profiles/attn_bwd_parity.txt)."""
import collections
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as ac  # noqa: E402
from sola_amd import _lib, ops  # noqa: E402
from sola_amd._lib import check, current_stream, lib  # noqa: E402

pytestmark = pytest.mark.gpu

P_DROP, SEED = 0.1, 777
SENTINEL = -7.25e10
WORST = collections.defaultdict(lambda: [0.0, 0.0, 0.0])  # (branch, "plain" | "dropout") -> worst error / bar of dq, dk, dv


@pytest.fixture(autouse=True)
def _reset_stage_dropout():
    yield
    ops.set_stage_dropout(0.0, 0)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    print("\nattention backward, f32 kernels against float64: worst max|error| / (3e-5 max|reference|) per branch")
    print(f"{'branch':<18}{'':<9}{'dq':>8}{'dk':>8}{'dv':>8}")
    for (branch, kind), r in sorted(WORST.items()):
        print(f"{branch:<18}{kind:<9}{r[0]:8.4f}{r[1]:8.4f}{r[2]:8.4f}")


def fptr(t, col=0):
    """Device pointer of column ``col`` of row 0 of a float32 matrix."""
    return C.c_void_p(t.data_ptr() + 4 * col)


def geometry(case):
    inner, qa, ka, _, _ = ac.addressing(case)
    return (case.G, case.H, case.DH, case.Sq, case.Sk, inner, *qa, *ka, float(ac.case_scale(case)))


def forward(case, q, k, v):
    inner, qa, ka, _, _ = ac.addressing(case)
    return ops.attention(q, k, v, case.G, case.H, case.Sq, case.Sk, inner, qa, ka, scale=ac.case_scale(case), return_lse=True)


def backward(case, q, k, v, o, dout, lse):
    """case.scratch: ops.attention_backward (always hands the chunk scratch over); else the entry without scratch."""
    inner, qa, ka, _, _ = ac.addressing(case)
    if case.scratch:
        return ops.attention_backward(q, k, v, o, dout, lse, case.G, case.H, case.Sq, case.Sk, inner, qa, ka, scale=ac.case_scale(case))
    D = q.shape[1]
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    dvec = torch.zeros((q.shape[0], case.H), device=q.device)
    check(lib().sola_attention_backward(fptr(q), D, fptr(k), D, fptr(v), D, fptr(o), fptr(dout), D, fptr(lse), fptr(dq), fptr(dk), fptr(dv),
                                        fptr(dvec), *geometry(case), current_stream(q.device)), "sola_attention_backward")
    return dq, dk, dv


def run(case, switches=None, inputs=None):
    """Forward and backward on the plain pitch: (o, (dq, dk, dv)) on the device."""
    q, k, v, dout = (t.cuda() for t in (inputs or ac.make_inputs(case)))
    o, lse = forward(case, q, k, v)
    with _lib.tuned(**(switches or {})):
        return o, backward(case, q, k, v, o, dout, lse)


def assert_parity(case, got, want, inputs, what, switches=None, mask=None, p=0.0):
    ratios = ac.error_ratios(case, [g.cpu() for g in got], want, inputs, mask, p)
    branch = ac.expected_branch(case, switches)
    print(f"{case.id} [{branch}] {what}: error / bar  dq {ratios['dq']:.4f}  dk {ratios['dk']:.4f}  dv {ratios['dv']:.4f}")
    w = WORST[(branch, "dropout" if mask is not None else "plain")]
    for i, n in enumerate(("dq", "dk", "dv")):
        w[i] = max(w[i], ratios[n])
    assert max(ratios.values()) <= 1.0, (case.id, branch, what, ratios)
    return ratios


# ---- 1: every case, default switches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_gradients_against_float64(case):
    inputs, want = ac.plain_reference(case)
    _, got = run(case)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and g.shape == w.shape
    assert_parity(case, got, want, inputs, "default")


# ---- 2: packed pitch ----------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.pitch == "packed"], ids=ac.case_id)
def test_gradients_into_column_blocks_leave_every_other_value_alone(case):
    """q, k, v = column blocks 0, 1, 2 of X [rows][4 D]; dq, dk, dv go to the same blocks of a sentinel-filled buffer of that pitch;
    o (from ops.attention) and dout are blocks 1 and 0 of two [q rows][2 D] buffers.  Whatever the inputs do not define is NaN: a
    stray read shows in the result, a stray write in the sentinels (block 3, the rows behind the shorter side, the rows between
    gapped units)."""
    inputs, want = ac.plain_reference(case)
    q, k, v, dout = inputs
    _, _, _, rq, rk = ac.addressing(case)
    qi, ki = ac.unit_rows(case)
    D, R, nan = case.H * case.DH, max(rq, rk), float("nan")
    free_q = torch.ones(rq, dtype=torch.bool).index_fill(0, qi.reshape(-1), False)
    free_k = torch.ones(rk, dtype=torch.bool).index_fill(0, ki.reshape(-1), False)
    X = torch.full((R, 4 * D), nan)
    X[:rq, :D], X[:rk, D:2 * D], X[:rk, 2 * D:3 * D] = q, k, v
    X[:rq, :D][free_q] = nan  # the rows between units are nobody's on the way in either
    X[:rk, D:3 * D][free_k] = nan
    GO = torch.full((rq, 2 * D), nan)
    GO[:, :D] = dout
    GO[:, :D][free_q] = nan
    X, GO = X.cuda(), GO.cuda()
    o, lse = forward(case, q.cuda(), k.cuda(), v.cuda())
    OB = torch.full((rq, 2 * D), nan, device="cuda")
    OB[:, D:][~free_q.cuda()] = o[~free_q.cuda()]
    GX = torch.full((R, 4 * D), SENTINEL, device="cuda")
    dvec = torch.zeros((rq, case.H), device="cuda")
    stream = current_stream(X.device)
    geo = geometry(case)
    args = (fptr(X), 4 * D, fptr(X, D), 4 * D, fptr(X, 2 * D), 4 * D, fptr(OB, D), fptr(GO), 2 * D, fptr(lse),
            fptr(GX), fptr(GX, D), fptr(GX, 2 * D), fptr(dvec), *geo)
    if case.scratch:
        n_scr = int(lib().sola_attention_backward_scratch_floats(rq, case.G, case.H, case.Sk))
        scr = torch.empty(max(n_scr, 1), device="cuda")
        check(lib().sola_attention_backward_ws(*args, rq, fptr(scr) if n_scr else None, n_scr, stream), "sola_attention_backward_ws")
    else:
        check(lib().sola_attention_backward(*args, stream), "sola_attention_backward")
    GX = GX.cpu()
    owned = torch.zeros((R, 4 * D), dtype=torch.bool)
    owned[qi.reshape(-1), :D] = True
    owned[ki.reshape(-1), D:3 * D] = True
    sentinel_bits = int(bits(torch.tensor([SENTINEL]))[0])
    touched = (bits(GX) != sentinel_bits) & ~owned
    assert not touched.any(), (case.id, touched.nonzero()[:8].tolist())
    assert not (bits(GX)[owned] == sentinel_bits).any()  # and every owned value was written
    got = torch.where(owned, GX, torch.zeros(()))
    assert_parity(case, (got[:rq, :D], got[:rk, D:2 * D], got[:rk, 2 * D:3 * D]), want, inputs, "packed")


# ---- 3: the A/B switches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switches", ac.SWITCH_SETTINGS[1:], ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_gradients_against_float64_under_the_switches(case, switches):
    inputs, want = ac.plain_reference(case)
    _, got = run(case, switches)
    assert_parity(case, got, want, inputs, ",".join(f"{k}={v}" for k, v in switches.items()), switches)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.Sq > 16 or c.Sk > 16], ids=ac.case_id)
def test_block_shared_staging_gives_the_bits_of_per_wave_staging(case):
    """docs/tune_keys.md: "attn_bwd_blk" 1 is bit-identical to 0."""
    _, blk = run(case, {"attn_bwd_fused": 0, "attn_bwd_blk": 1})
    _, wave = run(case, {"attn_bwd_fused": 0, "attn_bwd_blk": 0})
    for name, a, b in zip(("dq", "dk", "dv"), blk, wave):
        assert torch.equal(a, b), (case.id, name, float((a - b).abs().max()))


# ---- 4: repeatability of the chunked launches ---------------------------------------------------------------------------------------
CHUNKED = [c for c in ac.CASES if ac.is_chunked(c)]


@pytest.mark.parametrize("case", CHUNKED, ids=ac.case_id)
def test_chunked_launches_repeat_their_bits(case):
    """The reduce adds a unit's partial sums in chunk order, so two runs agree in every bit."""
    _, a = run(case)
    _, b = run(case)
    for name, x, y in zip(("dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), (case.id, name)


@pytest.mark.parametrize("case", [c for c in CHUNKED if c.Sq <= 256], ids=ac.case_id)
def test_chunked_and_unchunked_launches_of_one_shape_both_meet_the_bar(case):
    inputs, want = ac.plain_reference(case)
    whole = case._replace(scratch=False)
    assert ac.expected_branch(whole) == ac.expected_branch(case).split("/")[0] + "/nochunk"
    assert_parity(case, run(case)[1], want, inputs, "chunked")
    assert_parity(whole, run(whole, inputs=inputs)[1], want, inputs, "unchunked")


# ---- 5, 6: dropout ------------------------------------------------------------------------------------------------------------------
def recovered_mask(case, q, k, seed, passes=None):
    """(dropped probabilities [G, H, Sq, Sk'] float32 on the CPU, Sk' = the keys of the probe passes made)."""
    ops.set_stage_dropout(P_DROP, seed)
    n = ac.probe_passes(case) if passes is None else passes
    outs = [forward(case, q, k, ac.probe_v(case, b).cuda())[0].cpu() for b in range(n)]
    return ac.probe_collect(case, outs)


def dropout_check(case, switches):
    inputs = ac.make_inputs(case)
    q, k, v, dout = inputs
    qd, kd = q.cuda(), k.cuda()
    pd = recovered_mask(case, qd, kd, SEED)
    mask = pd != 0
    assert mask.numel() >= 4000
    keep = float(mask.double().mean())
    assert abs(keep - (1 - P_DROP)) < 0.03, (case.id, keep)
    P, o_ref = ac.forward64(case, q, k, v, mask, P_DROP)
    e_p = float((pd.double() - P).abs().max())
    o, got = run(case, switches)  # the same seed is still set
    e_o = float((o.cpu().double() - o_ref).abs().max())
    print(f"{case.id}: keep rate {keep:.4f}  max |dropped P - f64| {e_p:.3e} (bar 2e-6)  max |o - f64| {e_o:.3e} (bar 3e-6)")
    assert e_p <= 2e-6 and e_o <= 3e-6, (case.id, e_p, e_o)
    want = ac.reference(case, q, k, v, dout, mask, P_DROP)
    assert_parity(case, got, want, inputs, "dropout " + ",".join(f"{k_}={v_}" for k_, v_ in switches.items()), switches, mask, P_DROP)
    other = recovered_mask(case, qd, kd, SEED + 1, passes=1) != 0
    first = mask[..., :other.shape[-1]]
    assert float((other != first).double().mean()) > 0.05, case.id  # two independent masks at p = 0.1 differ in 18 % of the places


@pytest.mark.parametrize("case", ac.DROPOUT_CASES, ids=ac.case_id)
def test_dropout_mask_of_the_forward_is_the_mask_of_the_backward(case):
    dropout_check(case, {})


@pytest.mark.parametrize("case", ac.DROPOUT_CASES, ids=ac.case_id)
def test_dropout_under_the_two_pass_fallback(case):
    dropout_check(case, {"attn_bwd_fused": 0})


@pytest.mark.parametrize("case", [c for c in ac.DROPOUT_CASES if c.Sq <= 4 and c.Sk <= 4], ids=ac.case_id)
def test_dropout_without_the_register_kernel(case):
    dropout_check(case, {"attn_bwd_small": 0})
