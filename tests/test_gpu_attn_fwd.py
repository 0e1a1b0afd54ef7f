"""sola_attention in f32 against float64 (attn_fwd_cases.py, checked in test_attn_fwd_cpu.py) on every kernel launch_attention can pick:
the register-only short-sequence kernel, the register-only MFMA shape, the resident-K/V shape for few keys, the high-occupancy shape
in its double-buffered, single-buffered and training forms, and attn.hip's packed and shared shapes at every head dim (resident,
q-block loop, eight waves, streaming, capped grids) - o and the log-sum-exp, with and without it, into column blocks of fenced
buffers, under the sola_tune switches still in the build, twice for equal bits, with dropout (the mask read out by the one-hot
probe), and the calls the entry refuses.  With -s the module ends with the worst error / bar of every branch
(profiles/attn_fwd_parity.txt)."""
import collections
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fwd_cases as fc  # noqa: E402
from sola_amd import _lib, ops  # noqa: E402
from sola_amd._lib import SolaError, check, current_stream, lib  # noqa: E402

pytestmark = pytest.mark.gpu

P_DROP, SEED = 0.1, 777
SENTINEL = -7.25e10
WORST = collections.defaultdict(lambda: [0.0, None])  # (branch, "plain" | "spiked" | "saturated" | "dropout") -> worst error / bar of o and lse


@pytest.fixture(autouse=True)
def _reset_stage_dropout():
    yield
    ops.set_stage_dropout(0.0, 0)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    print("\nattention forward, f32 kernels against float64: worst max|error| / bar per branch")
    print("(o: 2e-5 max(1, max|reference|), with dropout 3e-6; lse: 2e-4)")
    print(f"{'branch':<24}{'':<10}{'o':>8}{'lse':>8}")
    for (branch, kind), r in sorted(WORST.items()):
        print(f"{branch:<24}{kind:<10}{r[0]:8.4f}" + (f"{r[1]:8.4f}" if r[1] is not None else f"{'-':>8}"))


def fptr(t, col=0):
    """Device pointer of column ``col`` of row 0 of a float32 matrix."""
    return C.c_void_p(t.data_ptr() + 4 * col)


def bits(t):
    return t.contiguous().view(torch.int32)


SENTINEL_BITS = int(bits(torch.tensor([SENTINEL]))[0])


def geometry(case):
    inner, qa, ka, _, _ = fc.addressing(case)
    return (case.G, case.H, case.DH, case.Sq, case.Sk, inner, *qa, *ka, float(fc.case_scale(case)))


@functools.lru_cache(maxsize=None)
def device_inputs(case, variant="normal"):
    """q, k, v on the device: made once per case and variant, shared, never modified."""
    return tuple(t.cuda() for t in fc.make_inputs(case, variant))


def run(case, lse, switches=None, variant="normal", v=None):
    """ops.attention on the plain pitch: (o, lse or None) on the device; o and lse start as zeros."""
    q, k, v0 = device_inputs(case, variant)
    inner, qa, ka, _, _ = fc.addressing(case)
    with _lib.tuned(**(switches or {})):
        out = ops.attention(q, k, v0 if v is None else v, case.G, case.H, case.Sq, case.Sk, inner, qa, ka, scale=fc.case_scale(case), return_lse=lse)
    return out if lse else (out, None)


def record(branch, kind, r_o, r_lse):
    w = WORST[(fc.base_branch(branch), kind)]
    w[0] = max(w[0], r_o)
    if r_lse is not None:
        w[1] = max(w[1] or 0.0, r_lse)


def assert_parity(case, branch, o, lse, want_o, want_lse, what, kind="plain"):
    """o (and lse where given) on the CPU against float64, in every row: the rows no unit owns are zero on both sides."""
    assert o.dtype == torch.float32 and o.shape == want_o.shape and not torch.isnan(o).any()
    r_o = fc.o_ratio(o, want_o)
    r_lse = None
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.shape == want_lse.shape and not torch.isnan(lse).any()
        r_lse = fc.lse_ratio(lse, want_lse)
    print(f"{case.id} [{branch}] {what}: error / bar  o {r_o:.4f}" + ("" if r_lse is None else f"  lse {r_lse:.4f}"))
    record(branch, kind, r_o, r_lse)
    assert r_o <= 1.0 and (r_lse is None or r_lse <= 1.0), (case.id, branch, what, r_o, r_lse)


def plain_check(case, switches=None, variant="normal"):
    _, want_o, want_lse = fc.plain_reference(case, variant)
    o, lse = run(case, case.lse, switches, variant)
    assert_parity(case, fc.expected_branch(case, switches), o.cpu(), None if lse is None else lse.cpu(), want_o, want_lse,
                  fc.switch_id(switches or {}) + ("" if variant == "normal" else " " + variant), "plain" if variant == "normal" else variant)
    return o, lse


# ---- 1: every case, default switches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_output_and_lse_against_float64(case):
    plain_check(case)


@pytest.mark.parametrize("case,variant", fc.VARIANTS, ids=lambda x: x if isinstance(x, str) else x.id)
def test_spiked_and_saturated_inputs_against_float64(case, variant):
    """A key of the last, partial key tile that takes the whole row (the running maximum moves in the last step, on a tile whose
    tail is masked), and rows close to one-hot (every other exponential underflows)."""
    plain_check(case, variant=variant)


# ---- 2: the log-sum-exp output does not change o --------------------------------------------------------------------------------------
SAME_KERNEL_WITH_LSE = [c for c in fc.CASES if fc.expected_branch(c, lse=True) == fc.expected_branch(c, lse=False)]


@pytest.mark.parametrize("case", SAME_KERNEL_WITH_LSE, ids=lambda c: c.id)
def test_asking_for_the_lse_leaves_every_bit_of_o(case):
    with_lse, lse = run(case, True)
    without, _ = run(case, False)
    assert torch.equal(bits(with_lse), bits(without)), (case.id, float((with_lse - without).abs().max()))
    want = fc.plain_reference(case)[2]
    assert fc.lse_ratio(lse.cpu(), want) <= 1.0


# ---- 3: column blocks of fenced buffers -----------------------------------------------------------------------------------------------
def fenced_check(case, switches=None):
    """q, k, v = column blocks 0, 1, 2 of X [rows][4 D] whose every other value is NaN - block 3, the rows behind the shorter side,
    the rows between gapped units: a stray read shows in the result.  o goes to block 1 of a sentinel-filled [q rows][2 D] buffer,
    the log-sum-exp into a sentinel-filled [q rows][H]: a stray write shows in the sentinels, a row not written too."""
    (q, k, v), want_o, want_lse = fc.plain_reference(case)
    _, _, _, rq, rk = fc.addressing(case)
    qi, ki = fc.unit_rows(case)
    D, R, nan = case.H * case.DH, max(rq, rk), float("nan")
    own_q = torch.zeros(rq, dtype=torch.bool).index_fill(0, qi.reshape(-1), True)
    own_k = torch.zeros(rk, dtype=torch.bool).index_fill(0, ki.reshape(-1), True)
    X = torch.full((R, 4 * D), nan)
    X[:rq, :D][own_q] = q[own_q]
    X[:rk, D:2 * D][own_k] = k[own_k]
    X[:rk, 2 * D:3 * D][own_k] = v[own_k]
    X = X.cuda()
    OB = torch.full((rq, 2 * D), SENTINEL, device="cuda")
    LB = torch.full((rq, case.H), SENTINEL, device="cuda")
    branch = fc.expected_branch(case, switches, ld=4 * D)
    assert branch == fc.expected_branch(case, switches)  # the pitch does not move a case of the table to another kernel
    with _lib.tuned(**(switches or {})):
        check(lib().sola_attention(fptr(X), 4 * D, fptr(X, D), 4 * D, fptr(X, 2 * D), 4 * D, fptr(OB, D), 2 * D, *geometry(case),
                                   fptr(LB) if case.lse else None, current_stream(X.device)), "sola_attention")
    OB, LB = OB.cpu(), LB.cpu()
    owned = torch.zeros((rq, 2 * D), dtype=torch.bool)
    owned[own_q, D:] = True
    touched = (bits(OB) != SENTINEL_BITS) & ~owned
    assert not touched.any(), (case.id, branch, touched.nonzero()[:8].tolist())
    assert not (bits(OB)[owned] == SENTINEL_BITS).any(), (case.id, branch)  # and every owned value was written
    lse = None
    if case.lse:
        lse_owned = own_q[:, None].expand(rq, case.H)
        touched = (bits(LB) != SENTINEL_BITS) & ~lse_owned
        assert not touched.any(), (case.id, branch, "lse", touched.nonzero()[:8].tolist())
        assert not (bits(LB)[lse_owned] == SENTINEL_BITS).any(), (case.id, branch, "lse")
        lse = torch.where(lse_owned, LB, torch.zeros(()))
    else:
        assert (bits(LB) == SENTINEL_BITS).all(), (case.id, branch, "lse written without being asked for")
    o = torch.where(owned, OB, torch.zeros(()))[:, D:]
    assert_parity(case, branch, o, lse, want_o, want_lse, "fenced " + fc.switch_id(switches or {}))


PACKED = [c for c in fc.CASES if c.pitch == "packed"]


@pytest.mark.parametrize("case", PACKED, ids=lambda c: c.id)
def test_column_blocks_of_fenced_buffers_leave_every_other_value_alone(case):
    fenced_check(case)


# ---- 4: the A/B switches ------------------------------------------------------------------------------------------------------------
MOVED = [(s, c) for s in fc.SWITCH_SETTINGS for c in fc.CASES if fc.expected_launch(c, s) != fc.expected_launch(c)]


@pytest.mark.parametrize("switches,case", MOVED, ids=[f"{fc.switch_id(s)}-{c.id}" for s, c in MOVED])
def test_output_and_lse_against_float64_under_the_switches(switches, case):
    """Every case whose kernel or launch parameters the setting changes."""
    o, lse = plain_check(case, switches)
    if "attn_simple_remap" in switches:  # another block order and nothing else: docs/tune_keys.md
        base_o, base_lse = run(case, case.lse)
        assert torch.equal(bits(o), bits(base_o)) and (lse is None or torch.equal(bits(lse), bits(base_lse))), case.id


MOVED_PACKED = [(s, c) for s, c in MOVED if c.pitch == "packed"]


@pytest.mark.parametrize("switches,case", MOVED_PACKED, ids=[f"{fc.switch_id(s)}-{c.id}" for s, c in MOVED_PACKED])
def test_column_blocks_of_fenced_buffers_under_the_switches(switches, case):
    fenced_check(case, switches)


# ---- 5: repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_two_runs_give_equal_bits(case):
    """No atomics and no order that depends on timing: a block that walks several units, or a capped grid, gives what it gave."""
    a, la = run(case, case.lse)
    b, lb = run(case, case.lse)
    assert torch.equal(bits(a), bits(b)), case.id
    assert la is None or torch.equal(bits(la), bits(lb)), case.id


# ---- 6: dropout ---------------------------------------------------------------------------------------------------------------------
def recovered(case, seed, passes=None):
    """Dropped probabilities [G, H, Sq, Sk'] float32 on the CPU (Sk' = the keys of the probe passes made)."""
    ops.set_stage_dropout(P_DROP, seed)
    n = fc.probe_passes(case) if passes is None else passes
    outs = [run(case, False, v=fc.probe_v(case, b).cuda())[0].cpu() for b in range(n)]
    return fc.probe_collect(case, outs)


@pytest.mark.parametrize("case", fc.DROPOUT_CASES, ids=lambda c: c.id)
def test_dropout_against_float64_through_the_recovered_mask(case):
    q, k, v = fc.make_inputs(case)
    branch = fc.expected_branch(case, dropout=True)
    pd = recovered(case, SEED)
    mask = pd != 0
    assert mask.numel() >= 4000
    keep = float(mask.double().mean())
    P, want_o = fc.forward64(case, q, k, v, mask, P_DROP)
    e_p = float((pd.double() - P).abs().max())
    o, lse = run(case, True)  # the same seed is still set
    e_o = float((o.cpu().double() - want_o).abs().max())
    r_lse = fc.lse_ratio(lse.cpu(), fc.lse64(case, q, k))
    print(f"{case.id} [{branch}]: keep rate {keep:.4f}  max |dropped P - f64| {e_p:.3e} (bar 2e-6)  max |o - f64| {e_o:.3e} (bar 3e-6)  "
          f"lse error / bar {r_lse:.4f}")
    record(branch, "dropout", e_o / 3e-6, r_lse)
    assert abs(keep - (1 - P_DROP)) < 0.03, (case.id, keep)
    assert e_p <= 2e-6 and e_o <= 3e-6 and r_lse <= 1.0, (case.id, branch, e_p, e_o, r_lse)
    other = recovered(case, SEED + 1, passes=1) != 0
    first = mask[..., :other.shape[-1]]
    assert float((other != first).double().mean()) > 0.05, case.id  # two independent masks at p = 0.1 differ in 18 % of the places
    # the kernels drop after normalising: the log-sum-exp is the one of the same kernel without dropout, bit for bit
    ops.set_stage_dropout(0.0, 0)
    same = next(s for s in fc.SAME_KERNEL_SETTINGS if fc.expected_branch(case, s, lse=True) == branch)
    _, lse_plain = run(case, True, same)
    assert torch.equal(bits(lse), bits(lse_plain)), (case.id, branch, float((lse - lse_plain).abs().max()))


# ---- 7: refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["pitch_q", "pitch_k", "pitch_v", "pitch_o", "head_dim_24", "no_groups"])
def test_calls_the_entry_refuses_leave_the_output_alone(what):
    """A pitch that is no multiple of 4 values (the kernels move 16 bytes at a time), a head dim nothing is compiled for, and an
    empty batch: an error through check(), before any launch."""
    H, DH, G, Sq, Sk = 8, 24 if what == "head_dim_24" else 16, 0 if what == "no_groups" else 3, 5, 7
    D = H * DH
    q = torch.randn(3 * Sq, D + 4, device="cuda")
    k, v = torch.randn(3 * Sk, D + 4, device="cuda"), torch.randn(3 * Sk, D + 4, device="cuda")
    o = torch.full((3 * Sq, D + 4), SENTINEL, device="cuda")
    lse = torch.full((3 * Sq, H), SENTINEL, device="cuda")
    ld = {n: D + 2 if what == "pitch_" + n else D + 4 for n in "qkvo"}
    status = lib().sola_attention(fptr(q), ld["q"], fptr(k), ld["k"], fptr(v), ld["v"], fptr(o), ld["o"], G, H, DH, Sq, Sk, 1,
                                  Sq, 0, 1, Sk, 0, 1, 0.25, fptr(lse), current_stream(q.device))
    assert status != 0
    with pytest.raises(SolaError):
        check(status, "sola_attention")
    torch.cuda.synchronize()
    assert (bits(o) == SENTINEL_BITS).all() and (bits(lse) == SENTINEL_BITS).all()
    if what == "head_dim_24":  # and the same sizes at a head dim that exists are taken
        DH, D = 16, 8 * 16
    elif what == "no_groups":
        G = 3
    else:
        ld = dict.fromkeys("qkvo", D + 4)
    check(lib().sola_attention(fptr(q), ld["q"], fptr(k), ld["k"], fptr(v), ld["v"], fptr(o), ld["o"], G, H, DH, Sq, Sk, 1,
                               Sq, 0, 1, Sk, 0, 1, 0.25, fptr(lse), current_stream(q.device)), "sola_attention")
    assert not (bits(o[:, :D]) == SENTINEL_BITS).any() and (bits(o[:, D:]) == SENTINEL_BITS).all() and not (bits(lse) == SENTINEL_BITS).any()
