"""The weight-gradient GEMMs dW = dY^T X against float64 (gemm_tn_cases.py, checked in test_gemm_tn_cpu.py) on every kernel and route of
sola_gemm_tn, sola_conv1d_cl_backward, sola_gemm_tn_f16, sola_conv1d_cl_wgrad_f16, sola_gemm_tn_split and sola_conv1d_cl_backward_split:
the one-tile exact-f32 kernel at eight and four waves, the persistent kernel and its conv gather, the row-major 16-bit kernel with f32 and
bfloat16 partial sums, the transposed-copy route and the split conv backward's col2im.  Every call goes through the C ABI on FENCED memory:
operands inside NaN-filled buffers (pad columns of a pitch, 64 rows behind - and, for a conv input, in front), outputs inside a
sentinel-filled arena, the scratch exactly as large as the entry point publishes, NaN-filled, with a sentinel tail - so a read past a row
or a matrix, a mixed-up pitch, a write past an output or a slab too far shows as a wrong value, never as a fault.  The route each call took
is read back from the profiler's stated bytes and launch counts.  With -s the module ends with the worst error / bar of every branch
(profiles/gemm_tn_parity.txt)."""
import collections
import os
import sys
import textwrap

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_tn_cases as gc  # noqa: E402
from sola_amd import _lib  # noqa: E402
from sola_amd._lib import check, current_stream, lib, ptr, tuned  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5A5A5          # the outputs' arena, as int32 (a NaN no kernel produces)
SCRATCH_FILL, TAIL_FILL, TAIL = 0xFF, 0xA5, 4096  # scratch bytes (NaN in every format) and the 4 KiB behind it
SOLA_ERR_ARG, SOLA_ERR_WORKSPACE = -1, -4
WORST = collections.defaultdict(lambda: [0.0, set()])  # (branch, "dW" | "db" | "dx") -> worst error / bar, the cases that reached it


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    print("\nweight-gradient GEMMs against float64: worst max|error| / bar per branch")
    print("(f32 and split: 3e-5 max|reference|; 16-bit operands, rounded-operand reference: 5e-6, bfloat16 partial sums 2^-7)")
    print(f"{'branch':<26}{'':<4}{'worst':>8}  cases (under the default switches or a setting of gemm_tn_cases.SWITCH_SETTINGS)")
    for (branch, what), (r, ids) in sorted(WORST.items()):
        print(f"{branch:<26}{what:<4}{r:8.4f}  {len(ids)}")
    for branch in sorted({b for b, _ in WORST}):
        print(textwrap.fill(f"{branch}: " + " ".join(sorted(WORST[(branch, 'dW')][1])), 140, subsequent_indent="    "))


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bits(t):
    return t.contiguous().view(torch.int32)


class Arena:
    """The outputs of one call as views into ONE int32 tensor of sentinels: each starts on 256 bytes, 256 bytes of sentinels on either side."""

    def __init__(self, shapes):
        self.at, n = {}, 64
        for name, (r, c) in shapes.items():
            self.at[name] = (n, r, c)
            n += -(-r * c // 64) * 64 + 64
        self.buf = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        self.inside = torch.zeros(n, dtype=torch.bool, device="cuda")
        for o, r, c in self.at.values():
            self.inside[o:o + r * c] = True

    def view(self, name):
        o, r, c = self.at[name]
        return self.buf[o:o + r * c].view(torch.float32).view(r, c)

    def assert_fence(self, written, what):
        held = self.buf == SENTINEL
        assert bool(held[~self.inside].all()), (what, "a write outside the outputs")
        if written:
            assert not bool(held[self.inside].any()), (what, "an output element was not written")
        else:
            assert bool(held.all()), (what, "an output was written by a refused call")


def device_fenced(mat, pitch=None, before=0):
    buf, _ = gc.fenced(mat, pitch, before)
    buf = buf.cuda()
    return buf, buf[before:before + mat.shape[0], :mat.shape[1]]


def published_scratch(case):
    L = lib()
    if case.entry in ("gemm_tn", "conv_bwd"):  # (sola_conv1d_cl_backward: the larger of this and one weight matrix - never the matrix)
        return max(L.sola_gemm_tn_scratch_bytes(case.M, case.N, case.K), 4 * case.N * case.K if case.entry == "conv_bwd" else 0)
    if case.entry == "conv_bwd_split":
        return L.sola_conv1d_cl_backward_split_scratch_bytes(*case.conv)
    return L.sola_gemm_tn_split_scratch_bytes(case.M, case.N, case.K)


def run(case, inputs, switches=None, pitched=False, short=0, want_dx=True):
    """One call of the case's entry point on fenced memory under ``switches``: {"dw", "db", "dx"} (those the entry point has) on the device.
    pitched: lda = N + 8, ldb = K + 12.  short: bytes taken off the published scratch size - the call must be refused and write nothing."""
    dy, x, w = inputs
    M, N, K = case.M, case.N, case.K
    assert not pitched or case.entry in gc.PITCHED_ENTRIES
    if case.conv is None:
        lda, ldb = (N + gc.PAD_A, K + gc.PAD_B) if pitched else (N, K)
        dy_buf, dy_v = device_fenced(dy, lda)
        x_buf, x_v = device_fenced(x, ldb)
        shapes = {"dw": (N, K)}
        if case.entry == "gemm_tn":
            shapes["db"] = (N, 1)
    else:
        R, T_in, cin, cout, k, s, p = case.conv
        dy_buf, dy_v = device_fenced(dy)
        x_buf, x_v = device_fenced(x, before=gc.FENCE_ROWS)
        w_d = w.cuda()
        shapes = {"dw": (N, K)}
        if case.entry != "conv_wgrad_f16":
            shapes["db"] = (N, 1)
            if want_dx:
                shapes["dx"] = (R * T_in, cin)
    arena = Arena(shapes)
    out = {name: arena.view(name) for name in shapes}
    stream = current_stream(dy_buf.device)
    L = lib()
    with tuned(**(switches or {})):
        nb = published_scratch(case)
        assert nb > 0 and nb % 4 == 0, (case.id, nb)
        scratch = torch.empty(nb + TAIL, dtype=torch.uint8, device="cuda")
        scratch[:nb] = SCRATCH_FILL
        scratch[nb:] = TAIL_FILL
        give = nb - short
        if case.entry == "gemm_tn":
            status = L.sola_gemm_tn(ptr(dy_v), lda, ptr(x_v), ldb, ptr(out["dw"]), ptr(out["db"]), M, N, K, ptr(scratch), give, stream)
        elif case.entry == "gemm_tn_f16":
            status = L.sola_gemm_tn_f16(ptr(dy_v), lda, ptr(x_v), ldb, ptr(out["dw"]), M, N, K, case.fmt, ptr(scratch), give, stream)
        elif case.entry == "gemm_tn_split":
            status = L.sola_gemm_tn_split(ptr(dy_v), lda, ptr(x_v), ldb, ptr(out["dw"]), M, N, K, ptr(scratch), give, stream)
        elif case.entry == "conv_wgrad_f16":
            status = L.sola_conv1d_cl_wgrad_f16(ptr(x_v), ptr(dy_v), ptr(out["dw"]), R, T_in, cin, cout, k, s, p, case.fmt, ptr(scratch), give, stream)
        else:
            fn = L.sola_conv1d_cl_backward if case.entry == "conv_bwd" else L.sola_conv1d_cl_backward_split
            status = fn(ptr(x_v), ptr(w_d), ptr(dy_v), ptr(out.get("dx")), ptr(out["dw"]), ptr(out["db"]), R, T_in, cin, cout, k, s, p, ptr(scratch), give, stream)
    torch.cuda.synchronize()
    what = (case.id, gc.switch_id(switches or {}), "pitched" if pitched else "plain")
    assert bool((scratch[nb:] == TAIL_FILL).all()), (what, "a write behind the published scratch size")
    if short:
        assert status in (SOLA_ERR_WORKSPACE, SOLA_ERR_ARG), (what, status)
        arena.assert_fence(False, what)
        assert bool((scratch[:nb] == SCRATCH_FILL).all()), (what, "the scratch was written by a refused call")
        return None
    check(status, case.id)
    arena.assert_fence(True, what)
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), (what, name, "not finite: something read a fence, a pad column or scratch nobody wrote")
    if "db" in out:
        out["db"] = out["db"].reshape(-1)
    return out


def record(case, branch, what, r):
    w = WORST[(branch, what)]
    w[0] = max(w[0], r)
    w[1].add(case.id)


def assert_parity(case, branch, out, ref, what):
    """Every element of every output against float64, as a fraction of the branch's bound."""
    _, dw, db, dx = ref
    rel = gc.bar(branch)
    for name, want, bound in (("dw", dw, rel), ("db", db, gc.F32_BAR), ("dx", dx, gc.F32_BAR)):
        if name not in out:
            continue
        r = gc.ratio(out[name].cpu(), want.reshape(out[name].shape), bound)
        print(f"{case.id} [{branch}] {what}: {name} error / bar {r:.4f}")
        record(case, branch, {"dw": "dW", "db": "db", "dx": "dx"}[name], r)
        assert r <= 1.0, (case.id, branch, what, name, r)


def same_bits(a, b, what, but=None):
    assert a.keys() == b.keys()
    for name in a:
        if name != but:
            assert torch.equal(bits(a[name]), bits(b[name])), (what, name)


def pitched_too(case):
    return (False, True) if case.entry in gc.PITCHED_ENTRIES else (False,)


def settings_of(case):
    """The default switches and every setting of gemm_tn_cases.SWITCH_SETTINGS that moves the case to another branch (at 256 CUs)."""
    return [{}] + [s for s in gc.SWITCH_SETTINGS if gc.expected_branch(case, s) != gc.expected_branch(case)]


# ---- 1: the route of every call, from the profiler's stated bytes and launch counts; the published scratch sizes -----------------------
ROUTED = [(c, s) for c in gc.CASES for s in settings_of(c)]


@pytest.mark.parametrize("case,switches", ROUTED, ids=lambda x: x.id if isinstance(x, gc.Case) else gc.switch_id(x))
def test_call_takes_the_route_of_the_restatement(case, switches):
    """gemm_tn bytes are 4 (M (N + K) + splits N K) with the PLANNED splits of the persistent route; the row-major 16-bit route states
    2 (M N + M K) + 4 ranges N K under gemm_split256, the transposed copies the NT GEMM's 2 (or 4) (N Mp + K Mp + N K); casts and folds
    are "misc" launches.  On a device of another CU count than 256 every case still runs, under the route the restatement gives there."""
    here = gc.expected_route(case, switches, cus())
    chosen = gc.expected_route(case, switches, 256)
    if cus() != 256 and (here[0], here[1]["planned"], here[1]["used"]) != (chosen[0], chosen[1]["planned"], chosen[1]["used"]):
        print(f"{case.id} {gc.switch_id(switches)}: {cus()} CUs - route {here[0]} {here[1]['planned']}/{here[1]['used']}, not the "
              f"{chosen[0]} {chosen[1]['planned']}/{chosen[1]['used']} the case was chosen for: that assertion is skipped")
    branch, info = here
    with tuned(**switches):
        assert published_scratch(case) == info["scratch"], (case.id, published_scratch(case), info["scratch"])
    try:
        _lib.profile_enable(True, categories=["gemm_tn", "gemm_split", "gemm_split256", "misc"])
        _lib.profile_read(reset=True)
        run(case, gc.make_inputs(case), switches, want_dx=False)
        pr = _lib.profile_read(reset=True)
    finally:
        _lib.profile_enable(False)
    print(f"{case.id} {gc.switch_id(switches)} [{branch}] planned {info['planned']} used {info['used']}:",
          {k: (v["launches"], v["bytes"]) for k, v in pr.items() if v["launches"]})
    for cat, want in info["prof"].items():
        cats = ("gemm_split", "gemm_split256") if cat == "gemm_split*" else (cat,)
        assert sum(pr[c]["launches"] for c in cats) == 1, (case.id, branch, cat)
        assert abs(sum(pr[c]["bytes"] for c in cats) - want) < 0.5, (case.id, branch, cat, [pr[c]["bytes"] for c in cats], want)
    if branch.startswith("f32/"):
        assert pr["gemm_split"]["launches"] + pr["gemm_split256"]["launches"] == 0
    else:
        assert pr["gemm_tn"]["launches"] == 0
        if case.fmt:
            assert pr["gemm_split"]["launches"] == 0
    if info.get("misc_launches") is not None:  # max|dY|, the casts: one per operand on the row-major route, one per tap on the other
        assert pr["misc"]["launches"] == info["misc_launches"], (case.id, branch, pr["misc"]["launches"])


# ---- 2: exact f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.F32_CASES, ids=lambda c: c.id)
def test_f32_routes_against_float64(case):
    """dW, the bias gradient (float64 column sums) and the conv's dx (float64 autograd through the oracle), every element, within 3e-5 of
    the largest reference entry; twice for equal bits; pitched = plain, bit for bit; the one-tile kernel's dW at four waves = at eight, bit
    for bit (the statement of gemm_tn.hip; its bias gradient sums the rows in another order there and is held to float64 under both); a
    persistent case also through the one-tile kernel (other bits: each is held to float64)."""
    ref = gc.reference(case)
    branch = gc.expected_branch(case, None, cus())
    first = None
    for pitched in pitched_too(case):
        out = run(case, ref[0], pitched=pitched)
        assert_parity(case, branch, out, ref, "pitched" if pitched else "plain")
        if first is None:
            first = out
            same_bits(first, run(case, ref[0]), (case.id, "run twice"))
        else:
            same_bits(first, out, (case.id, "pitched against plain"))
    # four waves against eight (docs/tune_keys.md: bit-identical dW, the bias gradient in another fixed summation order - held to float64)
    nw4 = {"gemm_tn_nw8": 0}
    if branch == "f32/tile/nw8":
        for pitched in pitched_too(case):
            out4 = run(case, ref[0], nw4, pitched=pitched)
            same_bits(first, out4, (case.id, "gemm_tn_nw8 0 against 1", pitched), but="db")
            assert_parity(case, gc.expected_branch(case, nw4, cus()), out4, ref, "gemm_tn_nw8=0" + (" pitched" if pitched else ""))
    else:
        off = {"gemm_tn_persist": 0}
        out = run(case, ref[0], off, pitched=pitched_too(case)[-1])
        assert_parity(case, gc.expected_branch(case, off, cus()), out, ref, "gemm_tn_persist=0")
        print(f"{case.id}: persistent and one-tile dW bit-equal: {torch.equal(bits(first['dw']), bits(out['dw']))}")
        out4 = run(case, ref[0], dict(off, **nw4))
        same_bits(out, out4, (case.id, "gemm_tn_nw8 0 against 1 under gemm_tn_persist 0"), but="db")
        assert_parity(case, gc.expected_branch(case, dict(off, **nw4), cus()), out4, ref, "gemm_tn_persist=0,gemm_tn_nw8=0")


# ---- 3: 16-bit operands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.F16_CASES, ids=lambda c: c.id)
def test_16bit_routes_against_float64_of_the_rounded_operands(case):
    """dW against the float64 product of the operands as the route rounds them (dY scaled by cast.hip's power of two; the conv through an
    explicit im2col): 5e-6 of the largest entry with f32 partial sums, 2^-7 with bfloat16 ones (train_bf16_store 3, the default for
    bfloat16 operands); the row-major cases also through the transposed copies (train_tn_tr 0: other bits, the same bound); twice for
    equal bits, pitched = plain.  GRADIENT_SIZED cases run on dY of size 1e-4."""
    ref = gc.reference(case, 1e-4 if case.id in gc.GRADIENT_SIZED else 1.0)
    by_setting = {}
    for switches in settings_of(case):
        branch = gc.expected_branch(case, switches, cus())
        first = None
        for pitched in pitched_too(case):
            out = run(case, ref[0], switches, pitched=pitched)
            assert_parity(case, branch, out, ref, gc.switch_id(switches) + (" pitched" if pitched else ""))
            if first is None:
                first = out
                same_bits(first, run(case, ref[0], switches), (case.id, switches, "run twice"))
            else:
                same_bits(first, out, (case.id, switches, "pitched against plain"))
        by_setting[gc.switch_id(switches)] = (branch, first["dw"])
    if "train_tn_tr=0" in by_setting:
        a, b = by_setting["train_bf16_store=2" if case.fmt == 2 else "default"], by_setting["train_tn_tr=0"]
        print(f"{case.id}: {a[0]} and {b[0]} dW bit-equal: {torch.equal(bits(a[1]), bits(b[1]))}")


# ---- 4: split-f16 operands --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mag", gc.SPLIT_MAGS)
@pytest.mark.parametrize("case", gc.SPLIT_CASES, ids=lambda c: c.id)
def test_split_route_against_float64(case, mag):
    """The transposed-copy route on split-f16 pairs (per-tap transposing im2col casts for a conv), and the split conv backward's bias
    gradient and dx (one GEMM over the output steps + col2im), at dY of size 1 and 1e-7: 3e-5 of the largest float64 entry."""
    ref = gc.reference(case, mag)
    branch = gc.expected_branch(case, None, cus())
    first = None
    for pitched in pitched_too(case):
        out = run(case, ref[0], pitched=pitched)
        assert_parity(case, branch, out, ref, f"mag {mag:g}" + (" pitched" if pitched else ""))
        if first is None:
            first = out
            same_bits(first, run(case, ref[0]), (case.id, "run twice"))
        else:
            same_bits(first, out, (case.id, "pitched against plain"))


# ---- 5: a scratch one byte short ------------------------------------------------------------------------------------------------------
SHORT_IDS = ["gemm_tn_129x132x260", "gemm_tn_600x1024x3072", "conv_bwd_r5_t33_32to64_k3s2p1", "gemm_tn_f16_200x256x256", "gemm_tn_bf16_100x264x72",
             "conv_wgrad_f16_r40_t16_256to256_k3s2p1", "gemm_tn_split_70x64x128", "conv_bwd_split_r9_t41_64to128_k3s2p1"]


@pytest.mark.parametrize("cid", SHORT_IDS)
def test_scratch_one_byte_short_is_refused_and_nothing_is_written(cid):
    assert {gc.BY_ID[i].entry for i in SHORT_IDS} == set(gc.ENTRIES)
    case = gc.BY_ID[cid]
    assert run(case, gc.make_inputs(case), short=1) is None


# ---- 6: the transposition catcher -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", gc.CATCHER_IDS)
def test_one_hot_rows_move_integers_to_known_places(cid):
    """dY of one-hot rows, X an asymmetric ramp of small integers: dW is a matrix of small integers, exact in every format and in f32 sums,
    so the f32 and f16 routes give it exactly (torch.equal); bfloat16 operands and split-f16 pairs are held to their bounds.  Pitched
    wherever the entry point takes a pitch."""
    case = gc.BY_ID[cid]
    ref = gc.reference(case, catcher=True)
    for switches in settings_of(case):
        branch = gc.expected_branch(case, switches, cus())
        out = run(case, ref[0], switches, pitched=case.entry in gc.PITCHED_ENTRIES)
        exact = torch.equal(out["dw"].cpu().double(), ref[1])
        print(f"{case.id} [{branch}] {gc.switch_id(switches)} catcher: dW exact: {exact}")
        if case.fmt == 1 or case.entry in ("gemm_tn", "conv_bwd"):
            assert exact, (case.id, branch, float((out["dw"].cpu().double() - ref[1]).abs().max()))
            if "db" in out:
                assert torch.equal(out["db"].cpu().double(), ref[2]), (case.id, branch, "db")
        assert_parity(case, branch, out, ref, gc.switch_id(switches) + " catcher")
