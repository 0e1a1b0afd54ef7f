"""GroupNorm forward and backward (sola_group_norm_ex, sola_group_norm_backward_ex: sola_amd/csrc/norm.hip, bwd.hip, gn_common.h): a Python
restatement of both shape ladders and of the format rules, the case tables that reach every kernel shape, row format and unit layout, the
inputs, the float64 references (oracle.sola_oracle.group_norm_tokens + leaky_relu, torch autograd for the backward), mutated float64 models
the bars have to tell from the truth, and the bars themselves.  Shared by test_gn_cpu.py and test_gpu_gn.py.

WHOEVER EDITS gn_common.h EDITS THIS: fwd_shape / bwd_shape restate gn_fwd_shape / gn_bwd_shape, formats_ok / bwd_formats_ok restate
kernels.h's group_norm_formats_ok / group_norm_bwd_formats_ok, bwd_reads_bf16_dy2 restates gn_bwd_reads_bf16_dy2 (test_gn_cpu.py holds
them to sola_group_norm_shape over a sweep)."""
import collections
import functools

import numpy as np
import torch

from oracle import sola_oracle

F32, SP16, F16, BF16 = 0, 1, 2, 3  # Elem codes (common.h)
FMT_NAME = {F32: "f32", SP16: "sp16", F16: "f16", BF16: "bf16"}
TORCH16 = {F16: torch.float16, BF16: torch.bfloat16}
WAVE, BLOCK, SLICED, THREE = 0, 1, 2, 3  # GnKind
KIND_NAME = {WAVE: "wave", BLOCK: "block", SLICED: "sliced", THREE: "three"}
SWITCHES = {"gn_variant": 1, "gn_wide": 1, "gn_slices": 1, "gn_h8": 1, "gn_bwd_reg": 1}  # the sola_tune keys and their defaults
GN_SLICE_R = 32
EPS, SLOPE = sola_oracle.GN_EPS, sola_oracle.LEAKY_SLOPE
F16_GUARD_LIMIT = 65000.0
DROP_P, DROP_SEED = 0.25, 0x5A17_0000_1234_5678  # (a seed with both halves set)


# ---- the ladders (gn_common.h) ---------------------------------------------------------------------------------------------------------
def gn_slots(ntok, lanes, lpt):
    return -(-ntok // (lanes // lpt)) if lanes % lpt == 0 else 1 << 30


def fwd_shape(ntok, cg, in_fmt=F32, out_fmt=F32, dropout=False, sw=None):
    """(kind, R, threads, channels per lane, slices) of gn_fwd_shape."""
    sw = dict(SWITCHES, **(sw or {}))
    three = (THREE, 0, 256, 4, 0)
    if not sw["gn_variant"]:
        return three
    f4 = cg // 4
    if sw["gn_h8"] and in_fmt == F16 and out_fmt == F16 and not dropout and cg % 8 == 0:
        f8 = cg // 8
        rw8, rb8, rk8 = gn_slots(ntok, 64, f8), gn_slots(ntok, 256, f8), gn_slots(ntok, 1024, f8)
        if rw8 <= 2:
            return (WAVE, rw8, 256, 8, 0)
        if rb8 <= 4:
            return (BLOCK, 2 if rb8 <= 2 else 4, 256, 8, 0)
        if rk8 <= 4:
            return (BLOCK, 4, 1024, 8, 0)
    rw, rb = gn_slots(ntok, 64, f4), gn_slots(ntok, 256, f4)
    if rw <= 4:
        return (WAVE, 4 if rw == 3 else rw, 256, 4, 0)
    if rb <= 16:
        return (BLOCK, 2 if rb <= 2 else 4 if rb <= 4 else 8 if rb <= 8 else 16, 256, 4, 0)
    if rb <= 32:
        return (BLOCK, 8, 1024, 4, 0) if sw["gn_wide"] and 1024 % f4 == 0 else (BLOCK, 32, 256, 4, 0)
    if sw["gn_slices"] and 256 % f4 == 0:
        return (SLICED, GN_SLICE_R, 256, 4, gn_slots(ntok, 256 * GN_SLICE_R, f4))
    return three


def bwd_shape(ntok, cg, sw=None):
    sw = dict(SWITCHES, **(sw or {}))
    f4 = cg // 4
    if not sw["gn_bwd_reg"] or f4 > 256:
        return (THREE, 0, 256, 4, 0)
    if f4 & (f4 - 1) == 0:
        rw = gn_slots(ntok, 64, f4) if f4 <= 64 else 1 << 30
        rb = gn_slots(ntok, 256, f4)
        if rw <= 4:
            return (WAVE, 4 if rw == 3 else rw, 256, 4, 0)
        if rb <= 8:
            return (BLOCK, 2 if rb <= 2 else 4 if rb <= 4 else 8, 256, 4, 0)
        if rb <= 16:
            return (BLOCK, 8, 512, 4, 0)
        if rb <= 32:
            return (BLOCK, 8, 1024, 4, 0)
    return (THREE, 0, 1024 if 1024 % f4 == 0 else 256, 4, 0)


def bwd_reads_bf16_dy2(shape):
    return not (shape[0] == BLOCK and shape[2] == 1024)


def formats_ok(in_fmt, out_fmt, cast_fmt):
    return in_fmt != SP16 and out_fmt != BF16 and (cast_fmt == F32 or (cast_fmt in (F16, BF16) and out_fmt == F32))


def bwd_formats_ok(x_fmt, dy2_fmt):
    return x_fmt in (F32, BF16) and dy2_fmt in (F32, BF16)


# every GN_REG instantiation of the two launchers, the sliced pair and the three-pass kernels, as (kind, R, threads, channels per lane)
FWD_KERNELS = ({(WAVE, r, 256, 4) for r in (1, 2, 4)} | {(BLOCK, r, 256, 4) for r in (2, 4, 8, 16, 32)} | {(BLOCK, 8, 1024, 4)} |
               {(WAVE, 1, 256, 8), (WAVE, 2, 256, 8), (BLOCK, 2, 256, 8), (BLOCK, 4, 256, 8), (BLOCK, 4, 1024, 8)} |
               {(SLICED, GN_SLICE_R, 256, 4), (THREE, 0, 256, 4)})
BWD_KERNELS = ({(WAVE, r, 256, 4) for r in (1, 2, 4)} | {(BLOCK, r, 256, 4) for r in (2, 4, 8)} | {(BLOCK, 8, 512, 4), (BLOCK, 8, 1024, 4)} |
               {(THREE, 0, 256, 4), (THREE, 0, 1024, 4)})


def shape_name(shape):
    kind, R, nthr, cpl, S = shape
    return KIND_NAME[kind] + (f"/R{R}" if R else "") + f"/{nthr}" + ("/h8" if cpl == 8 else "")


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id direction cg groups layout n_inst inner toks in_fmt out_fmt cast_fmt y2 leaky dropout in_scale "
                                      "dy2_fmt dx16 switches variants")
# direction "fwd" | "bwd".  layout: "rows" = n_inst instances of toks[0] consecutive tokens; "strided" = the (b, t') layout, instance
# i = (i / inner, i % inner) with its toks[0] tokens `inner` rows apart and pe row i % inner; "units" = a device int4 table, unit i of toks[i]
# tokens (mixed counts, strides 1 and 2, gaps of rows that belong to no unit, pe rows that are not i % inner).  in_fmt: the rows of x (the
# backward's x_fmt).  out_fmt / cast_fmt / y2 / in_scale: forward only.  dy2_fmt: None = no second gradient; dx16: backward only.
# switches: sola_tune settings of the case, a tuple of (key, value).  variants: the input variants the case runs on.
VARIANTS = {"wide": (0.3, 2.0), "offset": (30.0, 0.5), "tight": (0.3, 0.01)}  # x = mean + std * N(0, 1)
COMBOS = ((1, 1), (3, 1), (5, 1), (2, 3), (3, 2), (1, 8), (2, 2), (1, 3))  # (n_inst, groups): 1, 3, 5, 6, 6, 8, 4, 3 units per launch
LAYOUTS = ("rows", "units", "strided")


def _case(direction, cg, tok, i, in_fmt=F32, out_fmt=F32, cast_fmt=F32, y2=None, leaky=None, dropout=False, in_scale=None, dy2_fmt="auto",
          dx16=False, switches=(), variants=("wide", "offset"), layout=None):
    combos = [c for c in COMBOS if cg * c[1] <= 2048]
    n_inst, groups = combos[i % len(combos)]
    layout = layout or LAYOUTS[i % 3]
    inner, toks = 1, (tok,)
    if layout == "strided":
        if n_inst <= 2:
            n_inst = 4  # two outer steps of two instances: instance i reads pe row i % 2
        inner = n_inst if n_inst in (3, 5) else 2
    elif layout == "units":
        toks = (1, tok, max(1, tok // 3))
        n_inst = 3
    y2 = (i % 2 == 0) if y2 is None else y2
    leaky = (i % 4 != 3) if leaky is None else leaky
    if dy2_fmt == "auto":
        dy2_fmt = F32 if (direction == "bwd" and i % 2 == 0) else None
    sw = tuple(sorted(dict(switches).items()))
    cid = f"{direction}_cg{cg}_t{tok}_g{groups}_{layout}{n_inst}_{FMT_NAME[in_fmt]}"
    if direction == "fwd":
        cid += f"-{FMT_NAME[out_fmt]}" + (f"+{FMT_NAME[cast_fmt]}" if cast_fmt else "") + ("_pe" if y2 else "") + ("_scaled" if in_scale else "")
    else:
        cid += (f"_dy2{FMT_NAME[dy2_fmt]}" if dy2_fmt is not None else "") + ("_dx16" if dx16 else "")
    cid += ("_leaky" if leaky else "") + ("_drop" if dropout else "") + "".join(f"_{k}={v}" for k, v in sw)
    cid += "" if tuple(variants) == ("wide", "offset") else "_" + "+".join(variants)
    return Case(cid, direction, cg, groups, layout, n_inst, inner, toks, in_fmt, out_fmt, cast_fmt, bool(y2) and direction == "fwd", leaky,
                dropout, in_scale, dy2_fmt if direction == "bwd" else None, dx16, sw, tuple(variants))


def _ladder(direction, cg, toks, start=0, **kw):
    return [_case(direction, cg, t, start + j, **kw) for j, t in enumerate(toks)]


# token counts: every edge of the ladders with one token under it, on it and past it
T1024_F = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97)   # block R2 .. R16, 1024 threads, 2 / 3 / 4 slices of 32 tokens
T1024_B = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 100)               # block R2 R4 R8, 512, 1024 threads, three passes at 1024
T16_F = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)
T16_B = (15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)
T128_F = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 513)
T128_B = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300)
H8_128 = (3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257)                # wave R1 R2, block R2 R4, 1024 threads R4, past them
H8_16 = (32, 33, 64, 65, 256, 257, 512, 513, 2048)
H8_LEAVES = (4, 8, 32, 64, 65, 256)                                               # the same units leaving the h8 kernel
SHAPES_128 = (2, 4, 8, 9, 33, 100, 200, 300)   # one unit per forward shape at 128 channels per group: wave R1 R2 R4, block R2 R8 R16, 1024, sliced
SHAPES_128_B = (2, 4, 8, 16, 32, 64, 128, 256, 300)  # backward: wave R1 R2 R4, block R2 R4 R8, 512, 1024 threads, three passes

FWD_CASES = (
    _ladder("fwd", 1024, T1024_F) + _ladder("fwd", 16, T16_F) + _ladder("fwd", 128, T128_F) +
    _ladder("fwd", 8, (5, 33, 64, 65, 129)) + _ladder("fwd", 48, (1, 14, 21, 22, 43)) + _ladder("fwd", 24, (7, 43)) +
    # the wide shape switched off: R32 at 256 threads; the sliced shape switched off: three passes
    _ladder("fwd", 1024, (17, 31, 32), switches={"gn_wide": 0}) + _ladder("fwd", 16, (1025, 2048), 3, switches={"gn_wide": 0}) +
    _ladder("fwd", 128, (129, 256), 5, switches={"gn_wide": 0}) +
    _ladder("fwd", 1024, (33, 65), switches={"gn_slices": 0}) + _ladder("fwd", 128, (257,), 1, switches={"gn_slices": 0}) +
    # the eight-channel shapes (f16 rows in and out, no dropout), bfloat16 rows beside them, and the same units leaving the h8 kernel
    _ladder("fwd", 128, H8_128, in_fmt=F16, out_fmt=F16) + _ladder("fwd", 16, H8_16, 2, in_fmt=F16, out_fmt=F16) +
    _ladder("fwd", 8, (64, 65), 1, in_fmt=F16, out_fmt=F16) +
    _ladder("fwd", 128, H8_128, 1, in_fmt=BF16, out_fmt=F16) + _ladder("fwd", 16, (32, 65, 512), 4, in_fmt=BF16, out_fmt=F16) +
    _ladder("fwd", 128, H8_LEAVES, 2, in_fmt=F16, out_fmt=F16, switches={"gn_h8": 0}) +
    _ladder("fwd", 128, H8_LEAVES, 3, in_fmt=F16, out_fmt=F16, dropout=True) +
    _ladder("fwd", 128, H8_LEAVES, 4, in_fmt=F32, out_fmt=F16) +
    _ladder("fwd", 128, (4, 64), in_fmt=F16, out_fmt=F16, in_scale=0.25) +
    # the other formats on one unit per shape: 16-bit outputs, operand casts beside f32 outputs, 16-bit rows in, the input scale
    _ladder("fwd", 128, SHAPES_128, 0, out_fmt=SP16) + _ladder("fwd", 128, SHAPES_128, 1, in_fmt=F16, out_fmt=SP16, in_scale=4.0) +
    _ladder("fwd", 128, SHAPES_128, 2, out_fmt=F16) +
    _ladder("fwd", 128, SHAPES_128, 3, cast_fmt=F16, y2=True) + _ladder("fwd", 128, SHAPES_128, 4, in_fmt=BF16, cast_fmt=BF16, y2=True) +
    _ladder("fwd", 128, SHAPES_128, 5, in_fmt=F16) +
    _ladder("fwd", 1024, (2, 16, 32, 33, 97), 0, out_fmt=SP16) + _ladder("fwd", 1024, (4, 17, 65), 1, in_fmt=BF16, cast_fmt=BF16, y2=True) +
    _ladder("fwd", 8, (5, 33, 129), out_fmt=SP16) + _ladder("fwd", 48, (1, 14, 22), out_fmt=SP16) + _ladder("fwd", 24, (7,), out_fmt=SP16) +
    _ladder("fwd", 48, (14, 22), 1, in_fmt=F16, out_fmt=F16) + _ladder("fwd", 48, (14,), 2, in_fmt=BF16, cast_fmt=F16, y2=True) +
    # dropout on one unit per shape
    _ladder("fwd", 128, SHAPES_128, 6, dropout=True) + _ladder("fwd", 1024, (8, 32, 65), 2, dropout=True) + _ladder("fwd", 48, (14,), dropout=True) +
    _ladder("fwd", 16, (16, 64, 2049), 1, dropout=True) +
    # small-variance inputs: where eps sits shows
    _ladder("fwd", 128, (8, 100, 300), 7, variants=("tight",)) + _ladder("fwd", 48, (14,), 1, variants=("tight",)) +
    # 16-bit outputs (and their guard) in the shapes the ladders above reach with f32 rows only: block R4, and R32 with the wide shape off
    _ladder("fwd", 128, (20,), 8, out_fmt=SP16) + _ladder("fwd", 128, (200,), 1, out_fmt=SP16, switches={"gn_wide": 0}) +
    _ladder("fwd", 128, (200,), 2, out_fmt=F16, switches={"gn_wide": 0}) + _ladder("fwd", 1024, (20,), 3, out_fmt=SP16, switches={"gn_wide": 0}))

BWD_CASES = (
    _ladder("bwd", 1024, T1024_B) + _ladder("bwd", 16, T16_B) + _ladder("bwd", 128, T128_B) +
    _ladder("bwd", 8, (5, 33, 129)) + _ladder("bwd", 48, (1, 14, 22, 100)) + _ladder("bwd", 24, (1, 7, 43, 44)) +
    # bfloat16 x, a bfloat16 second gradient, dx once more as bfloat16 rows (the 1024-thread register shape reads no bfloat16 dy2)
    _ladder("bwd", 128, SHAPES_128_B, 1, in_fmt=BF16, dy2_fmt=F32, dx16=True) +
    _ladder("bwd", 128, [t for t in SHAPES_128_B if t != 256], 2, in_fmt=BF16, dy2_fmt=BF16, dx16=True) +
    _ladder("bwd", 128, (8, 64, 128, 300), 3, dy2_fmt=BF16) + _ladder("bwd", 1024, (4, 16, 40), 1, in_fmt=BF16, dy2_fmt=BF16, dx16=True) +
    _ladder("bwd", 1024, (32,), in_fmt=BF16, dy2_fmt=None, dx16=True) + _ladder("bwd", 24, (7, 44), 1, in_fmt=BF16, dy2_fmt=BF16, dx16=True) +
    # dropout on one unit per shape
    _ladder("bwd", 128, SHAPES_128_B, 4, dropout=True) + _ladder("bwd", 1024, (8, 16, 40), 2, dropout=True) + _ladder("bwd", 48, (14,), dropout=True) +
    _ladder("bwd", 128, (8, 300), 5, variants=("tight",)))

CASES = FWD_CASES + BWD_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [k for k, n in collections.Counter(c.id for c in CASES).items() if n > 1]


def ntok(case):
    return max(case.toks)


def channels(case):
    return case.cg * case.groups


def expected_shape(case, extra_switches=None):
    sw = dict(case.switches, **(extra_switches or {}))
    if case.direction == "fwd":
        return fwd_shape(ntok(case), case.cg, case.in_fmt, case.out_fmt, case.dropout, sw)
    return bwd_shape(ntok(case), case.cg, sw)


def three_pass_switch(case):
    return {"gn_variant": 0} if case.direction == "fwd" else {"gn_bwd_reg": 0}


Geometry = collections.namedtuple("Geometry", "units rows n_pe args owned")
# units: (first row, row stride, tokens, pe row) per instance; rows: rows of the matrix the units lie in; n_pe: rows of pe;
# args: (n_inst, inner, outer_stride, inner_stride, tok_stride, ntok) of the entry points; owned: bool [rows], the rows some unit owns


@functools.lru_cache(maxsize=None)
def geometry(case):
    t = case.toks[0]
    if case.layout == "rows":
        units = [(i * t, 1, t, 0) for i in range(case.n_inst)]
        rows, n_pe, args = case.n_inst * t, 1, (case.n_inst, 1, t, 0, 1, t)
    elif case.layout == "strided":
        inner = case.inner
        assert case.n_inst % inner == 0
        units = [((i // inner) * t * inner + i % inner, inner, t, i % inner) for i in range(case.n_inst)]
        rows, n_pe, args = case.n_inst * t, inner, (case.n_inst, inner, t * inner, 1, inner, t)
    else:
        units, row = [], 2  # two rows in front that belong to nobody
        for i, n in enumerate(case.toks):
            stride = 1 + i % 2
            units.append((row, stride, n, (2 * i + 1) % 3))
            row += (n - 1) * stride + 1 + (1, 3, 0)[i % 3]
        rows, n_pe, args = row + 1, 3, (len(units), 1, 0, 0, 1, max(case.toks))
    owned = torch.zeros(rows, dtype=torch.bool)
    for r0, st, n, _ in units:
        idx = r0 + st * torch.arange(n)
        assert not bool(owned[idx].any()) and int(idx[-1]) < rows
        owned[idx] = True
    return Geometry(tuple(units), rows, n_pe, args, owned)


def unit_rows(unit):
    r0, st, n, _ = unit
    return r0 + st * torch.arange(n)


def units_table(case):
    """The device int4 table of a "units" case (None for the strided layouts)."""
    if case.layout != "units":
        return None
    return torch.tensor(geometry(case).units, dtype=torch.int32)


# ---- dropout (common.h: make_dropout, dropout_keep) ------------------------------------------------------------------------------------
def dropout_scale():
    return float(np.float32(1.0 / (1.0 - float(np.float32(DROP_P)))))


def dropout_keep(rows, C):
    """bool [rows, C]: the elements a launch keeps; the mask is a pure function of (seed, element offset row * C + c)."""
    M = np.uint64(0xFFFFFFFF)
    idx = np.arange(rows * C, dtype=np.uint64)
    lo, hi = np.uint64(DROP_SEED & 0xFFFFFFFF), np.uint64(DROP_SEED >> 32)
    mul = lambda a, b: (a * np.uint64(b)) & M  # noqa: E731
    h = lo ^ mul(idx & M, 0x9E3779B1)
    h ^= h >> np.uint64(16); h = mul(h, 0x85EBCA6B); h ^= h >> np.uint64(13); h = mul(h, 0xC2B2AE35); h ^= h >> np.uint64(16)  # noqa: E702
    h ^= (hi + mul(idx >> np.uint64(32), 0x27D4EB2F)) & M
    h ^= h >> np.uint64(15); h = mul(h, 0x2C1B3C6D); h ^= h >> np.uint64(12); h = mul(h, 0x297A2D39); h ^= h >> np.uint64(15)  # noqa: E702
    thr = np.uint64(int((1.0 - float(np.float32(DROP_P))) * 4294967296.0))
    return torch.from_numpy((h < thr).reshape(rows, C))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
SIGN_MARGIN = 2e-4  # no pre-activation of a LeakyReLU case lies this close to zero: which side it is on is then the same in f32 and float64
MANTISSA = {F32: 23, F16: 10, BF16: 7}
Inputs = collections.namedtuple("Inputs", "x gamma beta pe dy dy2")
# x [rows, C] in the format under test (float32, float16 or bfloat16), NaN in the rows no unit owns; gamma, beta [C]; pe [n_pe, C];
# dy [rows, C] float32 and dy2 (float32 or bfloat16, or None): backward only, NaN in the rows no unit owns


def _stored(x, fmt):
    return x if fmt == F32 else x.to(TORCH16[fmt])


def _affine64(case, x64, gamma, beta):
    """(pre-activation [rows, C] float64 - zero in unowned rows -, statistics [n_inst * groups, 2] = (mean, rstd)): the reference's norm."""
    geo = geometry(case)
    out = torch.zeros_like(x64)
    stats = torch.zeros(len(geo.units) * case.groups, 2, dtype=torch.float64)
    for i, u in enumerate(geo.units):
        idx = unit_rows(u)
        xu = x64[idx]
        out[idx] = sola_oracle.group_norm_tokens(xu[None], gamma, beta, case.groups)[0]
        xg = xu.detach().reshape(len(idx), case.groups, case.cg)
        mean = xg.mean(dim=(0, 2))
        var = ((xg - mean[None, :, None]) ** 2).mean(dim=(0, 2))
        stats[i * case.groups:(i + 1) * case.groups, 0] = mean
        stats[i * case.groups:(i + 1) * case.groups, 1] = 1.0 / torch.sqrt(var + EPS)
    return out, stats


@functools.lru_cache(maxsize=None)
def make_inputs(case, variant):
    geo = geometry(case)
    C = channels(case)
    seed = sum(ord(ch) * (j + 1) for j, ch in enumerate(case.id + variant)) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    mean, std = VARIANTS[variant]
    scale = case.in_scale or 1.0
    x = _stored((mean + std * torch.randn(geo.rows, C, generator=g)) / scale, case.in_fmt)
    gamma = (0.5 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    beta = 0.3 * torch.randn(C, generator=g)
    pe = torch.randn(geo.n_pe, C, generator=g)
    if case.leaky:  # move the few elements whose pre-activation is about zero off it, by steps the row format can hold
        for _ in range(6):
            pre, _ = _affine64(case, x.double() * scale, gamma.double(), beta.double())
            amb = (pre.abs() < SIGN_MARGIN) & geo.owned[:, None]
            if not bool(amb.any()):
                break
            step = torch.maximum(3 * SIGN_MARGIN * std / gamma.abs()[None, :].expand_as(pre) / scale, 2 * x.float().abs() * 2.0 ** -MANTISSA[case.in_fmt])
            side = torch.where(pre >= 0, 1.0, -1.0) * torch.sign(gamma)[None, :]
            x = _stored(torch.where(amb, x.float() + (side * step).float(), x.float()), case.in_fmt)
        else:
            raise AssertionError(f"{case.id}: a pre-activation stays within {SIGN_MARGIN} of zero")
    x = x.clone()
    x[~geo.owned] = float("nan")
    dy = dy2 = None
    if case.direction == "bwd":
        dy = torch.randn(geo.rows, C, generator=g)
        dy[~geo.owned] = float("nan")
        if case.dy2_fmt is not None:
            dy2 = _stored(torch.randn(geo.rows, C, generator=g), case.dy2_fmt)
            dy2[~geo.owned] = float("nan")
    return Inputs(x, gamma, beta, pe, dy, dy2)


def x64_of(case, inp):
    """x as the kernel sees it (the stored rows widened, the input scale applied), float64, zeros in the rows no unit owns."""
    return torch.nan_to_num(inp.x.double(), nan=0.0) * (case.in_scale or 1.0)


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "y y2 stats")  # y, y2 [rows, C] float64 (NaN in unowned rows; y2 None without pe); stats (mean, rstd)
Backward = collections.namedtuple("Backward", "dx dgamma dbeta")


def _forward64(case, inp, x64):
    geo = geometry(case)
    pre, stats = _affine64(case, x64, inp.gamma.double(), inp.beta.double())
    y = sola_oracle.leaky_relu(pre) if case.leaky else pre
    if case.dropout:
        y = torch.where(dropout_keep(geo.rows, channels(case)), y * dropout_scale(), torch.zeros_like(y))
    pe_rows = torch.zeros(geo.rows, dtype=torch.long)
    for u in geo.units:
        pe_rows[unit_rows(u)] = u[3]
    y2 = y + inp.pe.double()[pe_rows]
    return y, y2, stats


@functools.lru_cache(maxsize=None)
def reference(case, variant):
    """Forward or Backward in float64 on the inputs as the format under test rounds them; computed once, shared, never modified."""
    geo = geometry(case)
    inp = make_inputs(case, variant)
    unowned = ~geo.owned
    if case.direction == "fwd":
        y, y2, stats = _forward64(case, inp, x64_of(case, inp))
        y, y2 = y.clone(), y2.clone()
        y[unowned] = float("nan")
        y2[unowned] = float("nan")
        return Forward(y, y2 if case.y2 else None, stats)
    x = x64_of(case, inp).requires_grad_(True)
    leaf = inp._replace(gamma=inp.gamma.double().requires_grad_(True), beta=inp.beta.double().requires_grad_(True))
    y, y2, _ = _forward64(case, leaf, x)
    loss = (y * torch.nan_to_num(inp.dy.double(), nan=0.0)).sum()
    if inp.dy2 is not None:
        loss = loss + (y2 * torch.nan_to_num(inp.dy2.double(), nan=0.0)).sum()
    loss.backward()
    dx = x.grad.clone()
    dx[unowned] = float("nan")
    return Backward(dx, leaf.gamma.grad, leaf.beta.grad)


# ---- mutated float64 models: what the bars must tell from the reference ----------------------------------------------------------------
FWD_MUTANTS = ("var_n_minus_1", "eps_outside_sqrt", "last_slice_full", "pe_row_inst", "last_token_dropped")
BWD_MUTANTS = ("leaky_on_x", "no_dy2")


def model64(case, variant, mutant=None):
    """The forward or backward written out in float64 with one mistake (``mutant``) - none: the reference itself, by other code."""
    geo = geometry(case)
    inp = make_inputs(case, variant)
    C, cg, G = channels(case), case.cg, case.groups
    x = x64_of(case, inp)
    gamma, beta = inp.gamma.double(), inp.beta.double()
    keep = dropout_keep(geo.rows, C) if case.dropout else None
    nan = torch.full((geo.rows, C), float("nan"), dtype=torch.float64)
    y, y2, dx = nan.clone(), nan.clone(), nan.clone()
    dgamma, dbeta = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    f4 = cg // 4
    ts = (256 // f4) * GN_SLICE_R if 256 % f4 == 0 else None  # tokens per slice of the sliced shape
    pe = inp.pe.double()
    if mutant == "pe_row_inst":  # rows behind pe's own: what a kernel reading row `inst` would find
        g = torch.Generator().manual_seed(7)
        pe = torch.cat([pe, torch.randn(len(geo.units), C, generator=g, dtype=torch.float64)])
    for i, u in enumerate(geo.units):
        idx = unit_rows(u)
        n = len(idx)
        xg = x[idx].reshape(n, G, cg)
        sg = xg[:-1] if (mutant == "last_token_dropped" and n > 1) else xg
        cnt = sg.shape[0] * cg
        if mutant == "last_slice_full" and ts is not None and n > ts:
            parts = [xg[a:a + ts] for a in range(0, n, ts)]
            w = [float(ts * cg)] * len(parts)  # the last slice weighted as a full one
            means = [p.mean(dim=(0, 2)) for p in parts]
            m2s = [((p - m[None, :, None]) ** 2).sum(dim=(0, 2)) for p, m in zip(parts, means)]
            mean = sum(m * (wi / (n * cg)) for m, wi in zip(means, w))
            var = sum(q + wi * (m - mean) ** 2 for q, m, wi in zip(m2s, means, w)) / (n * cg)
        else:
            mean = sg.sum(dim=(0, 2)) / cnt
            var = ((sg - mean[None, :, None]) ** 2).sum(dim=(0, 2)) / ((cnt - 1) if mutant == "var_n_minus_1" else cnt)
        rstd = 1.0 / (torch.sqrt(var) + EPS) if mutant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + EPS)
        xh = ((xg - mean[None, :, None]) * rstd[None, :, None]).reshape(n, C)
        pre = xh * gamma + beta
        act = torch.where(pre >= 0, pre, pre * SLOPE) if case.leaky else pre
        k = keep[idx].double() * dropout_scale() if keep is not None else 1.0
        y[idx] = act * k
        y2[idx] = act * k + pe[i if mutant == "pe_row_inst" else u[3]]
        if case.direction == "bwd":
            d = torch.nan_to_num(inp.dy[idx].double(), nan=0.0)
            if inp.dy2 is not None and mutant != "no_dy2":
                d = d + torch.nan_to_num(inp.dy2[idx].double(), nan=0.0)
            d = d * k
            if case.leaky:
                sign_of = x[idx] if mutant == "leaky_on_x" else pre
                d = torch.where(sign_of < 0, d * SLOPE, d)
            dgamma += (d * xh).sum(dim=0)
            dbeta += d.sum(dim=0)
            gg = (d * gamma).reshape(n, G, cg)
            xhg = xh.reshape(n, G, cg)
            m1 = gg.sum(dim=(0, 2)) / (n * cg)
            m2 = (gg * xhg).sum(dim=(0, 2)) / (n * cg)
            dx[idx] = (rstd[None, :, None] * (gg - m1[None, :, None] - xhg * m2[None, :, None])).reshape(n, C)
    if case.direction == "fwd":
        return Forward(y, y2 if case.y2 else None, None)
    return Backward(dx, dgamma, dbeta)


# ---- the float32 restatement the bar is measured on ------------------------------------------------------------------------------------
def model32(case, variant):
    """The two-pass formula (and the backward's) in numpy float32: a plain evaluation in the kernels' precision."""
    geo = geometry(case)
    inp = make_inputs(case, variant)
    f = np.float32
    C, cg, G = channels(case), case.cg, case.groups
    x = (torch.nan_to_num(inp.x.float(), nan=0.0).numpy() * f(case.in_scale or 1.0)).astype(f)
    gamma, beta, pe = inp.gamma.numpy(), inp.beta.numpy(), inp.pe.numpy()
    keep = dropout_keep(geo.rows, C).numpy() if case.dropout else None
    y, y2, dx = (np.full((geo.rows, C), np.nan, dtype=f) for _ in range(3))
    dgamma, dbeta = np.zeros(C, dtype=f), np.zeros(C, dtype=f)
    def gsum(t):  # [n, G, cg] -> [G]: each group's elements laid out in a row first, so that numpy adds them pairwise
        return np.ascontiguousarray(t.transpose(1, 0, 2)).reshape(G, -1).sum(axis=1, dtype=f)

    def csum(t):  # [n, C] -> [C], pairwise too
        return np.ascontiguousarray(t.T).sum(axis=1, dtype=f)

    for u in geo.units:
        idx = unit_rows(u).numpy()
        n = len(idx)
        cnt = f(n * cg)
        xg = x[idx].reshape(n, G, cg)
        mean = gsum(xg) / cnt
        cen = xg - mean[None, :, None]
        var = gsum(cen * cen) / cnt
        rstd = f(1.0) / np.sqrt(var + f(EPS))
        xh = (cen * rstd[None, :, None]).reshape(n, C)
        pre = xh * gamma + beta
        act = np.where(pre >= 0, pre, pre * f(SLOPE)) if case.leaky else pre
        k = (keep[idx] * f(dropout_scale())).astype(f) if keep is not None else f(1.0)
        y[idx] = act * k
        y2[idx] = act * k + pe[u[3]]
        if case.direction == "bwd":
            d = np.nan_to_num(inp.dy[idx].numpy(), nan=0.0)
            if inp.dy2 is not None:
                d = d + np.nan_to_num(inp.dy2[idx].float().numpy(), nan=0.0)
            d = (d * k).astype(f)
            if case.leaky:
                d = np.where(pre < 0, d * f(SLOPE), d)
            dgamma += csum(d * xh)
            dbeta += csum(d)
            gg = (d * gamma).reshape(n, G, cg)
            xhg = xh.reshape(n, G, cg)
            m1 = gsum(gg) / cnt
            m2 = gsum(gg * xhg) / cnt
            dx[idx] = (rstd[None, :, None] * (gg - m1[None, :, None] - xhg * m2[None, :, None])).reshape(n, C)
    if case.direction == "fwd":
        return Forward(torch.from_numpy(y), torch.from_numpy(y2) if case.y2 else None, None)
    return Backward(torch.from_numpy(dx), torch.from_numpy(dgamma), torch.from_numpy(dbeta))


# ---- bars ------------------------------------------------------------------------------------------------------------------------------
# F32_MEASURED: the worst max|error| / max|reference| of model32 over every case above, per direction and input variant (test_gn_cpu.py
# measures it again).  The bar of f32 rows in and out is 8 x that - room for other summation orders and the reciprocal square root.
# Per variant, because the error of the two-pass formula in float32 is the rounding of the mean, which grows with |mean| / std: it is
# measured about 14 times larger on "offset" (|mean| / std = 60) than on "wide" (0.15).  One number over all variants would be the "offset"
# one: no bar here is wider than that, the "wide" and "tight" ones are far narrower.
# A variance over n - 1 moves a unit of n elements by 1 / 2n of its largest entries: 1.5e-5 at 32k elements.  So wherever the largest unit
# of a case has LARGE_UNIT elements or more, the bar of every output that is normalised per unit - y, y2, dx - is CAPPED at
# LARGE_UNIT_BAR, under 1.2e-5, whatever 8 x the measured error comes to (f32_bar; on "offset" the cap is what holds).  dgamma and dbeta are
# sums over tokens and instances, not per-unit results: the float32 evaluation itself is 5e-6 off on "offset" at those sizes, and they keep
# 8 x the measured error.
F32_MEASURED = {("fwd", "wide"): 2.39e-7, ("fwd", "offset"): 3.30e-6, ("fwd", "tight"): 9.81e-7,
                ("bwd", "wide"): 2.42e-7, ("bwd", "offset"): 6.79e-6, ("bwd", "tight"): 1.35e-6}
F32_BAR = {k: 8.0 * v for k, v in F32_MEASURED.items()}
LARGE_UNIT, LARGE_UNIT_BAR = 16384, 1.19e-5  # elements; the bar a variance over n - 1 needs at units of this size and more
PER_UNIT_OUTPUTS = ("y", "y2", "dx")
ROUNDING = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8, SP16: 2.0 ** -21}  # of |reference|, per element (SP16: test_split_representation_has_22_bits)
FLOOR = {F32: 0.0, F16: 2.0 ** -25, BF16: 2.0 ** -134, SP16: 3.1e-8}      # underflow: half a subnormal step; the split pair's low half


def largest_unit(case):
    return ntok(case) * case.cg


def owned_max(ref):
    return max(1e-30, float(torch.nan_to_num(ref, nan=0.0).abs().max()))


def f32_bar(case, variant, name):
    """The bar of output ``name`` of the case on f32 rows, of max|reference|: 8 x the measured float32 error, capped where units are large."""
    bar = F32_BAR[(case.direction, variant)]
    if largest_unit(case) >= LARGE_UNIT and name in PER_UNIT_OUTPUTS:
        bar = min(bar, LARGE_UNIT_BAR)
    return bar


def ratio(got, ref, rel, fmt=F32):
    """max over the elements the reference has of |got - ref| / (rel max|ref| + ROUNDING[fmt] |ref| + FLOOR[fmt]); NaN in ``got`` = inf."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    have = ~torch.isnan(ref)
    g, r = got.double()[have], ref[have]
    if bool(torch.isnan(g).any()):
        return float("inf")
    bar = rel * owned_max(ref) + ROUNDING[fmt] * r.abs() + FLOOR[fmt]
    return float(((g - r).abs() / bar).max())


def rel_error(got, ref):
    """max |got - ref| / max |ref| over the elements the reference has."""
    have = ~torch.isnan(ref)
    return float((got.double()[have] - ref[have]).abs().max()) / owned_max(ref)


def outputs(case, res):
    """(name, tensor) of a Forward or Backward, those the case has."""
    if case.direction == "fwd":
        return [("y", res.y)] + ([("y2", res.y2)] if case.y2 else [])
    return [("dx", res.dx), ("dgamma", res.dgamma), ("dbeta", res.dbeta)]


def worst_ratio(case, variant, got, ref, fmt=F32):
    return max(ratio(g, r, f32_bar(case, variant, name), fmt) for (name, g), (_, r) in zip(outputs(case, got), outputs(case, ref)))


def decode_sp16(t):
    """Split-f16 rows (a float32 container, [8 x f16 hi | 8 x f16 lo] per 8 values) -> hi + lo, float64."""
    rows, K = t.shape
    h = t.contiguous().view(torch.float16).reshape(rows, K // 8, 2, 8).double()
    return (h[:, :, 0, :] + h[:, :, 1, :]).reshape(rows, K)
