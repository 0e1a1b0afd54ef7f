"""Attention forward in f32 (sola_attention: sola_amd/csrc/attn.hip, attn_simple.hip, attn_reg.hip, attn_res.hip): the case table that
reaches every kernel the launcher can pick, a plain restatement of the launcher's choice, the float64 yardstick for o and the
log-sum-exp, and the two input variants that stress the running maximum.  The row addressing, the float64 forward and the one-hot
dropout probe are attn_bwd_cases.py's.  Shared by test_attn_fwd_cpu.py and test_gpu_attn_fwd.py."""
import collections
import functools

import torch

from attn_bwd_cases import (GAP_K, GAP_Q, ODD_SCALE, TP, addressing, case_scale, dropout_case, forward64, probe_collect,  # noqa: F401
                            probe_passes, probe_v, unit_rows)

Case = collections.namedtuple("Case", "id H DH G Sq Sk layout lse pitch scale")
# layout   consecutive / strided / gapped: attn_bwd_cases.py
# lse      True: the call asks for the log-sum-exp (the training forward)
# pitch    "plain": rows of D values; "packed": the case ALSO runs with q, k, v and o as column blocks of wider, fenced buffers
# scale    None = 1 / sqrt(DH)
LAYOUTS = ("consecutive", "strided", "gapped")

# the sola_tune keys of the route and their defaults (docs/tune_keys.md)
SWITCHES = {"attn_variant": 1, "attn_target_blocks": 512, "attn_reg": 1, "attn_res": 1, "attn_res_tiles": 0, "attn_res_shape": 0,
            "attn_simple_db": 1, "attn_simple_remap": 0, "attn_simple_train": 1}
SWITCH_SETTINGS = (
    {"attn_reg": 0}, {"attn_reg": 2}, {"attn_res": 0}, {"attn_res_shape": 2}, {"attn_res_tiles": 1}, {"attn_simple_db": 0},
    {"attn_simple_remap": 1}, {"attn_simple_train": 0}, {"attn_variant": 0}, {"attn_variant": 2}, {"attn_variant": 3},
    {"attn_target_blocks": 8}, {"attn_variant": 3, "attn_target_blocks": 8},
)
RESIDENT_BLOCKS = 512  # g_attn_resident_blocks (attn.hip): no sola_tune key
LDK_PAD = 4            # SOLA_ATTN_LDK_PAD (attn.hip)

DH_PATHS = [f"packed{n}" for n in range(5)] + ["wide", "res_loop", "res_all", "stream"]
BRANCHES = (["small1", "small2", "small4", "reg/p1", "reg/p2", "reg/p3+", "res8/c1", "res8/cN", "res4pf/c1", "res4pf/cN"] +
            [f"simple{dh}/{kind}/{q}" for dh in (128, 64) for kind in ("db", "single", "train") for q in ("q1", "q2+")] +
            [f"dh{dh}/{path}" for dh in (16, 32, 64, 128) for path in DH_PATHS])
# a branch name may end in "/capped" (attn.hip's shared kernels: more units than resident blocks, blocks walk the rest) or in "/remap"
# (attn_simple.hip under attn_simple_remap: another block order); base_branch() takes both off


def switch_id(switches):
    return ",".join(f"{k}={v}" for k, v in switches.items()) or "default"


def base_branch(branch):
    for tail in ("/capped", "/remap"):
        if branch.endswith(tail):
            branch = branch[:-len(tail)]
    return branch


def _ceil(a, b):
    return -(-a // b)


def reg_offsets_fit(Sk, k_rs, ld):
    """attention_reg_supported's guard: attn_reg.hip addresses a unit's key rows with 32-bit byte offsets from its first row.  Not
    reachable at test size (Sk * k_rs * ld * 4 >= 2^32 is a buffer of several gigabytes): test_attn_fwd_cpu.py checks this
    restatement on made-up numbers only."""
    return Sk * k_rs * ld * 4 < (1 << 32)


def expected_launch(case, switches=None, dropout=False, lse=None, ld=None):
    """(branch, launch parameters) of a sola_attention call of ``case`` under the sola_tune ``switches``: the kernel family and
    instantiation, and the grid and loop parameters the launcher derives.  A restatement of launch_attention, launch_dh (attn.hip),
    attention_small_supported, attention_simple_supported, launch_attention_small, launch_s with simple_grid (attn_simple.hip), attention_reg_supported
    (attn_reg.hip), attention_res_supported, launch_res and launch_attention_res (attn_res.hip): whoever edits one of those edits this.
    ``lse``: overrides case.lse; ``ld``: the larger of the k and v pitches (default: rows of D values)."""
    sw = dict(SWITCHES, **(switches or {}))
    lse = case.lse if lse is None else lse
    H, DH, G, Sq, Sk = case.H, case.DH, case.G, case.Sq, case.Sk
    ld = H * DH if ld is None else ld
    k_rs = addressing(case)[2][2]
    variant, units = sw["attn_variant"], G * H
    # launch_attention: the order of the tests is the order of the code
    if variant == 1 and not lse and not dropout and Sq <= 4 and Sk <= 4 and DH == 128:  # attention_small_supported -> launch_attention_small
        need = max(Sq, Sk)
        return f"small{1 if need <= 1 else 2 if need <= 2 else 4}", {"blocks": _ceil(units, 8), "units": units}
    reg = bool(sw["attn_reg"]) and not dropout and DH == 128 and not (Sq <= 4 and Sk <= 4) and reg_offsets_fit(Sk, k_rs, ld) and \
        (sw["attn_reg"] == 2 or (Sq <= 16 and Sk <= 16) or 64 < Sk <= 96)  # attention_reg_supported
    if variant == 1 and reg:  # launch_attention_reg
        passes, n_tasks = _ceil(Sk, 64), units * _ceil(Sq, 16)
        return f"reg/p{passes if passes < 3 else '3+'}", {"blocks": _ceil(_ceil(n_tasks, 4), 8) * 8, "n_tasks": n_tasks, "key_tile": 64}
    if variant == 1 and sw["attn_res"] and not dropout and DH == 128 and Sk <= 64 and Sq >= 128:  # attention_res_supported -> launch_attention_res
        pf = sw["attn_res_shape"] == 2
        nw, max_tiles = (4, 8) if pf else (8, 4)  # launch_res<4, 3, true> / launch_res<8, 4, false>
        if sw["attn_res_tiles"] > 0:
            tiles = sw["attn_res_tiles"]
        else:
            per_tile = nw * 16
            nch = _ceil(Sq, max_tiles * per_tile)
            tiles = _ceil(Sq, per_tile * nch)
        nchunk = _ceil(Sq, nw * 16 * tiles)
        return f"res{'4pf' if pf else '8'}/{'c1' if nchunk == 1 else 'cN'}", \
            {"blocks": _ceil(units * nchunk, 8) * 8, "nchunk": nchunk, "tiles_per_wave": tiles, "key_tile": 16}
    simple = (Sq > 16 or Sk > 16) and DH in (64, 128) and not ((lse or dropout) and not sw["attn_simple_train"])  # attention_simple_supported
    if simple and (variant == 2 or (variant == 1 and Sq <= 128 and Sk <= 128)):  # launch_attention_simple -> launch_s
        nqb = _ceil(Sq, 64)  # simple_grid
        blocks = units * nqb
        kind = "train" if lse or dropout else "db" if sw["attn_simple_db"] else "single"
        remap = bool(sw["attn_simple_remap"]) and blocks % 8 == 0
        return f"simple{DH}/{kind}/{'q1' if nqb == 1 else 'q2+'}" + ("/remap" if remap else ""), \
            {"blocks": blocks, "nqb": nqb, "key_tile": 32 if kind == "single" else 16}
    if DH not in (16, 32, 64, 128):  # attn_dispatch_dh
        raise ValueError(f"attention: head_dim {DH} unsupported")
    # launch_dh
    row_bytes = ((DH + LDK_PAD) + (DH + 4)) * 4
    if Sq <= 16 and Sk <= 16:  # the packed shape
        need, lg = max(Sq, Sk), 0
        while (1 << lg) < need:
            lg += 1
        if variant == 0:
            lg = 4
        tiles = _ceil(units, 16 >> lg)
        return f"dh{DH}/packed{lg}", {"blocks": _ceil(tiles, 4), "tiles": tiles}
    wide = variant != 0 and 64 < Sk <= 128 and 128 * row_bytes <= 160 * 1024
    qrows = 128 if wide else 64
    nqb = _ceil(Sq, qrows)
    r16 = (Sk + 15) & ~15
    kv_rows = 64 if variant == 0 else min(r16, qrows)
    qsplit = nqb
    if variant != 0 and Sk <= kv_rows:  # K/V resident: a block loops over q-blocks
        qsplit = max(1, min(nqb, _ceil(sw["attn_target_blocks"], units)))
    blocks = units * qsplit
    resident = RESIDENT_BLOCKS // 2 if wide else RESIDENT_BLOCKS
    capped = variant != 0 and blocks > resident
    path = "wide" if wide else "stream" if Sk > kv_rows else "res_loop" if qsplit < nqb else "res_all"
    return f"dh{DH}/{path}" + ("/capped" if capped else ""), \
        {"blocks": min(blocks, resident) if capped else blocks, "units": blocks, "nqb": nqb, "qsplit": qsplit, "kv_rows": kv_rows, "key_tile": 64}


def expected_branch(case, switches=None, dropout=False, lse=None, ld=None):
    return expected_launch(case, switches, dropout, lse, ld)[0]


def instantiation(branch):
    """The compiled kernel a branch name stands for (the attn.hip shapes: (head dim, "packed" | "shared4" | "shared8"))."""
    b = base_branch(branch)
    if not b.startswith("dh"):
        return b
    dh, path = b.split("/")
    return f"{dh}/{'packed' if path.startswith('packed') else 'shared8' if path == 'wide' else 'shared4'}"


def _c(Sq, Sk, G=5, H=8, DH=128, layout="consecutive", lse=False, pitch="plain", scale=None):
    name = f"dh{DH}_h{H}_g{G}_{Sq}x{Sk}_{layout}" + ("_lse" if lse else "") + ("_packed" if pitch == "packed" else "") + \
           ("" if scale is None else "_scale")
    return Case(name, H, DH, G, Sq, Sk, layout, lse, pitch, scale)


CASES = [
    # ---- attn_fwd_small_kernel<1 / 2 / 4> (head dim 128, no log-sum-exp): eight units per block; 25, 15 and 40 units = a partial last block
    _c(1, 1, H=5, pitch="packed"), _c(1, 1, G=16, layout="gapped"),
    _c(2, 2, layout="strided", scale=ODD_SCALE), _c(2, 1, G=3, H=5),
    _c(4, 4, G=16), _c(3, 2, layout="gapped", pitch="packed"), _c(1, 4, layout="strided", H=5), _c(4, 3),
    # ---- attn_fwd_f32_reg_kernel: 5..16 steps, or 65..96 keys (one and two passes of 64 keys)
    _c(5, 16, H=5, lse=True), _c(16, 16, layout="strided", pitch="packed"), _c(9, 3, layout="gapped", lse=True, pitch="packed"), _c(16, 5, scale=ODD_SCALE),
    _c(17, 65, lse=True, pitch="packed"), _c(200, 96, layout="gapped"), _c(128, 80, layout="strided", lse=True), _c(33, 96, H=5),
    # ... wherever it can run (attn_reg 2): three and four passes, and the few-keys shapes of attn_res.hip
    _c(20, 200, layout="gapped", lse=True), _c(64, 129, pitch="packed"), _c(130, 5, H=5),
    # ---- attn_fwd_f32_res_kernel: >= 128 queries against <= 64 keys; one chunk of up to 512 queries, or several
    _c(128, 1, H=5, lse=True), _c(129, 5, layout="gapped", pitch="packed", lse=True), _c(128, 64, scale=ODD_SCALE), _c(129, 64, layout="strided"),
    _c(200, 48), _c(200, 37, lse=True), _c(128, 48, layout="strided", lse=True),
    _c(520, 48, layout="strided"), _c(520, 5, lse=True, layout="gapped"), _c(1400, 64, G=3, lse=True, pitch="packed"), _c(1400, 1, G=3),
    # ---- attn_fwd_f32_simple_kernel<128>: up to 128 x 128 where neither of the above applies; one or two 64-query blocks, 16-key stages
    _c(17, 1), _c(1, 17, H=5), _c(63, 15, layout="strided"), _c(64, 16, pitch="packed"), _c(5, 128, scale=ODD_SCALE), _c(64, 31, H=5),
    _c(65, 17, layout="gapped", pitch="packed"), _c(128, 128, layout="strided"), _c(65, 33),
    # ... its training instantiation (log-sum-exp)
    _c(17, 33, lse=True), _c(63, 31, lse=True, H=5), _c(17, 16, lse=True, layout="strided"),
    _c(65, 128, lse=True, layout="gapped", pitch="packed"), _c(100, 17, lse=True, layout="strided"), _c(128, 115, lse=True),
    # ---- attn_fwd_f32_simple_kernel<64>
    _c(17, 33, DH=64), _c(64, 17, DH=64, H=5), _c(65, 16, DH=64, layout="gapped", pitch="packed"), _c(128, 1, DH=64, pitch="packed"),
    _c(63, 31, DH=64, lse=True, layout="strided"), _c(17, 15, DH=64, lse=True), _c(128, 128, DH=64, lse=True), _c(65, 33, DH=64, lse=True, layout="gapped"),
    # ---- attn.hip, the packed shape (<= 16 x <= 16): 16, 8, 4, 2 and one unit per 16-row tile; head dim 128 comes here with a log-sum-exp
    _c(1, 1, DH=16, H=5, pitch="packed"), _c(2, 1, DH=16, lse=True), _c(3, 4, DH=16, layout="gapped"), _c(5, 8, DH=16, layout="strided", lse=True),
    _c(16, 9, DH=16, pitch="packed", lse=True),
    _c(1, 1, DH=32, lse=True), _c(1, 2, DH=32, layout="strided"), _c(4, 3, DH=32, layout="gapped", pitch="packed", lse=True), _c(7, 5, DH=32, H=5),
    _c(12, 16, DH=32),
    _c(1, 1, DH=64, G=3, H=5), _c(2, 2, DH=64, pitch="packed"), _c(3, 3, DH=64, lse=True), _c(8, 6, DH=64, lse=True, layout="strided"),
    _c(16, 16, DH=64, layout="gapped"),
    _c(1, 1, lse=True, layout="gapped"), _c(2, 1, lse=True, pitch="packed"), _c(4, 4, lse=True, H=5), _c(3, 4, lse=True, layout="strided"),
    # ... a second case of every packing depth and head dim, the other layouts (head dim 128 at 5..16 steps: under attn_reg 0)
    _c(1, 1, DH=16, layout="strided", lse=True), _c(1, 2, DH=16, layout="gapped", pitch="packed"), _c(4, 4, DH=16, G=16), _c(6, 7, DH=16, H=5),
    _c(9, 16, DH=16, layout="gapped"),
    _c(1, 1, DH=32, layout="gapped", pitch="packed"), _c(2, 2, DH=32, lse=True, H=5), _c(3, 1, DH=32, G=16), _c(8, 8, DH=32, layout="strided", lse=True),
    _c(16, 10, DH=32, layout="gapped", pitch="packed"),
    _c(1, 1, DH=64, layout="strided", lse=True), _c(1, 2, DH=64, layout="gapped"), _c(4, 2, DH=64, H=5, pitch="packed"), _c(5, 7, DH=64, layout="gapped"),
    _c(11, 13, DH=64, lse=True, H=5),
    _c(1, 1, lse=True, H=5, pitch="packed"), _c(1, 2, lse=True, layout="strided"), _c(5, 8, lse=True, layout="gapped"), _c(7, 6, pitch="packed"),
    # ---- attn.hip, the shared shape at four waves, K/V resident (<= 64 keys): every q-block in a block of its own ...
    _c(17, 33, DH=16, layout="gapped", lse=True), _c(130, 5, DH=16, layout="strided", pitch="packed"), _c(20, 20, DH=32, H=5),
    _c(200, 48, DH=64, layout="strided", lse=True), _c(130, 64, DH=64), _c(65, 17, DH=32, layout="gapped", lse=True, pitch="packed"),
    # ... more units than resident blocks (560 > 512): blocks walk the rest
    _c(20, 20, DH=16, G=70),
    # ... a block walks several q-blocks (512 or more units of two to four q-blocks), capped and not
    _c(200, 20, DH=16, G=70, lse=True), _c(200, 20, DH=32, G=70), _c(65, 5, DH=32, G=64, lse=True, pitch="packed"), _c(65, 64, DH=16, G=64),
    # ---- ... at eight waves (65..128 keys): two 64-key tiles of a resident 128-row tile, 128-query blocks
    _c(17, 65, DH=16, lse=True, pitch="packed"), _c(130, 128, DH=32, layout="gapped"), _c(20, 70, DH=32, G=35, layout="strided"),
    _c(130, 100, DH=16, layout="gapped"), _c(130, 70, DH=64, lse=True, pitch="packed"),
    _c(129, 97, DH=64, layout="gapped"), _c(129, 97, G=40, lse=True), _c(129, 97, layout="gapped", pitch="packed"), _c(200, 128, H=5, lse=True),
    # ---- ... streaming 64-key tiles (more than 128 keys; more than 64 under attn_variant 0): online softmax
    _c(20, 129, DH=16, lse=True), _c(17, 200, DH=16, layout="strided", pitch="packed"), _c(20, 129, DH=16, G=70), _c(70, 200, DH=32, layout="gapped", lse=True), _c(17, 129, DH=32, H=5),
    _c(130, 129, DH=64, lse=True), _c(200, 200, DH=64, pitch="packed"), _c(130, 200, scale=ODD_SCALE), _c(200, 129, layout="strided", lse=True),
]
BY_ID = {c.id: c for c in CASES}

# ---- input variants: standard normal, and two that move the running maximum -----------------------------------------------------------
SPIKE = 6.0
SPIKED_IDS = ["dh128_h8_g5_17x65_consecutive_lse_packed",   # reg/p2: key 64, the only key of the second pass
              "dh128_h8_g5_65x17_gapped_packed",            # simple128/db: key 16, the only key of the second 16-key stage
              "dh64_h8_g5_63x31_strided_lse",               # simple64/train: keys 16..30
              "dh64_h8_g5_130x129_consecutive_lse",         # dh64/stream: key 128, the third 64-key tile
              "dh128_h8_g5_20x200_gapped_lse",              # dh128/stream: keys 192..199
              "dh128_h8_g5_129x97_gapped_packed",           # dh128/wide: keys 64..96
              "dh128_h8_g5_200x37_consecutive_lse"]         # res8: keys 32..36 (one softmax over three 16-key tiles)
SATURATED_IDS = ["dh128_h8_g5_200x96_gapped", "dh128_h8_g5_17x33_consecutive_lse", "dh64_h8_g5_17x33_consecutive",
                 "dh128_h8_g5_130x200_consecutive_scale", "dh16_h8_g5_17x65_consecutive_lse_packed", "dh128_h8_g5_520x48_strided"]
VARIANTS = [(BY_ID[i], "spiked") for i in SPIKED_IDS] + [(BY_ID[i], "saturated") for i in SATURATED_IDS]


def key_tile(case, switches=None):
    """Keys per step of the running maximum in the kernel the case takes (for attn_res.hip, whose softmax is one pass: its 16-key tiles)."""
    return expected_launch(case, switches)[1].get("key_tile")


def spikes(case):
    """[(query, key)] positions inside a unit: up to three queries, each with its own key in the LAST, PARTIAL key tile of the kernel
    the case takes under the default switches."""
    tile = key_tile(case)
    first = (case.Sk - 1) // tile * tile
    assert first < case.Sk and case.Sk - first < tile, (case.id, "the last tile is a whole one")
    queries = sorted({3 % case.Sq, case.Sq // 2, case.Sq - 1})[:case.Sk - first]
    return [(qi, first + j) for j, qi in enumerate(queries)]


@functools.lru_cache(maxsize=None)
def make_inputs(case, variant="normal", seed=0):
    """(q, k, v) float32 [rows, H * DH]; the rows no unit owns hold values too (nothing may read them into a result).
    spiked: in every unit, key row ``kj`` = SPIKE * query row ``qi`` for spikes(case); saturated: q and k times 8."""
    _, _, _, rq, rk = addressing(case)
    g = torch.Generator().manual_seed((((seed * 1009 + case.Sq) * 1009 + case.Sk) * 1009 + case.G * 131 + case.DH) * 7 + case.H)
    D = case.H * case.DH
    q, k, v = (torch.randn(r, D, generator=g) for r in (rq, rk, rk))
    if variant == "spiked":
        qi, ki = unit_rows(case)
        for i, j in spikes(case):
            k[ki[:, j]] = SPIKE * q[qi[:, i]]
    elif variant == "saturated":
        q, k = q * 8, k * 8
    else:
        assert variant == "normal"
    return q, k, v


def lse64(case, q, k):
    """float64 log-sum-exp of the scaled scores, [q rows, H] as the kernels write it; zero in rows no unit owns."""
    qi, ki = unit_rows(case)
    qh = q.double()[qi].reshape(case.G, case.Sq, case.H, case.DH)
    kh = k.double()[ki].reshape(case.G, case.Sk, case.H, case.DH)
    s = torch.einsum("gqhd,gkhd->gqhk", qh, kh) * case_scale(case)
    out = torch.zeros(q.shape[0], case.H, dtype=torch.float64)
    return out.index_put((qi.reshape(-1),), torch.logsumexp(s, dim=-1).reshape(-1, case.H))


@functools.lru_cache(maxsize=None)
def plain_reference(case, variant="normal"):
    """(inputs, o float64, lse float64) without dropout: computed once per case and variant, shared, never modified."""
    inputs = make_inputs(case, variant)
    return inputs, forward64(case, *inputs)[1], lse64(case, *inputs[:2])


O_BAR, LSE_BAR = 2e-5, 2e-4  # o: test_gpu_kernels.py's stage bar, relative to max(1, max |reference|); lse: absolute (test_attention_cross_shapes)


def o_ratio(got, want):
    return float((got.double() - want).abs().max()) / (O_BAR * max(1.0, float(want.abs().max())))


def lse_ratio(got, want):
    return float((got.double() - want).abs().max()) / LSE_BAR


# ---- dropout: one case of every kernel that can drop, every head dim of attn.hip's ----------------------------------------------------
DROPOUT_IDS = [
    "dh128_h8_g5_17x33_consecutive_lse", "dh128_h8_g5_65x17_gapped_packed", "dh64_h8_g5_63x31_strided_lse", "dh64_h8_g5_65x16_gapped_packed",
    "dh16_h8_g5_3x4_gapped", "dh32_h8_g5_12x16_consecutive", "dh64_h8_g5_2x2_consecutive_packed", "dh128_h5_g5_5x16_consecutive_lse",
    "dh128_h8_g5_1x1_gapped_lse", "dh16_h8_g5_5x8_strided_lse",
    "dh16_h8_g5_17x65_consecutive_lse_packed", "dh32_h8_g35_20x70_strided", "dh64_h8_g5_129x97_gapped", "dh128_h8_g5_129x97_gapped_packed",
    "dh16_h8_g5_17x33_gapped_lse", "dh32_h5_g5_20x20_consecutive", "dh64_h8_g5_130x64_consecutive", "dh128_h8_g5_200x48_consecutive",
    "dh16_h8_g64_65x64_consecutive", "dh32_h8_g64_65x5_consecutive_lse_packed",
    "dh16_h8_g5_20x129_consecutive_lse", "dh32_h8_g5_70x200_gapped_lse", "dh64_h8_g5_130x129_consecutive_lse", "dh128_h8_g5_20x200_gapped_lse",
]
DROPOUT_CASES = [dropout_case(BY_ID[i]) for i in DROPOUT_IDS]
# what the no-dropout call of a dropout case is run under so that it takes the kernel of the dropout call (the first that does)
SAME_KERNEL_SETTINGS = ({}, {"attn_reg": 0}, {"attn_res": 0}, {"attn_variant": 3})
