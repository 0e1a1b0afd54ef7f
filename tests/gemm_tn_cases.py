"""Weight-gradient GEMMs dW = dY^T X (sola_gemm_tn, sola_conv1d_cl_backward, sola_gemm_tn_f16, sola_conv1d_cl_wgrad_f16, sola_gemm_tn_split,
sola_conv1d_cl_backward_split: sola_amd/csrc/gemm_tn.hip, gemm_tn_f32p.hip, gemm_tn_tr.hip, gemm_tn_split.hip): the case table that reaches
every kernel and route the launchers can pick, a plain restatement of the launchers' choices and of the published scratch sizes, the float64
yardsticks, and the builder of NaN-fenced operands.  Shared by test_gemm_tn_cpu.py and test_gpu_gemm_tn.py."""
import collections
import functools
import math

import torch

Case = collections.namedtuple("Case", "id entry fmt M N K conv")
# entry   the C entry point: gemm_tn / conv_bwd (exact f32), gemm_tn_f16 / conv_wgrad_f16 (fmt 1 = f16, 2 = bfloat16 operands),
#         gemm_tn_split / conv_bwd_split (split-f16 pairs, fmt 0)
# M N K   the product: M reduction rows, dW [N, K]; a conv has M = R * T_out, N = cout, K = k * cin (column = tap * cin + ci)
# conv    None or (R, T_in, cin, cout, k, stride, pad)
ENTRIES = ("gemm_tn", "conv_bwd", "gemm_tn_f16", "conv_wgrad_f16", "gemm_tn_split", "conv_bwd_split")
PITCHED_ENTRIES = ("gemm_tn", "gemm_tn_f16", "gemm_tn_split")  # the entry points that take lda and ldb
PAD_A, PAD_B, FENCE_ROWS = 8, 12, 64  # pitched operands: lda = N + 8, ldb = K + 12 (multiples of 4, which is all the entry points demand)

# the sola_tune keys of the routes and their defaults (docs/tune_keys.md)
SWITCHES = {"gemm_tn_persist": 1, "gemm_tn_nw8": 1, "train_tn_tr": 1, "train_bf16_store": 3}
SWITCH_SETTINGS = ({"gemm_tn_persist": 0}, {"gemm_tn_nw8": 0}, {"train_tn_tr": 0}, {"train_bf16_store": 2})

BRANCHES = (["f32/tile/nw8", "f32/tile/nw4", "f32/persist", "f32/persist_conv"] +
            [f"{t}/{r}" for t in ("f16", "bf16") for r in ("tr", "tr_conv", "copy", "copy/conv")] + ["split/copy", "split/copy/conv"])
SLABS_BF16 = "/slabs_bf16"  # a bf16 tr branch may end in this (train_bf16_store 3: bfloat16 partial sums); base_branch() takes it off

MAX_ROWS, MAX_OUTPUTS = 6000, 1024 * 3072  # the size cap of a case


def switch_id(switches):
    return ",".join(f"{k}={v}" for k, v in switches.items()) or "default"


def base_branch(branch):
    return branch[:-len(SLABS_BF16)] if branch.endswith(SLABS_BF16) else branch


def _ceil(a, b):
    return -(-a // b)


def t_out(conv):
    R, T_in, cin, cout, k, s, p = conv
    return (T_in + 2 * p - k) // s + 1


def conv_gathers(conv):
    """The entry points' conv flag: a 1x1, stride 1, unpadded conv is a plain product."""
    return conv is not None and (conv[4] > 1 or conv[5] > 1 or conv[6] > 0)


# ---- gemm_tn.hip ---------------------------------------------------------------------------------------------------------------------
TB, TM = 128, 32


def tn_splits(M, N, K):
    tiles = _ceil(N, TB) * _ceil(K, TB)
    return max(1, min(_ceil(768, tiles), _ceil(M, 4 * TM)))


def colsum_scratch_bytes(segments, seg_rows, cols):
    return 0 if seg_rows <= 256 else min(64, _ceil(seg_rows, 128)) * segments * cols * 4


# ---- gemm_tn_f32p.hip ----------------------------------------------------------------------------------------------------------------
def _fill(tiles, splits, cus):
    items = tiles * splits
    return items / (_ceil(items, cus) * cus)


def gemm_tn_persist_plan(M, N, K, cus, sw):
    """(splits, fill of the grid, rounded down to a multiple of 8?) - splits 0 = not the persistent kernel's shape.
    The rounding is not reachable at test size on 256 CUs: with t tiles it needs t * (splits mod 8) <= 10.24 * rounds, and below 6000
    rows (at most 23 splits) that leaves multiples of 8 only; the first shape that rounds is (6400, 512, 512), 25 -> 24 splits.
    test_gemm_tn_cpu.py checks this restatement of it on that shape and on other CU counts."""
    if not sw["gemm_tn_persist"] or N % 256 or K % 128:
        return 0, 0.0, False
    tiles = (N // 256) * (K // 128)
    most = min(64, max(1, M // 256))
    best, best_eff = 0, 0.0
    for rounds in range(1, 5):
        splits = min(most, rounds * cus // tiles)
        if splits < 1:
            continue
        if _fill(tiles, splits, cus) > best_eff + 0.02:
            best_eff, best = _fill(tiles, splits, cus), splits
    if best_eff < 0.70:
        return 0, best_eff, False
    rounded = best >= 8 and best % 8 != 0 and _fill(tiles, best & ~7, cus) >= _fill(tiles, best, cus) - 0.04
    return (best & ~7 if rounded else best), best_eff, rounded


def gemm_tn_persist_splits(M, N, K, lda, ldb, conv, max_splits, cus, sw, aligned=True):
    """conv: None or (Cin, stride) of a gathering conv by geometry.  aligned: both operands start on 16 bytes."""
    best = gemm_tn_persist_plan(M, N, K, cus, sw)[0]
    if best <= 0 or lda % 4 or (conv is None and ldb % 4):
        return 0
    if conv is not None and (conv[0] % 128 or K % conv[0] or K // conv[0] > 8):
        return 0
    if not aligned:
        return 0
    best = min(best, max_splits)
    if best < 1:
        return 0
    mps = _ceil(_ceil(M, best), 32) * 32
    if mps * max(lda, conv[0] * max(1, conv[1]) if conv is not None else ldb) * 4 >= 0x7fffff00:  # 31-bit byte offsets inside a split
        return 0
    return best


def persist_launch(M, splits, cus):
    """launch_gemm_tn_f32_persist: (rows per split, splits used - no empty split -, xcd_order)."""
    mps = _ceil(_ceil(M, splits), 32) * 32
    used = _ceil(M, mps)
    return mps, used, int(used % 8 == 0 and cus % 8 == 0)


def gemm_tn_scratch_bytes(M, N, K, cus, sw):
    one_tile = tn_splits(M, N, K) * (N * K + N) * 4
    ps = gemm_tn_persist_plan(M, N, K, cus, sw)[0]
    return max(one_tile, ps * N * K * 4 + colsum_scratch_bytes(1, M, N) if ps > 0 else 0)


# ---- gemm_tn_split.hip, gemm_tn_tr.hip -----------------------------------------------------------------------------------------------
def gemm_tn_split_supported(M, N, K):
    return N % 8 == 0 and K % 8 == 0 and M >= 64


def geometry(M, pure):
    """(ksplit, Mp): the k ranges of the transposed-copy route and the row count its transposed operands are padded to."""
    ks = 16 if M >= 8192 else 8 if M >= 2048 else 4 if M >= 512 else 2
    q = (128 if pure else 64) * ks
    return ks, _ceil(M, q) * q


def gemm_tn_split_scratch_bytes(M, N, K):
    if not gemm_tn_split_supported(M, N, K):
        return 0
    ks, Mp = geometry(M, True)
    return (N * Mp + K * Mp + ks * N * K + 64) * 4


def conv_bwd_split_scratch_bytes(conv):
    R, T_in, cin, cout, k, s, p = conv
    M = R * t_out(conv)
    if R <= 0 or t_out(conv) <= 0 or cout % 128 or cin % 8 or not gemm_tn_split_supported(M, cout, k * cin):
        return 0
    up = lambda b: (b + 255) & ~255  # noqa: E731
    return up(gemm_tn_split_scratch_bytes(M, cout, k * cin)) + up(M * cout * 4) + up(k * cin * cout * 4) + up(M * k * cin * 4) + 256


def gemm_tn_tr_supported(M, N, K, lda, ldb, sw):
    return bool(sw["train_tn_tr"]) and N % 256 == 0 and K % 256 == 0 and lda % 8 == 0 and ldb % 8 == 0 and M >= 128


def gemm_tn_tr_geometry(M, N, K, max_ranges, cus):
    """(ranges allowed before the rounding, after it, ranges used - no empty range -, 64-row k-tiles per range)."""
    nkt = _ceil(M, 64)
    tiles = (N // 256) * (K // 256)
    ks = min(max(1, cus // max(1, tiles)), max_ranges, max(1, nkt // 2))
    allowed = ks
    if ks >= 8:
        ks &= ~7
    kper = _ceil(nkt, ks)
    return allowed, ks, _ceil(nkt, kper), kper


def row_major_route(case, ldb, sw):
    """launch_gemm_tn_split's choice of gemm_tn_tr.hip's kernel over the transposed copies (16-bit operands only)."""
    gathers = conv_gathers(case.conv)
    cin = case.conv[2] if gathers else 0
    rows_in = case.conv[0] * case.conv[1] if gathers else 0
    return case.fmt != 0 and ldb % 4 == 0 and gemm_tn_tr_supported(case.M, case.N, case.K, 8, 8, sw) and \
        (not gathers or (cin % 256 == 0 and ldb == cin and rows_in > 0))


# ---- the route of a call -------------------------------------------------------------------------------------------------------------
def expected_route(case, switches=None, cus=256, pitched=False):
    """(branch, info) of a call of ``case`` under the sola_tune ``switches`` on a device of ``cus`` compute units, with the scratch the
    entry point publishes.  info: "planned" and "used" split counts, the stated bytes ("prof": profiler category -> bytes of its ONE
    launch; "gemm_split*" = gemm_split + gemm_split256 together), "misc_launches" where the route fixes them, and what the branch was
    chosen for (rows per split, the last split's rows, xcd_order, ...).  A restatement of launch_gemm_tn (gemm_tn.hip),
    gemm_tn_persist_plan, gemm_tn_persist_splits, launch_gemm_tn_f32_persist (gemm_tn_f32p.hip), launch_gemm_tn_split, geometry
    (gemm_tn_split.hip), gemm_tn_tr_supported and gemm_tn_tr_geometry (gemm_tn_tr.hip): whoever edits one of those edits this."""
    sw = dict(SWITCHES, **(switches or {}))
    M, N, K = case.M, case.N, case.K
    gathers = conv_gathers(case.conv)
    lda = N + PAD_A if pitched else N
    ldb = case.conv[2] if case.conv else (K + PAD_B if pitched else K)
    if case.entry in ("gemm_tn", "conv_bwd"):
        if M <= 0 or N <= 0 or K <= 0 or N % 4 or K % 4 or lda % 4 or (not gathers and ldb % 4) or (gathers and (case.conv[2] % 4 or K % case.conv[2])):
            raise ValueError(f"gemm_tn: bad dims {case.id}")
        scratch = gemm_tn_scratch_bytes(M, N, K, cus, sw)
        if case.entry == "conv_bwd":
            scratch = max(scratch, 4 * N * K)
        cs_need = colsum_scratch_bytes(1, M, N)  # the entry points always ask for the bias gradient here
        room = min(64, (scratch - min(scratch, cs_need)) // (N * K * 4))
        ps = gemm_tn_persist_splits(M, N, K, lda, ldb, (case.conv[2], case.conv[5]) if gathers else None, room, cus, sw) if room >= 1 else 0
        if ps > 0:
            mps, used, xcd = persist_launch(M, ps, cus)
            plan = gemm_tn_persist_plan(M, N, K, cus, sw)
            return "f32/persist_conv" if gathers else "f32/persist", {
                "planned": ps, "used": used, "rows_per_split": mps, "last_rows": M - (used - 1) * mps, "xcd_order": xcd, "fill": plan[1],
                "rounded": plan[2], "prof": {"gemm_tn": 4.0 * (M * (N + K) + ps * N * K)}, "scratch": scratch}
        splits = tn_splits(M, N, K)
        mps = _ceil(_ceil(M, splits), TM) * TM
        return f"f32/tile/nw{8 if sw['gemm_tn_nw8'] else 4}", {
            "planned": splits, "used": splits, "rows_per_split": mps, "last_rows": max(0, M - (splits - 1) * mps), "tiles": _ceil(N, TB) * _ceil(K, TB),
            "fill": gemm_tn_persist_plan(M, N, K, cus, sw)[1], "prof": {"gemm_tn": 4.0 * (M * (N + K) + splits * N * K)}, "scratch": scratch}
    if not gemm_tn_split_supported(M, N, K) or lda % 4 or (gathers and K % case.conv[2]):
        raise ValueError(f"gemm_tn_split: bad dims {case.id}")
    kind = {0: "split", 1: "f16", 2: "bf16"}[case.fmt]
    scratch = conv_bwd_split_scratch_bytes(case.conv) if case.entry == "conv_bwd_split" else gemm_tn_split_scratch_bytes(M, N, K)
    ks, Mp = geometry(M, case.fmt != 0)
    if row_major_route(case, ldb, sw):
        allowed, rounded, used, kper = gemm_tn_tr_geometry(M, N, K, ks, cus)
        slabs_bf16 = case.fmt == 2 and sw["train_bf16_store"] >= 3 and K % 4 == 0
        return f"{kind}/tr" + ("_conv" if gathers else "") + (SLABS_BF16 if slabs_bf16 else ""), {
            "planned": allowed, "rounded": rounded, "used": used, "kper": kper, "last_ktiles": _ceil(M, 64) - (used - 1) * kper,
            "xcd_order": int(used % 8 == 0), "prof": {"gemm_split256": 2.0 * (M * N + M * K) + 4.0 * used * N * K}, "misc_launches": 3, "scratch": scratch}
    taps = K // case.conv[2] if gathers else 1
    width = 2.0 if case.fmt else 4.0
    return f"{kind}/copy" + ("/conv" if gathers else ""), {
        "planned": ks, "used": ks, "Mp": Mp, "prof": {"gemm_split256" if case.fmt else "gemm_split*": width * (N * Mp + K * Mp + N * K)},
        "misc_launches": 2 + taps if case.entry != "conv_bwd_split" else None, "scratch": scratch}


def expected_branch(case, switches=None, cus=256, pitched=False):
    return expected_route(case, switches, cus, pitched)[0]


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _name(entry, fmt):
    return entry if fmt == 0 else entry[:-len("f16")] + ("f16" if fmt == 1 else "bf16")


def _g(entry, M, N, K, fmt=0):
    return Case(f"{_name(entry, fmt)}_{M}x{N}x{K}", entry, fmt, M, N, K, None)


def _v(entry, R, T_in, cin, cout, k, s, p, fmt=0):
    conv = (R, T_in, cin, cout, k, s, p)
    return Case(f"{_name(entry, fmt)}_r{R}_t{T_in}_{cin}to{cout}_k{k}s{s}p{p}", entry, fmt, R * t_out(conv), cout, k * cin, conv)


F32_GEMMS = [(5, 4, 8), (129, 132, 260), (1024, 512, 768), (512, 1024, 3072), (600, 1024, 3072), (2048, 1024, 1024), (2000, 1024, 1024),
             (5400, 512, 768)]
F32_CONVS = [(64, 8, 1024, 1024, 3, 1, 1), (256, 33, 256, 512, 3, 2, 1), (5, 33, 32, 64, 3, 2, 1), (4, 1, 32, 64, 3, 2, 1), (7, 5, 128, 128, 1, 1, 0)]
F16_GEMMS = [(128, 256, 256), (200, 256, 256), (2048, 256, 768), (2100, 512, 256), (8200, 256, 512), (100, 264, 72), (127, 256, 256), (300, 256, 264)]
F16_CONVS = [(77, 9, 256, 256, 5, 1, 2), (40, 16, 256, 256, 3, 2, 1), (12, 20, 128, 128, 3, 2, 1)]
SPLIT_GEMMS = [(70, 64, 128), (520, 264, 72)]
SPLIT_CONVS = [(9, 41, 64, 128, 3, 2, 1), (33, 4, 512, 1024, 3, 1, 1)]

CASES = ([_g("gemm_tn", *s) for s in F32_GEMMS] + [_v("conv_bwd", *g) for g in F32_CONVS] +
         [_g("gemm_tn_f16", *s, fmt=f) for f in (1, 2) for s in F16_GEMMS] + [_v("conv_wgrad_f16", *g, fmt=f) for f in (1, 2) for g in F16_CONVS] +
         [_g("gemm_tn_split", *s) for s in SPLIT_GEMMS] + [_v("conv_bwd_split", *g) for g in SPLIT_CONVS])
BY_ID = {c.id: c for c in CASES}
F32_CASES = [c for c in CASES if c.entry in ("gemm_tn", "conv_bwd")]
F16_CASES = [c for c in CASES if c.fmt != 0]
SPLIT_CASES = [c for c in CASES if c.entry in ("gemm_tn_split", "conv_bwd_split")]

# one case per 16-bit route runs on gradient-sized dY (1e-4) - the data-dependent scale has work to do; the others on dY of size 1
GRADIENT_SIZED = {"gemm_tn_f16_2100x512x256", "gemm_tn_bf16_2100x512x256", "gemm_tn_f16_300x256x264", "gemm_tn_bf16_300x256x264",
                  "conv_wgrad_f16_r77_t9_256to256_k5s1p2", "conv_wgrad_bf16_r77_t9_256to256_k5s1p2",
                  "conv_wgrad_f16_r12_t20_128to128_k3s2p1", "conv_wgrad_bf16_r12_t20_128to128_k3s2p1"}
SPLIT_MAGS = (1.0, 1e-7)

# the transposition catcher: one case per route (every one with lda and ldb runs pitched)
CATCHER_IDS = ["gemm_tn_129x132x260", "gemm_tn_600x1024x3072", "conv_bwd_r256_t33_256to512_k3s2p1", "conv_bwd_r5_t33_32to64_k3s2p1",
               "gemm_tn_f16_2100x512x256", "gemm_tn_bf16_2100x512x256", "gemm_tn_f16_300x256x264", "gemm_tn_bf16_300x256x264",
               "conv_wgrad_f16_r40_t16_256to256_k3s2p1", "conv_wgrad_bf16_r40_t16_256to256_k3s2p1",
               "conv_wgrad_f16_r12_t20_128to128_k3s2p1", "conv_wgrad_bf16_r12_t20_128to128_k3s2p1",
               "gemm_tn_split_520x264x72", "conv_bwd_split_r9_t41_64to128_k3s2p1"]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _seed(case):
    return ((case.M * 1009 + case.N) * 1009 + case.K) * 7 + case.fmt + (sum(case.conv) if case.conv else 0)


@functools.lru_cache(maxsize=None)
def make_inputs(case, mag=1.0):
    """float32 (dy [M, N], x, w): x = [M, K] or the channels-last conv input [R * T_in, cin]; w = the conv weight in GEMM layout
    [cout, k * cin] (the dx of the two conv backwards), None elsewhere.  dy has size ``mag``."""
    g = torch.Generator().manual_seed(_seed(case))
    dy = torch.randn(case.M, case.N, generator=g) * mag
    if case.conv is None:
        return dy, torch.randn(case.M, case.K, generator=g), None
    R, T_in, cin, cout, k, s, p = case.conv
    return dy, torch.randn(R * T_in, cin, generator=g), torch.randn(cout, k * cin, generator=g) * 0.1


@functools.lru_cache(maxsize=None)
def catcher_inputs(case):
    """dy = one-hot rows (row m's one in column 7 m mod N), x = an asymmetric ramp of small integers (exact in f16 and bfloat16; every dW
    entry a sum of a few of them: exact in f32, and below 256 in size - exact in a bfloat16 partial sum too).  A swapped tile index, a
    transposed fragment or a wrong tap moves integers to other places."""
    dy = torch.zeros(case.M, case.N)
    dy[torch.arange(case.M), (7 * torch.arange(case.M)) % case.N] = 1.0
    rows, cols = (case.M, case.K) if case.conv is None else (case.conv[0] * case.conv[1], case.conv[2])
    x = ((3 * torch.arange(rows)[:, None] + 5 * torch.arange(cols)[None, :]) % 17 - 8).float()
    assert math.ceil(case.M / math.gcd(7, case.N) / case.N) * 8 * math.gcd(7, case.N) <= 256
    w = None if case.conv is None else make_inputs(case)[2]
    return dy, x, w


def fenced(mat, pitch=None, before=0, after=FENCE_ROWS):
    """(buffer, view): ``mat`` [rows, cols] inside a NaN-filled [before + rows + after, pitch] buffer - ``before`` and ``after`` fence rows
    and pitch - cols pad columns, all NaN; view = the rows and columns of ``mat`` (what the entry point is given: view.data_ptr(), pitch)."""
    rows, cols = mat.shape
    pitch = cols if pitch is None else pitch
    assert pitch >= cols
    buf = torch.full((before + rows + after, pitch), float("nan"), dtype=mat.dtype)
    view = buf[before:before + rows, :cols]
    view.copy_(mat)
    return buf, view


# ---- float64 yardsticks --------------------------------------------------------------------------------------------------------------
def im2col(x, conv):
    """[R * T_out, k * cin] float64 (column = tap * cin + ci) of the channels-last conv input x [R * T_in, cin]; zero outside the sequence."""
    R, T_in, cin, cout, k, s, p = conv
    To = t_out(conv)
    xp = torch.nn.functional.pad(x.double().reshape(R, T_in, cin), (0, 0, p, p))
    return torch.stack([xp[:, kk:kk + (To - 1) * s + 1:s, :] for kk in range(k)], dim=2).reshape(R * To, k * cin)


def operand_b(case, x):
    return x.double() if case.conv is None else im2col(x, case.conv)


def product64(case, dy, x):
    """(dW [N, K], db [N]) in float64."""
    return dy.double().t() @ operand_b(case, x), dy.double().sum(dim=0)


def dy_scale(dy):
    """cast.hip's data-dependent power of two: max |dY| into [2^13, 2^14)."""
    return 2.0 ** (13 - math.floor(math.log2(float(dy.abs().max()))))


def rounded_product64(case, dy, x):
    """float64 dW of the operands as the 16-bit routes see them: dY scaled by dy_scale and rounded to the format, X rounded."""
    dt = torch.float16 if case.fmt == 1 else torch.bfloat16
    sc = dy_scale(dy)
    return ((dy * sc).to(dt).double().t() @ operand_b(case, x.to(dt))) / sc


def conv_dx64(case, dy, w):
    """dx [R * T_in, cin] by float64 autograd through the oracle's channels-last conv."""
    from oracle import sola_oracle
    R, T_in, cin, cout, k, s, p = case.conv
    xt = torch.zeros(R, T_in, cin, dtype=torch.float64, requires_grad=True)
    wt = w.double().reshape(cout, k, cin).permute(0, 2, 1).contiguous()
    y = sola_oracle.conv1d_cl(xt, wt, torch.zeros(cout, dtype=torch.float64), s, p)
    y.backward(dy.double().reshape(y.shape))
    return xt.grad.reshape(R * T_in, cin)


@functools.lru_cache(maxsize=None)
def reference(case, mag=1.0, catcher=False):
    """(inputs, dW, db, dx or None) float64 - dW on the rounded operands for the 16-bit formats; computed once, shared, never modified."""
    inputs = catcher_inputs(case) if catcher else make_inputs(case, mag)
    dy, x, w = inputs
    dw, db = product64(case, dy, x)
    if case.fmt != 0:
        dw = rounded_product64(case, dy, x)
    dx = conv_dx64(case, dy, w) if case.entry in ("conv_bwd", "conv_bwd_split") else None
    return inputs, dw, db, dx


F32_BAR = 3e-5                     # tests/test_gpu_backward.py's assert_close, relative to max |reference|; the split-f16 route's too
F32_SLABS_BAR = 5e-6               # 16-bit operands, f32 partial sums: test_weight_gradient_gemm_on_row_major_16bit_operands
BF16_SLABS_BAR = 2.0 ** -7         # ... bfloat16 partial sums (train_bf16_store 3)
ROUNDING = {1: 2.0 ** -9, 2: 2.0 ** -6}  # how far the rounded-operand product may lie from the unrounded one (of max |reference|)


def bar(branch):
    if branch.startswith("f32/") or branch.startswith("split/"):
        return F32_BAR
    return BF16_SLABS_BAR if branch.endswith(SLABS_BF16) else F32_SLABS_BAR


def ratio(got, want, rel):
    """max |got - want| as a fraction of the bound rel * max |want|; every element."""
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got.double() - want).abs().max()) / (rel * max(1e-30, float(want.abs().max())))
