"""gemm_tn_cases.py checked without a GPU: the case table reaches every kernel and route of the weight-gradient GEMMs (and keeps doing so:
a branch that loses its cases fails here), each table row takes the branch and the split counts it was chosen for, every sola_tune setting
of the routes moves cases, the float64 yardsticks agree with plain loops, and the fence builder puts NaN where it says."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_tn_cases as gc  # noqa: E402

SETTINGS = ({},) + gc.SWITCH_SETTINGS


def test_case_ids_are_unique_and_cases_are_within_the_size_cap():
    ids = [c.id for c in gc.CASES]
    assert len(set(ids)) == len(ids)
    assert set(gc.CATCHER_IDS) <= set(ids) and gc.GRADIENT_SIZED <= set(ids) and len(set(gc.CATCHER_IDS)) == len(gc.CATCHER_IDS)
    for c in gc.CASES:
        assert c.entry in gc.ENTRIES and c.fmt == (0 if c.entry in ("gemm_tn", "conv_bwd", "gemm_tn_split", "conv_bwd_split") else c.fmt) and c.fmt in (0, 1, 2)
        if c.conv:
            R, T_in, cin, cout, k, s, p = c.conv
            assert (c.M, c.N, c.K) == (R * gc.t_out(c.conv), cout, k * cin) and gc.t_out(c.conv) >= 1
        # 16 row ranges need geometry()'s M >= 8192: the one shape above the row cap
        assert c.M <= gc.MAX_ROWS or (c.M, c.N, c.K) == (8200, 256, 512), c.id
        assert c.N * c.K <= gc.MAX_OUTPUTS, c.id
        assert 2 * c.M * c.N * c.K <= 2 ** 32, c.id  # about 4 GFLOP
    assert all(s.keys() <= gc.SWITCHES.keys() for s in gc.SWITCH_SETTINGS)


def test_every_branch_is_reached_twice_under_the_settings_that_can_reach_it():
    reach = {b: set() for b in gc.BRANCHES}
    slabs = set()
    for s in SETTINGS:
        for c in gc.CASES:
            b = gc.expected_branch(c, s)
            assert gc.base_branch(b) in reach, (c.id, s, b)
            reach[gc.base_branch(b)].add(c.id)
            if b.endswith(gc.SLABS_BF16):
                assert b.startswith("bf16/tr")
                slabs.add((gc.base_branch(b), c.id))
    for b, ids in reach.items():
        assert len(ids) >= 2, (b, ids)
    for b in ("bf16/tr", "bf16/tr_conv"):
        assert sum(x == b for x, _ in slabs) >= 2, b
    # under the default switches alone: everything but what only a switch opens
    default = {}
    for c in gc.CASES:
        default.setdefault(gc.expected_branch(c), []).append(c.id)
    single = {"f16/copy/conv", "bf16/copy/conv"}  # one case each by default; train_tn_tr 0 sends the tr_conv cases there
    assert {gc.base_branch(b) for b in default} == set(gc.BRANCHES) - {"f32/tile/nw4"}
    assert "bf16/tr" not in default and "bf16/tr_conv" not in default  # f32 partial sums of bfloat16 operands: train_bf16_store 2 only
    assert all(len(ids) >= 2 or b in single for b, ids in default.items()), default


# (case id, branch under the default switches at 256 CUs, what the row of the table was chosen for)
TABLE = [
    ("gemm_tn_5x4x8", "f32/tile/nw8", {"tiles": 1, "planned": 1, "last_rows": 5}),
    ("gemm_tn_129x132x260", "f32/tile/nw8", {"tiles": 6, "planned": 2, "rows_per_split": 96, "last_rows": 33}),
    ("gemm_tn_1024x512x768", "f32/tile/nw8", {"planned": 8, "rows_per_split": 128}),
    ("gemm_tn_512x1024x3072", "f32/persist", {"planned": 2, "used": 2, "fill": 0.75, "rows_per_split": 256}),
    ("gemm_tn_600x1024x3072", "f32/persist", {"planned": 2, "used": 2, "rows_per_split": 320, "last_rows": 280}),
    ("gemm_tn_2048x1024x1024", "f32/persist", {"planned": 8, "used": 8, "xcd_order": 1}),
    ("gemm_tn_2000x1024x1024", "f32/persist", {"planned": 7, "used": 7, "rows_per_split": 288, "last_rows": 272, "xcd_order": 0}),
    ("gemm_tn_5400x512x768", "f32/persist", {"planned": 21, "used": 19, "xcd_order": 0}),
    ("conv_bwd_r64_t8_1024to1024_k3s1p1", "f32/persist_conv", {"planned": 2, "used": 2}),
    ("conv_bwd_r256_t33_256to512_k3s2p1", "f32/persist_conv", {"planned": 17, "used": 17}),
    ("conv_bwd_r5_t33_32to64_k3s2p1", "f32/tile/nw8", {"tiles": 1}),
    ("conv_bwd_r4_t1_32to64_k3s2p1", "f32/tile/nw8", {"tiles": 1, "last_rows": 4}),
    ("conv_bwd_r7_t5_128to128_k1s1p0", "f32/tile/nw8", {"tiles": 1}),
    ("gemm_tn_f16_128x256x256", "f16/tr", {"used": 1, "last_ktiles": 2}), ("gemm_tn_bf16_128x256x256", "bf16/tr/slabs_bf16", {"used": 1}),
    ("gemm_tn_f16_200x256x256", "f16/tr", {"used": 2, "kper": 2}), ("gemm_tn_bf16_200x256x256", "bf16/tr/slabs_bf16", {"used": 2}),
    ("gemm_tn_f16_2048x256x768", "f16/tr", {"planned": 8, "used": 8, "xcd_order": 1}),
    ("gemm_tn_bf16_2048x256x768", "bf16/tr/slabs_bf16", {"planned": 8, "used": 8, "xcd_order": 1}),
    ("gemm_tn_f16_2100x512x256", "f16/tr", {"planned": 8, "rounded": 8, "used": 7, "xcd_order": 0}),
    ("gemm_tn_bf16_2100x512x256", "bf16/tr/slabs_bf16", {"rounded": 8, "used": 7}),
    ("gemm_tn_f16_8200x256x512", "f16/tr", {"planned": 16, "used": 15}), ("gemm_tn_bf16_8200x256x512", "bf16/tr/slabs_bf16", {"planned": 16, "used": 15}),
    ("gemm_tn_f16_100x264x72", "f16/copy", {}), ("gemm_tn_f16_127x256x256", "f16/copy", {}), ("gemm_tn_f16_300x256x264", "f16/copy", {}),
    ("gemm_tn_bf16_100x264x72", "bf16/copy", {}), ("gemm_tn_bf16_127x256x256", "bf16/copy", {}), ("gemm_tn_bf16_300x256x264", "bf16/copy", {}),
    ("conv_wgrad_f16_r77_t9_256to256_k5s1p2", "f16/tr_conv", {}), ("conv_wgrad_f16_r40_t16_256to256_k3s2p1", "f16/tr_conv", {}),
    ("conv_wgrad_bf16_r77_t9_256to256_k5s1p2", "bf16/tr_conv/slabs_bf16", {}), ("conv_wgrad_bf16_r40_t16_256to256_k3s2p1", "bf16/tr_conv/slabs_bf16", {}),
    ("conv_wgrad_f16_r12_t20_128to128_k3s2p1", "f16/copy/conv", {}), ("conv_wgrad_bf16_r12_t20_128to128_k3s2p1", "bf16/copy/conv", {}),
    ("gemm_tn_split_70x64x128", "split/copy", {"Mp": 128}), ("gemm_tn_split_520x264x72", "split/copy", {"planned": 4}),
    ("conv_bwd_split_r9_t41_64to128_k3s2p1", "split/copy/conv", {}), ("conv_bwd_split_r33_t4_512to1024_k3s1p1", "split/copy/conv", {}),
]


def test_every_table_row_takes_the_branch_it_was_chosen_for():
    assert {t[0] for t in TABLE} == set(gc.BY_ID)
    for cid, branch, want in TABLE:
        got_branch, info = gc.expected_route(gc.BY_ID[cid])
        assert got_branch == branch, (cid, got_branch)
        for k, v in want.items():
            assert info[k] == v, (cid, k, info[k], v)
    # a pitch changes no route (lda and ldb stay multiples of 4; the tr route casts into buffers of its own)
    for c in gc.CASES:
        if c.entry in gc.PITCHED_ENTRIES:
            for s in SETTINGS:
                a, b = gc.expected_route(c, s), gc.expected_route(c, s, pitched=True)
                assert a[0] == b[0] and a[1]["planned"] == b[1]["planned"] and a[1]["used"] == b[1]["used"], c.id
    # the tap of a 128-column tile of the one-tile conv cases changes inside a tile (Cin 32: four taps per tile) or not at all (k = 1)
    assert gc.BY_ID["conv_bwd_r5_t33_32to64_k3s2p1"].K == 96 and gc.BY_ID["conv_bwd_r7_t5_128to128_k1s1p0"].conv[4] == 1
    assert not gc.conv_gathers(gc.BY_ID["conv_bwd_r7_t5_128to128_k1s1p0"].conv)
    # ragged last k-tile of the tr cases: 200 rows = three whole 64-row k-tiles and 8 rows
    assert 200 % 64 == 8 and 2100 % 64 == 52 and 8200 % 64 == 8


def test_every_switch_setting_moves_at_least_two_cases():
    for s in gc.SWITCH_SETTINGS:
        moved = [c.id for c in gc.CASES if gc.expected_branch(c, s) != gc.expected_branch(c)]
        assert len(moved) >= 2, (s, moved)
    # what each one does to the cases it moves
    for c in gc.CASES:
        b = gc.expected_branch(c)
        if b.startswith("f32/persist"):
            assert gc.expected_branch(c, {"gemm_tn_persist": 0}) == "f32/tile/nw8"
        if b == "f32/tile/nw8":
            assert gc.expected_branch(c, {"gemm_tn_nw8": 0}) == "f32/tile/nw4"
        if "/tr" in b:
            want = gc.base_branch(b).replace("/tr_conv", "/copy/conv").replace("/tr", "/copy")
            assert gc.expected_branch(c, {"train_tn_tr": 0}) == want
        if b.endswith(gc.SLABS_BF16):
            assert gc.expected_branch(c, {"train_bf16_store": 2}) == gc.base_branch(b)


@pytest.mark.parametrize("cus", [304, 64, 256])
def test_the_restatement_gives_a_route_at_other_cu_counts(cus):
    for s in SETTINGS:
        for c in gc.CASES:
            branch, info = gc.expected_route(c, s, cus)
            assert gc.base_branch(branch) in gc.BRANCHES
            assert 1 <= info["used"] <= info["planned"] <= 64 and info["scratch"] > 0 and all(v > 0 for v in info["prof"].values())
            if branch.startswith("f32/persist"):  # the partial sums and the column-sum scratch behind them fit in what is published
                assert info["planned"] * c.N * c.K * 4 + gc.colsum_scratch_bytes(1, c.M, c.N) <= info["scratch"]
            if "/tr" in branch:
                assert (info["used"] - 1) * info["kper"] < -(-c.M // 64) <= info["used"] * info["kper"]  # launch_gemm_tn_tr's covering check


def test_planning_paths_that_no_case_of_test_size_reaches():
    sw = gc.SWITCHES
    # gemm_tn_persist_plan's rounding to a multiple of 8 (see its docstring)
    assert gc.gemm_tn_persist_plan(6400, 512, 512, 256, sw) == (24, 200 / 256, True)
    assert gc.gemm_tn_persist_plan(6399, 512, 512, 256, sw) == (24, 192 / 256, False)
    assert not any(gc.gemm_tn_persist_plan(c.M, c.N, c.K, 256, sw)[2] for c in gc.CASES)
    # gemm_tn_persist_splits: the conditions besides the plan
    ok = gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 3072, None, 64, 256, sw)
    assert ok == 2
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 3072, None, 1, 256, sw) == 1  # the scratch has room for one slab
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 3072, None, 64, 256, sw, aligned=False) == 0
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1026, 3072, None, 64, 256, sw) == 0
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 3074, None, 64, 256, sw) == 0
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 0, (1024, 1), 64, 256, sw) == 2
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 0, (192, 1), 64, 256, sw) == 0      # Cin % 128
    assert gc.gemm_tn_persist_splits(512, 1024, 1152, 1024, 0, (128, 1), 64, 256, sw) == 0      # nine taps
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 1 << 22, None, 64, 256, sw) == 0    # 256 rows x 16 MiB: past 31-bit offsets
    assert gc.gemm_tn_persist_splits(512, 1024, 3072, 1024, 0, (1024, 2048), 64, 256, sw) == 0  # ... through the conv stride


def _loop_product(dy, b):
    M, N = dy.shape
    K = b.shape[1]
    out = torch.zeros(N, K, dtype=torch.float64)
    for n in range(N):
        for k in range(K):
            acc = 0.0
            for m in range(M):
                acc += float(dy[m, n]) * float(b[m, k])
            out[n, k] = acc
    return out


def test_float64_yardsticks_agree_with_plain_loops():
    g = gc.Case("loop_gemm", "gemm_tn", 0, 7, 8, 12, None)
    dy, x, _ = gc.make_inputs(g)
    dw, db = gc.product64(g, dy, x)
    assert float((dw - _loop_product(dy, x)).abs().max()) <= 1e-13
    assert float((db - torch.tensor([sum(float(dy[m, n]) for m in range(7)) for n in range(8)], dtype=torch.float64)).abs().max()) <= 1e-13
    conv = (2, 5, 4, 8, 3, 2, 1)
    R, T_in, cin, cout, k, s, p = conv
    c = gc.Case("loop_conv", "conv_bwd", 0, R * gc.t_out(conv), cout, k * cin, conv)
    assert gc.t_out(conv) == 3
    dy, x, w = gc.make_inputs(c)
    # the im2col by its definition: row (r, to), column tap * cin + ci = x[r, to * s - p + tap, ci], zero outside the sequence
    cols = torch.zeros(c.M, c.K, dtype=torch.float64)
    outside = 0
    for r in range(R):
        for to in range(3):
            for tap in range(k):
                ti = to * s - p + tap
                if 0 <= ti < T_in:
                    cols[r * 3 + to, tap * cin:(tap + 1) * cin] = x[r * T_in + ti].double()
                else:
                    outside += 1
    assert outside == 2 * R  # per sequence: tap 0 of the first output step and tap 2 of the last (T_in 5, stride 2, pad 1)
    got = gc.im2col(x, conv)
    assert torch.equal(got, cols)
    for r in range(R):  # the taps outside the sequence are zero, and nothing else is
        assert float(got[r * 3, :cin].abs().max()) == 0.0 and float(got[r * 3 + 2, 2 * cin:].abs().max()) == 0.0
    assert int((got == 0).sum()) == 2 * R * cin
    dw, db = gc.product64(c, dy, x)
    assert float((dw - _loop_product(dy, cols)).abs().max()) <= 1e-13
    # dx[r, ti, ci] = sum over (to, tap) with to * s - p + tap = ti of dy[(r, to)] . w[:, tap * cin + ci]
    dx = torch.zeros(R * T_in, cin, dtype=torch.float64)
    for r in range(R):
        for to in range(3):
            for tap in range(k):
                ti = to * s - p + tap
                if 0 <= ti < T_in:
                    for ci in range(cin):
                        dx[r * T_in + ti, ci] += sum(float(dy[r * 3 + to, co]) * float(w[co, tap * cin + ci]) for co in range(cout))
    assert float((gc.conv_dx64(c, dy, w) - dx).abs().max()) <= 1e-13


@pytest.mark.parametrize("cid", ["gemm_tn_f16_200x256x256", "gemm_tn_bf16_200x256x256", "gemm_tn_f16_300x256x264", "gemm_tn_bf16_100x264x72",
                                 "conv_wgrad_f16_r40_t16_256to256_k3s2p1", "conv_wgrad_bf16_r12_t20_128to128_k3s2p1"])
def test_rounded_operand_references_stay_near_the_unrounded_product(cid):
    """The 16-bit routes are held to the product of the ROUNDED operands; that reference lies within the rounding's own bound of the
    unrounded float64 product (2^-9 of the largest entry for f16, 2^-6 for bfloat16), at size 1 and at gradient size: the routes' bounds
    (5e-6, 2^-7) test the kernels, not the rounding."""
    c = gc.BY_ID[cid]
    for mag in (1.0, 1e-4):
        dy, x, _ = gc.make_inputs(c, mag)
        exact = gc.product64(c, dy, x)[0]
        err = float((gc.rounded_product64(c, dy, x) - exact).abs().max()) / float(exact.abs().max())
        assert err <= gc.ROUNDING[c.fmt], (cid, mag, err)
        assert gc.dy_scale(dy) * float(dy.abs().max()) >= 2.0 ** 13 and gc.dy_scale(dy) * float(dy.abs().max()) < 2.0 ** 14


def test_catcher_inputs_are_exact_in_every_format():
    for cid in gc.CATCHER_IDS:
        c = gc.BY_ID[cid]
        (dy, x, w), dw, db, dx = gc.reference(c, catcher=True)
        assert torch.equal(dy.sum(dim=1), torch.ones(c.M)) and set(dy.unique().tolist()) == {0.0, 1.0}
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 8 and torch.equal(x.bfloat16().float(), x)
        assert torch.equal(dw, dw.round()) and float(dw.abs().max()) < 256 and torch.equal(dw.float().bfloat16().double(), dw.float().double().bfloat16().double())
        assert torch.equal(dw, gc.product64(c, dy, x)[0])  # rounding the operands changes nothing
        assert not torch.equal(dw[:min(c.N, c.K), :min(c.N, c.K)], dw[:min(c.N, c.K), :min(c.N, c.K)].t())  # asymmetric
    assert sum(gc.BY_ID[i].entry in gc.PITCHED_ENTRIES for i in gc.CATCHER_IDS) >= 1
    assert {gc.base_branch(gc.expected_branch(gc.BY_ID[i])) for i in gc.CATCHER_IDS} == set(gc.BRANCHES) - {"f32/tile/nw4"}


def test_fence_builder_puts_nan_in_the_pad_columns_and_fence_rows_only():
    mat = torch.arange(5 * 4, dtype=torch.float32).reshape(5, 4)
    buf, view = gc.fenced(mat, pitch=4 + gc.PAD_B, before=3)
    assert buf.shape == (3 + 5 + gc.FENCE_ROWS, 16) and torch.equal(view, mat) and view.data_ptr() == buf[3:].data_ptr() and view.stride() == (16, 1)
    nan = torch.isnan(buf)
    want = torch.ones_like(nan)
    want[3:8, :4] = False
    assert torch.equal(nan, want)
    buf, view = gc.fenced(mat)  # no pitch, no rows in front: 64 NaN rows behind
    assert buf.shape == (5 + 64, 4) and view.is_contiguous() and not torch.isnan(buf[:5]).any() and torch.isnan(buf[5:]).all()
