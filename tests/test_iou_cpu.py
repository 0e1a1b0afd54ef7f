"""iou_cases.py checked without a GPU: the case table reaches every branch of the mask-IoU launcher (and keeps doing so: a branch that
loses its cases fails here), every "iou_shape" setting moves cases, the restated limits and scratch sizes hold on made-up numbers, the
matrix-product reference equals the pair-by-pair oracle - and, on the BUILT code object, the ticket form of the one-launch kernel
waits for its row stores before the barrier in front of its ticket."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou_cases as ic  # noqa: E402
from oracle import iou_oracle  # noqa: E402

BIG = 1 << 40  # a scratch that never declines


def small(case):
    return (case.P + case.R) * case.H * case.W <= (1 << 20)


def test_case_ids_are_unique_and_cases_are_well_formed():
    ids = [c.id for c in ic.CASES]
    assert len(set(ids)) == len(ids)
    for c in ic.CASES:
        assert c.dtype in ("u8", "f32") and c.scratch in ("max", "abi") and c.fill in ("random", "ones") and c.offset in (0, 1)
        assert dict(c.switches).keys() <= ic.SWITCHES.keys()
        assert ic.case_route(c) in ic.BRANCHES, c.id
        assert (c.P + c.R) * c.h * c.w * (1 if c.dtype == "u8" else 4) <= 10 * (1 << 20) + (1 << 16), c.id  # the largest upload: 10 MB
        # the ABI's figure is always enough for the call; "max" is enough for the one-launch kernel too
        assert ic.scratch_bytes(c) >= ic.abi_scratch_bytes(c.P, c.R, c.H, c.W)
        assert c.scratch == "abi" or ic.scratch_bytes(c) >= ic.fused_scratch_bytes(c.R, c.H * c.W // 32)


def test_every_branch_is_reached():
    reach = {b: [] for b in ic.BRANCHES}
    for c in ic.CASES:
        reach[ic.case_route(c)].append(c.id)
    assert all(reach.values()), [b for b, ids in reach.items() if not ids]
    # both forms of every G at a ragged, a full and a one-over last group, on more than one chunk
    for G in (1, 2, 4):
        for form in ("pk", "ticket"):
            rest = {c.R % (ic.launch_shape(c)[0] * ic.launch_shape(c)[1]) for c in ic.CASES
                    if ic.case_route(c) == f"onepass/G{G}/{form}" and ic.launch_shape(c)[3] > 1 and ic.launch_shape(c)[0] * ic.launch_shape(c)[1] > 1}
            assert 0 in rest and 1 in rest and len(rest) >= 3, (G, form, rest)
    # under the default switches alone: everything but G = 4 (only "iou_shape" opens it) and the switched-off kernel
    default = {ic.case_route(c) for c in ic.CASES if not c.switches}
    assert default == set(ic.BRANCHES) - {"onepass/G4/pk", "onepass/G4/ticket", "decline/off", "decline/groups"}
    # what serves a declined call: each pack route of the fallback
    assert {ic.case_fallback(c) for c in ic.CASES if ic.case_route(c).startswith("decline/")} == set(ic.FALLBACKS)


# (id, branch, (G, nb, groups, chunks) or None, fallback or None): the shapes of the table take the route they were chosen for
TABLE = [
    ("p1_r1_64x96", "onepass/G1/pk", (1, 1, 1, 1), None), ("p4_r16_64x96", "onepass/G1/pk", (1, 1, 16, 1), None),
    ("p3_r17_64x96", "onepass/G2/pk", (2, 1, 9, 1), None), ("p2_r33_64x96", "onepass/G2/pk", (2, 2, 9, 1), None),
    ("p4_r129_64x96", "onepass/G2/pk", (2, 4, 17, 1), None), ("p2_r7_8x4", "onepass/G1/pk", (1, 1, 7, 1), None),
    ("p4_r5_546x960_ones", "onepass/G1/pk", (1, 1, 5, 32), None),
    ("p3_r24_128x160_shape28", "onepass/G1/pk", (1, 12, 2, 2), None), ("p4_r25_128x160_packed0_shape28", "onepass/G1/ticket", (1, 12, 3, 2), None),
    ("p4_r19_128x160_shape65", "onepass/G4/pk", (4, 1, 5, 2), None), ("p4_r23_128x160_packed0_shape67", "onepass/G4/ticket", (4, 3, 2, 2), None),
    ("p3_r18_128x160_packed0_shape35", "onepass/G2/ticket", (2, 3, 3, 2), None),
    ("p3_r17_64x96_shape49", "onepass/G2/pk", (2, 1, 9, 1), None), ("p3_r17_64x96_shape68", "onepass/G2/pk", (2, 1, 9, 1), None),
    ("p3_r17_64x96_shape32", "onepass/G2/pk", (2, 1, 9, 1), None),
    ("p3_r5_512x1024", "onepass/G1/ticket", (1, 1, 5, 32), None), ("p2_r3_720x1280", "onepass/G1/ticket", (1, 1, 3, 57), None),
    ("p2_r3_1024x2048", "onepass/G1/ticket", (1, 1, 3, 128), None), ("p4_r1025_32x32", "onepass/G2/ticket", (2, 4, 129, 1), None),
    ("p4_r16_64x96_packed0", "onepass/G1/ticket", (1, 1, 16, 1), None), ("p3_r33_128x160_packed0", "onepass/G2/ticket", (2, 2, 9, 2), None),
    ("p4_r129_192x256_packed0", "onepass/G2/ticket", (2, 4, 17, 3), None), ("p2_r40_256x300_packed0", "onepass/G2/ticket", (2, 2, 10, 5), None),
    ("p4_r17_64x96_fused0", "decline/off", None, "pair-stream"), ("p3_r7_64x96_f32", "decline/dtype", None, "generic"),
    ("p5_r9_64x96", "decline/P", None, "pair-stream"), ("p2_r5_64x96_from96x128", "decline/resample", None, "resample-lds"),
    ("p2_r5_64x96_from48x80", "decline/resample", None, "generic"), ("p3_r9_36x100", "decline/hw32", None, "generic"),
    ("p1_r2_1025x2048", "decline/chunks", (1, 1, 2, 129), "pair-stream"), ("p4_r1025_32x32_shape17", "decline/groups", (1, 1, 1025, 1), "pair-stream"),
    ("p3_r9_64x96_off1", "decline/align", None, "generic"), ("p4_r300_8x4_abi", "decline/scratch", None, "pair-stream"),
]


@pytest.mark.parametrize("cid,branch,shape,fb", TABLE, ids=[t[0] for t in TABLE])
def test_the_shapes_of_the_table_take_the_branch_they_were_chosen_for(cid, branch, shape, fb):
    c = ic.BY_ID[cid]
    assert ic.case_route(c) == branch
    if shape is not None:
        assert ic.launch_shape(c) == shape
    if fb is not None:
        assert ic.case_fallback(c) == fb


def test_every_shape_setting_moves_cases_and_bad_shapes_move_none():
    for G, nb in ic.SHAPES:
        s = 16 * G + nb
        mine = [c for c in ic.CASES if dict(c.switches).get("iou_shape") == s]
        moved = [c.id for c in mine if (ic.case_route(c), ic.launch_shape(c)[:2]) !=
                 (ic.case_route(c, {"iou_shape": 0}), ic.launch_shape(c, {"iou_shape": 0})[:2])]
        assert len(mine) >= 6 and len(moved) >= 4, (G, nb, moved)  # (all but (1, 1) at 16 prompts, the default shape there)
        assert {ic.launch_shape(c)[:2] for c in mine} == {(G, nb)}
        assert {ic.case_route(c) for c in mine} >= {f"onepass/G{G}/pk", f"onepass/G{G}/ticket"}
    for s in ic.BAD_SHAPES:
        assert not ic.valid_shape(s >> 4, s & 15)
        mine = [c for c in ic.CASES if dict(c.switches).get("iou_shape") == s]
        assert mine and all(ic.case_route(c) == ic.case_route(c, {"iou_shape": 0}) and
                            ic.launch_shape(c) == ic.launch_shape(c, {"iou_shape": 0}) for c in mine)
        for R in (1, 16, 17, 32, 33, 128, 129, 5000):
            assert ic.onepass_shape(R, s) == ic.onepass_shape(R)
    assert [ic.onepass_shape(R) for R in (1, 16, 17, 32, 33, 128, 129, 5000)] == [(1, 1), (1, 1), (2, 1), (2, 1), (2, 2), (2, 2), (2, 4), (2, 4)]
    assert sorted((G, nb) for G in range(8) for nb in range(16) if ic.valid_shape(G, nb)) == \
        [(1, n) for n in range(1, 13)] + [(2, n) for n in range(1, 7)] + [(4, n) for n in range(1, 4)]


def test_the_limits_of_the_route_on_made_up_numbers():
    def r(P=4, R=16, H=64, W=96, h=None, w=None, dtype="u8", aligned=True, scratch=BIG, **sw):
        return ic.route(P, R, H, W, H if h is None else h, W if w is None else w, dtype, aligned, scratch, sw)

    # 2^19 pixels: the 19-bit fields of the pair words
    assert r(H=1, W=(1 << 19) - 32) == "onepass/G1/pk" and r(H=1, W=1 << 19) == "onepass/G1/ticket"
    assert r(H=546, W=960) == "onepass/G1/pk" and r(H=512, W=1024) == "onepass/G1/ticket"
    # 128 chunks of 512 words
    assert r(H=1, W=32 * 512 * 128) == "onepass/G1/ticket" and r(H=1, W=32 * 512 * 128 + 32) == "decline/chunks"
    assert r(H=1024, W=2048) == "onepass/G1/ticket" and r(H=1025, W=2048) == "decline/chunks"
    # 1024 prompts: the pair-word ring; 1024 groups: a quarter of the ticket ring
    assert r(R=1024) == "onepass/G2/pk" and r(R=1025) == "onepass/G2/ticket"
    assert r(R=8192) == "onepass/G2/ticket" and r(R=8193) == "decline/groups"
    assert r(R=1024, iou_shape=17) == "onepass/G1/pk" and r(R=1025, iou_shape=17) == "decline/groups"
    assert r(R=12288, iou_shape=16 * 4 + 3) == "onepass/G4/ticket" and r(R=12289, iou_shape=16 * 4 + 3) == "decline/groups"
    # the packed form's own chunk limit (126: a 7-bit arrival count) cannot bind: fewer than 2^19 pixels are at most 32 chunks
    assert ic._ceil(((1 << 19) - 32) // 32, ic.OP_CHUNK) == 32 < ic.PK_MAX_CHUNKS
    # the order of the declines: each reason wins over all that follow it
    bad = {"iou_fused": 0}, {"dtype": "f32"}, {"P": 5}, {"h": 48}, {"H": 36, "W": 100}, {"H": 1025, "W": 2048}, {"R": 9000}, {"aligned": False}, {"scratch": 0}
    names = [b.split("/")[1] for b in ic.BRANCHES if b.startswith("decline/")]
    for i, name in enumerate(names):
        kw = {}
        for later in reversed(bad[i:]):
            kw.update(later)
        if "h" in kw and "H" in kw:
            kw["h"] = kw["H"] - 1
        assert r(**kw) == f"decline/{name}", (name, kw)
    assert r(w=95) == "decline/resample" and r(P=4) != "decline/P"
    # the scratch: exactly the restated byte count is enough, one byte fewer is not
    need = ic.fused_scratch_bytes(16, 64 * 96 // 32)
    assert need == (9 * 16 + 64) * 1 * 4 and r(scratch=need) == "onepass/G1/pk" and r(scratch=need - 1) == "decline/scratch"
    assert ic.fused_scratch_bytes(3, 65536) == (27 + 64) * 128 * 4 and ic.fused_scratch_bytes(3, 65537) == (27 + 64) * 129 * 4
    assert ic.abi_scratch_bytes(4, 300, 8, 4) == 256 + 1280 + 256 + 2560 and ic.abi_scratch_bytes(1, 1, 36, 100) == 2 * 512 + 2 * 256  # 113 words
    # many prompts on tiny masks: the ABI's figure is below the one-launch kernel's rows
    assert ic.abi_scratch_bytes(4, 300, 8, 4) < ic.fused_scratch_bytes(300, 1) and ic.abi_scratch_bytes(4, 16, 8, 4) >= ic.fused_scratch_bytes(16, 1)


def test_the_count_rows_of_every_block_shape_fit_the_scratch_bound():
    """mask_iou_fused_scratch_bytes sizes the rows as 9 R + 64 counts per chunk; the kernel writes groups x (5 G nb + 4)."""
    for G in (1, 2, 4):
        for nb in range(1, 13):
            if not ic.valid_shape(G, nb):
                continue
            GB = G * nb
            for R in range(1, 401):
                assert ic._ceil(R, GB) * (5 * GB + 4) <= 9 * R + 64, (G, nb, R)
    for R in (1, 16, 17, 33, 129, 400, 5000):  # and the default shapes
        G, nb = ic.onepass_shape(R)
        assert ic._ceil(R, G * nb) * (5 * G * nb + 4) <= 9 * R + 64


def test_the_fallback_restatement():
    f = ic.fallback
    assert f(5, 9, 64, 96, 64, 96, "u8", True) == "pair-stream" and f(5, 9, 64, 96, 64, 96, "u8", False) == "generic"
    assert f(60000, 5536, 8, 4, 8, 4, "u8", True) == "stream" and f(4, 9, 36, 100, 36, 100, "u8", True) == "generic"
    assert f(4, 9, 64, 96, 64, 96, "f32", True) == "generic"
    assert f(2, 5, 64, 96, 96, 128, "u8", True) == "resample-lds" and f(2, 5, 64, 96, 96, 128, "u8", True, {"pack_resample_lds": 0}) == "generic"
    assert f(2, 5, 64, 96, 48, 80, "u8", True) == "generic" and f(2, 5, 64, 96, 48, 80, "u8", True, {"pack_resample_lds": 2}) == "resample-lds"
    assert f(2, 5, 64, 100, 96, 128, "u8", True) == "generic"  # destination rows of whole words only
    assert f(2, 5, 8, 32, 8, 97, "u8", True, {"pack_resample_lds": 2}) == "generic" and f(2, 5, 8, 32, 8, 96, "u8", True, {"pack_resample_lds": 2}) == "resample-lds"
    assert f(2, 5, 8, 2048, 8, 4128, "u8", True, {"pack_resample_lds": 2}) == "generic"
    assert f(2, 5, 64, 96, 96, 128, "f32", True) == "resample-lds" and f(2, 5, 64, 96, 96, 128, "u8", False) == "generic"


def test_every_mask_set_has_its_edges():
    for c in ic.CASES:
        if not small(c):
            continue
        for which in (0, 1):
            A, B = ic.make_masks(c, which)
            assert A.shape == (c.P, c.H, c.W) and B.shape == (c.R, c.h, c.w) and A.dtype == B.dtype == (np.uint8 if c.dtype == "u8" else np.float32)
            assert not A.flags.writeable and not B.flags.writeable
            assert ic.make_masks(c, which)[0] is A  # made once
        A, B = ic.make_masks(c, 0)
        A1, B1 = ic.make_masks(c, 1)
        if c.R >= 2:
            assert not B[0].any() and B1[0].all()  # an empty mask; in the other set a full one
        if (c.h, c.w) == (c.H, c.W):
            e = ic.equal_index(c)
            assert np.array_equal(B[e] != 0, A[0] != 0) and A[0].any()
            if c.R >= 3:
                assert not np.array_equal(B[e], A[0])  # ... in other bytes
        if c.P >= 2:
            assert not A[c.P - 1, : c.H // 2].any()
        if c.R >= 3:
            assert len(np.unique(B)) > 2  # "set" is any non-zero byte
        ri, ru = ic.reference(c, 0)
        ri1, ru1 = ic.reference(c, 1)
        assert ri.shape == (c.P, c.R) and (ri != ri1).mean() > 0.5 and (ru != ru1).mean() > 0.5  # a stale count of the other set is a wrong count
    ones = ic.BY_ID["p4_r5_546x960_ones"]
    assert int(ic.reference(ones)[0].max()) == 546 * 960 == (1 << 19) - 128  # every 19-bit field at its largest


def test_counts_ref_equals_the_oracle(iou_golden):
    for c in ic.CASES:
        if not small(c) or c.P * c.R > 600:
            continue
        A, B = ic.make_masks(c)
        if (c.h, c.w) != (c.H, c.W):
            B = iou_oracle.nearest_resize(B, c.H, c.W)
        ri, ru = iou_oracle.iou_matrix(A, (B != 0).astype(np.uint8))
        inter, union = ic.reference(c)
        assert inter.dtype == union.dtype == np.int64
        np.testing.assert_array_equal(inter, ri)
        np.testing.assert_array_equal(union, ru)
    A = np.unpackbits(iou_golden["pair_A"], axis=-1)[..., :960]
    B = np.unpackbits(iou_golden["pair_B"], axis=-1)[..., :960]
    inter, union = ic.counts_ref(A, B)
    got = np.array([[iou_oracle.iou_from_counts(int(inter[p, r]), int(union[p, r])) for r in range(len(B))] for p in range(len(A))])
    np.testing.assert_array_equal(got, iou_golden["pair_iou"])
    ri, ru = iou_oracle.iou_matrix(A, B)
    np.testing.assert_array_equal(inter, ri)
    np.testing.assert_array_equal(union, ru)


def test_ticket_form_waits_for_its_row_stores_in_the_built_code_object():
    """mask_iou_onepass_kernel<G, false> (iou.hip): a block stores its count rows with agent-scope atomic stores (global_store_dword ...
    sc1), then all its threads meet at a barrier, then thread 0 takes the group's ticket - an atomic on ANOTHER address.  The block
    that takes the last ticket folds every row, so each row must have landed before its block's ticket can: the storing lanes wait
    (s_waitcnt vmcnt(0)) between the stores and that barrier.  A workgroup-scope release fence alone compiles to no such wait, so the
    BUILT code object is checked, in all three instantiations.  The packed form <G, true> carries its data in the atomic itself."""
    from test_host_cpu import _code_object_text
    dis, _ = _code_object_text("iou.o")
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:", dis, re.M)]
    bodies = {name: dis[at:(heads[i + 1][0] if i + 1 < len(heads) else len(dis))] for i, (at, name) in enumerate(heads)}
    for G in (1, 2, 4):
        for pk in (0, 1):
            assert sum(f"mask_iou_onepass_kernelILi{G}ELb{pk}E" in n for n in bodies) == 1, (G, pk)
        body = next(b for n, b in bodies.items() if f"mask_iou_onepass_kernelILi{G}ELb0E" in n)
        lines = body.split("\n")
        store = next((i for i, ln in enumerate(lines) if re.search(r"\bglobal_store_dword\s.*\bsc1\b", ln)), None)
        assert store is not None, f"G = {G}: no agent-scope row store"
        barrier = next(i for i in range(store, len(lines)) if "s_barrier" in lines[i])
        ticket = next(i for i in range(barrier, len(lines)) if re.search(r"\bglobal_atomic_add\s", lines[i]))
        assert store < barrier < ticket
        waits = [ln for ln in lines[store + 1:barrier] if "s_waitcnt" in ln and "vmcnt(0)" in ln]
        assert waits, f"G = {G}: no s_waitcnt vmcnt(0) between the row store and the barrier in front of the ticket:\n" + "\n".join(lines[store:barrier + 1])
