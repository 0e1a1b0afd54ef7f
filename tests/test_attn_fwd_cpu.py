"""attn_fwd_cases.py checked without a GPU: the case table reaches every kernel the attention forward's launcher can pick (and keeps
doing so: a branch that loses its cases fails here), every sola_tune setting of the route moves cases, the float64 yardstick for o
and the log-sum-exp agrees with a plain per-unit loop, and the spiked and saturated inputs do to the softmax what they are there for."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fwd_cases as fc  # noqa: E402

SETTINGS = ({},) + fc.SWITCH_SETTINGS


def family(branch):
    b = fc.base_branch(branch)
    if b.startswith("small"):
        return "small"
    if b.startswith("res"):
        return "res"
    if b.startswith("dh"):
        return "dh/packed" if "/packed" in b else "dh/shared"
    return b.split("/")[0]  # reg, simple128, simple64


def test_case_ids_are_unique_and_cases_are_well_formed():
    ids = [c.id for c in fc.CASES]
    assert len(set(ids)) == len(ids)
    for c in fc.CASES:
        assert c.H in (5, 8) and c.DH in (16, 32, 64, 128) and c.layout in fc.LAYOUTS and c.pitch in ("plain", "packed") and c.lse in (True, False)
        assert c.scale is None or c.scale != 1 / math.sqrt(c.DH)
        inner, qa, ka, rq, rk = fc.addressing(c)
        qi, ki = fc.unit_rows(c)
        assert int(qi.max()) < rq and int(ki.max()) < rk
        assert rq <= 6000 or (c.G == 70 and c.Sq == 200 and c.DH <= 32), c.id  # the capped q-block loop needs 560 units of four q-blocks
        assert qi.unique().numel() == qi.numel() and ki.unique().numel() == ki.numel()  # no row belongs to two units
        if c.layout == "gapped":
            assert qi.numel() < rq and ki.numel() < rk
        else:
            assert qi.numel() == rq and ki.numel() == rk
    assert sum(c.G == 5 for c in fc.CASES) > len(fc.CASES) // 2
    assert all(s.keys() <= fc.SWITCHES.keys() for s in fc.SWITCH_SETTINGS)


def test_every_branch_is_reached_twice_under_the_settings_that_can_reach_it():
    reach = {b: set() for b in fc.BRANCHES}
    tails = {"/capped": set(), "/remap": set()}
    for s in SETTINGS:
        for c in fc.CASES:
            b = fc.expected_branch(c, s)
            assert fc.base_branch(b) in reach, (c.id, s, b)
            reach[fc.base_branch(b)].add(c.id)
            for t in tails:
                if b.endswith(t):
                    tails[t].add(c.id)
    for b, ids in {**reach, **tails}.items():
        assert len(ids) >= 2, (b, ids)
    # and under the default switches alone: everything but what only a switch opens
    default = {}
    for c in fc.CASES:
        default.setdefault(fc.base_branch(fc.expected_branch(c)), []).append(c.id)
    only_switched = {b for b in fc.BRANCHES if b == "reg/p3+" or b.startswith("res4pf") or "/single/" in b or
                     b in ("dh128/packed3", "dh128/packed4", "dh128/res_all", "dh128/res_loop", "dh64/res_loop")}
    assert set(default) == set(fc.BRANCHES) - only_switched
    assert all(len(ids) >= 2 for ids in default.values()), {b: ids for b, ids in default.items() if len(ids) < 2}
    assert sum(fc.expected_branch(c).endswith("/capped") for c in fc.CASES) >= 4


# (branch under the default switches, (Sq, Sk), what the case needs besides the shape)
TABLE = [
    ("small1", (1, 1), {"DH": 128, "lse": False}), ("small2", (2, 1), {"lse": False}), ("small4", (3, 2), {}), ("small4", (4, 4), {"DH": 128, "lse": False}),
    ("dh128/packed2", (4, 4), {"DH": 128, "lse": True}),
    ("reg/p1", (5, 16), {}), ("reg/p1", (16, 16), {"DH": 128}), ("reg/p2", (17, 65), {"DH": 128}), ("reg/p2", (200, 96), {}),
    ("res8/c1", (130, 5), {"DH": 128}), ("dh128/stream", (20, 200), {}),
    ("res8/c1", (128, 1), {"DH": 128}), ("res8/c1", (129, 5), {}), ("res8/cN", (520, 48), {}), ("res8/cN", (1400, 64), {}),
    ("simple128/db/q1", (17, 1), {}), ("simple128/db/q1", (63, 15), {}), ("simple128/db/q1", (64, 16), {}), ("simple128/db/q2+", (65, 17), {"DH": 128, "lse": False}),
    ("simple128/db/q2+", (128, 128), {"DH": 128, "lse": False}), ("simple128/db/q1", (64, 31), {}), ("simple128/train/q1", (17, 33), {"DH": 128, "lse": True}),
    ("dh16/res_all/capped", (20, 20), {"DH": 16, "G": 70}), ("dh32/wide/capped", (20, 70), {"DH": 32, "G": 35}), ("dh128/wide/capped", (129, 97), {"G": 40}),
    ("dh16/res_loop/capped", (200, 20), {"DH": 16}), ("dh32/res_loop/capped", (200, 20), {"DH": 32}),
    ("dh16/stream", (20, 129), {"DH": 16, "G": 5}), ("dh16/stream", (17, 200), {"DH": 16}), ("dh64/stream", (130, 129), {"DH": 64}), ("dh64/stream", (200, 200), {"DH": 64}),
    ("dh128/stream", (130, 200), {}), ("dh128/stream", (200, 129), {}),
]


@pytest.mark.parametrize("branch,shape,needs", TABLE, ids=[f"{b}-{s[0]}x{s[1]}" for b, s, _ in TABLE])
def test_the_shapes_of_the_table_take_the_branch_they_were_chosen_for(branch, shape, needs):
    needs = dict({"DH": 128}, **needs)
    found = [c for c in fc.CASES if (c.Sq, c.Sk) == shape and all(getattr(c, k) == v for k, v in needs.items())]
    assert found and all(fc.expected_branch(c) == branch for c in found), (branch, shape, [(c.id, fc.expected_branch(c)) for c in found])


def test_the_tail_shapes_of_every_family_are_in_the_table():
    def shapes(pred):
        return {(c.Sq, c.Sk) for c in fc.CASES if pred(fc.expected_branch(c))}

    simple = shapes(lambda b: b.startswith("simple"))
    assert {s[0] for s in simple} >= {17, 63, 64, 65, 128} and {s[1] for s in simple} >= {1, 15, 16, 17, 31, 33, 128}
    res = shapes(lambda b: b.startswith("res8"))
    assert {s[0] for s in res} >= {128, 129, 520, 1400} and {s[1] for s in res} >= {1, 5, 48, 64}
    assert shapes(lambda b: b.startswith("reg")) >= {(5, 16), (16, 16), (17, 65), (200, 96)}
    reg2 = {(c.Sq, c.Sk) for c in fc.CASES if fc.expected_branch(c, {"attn_reg": 2}).startswith("reg")}
    assert reg2 >= {(130, 5), (20, 200)}
    for dh in (16, 32, 64):  # a packed case with max(Sq, Sk) in each of {1, 2, 3..4, 5..8, 9..16}, and Sq != Sk among them
        packed = [c for c in fc.CASES if c.DH == dh and "/packed" in fc.expected_branch(c)]
        assert {fc.expected_branch(c)[-1] for c in packed} == set("01234") and any(c.Sq != c.Sk for c in packed)
    for dh in (16, 64, 128):
        assert {c.Sk for c in fc.CASES if fc.expected_branch(c) == f"dh{dh}/stream"} >= {129, 200}
    assert all(c.Sq > 128 for c in fc.CASES if fc.expected_branch(c) == "dh64/stream")


def test_every_switch_setting_changes_the_branch_of_at_least_two_cases():
    for s in fc.SWITCH_SETTINGS:
        moved = [c.id for c in fc.CASES if fc.expected_branch(c, s) != fc.expected_branch(c)]
        assert len(moved) >= 2, (s, moved)
    # what each setting is there to open
    def under(s):
        return {fc.base_branch(fc.expected_branch(c, s)) for c in fc.CASES}

    assert not any(b.startswith("reg") for b in under({"attn_reg": 0})) and "reg/p3+" in under({"attn_reg": 2})
    assert not any(b.startswith("res") for b in under({"attn_res": 0})) and "dh128/res_all" in under({"attn_res": 0})
    assert {"res4pf/c1", "res4pf/cN"} <= under({"attn_res_shape": 2}) and not any(b.startswith("res8") for b in under({"attn_res_shape": 2}))
    assert sum(fc.expected_launch(c, {"attn_res_tiles": 1})[1].get("nchunk", 0) > 8 for c in fc.CASES) >= 2
    assert {f"simple{dh}/single/{q}" for dh in (64, 128) for q in ("q1", "q2+")} <= under({"attn_simple_db": 0})
    assert not any("/train/" in b for b in under({"attn_simple_train": 0}))
    v0 = under({"attn_variant": 0})
    assert all(b.startswith("dh") and b.split("/")[1] in ("packed4", "res_all", "stream") for b in v0)
    assert all(b.startswith(("dh", "simple")) for b in under({"attn_variant": 2})) and all(b.startswith("dh") for b in under({"attn_variant": 3}))
    assert {"dh16/res_loop", "dh64/res_loop"} <= under({"attn_target_blocks": 8})
    assert "dh128/res_loop" in under({"attn_variant": 3, "attn_target_blocks": 8})


def test_layouts_pitches_and_five_heads_are_spread_over_the_families():
    fam = {}
    for c in fc.CASES:
        fam.setdefault(family(fc.expected_branch(c)), []).append(c)
    assert set(fam) == {"small", "reg", "res", "simple128", "simple64", "dh/packed", "dh/shared"}
    for name, cases in fam.items():
        assert {c.layout for c in cases} == set(fc.LAYOUTS), name
        assert any(c.pitch == "packed" for c in cases), name
        assert any(c.pitch == "packed" and c.layout == "gapped" for c in cases), name
        if name != "small":  # that kernel does not write one
            assert any(c.lse for c in cases) and any(not c.lse for c in cases), name
        if name != "simple64":
            assert any(c.H == 5 for c in cases), name
    for c in fc.CASES:
        if c.H == 5:
            assert (c.G * c.H) % 8, c.id  # a partial last block of eight units
    assert any(c.scale is not None for c in fam["small"] + fam["reg"]) and any(c.scale is not None for c in fam["simple128"] + fam["dh/shared"])


def test_the_offset_guard_of_the_register_shape():
    """attention_reg_supported refuses units whose key rows span 4 GiB or more; made-up numbers, no such buffer exists in a test."""
    assert fc.reg_offsets_fit(96, 1, 1024) and fc.reg_offsets_fit(200, 5, 4096)
    assert fc.reg_offsets_fit(1 << 10, 1 << 10, 1023) and not fc.reg_offsets_fit(1 << 10, 1 << 10, 1 << 10)  # 2^32 - 4096 bytes, 2^32
    big = fc._c(16, 16)
    assert fc.expected_branch(big) == "reg/p1" and fc.expected_branch(big, ld=1 << 26) == "dh128/packed4"
    wide = fc._c(17, 65, lse=True)
    assert fc.expected_branch(wide, ld=1 << 24) == "simple128/train/q1" and fc.expected_branch(wide, {"attn_reg": 2}, ld=1 << 24) == "simple128/train/q1"
    strided = fc._c(16, 16, layout="strided")  # the row stride counts: 16 * 5 * 2^24 * 4 >= 2^32, 16 * 1 * 2^24 * 4 < 2^32
    assert fc.expected_branch(strided, ld=1 << 24) == "dh128/packed4" and fc.expected_branch(big, ld=1 << 24) == "reg/p1"


def test_lse_and_dropout_move_the_cases_they_should():
    for c in fc.CASES:
        on, off = fc.expected_branch(c, lse=True), fc.expected_branch(c, lse=False)
        if off.startswith("small"):
            assert on == f"dh128/packed{(max(c.Sq, c.Sk) - 1).bit_length()}"
        elif off.startswith("simple"):
            assert "/db/" in off and on == off.replace("/db/", "/train/")
        else:
            assert on == off
        dropped = fc.expected_branch(c, dropout=True)
        assert dropped.startswith("dh") or "/train/" in dropped
    with pytest.raises(ValueError):
        fc.expected_branch(fc._c(4, 4, H=8, DH=24))


def test_the_dropout_cases_cover_every_kernel_that_can_drop():
    hit = {fc.base_branch(fc.expected_branch(c, dropout=True)) for c in fc.DROPOUT_CASES}
    assert {b.rsplit("/", 1)[0] for b in hit if b.startswith("simple")} == {"simple128/train", "simple64/train"}
    for dh in (16, 32, 64, 128):
        paths = {b.split("/")[1] for b in hit if b.startswith(f"dh{dh}/")}
        assert any(p.startswith("packed") for p in paths) and {"wide", "res_all", "stream"} <= paths, (dh, paths)
    assert {"dh16/res_loop", "dh32/res_loop"} <= hit
    assert {b[-1] for b in hit if "/packed" in b} == set("01234")
    for c, i in zip(fc.DROPOUT_CASES, fc.DROPOUT_IDS):
        assert c.G * c.H * c.Sq * c.Sk >= 4000 and fc.addressing(c)[3] <= 6000, c.id
        assert fc.instantiation(fc.expected_branch(c, dropout=True)) == fc.instantiation(fc.expected_branch(fc.BY_ID[i], dropout=True)), c.id
        # the no-dropout call can be made to take the same kernel: the log-sum-exp is compared bit for bit
        assert any(fc.expected_branch(c, s, lse=True) == fc.expected_branch(c, dropout=True) for s in fc.SAME_KERNEL_SETTINGS), c.id


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def loop_reference(case, q, k, v):
    """o and lse unit by unit, head by head, row by row, in float64 with Python's own exp and log."""
    qi, ki = fc.unit_rows(case)
    q, k, v = (t.double() for t in (q, k, v))
    o = torch.zeros_like(q)
    lse = torch.zeros(q.shape[0], case.H, dtype=torch.float64)
    for g in range(case.G):
        for h in range(case.H):
            cols = slice(h * case.DH, (h + 1) * case.DH)
            for i in qi[g].tolist():
                s = [float(q[i, cols] @ k[j, cols]) * fc.case_scale(case) for j in ki[g].tolist()]
                m = max(s)
                e = [math.exp(x - m) for x in s]
                lse[i, h] = m + math.log(sum(e))
                o[i, cols] = sum((w / sum(e)) * v[j, cols] for w, j in zip(e, ki[g].tolist()))
    return o, lse


@pytest.mark.parametrize("case", [fc.Case("tiny_consecutive", 2, 4, 3, 3, 5, "consecutive", True, "plain", None),
                                  fc.Case("tiny_strided", 3, 8, fc.TP, 2, 3, "strided", True, "plain", 0.3),
                                  fc.Case("tiny_gapped", 2, 4, 2, 4, 2, "gapped", True, "plain", None)], ids=fc.LAYOUTS)
def test_reference_equals_a_plain_loop_over_units(case):
    inputs, o, lse = fc.plain_reference(case)
    want_o, want_lse = loop_reference(case, *inputs)
    assert o.dtype == lse.dtype == torch.float64 and lse.shape == (inputs[0].shape[0], case.H)
    assert float((o - want_o).abs().max()) <= 1e-14 and float((lse - want_lse).abs().max()) <= 1e-14
    assert float(want_o.abs().max()) > 0.3
    if case.layout == "gapped":
        free = torch.ones(o.shape[0], dtype=torch.bool).index_fill(0, fc.unit_rows(case)[0].reshape(-1), False)
        assert int(free.sum()) == case.G * fc.GAP_Q and not o[free].any() and not lse[free].any()


# ---- the input variants ---------------------------------------------------------------------------------------------------------------
def test_variants_are_one_of_each_kind_per_family_with_a_running_maximum():
    for kind in ("spiked", "saturated"):
        fams = [family(fc.expected_branch(c)) for c, v in fc.VARIANTS if v == kind]
        assert {"reg", "res", "dh/shared"} <= set(fams) and any(f.startswith("simple") for f in fams), (kind, fams)
        paths = {fc.base_branch(fc.expected_branch(c)).split("/")[1] for c, v in fc.VARIANTS if v == kind and fc.expected_branch(c).startswith("dh")}
        assert {"stream", "wide"} <= paths, (kind, paths)
        assert any(fc.expected_branch(c) in ("reg/p2", "reg/p3+") for c, v in fc.VARIANTS if v == kind)


@pytest.mark.parametrize("case", [c for c, v in fc.VARIANTS if v == "spiked"], ids=lambda c: c.id)
def test_a_spiked_key_sits_in_the_last_partial_tile_and_takes_its_row(case):
    q, k, v = fc.make_inputs(case, "spiked")
    P, _ = fc.forward64(case, q, k, v)
    tile = fc.key_tile(case)
    n_tiles = -(-case.Sk // tile)
    assert case.Sk % tile and (n_tiles > 1 or fc.expected_branch(case).startswith("res"))
    for qi, kj in fc.spikes(case):
        assert kj // tile == n_tiles - 1 and kj < case.Sk
        assert float(P[:, :, qi, kj].min()) > 0.9, (case.id, qi, kj, float(P[:, :, qi, kj].min()))
    plain = fc.forward64(case, *fc.make_inputs(case))[0]
    assert float(plain.max(-1).values.median()) < 0.6  # what the standard normal inputs give


@pytest.mark.parametrize("case", [c for c, v in fc.VARIANTS if v == "saturated"], ids=lambda c: c.id)
def test_saturated_rows_are_close_to_one_hot(case):
    P, _ = fc.forward64(case, *fc.make_inputs(case, "saturated"))
    top = P.max(-1).values
    assert float((top > 0.99).double().mean()) > 0.5, (case.id, float((top > 0.99).double().mean()))
