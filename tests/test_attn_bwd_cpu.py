"""attn_bwd_cases.py checked without a GPU: the case table reaches every branch of the attention backward's launcher (and keeps
doing so: a branch that loses its cases fails here), the float64 yardstick agrees with finite differences of its own forward, and the
one-hot probe reads a known mask back exactly."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as ac  # noqa: E402

TWO_PASS = {"blk_both", "blk_dq+wave_dkv", "wave_dq+blk_dkv", "wave_both"}


def family(branch):
    return "small" if branch.startswith("small") else "two_pass" if branch in TWO_PASS else branch.split("/")[1]


def test_case_ids_are_unique_and_cases_are_well_formed():
    ids = [c.id for c in ac.CASES]
    assert len(set(ids)) == len(ids)
    for c in ac.CASES:
        assert c.H == 8 and c.DH in (16, 32, 64, 128) and c.layout in ("consecutive", "strided", "gapped") and c.pitch in ("plain", "packed")
        inner, qa, ka, rq, rk = ac.addressing(c)
        qi, ki = ac.unit_rows(c)
        assert int(qi.max()) < rq and int(ki.max()) < rk and rq <= 4400
        assert qi.unique().numel() == qi.numel() and ki.unique().numel() == ki.numel()  # no row belongs to two units
        if c.layout == "gapped":
            assert qi.numel() < rq and ki.numel() < rk
        else:
            assert qi.numel() == rq and ki.numel() == rk


def test_every_branch_is_reached_twice_under_the_default_switches():
    hits = {b: [c.id for c in ac.CASES if ac.expected_branch(c) == b] for b in ac.BRANCHES}
    assert {ac.expected_branch(c) for c in ac.CASES} <= set(ac.BRANCHES)
    for b, ids in hits.items():
        assert len(ids) >= 2, (b, ids)
    # at head dim 128 (the shipped width) alone, every branch but the per-wave pair, which no default launch of that width takes
    at128 = {ac.expected_branch(c) for c in ac.CASES if c.DH == 128}
    assert at128 == set(ac.BRANCHES) - {"wave_both"}


# (branch, (Sq, Sk), what the case needs besides the shape)
TABLE = [
    ("small1", (1, 1), {}), ("small2", (2, 2), {}), ("small2", (2, 1), {}), ("small4", (4, 4), {}), ("small4", (3, 2), {}),
    ("small4", (1, 4), {}), ("small4", (4, 3), {}),
    ("fused1/nochunk", (5, 16), {}), ("fused1/nochunk", (17, 12), {}), ("fused1/nochunk", (128, 1), {}), ("fused1/nochunk", (100, 5), {}),
    ("fused2/nochunk", (17, 17), {}), ("fused2/nochunk", (24, 32), {}), ("fused2/nochunk", (5, 20), {}),
    ("fused4/nochunk", (17, 33), {}), ("fused4/nochunk", (64, 64), {}), ("fused4/nochunk", (70, 65), {}), ("fused4/nochunk", (128, 128), {}),
    ("fused4/nochunk", (5, 100), {}), ("fused4/nochunk", (200, 48), {"scratch": False}), ("fused4/nochunk", (256, 64), {"scratch": False}),
    ("fused4/chunk64", (65, 37), {"G": 5}), ("fused4/chunk64", (100, 48), {"G": 5}), ("fused1/chunk64", (128, 16), {"G": 5}),
    ("fused2/chunk64", (129, 17), {"G": 5}), ("fused4/chunk64", (360, 64), {"G": 5}), ("fused1/chunk64", (700, 1), {"G": 5}),
    ("fused4/chunk256", (257, 37), {"G": 17}), ("fused4/chunk256", (1400, 48), {"G": 3}),
    ("blk_both", (130, 130), {}), ("blk_both", (129, 65), {}), ("blk_both", (200, 144), {}), ("blk_both", (300, 70), {}),
    ("blk_both", (64, 129), {}), ("blk_both", (17, 200), {}),
    ("blk_dq+wave_dkv", (300, 10), {"scratch": False}), ("blk_dq+wave_dkv", (300, 16), {"layout": "strided"}),
    ("wave_dq+blk_dkv", (10, 200), {}), ("wave_dq+blk_dkv", (16, 129), {}),
]


@pytest.mark.parametrize("branch,shape,needs", TABLE, ids=[f"{b}-{s[0]}x{s[1]}" for b, s, _ in TABLE])
def test_the_shapes_of_the_table_take_the_branch_they_were_chosen_for(branch, shape, needs):
    found = [c for c in ac.CASES if c.DH == 128 and (c.Sq, c.Sk) == shape and all(getattr(c, k) == v for k, v in needs.items())]
    assert found and all(ac.expected_branch(c) == branch for c in found), (branch, shape, [(c.id, ac.expected_branch(c)) for c in found])


def test_the_fallbacks_every_switch_setting_opens_are_reached():
    c128 = [c for c in ac.CASES if c.DH == 128]
    no_fused = {ac.expected_branch(c, {"attn_bwd_fused": 0}) for c in c128}
    assert no_fused == {"small1", "small2", "small4"} | TWO_PASS
    # the <= 16 x <= 16 shapes the one-pass kernel takes by default: the per-wave <128> kernels
    assert sum(ac.expected_branch(c, {"attn_bwd_fused": 0}) == "wave_both" for c in c128) >= 2
    no_blk = {ac.expected_branch(c, {"attn_bwd_fused": 0, "attn_bwd_blk": 0}) for c in c128}
    assert no_blk == {"small1", "small2", "small4", "wave_both"}
    tiny = [c for c in c128 if c.Sq <= 4 and c.Sk <= 4]
    assert len(tiny) >= 7 and all(ac.expected_branch(c, {"attn_bwd_small": 0}) == "fused1/nochunk" for c in tiny)
    both = {"attn_bwd_fused": 0, "attn_bwd_small": 0}
    assert all(ac.expected_branch(c, both) == "wave_both" for c in tiny)
    # the narrower heads never leave the per-wave kernels
    assert all(ac.expected_branch(c, s) == "wave_both" for c in ac.CASES if c.DH != 128 for s in ac.SWITCH_SETTINGS)


def test_layouts_and_pitches_are_spread_over_the_branch_families():
    fam = {}
    for c in ac.CASES:
        if c.DH == 128:
            fam.setdefault(family(ac.expected_branch(c)), []).append(c)
    assert set(fam) == {"small", "nochunk", "chunk64", "chunk256", "two_pass"}
    for name, cases in fam.items():
        layouts = {c.layout for c in cases}
        # chunked launches need consecutive rows: strided units cannot reach them
        assert layouts == ({"consecutive", "gapped"} if name.startswith("chunk") else {"consecutive", "strided", "gapped"}), (name, layouts)
        assert any(c.pitch == "packed" for c in cases), name
    assert any(c.pitch == "packed" and c.layout == "gapped" for c in ac.CASES)
    assert any(c.pitch == "packed" and c.Sq != c.Sk for c in ac.CASES) and any(c.pitch == "packed" and c.Sq == c.Sk for c in ac.CASES)
    assert any(c.scale is not None for c in ac.CASES) and not any(c.scale == 1 / math.sqrt(c.DH) for c in ac.CASES)
    # chunk64: unit first rows that are no multiples of the chunk; chunk256: a last chunk of one query
    for c in fam["chunk64"]:
        assert any(int(r) % 64 for r in ac.unit_rows(c)[0][:, 0]), c.id
    assert any(c.Sq % 256 == 1 for c in fam["chunk256"]) and all(ac.addressing(c)[3] > 4096 for c in fam["chunk256"])


def test_the_dropout_cases_cover_every_branch_with_enough_mask_elements():
    assert {ac.expected_branch(c) for c in ac.DROPOUT_CASES} == set(ac.BRANCHES) - {"wave_both"}
    assert "wave_both" in {ac.expected_branch(c, {"attn_bwd_fused": 0}) for c in ac.DROPOUT_CASES}
    assert {ac.expected_branch(c, {"attn_bwd_fused": 0}) for c in ac.DROPOUT_CASES} >= TWO_PASS
    assert sum(c.Sq <= 4 and c.Sk <= 4 for c in ac.DROPOUT_CASES) >= 3
    for c, i in zip(ac.DROPOUT_CASES, ac.DROPOUT_IDS):
        assert c.DH == 128 and c.G * c.H * c.Sq * c.Sk >= 4000, c.id
        assert ac.expected_branch(c) == ac.expected_branch(ac.BY_ID[i]), c.id  # more units, the same kernels
        assert ac.addressing(c)[3] <= 4400


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def tiny(layout, Sq, Sk, G, scale=None):
    return ac.Case(f"tiny_{layout}", 2, 4, G, Sq, Sk, layout, True, "plain", scale)


def loss(case, q, k, v, dout, mask, p):
    return float((ac.forward64(case, q, k, v, mask, p)[1] * dout).sum())


@pytest.mark.parametrize("case,p", [(tiny("consecutive", 3, 2, 2), 0.0), (tiny("strided", 2, 3, ac.TP, scale=0.3), 0.25),
                                    (tiny("gapped", 3, 4, 2), 0.0)], ids=["consecutive", "strided_mask", "gapped"])
def test_reference_agrees_with_central_finite_differences(case, p):
    g = torch.Generator().manual_seed(17)
    _, _, _, rq, rk = ac.addressing(case)
    D = case.H * case.DH
    q, k, v, dout = (torch.randn(r, D, generator=g, dtype=torch.float64) for r in (rq, rk, rk, rq))
    mask = (torch.rand(case.G, case.H, case.Sq, case.Sk, generator=g) >= p).double() if p else None
    assert mask is None or 0 < float(mask.mean()) < 1
    grads = ac.reference(case, q, k, v, dout, mask, p)
    eps = 1e-6
    for which, (x, grad) in enumerate(zip((q, k, v), grads)):
        fd = torch.zeros_like(x)
        for i in range(x.numel()):
            vals = []
            for sgn in (1, -1):
                moved = [t.clone() for t in (q, k, v)]
                moved[which].view(-1)[i] += sgn * eps
                vals.append(loss(case, *moved, dout, mask, p))
            fd.view(-1)[i] = (vals[0] - vals[1]) / (2 * eps)
        # f64 central differences at eps = 1e-6: truncation ~eps^2, rounding ~1e-16 / eps
        assert float((fd - grad).abs().max()) <= 1e-8 * max(1.0, float(grad.abs().max())), which
        assert float(grad.abs().max()) > 0.05
    if case.layout == "gapped":
        qi, ki = ac.unit_rows(case)
        free_q = torch.ones(rq, dtype=torch.bool).index_fill(0, qi.reshape(-1), False)
        free_k = torch.ones(rk, dtype=torch.bool).index_fill(0, ki.reshape(-1), False)
        assert int(free_q.sum()) == case.G * ac.GAP_Q and int(free_k.sum()) == case.G * ac.GAP_K
        assert not grads[0][free_q].any() and not grads[1][free_k].any() and not grads[2][free_k].any()


def test_reference_equals_the_plain_formula_on_consecutive_units():
    """forward64 / reference through the row tables against torch's own softmax attention on [G, S, H, DH] views."""
    case = ac.Case("plain", 8, 16, 3, 5, 7, "consecutive", True, "plain", None)
    q, k, v, dout = ac.make_inputs(case)
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (t.reshape(3, -1, 8, 16).permute(0, 2, 1, 3) for t in leaves)
    o = (torch.softmax(qh @ kh.transpose(-1, -2) / 4.0, -1) @ vh).permute(0, 2, 1, 3).reshape(15, 128)
    o.backward(dout.double())
    assert torch.allclose(ac.forward64(case, q, k, v)[1], o.detach(), rtol=0, atol=1e-14)
    for got, leaf in zip(ac.reference(case, q, k, v, dout), leaves):
        assert torch.allclose(got, leaf.grad, rtol=0, atol=1e-13)


# ---- the probe ----------------------------------------------------------------------------------------------------------------------
def forward_numpy(case, q, k, v, mask, p):
    """A stand-in for the forward kernel in NumPy float32: unit by unit, head by head, through the case's addressing."""
    qi, ki = (t.numpy() for t in ac.unit_rows(case))
    o = np.zeros_like(q)
    for g in range(case.G):
        for h in range(case.H):
            cols = slice(h * case.DH, (h + 1) * case.DH)
            s = (q[qi[g], cols] @ k[ki[g], cols].T) * np.float32(ac.case_scale(case))
            e = np.exp(s - s.max(1, keepdims=True))
            pd = e / e.sum(1, keepdims=True) * mask[g, h] / np.float32(1 - p)
            o[qi[g], cols] = pd @ v[ki[g], cols]
    return o


@pytest.mark.parametrize("case", [tiny("consecutive", 5, 3, 3), tiny("strided", 3, 10, 2 * ac.TP), tiny("gapped", 2, 9, 4)],
                         ids=["Sk<DH", "strided_Sk>DH", "gapped_Sk>DH"])
def test_probe_recovers_a_known_mask_exactly(case):
    p = 0.3
    rng = np.random.default_rng(5)
    _, _, _, rq, rk = ac.addressing(case)
    D = case.H * case.DH
    q, k = rng.standard_normal((rq, D), dtype=np.float32), rng.standard_normal((rk, D), dtype=np.float32)
    mask = rng.random((case.G, case.H, case.Sq, case.Sk)) >= p
    assert ac.probe_passes(case) == -(-case.Sk // case.DH) and 0 < mask.mean() < 1
    outs = [forward_numpy(case, q, k, ac.probe_v(case, b).numpy(), mask.astype(np.float32), p) for b in range(ac.probe_passes(case))]
    pd = ac.probe_collect(case, outs)
    assert pd.shape == mask.shape and np.array_equal((pd != 0).numpy(), mask)
    P, _ = ac.forward64(case, torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(k), torch.from_numpy(mask), p)
    assert float((pd.double() - P).abs().max()) < 1e-6
    # every key of every unit has its column in exactly one pass; the rows no unit owns stay zero
    total = sum(ac.probe_v(case, b) for b in range(ac.probe_passes(case)))
    _, ki = ac.unit_rows(case)
    assert torch.equal(total[ki.reshape(-1)].sum(1), torch.full((ki.numel(),), float(case.H)))
    assert float(total.sum()) == ki.numel() * case.H
