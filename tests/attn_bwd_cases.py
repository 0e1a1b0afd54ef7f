"""Attention backward (sola_amd/csrc/attn_bwd.hip): the case table that reaches every branch of the launcher at head dim 128, a plain
restatement of the launcher's choice, the float64 yardstick through each case's own row addressing, and the one-hot probe that reads
the dropout mask out of the forward.  Shared by test_attn_bwd_cpu.py and test_gpu_attn_bwd.py."""
import collections
import functools
import math

import torch

Case = collections.namedtuple("Case", "id H DH G Sq Sk layout scratch pitch scale")
# layout   consecutive  inner 1, row stride 1, outer = Sq / Sk: the units lie back to back
#          strided      the inter-object addressing: inner = TP, row stride TP, outer = S * TP (G is a multiple of TP)
#          gapped       consecutive with outer = S + GAP: GAP_Q / GAP_K rows behind every unit belong to nobody
# scratch  True: ops.attention_backward (sola_attention_backward_ws, the chunk scratch handed over); False: sola_attention_backward
# pitch    "plain": rows of D values; "packed": the case ALSO runs with q, k, v and the gradients as column blocks of [rows][4 D] buffers
# scale    None = 1 / sqrt(DH)
TP, GAP_Q, GAP_K = 5, 7, 3
H = 8
ODD_SCALE = 0.0625
SWITCHES = {"attn_bwd_fused": 1, "attn_bwd_blk": 1, "attn_bwd_small": 1}
SWITCH_SETTINGS = ({}, {"attn_bwd_fused": 0}, {"attn_bwd_fused": 0, "attn_bwd_blk": 0}, {"attn_bwd_small": 0})

BRANCHES = (["small1", "small2", "small4"] + [f"fused{n}/{c}" for n in (1, 2, 4) for c in ("nochunk", "chunk64", "chunk256")] +
            ["blk_both", "blk_dq+wave_dkv", "wave_dq+blk_dkv", "wave_both"])


def _c(Sq, Sk, G=5, layout="consecutive", scratch=True, pitch="plain", scale=None, DH=128):
    name = f"dh{DH}_g{G}_{Sq}x{Sk}_{layout}" + ("" if scratch else "_noscratch") + ("_packed" if pitch == "packed" else "") + \
           ("" if scale is None else "_scale")
    return Case(name, H, DH, G, Sq, Sk, layout, scratch, pitch, scale)


CASES = [
    # the register kernel (<= 4 steps): one-, two- and four-step instantiations; 16 units = two whole blocks of eight, 5 = a part of one
    _c(1, 1), _c(1, 1, G=16, pitch="packed"),
    _c(2, 2), _c(2, 1, G=16), _c(2, 2, layout="strided", scale=ODD_SCALE),
    _c(4, 4, G=16), _c(3, 2), _c(1, 4, layout="gapped", pitch="packed"), _c(4, 3, layout="strided"), _c(4, 4, layout="strided", pitch="packed"),
    # one-pass kernel, one wave per unit (<= 16 keys), every query tile in one block
    _c(5, 16), _c(17, 12, pitch="packed"), _c(128, 1, scratch=False), _c(100, 5, layout="strided"), _c(16, 16, layout="gapped"),
    # ... two waves (17..32 keys)
    _c(17, 17), _c(24, 32, layout="strided", pitch="packed"), _c(5, 20, layout="gapped", scale=ODD_SCALE),
    # ... four waves (33..128 keys; more than 64 keys = two key groups)
    _c(17, 33), _c(64, 64, pitch="packed"), _c(70, 65), _c(128, 128, layout="strided"), _c(5, 100, layout="gapped"),
    _c(200, 48, scratch=False), _c(256, 64, scratch=False, pitch="packed"),
    # 64-query chunks (scratch, consecutive rows, at most 4096 query rows, Sq > 64 against <= 64 keys): five units, so that the
    # units' first rows are no multiples of 64
    _c(65, 37, pitch="packed"), _c(100, 48, layout="gapped", pitch="packed"), _c(128, 16, layout="gapped"), _c(129, 17), _c(70, 32, scale=ODD_SCALE),
    _c(360, 64), _c(700, 1),
    # 256-query chunks (more than 4096 query rows, Sq > 256): a last chunk of one query; a partial last chunk and a partial last tile
    _c(257, 37, G=17), _c(1400, 48, G=3, pitch="packed"), _c(257, 16, G=17), _c(300, 5, G=14, layout="gapped"), _c(257, 17, G=17),
    _c(520, 32, G=8),
    # two-pass, block-shared staging on both sides
    _c(130, 130), _c(129, 65, pitch="packed"), _c(200, 144, layout="gapped"), _c(300, 70, scale=ODD_SCALE), _c(64, 129),
    _c(17, 200, layout="strided", pitch="packed"),
    # ... block-shared dQ with per-wave dK / dV (no more than 16 keys), and the other way round
    _c(300, 10, scratch=False, pitch="packed"), _c(300, 16, layout="strided"),
    _c(10, 200, pitch="packed"), _c(16, 129, layout="gapped"),
    # the narrower heads: two-pass per-wave kernels whatever the shape
    _c(17, 33, DH=16), _c(130, 5, DH=16, layout="strided"), _c(4, 4, DH=16, G=16),
    _c(17, 33, DH=32, layout="gapped"), _c(130, 5, DH=32, pitch="packed"), _c(4, 4, DH=32),
    _c(17, 33, DH=64, layout="strided"), _c(130, 5, DH=64), _c(4, 4, DH=64, layout="gapped", scale=ODD_SCALE),
]
BY_ID = {c.id: c for c in CASES}


def case_id(case):
    return case.id


def case_scale(case):
    return 1.0 / math.sqrt(case.DH) if case.scale is None else case.scale


def addressing(case):
    """(inner, q_addr, k_addr, q rows, k rows): q_addr / k_addr = (outer, inner stride, row stride) as ops.attention takes them."""
    if case.layout == "strided":
        assert case.G % TP == 0, case.id
        b = case.G // TP
        return TP, (case.Sq * TP, 1, TP), (case.Sk * TP, 1, TP), b * case.Sq * TP, b * case.Sk * TP
    gq, gk = (GAP_Q, GAP_K) if case.layout == "gapped" else (0, 0)
    return 1, (case.Sq + gq, 0, 1), (case.Sk + gk, 0, 1), case.G * (case.Sq + gq), case.G * (case.Sk + gk)


def unit_rows(case):
    """(q_idx [G, Sq], k_idx [G, Sk]) int64: the rows of every unit (attn_unit_strided, attn_common.h)."""
    inner, qa, ka, _, _ = addressing(case)
    g = torch.arange(case.G)

    def rows(addr, S):
        first = (g // inner) * addr[0] + (g % inner) * addr[1]
        return first[:, None] + torch.arange(S)[None, :] * addr[2]

    return rows(qa, case.Sq), rows(ka, case.Sk)


def expected_branch(case, switches=None):
    """The kernels a launch of ``case`` runs under the sola_tune ``switches``.  A restatement of launch_attention_bwd,
    bwd_small_shape, bwd_plan, launch_bwd_fused, launch_bwd_small and launch_bwd_dh (attn_bwd.hip): whoever edits one of those edits this."""
    sw = dict(SWITCHES, **(switches or {}))
    Sq, Sk = case.Sq, case.Sk
    if sw["attn_bwd_small"] and case.DH == 128 and Sq <= 4 and Sk <= 4:  # bwd_small_shape -> launch_bwd_small
        need = max(Sq, Sk)
        return "small1" if need <= 1 else "small2" if need <= 2 else "small4"
    q_rows = addressing(case)[3]
    # can_chunk: the scratch is there and large enough (the tests size it with the library's own function), rows consecutive
    can_chunk = case.scratch and Sk <= 64 and case.layout != "strided"
    fused = bool(sw["attn_bwd_fused"]) and case.DH == 128 and Sk <= 128 and (Sq <= 128 or (Sk <= 64 and (Sq <= 256 or can_chunk)))
    if fused:  # bwd_plan -> launch_bwd_fused
        qc = 4 if can_chunk and q_rows <= 4096 else 16
        chunk = ("chunk64" if qc == 4 else "chunk256") if Sq > 16 * qc and can_chunk else "nochunk"
        return f"fused{1 if Sk <= 16 else 2 if Sk <= 32 else 4}/{chunk}"
    if case.DH == 128 and sw["attn_bwd_blk"]:  # launch_bwd_dh
        if Sq > 16 and Sk > 16:
            return "blk_both"
        if Sq > 16:
            return "blk_dq+wave_dkv"
        if Sk > 16:
            return "wave_dq+blk_dkv"
    return "wave_both"


def is_chunked(case, switches=None):
    return "/chunk" in expected_branch(case, switches)


@functools.lru_cache(maxsize=None)
def make_inputs(case, seed=0):
    """(q, k, v, dout) float32 standard normal, [rows, H * DH]; the rows no unit owns hold values too (nothing may read them into a result)."""
    _, _, _, rq, rk = addressing(case)
    g = torch.Generator().manual_seed(((seed * 1009 + case.Sq) * 1009 + case.Sk) * 1009 + case.G * 131 + case.DH)
    D = case.H * case.DH
    return tuple(torch.randn(r, D, generator=g) for r in (rq, rk, rk, rq))


def _heads(x, idx, case):
    return x[idx].reshape(case.G, idx.shape[1], case.H, case.DH).permute(0, 2, 1, 3)  # [G, H, S, DH]


def forward64(case, q, k, v, mask=None, p=0.0):
    """float64: (P [G, H, Sq, Sk] = softmax(q k^T scale), times mask / (1 - p) when a mask is given; o = P v in the caller's layout,
    zero in rows no unit owns)."""
    qi, ki = unit_rows(case)
    q, k, v = (t.double() for t in (q, k, v))
    P = torch.softmax(_heads(q, qi, case) @ _heads(k, ki, case).transpose(-1, -2) * case_scale(case), dim=-1)
    if mask is not None:
        P = P * mask.double() / (1.0 - p)
    oh = (P @ _heads(v, ki, case)).permute(0, 2, 1, 3).reshape(case.G * case.Sq, case.H * case.DH)
    o = torch.zeros(q.shape, dtype=torch.float64).index_put((qi.reshape(-1),), oh)
    return P, o


def reference(case, q, k, v, dout, mask=None, p=0.0):
    """(dq, dk, dv) float64 in the caller's layout by autograd through forward64; rows no unit owns get zero."""
    leaves = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    _, o = forward64(case, *leaves, mask=mask, p=p)
    o.backward(dout.double())
    return tuple(t.grad for t in leaves)


@functools.lru_cache(maxsize=None)
def plain_reference(case):
    """(inputs, reference) without dropout: computed once per case, shared, never modified."""
    inputs = make_inputs(case)
    return inputs, reference(case, *inputs)


def cancelled_scale(case, k_or_q, v, dout, which, mask=None, p=0.0):
    """Sk = 1 only.  The single probability is 1, so dS = P (dP - D) = dO . v - dO . o is zero in exact arithmetic and so are dq and
    dk: "error <= bar * max |reference|" would ask float32 for exact cancellation.  What the kernels add up is two terms of size
    |dO . v'| (v' = v mask / (1 - p)) that cancel, so the bar is taken relative to the gradient of those terms WITHOUT the
    cancellation: dq_i = scale * 2 |dO_i . v'| |k|, dk = scale * sum_i 2 |dO_i . v'| |q_i|.  Returns its largest element."""
    assert case.Sk == 1
    qi, ki = unit_rows(case)
    dp = (_heads(dout.double(), qi, case) * _heads(v.double(), ki, case)).sum(-1, keepdim=True)  # [G, H, Sq, 1]
    if mask is not None:
        dp = dp * mask.double() / (1.0 - p)
    dp = 2 * dp.abs() * case_scale(case)
    if which == "dq":
        return float((dp * _heads(k_or_q.double(), ki, case).abs()).max())
    return float((dp * _heads(k_or_q.double(), qi, case).abs()).sum(2).max())


BAR = 3e-5  # the file-wide bar of test_gpu_backward.py: max error <= 3e-5 * max |reference| per matrix


def error_ratios(case, got, want, inputs, mask=None, p=0.0):
    """{name: max |got - want| / (BAR * max |want|)} for dq, dk, dv (``got``: float tensors on the CPU).  With one key the dq and dk
    references are zero by cancellation: their scale is cancelled_scale's."""
    q, k, v, dout = inputs
    out = {}
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        scale = float(w.abs().max())
        if case.Sk == 1 and name != "dv":
            scale = cancelled_scale(case, k if name == "dq" else q, v, dout, name, mask, p)
        out[name] = float((g.double() - w).abs().max()) / (BAR * scale)
    return out


# ---- the probe: V of one-hot rows makes the forward's output the (dropped) probability matrix -------------------------------------
def probe_passes(case):
    return (case.Sk + case.DH - 1) // case.DH


def probe_v(case, b):
    """V [k rows, H * DH] of pass ``b``: the key at position j of its unit holds 1 in column j - b * DH of every head when that
    column exists, so that o[query, h * DH + c] = P[query, key b * DH + c]."""
    _, ki = unit_rows(case)
    rk = addressing(case)[4]
    V = torch.zeros(rk, case.H, case.DH)
    j = torch.arange(case.Sk).expand(case.G, case.Sk)
    here = (j >= b * case.DH) & (j < (b + 1) * case.DH)
    V[ki[here], :, (j[here] - b * case.DH)] = 1.0
    return V.reshape(rk, case.H * case.DH)


def probe_collect(case, outs):
    """[G, H, Sq, Sk] from the forward outputs of the probe passes (each [q rows, H * DH], float, on the CPU)."""
    qi, _ = unit_rows(case)
    blocks = [_heads(torch.as_tensor(o), qi, case) for o in outs]
    return torch.cat(blocks, dim=-1)[..., :case.Sk]


def dropout_case(case, n_min=4000):
    """``case`` with enough units for at least ``n_min`` mask elements (a multiple of TP for strided units)."""
    per_unit = case.H * case.Sq * case.Sk
    G = max(case.G, -(-n_min // per_unit))
    if case.layout == "strided":
        G = -(-G // TP) * TP
    return case._replace(G=G, id=f"{case.id}_G{G}") if G != case.G else case


# one case of every branch of the table, the layouts and the no-scratch launch among them
DROPOUT_IDS = [
    "dh128_g5_1x1_consecutive", "dh128_g5_2x2_strided_scale", "dh128_g5_4x3_strided", "dh128_g5_1x4_gapped_packed",
    "dh128_g5_5x16_consecutive", "dh128_g5_17x12_consecutive_packed", "dh128_g5_128x1_consecutive_noscratch", "dh128_g5_24x32_strided_packed", "dh128_g5_70x65_consecutive",
    "dh128_g5_128x16_gapped", "dh128_g5_129x17_consecutive", "dh128_g5_100x48_gapped_packed",
    "dh128_g17_257x16_consecutive", "dh128_g17_257x17_consecutive", "dh128_g17_257x37_consecutive",
    "dh128_g5_129x65_consecutive_packed", "dh128_g5_200x144_gapped", "dh128_g5_300x16_strided", "dh128_g5_300x10_consecutive_noscratch_packed",
    "dh128_g5_10x200_consecutive_packed", "dh128_g5_16x129_gapped",
]
DROPOUT_CASES = [dropout_case(BY_ID[i]) for i in DROPOUT_IDS]
