"""Forward attention kernels that tools/attn_default_probe.py does not reach, one standalone launch site each: the training forward
(log-sum-exp output; f32 and bf16 q / k / v), head_dim 64, split-f16 q / k / v, the split arithmetic on f32 inputs.
Time per call (HIP events, best of 3 x 20 calls) in microseconds; the kernel a site runs is named in its tag.

    python tools/attn_sites_probe.py
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sola_amd import _lib, ops  # noqa: E402
from sola_amd._lib import check, current_stream, ptr  # noqa: E402

lib = _lib.lib()
D, B, N, Tp = 1024, 256, 64, 4
M = B * N * Tp
OBJ = (B * Tp, N, N, Tp, (N * Tp, 1, Tp))  # G, Sq, Sk, inner, (outer, inner stride, row stride): the inter-object attention
q, k, v = (torch.randn(M, D, device="cuda") for _ in range(3))
q16, k16, v16 = (t.to(torch.bfloat16) for t in (q, k, v))
qs, ks, vs = (ops.cast_sp16(t) for t in (q, k, v))
o32, o16 = torch.zeros(M, D, device="cuda"), torch.zeros(M, D, device="cuda", dtype=torch.bfloat16)


def obj(H, lse=False):
    G, Sq, Sk, inner, a = OBJ
    return lambda: ops.attention(q, k, v, G, H, Sq, Sk, inner, a, a, return_lse=lse)


def obj_bf16(H):
    G, Sq, Sk, inner, a = OBJ
    lse = torch.zeros(M, H, device="cuda")
    return lambda: check(lib.sola_attention_bf16(ptr(q16), D, ptr(k16), D, ptr(v16), D, ptr(o32), ptr(o16), D, G, H, D // H, Sq, Sk, inner, a[0], a[1], a[2],
                                                 a[0], a[1], a[2], 1.0 / math.sqrt(D // H), ptr(lse), current_stream(q.device)), "attention_bf16")


def obj_split():
    G, Sq, Sk, inner, a = OBJ
    return lambda: ops.attention_split(qs, ks, vs, G, 8, Sq, Sk, inner, a, a, out_split=True)


SITES = (  # tag, sola_tune keys for the site, call
    ("simple<128,16,DB,TR> obj 64x64 +lse", {}, obj(8, True)),
    ("simple<128,16,DB,TR,IN16> obj 64x64 bf16 in", {"attn_bf16_mfma": 0}, obj_bf16(8)),
    ("simple<64,16,DB> obj 64x64 dh64", {}, obj(16)),
    ("simple<64,32> obj 64x64 dh64 single stage", {"attn_simple_db": 0}, obj(16)),
    ("simple<64,16,DB,TR> obj 64x64 dh64 +lse", {}, obj(16, True)),
    ("simple<64,16,DB,TR,IN16> obj 64x64 dh64 bf16 in", {"attn_bf16_mfma": 0}, obj_bf16(16)),
    ("spin<16,DB> obj 64x64 split in/out", {}, obj_split()),
    ("spin<32> obj 64x64 split in/out single stage", {"attn_spin": 2}, obj_split()),
    ("splitm<128,32> obj 64x64 split arithmetic", {"attn_stage_split_math": 1, "attn_splitm": 1}, obj(8)),
)
for tag, tune, fn in SITES:
    with _lib.tuned(**tune):  # borrowed: each key gets back what it was
        best = 1e9
        for _ in range(3):
            fn(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20)
    print(f"{tag:52s} {best * 1e3:8.1f} us", flush=True)
