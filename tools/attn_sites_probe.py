"""Forward attention kernels that tools/attn_default_probe.py does not reach, one standalone launch site each: the training forward
(log-sum-exp output; f32 and bf16 q / k / v), head_dim 64, split-f16 q / k / v, the split arithmetic on f32 inputs, attn.hip's shared,
SPLIT and packed shapes where the switches still route to them, the register-only shape at 64 keys and the 16-bit kernels of attn_f16.hip.
Time per call (HIP events over 20 calls, median and best of 5) in microseconds; the kernel a site runs is named in its tag.
(Until the attention-forward steps change the tool printed the best of 3 x 20 calls only: the wording profiles/attn_common_bench.txt cites.)

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


def obj_f16():
    G, Sq, Sk, inner, a = OBJ
    qh, kh, vh, oh = (t.half() for t in (q, k, v, o32))
    return lambda: check(lib.sola_attention_f16(ptr(qh), D, ptr(kh), D, ptr(vh), D, ptr(oh), D, G, 8, D // 8, Sq, Sk, inner, a[0], a[1], a[2], a[0], a[1], a[2],
                                                1.0 / math.sqrt(D // 8), current_stream(q.device)), "attention_f16")


def motion(lse):
    return lambda: ops.attention(q, k, v, B * N, 8, Tp, Tp, 1, (Tp, 0, 1), (Tp, 0, 1), return_lse=lse)


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
    ("attn.hip shared<128,4> obj 64x64 +lse", {"attn_simple_train": 0}, obj(8, True)),
    ("attn.hip shared<64,4> obj 64x64 dh64 +lse", {"attn_simple_train": 0}, obj(16, True)),
    ("attn.hip shared<128,4,SPLIT> obj 64x64 split in/out", {"attn_spin": 0}, obj_split()),
    ("attn.hip packed<128> motion 4x4 +lse", {}, motion(True)),
    ("reg<2> obj 64x64", {"attn_reg": 2}, obj(8)),
    ("f16<128> obj 64x64 f16 in/out", {}, obj_f16()),
    ("f16<128,BF,TR> obj 64x64 bf16 in, bf16 products", {}, obj_bf16(8)),
)
for tag, tune, fn in SITES:
    with _lib.tuned(**tune):  # borrowed: each key gets back what it was
        times = []
        for _ in range(5):
            fn(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 20)
    print(f"{tag:52s} median {sorted(times)[2] * 1e3:8.1f} us  best {min(times) * 1e3:8.1f} us", flush=True)
