"""Attention backward per shape class, fused one-pass kernel (sola_tune attn_bwd_fused 1, default) vs the two-pass kernels (0):
time per call and fraction of the HBM peak on the algorithmic bytes (q, k, v, o, dO read + dQ, dK, dV written), max difference.

    python tools/attn_bwd_probe.py
    python tools/attn_bwd_probe.py --sites     one launch site per kernel family of attn_bwd.hip, for timing two builds of the library
                                               against each other (SOLA_HIP_LIB): one JSON line {site: microseconds per call}
"""
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sola_amd import _lib, ops  # noqa: E402

lib = _lib.lib()
D, H = 1024, 8


def timed(call, n=10, rounds=1):
    """kernels only (HIP events around the launches): best of ``rounds`` means over n calls, ms"""
    call()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(rounds):
        _lib.profile_enable(True); _lib.profile_read(reset=True)
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        best = min(best, _lib.profile_read(reset=True)["attn_bwd"]["ms"] / n)
        _lib.profile_enable(False)
    return best


def classes():
    for tag, B, N, Tp in (("NS/64", 64, 64, 4), ("N80/64", 64, 80, 4), ("C4/16", 16, 128, 16), ("N40 T'12", 64, 40, 12), ("N16 T'25", 64, 16, 25)):
        M = B * N * Tp
        q, k, v, do = (torch.randn(M, D, device="cuda") for _ in range(4))
        line = []
        for name, G, Sq, Sk, inner, qa in ((f"obj {N}x{N}", B * Tp, N, N, Tp, (N * Tp, 1, Tp)), (f"motion {Tp}x{Tp}", B * N, Tp, Tp, 1, (Tp, 0, 1))):
            o, lse = ops.attention(q, k, v, G, H, Sq, Sk, inner, qa, qa, return_lse=True)
            res, t = {}, {}
            for fused in (1, 0, 1, 0, 11, 12):  # 11 / 12: the one-pass kernel without its tile arithmetic / with only the first tile staged
                _lib.check(lib.sola_tune(b"attn_bwd_fused", 1 if fused else 0), "tune")
                _lib.check(lib.sola_tune(b"attn_bwd_ablate", fused - 10 if fused > 1 else 0), "tune")
                res[fused] = ops.attention_backward(q, k, v, o, do, lse, G, H, Sq, Sk, inner, qa, qa)
                t[fused] = min(t.get(fused, 1e9), timed(lambda: ops.attention_backward(q, k, v, o, do, lse, G, H, Sq, Sk, inner, qa, qa)))
            diff = max(float((a - b).abs().max()) for a, b in zip(res[1], res[0]))
            ref = max(float(b.abs().max()) for b in res[0])
            nbytes = 8 * M * D * 4
            line.append(f"{name}: fused {t[1] * 1e3:6.1f} us ({nbytes / t[1] / 1e6 / 8000 * 100:4.1f}%) two-pass {t[0] * 1e3:6.1f} us [no arithmetic {t[11] * 1e3:6.1f}, one staging {t[12] * 1e3:6.1f}]  maxdiff {diff:.1e} of {ref:.1e}")
        print(f"{tag:9s} " + " | ".join(line), flush=True)
    _lib.check(lib.sola_tune(b"attn_bwd_fused", 1), "tune")
    _lib.check(lib.sola_tune(b"attn_bwd_ablate", 0), "tune")


def sites():
    """Units of consecutive rows, 8 heads.  Two-pass kernels (attn_bwd_fused 0): per-wave at head dim 16 / 32 / 64 / 128 (12 x 12 units),
    block-shared at 128 (64 x 64), the two mixtures (300 x 16, 16 x 129); one-pass kernel with f32 products at one / two / four waves on
    f32 rows and on bf16 rows (attn_bwd_bf16_mfma 0).  The ragged (unit-table) forms of the per-wave kernels run inside the ragged
    training step only: tools/train_ragged_probe.py 64 f32 attn_bwd_fused=0, its attn_bwd figure."""
    out = {}

    def f32_site(tag, DH, G, Sq, Sk, **sw):
        W = H * DH
        q, do = (torch.randn(G * Sq, W, device="cuda") for _ in range(2))
        k, v = (torch.randn(G * Sk, W, device="cuda") for _ in range(2))
        o, lse = ops.attention(q, k, v, G, H, Sq, Sk, 1, (Sq, 0, 1), (Sk, 0, 1), return_lse=True)
        with _lib.tuned(**sw):
            out[tag] = round(1e3 * timed(lambda: ops.attention_backward(q, k, v, o, do, lse, G, H, Sq, Sk, 1, (Sq, 0, 1), (Sk, 0, 1)), 20, 3), 2)

    def bf16_site(tag, G, Sq, Sk):
        q16, k16, v16 = (torch.randn(n, D, device="cuda").to(torch.bfloat16) for n in (G * Sq, G * Sk, G * Sk))
        o, lse = ops.attention(q16.float(), k16.float(), v16.float(), G, H, Sq, Sk, 1, (Sq, 0, 1), (Sk, 0, 1), return_lse=True)
        do = torch.randn(G * Sq, D, device="cuda") * 1e-3
        gq, gk, gv = (torch.empty(n, D, device="cuda", dtype=torch.bfloat16) for n in (G * Sq, G * Sk, G * Sk))
        dq_scr, dvec = torch.empty(G * Sq, D, device="cuda"), torch.empty(G * Sq, H, device="cuda")
        n_scr = int(lib.sola_attention_backward_scratch_floats(G * Sq, G, H, Sk))
        scr = torch.empty(max(n_scr, 1), device="cuda")
        p, s = _lib.ptr, _lib.current_stream(do.device)

        def call():
            _lib.check(lib.sola_attention_backward_bf16(p(q16), D, p(k16), D, p(v16), D, p(o), 0, p(do), 0, D, p(lse), C.c_void_p(gq.data_ptr()), C.c_void_p(gk.data_ptr()),
                                                        C.c_void_p(gv.data_ptr()), D, D, D, p(dq_scr), p(dvec), G, H, 128, Sq, Sk, 1, Sq, 0, 1, Sk, 0, 1, 1.0 / math.sqrt(128),
                                                        G * Sq, p(scr) if n_scr else None, n_scr, s), "sola_attention_backward_bf16")

        with _lib.tuned(attn_bwd_bf16_mfma=0):
            out[tag] = round(1e3 * timed(call, 20, 3), 2)

    for DH in (16, 32, 64, 128):
        f32_site(f"two-pass per-wave dh{DH} 12x12", DH, 2560, 12, 12, attn_bwd_fused=0)
    f32_site("two-pass block-shared dh128 64x64", 128, 256, 64, 64, attn_bwd_fused=0)
    f32_site("two-pass blk dQ + wave dK/dV 300x16", 128, 64, 300, 16, attn_bwd_fused=0)
    f32_site("two-pass wave dQ + blk dK/dV 16x129", 128, 64, 16, 129, attn_bwd_fused=0)
    for tag, G, S in (("one wave 12x12", 2560, 12), ("two waves 25x25", 1024, 25), ("four waves 64x64", 256, 64)):
        f32_site(f"one-pass f32 {tag}", 128, G, S, S)
        bf16_site(f"one-pass bf16 rows, f32 products {tag}", G, S, S)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    sites() if "--sites" in sys.argv[1:] else classes()
