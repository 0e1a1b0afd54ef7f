"""Bit-for-bit record of the attention forward's results, for comparing two builds of the library (a refactor of the forward kernels
that moves no arithmetic must not move a bit).  The backward's counterpart is tools/attn_bwd_bitcheck.py; the whole forward and the
whole step are tools/infer_bitcheck.py and tools/grad_bitcheck.py.

    SOLA_HIP_LIB=<build A>/libsola_hip.so python tools/attn_fwd_bitcheck.py --out DIR_A
    SOLA_HIP_LIB=<build B>/libsola_hip.so python tools/attn_fwd_bitcheck.py --out DIR_B
    python tools/attn_fwd_bitcheck.py --compare DIR_A DIR_B

Recorded (o, and the log-sum-exp where the launch has one):
  * every case of tests/attn_fwd_cases.py (CASES) under every entry of SWITCH_SETTINGS, launched as tests/test_gpu_attn_fwd.py launches
    it - every f32 dispatch branch, pitched variants included - and its DROPOUT_CASES with p = 0.1 at a fixed seed;
  * the shapes of test_split_attention_kernel_vs_float64 through sola_attention_split, f32 and split output, under attn_spin 1, 2 and 0
    (attn_fwd_spin_kernel double- and single-buffered, attn.hip's SPLIT shape);
  * the shapes of test_attention_split_math_on_f32_inputs under attn_stage_split_math=1, attn_splitm=1 (attn_fwd_splitm_kernel), and in
    EXPERIMENTS=1 libraries also with attn_res_splitm=1 and with attn_ring 1 / 2 on exact-f32 products;
  * the tables of tests/test_gpu_f16.py (sola_attention_f16), every attn_f16_qpb mode it uses included;
  * the forward launches of tests/test_gpu_bf16_store.py (sola_attention_bf16): f32 products (attn_bf16_mfma 0) and bf16 products,
    with and without the f32 output, with the bf16 o_cast rows.
DIR/record.json holds one SHA-256 of the raw bytes per array; --compare checks that both records hold the same launches and arrays and
that every digest is equal; exit status 1 on any difference.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bitcheck_common import compare, digest, switch_name, write_record  # noqa: E402

P_DROP, SEED = 0.1, 777
H, DH = 8, 128
SPLIT_SHAPES = [(1, 64, 4, 1024), (2, 80, 1, 1024), (1, 130, 2, 128), (1, 20, 25, 128), (1, 128, 2, 1024), (2, 17, 3, 256),
                (3, 33, 2, 1024), (1, 100, 3, 1024), (2, 47, 1, 1024)]  # test_split_attention_kernel_vs_float64
SPLITM_SHAPES = [(1, 64, 4), (2, 80, 1), (1, 130, 2), (1, 20, 25), (1, 7, 16)]  # test_attention_split_math_on_f32_inputs
LANG_KEYS = (48, 37, 70)
F16_TABLE = [(6, 8, 64, 64, 3, "obj"), (40, 8, 4, 4, 1, "motion"), (3, 8, 200, 48, 1, "o2l"), (4, 8, 100, 130, 2, "long"),
             (9, 8, 16, 16, 1, "motion16"), (5, 8, 25, 25, 1, "motion25")]  # test_f16_attention_vs_float64
F16_QPB = [(200, 48, 2), (200, 48, 4), (300, 21, 4), (1000, 64, 8), (130, 5, 3)]  # ..._walking_several_query_blocks_over_staged_keys
BF16_CASES = ("inter_object", "inter_object_80", "motion_24", "motion_17x12", "object_to_language", "motion_4")


def record(out):
    import numpy as np
    import torch

    import attn_fwd_cases as fc
    import test_gpu_attn_fwd as tg
    import test_gpu_bf16_store as tb
    from sola_amd import ops
    from sola_amd._lib import check, current_stream, has_experiments, lib, ptr, tuned

    rec = {}

    def keep(name, **arrays):
        torch.cuda.synchronize()
        rec[name] = {n: digest(a) for n, a in arrays.items() if a is not None}
        print(name, *(d[:12] for d in rec[name].values()), flush=True)

    # ---- f32 q / k / v: every dispatch branch
    for case in fc.CASES:
        for sw in fc.SWITCH_SETTINGS:
            o, lse = tg.run(case, case.lse, sw)
            keep(f"{case.id} [{switch_name(sw)}] {fc.expected_branch(case, sw)}", o=o, lse=lse)
    for case in fc.DROPOUT_CASES:
        ops.set_stage_dropout(P_DROP, SEED)
        o, lse = tg.run(case, True)
        ops.set_stage_dropout(0.0, 0)
        keep(f"dropout {case.id} {fc.expected_branch(case, dropout=True)}", o=o, lse=lse)

    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    # ---- split-f16 q / k / v
    for B, N, Tp, D in SPLIT_SHAPES:
        rng = np.random.default_rng(N * Tp + D)
        q, k, v = (rng.standard_normal((B, N, Tp, D)).astype(np.float32) for _ in range(3))
        qs, ks, vs = (ops.cast_sp16(dev(t).reshape(B * N * Tp, D)) for t in (q, k, v))
        lang = [tuple(ops.cast_sp16(dev(rng.standard_normal((B, Wn, D)).astype(np.float32)).reshape(B * Wn, D)) for _ in range(2)) for Wn in LANG_KEYS]
        obj = (N * Tp, 1, Tp)
        for spin in (1, 2, 0):
            with tuned(attn_spin=spin):
                for split in (False, True):
                    keep(f"split {B}x{N}x{Tp}x{D} inter_object attn_spin={spin} out_split={split}",
                         o=ops.attention_split(qs, ks, vs, B * Tp, H, N, N, Tp, obj, obj, out_split=split))
                for Wn, (lk, lv) in zip(LANG_KEYS, lang):
                    keep(f"split {B}x{N}x{Tp}x{D} language W={Wn} attn_spin={spin}",
                         o=ops.attention_split(qs, lk, lv, B, H, N * Tp, Wn, 1, (N * Tp, 0, 1), (Wn, 0, 1)))
    # ---- f32 q / k / v, split-f16 products (and, in EXPERIMENTS=1 libraries, the ring-staged shape on exact products)
    modes = [("splitm", dict(attn_stage_split_math=1, attn_splitm=1))]
    if has_experiments():
        modes += [("splitm+res", dict(attn_stage_split_math=1, attn_splitm=1, attn_res_splitm=1)), ("ring1", dict(attn_ring=1)), ("ring2", dict(attn_ring=2))]
    for B, N, Tp in SPLITM_SHAPES:
        D = H * DH
        rng = np.random.default_rng(N * Tp + 7)
        q, k, v = (rng.standard_normal((B, N, Tp, D)).astype(np.float32) for _ in range(3))
        k[0, N // 2, 0] = 3.0 * q[0, 1, 0]
        qc, kc, vc = (dev(t).reshape(B * N * Tp, D) for t in (q, k, v))
        lang = [tuple(dev(rng.standard_normal((B, Wn, D)).astype(np.float32)).reshape(B * Wn, D) for _ in range(2)) for Wn in LANG_KEYS]
        for mode, sw in modes:
            with tuned(**sw):
                obj = (N * Tp, 1, Tp)
                keep(f"{mode} {B}x{N}x{Tp} inter_object", o=ops.attention(qc, kc, vc, B * Tp, H, N, N, Tp, obj, obj))
                if Tp > 4:
                    keep(f"{mode} {B}x{N}x{Tp} motion", o=ops.attention(qc, kc, vc, B * N, H, Tp, Tp, 1, (Tp, 0, 1), (Tp, 0, 1)))
                for Wn, (lk, lv) in zip(LANG_KEYS, lang):
                    keep(f"{mode} {B}x{N}x{Tp} language W={Wn}", o=ops.attention(qc, lk, lv, B, H, N * Tp, Wn, 1, (N * Tp, 0, 1), (Wn, 0, 1)))

    # ---- f16 q / k / v / o
    def f16_launch(q, k, v, G, Sq, Sk, inner, qa, ka):
        o = torch.zeros((q.shape[0], H * DH), device="cuda", dtype=torch.float16)
        check(lib().sola_attention_f16(ptr(q), H * DH, ptr(k), H * DH, ptr(v), H * DH, ptr(o), H * DH, G, H, DH, Sq, Sk, inner, *qa, *ka,
                                       1.0 / math.sqrt(DH), current_stream(o.device)), "sola_attention_f16")
        return o

    half = lambda rng, rows: torch.from_numpy(rng.standard_normal((rows, H * DH)).astype(np.float32)).half().cuda()
    for G, _, Sq, Sk, inner, case in F16_TABLE:
        rng = np.random.default_rng(G * 100 + Sq)
        if case in ("obj", "long"):
            rows_q = rows_k = G * max(Sq, Sk)
            qa = ka = (max(Sq, Sk) * inner, 1, inner)
        else:
            rows_q, rows_k, qa, ka, inner = G * Sq, G * Sk, (Sq, 0, 1), (Sk, 0, 1), 1
        q, k, v = half(rng, rows_q), half(rng, rows_k), half(rng, rows_k)
        keep(f"f16 {case} {G}x{Sq}x{Sk}", o=f16_launch(q, k, v, G, Sq, Sk, inner, qa, ka))
    for Sq, Sk, qpb in F16_QPB:
        G = 3
        rng = np.random.default_rng(Sq * 7 + Sk)
        q, k, v = half(rng, G * Sq), half(rng, G * Sk), half(rng, G * Sk)
        for mode in (1, -qpb):
            with tuned(attn_f16_qpb=mode):
                keep(f"f16 {Sq}x{Sk} attn_f16_qpb={mode}", o=f16_launch(q, k, v, G, Sq, Sk, 1, (Sq, 0, 1), (Sk, 0, 1)))

    # ---- bfloat16 q / k / v (the training step's 16-bit storage)
    for name in BF16_CASES + ("motion_12",):
        if name == "motion_12":
            G, Sq, Sk, inner, qa, ka, qrows, krows = 50, 12, 12, 1, (12, 0, 1), (12, 0, 1), 600, 600
        else:
            G, _, Sq, Sk, inner, qa, ka, qrows, krows = tb._attn_case(name)
        D = H * DH
        torch.manual_seed(3 + len(name))
        q16, k16, v16 = (tb.bf(torch.randn(n, D, device="cuda") * sc) for n, sc in ((qrows, 2.0), (krows, 2.0), (krows, 1.0)))
        for form, sw in (("f32_products", {"attn_bf16_mfma": 0}), ("bf16_products", {})):
            if form == "f32_products" and Sq <= 16 and Sk <= 16:
                continue  # attn_simple.hip's kernel takes more than 16 queries or keys
            for with_f32 in (True, False):
                o = torch.zeros(qrows, D, device="cuda") if with_f32 else None
                o16 = torch.zeros(qrows, D, device="cuda", dtype=torch.bfloat16)
                lse = torch.zeros(qrows, H, device="cuda")
                with tuned(**sw):
                    check(lib().sola_attention_bf16(ptr(q16), D, ptr(k16), D, ptr(v16), D, ptr(o) if with_f32 else None, ptr(o16), D, G, H, DH, Sq, Sk,
                                                    inner, *qa, *ka, 1.0 / math.sqrt(DH), ptr(lse), current_stream(q16.device)), "sola_attention_bf16")
                keep(f"bf16 {name} {form} f32_output={with_f32}", o=o, o_cast=o16, lse=lse)
    write_record(out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="record the launches into this directory")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(*args.compare) else 0)
    if not args.out:
        ap.error("--out DIR or --compare DIR_A DIR_B")
    record(args.out)
