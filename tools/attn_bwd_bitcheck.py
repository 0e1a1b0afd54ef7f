"""Bit-for-bit record of the attention backward's results, for comparing two builds of the library (a refactor of attn_bwd.hip that
moves no arithmetic must not move a bit).  The whole step's counterpart, which also reaches the ragged (unit-table) kernels, is
tools/grad_bitcheck.py (SOLA_TUNE=attn_bwd_fused=0 for the two-pass kernels there).

    SOLA_HIP_LIB=<build A>/libsola_hip.so python tools/attn_bwd_bitcheck.py --out DIR_A
    SOLA_HIP_LIB=<build B>/libsola_hip.so python tools/attn_bwd_bitcheck.py --out DIR_B
    python tools/attn_bwd_bitcheck.py --compare DIR_A DIR_B

Recorded: dq, dk, dv of
  * every case of tests/attn_bwd_cases.py (CASES) under every entry of SWITCH_SETTINGS, launched as tests/test_gpu_attn_bwd.py launches it;
  * its DROPOUT_CASES with p = 0.1 and a fixed seed, under the default switches and the two-pass fallback;
  * the bf16 launches of tests/test_gpu_bf16_store.py's table, one case per wave count of the one-pass kernel, the register kernel and a
    chunked launch, in the four forms: f32 products (attn_bwd_bf16_mfma 0), bf16 products, bf16 dO, bf16 dO and O.
DIR/record.json holds one SHA-256 of the raw bytes per array (the arrays themselves are some hundred MB); --compare checks that both
records hold the same launches and arrays and that every digest is equal; exit status 1 on any difference.
"""
import argparse
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bitcheck_common import compare, digest, switch_name, write_record  # noqa: E402

P_DROP, SEED = 0.1, 777
BF16_CASES = ("motion_17x12", "motion_24", "inter_object", "inter_object_80", "motion_4", "object_to_language")
BF16_FORMS = (("f32_products", {"attn_bwd_bf16_mfma": 0}, False, False), ("bf16_products", {}, False, False),
              ("bf16_dout", {}, True, False), ("bf16_dout_o", {}, True, True))


def record(out):
    import torch

    import attn_bwd_cases as ac
    import test_gpu_attn_bwd as tg
    import test_gpu_bf16_store as tb
    from sola_amd import ops
    from sola_amd._lib import check, current_stream, lib, ptr, tuned

    rec = {}

    def keep(name, grads):
        torch.cuda.synchronize()
        rec[name] = {n: digest(g) for n, g in zip(("dq", "dk", "dv"), grads)}
        print(name, rec[name]["dq"][:12], rec[name]["dk"][:12], rec[name]["dv"][:12], flush=True)

    for case in ac.CASES:
        for sw in ac.SWITCH_SETTINGS:
            keep(f"{case.id} [{switch_name(sw)}] {ac.expected_branch(case, sw)}", tg.run(case, sw)[1])
    for case in ac.DROPOUT_CASES:
        for sw in ({}, {"attn_bwd_fused": 0}):
            ops.set_stage_dropout(P_DROP, SEED)  # the forward inside run() drops with the same seed
            keep(f"dropout {case.id} [{switch_name(sw)}] {ac.expected_branch(case, sw)}", tg.run(case, sw)[1])
            ops.set_stage_dropout(0.0, 0)
    for name in BF16_CASES:
        G, H, Sq, Sk, inner, qa, ka, qrows, krows = tb._attn_case(name)
        D = H * 128
        torch.manual_seed(100 + len(name))
        q16, k16, v16 = (tb.bf(torch.randn(n, D, device="cuda") * sc) for n, sc in ((qrows, 1.5), (krows, 1.5), (krows, 1.0)))
        o, lse = ops.attention(q16.float(), k16.float(), v16.float(), G, H, Sq, Sk, inner, qa, ka, return_lse=True)
        dout = torch.randn(qrows, D, device="cuda") * 1e-3
        n_scr = int(lib().sola_attention_backward_scratch_floats(qrows, G, H, Sk))
        scr = torch.empty(max(n_scr, 1), device="cuda")
        for form, sw, dout_bf16, o_bf16 in BF16_FORMS:
            gq = torch.full((qrows, 3 * D), 7.0, device="cuda", dtype=torch.bfloat16)  # column slices of [rows][3 D], as backward.hip lays them out
            gk = torch.full((krows, 3 * D), 7.0, device="cuda", dtype=torch.bfloat16)
            dq_scr, dvec = torch.zeros(qrows, 3 * D, device="cuda"), torch.zeros(qrows, H, device="cuda")
            dout_arg, o_arg = (tb.bf(dout) if dout_bf16 else dout), (tb.bf(o) if o_bf16 else o)
            with tuned(**sw):
                check(lib().sola_attention_backward_bf16(
                    ptr(q16), D, ptr(k16), D, ptr(v16), D, C.c_void_p(o_arg.data_ptr()), int(o_bf16), C.c_void_p(dout_arg.data_ptr()), int(dout_bf16), D,
                    ptr(lse), C.c_void_p(gq.data_ptr()), C.c_void_p(gk.data_ptr() + 2 * D), C.c_void_p(gk.data_ptr() + 4 * D), 3 * D, 3 * D, 3 * D,
                    ptr(dq_scr), ptr(dvec), G, H, 128, Sq, Sk, inner, qa[0], qa[1], qa[2], ka[0], ka[1], ka[2], 1.0 / math.sqrt(128), qrows,
                    ptr(scr) if n_scr else None, n_scr, current_stream(q16.device)), "sola_attention_backward_bf16")
            keep(f"bf16 {name} {form}", (gq, gk[:, D:2 * D], gk[:, 2 * D:]))  # (gq whole: the columns behind dq must stay 7)
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
