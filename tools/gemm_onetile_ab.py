"""A/B of two builds of libsola_hip.so at the one-tile-per-block direct-to-LDS GEMM kernels, which the default routing of the big shapes
(tools/gemm_lib_ab.py) does not reach: split-f16 / f16 / bf16 operands x 128x128 and 256x256 blocks (sola_tune gemm_glds 1 / 4 with
gemm_persist 0), plain rows, f32 output, no residual.  Child processes per build, interleaved; per site the runs of each build
(us per call), their min - max spread and median.  usage: gemm_onetile_ab.py libA.so libB.so [rounds] [MxNxK]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
child = r'''
import sys, json, torch
sys.path.insert(0, sys.argv[1])
from sola_amd import ops, _lib
from sola_amd._lib import check, current_stream, lib, ptr, tuned
M, N, K = (int(v) for v in sys.argv[2].split("x"))
x, wt, b = torch.randn(M, K, device="cuda"), torch.randn(N, K, device="cuda") * 0.03, torch.randn(N, device="cuda")
out = torch.empty(M, N, device="cuda")
asp, wsp = ops.cast_sp16(x), ops.cast_sp16(wt, 64.0)
ah, wh, ab, wb = x.half(), wt.half(), x.bfloat16(), wt.bfloat16()
s = current_stream(out.device)
calls = {
    "split": lambda: ops.gemm_nt_split(asp, wsp, b, None, False, 1 / 64, False),
    "f16": lambda: check(lib().sola_gemm_nt_f16(ptr(ah), K, ptr(wh), ptr(b), None, N, ptr(out), N, 0, M, N, K, 1.0, s), "f16"),
    "bf16": lambda: check(lib().sola_gemm_nt_bf16(ptr(ab), K, ptr(wb), ptr(b), None, N, 0, ptr(out), N, 0, M, N, K, s), "bf16"),
}
res = {}
for kind, fn in calls.items():
    for glds in (1, 4):
        with tuned(gemm_glds_force=1, gemm_glds=glds, gemm_persist=0):
            ts = []
            for rnd in range(5):
                fn(); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10): fn()
                e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 100)
            res[f"{kind} {128 if glds == 1 else 256}x{128 if glds == 1 else 256} {M}x{N}x{K}"] = min(ts)
print("RESULT " + json.dumps(res))
'''
la, lb = sys.argv[1], sys.argv[2]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
shape = sys.argv[4] if len(sys.argv) > 4 else "16384x1024x1024"
res = {la: {}, lb: {}}
for rnd in range(rounds):
    for lib_ in (la, lb):
        p = subprocess.run([sys.executable, "-c", child, ROOT, shape], env=dict(os.environ, SOLA_HIP_LIB=os.path.abspath(lib_)), capture_output=True, text=True, timeout=300)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-2000:]); sys.exit(1)
        for k, v in json.loads(line[0][7:]).items(): res[lib_].setdefault(k, []).append(v)
for k in res[la]:
    a, b = res[la][k], res[lb][k]
    verdict = "within A's spread" if min(a) <= statistics.median(b) <= max(a) else ("FASTER than A's spread" if statistics.median(b) < min(a) else "SLOWER than A's spread")
    print(f"{k}:  A {' '.join(f'{v:.1f}' for v in a)} (min {min(a):.1f} max {max(a):.1f} median {statistics.median(a):.1f})   "
          f"B {' '.join(f'{v:.1f}' for v in b)} (median {statistics.median(b):.1f})  us  -> B {verdict}")
