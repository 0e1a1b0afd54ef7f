"""The boundary between two steps of bench.py's headline workload, from a rocprofv3 kernel trace (profiles/step_boundary.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 20 --warmup 3
    python tools/step_boundary.py DIR LABEL

Prints the kernels' time per step, then per boundary (score head of one step -> first persistent GEMM of the next): the idle time behind
the score head, the loss pair's time, the span up to the first GEMM, and the launches around the last boundary with their start times."""
import csv
import glob
import statistics
import sys

root, label = sys.argv[1], sys.argv[2]
files = glob.glob(root + "/**/*kernel_trace.csv", recursive=True)
assert files, "no kernel trace under " + root
rows = []
for f in files:
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
heads = [i for i, r in enumerate(rows) if "score_head_kernel" in r[2]]
steps = len(heads)
print(f"== {label}: {len(rows)} dispatches, {steps} steps (score_head launches)")
tot = {}
for s, e, n in rows:
    t = tot.setdefault(n, [0, 0])
    t[0] += 1
    t[1] += e - s
allk = sum(v[1] for v in tot.values()) / 1e3 / steps
gemm = sum(v[1] for k, v in tot.items() if "gemm" in k) / 1e3 / steps
for n, (cnt, ns) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
    if ns / 1e3 / steps >= 15.0 or "loss" in n or "copyBuffer" in n or "fillBuffer" in n or "select" in n:
        print(f"   {cnt / steps:8.2f} launches/step {ns / 1e3 / steps:9.1f} us/step {ns / 1e3 / cnt:9.1f} us/launch  {n[:110]}")
print(f"   all gemm kernels: {gemm:.1f} us/step; all kernels: {allk:.1f} us/step")
# boundary of every step but the last: idle between the score head's end and the next dispatch's start; loss pair
idle, lossp, lterm, lred, span = [], [], [], [], []
for j in heads[:-1]:
    k = j + 1
    while k < len(rows) and "copyBuffer" in rows[k][2]:  # (the guard read-back is not work the step waits for)
        k += 1
    idle.append((rows[k][0] - rows[j][1]) / 1e3)
    k = j + 1
    while k < len(rows) and "loss_terms" not in rows[k][2]:
        k += 1
    if k + 1 < len(rows) and "loss_reduce" in rows[k + 1][2]:
        lterm.append((rows[k][1] - rows[k][0]) / 1e3)
        lred.append((rows[k + 1][1] - rows[k + 1][0]) / 1e3)
        lossp.append((rows[k + 1][1] - rows[k][0]) / 1e3)
    g = j + 1
    while g < len(rows) and "persist" not in rows[g][2]:
        g += 1
    if g < len(rows):
        span.append((rows[g][0] - rows[j][1]) / 1e3)
med = statistics.median
print(f"   idle score head end -> start of the first kernel behind it (the read-back copy aside): median {med(idle):.1f} us (min {min(idle):.1f}, max {max(idle):.1f}) over {len(idle)} boundaries")
print(f"   loss_terms median {med(lterm):.1f} us, loss_reduce median {med(lred):.1f} us, pair first start -> last end median {med(lossp):.1f} us")
print(f"   score head end -> first persistent GEMM start of the next step: median {med(span):.1f} us")
j = heads[-2]
i0 = j
while i0 > 0 and "attn" not in rows[i0][2]:
    i0 -= 1
t0 = rows[j][1]
print("   tail of the step before the last and head of the last step (times relative to the END of the score head):")
i = i0
while i < len(rows):
    s, e, n = rows[i]
    print(f"     {(s - t0) / 1e3:+9.1f} us {(e - s) / 1e3:8.1f} us  {n[:100]}")
    if i > j and "persist" in n:
        break
    i += 1
