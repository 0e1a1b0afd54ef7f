#!/usr/bin/env python3
"""Times sola_ms_deform_attn_backward (multi-scale deformable attention, backward; DESIGN row f14) against torch autograd's
backward of the public statement of the operator (one F.grid_sample per level, weighted and summed) on the device.

    python tools/bench_msda_bwd.py [--reps 30] [--head_dim 32]

Shapes and location patterns are bench_msda.py's: N = 1, M = 8, D = 32, L = 4, P = 4 over the levels of an 800 x 1333 image;
encoder (Lq = S = 22 223) with locations near the query's own pixel and uniform ones, decoder (Lq = 900, uniform).
``--head_dim 16`` / ``64`` run the same cases at the other two head widths (an atomic wave-instruction is then four 64-byte
row segments / one 256-byte row instead of two 128-byte ones).

Timed, alternating call by call inside one loop, medians of ``--reps`` calls between device events after warm-up calls:
the backward with all three outputs (the memset of grad_value included), the backward without grad_value, and
torch.autograd.grad of the float32 statement (the backward alone: its graph is recorded once, outside the timing).
Printed per case: the bytes the call adds to grad_value with float atomics (counting corners x D x 4) over the time of the full
call, next to the 1.3 TB/s at which the chip adds them, and the largest differences between the two routes' gradients."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_msda  # noqa: E402  (also puts the repository and tests/ on the path)
from bench_msda import LEVELS, M, P, alternate_us, inputs  # noqa: E402
import msda_cases as mc  # noqa: E402
from sola_amd import ops  # noqa: E402

ATOMIC_TBS = 1.3  # chip-wide rate of float32 atomic adds, in added bytes


def counting_corners(shapes, loc):
    """How many of the N Lq M L P x 4 corners lie inside their map (well-formed tables: every such row is in value)."""
    size = shapes.flip(-1).to(torch.float64).view(1, 1, 1, -1, 1, 2)
    p0 = torch.floor(loc.double() * size - 0.5)
    total = 0
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = p0[..., 0] + dx, p0[..., 1] + dy
            total += int(((x >= 0) & (x < size[..., 0]) & (y >= 0) & (y < size[..., 1])).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--head_dim", type=int, default=bench_msda.D, choices=ops.MSDA_HEAD_DIMS)
    args = ap.parse_args()
    D = bench_msda.D = args.head_dim  # inputs() builds value with it
    if not torch.cuda.is_available():
        sys.exit("bench_msda_bwd.py needs a GPU: nothing is measured without one")
    print(f"sola_ms_deform_attn_backward vs torch autograd through the grid_sample statement; N=1 M={M} D={D} L={len(LEVELS)} P={P}, "
          f"levels {LEVELS}; {torch.cuda.get_device_name(0)}; medians of {args.reps} alternating calls between device events", flush=True)
    for kind in ("encoder-near", "encoder-uniform", "decoder"):
        value, shapes, start, loc, w = inputs(kind)
        S, Lq = value.shape[1], loc.shape[1]
        grad_out = torch.randn(1, Lq, M * D, generator=torch.Generator().manual_seed(1))
        atomic_bytes = counting_corners(shapes, loc) * D * 4
        dev = [t.cuda() for t in (value, shapes, start, loc, w, grad_out)]
        leaves = [dev[i].clone().requires_grad_(True) for i in (0, 3, 4)]
        out = mc.statement(leaves[0], shapes, start, leaves[1], leaves[2], torch.float32)
        torch_bwd = lambda: torch.autograd.grad(out, leaves, dev[5], retain_graph=True)  # noqa: E731
        got, ref = ops.ms_deform_attn_backward(*dev), torch_bwd()
        diffs = [float((a - b).abs().max()) for a, b in zip(got, ref)]
        (f_med, f_min), (p_med, p_min), (t_med, t_min) = alternate_us(
            [lambda: ops.ms_deform_attn_backward(*dev), lambda: ops.ms_deform_attn_backward(*dev, need=(False, True, True)), torch_bwd], args.reps)
        rate = atomic_bytes / f_med / 1e6
        print(f"{kind}: Lq = {Lq}, S = {S}", flush=True)
        print(f"  backward, all three gradients   {f_med:9.1f} us (min {f_min:9.1f})   atomic adds {atomic_bytes / 1e6:7.1f} MB = {rate:5.2f} TB/s"
              f" = {100 * rate / ATOMIC_TBS:5.1f} % of {ATOMIC_TBS} TB/s (floor {atomic_bytes / ATOMIC_TBS / 1e6:7.1f} us)", flush=True)
        print(f"  backward without grad_value     {p_med:9.1f} us (min {p_min:9.1f})", flush=True)
        print(f"  torch autograd of the statement {t_med:9.1f} us (min {t_min:9.1f})   x{t_med / f_med:6.2f} the full call's time;"
              f" max |difference| grad_value {diffs[0]:.2e}  grad_loc {diffs[1]:.2e}  grad_weight {diffs[2]:.2e}", flush=True)


if __name__ == "__main__":
    main()
