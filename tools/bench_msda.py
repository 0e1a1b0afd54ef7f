#!/usr/bin/env python3
"""Times sola_ms_deform_attn (multi-scale deformable attention, forward; DESIGN row f13) against the public torch statement of the
same operator (one F.grid_sample per level, weighted and summed: the route GroundingDINO's own fallback takes) on the device.

    python tools/bench_msda.py [--reps 30]

Shapes: N = 1, M = 8, D = 32, L = 4, P = 4 over the levels of an 800 x 1333 image at strides 8 to 64 (100x167, 50x84, 25x42,
13x21; S = 22 223).  Encoder: Lq = S, every query samples around its own pixel's reference point (offsets of a few pixels, the
pattern of a trained encoder) and, as the other extreme, uniformly anywhere.  Decoder: Lq = 900, uniform.

Every time is the median of ``--reps`` calls, each between two torch.cuda.Event records, after warm-up calls; the kernel and
the torch statement alternate call by call inside one loop.  Printed per case: the launch's algorithmic bytes (value once,
locations, weights, output) and the gathered bytes (N Lq M L P x 4 corners x D x 4) with both as rates over the kernel's
median, and the largest difference between the two outputs."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import msda_cases as mc  # noqa: E402
from sola_amd import ops  # noqa: E402

LEVELS = ((100, 167), (50, 84), (25, 42), (13, 21))
M, D, P = 8, 32, 4


def reference_points(levels):
    """[S, 2] normalised (x, y) pixel centres of every level, in level order: the encoder's queries."""
    pts = []
    for h, w in levels:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")
        pts.append(torch.stack([xs.flatten(), ys.flatten()], -1))
    return torch.cat(pts)


def inputs(kind, seed=0):
    shapes, start, S = mc.level_tables(LEVELS)
    L = len(LEVELS)
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(1, S, M, D, generator=g)
    Lq = 900 if kind == "decoder" else S
    if kind == "encoder-near":  # reference point + offsets of about two pixels of the sampled level
        ref = reference_points(LEVELS).view(1, S, 1, 1, 1, 2)
        wh = torch.tensor([[w, h] for h, w in LEVELS], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
        loc = ref + torch.randn(1, Lq, M, L, P, 2, generator=g) * 2.0 / wh
    else:
        loc = torch.rand(1, Lq, M, L, P, 2, generator=g)
    w = torch.softmax(torch.randn(1, Lq, M, L * P, generator=g), -1).reshape(1, Lq, M, L, P)
    return value, shapes, start, loc, w


def alternate_us(fns, reps, warmup=5):
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1000.0)
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_msda.py needs a GPU: nothing is measured without one")
    print(f"sola_ms_deform_attn vs the torch grid_sample statement; N=1 M={M} D={D} L={len(LEVELS)} P={P}, levels {LEVELS}; "
          f"{torch.cuda.get_device_name(0)}; medians of {args.reps} alternating calls between device events", flush=True)
    for kind in ("encoder-near", "encoder-uniform", "decoder"):
        value, shapes, start, loc, w = inputs(kind)
        S, Lq, L = value.shape[1], loc.shape[1], loc.shape[3]
        dev = [t.cuda() for t in (value, shapes, start, loc, w)]
        algo = 4 * (value.numel() + loc.numel() + w.numel() + Lq * M * D)
        gathered = Lq * M * L * P * 4 * D * 4
        out = ops.ms_deform_attn(*dev)
        ref = mc.statement(dev[0], shapes, start, dev[3], dev[4], torch.float32)
        diff = float((out - ref).abs().max())
        (k_med, k_min), (t_med, t_min) = alternate_us(
            [lambda: ops.ms_deform_attn(*dev), lambda: mc.statement(dev[0], shapes, start, dev[3], dev[4], torch.float32)], args.reps)
        print(f"{kind}: Lq = {Lq}, S = {S}", flush=True)
        print(f"  sola_ms_deform_attn        {k_med:9.1f} us (min {k_min:9.1f})   algorithmic {algo / 1e6:7.1f} MB = {algo / k_med / 1e6:6.2f} TB/s"
              f"   gathered {gathered / 1e6:7.1f} MB = {gathered / k_med / 1e6:6.2f} TB/s", flush=True)
        print(f"  torch grid_sample statement {t_med:8.1f} us (min {t_min:9.1f})   x{t_med / k_med:6.2f} the kernel's time;"
              f" max |difference of the outputs| {diff:.2e}", flush=True)


if __name__ == "__main__":
    main()
