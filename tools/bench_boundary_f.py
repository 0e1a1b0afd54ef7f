#!/usr/bin/env python3
"""DAVIS boundary F of one video (boundary_f.hip) on bench_jf.py's workload: 40 blob masklets (36 tracks + 4 GT objects),
16 expressions (1-8 selected tracks, 1-2 GT objects each), T = 100, at 540x960, 720x1280 and 1080x1920 with the benchmark's
radius (9 / 12 / 18).  Prints one JSON object per case with HIP-event medians of
  a  the existing decode + count launches (sola_rle_pack_cm + sola_mask_select_counts),
  b  the boundary launch alone (sola_mask_select_boundary_counts on the same planes),
  c  the same four counts from stock PyTorch on the device, starting from the merged uint8 masks of every expression:
     float boundary maps from shifted slices, F.conv2d with the disk, `> 0`, products and sums, one expression per call
     (what a user would write; [T, 1, h, w] float32 per side),
and the ratios b / a and b / c.  Every shape is warmed up; a, b and c alternate inside one run; (b)'s counts are checked
equal to (c)'s and, at --check frames, to the numpy restatement of tests/boundary_cases.py.

    python tools/bench_boundary_f.py [--shapes 540x960,720x1280,1080x1920] [--frames 100] [--reps 10] [--stock_reps 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boundary_cases as bc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="540x960,720x1280,1080x1920")
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--stock_reps", type=int, default=3)
ap.add_argument("--check", type=int, default=2, help="frames of expression 0 compared with the numpy restatement")
args = ap.parse_args()

N_TRACKS, N_GT, E = 36, 4, 16
if not torch.cuda.is_available():
    sys.exit("bench_boundary_f.py needs a GPU")
L = _lib.lib()
dev = torch.device("cuda")


def make_masklets(T, h, w, seed):
    out = []
    for k in range(N_TRACKS + N_GT):
        base = torch.from_numpy(mc.blob_masklet(11, h, w, seed * 100 + k)[:8]).to(dev)  # without the empty / full / noise frames
        frames = torch.stack([torch.roll(base[t % 8], shifts=((7 * t) % h, (13 * t) % w), dims=(0, 1)) for t in range(T)])
        out.append(seg_utils.encode_rle_masklet(frames))
    return out


def make_sets(seed):
    rng = np.random.default_rng(seed)
    pred = [sorted(rng.choice(N_TRACKS, size=int(rng.integers(1, 9)), replace=False).tolist()) for _ in range(E)]
    gt = [sorted((N_TRACKS + rng.choice(N_GT, size=int(rng.integers(1, 3)), replace=False)).tolist()) for _ in range(E)]
    return pred, gt


def stock_counts(fg, gt, disk):
    """[T,h,w] uint8 x2 -> int64 [T,4] with stock PyTorch ops."""
    def boundary(m):
        m = m.float()
        b = torch.zeros_like(m)
        b[:, :, :-1] += (m[:, :, :-1] != m[:, :, 1:]).float()
        b[:, :-1, :] += (m[:, :-1, :] != m[:, 1:, :]).float()
        b[:, :-1, :-1] += (m[:, :-1, :-1] != m[:, 1:, 1:]).float()
        return (b > 0).float()

    def dilate(b):
        return (F.conv2d(b[:, None], disk, padding=disk.shape[-1] // 2)[:, 0] > 0).float()

    bf, bg = boundary(fg), boundary(gt)
    return torch.stack([bf.sum((1, 2)), bg.sum((1, 2)), (bf * dilate(bg)).sum((1, 2)), (bg * dilate(bf)).sum((1, 2))], 1).long()


def median_ms(samples):
    return float(np.median(samples))


for shape in args.shapes.split(","):
    h, w = (int(v) for v in shape.split("x"))
    T = args.frames
    r = seg_utils.boundary_radius(h, w)
    masklets = make_masklets(T, h, w, seed=h + T)
    pred, gt = make_sets(T * h)
    ids = sorted({i for s in pred + gt for i in s})
    local = {m: k for k, m in enumerate(ids)}
    cum, off = seg_utils._planes_cum(masklets, ids, T, h * w)
    stride = L.sola_jf_plane_words(h, w)
    cum_t = torch.from_numpy(cum.view(np.int32)).to(dev)
    off_t = torch.from_numpy(off).to(dev)
    bits = torch.empty((len(ids) * T, stride), device=dev, dtype=torch.int32)
    po = torch.tensor(np.cumsum([0] + [len(s) for s in pred]), dtype=torch.int32, device=dev)
    go = torch.tensor(np.cumsum([0] + [len(s) for s in gt]), dtype=torch.int32, device=dev)
    pi = torch.tensor([local[i] for s in pred for i in s], dtype=torch.int32, device=dev)
    gi = torch.tensor([local[i] for s in gt for i in s], dtype=torch.int32, device=dev)
    counts = torch.empty((E, T, 3), device=dev, dtype=torch.int64)
    bcounts = torch.empty((E, T, 4), device=dev, dtype=torch.int64)
    # (c)'s inputs: every expression's merged masks, unpacked
    merged = [(seg_utils.rle_merge_or([masklets[i] for i in ps], dev), seg_utils.rle_merge_or([masklets[i] for i in gs], dev))
              for ps, gs in zip(pred, gt)]
    disk = torch.from_numpy(bc.disk(r).astype(np.float32)).to(dev)[None, None]
    st, s = _lib.current_stream(), torch.cuda.current_stream()

    def run_a():
        _lib.check(L.sola_rle_pack_cm(_lib.ptr(cum_t), _lib.ptr(off_t), len(ids) * T, h, w, stride, _lib.ptr(bits), st), "pack")
        _lib.check(L.sola_mask_select_counts(_lib.ptr(bits), stride, len(ids), T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(go),
                                             _lib.ptr(gi), E, _lib.ptr(counts), st), "count")

    def run_b():
        _lib.check(L.sola_mask_select_boundary_counts(_lib.ptr(bits), stride, len(ids), T, h, w, r, _lib.ptr(po), _lib.ptr(pi),
                                                      _lib.ptr(go), _lib.ptr(gi), E, _lib.ptr(bcounts), None, 0, st), "boundary")

    stock = [None]

    def run_c():
        stock[0] = torch.stack([stock_counts(p, g, disk) for p, g in merged])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for fn in (run_a, run_b, run_c):  # warm-up of this shape
        timed(fn)
    ta, tb, tc = [], [], []
    for rep in range(args.reps):  # alternating
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        if rep < args.stock_reps:
            tc.append(timed(run_c))
    got = bcounts.cpu()
    assert torch.equal(got, stock[0].cpu()), "boundary counts differ from the stock PyTorch formulation"
    for t in range(min(args.check, T)):
        want = bc.boundary_counts(merged[0][0][t].cpu().numpy(), merged[0][1][t].cpu().numpy(), r, bc.disk_dilate_rows)
        assert np.array_equal(got[0, t].numpy(), want), "boundary counts differ from the numpy restatement"
    a, b, c = median_ms(ta), median_ms(tb), median_ms(tc)
    print(json.dumps({
        "workload": f"boundary F T={T} {h}x{w} radius {r}, {N_TRACKS + N_GT} masks, {E} expressions",
        "a_decode_plus_count_ms": round(a, 3), "b_boundary_ms": round(b, 3), "c_stock_pytorch_ms": round(c, 3),
        "b_over_a": round(b / a, 3), "b_over_c": round(b / c, 5), "b_le_c": bool(b <= c),
        "reps": args.reps, "stock_reps": len(tc), "b_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
        "counts_equal_stock": True,
    }), flush=True)
    del masklets, merged
