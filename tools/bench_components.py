#!/usr/bin/env python3
"""fill_holes_in_mask_scores (components.hip) against the only stock route a ROCm user has: copy the scores to the host and
run ``scipy.ndimage.label`` per frame, on the same scores in the same process.  Cases: blob scores [8,256,256] and
[4,1024,1024] and 100 frames of 1080x1920, each sprinkled with holes of 1-12 pixels; one all-background 1080p frame (a single
component of every pixel); the serpentine of the tests at 540x960 as background (the deep-tree case).  Prints one JSON
object per case: HIP-event medians (and min-max) of the four launches of one call (sola_mask_fill_small_profile: tile
labelling, tile borders, flatten + counts, rewrite), each launch's bytes over its time as a fraction of 6.3 TB/s, the
HIP-event and wall medians of one ``fill_holes_in_mask_scores`` call, the wall median of the host copy + scipy path where
scipy is present, and their ratio.  Frame 0 of every case is checked against scipy's components.
Bytes per launch (float32 scores, int32 parent / count): tile = 12 per pixel (scores in, parent and count out); borders =
24 per tile-edge pixel (its own and its neighbours' parents; the union chains are not counted); flatten = 4 per pixel (count);
rewrite = 12 per pixel (scores and parent in, scores out; the two gathers behind a set pixel are not counted)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_cases as cc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

HBM = 6.3e12
MAX_AREA = 8
if not torch.cuda.is_available():
    sys.exit("bench_components.py needs a GPU")
L = _lib.lib()
dev = torch.device("cuda")
LAUNCHES = ["tile", "borders", "flatten", "rewrite"]


def blob_scores(T, h, w, seed, holes_per_frame):
    """+2 on drifting blobs, -2 elsewhere, and boxes of 1-12 pixels of -1 sprinkled over every frame."""
    base = torch.from_numpy(mc.blob_masklet(11, h, w, seed)[:8]).to(dev)
    m = torch.stack([torch.roll(base[t % 8], shifts=((7 * t) % h, (13 * t) % w), dims=(0, 1)) for t in range(T)])
    s = torch.where(m != 0, 2.0, -2.0).float().contiguous()
    rng = np.random.default_rng(seed)
    for t in range(T):
        ys, xs = rng.integers(0, h - 3, holes_per_frame), rng.integers(0, w - 4, holes_per_frame)
        hh, ww = rng.integers(1, 4, holes_per_frame), rng.integers(1, 5, holes_per_frame)
        for y, x, a, b in zip(ys.tolist(), xs.tolist(), hh.tolist(), ww.tolist()):
            s[t, y:y + a, x:x + b] = -1.0
    return s


def launch_times(x, reps):
    n, h, w = x.shape
    nb = L.sola_mask_components_scratch_bytes(n, h, w)
    scratch = torch.empty(nb, device=dev, dtype=torch.uint8)
    out = torch.empty_like(x)
    us = (ctypes.c_float * 4)()
    rows = []
    for r in range(reps + 1):
        _lib.check(L.sola_mask_fill_small_profile(_lib.ptr(x), 3, n, h, w, 8, MAX_AREA, 0.1, _lib.ptr(out), _lib.ptr(scratch), nb,
                                                  _lib.current_stream(), us), "sola_mask_fill_small_profile")
        if r:
            rows.append([us[i] * 1e-6 for i in range(4)])
    return [[row[i] for row in rows] for i in range(4)]


def call_times(x, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    s, ts, wall = torch.cuda.current_stream(), [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record(s)
        seg_utils.fill_holes_in_mask_scores(x, MAX_AREA)
        ev[1].record(s)
        torch.cuda.synchronize()
        if r:
            wall.append(time.perf_counter() - t0)
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return ts, wall


def scipy_path(x):
    out = []
    for f in x.cpu().numpy():
        out.append(ndimage.label(f <= 0, structure=np.ones((3, 3), int)))
    return out


def check_frame0(x):
    got = seg_utils.fill_holes_in_mask_scores(x[:1], MAX_AREA)[0].cpu().numpy()
    f = x[0].cpu().numpy()
    lab, n = ndimage.label(f <= 0, structure=np.ones((3, 3), int))
    small = (np.bincount(lab.ravel(), minlength=n + 1) <= MAX_AREA)[lab] & (lab > 0)
    want = f.copy()
    want[small] = np.float32(0.1)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    return int(small.sum())


def spread(ts, scale):
    return {"median": round(statistics.median(ts) * scale, 2), "min": round(min(ts) * scale, 2), "max": round(max(ts) * scale, 2)}


cases = [("blobs+holes [8,256,256]", lambda: blob_scores(8, 256, 256, 3, 40)),
         ("blobs+holes [4,1024,1024]", lambda: blob_scores(4, 1024, 1024, 4, 400)),
         ("blobs+holes [100,1080,1920]", lambda: blob_scores(100, 1080, 1920, 5, 300)),
         ("all background [1,1080,1920]", lambda: torch.full((1, 1080, 1920), -1.0, device=dev)),
         ("serpentine background [1,540,960]", lambda: torch.from_numpy(np.where(cc.serpentine(540, 960) != 0, -1.0, 1.0).astype(np.float32))[None].to(dev))]
for name, make in cases:
    x = make()
    n, h, w = x.shape
    filled0 = check_frame0(x) if ndimage is not None else None
    per_launch = launch_times(x, 10)
    t_call, t_wall = call_times(x, 10)
    px = x.numel()
    ty, tx = (h + seg_utils.CC_TILE[0] - 1) // seg_utils.CC_TILE[0], (w + seg_utils.CC_TILE[1] - 1) // seg_utils.CC_TILE[1]
    nbytes = [12 * px, 24 * n * ((ty - 1) * w + (tx - 1) * h), 4 * px, 12 * px]
    row = {"workload": name, "scores_MB": round(px * 4 / 1e6, 1), "max_area": MAX_AREA, "filled_pixels_frame0": filled0}
    for i, ln in enumerate(LAUNCHES):
        row[f"{ln}_us"] = spread(per_launch[i], 1e6)
        row[f"{ln}_frac_of_6.3TBps"] = round(nbytes[i] / statistics.median(per_launch[i]) / HBM, 4)
    row["fill_holes_call_us_events"] = spread(t_call, 1e6)
    row["fill_holes_call_ms_wall"] = spread(t_wall, 1e3)
    if ndimage is not None:
        t_host = []
        for _ in range(3 if n < 50 else 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scipy_path(x)
            t_host.append(time.perf_counter() - t0)
        row["d2h_scipy_label_ms_wall"] = spread(t_host, 1e3)
        row["gpu_over_scipy"] = round(statistics.median(t_wall) / statistics.median(t_host), 5)
    print(json.dumps(row), flush=True)
    del x
