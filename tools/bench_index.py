#!/usr/bin/env python3
"""Times sola_index_hist and both layouts of sola_index_pack (index maps -> bit planes) against the host route and the
stock-torch device route on the same maps, and one compute_JF_batch(boundary=True) call on a Ref-DAVIS-like video.

    python tools/bench_index.py [--reps 30]

Every device time is the median of ``--reps`` launches, each between two torch.cuda.Event records after warm-up launches; the
bytes of a launch (maps read once + planes written) are printed over 6.3 TB/s.  The comparison that matters is the kernel
against the stock-torch device route in the same process."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sola_amd import _lib, seg_utils  # noqa: E402
from sola_amd import data as sdata  # noqa: E402

HBM = 6.3e12


def device_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(times)), float(np.min(times))


def video(T, h, w, n_obj, seed=0):
    """Blobby index maps: n_obj ellipses that move, later objects on top."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    maps = np.zeros((T, h, w), np.uint8)
    for k in range(1, n_obj + 1):
        cy, cx, ry, rx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w, rng.uniform(0.08, 0.25) * h, rng.uniform(0.08, 0.25) * w
        vy, vx = rng.uniform(-1, 1), rng.uniform(-2, 2)
        for t in range(T):
            maps[t][((yy - cy - vy * t) / ry) ** 2 + ((xx - cx - vx * t) / rx) ** 2 <= 1.0] = k
    return maps


def line(name, us, nbytes=None, base=None):
    med, low = us
    s = f"  {name:<46s} {med:10.1f} us (min {low:9.1f})"
    if nbytes is not None:
        s += f"  {nbytes / 1e6:8.1f} MB  floor {nbytes / HBM * 1e6:6.1f} us  = {nbytes / HBM * 1e6 / med * 100:5.1f} % of 6.3 TB/s"
    if base is not None:
        s += f"  x{base / med:6.2f} vs torch"
    print(s, flush=True)


def bench_case(T, h, w, n_obj, reps, reference_loop=False):
    print(f"T = {T}, {h}x{w}, {n_obj} objects", flush=True)
    maps = video(T, h, w, n_obj)
    d = torch.from_numpy(maps).cuda()
    ids = list(range(1, n_obj + 1))
    d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    n_in = maps.size
    counts = torch.empty((T, 256), dtype=torch.int64, device="cuda")
    line("sola_index_hist", device_us(lambda: _lib.check(L.sola_index_hist(_lib.ptr(d), T, h, w, _lib.ptr(counts), _lib.current_stream()), "hist"), reps),
         n_in + counts.numel() * 8)
    line("torch: bincount per frame", device_us(lambda: [torch.bincount(f.reshape(-1).int(), minlength=256) for f in d], max(3, reps // 6)))
    for layout, name, words in ((0, "row", L.sola_mask_words(h, w)), (1, "cm", L.sola_jf_plane_words(h, w))):
        bits = torch.empty((n_obj * T, words), dtype=torch.int32, device="cuda")
        area = torch.empty((n_obj * T,), dtype=torch.int64, device="cuda") if layout == 0 else None

        def torch_route():
            m = (d[None] == d_ids[:, None, None, None].to(torch.uint8)).view(n_obj * T, h, w)
            if layout == 1:
                m = m.transpose(1, 2).contiguous()  # compute_F_boundary's way to column-major planes
            return seg_utils.pack_masks(m)

        base = device_us(torch_route, max(3, reps // 3))
        line(f"sola_index_pack layout {layout} ({name})",
             device_us(lambda: _lib.check(L.sola_index_pack(_lib.ptr(d), T, h, w, _lib.ptr(d_ids), n_obj, None, layout, words, _lib.ptr(bits),
                                                            _lib.ptr(area), _lib.current_stream()), "pack"), reps),
             n_in + bits.numel() * 4, base[0])
        line(f"torch: (maps == ids) + pack_masks ({name})", base, None)
        t0 = time.perf_counter()
        for k in ids:
            m = maps == k
            np.packbits((m if layout == 0 else m.transpose(0, 2, 1)).reshape(T, -1), axis=1, bitorder="little")
        print(f"  {'host: [(m == k) for k in ids] + np.packbits (' + name + ')':<46s} {(time.perf_counter() - t0) * 1e6:10.1f} us", flush=True)
    if reference_loop:
        t0 = time.perf_counter()
        out = {}
        for k in range(1, 256):  # track_generation/seg_utils.py:37-48: every id is compared, stacked and summed
            m = np.stack([(f == k).astype(np.float32) for f in maps])
            if m.sum() > 0:
                out[str(k)] = m
        print(f"  {'host: the 255-id loop of get_masklets_ytbvos':<46s} {(time.perf_counter() - t0) * 1e6:10.1f} us", flush=True)


def bench_jf(reps):
    T, h, w, n_obj, n_exp, n_tracks = 80, 480, 854, 3, 12, 20
    print(f"compute_JF_batch(boundary=True): T = {T}, {h}x{w}, {n_obj} objects, {n_exp} expressions, {n_tracks} RLE tracks", flush=True)
    maps = video(T, h, w, n_obj, seed=1)
    d = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(2)
    tracks = []
    for j in range(n_tracks):
        m = video(T, h, w, 1, seed=100 + j)
        tracks.append([sdata.rle_encode_uncompressed(f) for f in m])
    gts = [seg_utils.IndexMasklet(d, k) for k in range(1, n_obj + 1)]
    gts_rle = [[sdata.rle_encode_uncompressed((f == k).astype(np.uint8)) for f in maps] for k in range(1, n_obj + 1)]
    pred_sets = [sorted(set(rng.integers(0, n_tracks, size=4).tolist())) for _ in range(n_exp)]
    gt_sets = [[n_tracks + e % n_obj] for e in range(n_exp)]
    for name, masklets in (("index-map ground truth", tracks + gts), ("RLE ground truth", tracks + gts_rle)):
        times = []
        for _ in range(max(3, reps // 6)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", boundary=True)
            times.append((time.perf_counter() - t0) * 1e3)
        print(f"  {name:<46s} {np.median(times):10.2f} ms wall (min {np.min(times):.2f}), host parse included", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    bench_case(100, 480, 854, 3, a.reps, reference_loop=True)
    bench_case(100, 480, 854, 10, a.reps)
    bench_case(100, 1080, 1920, 10, a.reps)
    bench_jf(a.reps)


if __name__ == "__main__":
    main()
