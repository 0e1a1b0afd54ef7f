#!/usr/bin/env python3
"""Mask-level J&F of one video (jf.hip, seg_utils.compute_JF_batch): 40 SAM2-like blob masklets (36 tracks + 4 GT objects)
and 16 expressions (1-8 selected tracks, 1-2 GT objects each) at 720x1280 and 1080x1920, T = 100 and 200.  Prints one
JSON object per case: HIP-event time of the decode launch (sola_rle_pack_cm) and of the count launch
(sola_mask_select_counts), each launch's traffic over its time as a fraction of 6.3 TB/s (decode: planes written + runs
read; count: the planes every expression reads, and the referenced planes once), the wall time of one compute_JF_batch
call (host parse, uploads, both launches, the copy), and for comparison the per-expression library path
(rle_merge_or of the selected tracks and of the GT objects, then compute_JF: what merged_masklet(device=...) +
compute_JF do, without the file reads) and the host oracle path (numpy decode + OR + compute_J / compute_F) on two
expressions.  Every compared result is checked equal to compute_JF_batch's.

Masklets: blob frames of tests/masklet_cases.py (8 per mask, drifted on the GPU to T frames) encoded by the library's
GPU RLE encoder."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

HBM = 6.3e12
N_TRACKS, N_GT, E = 36, 4, 16
if not torch.cuda.is_available():
    sys.exit("bench_jf.py needs a GPU")
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


def launch_times(masklets, pred, gt, T, h, w, reps):
    """HIP-event seconds of the decode and the count launch (mean of reps after one warm-up) and their bytes."""
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
    st, s = _lib.current_stream(), torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tot = np.zeros(2)
    for r in range(reps + 1):
        ev[0].record(s)
        _lib.check(L.sola_rle_pack_cm(_lib.ptr(cum_t), _lib.ptr(off_t), len(ids) * T, h, w, stride, _lib.ptr(bits), st), "pack")
        ev[1].record(s)
        _lib.check(L.sola_mask_select_counts(_lib.ptr(bits), stride, len(ids), T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(go),
                                             _lib.ptr(gi), E, _lib.ptr(counts), st), "count")
        ev[2].record(s)
        torch.cuda.synchronize()
        if r:
            tot += [ev[0].elapsed_time(ev[1]) * 1e-3, ev[1].elapsed_time(ev[2]) * 1e-3]
    plane = stride * 4
    pack_bytes = len(ids) * T * plane + 4 * len(cum) + 8 * len(off)
    count_bytes = sum(len(a) + len(b) for a, b in zip(pred, gt)) * T * plane
    return tot / reps, pack_bytes, count_bytes, len(ids) * T * plane, counts.cpu()


def per_expression(masklets, ps, gs):
    p = seg_utils.rle_merge_or([masklets[i] for i in ps], dev)
    g = seg_utils.rle_merge_or([masklets[i] for i in gs], dev)
    return seg_utils.compute_JF(p, g)


def oracle(masklets, ps, gs):
    p = np.logical_or.reduce([mo.masklet_decode(masklets[i]) for i in ps])
    g = np.logical_or.reduce([mo.masklet_decode(masklets[i]) for i in gs])
    J, F = mo.compute_J(p, g), mo.compute_F(p, g)
    return J, F, (J + F) / 2


for T, h, w in [(100, 720, 1280), (200, 720, 1280), (100, 1080, 1920), (200, 1080, 1920)]:
    masklets = make_masklets(T, h, w, seed=h + T)
    pred, gt = make_sets(T * h)
    want = seg_utils.compute_JF_batch(masklets, pred, gt, dev)  # warm-up
    (t_pack, t_count), pack_bytes, count_bytes, unique_bytes, counts = launch_times(masklets, pred, gt, T, h, w, 10)
    assert [(float(seg_utils.J_from_counts(c)), float(seg_utils.F_from_counts(c))) for c in counts] == [(j, f) for j, f, _ in want]
    reps = 5
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        got = seg_utils.compute_JF_batch(masklets, pred, gt, dev)
    wall = (time.perf_counter() - t0) / reps
    assert got == want
    per_expression(masklets, pred[0], gt[0])  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per = [per_expression(masklets, ps, gs) for ps, gs in zip(pred, gt)]
    t_per = time.perf_counter() - t0
    assert per == want
    t0 = time.perf_counter()
    host = [oracle(masklets, pred[e], gt[e]) for e in range(2)]
    t_host = (time.perf_counter() - t0) / 2
    assert host == want[:2]
    print(json.dumps({
        "workload": f"J&F T={T} {h}x{w}, {N_TRACKS + N_GT} masks, {E} expressions",
        "referenced_planes_MB": round(unique_bytes / 1e6, 1),
        "decode_us": round(t_pack * 1e6, 1), "decode_frac_of_6.3TBps": round(pack_bytes / t_pack / HBM, 3),
        "count_us": round(t_count * 1e6, 1), "count_frac_of_6.3TBps (per-expression reads)": round(count_bytes / t_count / HBM, 3),
        "count_frac_of_6.3TBps (referenced planes once)": round(unique_bytes / t_count / HBM, 3),
        "compute_JF_batch_ms_wall": round(wall * 1e3, 2),
        "per_expression_path_ms_wall (16 expressions)": round(t_per * 1e3, 1),
        "host_oracle_ms_per_expression (numpy)": round(t_host * 1e3, 1),
    }), flush=True)
    del masklets
