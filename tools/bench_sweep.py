#!/usr/bin/env python3
"""J&F threshold sweep of one video (jf.hip sola_mask_nested_counts, seg_utils.masklet_sweep_counts): the masklets of
tools/bench_jf.py (40 SAM2-like blob masklets = 36 tracks + 4 GT objects, 16 expressions) at 720x1280 and 1080x1920, T = 100 and
200, with every expression's 1-8 candidate tracks entering over K = 4, 9, 19 thresholds.  Prints one JSON object per case:

  a  sola_mask_nested_counts: every level's counts from one pass over the planes of the largest selection (two launches at
     K = 19), median HIP-event time on the stream;
  b  the same numbers from the one-level launch: sola_mask_select_counts with every (expression, level) as a pseudo-expression,
     which reads the planes of each level's prefix again; median HIP-event time;
  c  K separate seg_utils.masklet_select_counts calls (parse, decode, count, copy per threshold), wall;
  d  one seg_utils.masklet_sweep_counts call, wall;

a and b each with the plane bytes they read over their time as a fraction of 6.3 TB/s.  Both sides run in this process on the
same planes after a warm-up; a, b: medians of 20 taken alternately, c, d: medians of 5.  Every route's counts are checked equal."""
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
from sola_amd import _lib, seg_utils  # noqa: E402

HBM = 6.3e12
N_TRACKS, N_GT, E = 36, 4, 16
if not torch.cuda.is_available():
    sys.exit("bench_sweep.py needs a GPU")
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
    cand = [sorted(rng.choice(N_TRACKS, size=int(rng.integers(1, 9)), replace=False).tolist()) for _ in range(E)]
    gt = [sorted((N_TRACKS + rng.choice(N_GT, size=int(rng.integers(1, 3)), replace=False)).tolist()) for _ in range(E)]
    probs = [rng.random(len(c)).astype(np.float32) for c in cand]
    return cand, probs, gt


def median_us(fns, reps):
    """Median HIP-event microseconds of each of ``fns``, taken alternately after one warm-up of each."""
    s = torch.cuda.current_stream()
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return [float(np.median(ts)) for ts in times]


def median_wall_ms(fn, reps):
    out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def i32(x):
    return torch.tensor(list(x) + [0], dtype=torch.int32, device=dev)


for T, h, w in [(100, 720, 1280), (200, 720, 1280), (100, 1080, 1920), (200, 1080, 1920)]:
    masklets = make_masklets(T, h, w, seed=h + T)
    cand, probs, gt = make_sets(T * h)
    stride = L.sola_jf_plane_words(h, w)
    plane = stride * 4
    for K in (4, 9, 19):
        thresholds = [(k + 1) / (K + 1) for k in range(K)]  # ascending, as a user writes them
        levels = [seg_utils.sweep_levels(p, thresholds) for p in probs]
        perm = levels[0][2]
        ordered = [[cand[e][i] for i in levels[e][0]] for e in range(E)]
        ends = [levels[e][1].tolist() for e in range(E)]
        ids = sorted({i for s in ordered + gt for i in s})
        local = {m: k for k, m in enumerate(ids)}
        cum, off = seg_utils._planes_cum(masklets, ids, T, h * w)
        cum_t, off_t = torch.from_numpy(cum.view(np.int32)).to(dev), torch.from_numpy(off).to(dev)
        bits = torch.empty((len(ids) * T, stride), device=dev, dtype=torch.int32)
        st = _lib.current_stream()
        _lib.check(L.sola_rle_pack_cm(_lib.ptr(cum_t), _lib.ptr(off_t), len(ids) * T, h, w, stride, _lib.ptr(bits), st), "pack")
        po, pi = i32(np.cumsum([0] + [len(s) for s in ordered])), i32(local[i] for s in ordered for i in s)
        go, gi = i32(np.cumsum([0] + [len(s) for s in gt])), i32(local[i] for s in gt for i in s)
        le = i32(x for row in ends for x in row)
        prefixes = [ordered[e][:ends[e][k]] for e in range(E) for k in range(K)]
        gts = [gt[e] for e in range(E) for _ in range(K)]
        qo, qi = i32(np.cumsum([0] + [len(s) for s in prefixes])), i32(local[i] for s in prefixes for i in s)
        ho, hi = i32(np.cumsum([0] + [len(s) for s in gts])), i32(local[i] for s in gts for i in s)
        ca = torch.empty((E, K, T, 3), device=dev, dtype=torch.int64)
        cb = torch.empty((E * K, T, 3), device=dev, dtype=torch.int64)

        def route_a():
            _lib.check(L.sola_mask_nested_counts(_lib.ptr(bits), stride, len(ids), T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(le), K,
                                                 _lib.ptr(go), _lib.ptr(gi), E, _lib.ptr(ca), st), "nested")

        def route_b():
            _lib.check(L.sola_mask_select_counts(_lib.ptr(bits), stride, len(ids), T, _lib.ptr(qo), _lib.ptr(qi), _lib.ptr(ho),
                                                 _lib.ptr(hi), E * K, _lib.ptr(cb), st), "select")

        us_a, us_b = median_us([route_a, route_b], 20)
        assert torch.equal(ca.reshape(E * K, T, 3), cb)
        chunks = [range(c, min(c + 16, K)) for c in range(0, K, 16)]  # a reads the prefix of a chunk's last level and the GT per chunk
        bytes_a = sum(ends[e][ch[-1]] + len(gt[e]) for e in range(E) for ch in chunks) * T * plane
        bytes_b = sum(len(p) + len(g) for p, g in zip(prefixes, gts)) * T * plane
        selections = [[[c for c, p in zip(cand[e], probs[e]) if np.float32(p) > np.float32(th)] for e in range(E)] for th in thresholds]
        ms_c, sep = median_wall_ms(lambda: [seg_utils.masklet_select_counts(masklets, s, gt, dev) for s in selections], 5)
        ms_d, swept = median_wall_ms(lambda: seg_utils.masklet_sweep_counts(masklets, cand, probs, thresholds, gt, dev), 5)
        assert torch.equal(swept, torch.stack(sep, 1)) and torch.equal(swept, ca.cpu()[:, torch.from_numpy(perm)])
        print(json.dumps({
            "workload": f"sweep K={K} T={T} {h}x{w}, {N_TRACKS + N_GT} masks, {E} expressions",
            "largest_selection_tracks": sum(e[-1] for e in ends), "sum_of_prefix_tracks": sum(sum(e) for e in ends),
            "a_nested_us": round(us_a, 1), "a_plane_MB": round(bytes_a / 1e6, 1), "a_frac_of_6.3TBps": round(bytes_a / (us_a * 1e-6) / HBM, 3),
            "b_pseudo_expressions_us": round(us_b, 1), "b_plane_MB": round(bytes_b / 1e6, 1),
            "b_frac_of_6.3TBps": round(bytes_b / (us_b * 1e-6) / HBM, 3), "b_over_a": round(us_b / us_a, 2),
            "c_K_select_calls_ms_wall": round(ms_c, 2), "d_one_sweep_call_ms_wall": round(ms_d, 2), "c_over_d": round(ms_c / ms_d, 2),
        }), flush=True)
    del masklets
