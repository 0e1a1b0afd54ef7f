#!/usr/bin/env python3
"""Every threshold's PNG files of a video from one decode (seg_utils.encode_png_sweep: sola_planes_cm_to_rm +
sola_png_deflate_sizes_select + sola_png_deflate_write) against the route it replaces, ``rle_merge_or`` +
``encode_png_masklet`` per (expression, threshold), on the same RLE tracks in the same process, alternating.

A video has 40 tracks (blob masklets of tests/masklet_cases.py, drifted on the GPU and RLE-encoded by encode_rle_masklet) and 16
expressions over all of them with scores ``u**3`` (u uniform: about 8 tracks above 0.5, 21 above 0.1); 720x1280 / 1080x1920,
T = 100 / 200, K = 1 / 4 / 9 thresholds around 0.5, plus the single-expression single-threshold video (E = 1, K = 1) that decides
whether inference.py keeps save_masklet there.  Prints one JSON object per case: HIP-event medians (min-max) of the transpose
launch over the 40 tracks' planes, of the select-sizes call and of the write call over the first scratch block (its expressions
and streams are given), wall-time median and spread of one encode_png_sweep call and of the parent route, and their ratio.  The
files of both routes are compared byte for byte.

usage: python tools/bench_png_select.py [--quick]   (--quick: 720x1280, T = 100 only)"""
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
import masklet_cases as mc  # noqa: E402
from sola_amd import _lib, seg_utils as su  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_png_select.py needs a GPU")
L = _lib.lib()
dev = torch.device("cuda")
M, E_FULL = 40, 16
MAX_SCRATCH = 1 << 30


def tracks(T, h, w):
    out = []
    for m in range(M):
        base = torch.from_numpy(mc.blob_masklet(11, h, w, 100 + m)[:8]).to(dev)
        x = torch.stack([torch.roll(base[(t + m) % 8], shifts=((7 * t + 31 * m) % h, (13 * t + 57 * m) % w), dims=(0, 1)) for t in range(T)])
        out.append(su.encode_rle_masklet(x.contiguous()))
    return out


def thresholds(K):
    return {1: [0.5], 4: [0.3, 0.4, 0.5, 0.6], 9: [round(0.1 * i, 1) for i in range(1, 10)]}[K]


def parent_route(rles, cand, probs, ths, T, h, w):
    out = []
    for c, p in zip(cand, probs):
        per = []
        for t in ths:
            sel = [rles[i] for i, q in zip(c, p) if np.float32(q) > np.float32(t)]
            masklet = su.rle_merge_or(sel, dev) if sel else torch.zeros((T, h, w), dtype=torch.uint8, device=dev)
            per.append(su.encode_png_masklet(masklet))
        out.append(per)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def spread(ts, scale, nd=2):
    return {"median": round(statistics.median(ts) * scale, nd), "min": round(min(ts) * scale, nd), "max": round(max(ts) * scale, nd)}


def launch_times(rles, cand, probs, ths, T, h, w, reps):
    """HIP-event seconds of the transpose over every track's planes and of the two PNG calls over the first scratch block."""
    K = len(ths)
    stride_cm = L.sola_jf_plane_words(h, w)
    (grp, local, cm, n_ids), = list(su._plane_groups(rles, [list(range(M))], T, h, w, stride_cm, dev, 1 << 40))
    rm = su.planes_cm_to_rm(cm, h, w)
    kc = min(16, K)
    fit = 1
    while fit < len(cand) and L.sola_png_deflate_scratch_bytes((fit + 1) * kc * T, h, w) <= MAX_SCRATCH:
        fit += 1
    off, idx, lend = [0], [], []
    for c, p in zip(cand[:fit], probs[:fit]):
        order, level_end, _ = su.sweep_levels(p, ths)
        idx += [local[c[i]] for i in order]
        off.append(len(idx))
        lend += level_end.tolist()[:kc]
    ints = torch.tensor(lend + off + idx + [0], dtype=torch.int32, device=dev)
    d_lend, d_off, d_idx = _lib.ptr(ints), _lib.ptr(ints[len(lend):]), _lib.ptr(ints[len(lend) + len(off):])
    n = fit * kc * T
    nb = L.sola_png_deflate_scratch_bytes(n, h, w)
    scratch = torch.empty((nb + 7) // 8, device=dev, dtype=torch.int64)
    boff = torch.empty(n + 1, device=dev, dtype=torch.int64)
    adler = torch.empty(n, device=dev, dtype=torch.int32)
    st, s = _lib.current_stream(), torch.cuda.current_stream()

    def sizes():
        _lib.check(L.sola_png_deflate_sizes_select(_lib.ptr(rm), rm.shape[1], n_ids, T, h, w, d_off, d_idx, d_lend, kc, fit, _lib.ptr(boff),
                                                   _lib.ptr(adler), _lib.ptr(scratch), nb, st), "sizes_select")

    sizes()
    total = int(boff[n])
    out = torch.empty(total, device=dev, dtype=torch.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    a, b, c = [], [], []
    for r in range(reps + 1):
        ev[0].record(s)
        su.planes_cm_to_rm(cm, h, w, out=rm)
        ev[1].record(s)
        sizes()
        ev[2].record(s)
        _lib.check(L.sola_png_deflate_write(_lib.ptr(rm), 0, n, h, w, _lib.ptr(boff), _lib.ptr(adler), _lib.ptr(out), _lib.ptr(scratch), nb, st),
                   "write")
        ev[3].record(s)
        torch.cuda.synchronize()
        if r:
            a.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            b.append(ev[1].elapsed_time(ev[2]) * 1e-3)
            c.append(ev[2].elapsed_time(ev[3]) * 1e-3)
    plane_bytes = 2 * cm.numel() * 4  # read once, written once
    return a, b, c, fit, n, plane_bytes, total


quick = "--quick" in sys.argv
shapes = [(720, 1280, 100)] if quick else [(720, 1280, 100), (720, 1280, 200), (1080, 1920, 100), (1080, 1920, 200)]
for h, w, T in shapes:
    rles = tracks(T, h, w)
    rng = np.random.default_rng(h + T)
    cases = [(E_FULL, K) for K in (1, 4, 9)] + ([(1, 1)] if T == 100 else [])
    for E, K in cases:
        ths = thresholds(K)
        cand = [list(range(M)) for _ in range(E)]
        probs = [(rng.random(M) ** 3).astype(np.float32) for _ in range(E)]
        new = su.encode_png_sweep(rles, cand, probs, ths, dev)  # warm-up, and the files of both routes are the same
        old = parent_route(rles, cand, probs, ths, T, h, w)
        assert new == old, (h, w, T, E, K)
        t_new, t_old = [], []
        for _ in range(3):  # alternating
            _, t = wall(lambda: su.encode_png_sweep(rles, cand, probs, ths, dev))
            t_new.append(t)
            _, t = wall(lambda: parent_route(rles, cand, probs, ths, T, h, w))
            t_old.append(t)
        tr, sz, wr, fit, n, plane_bytes, total = launch_times(rles, cand, probs, ths, T, h, w, 5)
        sel = [int((p > np.float32(t)).sum()) for p in probs for t in ths]
        print(json.dumps({
            "workload": f"{h}x{w} T={T} M={M} E={E} K={K}", "tracks_selected_per_level_mean": round(float(np.mean(sel)), 1),
            "transpose_us": spread(tr, 1e6, 1), "transpose_frac_of_6.3TBps": round(plane_bytes / statistics.median(tr) / 6.3e12, 3),
            "first_block": {"expressions": fit, "streams": n, "stream_MB": round(total / 1e6, 1)},
            "select_sizes_us": spread(sz, 1e6, 1), "write_us": spread(wr, 1e6, 1),
            "encode_png_sweep_ms_wall": spread(t_new, 1e3), "parent_route_ms_wall": spread(t_old, 1e3),
            "sweep_over_parent": round(statistics.median(t_new) / statistics.median(t_old), 4),
            "files_MB": round(sum(len(f) for e in new for k in e for f in k) / 1e6, 1),
        }), flush=True)
    del rles
