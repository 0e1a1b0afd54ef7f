#!/usr/bin/env python3
"""Masks -> COCO compressed RLE (rle_encode.hip, seg_utils.encode_rle_masklet): T = 64 and 200 frames of 720x1280 and
1080x1920 SAM2-like blob masklets, as uint8 masks and as float32 tracker logits.  Prints one JSON object per case:
HIP-event time of each of the three library calls (1 count + scans, 2 emit + character count, 3 characters), the
input bytes over the read phases' time as a fraction of the achievable 6.3 TB/s, the wall time of one
seg_utils.encode_rle_masklet call (size reads and the final character copy included), and, for contrast, the reference's
host path on the same masks: the device-to-host copy of the float32 masklet plus the oracle's numpy encoder (numpy, not
pycocotools).  The strings of a subset of frames are checked against the oracle.
--quick: T=200 1080x1920 only, 3 repetitions, no host path (the target of a rocprofv3 kernel trace)."""
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
quick = "--quick" in sys.argv
if not torch.cuda.is_available():
    sys.exit("bench_rle.py needs a GPU")
L = _lib.lib()


def blobs(T, h, w, seed):
    return mc.blob_masklet(T + 3, h, w, seed)[:T]  # drop the empty / full / white-noise frames blob_masklet ends with


def phases(x, et, reps):
    """HIP-event times (s) of the three calls, averaged over reps; outputs allocated once."""
    n, h, w = x.shape
    s = torch.cuda.current_stream()
    st = _lib.current_stream()
    nb = L.sola_rle_encode_scratch_bytes(n, h, w)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    offs = torch.zeros((2, n + 1), dtype=torch.int64, device="cuda")
    run_off, char_off = offs[0], offs[1]
    _lib.check(L.sola_rle_encode_runs(_lib.ptr(x), et, n, h, w, _lib.ptr(run_off), _lib.ptr(scratch), nb, st), "runs")
    cum = torch.empty(int(run_off[n]), dtype=torch.int32, device="cuda")
    _lib.check(L.sola_rle_encode_cum(_lib.ptr(x), et, n, h, w, _lib.ptr(run_off), _lib.ptr(cum), _lib.ptr(char_off),
                                     _lib.ptr(scratch), nb, st), "cum")
    chars = torch.empty(int(char_off[n]), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tot = np.zeros(3)
    for _ in range(reps):
        ev[0].record(s)
        _lib.check(L.sola_rle_encode_runs(_lib.ptr(x), et, n, h, w, _lib.ptr(run_off), _lib.ptr(scratch), nb, st), "runs")
        ev[1].record(s)
        _lib.check(L.sola_rle_encode_cum(_lib.ptr(x), et, n, h, w, _lib.ptr(run_off), _lib.ptr(cum), _lib.ptr(char_off),
                                         _lib.ptr(scratch), nb, st), "cum")
        ev[2].record(s)
        _lib.check(L.sola_rle_encode_chars(_lib.ptr(cum), _lib.ptr(run_off), _lib.ptr(char_off), n, _lib.ptr(chars), st), "chars")
        ev[3].record(s)
        torch.cuda.synchronize()
        tot += [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(3)]
    return tot / reps, int(cum.numel()), int(chars.numel())


cases = [(200, 1080, 1920)] if quick else [(64, 720, 1280), (200, 720, 1280), (64, 1080, 1920), (200, 1080, 1920)]
pool = {}
for T, h, w in cases:
    if (h, w) not in pool:
        pool[(h, w)] = torch.from_numpy(blobs(max(t for t, hh, ww in cases if (hh, ww) == (h, w)), h, w, seed=h)).cuda()
    m8 = pool[(h, w)][:T].contiguous()
    g = torch.Generator(device="cuda").manual_seed(T + h)
    logits = (m8.float() * 2 - 1) * (0.25 + 8 * torch.rand(m8.shape, device="cuda", generator=g))
    for kind, x in (("uint8", m8), ("float32 logits", logits)):
        lg = kind != "uint8"
        et = 2 if lg else 0
        got = seg_utils.encode_rle_masklet(x, logits=lg)  # warm-up + check on a subset of frames
        ref_frames = m8[:: max(1, T // 8)].cpu().numpy()
        want = [mo.rle_counts_to_string(mo.mask_to_counts(f)) for f in ref_frames]
        assert [r["counts"] for r in got[:: max(1, T // 8)]] == want, "mismatch against the oracle"
        reps = 3 if quick else 10
        (t1, t2, t3), runs, nchars = phases(x, et, reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            seg_utils.encode_rle_masklet(x, logits=lg)
        wall = (time.perf_counter() - t0) / reps
        res = {"workload": f"rle encode T={T} {h}x{w} {kind}", "input_MB": round(x.numel() * x.element_size() / 1e6, 1), "runs": runs,
               "chars": nchars, "phase1_count_us": round(t1 * 1e6, 1), "phase2_emit_us": round(t2 * 1e6, 1),
               "phase3_chars_us": round(t3 * 1e6, 1), "phase1_read_frac_of_6.3TBps": round(x.numel() * x.element_size() / t1 / HBM, 3),
               "phases12_read_frac_of_6.3TBps": round(2 * x.numel() * x.element_size() / (t1 + t2) / HBM, 3),
               "call_ms_wall": round(wall * 1e3, 3)}
        if quick:
            print(json.dumps(res), flush=True)
            continue
        # the reference's host path: the float32 masklet to the host, then encode frame by frame (oracle = numpy restatement)
        f32 = (x > 0).float() if lg else m8.float()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = f32.cpu()
        d2h = time.perf_counter() - t0
        t0 = time.perf_counter()
        hn = host.numpy()
        for f in hn:
            mo.rle_counts_to_string(mo.mask_to_counts(f.astype(np.uint8)))
        enc = time.perf_counter() - t0
        res["host_path_ms (numpy, not pycocotools)"] = {"d2h_f32_masklet": round(d2h * 1e3, 1), "encode": round(enc * 1e3, 1),
                                                         "f32_MB": round(f32.numel() * 4 / 1e6, 1)}
        print(json.dumps(res), flush=True)
        del f32, host, hn
