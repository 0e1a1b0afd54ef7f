#!/usr/bin/env python3
"""Masklet -> PNG files (png_encode.hip, seg_utils.encode_png_masklet) against the path it replaces in inference.py (copy the
masklet to the host, one ``PIL.Image.save`` per frame), on the same masks in the same process.  Cases: T = 100 and 200 blob
frames (tests/masklet_cases.py, drifted on the GPU) at 720x1280 and 1080x1920, plus all-empty and noise (p = 0.5) masklets
of T = 100 at 1080x1920.  Prints one JSON object per case: HIP-event median (and min-max) of the sizes call and the write
call, each call's bytes over its time as a fraction of 6.3 TB/s (sizes: masks read once + raw bitmap written; write:
bitmap read + streams written - the masks are read once per encode, the two calls share their scan through the scratch),
wall-time median and spread of one ``encode_png_masklet`` call, the same for the PIL path, their ratio, and the bytes of
both outputs.  Every GPU file is opened with PIL and compared with the mask."""
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import masklet_cases as mc  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

HBM = 6.3e12
if not torch.cuda.is_available():
    sys.exit("bench_png.py needs a GPU")
L = _lib.lib()
dev = torch.device("cuda")


def blobs(T, h, w, seed):
    base = torch.from_numpy(mc.blob_masklet(11, h, w, seed)[:8]).to(dev)  # without the empty / full / noise frames
    return torch.stack([torch.roll(base[t % 8], shifts=((7 * t) % h, (13 * t) % w), dims=(0, 1)) for t in range(T)]).contiguous()


def launch_times(x, reps):
    """HIP-event seconds of the two calls (reps after one warm-up) and the size of the streams."""
    n, h, w = x.shape
    nb = L.sola_png_deflate_scratch_bytes(n, h, w)
    scratch = torch.empty(nb // 8, device=dev, dtype=torch.int64)
    off = torch.empty(n + 1, device=dev, dtype=torch.int64)
    adler = torch.empty(n, device=dev, dtype=torch.int32)
    st, s = _lib.current_stream(), torch.cuda.current_stream()
    _lib.check(L.sola_png_deflate_sizes(_lib.ptr(x), 0, n, h, w, _lib.ptr(off), _lib.ptr(adler), _lib.ptr(scratch), nb, st), "sizes")
    total = int(off[n])
    out = torch.empty(total, device=dev, dtype=torch.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    a, b = [], []
    for r in range(reps + 1):
        ev[0].record(s)
        _lib.check(L.sola_png_deflate_sizes(_lib.ptr(x), 0, n, h, w, _lib.ptr(off), _lib.ptr(adler), _lib.ptr(scratch), nb, st), "sizes")
        ev[1].record(s)
        _lib.check(L.sola_png_deflate_write(_lib.ptr(x), 0, n, h, w, _lib.ptr(off), _lib.ptr(adler), _lib.ptr(out), _lib.ptr(scratch), nb, st),
                   "write")
        ev[2].record(s)
        torch.cuda.synchronize()
        if r:
            a.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            b.append(ev[1].elapsed_time(ev[2]) * 1e-3)
    bitmap = n * ((h * (w + 1) + 63) // 64) * 8
    return a, b, x.numel() + bitmap, bitmap + total, total


def pil_path(x):
    out = []
    for m in x.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray((np.asarray(m) * 255).astype(np.uint8)).save(buf, "PNG")
        out.append(buf.getvalue())
    return out


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, ts


def spread(ts, scale):
    return {"median": round(statistics.median(ts) * scale, 2), "min": round(min(ts) * scale, 2), "max": round(max(ts) * scale, 2)}


cases = [(f"blobs T={T} {h}x{w}", lambda T=T, h=h, w=w: blobs(T, h, w, h + T)) for h, w in ((720, 1280), (1080, 1920)) for T in (100, 200)]
cases.append(("empty T=100 1080x1920", lambda: torch.zeros((100, 1080, 1920), dtype=torch.uint8, device=dev)))
cases.append(("noise T=100 1080x1920", lambda: (torch.rand((100, 1080, 1920), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.5).to(torch.uint8)))
for name, make in cases:
    x = make()
    files = seg_utils.encode_png_masklet(x)  # warm-up
    host = x.cpu().numpy()
    for t in range(0, len(files), 7):
        img = Image.open(io.BytesIO(files[t]))
        assert img.mode == "L" and np.array_equal(np.array(img), host[t] * 255), (name, t)
    t_sizes, t_write, sizes_bytes, write_bytes, total = launch_times(x, 10)
    files, t_gpu = wall(lambda: seg_utils.encode_png_masklet(x), 7)
    pil, t_pil = wall(lambda: pil_path(x), 3 if "noise" not in name else 2)
    ms, mw = statistics.median(t_sizes), statistics.median(t_write)
    print(json.dumps({
        "workload": name, "mask_MB": round(x.numel() / 1e6, 1),
        "sizes_call_us": spread(t_sizes, 1e6), "sizes_frac_of_6.3TBps": round(sizes_bytes / ms / HBM, 3),
        "write_call_us": spread(t_write, 1e6), "write_frac_of_6.3TBps": round(write_bytes / mw / HBM, 4),
        "encode_png_masklet_ms_wall": spread(t_gpu, 1e3), "pil_path_ms_wall": spread(t_pil, 1e3),
        "gpu_over_pil": round(statistics.median(t_gpu) / statistics.median(t_pil), 4),
        "gpu_files_KB_per_frame": round(sum(map(len, files)) / len(files) / 1e3, 1),
        "pil_files_KB_per_frame": round(sum(map(len, pil)) / len(pil) / 1e3, 1),
    }), flush=True)
    del x
