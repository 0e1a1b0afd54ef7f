"""JPEG decode on the GPU against the present route, on 32 frames of 1080p and of 720p (4:2:0, quality 90,
photographic-like content made here and encoded by Pillow).  Medians, the alternatives alternating in one process:

  * one frames.decode_jpeg call (host parse + upload of the files' scans + sola_jpeg_decode) against PIL in 8 reader threads + the
    upload of the RGB frames; the HIP-event time of each stage of sola_jpeg_decode and its number of sync rounds;
  * one frames.load_video_frames call with jpeg_decoder="pil" (the default) and "gpu" on the same files.

usage: python tools/bench_jpeg.py [--frames 32] [--reps 7] [--subseq 0 64 256] [--sizes 1080 720]
Prints one JSON line per measurement."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sola_amd import _lib, frames  # noqa: E402

STAGES = ["layout", "sync", "prefix+write", "dc_scan", "idct", "upsample+colour"]


def photo(h, w, seed):
    """Smooth shading, a few edges, texture that grows towards one corner, sensor-like noise: about 0.4 MB per 1080p frame at quality 90."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        img[..., c] = 120 + 60 * np.sin(x / (90 + 20 * c) + seed) * np.cos(y / (70 + 10 * c)) + 30 * np.sin((x + 2 * y) / 23.0 + c)
    for _ in range(12):  # rectangles: hard edges
        x0, y0 = int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64))
        img[y0:y0 + int(rng.integers(32, h // 3)), x0:x0 + int(rng.integers(32, w // 3))] += rng.uniform(-50, 50, size=3)
    tex = rng.normal(0, 1, size=(h, w, 1)).astype(np.float32)
    img += tex * (1.5 + 9 * (x / w * y / h))[..., None]
    return np.clip(img, 0, 255).astype(np.uint8)


def make_files(n, h, w):
    out = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(photo(h, w, i)).save(buf, "JPEG", quality=90, subsampling="4:2:0")
        out.append(buf.getvalue())
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pil_route(datas, pinned, pool, dev):
    def one(j):
        with Image.open(io.BytesIO(datas[j])) as im:
            pinned[j].numpy()[...] = np.asarray(im.convert("RGB"))
    list(pool.map(one, range(len(datas))))
    return pinned.to(dev, non_blocking=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--subseq", type=int, nargs="*", default=[0])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1080, 720])
    ap.add_argument("--no-video", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    for h in args.sizes:
        w = h * 16 // 9
        datas = make_files(args.frames, h, w)
        parsed = [frames.jpeg_parse(d) for d in datas]
        scan = sum(p.scan_end - p.scan_begin for p, _ in parsed)
        base = {"frames": args.frames, "size": f"{w}x{h}", "file_mb": round(sum(map(len, datas)) / 1e6, 2), "scan_mb": round(scan / 1e6, 2)}
        pinned = torch.empty((args.frames, h, w, 3), dtype=torch.uint8, pin_memory=True)
        with ThreadPoolExecutor(max_workers=frames.READER_THREADS) as pool:
            want = pil_route(datas, pinned, pool, dev).clone()
            for s in args.subseq:
                got = frames.decode_jpeg(datas, subseq_bytes=s)  # warm-up, and the check that the bench measures the right bytes
                assert torch.equal(got, want), "decode_jpeg differs from Pillow"
            t_pil, t_gpu = [], {s: [] for s in args.subseq}
            t_parse, t_stage, rounds = [], {s: [] for s in args.subseq}, {}
            for _ in range(args.reps):
                t_pil.append(timed(lambda: pil_route(datas, pinned, pool, dev)))
                for s in args.subseq:
                    t_gpu[s].append(timed(lambda: frames.decode_jpeg(datas, subseq_bytes=s)))
                t0 = time.perf_counter()
                [frames.jpeg_parse(d) for d in datas]
                t_parse.append((time.perf_counter() - t0) * 1e3)
                for s in args.subseq:  # the stages of the device call, on their own: events at every stage boundary
                    ms = (C.c_float * 6)()
                    L.sola_jpeg_profile(ms)
                    _, _, rounds[s] = frames._jpeg_decode_chunk(parsed, datas, dev, s)
                    L.sola_jpeg_profile(None)
                    t_stage[s].append(list(ms))
        print(json.dumps({**base, "what": "PIL in 8 threads + upload of RGB", "ms": round(statistics.median(t_pil), 2)}), flush=True)
        print(json.dumps({**base, "what": "host parse alone (one thread)", "ms": round(statistics.median(t_parse), 2)}), flush=True)
        for s in args.subseq:
            st = np.median(np.array(t_stage[s]), axis=0)
            print(json.dumps({**base, "what": "decode_jpeg", "subseq_bytes": s or frames.JPEG_SUBSEQ_DEFAULT, "ms": round(statistics.median(t_gpu[s]), 2),
                              "sync_rounds": rounds[s], "stage_ms": {k: round(float(v), 3) for k, v in zip(STAGES, st)},
                              "device_ms": round(float(st.sum()), 3)}), flush=True)
        if args.no_video:
            continue
        with tempfile.TemporaryDirectory() as d:
            for i, data in enumerate(datas):
                with open(os.path.join(d, f"{i}.jpg"), "wb") as f:
                    f.write(data)
            a, _, _ = frames.load_video_frames(d, 1024, False)
            b, _, _ = frames.load_video_frames(d, 1024, False, jpeg_decoder="gpu")
            assert torch.equal(a, b), "load_video_frames: the two modes differ"
            t = {"pil": [], "gpu": []}
            for _ in range(args.reps):
                for mode in ("pil", "gpu"):
                    t[mode].append(timed(lambda: frames.load_video_frames(d, 1024, False, jpeg_decoder=mode)))
            for mode in ("pil", "gpu"):
                print(json.dumps({**base, "what": f'load_video_frames(jpeg_decoder="{mode}") -> 1024x1024', "ms": round(statistics.median(t[mode]), 2)}), flush=True)


if __name__ == "__main__":
    main()
