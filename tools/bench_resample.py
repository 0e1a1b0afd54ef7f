#!/usr/bin/env python3
"""Frame preprocessing (resample.hip, sola_amd/frames.py) against the host PIL path it replaces, in one process.

Kernel cases: T = 16 and 64 frames of 720x1280 and 1080x1920 uint8 RGB -> float32 [T,3,1024,1024], bicubic with the SAM2 table
(what init_state does per frame), and one 1080x1920 frame -> 750x1333 bilinear with the ToTensor / Normalize table
(GroundingDINO's transform).  Per case one JSON object: the HIP-event median (min, max) of one ``frames.preprocess`` call after
warm-up, the bytes the algorithm needs (source read once + output written once) over that time as a fraction of 6.3 TB/s, and
the host recipe's wall time per frame on the same pixels.  One frame of every case is compared with PIL + the host recipe.

Video case: 32 JPEG frames of 1080x1920 written to a temporary directory; the wall time of one ``frames.load_video_frames`` call
(decode in reader threads, upload, preprocess) against SAM2's host recipe on the same files (PIL decode, convert, resize,
/ 255, - mean, / std), and the host recipe's share that is the resize alone."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sola_amd import frames  # noqa: E402

HBM = 6.3e12
MEAN, STD = frames.SAM2_MEAN, frames.SAM2_STD
if not torch.cuda.is_available():
    sys.exit("bench_resample.py needs a GPU")
dev = torch.device("cuda")


def natural(T, H, W, seed):
    """Smooth colour fields with noise on top: closer to video frames than white noise is (the arithmetic does not care)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        for c in range(3):
            f = 127 + 90 * np.sin(x / (40 + 9 * c) + t) * np.cos(y / (55 + 7 * c) - 0.3 * t)
            out[t, :, :, c] = np.clip(f + rng.normal(0, 12, size=(H, W)), 0, 255).astype(np.uint8)
    return out


def spread(ts, scale):
    return {"median": round(statistics.median(ts) * scale, 2), "min": round(min(ts) * scale, 2), "max": round(max(ts) * scale, 2)}


def host_frame(img, size, filt, recipe):
    """One frame through the host recipe -> float32 [3,h,w]."""
    h, w = size
    m = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    resized = np.array(Image.fromarray(img, "RGB").resize((w, h), Image.BICUBIC if filt == "bicubic" else Image.BILINEAR))
    if recipe == "sam2_video":
        out = torch.zeros(3, h, w, dtype=torch.float32)
        out[:] = torch.from_numpy(resized / 255.0).permute(2, 0, 1)
        out -= m
        out /= s
        return out
    return torch.from_numpy(resized).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(m).div_(s)


def kernel_case(name, T, H, W, size, filt, recipe, reps=20):
    tile = natural(min(T, 4), H, W, H + T)
    src = torch.from_numpy(tile).to(dev).repeat((T + len(tile) - 1) // len(tile), 1, 1, 1)[:T].contiguous()
    table = frames.normalise_table(MEAN, STD, recipe).to(dev)
    out = torch.empty((T, 3) + size, dtype=torch.float32, device=dev)
    for _ in range(3):
        frames.preprocess(src, size, filt, table, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = host_frame(tile[1 % len(tile)], size, filt, recipe)
    host_s = time.perf_counter() - t0
    assert torch.equal(out[1 % len(tile)].cpu(), want), name
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        frames.preprocess(src, size, filt, table, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    nbytes = src.numel() + out.numel() * 4
    med = statistics.median(ts)
    print(json.dumps({"workload": name, "frames": T, "MB_read": round(src.numel() / 1e6, 1), "MB_written": round(out.numel() * 4 / 1e6, 1),
                      "preprocess_call_us": spread(ts, 1e6), "us_per_frame": round(med / T * 1e6, 2),
                      "frac_of_6.3TBps": round(nbytes / med / HBM, 4), "host_recipe_ms_per_frame_one_run": round(host_s * 1e3, 1)}), flush=True)


def sam2_host(video_path, image_size):
    names = sorted((p for p in os.listdir(video_path) if p.endswith(".jpg")), key=lambda p: int(os.path.splitext(p)[0]))
    images = torch.zeros(len(names), 3, image_size, image_size, dtype=torch.float32)
    t_resize = 0.0
    for n, name in enumerate(names):
        rgb = Image.open(os.path.join(video_path, name)).convert("RGB")
        t0 = time.perf_counter()
        small = rgb.resize((image_size, image_size))
        t_resize += time.perf_counter() - t0
        images[n] = torch.from_numpy(np.array(small) / 255.0).permute(2, 0, 1)
    images -= torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    images /= torch.tensor(STD, dtype=torch.float32)[:, None, None]
    return images, t_resize


def video_case(T=32, H=1080, W=1920, S=1024):
    with tempfile.TemporaryDirectory() as d:
        for t, f in enumerate(natural(T, H, W, 5)):
            Image.fromarray(f, "RGB").save(os.path.join(d, f"{t}.jpg"), quality=90)
        frames.load_video_frames(d, S, False, compute_device=dev)  # warm-up: tables, pinned buffers' first touch
        gpu_t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images, _, _ = frames.load_video_frames(d, S, False, compute_device=dev)
            torch.cuda.synchronize()
            gpu_t.append(time.perf_counter() - t0)
        host_t, resize_t = [], []
        for _ in range(2):
            t0 = time.perf_counter()
            want, t_resize = sam2_host(d, S)
            want = want.to(dev)
            torch.cuda.synchronize()
            host_t.append(time.perf_counter() - t0)
            resize_t.append(t_resize)
        assert torch.equal(images, want)
        print(json.dumps({"workload": f"load_video_frames T={T} {H}x{W} jpg -> {S}x{S}", "reader_threads": frames.READER_THREADS,
                          "chunk_frames": frames.CHUNK_FRAMES, "load_video_frames_ms_wall": spread(gpu_t, 1e3),
                          "host_recipe_ms_wall": spread(host_t, 1e3), "host_resize_alone_ms": spread(resize_t, 1e3),
                          "gpu_over_host": round(statistics.median(gpu_t) / statistics.median(host_t), 4),
                          "equal_to_host_recipe": True}), flush=True)


for H, W in ((720, 1280), (1080, 1920)):
    for T in (16, 64):
        kernel_case(f"sam2 bicubic T={T} {H}x{W} -> 1024x1024", T, H, W, (1024, 1024), "bicubic", "sam2_video")
kernel_case("gdino bilinear T=1 1080x1920 -> 750x1333", 1, 1080, 1920, (750, 1333), "bilinear", "to_tensor", reps=50)
video_case()
