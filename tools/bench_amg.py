#!/usr/bin/env python3
"""The grid-prompt stage (amg.hip, seg_utils' last section) against what a ROCm user has without it, on the same tensors in
the same process.  Medians (and min-max) after warm-up; HIP events for stream work, wall time for calls.  One JSON object
per case.
  stats   n = 192 float32 logit maps at 720p and 1080p: sola_mask_logit_stats on the stream (memset + the counting kernel + the
          one-thread-per-map finish) between two events, its bytes (4 per pixel, read once) over that time as a fraction of
          6.3 TB/s, and the stock-torch statement of the same seven numbers: two thresholded sums, the threshold, the max / min
          box.  The two tables are compared.
  nms     n = 300, 1000, 3072 clustered boxes: the two launches of sola_box_nms_profile, the seg_utils.nms call (sort, two
          launches, one host read), and the numpy double loop on the host, copy included.
  parts   100 and 300 masks of 1080p: seg_utils.filter_part_masks against the loop of one seg_utils.compute_P per surviving
          mask (the one-to-one swap)."""
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
import amg_cases as ac  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

HBM = 6.3e12
if not torch.cuda.is_available():
    sys.exit("bench_amg.py needs a GPU")
L = _lib.lib()
dev = torch.device("cuda")


def spread(ts, scale):
    return {"median": round(statistics.median(ts) * scale, 2), "min": round(min(ts) * scale, 2), "max": round(max(ts) * scale, 2)}


def timed(fn, reps, warm=2):
    """(event seconds, wall seconds) per call of fn, each call followed by a device synchronise."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    s, ts, wall = torch.cuda.current_stream(), [], []
    for r in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record(s)
        fn()
        ev[1].record(s)
        torch.cuda.synchronize()
        if r >= warm:
            wall.append(time.perf_counter() - t0)
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return ts, wall


def torch_stats(x, thr, off):
    """The seven numbers the way SAM2's generator gets them from stock torch (calculate_stability_score's two sums, the
    threshold, batched_mask_to_box's max / min over both axes)."""
    hi = (x > (thr + off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    lo = (x > (thr - off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    m = x > thr
    h, w = m.shape[-2:]
    in_h, _ = torch.max(m, dim=-1)
    hc = in_h * torch.arange(h, device=x.device)[None, :]
    bottom, _ = torch.max(hc, dim=-1)
    top, _ = torch.min(hc + h * (~in_h), dim=-1)
    in_w, _ = torch.max(m, dim=-2)
    wc = in_w * torch.arange(w, device=x.device)[None, :]
    right, _ = torch.max(wc, dim=-1)
    left, _ = torch.min(wc + w * (~in_w), dim=-1)
    empty = (right < left) | (bottom < top)
    box = torch.stack([left, top, right, bottom], dim=-1) * (~empty).unsqueeze(-1)
    return torch.cat([hi[:, None].long(), lo[:, None].long(), m.flatten(1).sum(1)[:, None], box], 1)


def bench_stats(n, h, w):
    g = torch.Generator(device="cuda").manual_seed(h)
    yy = torch.arange(h, device=dev)[None, :, None]
    xx = torch.arange(w, device=dev)[None, None, :]
    c = torch.rand((n, 4), device=dev, generator=g)
    d = ((yy - c[:, 0, None, None] * h) / (0.05 * h + c[:, 2, None, None] * 0.3 * h)) ** 2 + \
        ((xx - c[:, 1, None, None] * w) / (0.05 * w + c[:, 3, None, None] * 0.3 * w)) ** 2
    x = ((1.0 - d) * 4.0).clamp_(-8, 8).float().contiguous()  # soft blobs: logits fall through +1, 0, -1 at the rim
    del d
    stats = torch.empty((n, 7), device=dev, dtype=torch.int64)
    stream = _lib.current_stream()

    def call():
        _lib.check(L.sola_mask_logit_stats(_lib.ptr(x), 2, n, h, w, 0.0, 1.0, -1.0, _lib.ptr(stats), stream), "sola_mask_logit_stats")

    t_lib, _ = timed(call, 20)
    want = torch_stats(x, 0.0, 1.0)
    assert torch.equal(stats, want), "the library's table differs from the torch statement"
    t_torch, _ = timed(lambda: torch_stats(x, 0.0, 1.0), 5)
    _, w_py = timed(lambda: seg_utils.mask_logit_stats(x), 20)
    nbytes = x.numel() * 4
    return {"workload": f"stats: {n} float32 logit maps {h}x{w}", "logits_MB": round(nbytes / 1e6, 1),
            "lib_stream_us_events": spread(t_lib, 1e6), "lib_frac_of_6.3TBps": round(nbytes / statistics.median(t_lib) / HBM, 4),
            "mask_logit_stats_call_us_wall": spread(w_py, 1e6), "torch_seven_numbers_us_events": spread(t_torch, 1e6),
            "torch_over_lib": round(statistics.median(t_torch) / statistics.median(t_lib), 2)}


def bench_nms(n):
    boxes = ac.float_boxes(n, n)
    scores = ac.tied_scores(n, n)
    b, s = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    order = torch.sort(s, descending=True, stable=True).indices.contiguous()
    nb = L.sola_box_nms_scratch_bytes(n)
    scratch = torch.empty(nb // 8, device=dev, dtype=torch.int64)
    out = torch.empty(n + 1, device=dev, dtype=torch.int64)
    us = (ctypes.c_float * 2)()
    rows = []
    for r in range(12):
        _lib.check(L.sola_box_nms_profile(_lib.ptr(b), _lib.ptr(order), None, n, 0.7, _lib.ptr(out[1:]), _lib.ptr(out), _lib.ptr(scratch), nb,
                                          _lib.current_stream(), us), "sola_box_nms_profile")
        if r >= 2:
            rows.append((us[0] * 1e-6, us[1] * 1e-6))
    t_call, w_call = timed(lambda: seg_utils.nms(b, s, 0.7), 10)
    got = seg_utils.nms(b, s, 0.7).cpu().tolist()

    def host():
        return ac.box_nms(b.cpu().numpy(), s.cpu().numpy(), None, 0.7)

    assert got == host(), "the library's keep list differs from the numpy loop"
    _, w_host = timed(host, 3, warm=1)
    return {"workload": f"nms: {n} boxes, threshold 0.7", "kept": len(got), "matrix_launch_us": spread([r[0] for r in rows], 1e6),
            "resolve_launch_us": spread([r[1] for r in rows], 1e6), "nms_call_us_events": spread(t_call, 1e6),
            "nms_call_us_wall": spread(w_call, 1e6), "d2h_numpy_loop_us_wall": spread(w_host, 1e6),
            "numpy_over_lib": round(statistics.median(w_host) / statistics.median(w_call), 2)}


def bench_parts(n, h, w):
    masks = torch.from_numpy(ac.part_masks(n, h, w, n)).to(dev).float()  # float32 {0,1}, as generate_prompts_grid.py stacks them

    def loop():
        is_part = torch.tensor([False] * n)
        for idx in range(n - 1):
            if is_part[idx]:
                continue
            P = seg_utils.compute_P(masks, masks[idx])
            is_part[(P > 0.7).cpu()] = True
            is_part[idx] = False
        return is_part

    want = loop()
    got = seg_utils.filter_part_masks(masks)
    assert torch.equal(got, want), "filter_part_masks differs from the compute_P loop"
    _, w_new = timed(lambda: seg_utils.filter_part_masks(masks), 5, warm=1)
    _, w_old = timed(loop, 3, warm=1)
    return {"workload": f"parts: {n} masks {h}x{w}", "parts": int(got.sum()), "full_masks_visited": int(n - 1 - got[:n - 1].sum()),
            "filter_part_masks_ms_wall": spread(w_new, 1e3), "compute_P_loop_ms_wall": spread(w_old, 1e3),
            "loop_over_filter": round(statistics.median(w_old) / statistics.median(w_new), 2)}


for args in ((192, 720, 1280), (192, 1080, 1920)):
    print(json.dumps(bench_stats(*args)), flush=True)
    torch.cuda.empty_cache()
for n in (300, 1000, 3072):
    print(json.dumps(bench_nms(n)), flush=True)
for n in (100, 300):
    print(json.dumps(bench_parts(n, 1080, 1920)), flush=True)
    torch.cuda.empty_cache()
