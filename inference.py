#!/usr/bin/env python3
"""Inference entry point with the reference's CLI / layout (inference.py of cvlab-kaist/SOLA):

    python inference.py --config mevis/default --eval_weight_epoch K [--eval_pred_threshold 0.5] [--synthetic true]
                        [--ragged_max_samples 128] [--ragged_max_rows 1048576] [--gpu_png true] [--sweep_thresholds 0.3,0.5,0.7]

Loads ``<output_dir>/<exp_name>/<train.data_name>/epoch_K.pth`` (a reference checkpoint loads unchanged: same 84
state_dict keys) and scores the test split.  The reference scores ONE (video, expression) per forward (inference.py:44-58,
batch_size 1): here up to ``ragged_max_samples`` samples of different (N, T, L) go through sola_forward_ragged in one pass,
and the expressions of one video share the text-independent half of the network (encoder + layer 0's inter-object and
motion sub-blocks).  sola_select applies the threshold (inference.py:59-60); the selected tracks' masklets are RLE-decoded
and OR-merged on the GPU and written as ``<test_output_dir>/.../<video>/<expression>/<frame>.png``.
``--gpu_png true`` writes the same files from the GPU: the merged masklet stays on the device, sola_png_deflate_* turns it
into the frames' zlib streams (seg_utils.encode_png_masklet) and the host only adds the PNG chunk framing and writes the
files - no ``[T,h,w]`` host copy, no PIL.  Same paths and pixels; the files are larger (fixed Huffman table).  The default
is the PIL writer.  With the flag a batch's samples are collected per video and written through
seg_utils.encode_png_selections: the tracks some expression of the video selects are parsed and decoded once, and no
``[T,h,w]`` masklet is formed (the PNG encoder ORs a selection's bit planes as it reads them).
``--sweep_thresholds 0.3,0.5,0.7`` (a comma list, or one value; each in [0, 1]; implies the GPU writer) writes the files of every
listed threshold from the same forward and the same decode: each gets a sibling directory of the run's own,
``pred_threshold_<t>/epoch_K/<video>/<expression>/<frame>.png`` (named by load_configs' rule, 0.25 -> ``025``), holding the OR of
the tracks with float32 prob > float32 t (seg_utils.encode_png_sweep).  The run's own ``--eval_pred_threshold`` directory is
written as without the flag, once if its threshold is also in the list.  Synthetic tracks have no masklets: every threshold's
directory gets the ``<eid>_pred.npy`` decision vectors instead.
With several GPUs (torchrun) every rank takes a contiguous block of the samples; no collective is involved.
"""
import os
import time

import numpy as np
import torch

from sola_amd import dist as sdist
from sola_amd import ops
from sola_amd.config import load_configs, parse_sweep_thresholds, sweep_dir_name
from sola_amd.data import DevicePrefetcher, make_ragged_batches
from sola_amd.module import LanguageAlignedTrackSelectionModule
from sola_amd.text import TextEncoder


def save_masklet(dataset, vid, eid, pred, frames, out_dir, device, gpu_png=False):
    """Write ``<out_dir>/<vid>/<eid>/<frame>.png`` for the OR of the selected tracks (RLE decode + OR on the GPU).  PIL
    encodes a host copy of the masklet frame by frame; with ``gpu_png`` the masklet stays on the device and the files come
    from seg_utils.encode_png_masklet."""
    masklet = dataset.merged_masklet(vid, eid, pred, device=device)
    os.makedirs(os.path.join(out_dir, vid, eid), exist_ok=True)
    if gpu_png:
        from sola_amd import seg_utils

        for frame_id, png in zip(frames, seg_utils.encode_png_masklet(masklet)):
            with open(os.path.join(out_dir, vid, eid, f"{frame_id}.png"), "wb") as f:
                f.write(png)
        return
    from PIL import Image

    for frame_id, mask in zip(frames, masklet.cpu().numpy()):
        Image.fromarray((np.asarray(mask) * 255).astype(np.uint8)).save(os.path.join(out_dir, vid, eid, f"{frame_id}.png"))


def _write_pngs(out_dir, vid, eid, frames, pngs):
    os.makedirs(os.path.join(out_dir, vid, eid), exist_ok=True)
    for frame_id, png in zip(frames, pngs):
        with open(os.path.join(out_dir, vid, eid, f"{frame_id}.png"), "wb") as f:
            f.write(png)


def save_video_masklets(dataset, vid, rows, out_dirs, thresholds, device, own_threshold=0.5):
    """The GPU writer for every sample of one video in a batch.  ``rows``: (expression id, frames, pred [N], prob [N]) per sample.
    ``out_dirs[0]`` is the run's own directory and gets the OR of the tracks with pred > 0 (seg_utils.encode_png_selections, the
    files of ``save_masklet(gpu_png=True)``); ``out_dirs[1 + j]`` gets the selection at ``thresholds[j]`` (encode_png_sweep; when pred
    is the sweep's rule at ``own_threshold``, as ops.select's is, the own directory is one more level of the same call).  The
    video's tracks are the same list objects for every expression (TrackDataset.track_rles), so each is parsed and decoded once per
    call."""
    from sola_amd import seg_utils
    masklets, index = [], {}

    def idx(rle_list):
        k = id(rle_list)
        if k not in index:
            index[k] = len(masklets)
            masklets.append(rle_list)
        return index[k]

    cand_sets = []
    for eid, _, pred, _ in rows:
        tracks = dataset.track_rles(vid, eid)
        if len(tracks) != len(pred):
            raise RuntimeError(f"{vid}/{eid}: {len(tracks)} track files but {len(pred)} predictions")
        cand_sets.append([idx(t) for t in tracks])
    sel = [np.flatnonzero(r[2] > 0) for r in rows]
    if thresholds and all(np.array_equal(np.flatnonzero(r[3].astype(np.float32) > np.float32(own_threshold)), j) for r, j in zip(rows, sel)):
        # ops.select's decision is the sweep's rule at the run's own threshold: the own directory is one more level of the one decode
        swept = seg_utils.encode_png_sweep(masklets, cand_sets, [r[3] for r in rows], [own_threshold] + list(thresholds), device)
        for (eid, frames, _, _), levels in zip(rows, swept):
            for out_dir, pngs in zip(out_dirs, levels):
                _write_pngs(out_dir, vid, eid, frames, pngs)
        return
    own = seg_utils.encode_png_selections(masklets, [[c[j] for j in js] for c, js in zip(cand_sets, sel)], device)
    for (eid, frames, _, _), pngs in zip(rows, own):
        _write_pngs(out_dirs[0], vid, eid, frames, pngs)
    if thresholds:
        swept = seg_utils.encode_png_sweep(masklets, cand_sets, [r[3] for r in rows], thresholds, device)
        for (eid, frames, _, _), levels in zip(rows, swept):
            for out_dir, pngs in zip(out_dirs[1:], levels):
                _write_pngs(out_dir, vid, eid, frames, pngs)


@torch.no_grad()
def inference(cfg):
    try:
        sweep = parse_sweep_thresholds(cfg.get("sweep_thresholds"))
    except ValueError as e:
        raise SystemExit(f"inference.py: {e}")
    rank, local_rank, world = sdist.init_from_env()
    device = torch.device("cuda", local_rank % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    module = LanguageAlignedTrackSelectionModule(cfg["model"])
    module.load_state_dict(torch.load(cfg["eval"]["weight_path"], map_location="cpu", weights_only=True))
    module = module.to(device).eval()
    text = TextEncoder(cfg["model"]["roberta_version"], cfg["model"]["lang_token_dim"], device,
                       allow_standin=bool(cfg.get("synthetic", False)))
    batches, dataset = make_ragged_batches(cfg["dataset"], "test", rank, world, cfg.get("synthetic", None), cfg["model"])
    thr = cfg["eval"]["pred_threshold"]
    out_dir = cfg["results"]["test_output_dir"]
    gpu_png = bool(cfg.get("gpu_png", False)) or sweep is not None
    # the listed thresholds' sibling directories <...>/pred_threshold_<t>/epoch_K; one that names the run's own is written once, as the
    # run's own
    sweep_dirs = []
    for t in sweep or []:
        d = os.path.join(os.path.dirname(os.path.dirname(out_dir)), f"pred_threshold_{sweep_dir_name(t)}", os.path.basename(out_dir))
        if os.path.normpath(d) != os.path.normpath(out_dir) and all(d != x for _, x in sweep_dirs):
            sweep_dirs.append((t, d))
    sweep_t = [t for t, _ in sweep_dirs]
    out_dirs = [out_dir] + [d for _, d in sweep_dirs]
    n_selected = n_tracks = n_samples = n_videos = n_calls = 0
    t_score = 0.0
    t_wall0 = time.perf_counter()
    for batch in DevicePrefetcher(batches, device):  # the next batch's tokens are copied to the GPU while this one is scored
        t0 = time.perf_counter()
        videos = batch["videos"]
        texts, _pos = text.encode_ragged([s["expression"] for s in batch["samples"]])
        module.forward_ragged(videos, texts, batch["sample_video"])
        flat, _tok, _offs, counts = module.last_ragged
        prob, pred = ops.select(flat, thr)  # inference.py:59-60
        pred = pred.cpu().numpy()
        prob = prob.cpu().numpy() if sweep_t else None
        t_score += time.perf_counter() - t0
        n_calls += 1
        n_videos += len(videos)
        o = 0
        by_video = {}  # the GPU writer takes a video's samples together: one parse and one decode of its tracks
        for smp, n in zip(batch["samples"], counts):
            p = pred[o:o + n]
            q = prob[o:o + n] if sweep_t else None
            o += n
            vid, eid = smp["video_id"], smp["expression_id"]
            n_selected += int(p.sum())
            n_tracks += n
            n_samples += 1
            if hasattr(dataset, "merged_masklet"):
                if gpu_png:
                    by_video.setdefault(vid, []).append((eid, smp["frames"], p, q))
                else:
                    save_masklet(dataset, vid, eid, p, smp["frames"], out_dir, device, gpu_png)
            else:  # synthetic tracks have no masklets: keep the decision vector, at every threshold
                os.makedirs(os.path.join(out_dir, vid), exist_ok=True)
                np.save(os.path.join(out_dir, vid, f"{eid}_pred.npy"), p)
                for t, d in sweep_dirs:
                    os.makedirs(os.path.join(d, vid), exist_ok=True)
                    np.save(os.path.join(d, vid, f"{eid}_pred.npy"), (q.astype(np.float32) > np.float32(t)).astype(p.dtype))
        for vid, rows in by_video.items():
            save_video_masklets(dataset, vid, rows, out_dirs, sweep_t, device, thr)
    rate = n_samples / t_score if t_score > 0 else 0.0
    wall = n_samples / max(time.perf_counter() - t_wall0, 1e-9)
    print(f"[rank {rank}] selected {n_selected} of {n_tracks} tracks over {n_samples} samples / {n_videos} video passes in {n_calls} "
          f"ragged calls ({rate:.1f} samples/s scoring incl. text encoding and the decision copy, token upload prefetched; "
          f"{wall:.1f} samples/s wall incl. dataset reads and output files; text encoder: {text.kind}; "
          f"PNG writer: {'GPU deflate' if gpu_png else 'PIL'}); outputs in {out_dir}" +
          (f"; sweep thresholds {sweep_t} in {[d for _, d in sweep_dirs]}" if sweep_dirs else ""))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    inference(load_configs("inference"))
