#!/usr/bin/env python3
"""Evaluation entry point with the reference's CLI / layout (eval.py + the loss/selection part of evaluator.py):

    python eval.py --config mevis/default --eval_weight_epoch K [--eval_pred_threshold 0.5] [--synthetic true]

Reports the losses and track-level TP/FP/FN/TN of the valid split and writes ``<eval_output_dir>/track_metrics.json``.
Scoring runs on ragged batches (sola_forward_ragged: up to ``--ragged_max_samples`` samples of different shapes per launch,
one pass of the text-independent half per video); every sample's losses are its own means, as at the reference's batch
size of 1.

Mask-level J&F (evaluator.py:174-247): each sample's selection vector comes back with one host copy per batch; a track is
selected when its prediction is > 0, as in get_sam2_masklet.  The expressions of a video are then scored by ONE
seg_utils.compute_JF_batch call: every referenced track and GT masklet decoded once on the GPU, every (expression, frame)
counted in one launch.  Writes ``<eval_output_dir>/<data_type>_JF_metrics_<K>epoch.json`` as ``{video: {exp_id: {expression,
J, F, JF}}}`` and adds ``mean_J`` / ``mean_F`` / ``mean_JF`` to track_metrics.json and the printed line; with several ranks
rank 0 gathers every rank's entries.  J is the mean over frames of inter / union (1.0 for an empty union), F the pixel F1
over the whole masklet (0.0 without a true positive) - the reference's definition; the DAVIS boundary F is behind
``--boundary_f`` below.  Counts are
exact int64 (the reference's float32 sums are exact below 2^24).  An expression without GT ids scores against an all-zero
ground truth (the reference fails there).  ``--boundary_f true`` (``--boundary_th``, default 0.008) adds the benchmark's
F: every entry gains ``F_boundary`` (mean over frames of the DAVIS contour F-measure: boundary maps of prediction and
ground truth, each matched against the other dilated by a disk of ``boundary_th`` of the image diagonal; no void pixels)
and ``JF_boundary`` = (J + F_boundary) / 2, track_metrics.json and the printed line ``mean_F_boundary`` /
``mean_JF_boundary`` / ``boundary_th``, from one more launch on the planes the J pass decoded
(sola_mask_select_boundary_counts).  J&F needs mask ground truth: MeViS with a ``mask_dict.json`` (COCO RLE), or Ref-DAVIS
with its ``Annotations/<video>/`` folders of palette PNGs, whose index maps are uploaded once per video and turned into the
same planes on the GPU (sola_index_pack; object k's ground truth is ``maps == k``, not the reference loader's, which gives
every object the last object's masks).  A video whose tracks and annotation differ in their number of frames raises a
RuntimeError naming the video and both counts.  Without ground truth (synthetic data, the MeViS ``valid`` test split,
Ref-YouTube-VOS, whose valid split has no public annotation) or with ``--jf false`` one line says why J&F was skipped and
the outputs are the loss / track metrics alone.

``--sweep_thresholds 0.1,0.3,0.5`` (a comma list, or one value; each in [0, 1]) adds the J / F / J&F curve over the selection
threshold from the same run: the tracks' probabilities come back with one more host copy per batch, and every video's
expressions are scored at all K thresholds by ONE seg_utils.compute_JF_sweep call next to the compute_JF_batch call (the
selections at descending thresholds are nested, so sola_mask_nested_counts reads each plane of the largest one once and
emits every level's counts; a track is selected when float32 prob > float32 threshold, as above).  Writes
``<eval_output_dir>/threshold_sweep.json``: ``thresholds`` (the caller's order), ``mean_J`` / ``mean_F`` / ``mean_JF`` as lists
over them (with ``--boundary_f true`` also ``mean_F_boundary`` / ``mean_JF_boundary`` and ``boundary_th``), ``best`` =
{threshold, metric, value} (``mean_JF_boundary`` with boundary F, else ``mean_JF``; the first threshold among equals) and
``expressions`` = {video: {expression id: {J: [...], F: [...], JF: [...]}}}; track_metrics.json gains
``sweep_best_threshold`` / ``sweep_best_value``.  The JF file and every other key are what they are without the flag.  When
J&F is skipped no sweep file is written.

BCE convention: ``bce`` / ``total`` follow train.py:98-113 (BCE-with-logits on the LOGITS, what the
network is trained and validated with).  The reference's evaluator applies binary_cross_entropy_with_logits to the
already SIGMOID-ed scores (evaluator.py:101,107-111) - a double sigmoid; that number is reported separately as
``bce_evaluator_convention`` so eval JSONs can be compared line by line, and never enters ``total``.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from sola_amd import dist as sdist
from sola_amd.config import load_configs, parse_sweep_thresholds
from sola_amd.data import make_ragged_batches
from sola_amd.module import LanguageAlignedTrackSelectionModule
from sola_amd.text import TextEncoder
from train import run_split_ragged


def jf_skip_reason(cfg, ds):
    """Why J&F cannot be computed for this run, or None."""
    if not cfg.get("jf", True):
        return "--jf false"
    if cfg.get("synthetic", False):
        return "synthetic tracks have no masks"
    if not getattr(ds, "has_mask_gt", False):
        return f"no mask ground truth (mask_dict.json / Annotations) for {getattr(ds, 'data_type', 'this split')}"
    return None


class SelectionCollector:
    """run_split_ragged's on_batch: keeps (video, expression id, expression, selected [N] bool) per sample."""

    def __init__(self):
        self.rows = []

    def __call__(self, batch, pred):
        sel = (pred > 0).cpu().numpy()  # one host copy per batch
        o = 0
        for s, v in zip(batch["samples"], batch["sample_video"]):
            n = int(batch["videos"][v].shape[0])
            self.rows.append((s["video_id"], s["expression_id"], s["expression"], sel[o:o + n]))
            o += n


class ProbCollector:
    """run_split_ragged's on_prob: keeps every sample's float32 track probabilities [N], in the order of SelectionCollector's rows."""

    def __init__(self):
        self.rows = []

    def __call__(self, batch, prob):
        p = prob.float().cpu().numpy()  # one host copy per batch
        o = 0
        for v in batch["sample_video"]:
            n = int(batch["videos"][v].shape[0])
            self.rows.append(p[o:o + n])
            o += n


def jf_entries(ds, rows, device, boundary=None, sweep=None):
    """[(video, expression id, {expression, J, F, JF})] in the order of ``rows``, one compute_JF_batch call per video;
    with ``boundary`` (the DAVIS bound_th) every entry also has F_boundary and JF_boundary.  ``sweep`` = (the probabilities
    of every row's tracks, thresholds) adds one compute_JF_sweep call per video on the same masklets and returns
    ``(entries, [(video, expression id, {J: [..], F: [..], JF: [..], ...})])``, each list over the thresholds."""
    from sola_amd import seg_utils
    by_video = OrderedDict()
    for j, r in enumerate(rows):
        by_video.setdefault(r[0], []).append(r if sweep is None else r + (sweep[0][j],))
    out, sweep_out = [], []
    for vid, rs in by_video.items():
        masklets, index = [], {}

        def idx(rle_list):  # shared tracks / GT objects are the same list objects: decoded once per video
            k = id(rle_list)
            if k not in index:
                index[k] = len(masklets)
                masklets.append(rle_list)
            return index[k]

        pred_sets, gt_sets, no_tracks, cand_sets = [], [], [], []
        for _, eid, _, sel in (r[:4] for r in rs):
            tracks = ds.track_rles(vid, eid)
            if len(tracks) != len(sel):
                raise RuntimeError(f"{vid}/{eid}: {len(tracks)} track files but {len(sel)} predictions")
            ids = [idx(t) for t in tracks]
            cand_sets.append(ids)
            pred_sets.append([ids[j] for j in np.flatnonzero(sel)])
            gts = ds.gt_masklets(vid, eid, device)
            for g in gts:  # (an RLE list from mask_dict.json and an annotation folder are checked alike)
                if tracks and len(tracks[0]) != len(g):
                    raise RuntimeError(f"{vid}: the tracks have {len(tracks[0])} frames but the annotation has {len(g)}")
            gt_sets.append([idx(g) for g in gts])
            no_tracks.append(not tracks)
        keys = ("J", "F", "JF") if boundary is None else ("J", "F", "JF", "F_boundary", "JF_boundary")
        scores = (seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, device, boundary=boundary) if masklets
                  else [(0.0,) * len(keys)] * len(rs))
        for (_, eid, exp, _), score, empty in zip((r[:4] for r in rs), scores, no_tracks):
            if empty:  # no track files at all: get_sam2_masklet returns None and the evaluator scores 0
                score = (0.0,) * len(keys)
            out.append((vid, eid, {"expression": exp, **dict(zip(keys, score))}))
        if sweep is not None:
            K = len(sweep[1])
            for r in rs:
                if len(r[4]) != len(r[3]):
                    raise RuntimeError(f"{vid}/{r[1]}: {len(r[3])} predictions but {len(r[4])} probabilities")
            curves = (seg_utils.compute_JF_sweep(masklets, cand_sets, [r[4] for r in rs], sweep[1], gt_sets, device, boundary=boundary)
                      if masklets else [[(0.0,) * len(keys)] * K] * len(rs))
            for r, curve, empty in zip(rs, curves, no_tracks):
                if empty:
                    curve = [(0.0,) * len(keys)] * K
                sweep_out.append((vid, r[1], {k: [score[i] for score in curve] for i, k in enumerate(keys)}))
    return out if sweep is None else (out, sweep_out)


def sweep_summary(sweep_entries, thresholds, boundary=None):
    """The contents of threshold_sweep.json from every rank's sweep entries."""
    keys = ("J", "F", "JF") if boundary is None else ("J", "F", "JF", "F_boundary", "JF_boundary")
    out = OrderedDict(thresholds=list(thresholds))
    for key in keys:
        out[f"mean_{key}"] = [float(np.mean([e[key][k] for _, _, e in sweep_entries])) if sweep_entries else 0.0
                              for k in range(len(thresholds))]
    if boundary is not None:
        out["boundary_th"] = boundary
    metric = "mean_JF" if boundary is None else "mean_JF_boundary"
    best = max(range(len(thresholds)), key=lambda k: out[metric][k])  # (max keeps the first among equals)
    out["best"] = {"threshold": thresholds[best], "metric": metric, "value": out[metric][best]}
    exps = OrderedDict()
    for vid, eid, e in sweep_entries:
        exps.setdefault(vid, OrderedDict())[eid] = e
    out["expressions"] = exps
    return out


@torch.no_grad()
def evaluate(cfg):
    try:
        thresholds = parse_sweep_thresholds(cfg.get("sweep_thresholds"))
    except ValueError as e:
        raise SystemExit(f"eval.py: {e}")
    rank, local_rank, world = sdist.init_from_env()
    device = torch.device("cuda", local_rank % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    module = LanguageAlignedTrackSelectionModule(cfg["model"])
    module.load_state_dict(torch.load(cfg["eval"]["weight_path"], map_location="cpu", weights_only=True))
    module = module.to(device).eval()
    text = TextEncoder(cfg["model"]["roberta_version"], cfg["model"]["lang_token_dim"], device,
                       allow_standin=bool(cfg.get("synthetic", False)))
    batches, ds = make_ragged_batches(cfg["dataset"], "valid", rank, world, cfg.get("synthetic", None), cfg["model"])
    tcfg = dict(cfg["train"])
    tcfg["pred_threshold"] = cfg["eval"]["pred_threshold"]
    skip = jf_skip_reason(cfg, ds)
    selections = None if skip else SelectionCollector()
    probs = ProbCollector() if thresholds is not None and not skip else None
    m = run_split_ragged(module, text, batches, tcfg, device, world, on_batch=selections, on_prob=probs)
    m["text_encoder"] = text.kind
    m["precision"] = m["tp"] / max(m["tp"] + m["fp"], 1.0)
    m["recall"] = m["tp"] / max(m["tp"] + m["fn"], 1.0)
    if selections is not None:
        boundary = float(cfg.get("boundary_th", 0.008)) if cfg.get("boundary_f", False) else None
        sweep_entries = None
        if probs is None:
            entries = jf_entries(ds, selections.rows, device, boundary)
        else:
            entries, sweep_entries = jf_entries(ds, selections.rows, device, boundary, sweep=(probs.rows, thresholds))
        if world > 1:
            gathered = [None] * world
            torch.distributed.all_gather_object(gathered, entries)
            entries = [e for part in gathered for e in part]
            if sweep_entries is not None:
                torch.distributed.all_gather_object(gathered, sweep_entries)
                sweep_entries = [e for part in gathered for e in part]
        if rank == 0:
            jf = OrderedDict()
            for vid, eid, e in entries:
                jf.setdefault(vid, OrderedDict())[eid] = e
            for key in ("J", "F", "JF") + (() if boundary is None else ("F_boundary", "JF_boundary")):
                m[f"mean_{key}"] = float(np.mean([e[key] for _, _, e in entries])) if entries else 0.0
            if boundary is not None:
                m["boundary_th"] = boundary
            name = f"{cfg['dataset']['valid']['data_type']}_JF_metrics_{cfg['eval']['weight_epoch']}epoch.json"
            with open(os.path.join(cfg["results"]["eval_output_dir"], name), "w") as f:
                json.dump(jf, f, indent=4)
            if sweep_entries is not None:
                sweep = sweep_summary(sweep_entries, thresholds, boundary)
                m["sweep_best_threshold"], m["sweep_best_value"] = sweep["best"]["threshold"], sweep["best"]["value"]
                with open(os.path.join(cfg["results"]["eval_output_dir"], "threshold_sweep.json"), "w") as f:
                    json.dump(sweep, f, indent=4)
    if rank == 0:
        if skip:
            print(f"J&F skipped: {skip}" + ("; no threshold sweep" if thresholds is not None else ""))
        print(json.dumps(m))
        with open(os.path.join(cfg["results"]["eval_output_dir"], "track_metrics.json"), "w") as f:
            json.dump(m, f, indent=2)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    evaluate(load_configs("eval"))
