"""Mask-level J&F on the GPU: the column-major RLE decode (sola_rle_pack_cm), the select / OR / count launch
(sola_mask_select_counts), compute_JF_batch against the CPU oracle, and eval.py end to end on a MeViS-layout tree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import jf_cases as jc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

pytestmark = pytest.mark.gpu


def cm_planes(masks, stride):
    """uint8 [n,h,w] -> uint32 [n, stride]: column-major bit planes (bit j of word i = position 32*i + j), zero padded."""
    n = masks.shape[0]
    flat = np.zeros((n, stride * 32), np.uint8)
    flat[:, :masks.shape[1] * masks.shape[2]] = (np.asarray(masks) != 0).transpose(0, 2, 1).reshape(n, -1)
    return np.packbits(flat, axis=1, bitorder="little").view("<u4")


def pack_cm(cum, off, n, h, w):
    dev = torch.device("cuda")
    stride = _lib.lib().sola_jf_plane_words(h, w)
    cum_t = torch.from_numpy(np.ascontiguousarray(cum if len(cum) else np.zeros(1, np.uint32)).view(np.int32)).to(dev)
    off_t = torch.from_numpy(np.asarray(off, np.int64)).to(dev)
    bits = torch.full((n, stride), -1, device=dev, dtype=torch.int32)  # every word must be written, pad words as zeros
    _lib.check(_lib.lib().sola_rle_pack_cm(_lib.ptr(cum_t), _lib.ptr(off_t), n, h, w, stride, _lib.ptr(bits), _lib.current_stream()),
               "sola_rle_pack_cm")
    return bits.cpu().numpy().view(np.uint32), cum_t, off_t, stride


def fill_or(cum_t, off_t, n, h, w):
    out = torch.empty((n, h, w), device="cuda", dtype=torch.uint8)
    _lib.check(_lib.lib().sola_rle_fill_or(_lib.ptr(cum_t), _lib.ptr(off_t), n, 1, h, w, _lib.ptr(out), None, None,
                                           _lib.current_stream()), "sola_rle_fill_or")
    return out.cpu().numpy()


def frame_cases(h, w, rng):
    """(rle dicts or None, the oracle's decode) covering full / empty / noisy masks, an empty first run, zero-length runs,
    absent frames, compressed and uncompressed counts."""
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8)]
    masks += list(mc.blob_masklet(4, h, w, int(rng.integers(1 << 30))))
    m = (rng.random((h, w)) < 0.3).astype(np.uint8)
    m[0, 0] = 1  # position 0 set: the first (zero) run is empty
    masks.append(m)
    rles, want = [], []
    for i, m in enumerate(masks):
        c = mo.mask_to_counts(m)
        rles.append({"size": [h, w], "counts": mo.rle_counts_to_string(c) if i % 2 else c})
        want.append(m)
        if len(c) > 2:  # zero-length runs spliced in: the same mask
            z = c[:1] + [0, 0] + c[1:2] + [0, 0] + c[2:]
            rles.append({"size": [h, w], "counts": z if i % 2 else mo.rle_counts_to_string(z)})
            want.append(m)
    rles.append(None)  # absent frame
    want.append(np.zeros((h, w), np.uint8))
    return rles, np.stack(want)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (29, 1), (23, 37), (32, 4), (17, 33), (90, 160)])
def test_rle_pack_cm_matches_the_oracle_and_rle_fill_or(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    rles, want = frame_cases(h, w, rng)
    cum, off = seg_utils._planes_cum([rles], [0], len(rles), h * w)
    n = len(rles)
    got, cum_t, off_t, stride = pack_cm(cum, off, n, h, w)
    for r, m in zip(rles, want):
        if r is not None:
            np.testing.assert_array_equal(mo.rle_decode(r), m)
    np.testing.assert_array_equal(got, cm_planes(want, stride))  # pad words included: zero
    np.testing.assert_array_equal(got, cm_planes(fill_or(cum_t, off_t, n, h, w), stride))


def test_short_runs_follow_rle_fill_or():
    """Runs covering fewer than h*w pixels: the value after the last run is the parity of the runs, as rle_fill_or_kernel."""
    h, w = 5, 9
    rles = [{"size": [h, w], "counts": c} for c in ([3], [3, 4], [0, 7, 2], [], [10, 0, 3])]
    cum, off = seg_utils._planes_cum([rles], [0], len(rles), h * w)
    got, cum_t, off_t, stride = pack_cm(cum, off, len(rles), h, w)
    ref = fill_or(cum_t, off_t, len(rles), h, w)
    np.testing.assert_array_equal(got, cm_planes(ref, stride))
    assert ref[0].T.reshape(-1)[3:].all() and not ref[1].T.reshape(-1)[7:].any()


def test_rle_pack_cm_more_than_65535_planes():
    h, w, n = 1, 3, 70000
    rng = np.random.default_rng(7)
    masks = (rng.random((n, h, w)) < 0.5).astype(np.uint8)
    strings = [mo.rle_counts_to_string(mo.mask_to_counts(m)) for m in masks]
    cum, off = seg_utils.rle_strings_to_cum(strings, h * w)
    got, _, _, stride = pack_cm(cum, off, n, h, w)
    np.testing.assert_array_equal(got, cm_planes(masks, stride))


def select_counts(bits, stride, M, T, pred_sets, gt_sets):
    dev = torch.device("cuda")
    def csr(sets):
        off, idx = [0], []
        for s in sets:
            idx += list(s)
            off.append(len(idx))
        return torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(idx + [0], dtype=torch.int32, device=dev)
    (po, pi), (go, gi) = csr(pred_sets), csr(gt_sets)
    E = len(pred_sets)
    counts = torch.empty((E, T, 3), device=dev, dtype=torch.int64)
    _lib.check(_lib.lib().sola_mask_select_counts(_lib.ptr(bits), stride, M, T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(go), _lib.ptr(gi),
                                                  E, _lib.ptr(counts), _lib.current_stream()), "sola_mask_select_counts")
    return counts.cpu().numpy()


def numpy_counts(planes, T, pred_sets, gt_sets):
    M = planes.shape[0] // T
    pl = planes.reshape(M, T, -1)
    out = np.zeros((len(pred_sets), T, 3), np.int64)
    for e, (ps, gs) in enumerate(zip(pred_sets, gt_sets)):
        p = np.bitwise_or.reduce(pl[list(ps)], axis=0) if len(ps) else np.zeros_like(pl[0])
        g = np.bitwise_or.reduce(pl[list(gs)], axis=0) if len(gs) else np.zeros_like(pl[0])
        bc = lambda a: np.unpackbits(a.view(np.uint8), axis=1).sum(1)  # noqa: E731
        out[e] = np.stack([bc(p & g), bc(p), bc(g)], 1)
    return out


@pytest.mark.parametrize("M,T,stride,E", [(9, 5, 44, 12), (40, 3, 4, 300), (3, 250, 4, 300), (3, 2, 1032, 5)])
def test_select_counts_match_numpy(M, T, stride, E):
    rng = np.random.default_rng(M * 31 + E)
    planes = rng.integers(0, 1 << 32, size=(M * T, stride), dtype=np.uint64).astype(np.uint32)
    planes[rng.random(M * T) < 0.1] = 0
    pred_sets = [list(rng.integers(0, M, size=rng.integers(0, 6))) for _ in range(E)]
    gt_sets = [list(rng.integers(0, M, size=rng.integers(0, 4))) for _ in range(E)]
    pred_sets[0], gt_sets[1] = [], []                   # empty lists: all-zero masks
    pred_sets[2], gt_sets[2] = [1, 1, M - 1], [M - 1, 1]  # duplicates, the same masks in both lists
    pred_sets[3], gt_sets[3] = [], []
    bits = torch.from_numpy(planes.view(np.int32)).cuda()
    got = select_counts(bits, stride, M, T, pred_sets, gt_sets)  # (3, 250, 4, 300): E*T = 75000 blocks; 1032 words: 258 quads, lanes 0 and 1 loop twice
    np.testing.assert_array_equal(got, numpy_counts(planes, T, pred_sets, gt_sets))


def test_select_counts_skip_indices_outside_the_masks():
    """A list entry >= n_masks is skipped: the counts are those of the lists without it."""
    M, T, stride = 4, 3, 12
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 1 << 32, size=(M * T, stride), dtype=np.uint64).astype(np.uint32)
    pred_sets = [[0, M, 2], [M + 7], [M, 1, M], [3]]
    gt_sets = [[1], [2, M], [M], [M + 1, 3, 0]]
    inside = lambda sets: [[i for i in s if i < M] for s in sets]  # noqa: E731
    got = select_counts(torch.from_numpy(planes.view(np.int32)).cuda(), stride, M, T, pred_sets, gt_sets)
    np.testing.assert_array_equal(got, numpy_counts(planes, T, inside(pred_sets), inside(gt_sets)))


def oracle_jf(masklets, pred_sets, gt_sets):
    dec = [mo.masklet_decode(m) for m in masklets]
    zeros = np.zeros_like(dec[0])
    out = []
    for ps, gs in zip(pred_sets, gt_sets):
        p = np.logical_or.reduce([dec[i] for i in ps]) if ps else zeros
        g = np.logical_or.reduce([dec[i] for i in gs]) if gs else zeros
        J, F = mo.compute_J(p, g), mo.compute_F(p, g)
        out.append((J, F, (J + F) / 2))
    return out


def test_compute_JF_batch_equals_the_oracle():
    T, h, w = 7, 31, 45
    rng = np.random.default_rng(11)
    masklets = []
    for k in range(12):
        masks = mc.blob_masklet(T, h, w, 300 + k)
        if k == 5:
            masks[:] = 0
        masklets.append(jc.rle_list(masks, compressed=k != 3, missing=(k % T,) if k % 4 == 0 else ()))
    pred_sets = [sorted(set(rng.integers(0, 12, size=rng.integers(1, 5)).tolist())) for _ in range(9)]
    gt_sets = [rng.integers(0, 12, size=rng.integers(1, 3)).tolist() for _ in range(9)]
    pred_sets[0], gt_sets[1], pred_sets[2], gt_sets[2] = [], [], [], []
    pred_sets[3], gt_sets[3] = [4, 4, 6], [6]
    gt_sets[4] = [5]
    want = oracle_jf(masklets, pred_sets, gt_sets)
    got = seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda")
    assert got == want  # float ==, per expression
    assert seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", max_plane_bytes=1) == want  # one expression per group
    small = 3 * T * _lib.lib().sola_jf_plane_words(h, w) * 4
    assert seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", max_plane_bytes=small) == want
    c = seg_utils.masklet_select_counts(masklets, pred_sets, gt_sets, "cuda")
    assert c.dtype == torch.int64 and tuple(c.shape) == (9, T, 3) and not c.is_cuda
    with pytest.raises(_lib.SolaError):
        seg_utils.masklet_select_counts(masklets + [masklets[0][:-1]], [[0]], [[1]], "cuda")  # T differs
    with pytest.raises(_lib.SolaError):
        other = jc.rle_list(mc.blob_masklet(T, h + 1, w, 1))
        seg_utils.masklet_select_counts(masklets + [other], [[0]], [[1]], "cuda")  # (h, w) differs


def test_masklet_select_counts_with_no_prediction_or_no_gt_index_at_all():
    """Groups that have planes while every prediction list, or every GT list, is empty (the uploaded index list is then only
    its pad entry), one expression with both lists empty among them: the counts of the numpy restatement on the same planes."""
    T, h, w = 3, 13, 21
    masklets = [jc.rle_list(mc.blob_masklet(T, h, w, 70 + k)) for k in range(3)]
    stride = _lib.lib().sola_jf_plane_words(h, w)
    planes = cm_planes(np.concatenate([mo.masklet_decode(m) for m in masklets]), stride)
    for pred_sets, gt_sets in [([[], [], []], [[0], [], [1, 2]]), ([[0], [], [1, 2]], [[], [], []])]:
        want = numpy_counts(planes, T, pred_sets, gt_sets)
        assert want.any() and not want[1].any()
        got = seg_utils.masklet_select_counts(masklets, pred_sets, gt_sets, "cuda")
        np.testing.assert_array_equal(got.numpy(), want)
        got, bgot = seg_utils.masklet_select_counts(masklets, pred_sets, gt_sets, "cuda", boundary=True)
        np.testing.assert_array_equal(got.numpy(), want)
        assert tuple(bgot.shape) == (3, T, 4) and not bgot[1].any()  # nothing on either side: no boundary pixel


# ------------------------------------------------------------------------------------------------ eval.py end to end
def _run_eval(tmp_path, threshold, extra=()):
    env = dict(os.environ, SOLA_ALLOW_TEXT_STANDIN="1", HF_HUB_OFFLINE="1")
    env.pop("SOLA_PRECISION", None)  # the entry point's own default
    cmd = [sys.executable, os.path.join(ROOT, "eval.py"), "--config", "mevis/jf", "--eval_weight_epoch", "1",
           "--eval_pred_threshold", str(threshold), *extra]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    thr = str(threshold).replace(".", "")
    return r.stdout, os.path.join(tmp_path, "SOLA", "EVAL", "jf", "mevis", f"pred_threshold_{thr}", "epoch_1")


@pytest.fixture(scope="module")
def eval_tree(tmp_path_factory):
    from sola_amd import synth
    from sola_amd.module import LanguageAlignedTrackSelectionModule
    tmp = tmp_path_factory.mktemp("jf_eval")
    model = dict(synth.SMALL_MODEL_CFG, roberta_version="sentence-transformers/all-roberta-large-v1")
    data_root, track_root, split = jc.make_tree(str(tmp), token_dim=model["object_token_dim"])
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mevis", "default.yaml")))
    cfg.update(exp_name="jf", model=model)
    cfg["dataset"].update(data_root=data_root, track_root=track_root, valid=split)
    os.makedirs(tmp / "configs" / "mevis")
    yaml.safe_dump(cfg, open(tmp / "configs" / "mevis" / "jf.yaml", "w"))
    torch.manual_seed(0)
    wdir = tmp / "SOLA" / "TRAIN" / "jf" / "mevis"
    os.makedirs(wdir)
    torch.save(LanguageAlignedTrackSelectionModule(model).state_dict(), wdir / "epoch_1.pth")
    return tmp


def _check_layout(out, metrics):
    jf = json.load(open(os.path.join(out, "valid_u_JF_metrics_1epoch.json")))
    entries = []
    for vid, (_, exps) in jc.VIDEOS.items():
        assert list(jf[vid]) == list(exps)
        for eid, (exp, _, _) in exps.items():
            e = jf[vid][eid]
            assert set(e) == {"expression", "J", "F", "JF"} and e["expression"] == exp
            assert e["JF"] == (e["J"] + e["F"]) / 2
            entries.append(e)
    for k in ("J", "F", "JF"):
        assert metrics[f"mean_{k}"] == float(np.mean([e[k] for e in entries]))
    return jf


def _gt(vid, eid):
    annos = jc.VIDEOS[vid][1][eid][1]
    g = np.logical_or.reduce([jc.gt_masks(a) for a in annos])
    if 3 in annos and len(annos) == 1:
        g[4] = 0  # object 3's frame 4 is missing in mask_dict.json
    elif 3 in annos:
        g[4] = jc.gt_masks(7)[4]
    return g


def test_eval_writes_jf_metrics_nothing_selected(eval_tree):
    stdout, out = _run_eval(eval_tree, 1.0)
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    assert m["tp"] + m["fp"] == 0
    jf = _check_layout(out, m)
    for vid, (_, exps) in jc.VIDEOS.items():
        for eid in exps:
            g = _gt(vid, eid)
            assert jf[vid][eid]["J"] == float(np.mean([1.0 if not f.any() else 0.0 for f in g]))
            assert jf[vid][eid]["F"] == 0.0
    assert '"mean_JF"' in stdout.strip().splitlines()[-1]


def test_eval_writes_jf_metrics_everything_selected(eval_tree):
    _, out = _run_eval(eval_tree, 0.0)
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    n_tracks = sum(len(grid) + len(exps[e][2]) for grid, exps in jc.VIDEOS.values() for e in exps)
    assert m["tp"] + m["fp"] == n_tracks  # sigmoid > 0 everywhere: every track selected
    jf = _check_layout(out, m)
    for vid, (grid, exps) in jc.VIDEOS.items():
        for eid, (_, _, gd) in exps.items():
            preds = np.logical_or.reduce([mo.masklet_decode(jc.rle_list(mc.blob_masklet(jc.T, jc.H, jc.W, a),
                                                                        missing=(0,) if a == 41 else ()))
                                          for a in list(grid) + list(gd)])
            g = _gt(vid, eid)
            J, F = mo.compute_J(preds, g), mo.compute_F(preds, g)
            assert (jf[vid][eid]["J"], jf[vid][eid]["F"]) == (J, F)


def test_eval_without_mask_gt_keeps_todays_outputs(eval_tree):
    keys = {"total", "bce", "alignment", "tp", "fp", "fn", "tn", "bce_evaluator_convention", "samples", "text_encoder",
            "precision", "recall"}
    stdout, out = _run_eval(eval_tree, 0.3, ("--synthetic", "true", "--synthetic_samples", "4", "--synthetic_tracks", "8",
                                             "--synthetic_frames", "8"))
    assert set(json.load(open(os.path.join(out, "track_metrics.json")))) == keys
    assert os.listdir(out) == ["track_metrics.json"]
    assert "J&F skipped" in stdout
    stdout, out = _run_eval(eval_tree, 0.4, ("--jf", "false"))
    assert set(json.load(open(os.path.join(out, "track_metrics.json")))) == keys
    assert os.listdir(out) == ["track_metrics.json"] and "J&F skipped: --jf false" in stdout
