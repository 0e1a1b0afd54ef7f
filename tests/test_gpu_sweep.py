"""J&F at every selection threshold from one counting pass: sola_mask_nested_counts against the numpy restatement of
tests/sweep_cases.py and against sola_mask_select_counts on the materialised prefixes, masklet_sweep_counts / compute_JF_sweep
against compute_JF_batch per threshold, and eval.py --sweep_thresholds end to end on the MeViS-layout tree of jf_cases."""
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
import sweep_cases as sc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLDS = [0.5, 0.9, 0.1, 0.5, 0.0, 1.0]  # unsorted, with a duplicate


def _csr(lists):
    off, idx = [0], []
    for s in lists:
        idx += [int(i) for i in s]
        off.append(len(idx))
    dev = torch.device("cuda")
    return torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(idx + [0], dtype=torch.int32, device=dev)


def nested_counts(bits, stride, M, T, pred_lists, level_ends, gt_sets):
    """sola_mask_nested_counts on device planes -> int64 [E, K, T, 3] on the host; the output starts as -1 everywhere."""
    (po, pi), (go, gi) = _csr(pred_lists), _csr(gt_sets)
    E, K = len(pred_lists), len(level_ends[0])
    le = torch.tensor(np.asarray(level_ends, np.int32).reshape(E, K), device="cuda")
    counts = torch.full((E, K, T, 3), -1, device="cuda", dtype=torch.int64)
    _lib.check(_lib.lib().sola_mask_nested_counts(_lib.ptr(bits), stride, M, T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(le), K, _lib.ptr(go),
                                                  _lib.ptr(gi), E, _lib.ptr(counts), _lib.current_stream()), "sola_mask_nested_counts")
    return counts.cpu().numpy()


def select_counts(bits, stride, M, T, pred_sets, gt_sets):
    (po, pi), (go, gi) = _csr(pred_sets), _csr(gt_sets)
    E = len(pred_sets)
    counts = torch.empty((E, T, 3), device="cuda", dtype=torch.int64)
    _lib.check(_lib.lib().sola_mask_select_counts(_lib.ptr(bits), stride, M, T, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(go), _lib.ptr(gi),
                                                  E, _lib.ptr(counts), _lib.current_stream()), "sola_mask_select_counts")
    return counts.cpu().numpy()


M1, T1, STRIDE1, E1 = 9, 5, 44, 12


def raw_case(K):
    """Random planes and the 12 expressions of the raw-ABI tests at K levels."""
    rng = np.random.default_rng(100 + K)
    planes = rng.integers(0, 1 << 32, size=(M1 * T1, STRIDE1), dtype=np.uint64).astype(np.uint32)
    planes[rng.random(M1 * T1) < 0.1] = 0
    pred = [rng.integers(0, M1, size=int(rng.integers(1, 8))).tolist() for _ in range(E1)]
    gt = [rng.integers(0, M1, size=int(rng.integers(1, 4))).tolist() for _ in range(E1)]
    ends = [np.sort(rng.integers(0, len(p) + 1, size=K)).tolist() for p in pred]
    late = min(16, K - 1)  # the first level of the second chunk, where there is one
    pred[0], ends[0] = [], [3] * K                     # an empty candidate list (its ends are too long: clamped to 0)
    gt[1] = []                                         # an empty GT list
    pred[2], gt[2], ends[2] = [], [], [0] * K          # both empty
    pred[3], gt[3] = [1, 1, 8, 1, 8], [8, 1]           # duplicated ids, the same ids in both lists
    ends[3] = np.sort(rng.integers(0, 6, size=K)).tolist()
    pred[4], gt[4] = [2, M1 + 3, 4, -1, 6], [M1, 5]    # ids outside [0, M): ignored
    ends[4] = [min(5, k + 1) for k in range(K)]
    pred[5] = [0, 3, 5, 7]
    ends[5] = [min(4, 2 * (k // 3)) for k in range(K)]  # consecutive equal ends: levels that add nothing
    ends[6] = [0] * (K // 2) + [len(pred[6])] * (K - K // 2)  # leading levels without a track
    ends[7] = [len(pred[7])] * K                       # every track enters at level 0
    pred[8] = [4, 0, 6, 2, 7, 1, 3]
    ends[8] = [0] * late + [7] * (K - late)            # every track enters at level `late`
    pred[9] = [5, 1, 6, 2]
    ends[9] = [min(k + 1, 3) for k in range(K)]
    ends[9][K // 2] = 0                                # one decreasing entry: clamped up to the level before
    ends[9][-1] = 99                                   # one too-long entry: clamped to the list
    if K >= 17:
        ends[10] = [1] * 16 + [len(pred[10])] * (K - 16)  # a non-empty prefix that the second chunk did not build itself
    return planes, pred, ends, gt


@pytest.mark.parametrize("K", [1, 5, 16, 17, 33])
def test_nested_counts_match_numpy(K):
    planes, pred, ends, gt = raw_case(K)
    bits = torch.from_numpy(planes.view(np.int32)).cuda()
    got = nested_counts(bits, STRIDE1, M1, T1, pred, ends, gt)
    assert not (got == -1).any()  # every entry is written
    np.testing.assert_array_equal(got, sc.numpy_nested_counts(planes, T1, pred, ends, gt))
    assert got[8, :min(16, K - 1), :, 1].sum() == 0 and got[7, 0, :, 1].sum() > 0 and got[0, :, :, 1].sum() == 0
    if K > 1:
        assert got[8, K - 1, :, 1].sum() > 0 and not np.array_equal(got[4, 0], got[4, K - 1])
    again = nested_counts(bits, STRIDE1, M1, T1, pred, ends, gt)
    np.testing.assert_array_equal(got, again)  # order-independent: the same from run to run


@pytest.mark.parametrize("K", [1, 5, 16, 17, 33])
def test_nested_level_equals_select_counts_on_the_prefix(K):
    planes, pred, ends, gt = raw_case(K)
    bits = torch.from_numpy(planes.view(np.int32)).cuda()
    got = nested_counts(bits, STRIDE1, M1, T1, pred, ends, gt)
    clamped = [sc.prefix_ends(le, len(p)) for p, le in zip(pred, ends)]
    prefixes = [p[:clamped[e][k]] for e, p in enumerate(pred) for k in range(K)]  # pseudo-expression e*K + k
    want = select_counts(bits, STRIDE1, M1, T1, prefixes, [g for g in gt for _ in range(K)])
    np.testing.assert_array_equal(got.reshape(E1 * K, T1, 3), want)


def test_nested_counts_on_decoded_planes_of_more_than_256_quads():
    h, w, T, M, E, K = 181, 197, 2, 6, 4, 5
    L = _lib.lib()
    stride = L.sola_jf_plane_words(h, w)
    assert stride == 1116 and stride // 4 == 279  # lanes 0..22 run two quad iterations, the others one
    dense = [mc.blob_masklet(T, h, w, 500 + m) for m in range(M)]
    dense[4][:, -1, -1] = 1  # the last position of the plane: the ragged tail word is in use
    masklets = [jc.rle_list(d) for d in dense]
    cum, off = seg_utils._planes_cum(masklets, list(range(M)), T, h * w)
    cum_t = torch.from_numpy(cum.view(np.int32)).cuda()
    off_t = torch.from_numpy(off).cuda()
    bits = torch.full((M * T, stride), -1, device="cuda", dtype=torch.int32)
    _lib.check(L.sola_rle_pack_cm(_lib.ptr(cum_t), _lib.ptr(off_t), M * T, h, w, stride, _lib.ptr(bits), _lib.current_stream()),
               "sola_rle_pack_cm")
    planes = bits.cpu().numpy().view(np.uint32)
    pred = [[0, 1, 2, 3], [4, 2], [5], [3, 4, 0]]
    ends = [[0, 1, 2, 2, 4], [1, 1, 1, 2, 2], [0, 0, 0, 0, 1], [3, 3, 3, 3, 3]]
    gt = [[4, 5], [0], [5, 1], []]
    got = nested_counts(bits, stride, M, T, pred, ends, gt)
    assert not (got == -1).any()
    np.testing.assert_array_equal(got, sc.numpy_nested_counts(planes, T, pred, ends, gt))
    for e in range(E):  # and against the dense masks themselves at the last level
        p = np.logical_or.reduce([dense[m] for m in pred[e][:ends[e][-1]]])
        g = np.logical_or.reduce([dense[m] for m in gt[e]]) if gt[e] else np.zeros_like(p)
        want = np.stack([(p & g).reshape(T, -1).sum(1), p.reshape(T, -1).sum(1), g.reshape(T, -1).sum(1)], 1)
        np.testing.assert_array_equal(got[e, K - 1], want)


# ------------------------------------------------------------------------------------------ masklets, scores, thresholds
@pytest.fixture(scope="module")
def masklet_case():
    """The construction of test_compute_JF_batch_equals_the_oracle (T = 7, 31x45, 12 masklets with missing frames, one empty,
    one uncompressed) plus one IndexMasklet ground truth, candidate lists with float32 scores, and the selection of every
    threshold."""
    T, h, w = 7, 31, 45
    rng = np.random.default_rng(11)
    masklets = []
    for k in range(12):
        masks = mc.blob_masklet(T, h, w, 300 + k)
        if k == 5:
            masks[:] = 0
        masklets.append(jc.rle_list(masks, compressed=k != 3, missing=(k % T,) if k % 4 == 0 else ()))
    maps = np.zeros((T, h, w), np.uint8)
    for k in (1, 2):
        maps[mc.blob_masklet(T, h, w, 340 + k) != 0] = k
    masklets.append(seg_utils.IndexMasklet(torch.from_numpy(maps).cuda(), 2))
    cand_sets = [sorted(set(rng.integers(0, 12, size=rng.integers(1, 7)).tolist())) for _ in range(9)]
    gt_sets = [rng.integers(0, 12, size=rng.integers(1, 3)).tolist() for _ in range(9)]
    cand_sets[0], gt_sets[1], cand_sets[2], gt_sets[2] = [], [], [], []
    cand_sets[3], gt_sets[3] = [4, 4, 6], [6]
    gt_sets[4] = [5]
    gt_sets[6] = [12]       # the index-map ground truth
    gt_sets[7] = [12, 1]
    probs = [rng.random(len(c)).astype(np.float32) for c in cand_sets]
    probs[5][0] = 0.5       # equal to a threshold: not selected there
    probs[3][:] = [0.95, 0.3, 0.05]
    selections = [[[c for c, p in zip(cand_sets[e], probs[e]) if np.float32(p) > np.float32(th)] for e in range(9)]
                  for th in THRESHOLDS]
    assert any(selections[1][e] for e in range(9)) and selections[4] == [list(c) for c in cand_sets] and not any(selections[5])
    return T, h, w, masklets, cand_sets, probs, gt_sets, selections


def test_masklet_sweep_equals_compute_JF_batch_per_threshold(masklet_case):
    T, h, w, masklets, cand_sets, probs, gt_sets, selections = masklet_case
    K = len(THRESHOLDS)
    counts = seg_utils.masklet_sweep_counts(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda")
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (9, K, T, 3) and not counts.is_cuda
    got = seg_utils.compute_JF_sweep(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda")
    for j in range(K):
        assert torch.equal(counts[:, j], seg_utils.masklet_select_counts(masklets, selections[j], gt_sets, "cuda"))
        want = seg_utils.compute_JF_batch(masklets, selections[j], gt_sets, "cuda")
        assert [row[j] for row in got] == want  # float ==, per expression
    assert torch.equal(counts[:, 0], counts[:, 3])  # the duplicated threshold
    assert len({tuple(counts[:, j].reshape(-1).tolist()) for j in range(K)}) == K - 1
    assert seg_utils.compute_JF_sweep(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda", max_plane_bytes=1) == got
    small = 3 * T * _lib.lib().sola_jf_plane_words(h, w) * 4
    assert seg_utils.compute_JF_sweep(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda", max_plane_bytes=small) == got
    with pytest.raises(_lib.SolaError):
        seg_utils.masklet_sweep_counts(masklets, cand_sets, probs, [], gt_sets, "cuda")


def test_masklet_sweep_boundary_counts_equal_select_counts_per_threshold(masklet_case):
    T, h, w, masklets, cand_sets, probs, gt_sets, selections = masklet_case
    K = len(THRESHOLDS)
    counts, bcounts = seg_utils.masklet_sweep_counts(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda", boundary=True)
    assert bcounts.dtype == torch.int64 and tuple(bcounts.shape) == (9, K, T, 4) and not bcounts.is_cuda
    got = seg_utils.compute_JF_sweep(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda", boundary=True)
    for j in range(K):
        c, b = seg_utils.masklet_select_counts(masklets, selections[j], gt_sets, "cuda", boundary=True)
        assert torch.equal(counts[:, j], c) and torch.equal(bcounts[:, j], b)
        assert [row[j] for row in got] == seg_utils.compute_JF_batch(masklets, selections[j], gt_sets, "cuda", boundary=True)
    assert bcounts[:, 4, :, 0].sum() > 0 and bcounts[:, 5, :, 0].sum() == 0
    small = 3 * T * _lib.lib().sola_jf_plane_words(h, w) * 4
    c, b = seg_utils.masklet_sweep_counts(masklets, cand_sets, probs, THRESHOLDS, gt_sets, "cuda", max_plane_bytes=small, boundary=True)
    assert torch.equal(c, counts) and torch.equal(b, bcounts)


# ------------------------------------------------------------------------------------------------ eval.py end to end
def _eval(tmp_path, threshold, extra=()):
    env = dict(os.environ, SOLA_ALLOW_TEXT_STANDIN="1", HF_HUB_OFFLINE="1")
    env.pop("SOLA_PRECISION", None)  # the entry point's own default
    cmd = [sys.executable, os.path.join(ROOT, "eval.py"), "--config", "mevis/jf", "--eval_weight_epoch", "1",
           "--eval_pred_threshold", str(threshold), *extra]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    thr = str(threshold).replace(".", "")
    return r, os.path.join(tmp_path, "SOLA", "EVAL", "jf", "mevis", f"pred_threshold_{thr}", "epoch_1")


def _run_eval(tmp_path, threshold, extra=()):
    r, out = _eval(tmp_path, threshold, extra)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, out


@pytest.fixture(scope="module")
def eval_tree(tmp_path_factory):
    from sola_amd import synth
    from sola_amd.module import LanguageAlignedTrackSelectionModule
    tmp = tmp_path_factory.mktemp("sweep_eval")
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


def _gt(vid, eid):
    annos = jc.VIDEOS[vid][1][eid][1]
    g = np.logical_or.reduce([jc.gt_masks(a) for a in annos])
    if 3 in annos and len(annos) == 1:
        g[4] = 0  # object 3's frame 4 is missing in mask_dict.json
    elif 3 in annos:
        g[4] = jc.gt_masks(7)[4]
    return g


JF_KEYS = {"total", "bce", "alignment", "tp", "fp", "fn", "tn", "bce_evaluator_convention", "samples", "text_encoder", "precision",
           "recall", "mean_J", "mean_F", "mean_JF"}


def test_eval_sweep_writes_the_curve(eval_tree):
    _, out = _run_eval(eval_tree, 0.5, ("--sweep_thresholds", "0.0,0.5,1.0"))
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    jf = json.load(open(os.path.join(out, "valid_u_JF_metrics_1epoch.json")))
    sw = json.load(open(os.path.join(out, "threshold_sweep.json")))
    assert set(sw) == {"thresholds", "mean_J", "mean_F", "mean_JF", "best", "expressions"}
    assert sw["thresholds"] == [0.0, 0.5, 1.0]
    assert set(m) == JF_KEYS | {"sweep_best_threshold", "sweep_best_value"}
    curves = []
    for vid, (grid, exps) in jc.VIDEOS.items():
        assert list(sw["expressions"][vid]) == list(exps)
        for eid, (_, _, gd) in exps.items():
            c = sw["expressions"][vid][eid]
            assert set(c) == {"J", "F", "JF"} and all(len(c[k]) == 3 for k in c)
            assert c["JF"] == [(j + f) / 2 for j, f in zip(c["J"], c["F"])]
            curves.append(c)
            # at 0.5: the JF file's entry, exactly
            assert (c["J"][1], c["F"][1], c["JF"][1]) == (jf[vid][eid]["J"], jf[vid][eid]["F"], jf[vid][eid]["JF"])
            g = _gt(vid, eid)
            # at 1.0 nothing is selected: J is the share of empty GT frames, F is 0
            assert c["J"][2] == float(np.mean([1.0 if not f.any() else 0.0 for f in g])) and c["F"][2] == 0.0
            # at 0.0 every track is selected: the oracle on the OR of all tracks
            preds = np.logical_or.reduce([mo.masklet_decode(jc.rle_list(mc.blob_masklet(jc.T, jc.H, jc.W, a),
                                                                        missing=(0,) if a == 41 else ()))
                                          for a in list(grid) + list(gd)])
            assert (c["J"][0], c["F"][0]) == (mo.compute_J(preds, g), mo.compute_F(preds, g))
    for k in ("J", "F", "JF"):
        assert sw[f"mean_{k}"] == [float(np.mean([c[k][j] for c in curves])) for j in range(3)]
        assert sw[f"mean_{k}"][1] == m[f"mean_{k}"]
    best = int(np.argmax(sw["mean_JF"]))  # (argmax takes the first among equals)
    assert sw["best"] == {"threshold": sw["thresholds"][best], "metric": "mean_JF", "value": sw["mean_JF"][best]}
    assert (m["sweep_best_threshold"], m["sweep_best_value"]) == (sw["best"]["threshold"], sw["best"]["value"])


def test_eval_without_the_flag_is_todays(eval_tree):
    _, out = _run_eval(eval_tree, 0.4)
    assert sorted(os.listdir(out)) == ["track_metrics.json", "valid_u_JF_metrics_1epoch.json"]
    assert set(json.load(open(os.path.join(out, "track_metrics.json")))) == JF_KEYS


def test_eval_sweep_single_value_with_boundary_f(eval_tree):
    _, out = _run_eval(eval_tree, 0.3, ("--sweep_thresholds", "0.3", "--boundary_f", "true"))
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    jf = json.load(open(os.path.join(out, "valid_u_JF_metrics_1epoch.json")))
    sw = json.load(open(os.path.join(out, "threshold_sweep.json")))
    assert sw["thresholds"] == [0.3] and sw["boundary_th"] == m["boundary_th"] == 0.008
    assert set(sw) == {"thresholds", "mean_J", "mean_F", "mean_JF", "mean_F_boundary", "mean_JF_boundary", "boundary_th", "best",
                       "expressions"}
    for k in ("J", "F", "JF", "F_boundary", "JF_boundary"):
        assert sw[f"mean_{k}"] == [m[f"mean_{k}"]]
        for vid, exps in jf.items():
            for eid, e in exps.items():
                assert sw["expressions"][vid][eid][k] == [e[k]]
    assert sw["best"] == {"threshold": 0.3, "metric": "mean_JF_boundary", "value": m["mean_JF_boundary"]}


def test_eval_refuses_a_threshold_outside_0_1(eval_tree):
    r, out = _eval(eval_tree, 0.2, ("--sweep_thresholds", "1.5"))
    assert r.returncode != 0 and "--sweep_thresholds: 1.5 is outside [0, 1]" in r.stderr
    assert os.listdir(out) == []
    r, _ = _eval(eval_tree, 0.2, ("--sweep_thresholds", "0.1,x"))
    assert r.returncode != 0 and "is not a number" in r.stderr
