"""DAVIS boundary F on the GPU (sola_mask_select_boundary_counts): the kernel against the numpy restatement of
boundary_cases on every small shape and radius, the strip path at production sizes, compute_JF_batch(boundary=...) and
compute_F_boundary against the restatement on the oracle's decoded masks, two streams, and eval.py --boundary_f end to end.
Every comparison is exact."""
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

import boundary_cases as bc  # noqa: E402
import jf_cases as jc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


def planes_cm(masks):
    """uint8 [n,h,w] -> int32 [n, stride]: bit j of word i = COCO position 32*i + j (position = x*h + y), zero padded."""
    n, h, w = masks.shape
    stride = _lib.lib().sola_jf_plane_words(h, w)
    flat = np.zeros((n, stride * 32), np.uint8)
    flat[:, :h * w] = (np.asarray(masks) != 0).transpose(0, 2, 1).reshape(n, -1)
    return np.packbits(flat, axis=1, bitorder="little").view("<u4").view(np.int32), stride


def csr(sets, dev):
    off, idx = [0], []
    for s in sets:
        idx += [int(i) for i in s]
        off.append(len(idx))
    return torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(idx + [0], dtype=torch.int32, device=dev)


def kernel_counts(bits, stride, M, T, h, w, r, pred_sets, gt_sets, stream=None):
    """sola_mask_select_boundary_counts on device planes ``bits`` -> device int64 [E, T, 4], every entry pre-set to a sentinel."""
    dev = bits.device
    L = _lib.lib()
    (po, pi), (go, gi) = csr(pred_sets, dev), csr(gt_sets, dev)
    E = len(pred_sets)
    counts = torch.full((E, T, 4), SENTINEL, device=dev, dtype=torch.int64)
    nb = L.sola_boundary_counts_workspace_bytes(h, w, r, E, T)
    ws = torch.empty((max(nb, 1),), device=dev, dtype=torch.uint8)
    _lib.check(L.sola_mask_select_boundary_counts(_lib.ptr(bits), stride, M, T, h, w, r, _lib.ptr(po), _lib.ptr(pi), _lib.ptr(go),
                                                  _lib.ptr(gi), E, _lib.ptr(counts), _lib.ptr(ws), nb,
                                                  _lib.current_stream() if stream is None else stream),
               "sola_mask_select_boundary_counts")
    return counts, (po, pi, go, gi, ws)


def numpy_counts(masks, T, r, pred_sets, gt_sets, dilate=bc.disk_dilate):
    """masks [M*T, h, w] (mask m at frame t = masks[m*T + t]) -> int64 [E, T, 4] from the restatement."""
    M = masks.shape[0] // T
    ml = masks.reshape(M, T, *masks.shape[1:]) != 0
    zeros = np.zeros_like(ml[0])
    out = np.zeros((len(pred_sets), T, 4), np.int64)
    for e, (ps, gs) in enumerate(zip(pred_sets, gt_sets)):
        p = np.logical_or.reduce(ml[[int(i) for i in ps]], axis=0) if len(ps) else zeros
        g = np.logical_or.reduce(ml[[int(i) for i in gs]], axis=0) if len(gs) else zeros
        for t in range(T):
            out[e, t] = bc.boundary_counts(p[t], g[t], r, dilate)
    return out


def small_masks(h, w, rng):
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8)]
    masks += list(mc.blob_masklet(5, h, w, int(rng.integers(1 << 30))))
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]:  # the corners and an interior pixel
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        masks.append(m)
    row, col, frame = (np.zeros((h, w), np.uint8) for _ in range(3))
    row[h // 2, :] = 1   # one-pixel-wide full row
    col[:, w // 3] = 1   # one-pixel-wide full column
    frame[0, :] = frame[h - 1, :] = frame[:, 0] = frame[:, w - 1] = 1  # touches all four borders
    frame[h // 3:h // 3 + 2, :] = 1
    return np.stack(masks + [row, col, frame])


SHAPES = [(1, 1), (1, 37), (29, 1), (2, 2), (23, 37), (32, 4), (64, 5), (33, 70), (17, 33), (90, 160)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_matches_the_restatement(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    masks = small_masks(h, w, rng)
    M, T = masks.shape[0], 1
    pred_sets = [[i] for i in range(M)] + [list(rng.integers(0, M, size=rng.integers(0, 4))) for _ in range(10)]
    gt_sets = [[(i * 7 + 3) % M] for i in range(M)] + [list(rng.integers(0, M, size=rng.integers(0, 3))) for _ in range(10)]
    pred_sets += [[], [2], [], [3, 3, M - 1], [4]]  # empty sets, duplicates, the same masks on both sides
    gt_sets += [[2], [], [], [M - 1, 3], [4]]
    planes, stride = planes_cm(masks)
    bits = torch.from_numpy(planes).cuda()
    for r in (0, 1, 2, 3, 5, 9):
        got, _ = kernel_counts(bits, stride, M, T, h, w, r, pred_sets, gt_sets)
        np.testing.assert_array_equal(got.cpu().numpy(), numpy_counts(masks, T, r, pred_sets, gt_sets), err_msg=f"radius {r}")


def test_kernel_with_several_frames_and_ignored_ids():
    """T > 1 (mask m at frame t = plane m*T + t) and ids outside [0, n_masks), which are ignored as in sola_mask_select_counts."""
    h, w, T, M = 23, 37, 6, 4
    masks = np.concatenate([mc.blob_masklet(T, h, w, 70 + k) for k in range(M)])
    planes, stride = planes_cm(masks)
    bits = torch.from_numpy(planes).cuda()
    pred_sets, gt_sets = [[0, 1], [2], [3, 0], []], [[3], [2, 1], [], [1]]
    want = numpy_counts(masks, T, 1, pred_sets, gt_sets)
    got, _ = kernel_counts(bits, stride, M, T, h, w, 1, pred_sets, gt_sets)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    got, _ = kernel_counts(bits, stride, M, T, h, w, 1, [[0, M, 1], [2, -1], [3, 0], [M + 5]], gt_sets)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_production_540p_through_the_strips():
    h, w, T, r = 540, 960, 4, 9
    assert seg_utils.boundary_radius(h, w) == r
    masks = np.concatenate([mc.blob_masklet(11, h, w, 900 + k)[:T] for k in range(5)])  # drifting blobs, no noise frame
    pred_sets, gt_sets = [[0, 1], [2], [3, 0]], [[4], [1, 4], [3]]
    planes, stride = planes_cm(masks)
    got, _ = kernel_counts(torch.from_numpy(planes).cuda(), stride, 5, T, h, w, r, pred_sets, gt_sets)
    want = numpy_counts(masks, T, r, pred_sets, gt_sets, bc.disk_dilate_rows)
    assert want[:, :, :2].min() > 0 and (want[:, :, 2] < want[:, :, 0]).any()  # real boundaries, partly matched
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_production_1080p_through_the_strips():
    h, w, r = 1080, 1920, 18
    assert seg_utils.boundary_radius(h, w) == r
    masks = np.stack([mc.blob_masklet(11, h, w, 950)[2], mc.blob_masklet(11, h, w, 951)[2]])
    masks[1] |= np.roll(masks[0], (11, 23), (0, 1))  # a near miss of mask 0's contour inside mask 1
    planes, stride = planes_cm(masks)
    got, _ = kernel_counts(torch.from_numpy(planes).cuda(), stride, 2, 1, h, w, r, [[0], [1, 0]], [[1], [0]])
    want = numpy_counts(masks, 1, r, [[0], [1, 0]], [[1], [0]], bc.disk_dilate_rows)
    assert want[0, 0, 2] > 0
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def jf_batch_case():
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
    return T, h, w, masklets, pred_sets, gt_sets


def merged(masklets, pred_sets, gt_sets):
    dec = [mo.masklet_decode(m) for m in masklets]
    zeros = np.zeros_like(dec[0])
    for ps, gs in zip(pred_sets, gt_sets):
        yield (np.logical_or.reduce([dec[i] for i in ps]) if ps else zeros,
               np.logical_or.reduce([dec[i] for i in gs]) if gs else zeros)


@pytest.mark.parametrize("bound_th", [True, 0.05, 2])
def test_compute_JF_batch_boundary_equals_the_restatement(bound_th):
    T, h, w, masklets, pred_sets, gt_sets = jf_batch_case()
    th = 0.008 if bound_th is True else bound_th
    plain = seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda")
    want = []
    for (p, g), (J, F, JF) in zip(merged(masklets, pred_sets, gt_sets), plain):
        Fb = bc.masklet_f(p, g, th)
        want.append((J, F, JF, Fb, (J + Fb) / 2))
    assert len({x[3] for x in want}) > 4  # the expressions differ
    got = seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", boundary=bound_th)
    assert got == want  # float ==, per expression; the first three fields are the call's without `boundary`
    assert seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", boundary=bound_th, max_plane_bytes=1) == want
    small = 3 * T * _lib.lib().sola_jf_plane_words(h, w) * 4
    assert seg_utils.compute_JF_batch(masklets, pred_sets, gt_sets, "cuda", boundary=bound_th, max_plane_bytes=small) == want
    c, b = seg_utils.masklet_select_counts(masklets, pred_sets, gt_sets, "cuda", boundary=bound_th)
    assert torch.equal(c, seg_utils.masklet_select_counts(masklets, pred_sets, gt_sets, "cuda"))
    assert b.dtype == torch.int64 and tuple(b.shape) == (9, T, 4) and not b.is_cuda
    r = bc.radius(h, w, th)
    for e, (p, g) in enumerate(merged(masklets, pred_sets, gt_sets)):
        np.testing.assert_array_equal(b[e].numpy(), np.stack([bc.boundary_counts(p[t], g[t], r) for t in range(T)]))


def test_masklet_select_counts_boundary_without_any_mask():
    T, h, w, masklets, _, _ = jf_batch_case()
    c, b = seg_utils.masklet_select_counts(masklets, [[], []], [[], []], "cuda", boundary=True)
    assert not c.any() and not b.any() and tuple(b.shape) == (2, T, 4)
    assert seg_utils.compute_JF_batch(masklets, [[]], [[]], "cuda", boundary=True) == [(1.0, 0.0, 0.5, 1.0, 1.0)]
    missing = [[None] * T]
    c, b = seg_utils.masklet_select_counts(missing, [[0]], [[0]], "cuda", boundary=True)
    assert tuple(c.shape) == (1, T, 3) and tuple(b.shape) == (1, T, 4) and not b.any()


def test_compute_F_boundary_on_dense_masklets():
    T, h, w, masklets, pred_sets, gt_sets = jf_batch_case()
    for p, g in list(merged(masklets, pred_sets, gt_sets))[3:7]:
        pt, gt = torch.from_numpy(p.astype(np.uint8)).cuda(), torch.from_numpy(g.astype(np.uint8)).cuda()
        assert float(seg_utils.compute_F_boundary(pt, gt)) == bc.masklet_f(p, g)
        assert float(seg_utils.compute_F_boundary(pt.float(), gt.bool(), bound_th=3)) == bc.masklet_f(p, g, 3)
    fg, gt = mc.blob_masklet(3, 90, 160, 21), mc.blob_masklet(3, 90, 160, 22)
    assert float(seg_utils.compute_F_boundary(torch.from_numpy(fg).cuda(), torch.from_numpy(gt).cuda())) == bc.masklet_f(fg, gt)


def test_two_streams_keep_their_own_results():
    h, w, T, r = 90, 160, 5, 2
    rng = np.random.default_rng(3)
    cases = []
    for k in range(2):
        masks = np.concatenate([mc.blob_masklet(T, h, w, 500 + 10 * k + j) for j in range(4)])
        sets = [list(rng.integers(0, 4, size=2)) for _ in range(6)], [list(rng.integers(0, 4, size=1)) for _ in range(6)]
        planes, stride = planes_cm(masks)
        cases.append((masks, sets, torch.from_numpy(planes).cuda(), stride))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got, keep = [], []
    for _ in range(3):  # interleaved launches
        for (masks, (ps, gs), bits, stride), s in zip(cases, streams):
            with torch.cuda.stream(s):
                c, k = kernel_counts(bits, stride, 4, T, h, w, r, ps, gs, stream=_lib.current_stream())
            got.append(c)
            keep.append(k)
    torch.cuda.synchronize()
    want = [numpy_counts(masks, T, r, ps, gs) for masks, (ps, gs), _, _ in cases]
    assert not np.array_equal(want[0], want[1])
    for i, c in enumerate(got):
        np.testing.assert_array_equal(c.cpu().numpy(), want[i % 2])


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
    tmp = tmp_path_factory.mktemp("boundary_eval")
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


def _check_layout(out, stdout, th):
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    jf = json.load(open(os.path.join(out, "valid_u_JF_metrics_1epoch.json")))
    entries = []
    for vid, (_, exps) in jc.VIDEOS.items():
        assert list(jf[vid]) == list(exps)
        for eid, (exp, _, _) in exps.items():
            e = jf[vid][eid]
            assert set(e) == {"expression", "J", "F", "JF", "F_boundary", "JF_boundary"} and e["expression"] == exp
            assert e["JF"] == (e["J"] + e["F"]) / 2 and e["JF_boundary"] == (e["J"] + e["F_boundary"]) / 2
            entries.append(e)
    for k in ("J", "F", "JF", "F_boundary", "JF_boundary"):
        assert m[f"mean_{k}"] == float(np.mean([e[k] for e in entries]))
    assert m["boundary_th"] == th
    printed = json.loads(stdout.strip().splitlines()[-1])
    assert {"mean_F_boundary", "mean_JF_boundary", "boundary_th"} <= set(printed) and printed == m
    return jf


def test_eval_boundary_f_nothing_selected(eval_tree):
    stdout, out = _run_eval(eval_tree, 1.0, ("--boundary_f", "true"))
    jf = _check_layout(out, stdout, 0.008)
    for vid, (_, exps) in jc.VIDEOS.items():
        for eid in exps:
            g = _gt(vid, eid)
            want = float(np.mean([1.0 if not bc.boundary_map(f).any() else 0.0 for f in g]))
            assert jf[vid][eid]["F_boundary"] == want == bc.masklet_f(np.zeros_like(g), g)
            assert jf[vid][eid]["F"] == 0.0


def test_eval_boundary_f_everything_selected(eval_tree):
    stdout, out = _run_eval(eval_tree, 0.0, ("--boundary_f", "true", "--boundary_th", "0.05"))
    jf = _check_layout(out, stdout, 0.05)
    assert bc.radius(jc.H, jc.W, 0.05) == 3
    for vid, (grid, exps) in jc.VIDEOS.items():
        for eid, (_, _, gd) in exps.items():
            preds = np.logical_or.reduce([mo.masklet_decode(jc.rle_list(mc.blob_masklet(jc.T, jc.H, jc.W, a),
                                                                        missing=(0,) if a == 41 else ()))
                                          for a in list(grid) + list(gd)])
            g = _gt(vid, eid)
            assert jf[vid][eid]["F_boundary"] == bc.masklet_f(preds, g, 0.05)
            assert (jf[vid][eid]["J"], jf[vid][eid]["F"]) == (mo.compute_J(preds, g), mo.compute_F(preds, g))
