"""Index maps -> bit planes on the GPU: sola_index_hist and both layouts of sola_index_pack against the numpy restatement of
tests/index_cases.py (exact equality of every word and count), the seg_utils wrappers, IndexMasklet ground truth mixed with RLE
tracks in compute_JF_batch, and eval.py end to end on a Ref-DAVIS-layout tree."""
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
import index_cases as ic  # noqa: E402
import jf_cases as jc  # noqa: E402
import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402
from sola_amd import data as sdata  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
VALUES = [0, 1, 2, 3, 5, 9, 200, 255]
ABSENT = 77


def on_device(maps, offset=0):
    """The maps as a [T,h,w] view that starts ``offset`` bytes into a 256-byte-aligned allocation."""
    buf = torch.empty(maps.size + offset + 64, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + maps.size].view(maps.shape)
    view.copy_(torch.from_numpy(maps))
    assert view.data_ptr() % 16 == offset % 16
    return view


# ----------------------------------------------------------------------------------------------------------- histogram
def hist_contents(T, h, w):
    yield "uniform", ic.random_maps(T, h, w, 1)
    for v in (0, 7, 255):
        yield f"all {v}", np.full((T, h, w), v, np.uint8)
    yield "two values", ic.random_maps(T, h, w, 2, values=[3, 250])


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 37, 61), (2, 64, 256), (1, 480, 854)])
def test_index_hist_matches_bincount(shape):
    for name, maps in hist_contents(*shape):
        for offset in (0, 1):
            got = seg_utils.index_hist(on_device(maps, offset))
            assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], 256) and got.is_cuda
            np.testing.assert_array_equal(got.cpu().numpy(), ic.hist(maps), err_msg=f"{name}, offset {offset}")


def test_index_hist_is_the_same_on_every_run_and_object_ids_follow_the_rules():
    maps = ic.random_maps(3, 37, 61, 5, values=VALUES)
    maps[0][maps[0] == 9] = 0  # object 9 is absent from frame 0
    d = on_device(maps, 3)
    first = seg_utils.index_hist(d)
    for _ in range(3):
        assert torch.equal(seg_utils.index_hist(d), first)
    assert seg_utils.index_object_ids(d, "davis") == ic.object_ids(maps, "davis") == [1, 2, 3, 5, 200]
    assert seg_utils.index_object_ids(d, "ytbvos") == ic.object_ids(maps, "ytbvos") == [1, 2, 3, 5, 9, 200, 255]


# ---------------------------------------------------------------------------------------------------------------- pack
def id_list(K):
    pool = [5, ABSENT, 0, 255, 5, -1, 256, 1, 2, 3, 9, 200, 1000, 255, 4, 0, 2]
    assert len(pool) == 2 * ic.ID_CHUNK + 1
    return pool[:K]


def run_pack(d_maps, ids, layout, stride, first=None, rows=None, stream=None):
    """(bits uint32 [rows, stride], area int64 [rows]) from one sola_index_pack call into sentinel-filled buffers."""
    T, h, w = d_maps.shape
    rows = len(ids) * T if rows is None else rows
    bits = torch.full((rows, stride), SENTINEL, device="cuda", dtype=torch.int32)
    area = torch.full((rows,), -7, device="cuda", dtype=torch.int64)
    d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    d_first = None if first is None else torch.tensor(first, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().sola_index_pack(_lib.ptr(d_maps), T, h, w, _lib.ptr(d_ids), len(ids), _lib.ptr(d_first), layout, stride,
                                          _lib.ptr(bits), _lib.ptr(area), stream or _lib.current_stream()), "sola_index_pack")
    return bits, area


def popcounts(planes):
    return np.unpackbits(planes.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


PACK_SHAPES = [(1, 1), (1, 70), (70, 1), (5, 3), (31, 33), (32, 32), (33, 31), (37, 61), (64, 256), (100, 7), (1100, 70), (37, 300)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hw", PACK_SHAPES)
def test_index_pack_matches_the_restatement(hw, layout):
    h, w = hw
    planes_of = ic.cm_planes if layout else ic.rm_planes
    least = ic.cm_words(h, w) if layout else ic.rm_words(h, w)
    for T, offset in ((1, 0), (3, 5)):  # (offset 5: an unaligned base pointer)
        maps = ic.random_maps(T, h, w, 10 * h + w + T, values=VALUES)
        d_maps = on_device(maps, offset)
        for K in (1, 3, ic.ID_CHUNK + 1, 2 * ic.ID_CHUNK + 1):
            ids = id_list(K)
            what = f"T {T}, K {K}"
            # planes k*T + t, the least stride
            bits, area = run_pack(d_maps, ids, layout, least)
            want = planes_of(maps, ids)
            np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), want, err_msg=what)
            np.testing.assert_array_equal(area.cpu().numpy(), popcounts(want), err_msg=what)
            # a wider stride (pad words are zeros) and permuted first planes with one block of T rows nobody addresses
            stride = least + 8
            perm = np.random.default_rng(K).permutation(K + 1)
            first = [int(p) * T for p in perm[:K]]
            bits, area = run_pack(d_maps, ids, layout, stride, first=first, rows=(K + 1) * T)
            want = np.full(((K + 1) * T, stride), SENTINEL, np.uint32)
            want_area = np.full(((K + 1) * T,), -7, np.int64)
            padded = planes_of(maps, ids, stride)
            for k, p in enumerate(first):
                want[p:p + T] = padded[k * T:(k + 1) * T]
                want_area[p:p + T] = popcounts(padded[k * T:(k + 1) * T])
            np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), want, err_msg=what + ", first_plane")
            np.testing.assert_array_equal(area.cpu().numpy(), want_area, err_msg=what + ", first_plane")


@pytest.mark.parametrize("layout", [0, 1])
def test_index_pack_on_a_side_stream_gives_the_same_bits(layout):
    T, h, w = 3, 37, 61
    maps = ic.random_maps(T, h, w, 3, values=VALUES)
    d_maps = on_device(maps, 1)
    stride = ic.cm_words(h, w) if layout else ic.rm_words(h, w)
    ids = id_list(ic.ID_CHUNK + 1)
    bits, area = run_pack(d_maps, ids, layout, stride)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        bits2, area2 = run_pack(d_maps, ids, layout, stride, stream=_lib.current_stream())
    side.synchronize()
    assert torch.equal(bits, bits2) and torch.equal(area, area2)
    np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), (ic.cm_planes if layout else ic.rm_planes)(maps, ids))


def test_pack_index_masklets_wrapper():
    T, h, w = 2, 33, 31
    maps = ic.random_maps(T, h, w, 8, values=VALUES)
    d = on_device(maps)
    bits, area = seg_utils.pack_index_masklets(d, [1, 255, ABSENT])
    np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), ic.rm_planes(maps, [1, 255, ABSENT]))
    np.testing.assert_array_equal(area.cpu().numpy(), popcounts(ic.rm_planes(maps, [1, 255, ABSENT])))
    ref_bits, ref_area = seg_utils.pack_masks(torch.from_numpy((maps == 255).astype(np.uint8)).cuda())
    assert torch.equal(bits[T:2 * T], ref_bits) and torch.equal(area[T:2 * T], ref_area)  # sola_mask_pack's own planes
    cm, none = seg_utils.pack_index_masklets(d, torch.tensor([2, 0], dtype=torch.int32, device="cuda"), "cm")
    assert none is None
    np.testing.assert_array_equal(cm.cpu().numpy().view(np.uint32), ic.cm_planes(maps, [2, 0]))
    out = torch.full((3 * T, ic.cm_words(h, w)), 11, dtype=torch.int32, device="cuda")
    same, _ = seg_utils.pack_index_masklets(d, [3], "cm", out=out, first_plane=[2 * T])
    assert same is out and (out[:2 * T] == 11).all()
    np.testing.assert_array_equal(out[2 * T:].cpu().numpy().view(np.uint32), ic.cm_planes(maps, [3]))
    for ids, first in (([3, 5], [0, T - 1]), ([3], [-1]), ([3], [2 * T + 1])):  # overlapping, negative, past the end
        with pytest.raises(_lib.SolaError):
            seg_utils.pack_index_masklets(d, ids, "cm", out=out, first_plane=first)
    with pytest.raises(_lib.SolaError):
        seg_utils.pack_index_masklets(d, [3], "diagonal")


# ------------------------------------------------------------------------------------------------------------ wrappers
def test_index_masklets_equals_the_dict_restatement():
    T, h, w = 3, 37, 61
    maps = ic.random_maps(T, h, w, 4, values=VALUES)
    d = on_device(maps, 2)
    want = ic.masklets_dict(maps)
    got = seg_utils.index_masklets(d)
    assert list(got) == list(want) == ["1", "2", "3", "5", "9", "200", "255"]
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].is_cuda
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k])
    got = seg_utils.index_masklets(d, ids=[9, ABSENT, 2, 300])
    assert list(got) == ["9", "2"]  # empties dropped
    np.testing.assert_array_equal(got["2"].cpu().numpy(), want["2"])
    assert seg_utils.index_masklets(on_device(np.zeros((2, 5, 5), np.uint8))) == {}


def test_index_masklets_reshape_is_reshape_masklet_on_the_compare():
    T, h, w = 3, 20, 36
    maps = np.zeros((T, h, w), np.uint8)
    for k in (1, 2, 6):
        maps[mc.blob_masklet(T, h, w, 40 + k) != 0] = k
    d = on_device(maps, 1)
    got = seg_utils.index_masklets(d, reshape=True, target_shape=(27, 48))
    assert list(got) == [str(k) for k in ic.object_ids(maps, "ytbvos")] and len(got) >= 2
    for k, m in got.items():
        want = seg_utils.reshape_masklet((d == int(k)).to(torch.uint8), (27, 48))
        assert tuple(m.shape) == (T, 27, 48) and torch.equal(m, want)
    one = seg_utils.index_masklets(d, ids=[2], reshape=True)
    assert torch.equal(one["2"], seg_utils.reshape_masklet((d == 2).to(torch.uint8))) and tuple(one["2"].shape) == (T, 540, 960)


# ------------------------------------------------------------------------------------------------------------ mixed J&F
@pytest.mark.parametrize("hw", [(37, 61), (100, 7)])
def test_compute_JF_batch_with_index_ground_truth_equals_rle_ground_truth(hw):
    T, (h, w) = 3, hw
    rng = np.random.default_rng(h)
    maps = np.zeros((T, h, w), np.uint8)
    for k in (1, 2, 3):
        maps[mc.blob_masklet(T, h, w, 70 + k) != 0] = k
    d = on_device(maps, 1)
    tracks = [jc.rle_list(mc.blob_masklet(T, h, w, 80 + j), compressed=j != 2, missing=(1,) if j == 3 else ()) for j in range(5)]
    objects = [1, 2, 3, ABSENT]
    as_index = tracks + [seg_utils.IndexMasklet(d, k) for k in objects]
    as_rle = tracks + [[sdata.rle_encode_uncompressed((f == k).astype(np.uint8)) for f in maps] for k in objects]
    pred_sets = [sorted(set(rng.integers(0, 5, size=rng.integers(1, 4)).tolist())) for _ in range(7)]
    gt_sets = [[5], [6], [7], [8], [5, 7], [6, 6], []]
    before = seg_utils.masklet_select_counts(tracks, pred_sets, [[0]] * 7, "cuda", boundary=True)
    want = seg_utils.masklet_select_counts(as_rle, pred_sets, gt_sets, "cuda", boundary=True)
    got = seg_utils.masklet_select_counts(as_index, pred_sets, gt_sets, "cuda", boundary=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0][:, :, 2].sum() > 0 and len({tuple(c.reshape(-1).tolist()) for c in got[0]}) > 4
    g = np.logical_or(maps == 1, maps == 3)  # and against numpy on the maps themselves
    assert got[0][4, :, 2].tolist() == g.reshape(T, -1).sum(axis=1).tolist()
    assert seg_utils.compute_JF_batch(as_index, pred_sets, gt_sets, "cuda", boundary=True) == \
        seg_utils.compute_JF_batch(as_rle, pred_sets, gt_sets, "cuda", boundary=True)
    assert seg_utils.compute_JF_batch(as_index, pred_sets, gt_sets, "cuda", max_plane_bytes=1) == \
        seg_utils.compute_JF_batch(as_rle, pred_sets, gt_sets, "cuda")
    after = seg_utils.masklet_select_counts(tracks, pred_sets, [[0]] * 7, "cuda", boundary=True)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])  # no state leaks
    with pytest.raises(_lib.SolaError):
        seg_utils.masklet_select_counts(as_index + [seg_utils.IndexMasklet(d[:2], 1)], [[0]], [[9]], "cuda")  # T differs
    with pytest.raises(_lib.SolaError):
        seg_utils.masklet_select_counts(as_index + [seg_utils.IndexMasklet(d[:, 1:], 1)], [[0]], [[9]], "cuda")  # (h, w) differs


# ------------------------------------------------------------------------------------------------ eval.py end to end
@pytest.fixture(scope="module")
def davis_tree(tmp_path_factory):
    from sola_amd import synth
    from sola_amd.module import LanguageAlignedTrackSelectionModule
    tmp = tmp_path_factory.mktemp("davis_eval")
    model = dict(synth.SMALL_MODEL_CFG, roberta_version="sentence-transformers/all-roberta-large-v1")
    data_root, track_root, split = ic.make_davis_tree(str(tmp), token_dim=model["object_token_dim"])
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mevis", "default.yaml")))
    cfg.update(exp_name="jf", model=model)
    cfg["dataset"].update(data_root=data_root, track_root=track_root, valid=split)
    os.makedirs(tmp / "configs" / "ref-davis")
    yaml.safe_dump(cfg, open(tmp / "configs" / "ref-davis" / "jf.yaml", "w"))
    torch.manual_seed(0)
    wdir = tmp / "SOLA" / "TRAIN" / "jf" / cfg["dataset"]["train"]["data_name"]
    os.makedirs(wdir)
    torch.save(LanguageAlignedTrackSelectionModule(model).state_dict(), wdir / "epoch_1.pth")
    return tmp, (data_root, track_root, split)


def test_eval_scores_ref_davis_against_the_annotation_frames(davis_tree):
    tmp, _ = davis_tree
    env = dict(os.environ, SOLA_ALLOW_TEXT_STANDIN="1", HF_HUB_OFFLINE="1")
    env.pop("SOLA_PRECISION", None)
    cmd = [sys.executable, os.path.join(ROOT, "eval.py"), "--config", "ref-davis/jf", "--eval_weight_epoch", "1",
           "--eval_pred_threshold", "0.0", "--boundary_f", "true"]
    r = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "J&F skipped" not in r.stdout
    out = os.path.join(tmp, "SOLA", "EVAL", "jf", "ref-davis", "pred_threshold_00", "epoch_1")
    m = json.load(open(os.path.join(out, "track_metrics.json")))
    jf = json.load(open(os.path.join(out, "valid_JF_metrics_1epoch.json")))
    entries = []
    for vid, (grid, _, exps) in ic.VIDEOS.items():
        assert list(jf[vid]) == list(exps)
        preds = np.logical_or.reduce([ic.track_masks(a) for a in grid])  # threshold 0: every track is selected
        maps = ic.annotation(vid)
        for eid, (exp, obj) in exps.items():
            e = jf[vid][eid]
            g = maps == obj
            assert set(e) == {"expression", "J", "F", "JF", "F_boundary", "JF_boundary"} and e["expression"] == exp
            assert (e["J"], e["F"]) == (mo.compute_J(preds, g), mo.compute_F(preds, g))
            assert e["F_boundary"] == bc.masklet_f(preds, g, 0.008)
            assert e["JF"] == (e["J"] + e["F"]) / 2 and e["JF_boundary"] == (e["J"] + e["F_boundary"]) / 2
            entries.append(e)
    assert len({e["J"] for e in entries}) > 3  # the objects of a video score differently: no shared ground truth
    for k in ("J", "F", "JF", "F_boundary", "JF_boundary"):
        assert m[f"mean_{k}"] == float(np.mean([e[k] for e in entries]))
    assert json.loads(r.stdout.strip().splitlines()[-1]) == m


def test_jf_entries_share_one_upload_and_refuse_a_frame_count_mismatch(davis_tree):
    import eval as ev
    _, (data_root, track_root, split) = davis_tree
    ds = sdata.TrackDataset(split, data_root, track_root)
    a = ds.gt_masklets("bear", "0", "cuda")
    b = ds.gt_masklets("bear", "1", "cuda")
    c = ds.gt_masklets("bear", "2", "cuda")
    assert len(a) == 1 and a[0] is b[0] and c[0] is not a[0] and c[0].index_maps is a[0].index_maps
    assert isinstance(a[0], seg_utils.IndexMasklet) and a[0].index_maps.is_cuda and (a[0].obj_id, c[0].obj_id) == (1, 3)
    rows = [("camel", e, x, np.ones(2, bool)) for e, (x, _) in ic.VIDEOS["camel"][2].items()]
    got = ev.jf_entries(ds, rows, torch.device("cuda"))
    preds = np.logical_or.reduce([ic.track_masks(t) for t in ic.VIDEOS["camel"][0]])
    for (_, eid, e), (_, obj) in zip(got, ic.VIDEOS["camel"][2].values()):
        assert e["J"] == mo.compute_J(preds, ic.annotation("camel") == obj)
    short = sdata.TrackDataset(split, data_root, track_root)
    short._index_cache = ("camel", ic.annotation("camel")[:-1].copy())  # an annotation folder with a frame less
    with pytest.raises(RuntimeError, match=f"camel.*{ic.T} frames.*{ic.T - 1}"):
        ev.jf_entries(short, rows, torch.device("cuda"))
