"""The PNG selection path on the GPU against the numpy restatement of png_select_cases.py and against the library's existing
route (rle_merge_or + encode_png_masklet), byte for byte: sola_planes_cm_to_rm, sola_png_deflate_sizes_select,
seg_utils.encode_png_selections / encode_png_sweep, and inference.py's --gpu_png and --sweep_thresholds end to end."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import jf_cases as jc  # noqa: E402
import masklet_cases as mc  # noqa: E402
import png_cases as pc  # noqa: E402
import png_select_cases as ps  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_TRACKS, _WANT = {}, {}


@pytest.fixture(scope="module")
def su():
    from sola_amd import seg_utils
    return seg_utils


def tracks(h, w, special=False):
    if (h, w, special) not in _TRACKS:
        _TRACKS[(h, w, special)] = ps.tracks(h, w, special)
    return _TRACKS[(h, w, special)]


def decoded_cm(su, rles, h, w):
    """The tracks' column-major planes as the library decodes them (sola_rle_pack_cm through _plane_groups): [M*T, stride]."""
    from sola_amd import _lib
    stride = _lib.lib().sola_jf_plane_words(h, w)
    dev = torch.device("cuda", 0)
    (grp, local, bits, n_ids), = list(su._plane_groups(rles, [list(range(len(rles)))], ps.T, h, w, stride, dev, 1 << 40))
    assert n_ids == len(rles) and [local[m] for m in range(len(rles))] == list(range(len(rles)))
    return bits


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("h,w", ps.SIZES, ids=[f"{h}x{w}" for h, w in ps.SIZES])
def test_transpose_writes_every_word_of_the_row_major_planes(su, h, w):
    masks, rles = tracks(h, w)
    cm = decoded_cm(su, rles, h, w)
    np.testing.assert_array_equal(cm.cpu().numpy().view(np.uint32), ps.cm_planes(masks.reshape(-1, h, w), cm.shape[1]))
    words = su.rm_plane_words(h, w)
    for stride in (words, words + 8):  # pad words behind the plane are written as zero too
        out = torch.full((cm.shape[0], stride), -1, dtype=torch.int32, device="cuda")  # 0xFF everywhere
        got = su.planes_cm_to_rm(cm, h, w, out=out)
        assert got is out
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ps.rm_planes(masks.reshape(-1, h, w), stride))
    fresh = su.planes_cm_to_rm(cm, h, w)
    assert fresh.shape == (cm.shape[0], words) and torch.equal(fresh, su.planes_cm_to_rm(cm, h, w))


def test_transposed_planes_feed_the_iou_kernels(su):
    """The layout is pack_masks': the row-major planes of RLE tracks give pair_counts what the uint8 route gives it."""
    h, w = 33, 95
    masks, rles = tracks(h, w)
    rm = su.planes_cm_to_rm(decoded_cm(su, rles, h, w), h, w)
    words = (h * w + 31) // 32
    bits, area = su.pack_masks(torch.from_numpy(masks.reshape(-1, h, w)).cuda())
    assert torch.equal(rm[:, :words].contiguous(), bits)
    inter, union = su.pair_counts(rm[:, :words].contiguous(), area, bits, area)
    flat = masks.reshape(len(area), -1).astype(np.int64)
    np.testing.assert_array_equal(inter.cpu().numpy(), flat @ flat.T)


# ---------------------------------------------------------------------------------------------------------------- select
def run_select(bits, stride, n_masks, h, w, lists, ends, K, level_end_null=False):
    """One sola_png_deflate_sizes_select + sola_png_deflate_write pair into sentinel-filled buffers: (offs, adler, bytes)."""
    from sola_amd import _lib
    from sola_amd._lib import check, current_stream, ptr
    L = _lib.lib()
    dev = bits.device
    E, n = len(lists), len(lists) * K * ps.T
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    idx = np.array([i for x in lists for i in x] + [0], np.int32)
    off_t, idx_t = torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev)
    lend_t = None if level_end_null else torch.tensor([v for e in ends for v in e], dtype=torch.int32, device=dev)
    nb = L.sola_png_deflate_scratch_bytes(n, h, w)
    scratch = torch.full(((nb + 7) // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)  # dirty scratch
    byte_off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    adler = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stream = current_stream(dev)
    check(L.sola_png_deflate_sizes_select(ptr(bits), stride, n_masks, ps.T, h, w, ptr(off_t), ptr(idx_t), ptr(lend_t), K, E, ptr(byte_off),
                                          ptr(adler), ptr(scratch), nb, stream), "sola_png_deflate_sizes_select")
    offs = byte_off.cpu().tolist()
    out = torch.full((offs[n] + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    check(L.sola_png_deflate_write(ptr(bits), 0, n, h, w, ptr(byte_off), ptr(adler), ptr(out), ptr(scratch), nb, stream),
          "sola_png_deflate_write")
    assert bool((out[offs[n]:] == SENTINEL).all()), "bytes behind the last stream were written"
    return offs, adler.cpu().numpy().view(np.uint32).tolist(), out[:offs[n]].cpu().numpy().tobytes()


def want_streams(h, w, special, K):
    key = (h, w, special, K)
    if key not in _WANT:
        lists = ps.selection_lists()
        ends = ps.level_ends(lists, K)
        _WANT[key] = (lists, ends, ps.select_streams(tracks(h, w, special)[0], lists, ends))
    return _WANT[key]


SELECT_SIZES = [(1, 1, False), (33, 95, False), (64, 63, False), (130, 31, False), (7, 200, False), (100, 200, False), (100, 200, True)]


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("h,w,special", SELECT_SIZES, ids=[f"{h}x{w}{'_ones_zeros' if s else ''}" for h, w, s in SELECT_SIZES])
def test_select_streams_equal_the_restatement_byte_for_byte(su, h, w, special, K):
    masks, rles = tracks(h, w, special)
    lists, ends, want = want_streams(h, w, special, K)
    rm = su.planes_cm_to_rm(decoded_cm(su, rles, h, w), h, w)
    offs, adler, data = run_select(rm, rm.shape[1], ps.M, h, w, lists, ends, K)
    n = len(want)
    assert offs[0] == 0 and [offs[i + 1] - offs[i] for i in range(n)] == [len(s) for s in want]
    assert adler == [ps.adler_of(s) for s in want]
    for i in range(n):
        assert data[offs[i]:offs[i + 1]] == want[i], f"stream {i} (e {i // (K * ps.T)}, level {i // ps.T % K}, frame {i % ps.T})"
    if K == 1:  # a null level_end is the whole list
        assert run_select(rm, rm.shape[1], ps.M, h, w, lists, ends, 1, level_end_null=True) == (offs, adler, data)


@pytest.mark.parametrize("h,w,special", [(33, 95, False), (100, 200, True)])
def test_select_streams_equal_the_existing_route(su, h, w, special):
    """encode_png_masklet(rle_merge_or(selected)) per (list, level): the route inference.py took before."""
    K = 3
    masks, rles = tracks(h, w, special)
    lists, ends, _ = want_streams(h, w, special, K)
    rm = su.planes_cm_to_rm(decoded_cm(su, rles, h, w), h, w)
    offs, _, data = run_select(rm, rm.shape[1], ps.M, h, w, lists, ends, K)
    for e, lst in enumerate(lists):
        for k, end in enumerate(ps.clamp_ends(ends[e], len(lst))):
            sel = [rles[m] for m in lst[:end] if 0 <= m < ps.M]
            merged = su.rle_merge_or(sel, "cuda") if sel else torch.zeros((ps.T, h, w), dtype=torch.uint8, device="cuda")
            files = su.encode_png_masklet(merged)
            for t in range(ps.T):
                i = (e * K + k) * ps.T + t
                assert pc.png_wrap(data[offs[i]:offs[i + 1]], h, w) == files[t], (e, k, t)


# ---------------------------------------------------------------------------------------------------------------- python entries
def test_encode_png_selections_equals_the_existing_route_and_the_restatement(su):
    h, w = 65, 129
    masks, rles = tracks(h, w)
    sets = [[], [4], [0, 1, 2, 3, 4, 5], [5, 1, 5], [2, 0]]
    got = su.encode_png_selections(rles, sets, "cuda")
    assert len(got) == len(sets)
    for s, files in zip(sets, got):
        want = np.zeros((ps.T, h, w), np.uint8)
        for m in s:
            want |= masks[m]
        assert files == [pc.png_file(f) for f in want]
        if s:
            assert files == su.encode_png_masklet(su.rle_merge_or([rles[m] for m in s], "cuda"))
    # several groups of planes and one expression per scratch block: the same files
    small = su.encode_png_selections(rles, sets, "cuda", max_plane_bytes=1, max_scratch_bytes=1)
    assert small == got


@pytest.mark.parametrize("K", [17, 33])
def test_sweep_chunks_levels_blocks_and_groups(su, K):
    """More levels than one launch carries, scratch blocks of one or two expressions and plane groups of a few tracks; scores equal to
    a threshold are not selected (strict >)."""
    from sola_amd import _lib
    h, w = 33, 95
    masks, rles = tracks(h, w)
    rng = np.random.default_rng(K)
    thresholds = [float(np.float32(t)) for t in rng.permutation(np.linspace(0.0, 1.0, K))]  # the caller's order, not sorted
    cand = [[0, 1, 2, 3, 4, 5], [5, 3, 1], [], [2, 2, 4, 0]]
    probs = [np.array([thresholds[i % K] if i % 2 == 0 else rng.random() for i in range(len(c))], np.float32) for c in cand]
    L = _lib.lib()
    plane_bytes = 2 * ps.T * L.sola_jf_plane_words(h, w) * 4              # two tracks' planes per group
    scratch_bytes = L.sola_png_deflate_scratch_bytes(2 * 16 * ps.T, h, w)  # two expressions x 16 levels per block
    got = su.encode_png_sweep(rles, cand, probs, thresholds, "cuda", max_plane_bytes=plane_bytes, max_scratch_bytes=scratch_bytes)
    assert len(got) == len(cand) and all(len(g) == K and all(len(f) == ps.T for f in g) for g in got)
    equal_seen = 0
    for j, t in enumerate(thresholds):
        sets = [[c[i] for i in range(len(c)) if np.float32(p[i]) > np.float32(t)] for c, p in zip(cand, probs)]
        equal_seen += sum(int(np.float32(p[i]) == np.float32(t)) for p in probs for i in range(len(p)))
        assert [g[j] for g in got] == su.encode_png_selections(rles, sets, "cuda"), (j, t)
    assert equal_seen >= 3
    assert su.encode_png_sweep(rles, cand, probs, thresholds, "cuda") == got  # one group, one block per level chunk; a second run
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = su.encode_png_sweep(rles, cand, probs, thresholds, "cuda", max_plane_bytes=plane_bytes, max_scratch_bytes=scratch_bytes)
    s.synchronize()
    assert side == got


def test_unsized_video_is_refused_and_empty_selection_is_zero_frames(su):
    from sola_amd._lib import SolaError
    with pytest.raises(SolaError, match="no size"):
        su.encode_png_selections([[None] * 3, [None] * 3], [[0, 1]], "cuda")
    h, w = 7, 200
    _, rles = tracks(h, w)
    zero = pc.png_file(np.zeros((h, w), np.uint8))
    assert su.encode_png_selections(rles, [[], []], "cuda") == [[zero] * ps.T] * 2
    assert su.encode_png_sweep(rles, [[0, 1]], [[0.4, 0.6]], [1.0, 0.6], "cuda") == [[[zero] * ps.T] * 2]


# ---------------------------------------------------------------------------------------------------------------- inference.py
def _dataset(tree):
    from sola_amd import data as sdata
    cfg = yaml.safe_load(open(tree / "configs" / "mevis" / "jf.yaml"))
    return sdata.TrackDataset(cfg["dataset"]["test"], cfg["dataset"]["data_root"], cfg["dataset"]["track_root"])


def _track_masks(vid, eid):
    """[N,T,h,w] of the expression's tracks in the dataset's order (grid tracks, then its GroundingDINO tracks)."""
    grid, exps = jc.VIDEOS[vid]
    out = []
    for aid in list(grid) + list(exps[eid][2]):
        m = np.asarray(mc.blob_masklet(jc.T, jc.H, jc.W, aid) != 0).astype(np.uint8)
        if aid == 41:
            m[0] = 0  # track 41 starts with a missing frame
        out.append(m)
    return np.stack(out)


def test_save_video_masklets_writes_prob_above_threshold_per_directory(su, tmp_path):
    """The writer under --sweep_thresholds with scores it is handed: strict >, float32, one directory per threshold; the own
    directory follows pred."""
    import inference
    jc.make_tree(str(tmp_path))
    from sola_amd import data as sdata
    ds = sdata.TrackDataset({"data_name": "mevis", "data_type": "valid_u", "sam2_output_dirs": "grid_tracks,gdino_tracks", "batch_size": 1},
                            str(tmp_path / "data"), str(tmp_path / "tracks"))
    frames = [f"{t:05d}" for t in range(jc.T)]
    thresholds = [0.25, 0.5, 0.75]
    rows, vid = [], "vidA"
    for i, eid in enumerate(jc.VIDEOS[vid][1]):
        n = len(_track_masks(vid, eid))
        prob = np.array([[0.1, 0.25, 0.5, 0.75, 0.9][(i + j) % 5] for j in range(n)], np.float32)
        pred = (np.arange(n) % 2 == i % 2).astype(np.float32) if i else (prob > np.float32(0.5)).astype(np.float32)
        rows.append((eid, frames, pred, prob))
    dirs = [str(tmp_path / "own")] + [str(tmp_path / f"t{j}") for j in range(3)]
    inference.save_video_masklets(ds, vid, rows, dirs, thresholds, torch.device("cuda", 0), 0.5)
    for eid, _, pred, prob in rows:
        masks = _track_masks(vid, eid)
        for d, sel in zip(dirs, [pred > 0] + [prob > np.float32(t) for t in thresholds]):
            want = np.logical_or.reduce(masks[sel]) if sel.any() else np.zeros(masks.shape[1:], bool)
            assert sorted(os.listdir(os.path.join(d, vid, eid))) == [f"{f}.png" for f in frames]
            for t, f in enumerate(frames):
                assert open(os.path.join(d, vid, eid, f"{f}.png"), "rb").read() == pc.png_file(want[t]), (d, eid, f)


@pytest.fixture(scope="module")
def infer_tree(tmp_path_factory):
    """jf_cases' tree as the test split, a small model and a checkpoint from train.py --synthetic."""
    from sola_amd import synth
    tmp = tmp_path_factory.mktemp("png_select_infer")
    model = dict(synth.SMALL_MODEL_CFG, roberta_version="sentence-transformers/all-roberta-large-v1")
    data_root, track_root, split = jc.make_tree(str(tmp), token_dim=model["object_token_dim"])
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mevis", "default.yaml")))
    cfg.update(exp_name="jf", model=model)
    cfg["dataset"].update(data_root=data_root, track_root=track_root, test=split)
    os.makedirs(tmp / "configs" / "mevis")
    yaml.safe_dump(cfg, open(tmp / "configs" / "mevis" / "jf.yaml", "w"))
    _run(tmp, "train.py", "--synthetic", "true", "--synthetic_samples", "6", "--synthetic_tracks", "8", "--synthetic_frames", "16",
         "--n_epochs_override", "1")
    return tmp


def _run(tmp, script, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT, SOLA_ALLOW_TEXT_STANDIN="1", HF_HUB_OFFLINE="1")
    env.pop("SOLA_PRECISION", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", "mevis/jf", *extra], cwd=tmp, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _files(d):
    return {str(f.relative_to(d)): f.read_bytes() for f in sorted(d.rglob("*")) if f.is_file()}


def test_inference_writes_every_threshold_from_one_run(infer_tree):
    base = infer_tree / "SOLA" / "INFERENCE" / "jf" / "mevis"
    names = {os.path.join(vid, eid, f"{t:05d}.png") for vid, (_, exps) in jc.VIDEOS.items() for eid in exps for t in range(jc.T)}
    # without either flag: the PIL writer's tree, as it was
    out = _run(infer_tree, "inference.py", "--eval_weight_epoch", "1", "--eval_pred_threshold", "0.5")
    assert "PNG writer: PIL" in out
    assert sorted(os.listdir(base)) == ["pred_threshold_05"]
    pil = _files(base / "pred_threshold_05" / "epoch_1")
    assert set(pil) == names
    merged = {}
    for rel, raw in pil.items():
        img = Image.open(io.BytesIO(raw))
        assert img.mode == "L" and img.size == (jc.W, jc.H)
        merged[rel] = np.array(img) != 0
    # --gpu_png true (another threshold directory, the same selection rule): the files the per-sample GPU writer gave
    out = _run(infer_tree, "inference.py", "--eval_weight_epoch", "1", "--eval_pred_threshold", "0.5", "--gpu_png", "true")
    assert "PNG writer: GPU deflate" in out
    gpu = _files(base / "pred_threshold_05" / "epoch_1")
    assert gpu == {rel: pc.png_file(m) for rel, m in merged.items()}
    # the sweep: three directories; the own one is written once and holds the same files
    out = _run(infer_tree, "inference.py", "--eval_weight_epoch", "1", "--eval_pred_threshold", "0.5", "--sweep_thresholds", "0.0,0.5,1.0")
    assert "PNG writer: GPU deflate" in out
    assert sorted(os.listdir(base)) == ["pred_threshold_00", "pred_threshold_05", "pred_threshold_10"]
    assert _files(base / "pred_threshold_05" / "epoch_1") == gpu
    low, high = _files(base / "pred_threshold_00" / "epoch_1"), _files(base / "pred_threshold_10" / "epoch_1")
    assert set(low) == set(high) == names
    zero = pc.png_file(np.zeros((jc.H, jc.W), np.uint8))
    assert all(raw == zero for raw in high.values())  # no probability exceeds 1.0
    for vid, (_, exps) in jc.VIDEOS.items():
        for eid in exps:
            every = np.logical_or.reduce(_track_masks(vid, eid))  # a sigmoid is > 0.0: every track
            for t in range(jc.T):
                rel = os.path.join(vid, eid, f"{t:05d}.png")
                assert low[rel] == pc.png_file(every[t]), rel
                assert not (merged[rel] & ~every[t]).any()  # the selections are nested
