"""The GPU PNG writer (sola_png_deflate_*, seg_utils.encode_png_*, inference.save_masklet) against the restatement of its
format in png_cases.py, byte for byte, and against PIL, which does not share the restatement."""
import io
import json
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

import masklet_cases as mc  # noqa: E402
import png_cases as pc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


@pytest.fixture(scope="module")
def su():
    from sola_amd import seg_utils
    return seg_utils


def masklet(h, w):
    """(names, (T,h,w) uint8 {0,1}, [png_file of each frame]) of a size, computed once."""
    if (h, w) not in _WANT:
        fr = pc.frames(h, w)
        _WANT[(h, w)] = ([n for n, _ in fr], np.stack([m for _, m in fr]), [pc.png_file(m) for _, m in fr])
    return _WANT[(h, w)]


def as_dtype(m, kind, seed=0):
    """{0,1} uint8 -> a CUDA tensor of the kind whose set pixels are m's; the float kinds carry every sign of zero and both
    signs of value on both sides."""
    t = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    if kind == "uint8":
        return t * 255 if seed % 2 else t  # any non-zero byte counts
    if kind == "bool":
        return t.bool()
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand(t.shape, device="cuda", generator=g) + 0.01
    pick = torch.randint(0, 3, t.shape, device="cuda", generator=g)
    if kind == "float32":  # != 0: negative values are set, both zeros are clear
        on = torch.where(pick == 0, -r, r)
        off = torch.where(pick == 0, torch.full_like(r, -0.0), torch.zeros_like(r))
    else:  # logits: > 0; negative, zero and -0.0 are clear
        on = r
        off = torch.where(pick == 0, -r, torch.where(pick == 1, torch.full_like(r, -0.0), torch.zeros_like(r)))
    return torch.where(t != 0, on, off).float()


def check_files(got, names, m, want):
    assert len(got) == len(want)
    for t, name in enumerate(names):
        assert got[t] == want[t], f"frame {t} ({name}) differs from the restatement: {len(got[t])} vs {len(want[t])} bytes"
        img = Image.open(io.BytesIO(got[t]))
        assert img.mode == "L", name
        np.testing.assert_array_equal(np.array(img), m[t] * 255, err_msg=name)


@pytest.mark.parametrize("kind", ["uint8", "bool", "float32", "logits"])
@pytest.mark.parametrize("h,w", pc.SIZES, ids=[f"{h}x{w}" for h, w in pc.SIZES])
def test_mixed_masklet_equals_the_restatement_byte_for_byte(su, h, w, kind):
    """A few dozen mixed frames in one call: empty, full, corners, checkerboard, stripes of every width of the match rule in
    both directions, noise, blobs."""
    names, m, want = masklet(h, w)
    x = as_dtype(m, kind, seed=h + w)
    got = su.encode_png_masklet(x, logits=(kind == "logits"))
    check_files(got, names, m, want)


@pytest.mark.parametrize("h,w", pc.SIZES, ids=[f"{h}x{w}" for h, w in pc.SIZES])
def test_single_frames_and_encode_png_mask(su, h, w):
    """T = 1, frame by frame (a frame's stream must not depend on its neighbours in the call)."""
    names, m, want = masklet(h, w)
    pick = range(len(names)) if h * w < 100000 else [names.index(n) for n in ("empty", "full", "corner_br", "vstripe259", "noise0.5", "blob1")]
    for t in pick:
        x = torch.from_numpy(m[t]).cuda()
        assert su.encode_png_masklet(x[None]) == [want[t]], names[t]
        assert su.encode_png_mask(x) == want[t], names[t]
    assert su.encode_png_masklet(torch.zeros((0, h, w), dtype=torch.uint8, device="cuda")) == []


def test_unaligned_views_and_many_frames(su):
    """A masklet that starts 1, 2, 3 ... bytes into its allocation (no 16-byte loads possible), and more frames than one
    launch's worth of workgroups on a small frame."""
    names, m, want = masklet(65, 257)
    flat = torch.zeros(m.size + 64, dtype=torch.uint8, device="cuda")
    for shift in (1, 2, 3, 4, 8, 15):
        flat[shift:shift + m.size] = torch.from_numpy(m.reshape(-1)).cuda()
        x = flat[shift:shift + m.size].view(m.shape)
        assert x.data_ptr() % 16 == shift
        assert su.encode_png_masklet(x) == want, shift
    rng = np.random.default_rng(2)
    many = (rng.random((70000, 3, 5)) < 0.5).astype(np.uint8)  # > 65535 frames: two launches
    got = su.encode_png_masklet(torch.from_numpy(many).cuda())
    for t in list(range(0, 70000, 997)) + [65534, 65535, 65536, 69999]:
        assert got[t] == pc.png_file(many[t]), t


def test_encode_png_masklets_equals_per_masklet_calls(su):
    for h, w in [(7, 5), (65, 257), (480, 854)]:
        _, m, want = masklet(h, w)
        parts = [m[:3], m[3:4], m[4:]]
        got = su.encode_png_masklets([torch.from_numpy(p).cuda() for p in parts])
        assert [len(g) for g in got] == [len(p) for p in parts]
        assert [f for g in got for f in g] == want
        for p, g in zip(parts, got):
            assert su.encode_png_masklet(torch.from_numpy(p).cuda()) == g


@pytest.mark.parametrize("h,w", [(7, 5), (65, 257), (720, 1280)])
def test_every_output_byte_is_written(su, h, w):
    """The same streams into buffers pre-filled with 0xA5, 0x00 and 0xFF: partially filled last bytes included."""
    _, m, want = masklet(h, w)
    x = torch.from_numpy(m).cuda()
    ref, offs = su.png_deflate_masklet(x)
    assert [pc.png_wrap(ref[offs[t]:offs[t + 1]], h, w) for t in range(len(m))] == want
    for fill in (0xA5, 0x00, 0xFF):
        out = torch.full((offs[-1] + 32,), fill, dtype=torch.uint8, device="cuda")
        got, o2 = su.png_deflate_masklet(x, out=out)
        assert o2 == offs and got == ref, hex(fill)
        assert bool((out[offs[-1]:] == fill).all())  # and nothing past the end


def test_repeatable_and_stream_independent(su):
    _, m, want = masklet(480, 854)
    x = torch.from_numpy(m).cuda()
    a = su.encode_png_masklet(x)
    b = su.encode_png_masklet(x)
    assert a == b == want
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = su.encode_png_masklet(x)
    s.synchronize()
    assert c == a


def _track_dataset(tmp_path):
    """The small on-disk track dataset of test_gpu_masklet.py::test_dataset_merged_masklet_on_device_matches_host_decoder."""
    from sola_amd import data as sdata
    data_root, track_root = tmp_path / "data", tmp_path / "tracks"
    os.makedirs(data_root / "mevis" / "valid_u")
    meta = {"videos": {"vidA": {"frames": ["00000", "00001", "00002"], "expressions": {"0": {"exp": "a cat", "anno_id": [3]}}}}}
    json.dump(meta, open(data_root / "mevis" / "valid_u" / "meta_expressions.json", "w"))
    mdir = track_root / "grid_tracks" / "mevis" / "valid_u" / "sam2_masklets" / "vidA"
    tdir = track_root / "grid_tracks" / "mevis" / "valid_u" / "sam2_object_tokens" / "vidA"
    os.makedirs(mdir), os.makedirs(tdir)
    for aid in (2, 5, 11):
        frames = mc.blob_masklet(3, 40, 64, aid)
        rle = [{"size": [40, 64], "counts": mo.rle_counts_to_string(mo.mask_to_counts(f))} for f in frames]
        json.dump({"anno_id": aid, "prompt_type": "X", "rle": rle}, open(mdir / f"{aid:05d}.json", "w"))
        np.save(tdir / f"{aid:05d}.npy", np.zeros((3, 256), np.float32))
    split = {"data_name": "mevis", "data_type": "valid_u", "sam2_output_dirs": "grid_tracks", "batch_size": 1}
    return sdata.TrackDataset(split, str(data_root), str(track_root))


def test_save_masklet_writes_the_same_files_with_and_without_gpu_png(tmp_path):
    import inference
    ds = _track_dataset(tmp_path)
    frames = ["00000", "00001", "00002"]
    device = torch.device("cuda", 0)
    for tag, preds in (("several", [1, 0, 1]), ("single", [0, 1, 0]), ("none", [0, 0, 0])):
        p = np.array(preds)
        dirs = {}
        for gpu_png in (False, True):
            out = tmp_path / f"out_{tag}_{int(gpu_png)}"
            inference.save_masklet(ds, "vidA", "0", p, frames, str(out), device, gpu_png=gpu_png)
            dirs[gpu_png] = out
        files = {k: sorted(str(f.relative_to(d)) for f in d.rglob("*") if f.is_file()) for k, d in dirs.items()}
        assert files[False] == files[True] == [os.path.join("vidA", "0", f"{f}.png") for f in frames]
        merged = np.asarray(ds.merged_masklet("vidA", "0", p)) != 0
        assert merged.any() == (tag != "none")
        for t, rel in enumerate(files[True]):
            a, b = Image.open(dirs[False] / rel), Image.open(dirs[True] / rel)
            assert a.mode == b.mode == "L" and a.size == b.size
            np.testing.assert_array_equal(np.array(a), np.array(b))
            np.testing.assert_array_equal(np.array(b), merged[t] * 255)
            assert open(dirs[True] / rel, "rb").read() == pc.png_file(merged[t]), (tag, rel)


def test_inference_subprocess_takes_the_flag_on_synthetic_tracks(tmp_path):
    """The set-up of test_gpu_entrypoints.py::test_train_eval_inference_roundtrip: synthetic tracks have no masks, so the flag
    changes nothing but the report of which writer is configured."""
    os.makedirs(tmp_path / "configs" / "mevis")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mevis", "default.yaml")))
    cfg["dataset"]["track_root"] = str(tmp_path / "no_such_dir")
    yaml.safe_dump(cfg, open(tmp_path / "configs" / "mevis" / "default.yaml", "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SOLA_PRECISION", None)
    common = ["--config", "mevis/default", "--synthetic", "true", "--synthetic_samples", "6", "--synthetic_tracks", "8", "--synthetic_frames", "16"]

    def run(script, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), *common, *extra], cwd=tmp_path, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout

    run("train.py", "--n_epochs_override", "1")
    out = run("inference.py", "--eval_weight_epoch", "1", "--gpu_png", "true")
    assert "PNG writer: GPU deflate" in out
    inf = tmp_path / "SOLA" / "INFERENCE" / "default" / "mevis" / "pred_threshold_05" / "epoch_1"
    assert len(list(inf.rglob("*_pred.npy"))) == 6 and not list(inf.rglob("*.png"))
    assert "PNG writer: PIL" in run("inference.py", "--eval_weight_epoch", "1")
