"""Masks -> COCO compressed RLE on the GPU (rle_encode.hip, seg_utils.encode_rle_*): every frame's string byte for byte
against the CPU oracle's pycocotools restatement, rle_counts_to_string(mask_to_counts(frame)), and round trips through the
decoders already in the tree."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import masklet_cases as mc  # noqa: E402
from oracle import masklet_oracle as mo  # noqa: E402
from sola_amd import _lib, data  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def su():
    from sola_amd import seg_utils
    return seg_utils


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def oracle(frames):
    return [mo.rle_counts_to_string(mo.mask_to_counts(f)) for f in np.asarray(frames)]


def assert_encodes(su, frames, dtype=torch.uint8, **kw):
    frames = np.asarray(frames)
    got = su.encode_rle_masklet(dev(frames, dtype), **kw)
    want = oracle(frames != 0)
    assert len(got) == len(want)
    h, w = frames.shape[1:]
    for t, (g, s) in enumerate(zip(got, want)):
        assert g["size"] == [h, w], (t, g["size"])
        assert type(g["counts"]) is str
        assert g["counts"] == s, (t, h, w, g["counts"][:80], s[:80])
    return got


def from_runs(h, w, runs):
    runs = list(runs) + [h * w - sum(runs)]
    assert runs[-1] >= 0
    return mo.rle_decode({"size": [h, w], "counts": runs})


def test_hand_vectors(su):
    m = np.array([0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1], np.uint8).reshape(4, 3).T  # column-major 3x4 of test_entrypoints_cpu
    assert su.encode_rle_mask(dev(m)) == {"size": [3, 4], "counts": "2340"}
    assert su.encode_rle_mask(dev(np.zeros((10, 10), np.uint8))) == {"size": [10, 10], "counts": "T3"}
    assert su.encode_rle_mask(dev(np.ones((1, 1), np.uint8)))["counts"] == mo.rle_counts_to_string([0, 1])


@pytest.mark.parametrize("hw", [(540, 960), (960, 540), (720, 1280), (1080, 1920)])
def test_sam2_like_blobs(su, hw):
    h, w = hw
    assert_encodes(su, mc.blob_masklet(6, h, w, seed=h + w))  # blobs, an empty, a full and a white-noise frame


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (37, 53), (33, 65), (65, 16), (127, 20), (130, 17), (64, 64), (200, 48),
                                (3, 1024)])
def test_small_and_odd_shapes(su, hw):
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    frames = np.concatenate([(rng.random((3, h, w)) < p).astype(np.uint8) for p in (0.05, 0.5, 0.95)]
                            + [mc.blob_masklet(4, h, w, seed=w)])
    assert_encodes(su, frames)


def test_content_edge_cases(su):
    h, w = 70, 33  # more rows than one band, width not a multiple of 4
    f = []
    f.append(np.zeros((h, w), np.uint8))
    f.append(np.ones((h, w), np.uint8))
    m = np.zeros((h, w), np.uint8); m[0, 0] = 1; f.append(m)                  # only (0,0): first run of length 0
    m = np.zeros((h, w), np.uint8); m[h - 1, w - 1] = 1; f.append(m)          # only the last pixel
    m = np.zeros((h, w), np.uint8); m[h - 5:, 10] = 1; m[:7, 11] = 1; f.append(m)  # one run wrapping from column 10 to 11
    m = np.zeros((h, w), np.uint8); m[h - 1, 3] = 1; m[0, 4] = 1; f.append(m)  # wrap of length 2 across the band walk's seam
    m = np.zeros((h, w), np.uint8); m[63:65, :] = 1; f.append(m)             # a run across the band boundary
    f.append((np.arange(w)[None, :] % 2 == 0).repeat(h, 0).astype(np.uint8))  # width-1 vertical stripes
    f.append((np.arange(h)[:, None] % 2 == 1).repeat(w, 1).astype(np.uint8))  # horizontal stripes
    assert_encodes(su, np.stack(f))


def test_checkerboard(su):
    cb = ((np.arange(128)[:, None] + np.arange(128)[None, :]) % 2).astype(np.uint8)
    got = assert_encodes(su, np.stack([cb, 1 - cb]))
    # every pixel starts a run except the first of each column, which repeats the last of the column before
    assert len(mo.rle_string_to_counts(got[0]["counts"])) == 128 * 128 - 127
    assert len(mo.rle_string_to_counts(got[1]["counts"])) == 128 * 128 - 127 + 1  # (0,0) set: an empty first run


def test_run_lengths_cover_every_character_count(su):
    """Runs around 15/16, 511/512, 16383/16384 and above 2^19, in growing and shrinking order, so the deltas rleToString
    writes take 1 to 5 characters of both signs."""
    h, w = 1080, 1920
    ladder = [15, 16, 15, 16, 511, 512, 511, 16383, 16384, 16383, 15, 600000, 1, 524289, 16, 16384, 511, 1, 512, 16383]
    frames = [from_runs(h, w, ladder), from_runs(h, w, [0] + ladder), from_runs(h, w, [1_000_003, 1])]  # last: one pixel set
    frames.append(from_runs(h, w, [h * w - 1]))  # only the very last pixel set
    got = assert_encodes(su, np.stack(frames))
    lens = set()
    for s in [g["counts"] for g in got]:
        p = 0
        while p < len(s):  # group the string into its values
            q = p
            while (ord(s[q]) - 48) & 0x20:
                q += 1
            lens.add(q - p + 1)
            p = q + 1
    assert {1, 2, 3, 4, 5} <= lens, lens


def test_dtypes(su):
    rng = np.random.default_rng(7)
    frames = mc.blob_masklet(5, 96, 160, seed=3)
    base = assert_encodes(su, frames, torch.uint8)
    assert su.encode_rle_masklet(dev(frames.astype(bool))) == base
    assert su.encode_rle_masklet(dev(frames, torch.float32)) == base
    # float32 pixels count when != 0 (any value, -0.0 does not), as in the library's other mask functions
    vals = rng.standard_normal(frames.shape).astype(np.float32) * frames
    vals[0, :3, :3] = -0.0
    assert su.encode_rle_masklet(dev(vals)) == base
    # tracker logits: (x > 0), equal to encoding the thresholded masks
    logits = (rng.standard_normal((5, 96, 160)) * 4).astype(np.float32)
    logits[1, ::3, ::5] = 0.0
    logits[2, 1::4] = -0.0
    got = su.encode_rle_masklet(dev(logits), logits=True)
    assert got == su.encode_rle_masklet(dev(logits > 0))
    assert [g["counts"] for g in got] == oracle(logits > 0)
    # the float paths at a width that takes the scalar lane walk
    odd = (rng.standard_normal((3, 70, 33))).astype(np.float32)
    assert [g["counts"] for g in su.encode_rle_masklet(dev(odd), logits=True)] == oracle(odd > 0)
    assert [g["counts"] for g in su.encode_rle_masklet(dev(odd))] == oracle(odd != 0)
    with pytest.raises(_lib.SolaError):
        su.encode_rle_masklet(dev(frames), logits=True)


def test_unaligned_base_pointer(su):
    rng = np.random.default_rng(11)
    frames = (rng.random((3, 20, 64)) < 0.3).astype(np.uint8)
    flat = torch.zeros(1 + frames.size, dtype=torch.uint8, device="cuda")
    view = flat[1:].view(frames.shape)
    view.copy_(dev(frames))
    assert view.data_ptr() % 16 == 1
    assert [g["counts"] for g in su.encode_rle_masklet(view)] == oracle(frames)


def test_round_trips(su):
    rng = np.random.default_rng(5)
    frames = np.concatenate([mc.blob_masklet(6, 120, 200, seed=9), (rng.random((2, 120, 200)) < 0.5).astype(np.uint8)])
    T, h, w = frames.shape
    rles = su.encode_rle_masklet(dev(frames))
    # cum -> sola_rle_fill_or on the device (offsets = run_off, K = 1)
    cum, run_off = su.encode_rle_masklet(dev(frames), return_cum=True)
    assert cum.dtype == torch.int32 and run_off.dtype == torch.int64 and run_off.shape == (T + 1,)
    ro = run_off.cpu().numpy()
    cum_np = cum.cpu().numpy().view(np.uint32)
    assert ro[0] == 0 and ro[-1] == len(cum_np)
    for t in range(T):
        np.testing.assert_array_equal(cum_np[ro[t]:ro[t + 1]], np.cumsum(mo.mask_to_counts(frames[t])))
    out = torch.empty((T, h, w), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().sola_rle_fill_or(_lib.ptr(cum), _lib.ptr(run_off), T, 1, h, w, _lib.ptr(out), None, None,
                                           _lib.current_stream()), "sola_rle_fill_or")
    np.testing.assert_array_equal(out.cpu().numpy(), frames)
    # strings -> data.rle_decode, the library's host parser, seg_utils.rle_merge_or
    for t, r in enumerate(rles):
        np.testing.assert_array_equal(data.rle_decode(r), frames[t])
        np.testing.assert_array_equal(su._rle_cum(r, h * w), cum_np[ro[t]:ro[t + 1]])
    np.testing.assert_array_equal(su.rle_merge_or([rles], "cuda").cpu().numpy(), frames)
    # the character phase alone encodes prefix sums that came from the decoder side
    cum2 = torch.from_numpy(np.concatenate([su._rle_cum(r, h * w) for r in rles]).view(np.int32)).cuda()
    lens = [len(r["counts"]) for r in rles]
    char_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device="cuda")
    chars = torch.empty(sum(lens), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().sola_rle_encode_chars(_lib.ptr(cum2), _lib.ptr(run_off), _lib.ptr(char_off), T, _lib.ptr(chars),
                                                _lib.current_stream()), "sola_rle_encode_chars")
    assert chars.cpu().numpy().tobytes().decode() == "".join(r["counts"] for r in rles)


def test_masklets_of_a_batch_in_one_call(su):
    tracks = [mc.blob_masklet(T, 90, 128, seed=T) for T in (4, 1, 7, 3)]
    got = su.encode_rle_masklets([dev(m) for m in tracks])
    assert got == [su.encode_rle_masklet(dev(m)) for m in tracks]
    assert [[g["counts"] for g in track] for track in got] == [oracle(m) for m in tracks]


def test_two_streams_at_once(su):
    rng = np.random.default_rng(3)
    inputs = [np.concatenate([mc.blob_masklet(5, 360, 640, seed=s), (rng.random((1, 360, 640)) < 0.5).astype(np.uint8)])
              for s in (1, 2)]
    want = [oracle(x) for x in inputs]
    tensors = [dev(x) for x in inputs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results, errors = [None, None], []

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                for _ in range(4):
                    results[i] = [g["counts"] for g in su.encode_rle_masklet(tensors[i])]
                    assert results[i] == want[i]
        except Exception as e:  # reported on the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results == want
    # the return_cum form on a side stream, checked after that stream alone
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        cum, run_off = su.encode_rle_masklet(tensors[0], return_cum=True)
    s.synchronize()
    ro = run_off.cpu().numpy()
    np.testing.assert_array_equal(cum.cpu().numpy().view(np.uint32)[ro[2]:ro[3]], np.cumsum(mo.mask_to_counts(inputs[0][2])))


def test_more_frames_than_one_launch_holds(su):
    """n above the 65535 frames of one launch's grid: the launches are chunked."""
    n, h, w = 70_000, 2, 3
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 64, n)
    pats = ((np.arange(64)[:, None] >> np.arange(6)[None, :]) & 1).astype(np.uint8).reshape(64, h, w)
    table = oracle(pats)
    got = su.encode_rle_masklet(dev(pats[codes]))
    assert [g["counts"] for g in got] == [table[c] for c in codes]
