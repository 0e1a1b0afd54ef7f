"""Baseline JPEG decode on the GPU: frames.decode_jpeg against np.asarray(Image.open(f).convert("RGB")) under torch.equal, every
case at the default subsequence size and at the smallest one; the coefficient buffer against tests/jpeg_cases.py's sequential
restatement; run-to-run and stream-to-stream bits; load_video_frames(jpeg_decoder="gpu") against the default; damaged scans between
sentinel fences.  Pillow's encoder makes every file here.  Everything is exact: there is no tolerance in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import jpeg_cases as jc  # noqa: E402
from sola_amd import _lib, frames  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402

pytestmark = pytest.mark.gpu

SUBSEQS = (0, jc.SUBSEQ_MIN)
SENTINEL = 0xA5
FENCE = 4096


def same_as_pillow(datas):
    want = torch.from_numpy(np.stack([jc.pillow_rgb(d) for d in datas]))
    for s in SUBSEQS:
        got = frames.decode_jpeg(datas, subseq_bytes=s)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.cpu(), want), f"subseq_bytes {s}"


def n_subsequences(data, s):
    return len(jc.subsequence_starts(jc.parse(data), s or jc.SUBSEQ_DEFAULT))


def test_constants_are_the_librarys():
    hdr = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert f"#define SOLA_JPEG_SUBSEQ_MIN {jc.SUBSEQ_MIN}\n" in hdr and f"#define SOLA_JPEG_SUBSEQ_DEFAULT {jc.SUBSEQ_DEFAULT}\n" in hdr
    assert (frames.JPEG_SUBSEQ_MIN, frames.JPEG_SUBSEQ_DEFAULT) == (jc.SUBSEQ_MIN, jc.SUBSEQ_DEFAULT)
    src = open(os.path.join(ROOT, "sola_amd", "csrc", "jpeg.hip")).read()
    assert f"#define SOLA_JPEG_NT {jc.THREADS_PER_BLOCK} " in src


def test_one_grey_block():
    same_as_pillow([jc.case(8, 8, "grey", 75, "noise")])


def test_single_partial_mcu():
    same_as_pillow([jc.case(17, 13, "4:2:0", 75, "noise")])
    same_as_pillow([jc.case(13, 11, "4:2:0", 75, "smooth")])  # one MCU, cut on both axes


@pytest.mark.parametrize("sampling", jc.SAMPLINGS)
@pytest.mark.parametrize("quality", [30, 95])
def test_samplings_with_optimised_tables(sampling, quality):
    same_as_pillow([jc.case(40, 52, sampling, quality, "noise", "optimize")])


@pytest.mark.parametrize("interval", [1, 3])
def test_restart_intervals(interval):
    data = jc.case(33, 47, "4:2:0", 75, "noise", f"restart{interval}")
    assert frames.jpeg_info(data)["restart_interval"] == interval and jc.parse(data)["n_segments"] == -(-9 // interval)
    same_as_pillow([data])
    same_as_pillow([jc.case(33, 47, "4:2:2", 95, "smooth", f"restart{interval}+optimize")])


def test_narrow_planes_take_replication():
    # cropped chroma planes of 1 and 2 samples: libjpeg replicates instead of the triangle filter
    for (w, h) in [(3, 5), (4, 4), (2, 17), (1, 1)]:
        for sampling in ("4:2:2", "4:2:0"):
            same_as_pillow([jc.case(w, h, sampling, 90, "noise")])


def test_noise_crosses_workgroups():
    data = jc.case(256, 192, "4:2:0", 95, "noise")
    plan = jc.parse(data)
    for s in SUBSEQS:  # the synchronisation crosses workgroups at either size ...
        assert n_subsequences(data, s) > jc.THREADS_PER_BLOCK
    # ... and an 8x8 block spans several subsequences at the smallest
    assert n_subsequences(data, jc.SUBSEQ_MIN) > 2 * plan["n_blocks"]
    same_as_pillow([data])


def test_smooth_has_many_blocks_per_subsequence():
    data = jc.case(256, 192, "4:2:0", 30, "smooth")
    assert jc.parse(data)["n_blocks"] > 8 * n_subsequences(data, 0)
    same_as_pillow([data])


def test_stuffed_zero_on_a_subsequence_boundary():
    data, plan, hits = jc.stuffed_case(jc.SUBSEQ_MIN)
    scan = data[plan["scan_begin"]:plan["scan_end"]]
    assert scan.count(b"\xff\x00") > 0
    starts = jc.subsequence_starts(plan, jc.SUBSEQ_MIN)
    assert any(scan[b - 1] == 0xFF and scan[b] == 0x00 for b in starts if b > 0) and hits
    same_as_pillow([data])


def test_scan_shorter_than_a_subsequence():
    data = jc.case(8, 8, "4:2:0", 30, "smooth")
    plan = jc.parse(data)
    assert plan["scan_end"] - plan["scan_begin"] < jc.SUBSEQ_MIN
    same_as_pillow([data])


def test_batch_with_tables_per_frame():
    datas = [jc.case(40, 52, "4:2:0", q, c, "optimize", seed=i) for i, (q, c) in enumerate([(30, "noise"), (95, "smooth"), (75, "noise"), (100, "noise"), (50, "smooth")])]
    assert len({bytes(np.concatenate([h[3] for h in jc.parse(d)["huff"]])) for d in datas}) > 1  # the tables do differ
    same_as_pillow(datas)


def test_frames_of_different_geometry_are_refused():
    with pytest.raises(SolaError, match="differs from frame 0"):
        frames.decode_jpeg([jc.case(40, 52, "4:2:0"), jc.case(40, 52, "4:2:2")])
    with pytest.raises(SolaError, match="progressive"):
        frames.decode_jpeg([jc.encode(jc.image(16, 16, "noise", 0), progressive=True)])
    with pytest.raises(SolaError, match="subseq_bytes"):
        frames.decode_jpeg([jc.case(16, 16)], subseq_bytes=24)


def decode_chunk(datas, s, want=None):
    parsed = [frames.jpeg_parse(d) for d in datas]
    return frames._jpeg_decode_chunk(parsed, datas, torch.device("cuda", torch.cuda.current_device()), s, want=want)


def test_coefficients_are_the_restatements():
    datas = [jc.case(40, 52, "4:2:0", 75, "noise", "restart3"), jc.case(40, 52, "4:2:0", 95, "smooth", "optimize")]
    for s in SUBSEQS:
        for t, d in enumerate(datas):
            _, err, _, coef = decode_chunk(datas, s, want=t)
            assert err == [0, 0]
            assert np.array_equal(coef, jc.decode_coefficients(d)), (s, t)


def test_same_bits_on_every_run_and_stream():
    datas = [jc.case(256, 192, "4:2:0", 95, "noise"), jc.case(256, 192, "4:2:0", 30, "smooth")]
    first, err, rounds, coef = decode_chunk(datas, jc.SUBSEQ_MIN, want=0)
    first = first.clone()
    assert err == [0, 0] and rounds >= 2
    again, _, rounds2, coef2 = decode_chunk(datas, jc.SUBSEQ_MIN, want=0)
    assert torch.equal(first, again) and np.array_equal(coef, coef2) and rounds2 == rounds
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other, _, rounds3, coef3 = decode_chunk(datas, jc.SUBSEQ_MIN, want=0)
        side.synchronize()
    assert torch.equal(first, other) and np.array_equal(coef, coef3) and rounds3 == rounds


def test_load_video_frames_gpu_mode(tmp_path):
    for i in range(6):
        arr = jc.image(72, 56, "smooth" if i % 2 else "noise", 40 + i)
        data = jc.encode(arr, 90, "4:2:0", "plain", progressive=True) if i == 3 else jc.encode(arr, 90, "4:2:0", "optimize" if i == 4 else "plain")
        (tmp_path / f"{i}.jpg").write_bytes(data)
    with pytest.raises(SolaError, match="progressive"):
        frames.jpeg_info((tmp_path / "3.jpg").read_bytes())  # that frame takes the PIL reader
    want, H, W = frames.load_video_frames(str(tmp_path), 48, False)
    got, H2, W2 = frames.load_video_frames(str(tmp_path), 48, False, jpeg_decoder="gpu")
    assert (H, W) == (H2, W2) == (56, 72) and tuple(got.shape) == (6, 3, 48, 48)
    assert torch.equal(got, want)
    with pytest.raises(SolaError, match="jpeg_decoder"):
        frames.load_video_frames(str(tmp_path), 48, False, jpeg_decoder="nvjpeg")


def fenced(nbytes):
    """(whole buffer, the nbytes in the middle, 256-byte aligned), sentinel everywhere."""
    buf = torch.full((nbytes + 2 * FENCE,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[FENCE:FENCE + nbytes]


@pytest.mark.parametrize("damage", ["truncated", "bit-flipped"])
def test_damaged_scan_stays_inside_its_buffers(damage):
    """A kernel that range-checks every access by construction, shown a scan the parser accepts but no encoder wrote: the call returns,
    the fences around the output and the scratch are intact, and the error word is set or the pixels merely differ."""
    good = jc.case(64, 48, "4:2:0", 90, "noise", "restart4")
    plan = jc.parse(good)
    if damage == "truncated":
        bad = good[:plan["scan_begin"] + (plan["scan_end"] - plan["scan_begin"]) * 2 // 3]
    else:
        rng = np.random.default_rng(5)
        while True:  # a flip inside the scan that the parser still accepts (no marker made or destroyed)
            b = bytearray(good)
            at = int(rng.integers(plan["scan_begin"] + 8, plan["scan_end"] - 8))
            b[at] ^= 1 << int(rng.integers(0, 8))
            try:
                frames.jpeg_parse(bytes(b))
            except SolaError:
                continue
            bad = bytes(b)
            break
    parsed = [frames.jpeg_parse(bad)]
    dev = torch.device("cuda", torch.cuda.current_device())
    for s in SUBSEQS:
        chunk = frames._JpegChunk(parsed, [bad])
        blob = chunk.blob.to(dev)
        need = _lib.lib().sola_jpeg_scratch_bytes(chunk.plans, 1, s)
        assert need > 0
        out_all, out = fenced(48 * 64 * 3)
        scratch_all, scratch = fenced(need)
        err, rounds = (C.c_int32 * 1)(), C.c_int32()
        base = blob.data_ptr()
        _lib.check(_lib.lib().sola_jpeg_decode(C.c_void_p(base + chunk.off_scan), chunk.scan_bytes, C.c_void_p(base + chunk.off_segs), chunk.n_segs,
                                               chunk.plans, C.c_void_p(base), 1, s, _lib.ptr(out), _lib.ptr(scratch), need, err, C.byref(rounds),
                                               _lib.current_stream(dev)), "sola_jpeg_decode")
        torch.cuda.synchronize()
        for whole, n in ((out_all, out.numel()), (scratch_all, need)):
            assert bool((whole[:FENCE] == SENTINEL).all()) and bool((whole[FENCE + n:] == SENTINEL).all())
        pixels = out.view(48, 64, 3).cpu().numpy()
        assert err[0] != 0 or not np.array_equal(pixels, jc.pillow_rgb(good))
        if damage == "truncated":
            assert err[0] & 8  # a segment that ends before its last block
