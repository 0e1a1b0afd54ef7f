"""The PNG selection path's host side without a GPU: the restatement of png_select_cases.py pinned against PIL and png_cases
before test_gpu_png_select.py uses it as the yardstick; the argument checks of sola_planes_cm_to_rm and
sola_png_deflate_sizes_select, which refuse before any launch; --sweep_thresholds on inference.py's side."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import png_cases as pc  # noqa: E402
import png_select_cases as ps  # noqa: E402
from sola_amd import _lib  # noqa: E402

FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below is refused before it launches anything
ODD = ctypes.c_void_p((1 << 20) + 8)
BIG = 1 << 62


def _unpack(planes, n_bits):
    return np.unpackbits(planes.view(np.uint8), axis=1, bitorder="little")[:, :n_bits]


@pytest.mark.parametrize("h,w", ps.SIZES, ids=[f"{h}x{w}" for h, w in ps.SIZES])
def test_plane_layouts_hold_the_pixels_where_the_header_says(h, w):
    masks, _ = ps.tracks(h, w)
    flat = masks.reshape(-1, h, w)
    cm, rm = ps.cm_planes(flat), ps.rm_planes(flat)
    words = ps.round4(ps.mask_words(h, w))
    assert cm.shape == rm.shape == (len(flat), words) and cm.dtype == rm.dtype == np.dtype("<u4")
    for n in (0, len(flat) - 1):
        for y, x in {(0, 0), (h - 1, w - 1), (h // 2, w // 3), (0, w - 1), (h - 1, 0)}:
            pos_cm, pos_rm = x * h + y, y * w + x
            assert (int(cm[n, pos_cm // 32]) >> (pos_cm % 32)) & 1 == flat[n, y, x]
            assert (int(rm[n, pos_rm // 32]) >> (pos_rm % 32)) & 1 == flat[n, y, x]
    # every pixel, and zero tail and pad bits
    np.testing.assert_array_equal(_unpack(rm, h * w).reshape(-1, h, w), flat)
    np.testing.assert_array_equal(_unpack(cm, h * w).reshape(-1, w, h).transpose(0, 2, 1), flat)
    assert not np.unpackbits(rm.view(np.uint8), axis=1, bitorder="little")[:, h * w:].any()
    assert not np.unpackbits(cm.view(np.uint8), axis=1, bitorder="little")[:, h * w:].any()


@pytest.mark.parametrize("K", [1, 3, 16])
def test_nested_streams_open_with_pil_to_the_ors(K):
    h, w = 33, 95
    masks, _ = ps.tracks(h, w)
    lists = ps.selection_lists()
    ends = ps.level_ends(lists, K)
    streams = ps.select_streams(masks, lists, ends)
    assert len(streams) == len(lists) * K * ps.T
    for e, lst in enumerate(lists):
        clamped = ps.clamp_ends(ends[e], len(lst))
        assert clamped == sorted(clamped) and clamped[-1] <= len(lst)
        for k in range(K):
            want = np.zeros((ps.T, h, w), np.uint8)
            for m in lst[:clamped[k]]:
                if 0 <= m < ps.M:
                    want |= masks[m]
            for t in range(ps.T):
                s = streams[(e * K + k) * ps.T + t]
                assert s == pc.zlib_stream(want[t])
                assert ps.adler_of(s) == ps.raw_adler(want[t])
                img = Image.open(io.BytesIO(pc.png_wrap(s, h, w)))
                assert img.mode == "L"
                np.testing.assert_array_equal(np.array(img), want[t] * 255)
    assert not ps.nested_ors(masks, lists[0], ends[0]).any()  # the empty list
    if K == 1:  # one level: the whole list, ids outside [0, M) ignored
        np.testing.assert_array_equal(ps.nested_ors(masks, lists[4], ends[4])[0], masks[3] | masks[0] | masks[2])


def _refused(status, *words):
    assert status == -1
    msg = _lib.lib().sola_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_planes_cm_to_rm_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    cmw, rmw = L.sola_jf_plane_words(8, 8), ps.round4(L.sola_mask_words(8, 8))
    _refused(L.sola_planes_cm_to_rm(None, cmw, 2, 8, 8, FAKE, rmw, None), "null")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw, 2, 8, 8, None, rmw, None), "null")
    for n, h, w in [(0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, -3)]:
        _refused(L.sola_planes_cm_to_rm(FAKE, BIG, n, h, w, FAKE, BIG, None), "bad sizes")
    for h, w in [(65536, 32768), (1, 400000)]:  # h*w >= 2^31; a row that does not fit the transpose's LDS tile
        _refused(L.sola_planes_cm_to_rm(FAKE, 1 << 40, 1, h, w, FAKE, 1 << 40, None), "too large")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw - 4, 2, 8, 8, FAKE, rmw, None), "words_stride_cm")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw + 2, 2, 8, 8, FAKE, rmw, None), "multiple of 4")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw, 2, 8, 8, FAKE, rmw - 4, None), "words_stride_rm")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw, 2, 8, 8, FAKE, rmw + 1, None), "multiple of 4")
    _refused(L.sola_planes_cm_to_rm(ODD, cmw, 2, 8, 8, FAKE, rmw, None), "aligned")
    _refused(L.sola_planes_cm_to_rm(FAKE, cmw, 2, 8, 8, ODD, rmw, None), "aligned")


def test_sizes_select_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    h, w, T, K, E = 8, 8, 2, 3, 2
    words = ps.round4(L.sola_mask_words(h, w))
    ok = L.sola_png_deflate_scratch_bytes(E * K * T, h, w)

    def call(bits=FAKE, stride=words, n_masks=4, T=T, h=h, w=w, off=FAKE, idx=FAKE, lend=FAKE, K=K, E=E, boff=FAKE, adler=FAKE, sc=FAKE,
             nb=ok):
        return L.sola_png_deflate_sizes_select(bits, stride, n_masks, T, h, w, off, idx, lend, K, E, boff, adler, sc, nb, None)

    for name in ("bits", "off", "idx", "boff", "adler", "sc"):
        _refused(call(**{name: None}), "null")
    _refused(call(lend=None), "null")           # a null level_end needs K == 1 ...
    _refused(call(lend=None, K=1, nb=0), "scratch")  # ... and with K == 1 it is accepted: the next check speaks
    for bad in (dict(K=0), dict(E=0), dict(T=0), dict(K=-1), dict(E=-2), dict(T=-1), dict(h=0), dict(w=0), dict(K=17)):
        _refused(call(nb=BIG, **bad), "bad sizes")
    assert L.sola_png_deflate_scratch_bytes(1, 8, 8) > 0 and K <= 16
    _refused(call(E=1 << 20, K=16, T=1 << 7, nb=BIG), "too large")       # E*K*T = 2^31
    for hh, ww in [(65536, 32768), (32768, 65535)]:                      # h*(w+1) >= 2^31 (h*w alone is below it in the second)
        _refused(call(h=hh, w=ww, stride=1 << 40, nb=BIG), "too large")
    _refused(call(stride=words + 2), "multiple of 4")
    _refused(call(stride=words - 4), "words_stride")
    _refused(call(bits=ODD), "aligned")
    _refused(call(sc=ctypes.c_void_p((1 << 20) + 4)), "aligned")
    _refused(call(nb=ok - 1), "scratch")


def test_existing_png_entries_still_refuse_elem_type_3_and_null_masks():
    L = _lib.lib()
    ok = L.sola_png_deflate_scratch_bytes(2, 8, 8)
    _refused(L.sola_png_deflate_sizes(FAKE, 3, 2, 8, 8, FAKE, FAKE, FAKE, ok, None), "elem_type")
    _refused(L.sola_png_deflate_write(FAKE, 3, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, ok, None), "elem_type")
    _refused(L.sola_png_deflate_write(None, 0, 2, 8, 8, FAKE, FAKE, FAKE, FAKE, ok, None), "null")


def test_sweep_thresholds_reach_the_config_only_when_given():
    from sola_amd.config import load_configs
    root = os.path.join(os.path.dirname(HERE), "configs")
    base = ["--config", "mevis/default", "--eval_weight_epoch", "1"]
    cfg = load_configs("inference", base + ["--sweep_thresholds", "0.3,0.5,0.7"], config_root=root)
    assert cfg["sweep_thresholds"] == "0.3,0.5,0.7"
    assert "sweep_thresholds" not in load_configs("inference", base, config_root=root)
    assert "sweep_thresholds" not in load_configs("inference", base + ["--gpu_png", "true"], config_root=root)
    assert load_configs("inference", base + ["--sweep_thresholds", "0.25"], config_root=root)["sweep_thresholds"] == 0.25


def test_threshold_directory_names_follow_load_configs():
    from sola_amd.config import load_configs, sweep_dir_name
    assert [sweep_dir_name(t) for t in (0.5, 0.25, 1.0, 0.0)] == ["05", "025", "10", "00"]
    root = os.path.join(os.path.dirname(HERE), "configs")
    for t in (0.5, 0.25, 1.0):
        cfg = load_configs("inference", ["--config", "mevis/default", "--eval_weight_epoch", "2", "--eval_pred_threshold", str(t)],
                           config_root=root)
        parts = cfg["results"]["test_output_dir"].split(os.sep)
        assert parts[-2:] == [f"pred_threshold_{sweep_dir_name(t)}", "epoch_2"]


def test_parse_sweep_thresholds_is_one_function_in_both_places():
    import eval as eval_entry
    import inference
    from sola_amd import config
    assert eval_entry.parse_sweep_thresholds is config.parse_sweep_thresholds is inference.parse_sweep_thresholds
    assert config.parse_sweep_thresholds(None) is None
    assert config.parse_sweep_thresholds("0.1, 0.3,0.5") == [0.1, 0.3, 0.5]
    assert config.parse_sweep_thresholds(0.5) == [0.5]
    with pytest.raises(ValueError, match="needs a value"):
        config.parse_sweep_thresholds(True)
    with pytest.raises(ValueError, match="outside"):
        config.parse_sweep_thresholds("0.5,1.5")
    with pytest.raises(ValueError, match="not a number"):
        config.parse_sweep_thresholds("0.5,x")


def test_seg_utils_entry_points_exist_and_refuse_what_cannot_be_sized():
    from sola_amd import seg_utils
    from sola_amd._lib import SolaError
    for name in ("planes_cm_to_rm", "encode_png_selections", "encode_png_sweep"):
        assert callable(getattr(seg_utils, name))
    with pytest.raises(SolaError, match="no size"):  # every frame missing: refused before anything touches a device
        seg_utils.encode_png_selections([[None, None]], [[0]], "cuda")
    with pytest.raises(SolaError, match="outside"):
        seg_utils.encode_png_selections([[None, None]], [[1]], "cuda")
    with pytest.raises(SolaError, match="no thresholds"):
        seg_utils.encode_png_sweep([[None]], [[0]], [[0.5]], [], "cuda")
