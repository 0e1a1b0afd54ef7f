"""The threshold sweep without a GPU: the symbol and its declarations, the argument checks of sola_mask_nested_counts (refused
before any launch), seg_utils.sweep_levels against the brute-force rule, and the numpy yardstick of tests/sweep_cases.py
against K separate ORs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sweep_cases as sc  # noqa: E402
from sola_amd import _lib, seg_utils  # noqa: E402
from sola_amd._lib import SolaError  # noqa: E402


def test_symbol_is_exported_and_declared():
    L = _lib.lib()
    name = "sola_mask_nested_counts"
    assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "sola_hip.h")).read()
    assert f"int {name}(" in header
    assert "#define SOLA_NESTED_MAX_LEVELS 16\n" in header


def _err():
    return _lib.lib().sola_last_error().decode()


def _call(bits=0x4000, stride=44, M=3, T=2, poff=0x1000, pidx=0x2000, lend=0x3000, K=5, goff=0x5000, gidx=0x6000, E=4,
          counts=0x8000):
    return _lib.lib().sola_mask_nested_counts(bits, stride, M, T, poff, pidx, lend, K, goff, gidx, E, counts, None)


@pytest.mark.parametrize("kw", [{"bits": None}, {"poff": None}, {"pidx": None}, {"lend": None}, {"goff": None}, {"gidx": None},
                                {"counts": None}, {"K": 0}, {"K": -3}, {"E": 0}, {"E": -1}, {"T": 0}, {"T": -2}, {"M": -1},
                                {"stride": 0}, {"stride": -4}, {"stride": 42}, {"stride": 1 << 26}, {"bits": 0x4004},
                                {"bits": 0x4008}, {"E": 1 << 16, "T": 1 << 15}])
def test_nested_counts_argument_errors_without_gpu(kw):
    _lib.lib().sola_tune(b"no_such_key", 0)  # leaves another text in sola_last_error
    before = _err()
    assert _call(**kw) < 0
    text = _err()
    assert text and text != before and text.startswith("mask_nested_counts:")


def _check_levels(probs, thresholds):
    probs = np.asarray(probs, np.float32)
    order, level_end, perm = seg_utils.sweep_levels(probs, thresholds)
    K = len(thresholds)
    want = sc.sweep_levels_ref(probs, thresholds)
    assert level_end.dtype == np.int32 and level_end.shape == (K,) and len(perm) == K
    assert sorted(perm.tolist()) == list(range(K))
    th32 = np.asarray(thresholds, np.float32)
    by_level = np.empty(K, np.float32)
    by_level[perm] = th32  # level perm[j] is the caller's threshold j
    assert np.all(np.diff(by_level) <= 0)  # the levels are the thresholds sorted descending
    assert np.all(np.diff(level_end) >= 0) and (K == 0 or level_end[-1] == len(order))
    assert len(set(order.tolist())) == len(order)
    for j in range(K):
        prefix = order[:level_end[perm[j]]].tolist()
        assert set(prefix) == want[j] and len(prefix) == len(want[j])
    # stable: within the tracks that enter at one level, the index order
    ends = [0] + level_end.tolist()
    for a, b in zip(ends, ends[1:]):
        assert order[a:b].tolist() == sorted(order[a:b].tolist())
    return order, level_end, perm


def test_sweep_levels_random_scores_unsorted_and_duplicated_thresholds():
    rng = np.random.default_rng(3)
    for n in (1, 7, 40):
        probs = rng.random(n).astype(np.float32)
        _check_levels(probs, [0.5, 0.9, 0.1, 0.5, 0.3, 0.9])
        _check_levels(probs, rng.random(19).tolist())
        _check_levels(probs, [0.4])


def test_sweep_levels_scores_equal_to_a_threshold_are_not_selected():
    order, level_end, perm = _check_levels([0.5, 0.25, 0.75, 0.5], [0.25, 0.5, 0.75])
    assert level_end.tolist() == [0, 1, 3] and order.tolist() == [2, 0, 3] and perm.tolist() == [2, 1, 0]


def test_sweep_levels_threshold_that_is_no_float32_value():
    p = np.float32(0.1)
    assert float(p) > 0.1  # in double the float32 score exceeds the threshold; in float32 they are equal
    order, level_end, _ = _check_levels([p, np.nextafter(p, np.float32(1)), np.nextafter(p, np.float32(0))], [0.1])
    assert order.tolist() == [1] and level_end.tolist() == [1]


def test_sweep_levels_thresholds_zero_and_one():
    order, level_end, perm = _check_levels([0.0, 1.0, 0.5, 1e-30], [0.0, 1.0])
    assert perm.tolist() == [1, 0] and level_end.tolist() == [0, 3] and order.tolist() == [1, 2, 3]


def test_sweep_levels_without_tracks():
    order, level_end, perm = _check_levels([], [0.5, 0.1, 0.9])
    assert len(order) == 0 and level_end.tolist() == [0, 0, 0] and perm.tolist() == [1, 2, 0]


def _numpy_counts(planes, T, pred_sets, gt_sets):
    """The restatement of tests/test_gpu_jf.py (numpy_counts), for one selection."""
    M = planes.shape[0] // T
    pl = planes.reshape(M, T, -1)
    out = np.zeros((len(pred_sets), T, 3), np.int64)
    for e, (ps, gs) in enumerate(zip(pred_sets, gt_sets)):
        p = np.bitwise_or.reduce(pl[list(ps)], axis=0) if len(ps) else np.zeros_like(pl[0])
        g = np.bitwise_or.reduce(pl[list(gs)], axis=0) if len(gs) else np.zeros_like(pl[0])
        bc = lambda a: np.unpackbits(a.view(np.uint8), axis=1).sum(1)  # noqa: E731
        out[e] = np.stack([bc(p & g), bc(p), bc(g)], 1)
    return out


def test_numpy_nested_counts_equals_separate_evaluations():
    rng = np.random.default_rng(5)
    M, T, stride = 4, 2, 4
    planes = rng.integers(0, 1 << 32, size=(M * T, stride), dtype=np.uint64).astype(np.uint32)
    pred_lists = [[2, 0, 3], [1, 1, 0], [], [3]]
    level_ends = [[0, 1, 3], [2, 1, 9], [0, 0, 0], [1, 1, 1]]  # a decreasing and a too-long entry: clamped to [2, 2, 3]
    gt_sets = [[1], [0, 2], [3], []]
    got = sc.numpy_nested_counts(planes, T, pred_lists, level_ends, gt_sets)
    assert got.shape == (4, 3, T, 3)
    assert sc.prefix_ends(level_ends[1], 3) == [2, 2, 3]
    for k, prefixes in enumerate([[[], [1, 1], [], [3]], [[2], [1, 1], [], [3]], [[2, 0, 3], [1, 1, 0], [], [3]]]):
        np.testing.assert_array_equal(got[:, k], _numpy_counts(planes, T, prefixes, gt_sets))
    assert got[0, 0, :, 1].sum() == 0 and got[0, 2, :, 1].sum() > got[0, 1, :, 1].sum() > 0
    ignored = sc.numpy_nested_counts(planes, T, [[2, 7, -1, 0, 3]], [[0, 3, 5]], [[1, 4]])  # ids outside [0, M)
    np.testing.assert_array_equal(ignored[0, 1], got[0, 1])
    np.testing.assert_array_equal(ignored[0, 2], got[0, 2])


def test_masklet_sweep_counts_refuses_bad_arguments_before_the_gpu():
    rle = [[{"size": [2, 2], "counts": [4]}]]
    with pytest.raises(SolaError, match="no thresholds"):
        seg_utils.masklet_sweep_counts(rle, [[0]], [[0.5]], [], [[0]], "cuda")
    with pytest.raises(SolaError, match="1 tracks but 2 scores"):
        seg_utils.masklet_sweep_counts(rle, [[0]], [[0.5, 0.5]], [0.5], [[0]], "cuda")
    with pytest.raises(SolaError, match="outside the 1 masklets"):
        seg_utils.masklet_sweep_counts(rle, [[1]], [[0.5]], [0.5], [[0]], "cuda")
    c, b = seg_utils.masklet_sweep_counts([[None, None]], [[0]], [[0.9]], [0.5, 0.1], [[0]], "cuda", boundary=True)  # no frame size known
    assert tuple(c.shape) == (1, 2, 2, 3) and tuple(b.shape) == (1, 2, 2, 4) and not c.any() and not b.any()
    assert tuple(seg_utils.masklet_sweep_counts(rle, [], [], [0.5], [], "cuda").shape) == (0, 1, 1, 3)
