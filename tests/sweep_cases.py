"""Numpy restatements for the threshold-sweep tests: the nested counts of sola_mask_nested_counts on dense planes, and the
selection rule of seg_utils.sweep_levels by brute force."""
import numpy as np


def _popc(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=1).sum(1).astype(np.int64)


def prefix_ends(level_end, n):
    """end(e, -1) = 0, end(e, k) = min(max(level_end[k], end(e, k - 1)), n)."""
    out, prev = [], 0
    for v in level_end:
        prev = min(max(int(v), prev), n)
        out.append(prev)
    return out


def numpy_nested_counts(planes, T, pred_lists, level_ends, gt_sets):
    """planes uint32 [M*T, stride] (mask m at frame t = row m*T + t); pred_lists[e] the ordered candidate ids, level_ends[e] its K
    prefix lengths as given (clamped here), gt_sets[e] the GT ids; ids outside [0, M) are ignored -> int64 [E, K, T, 3]."""
    M = planes.shape[0] // T
    pl = planes.reshape(M, T, -1)
    zero = np.zeros_like(pl[0]) if M else np.zeros((T, planes.shape[1]), planes.dtype)
    K = len(level_ends[0])
    out = np.zeros((len(pred_lists), K, T, 3), np.int64)

    def union(ids):
        ids = [int(i) for i in ids if 0 <= int(i) < M]
        return np.bitwise_or.reduce(pl[ids], axis=0) if ids else zero

    for e, (ps, le, gs) in enumerate(zip(pred_lists, level_ends, gt_sets)):
        g = union(gs)
        for k, end in enumerate(prefix_ends(le, len(ps))):
            p = union(ps[:end])
            out[e, k] = np.stack([_popc(p & g), _popc(p), _popc(g)], 1)
    return out


def sweep_levels_ref(probs, thresholds):
    """Per threshold (the caller's order) the set {i : float32(p_i) > float32(theta)}."""
    return [{i for i, p in enumerate(probs) if np.float32(p) > np.float32(th)} for th in thresholds]
