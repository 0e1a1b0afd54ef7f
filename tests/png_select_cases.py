"""sola_planes_cm_to_rm and sola_png_deflate_sizes_select (include/sola_hip.h) restated in numpy: the two plane layouts from
decoded masks, the nested ORs of a selection with the level rules of sola_mask_nested_counts, and their PNG streams through
png_cases.  Shared by test_png_select_cpu.py (which pins this restatement against PIL) and test_gpu_png_select.py (which uses it as
the yardstick)."""
import zlib

import numpy as np

import jf_cases as jc
import masklet_cases as mc
import png_cases as pc

# (h, w): w + 1 = 2, 65, 96, 64, 32, 201, 130; (100, 200) has two PNG workgroups per frame (20100 raw bytes > 16384), (130, 31)
# and (100, 200) more than one workgroup of 64 rows in the transpose, (65, 129) a last workgroup of one row
SIZES = [(1, 1), (40, 64), (33, 95), (64, 63), (130, 31), (7, 200), (100, 200), (65, 129)]
M, T = 6, 3
MISSING = {1: (0,), 4: (1, 2)}  # track -> frames without an RLE dict


def round4(n):
    return (n + 3) // 4 * 4


def mask_words(h, w):
    return (h * w + 31) // 32


def _planes(flat, stride):
    """[n, h*w] {0,1} in the layout's pixel order -> uint32 [n, stride]: bit j of word i is position 32*i + j, the rest zero."""
    n = flat.shape[0]
    by = np.packbits(flat.astype(np.uint8), axis=1, bitorder="little")
    out = np.zeros((n, stride * 4), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u4")


def cm_planes(masks, stride=None):
    """[n,h,w] masks -> the column-major planes of sola_rle_pack_cm: position x*h + y."""
    n, h, w = masks.shape
    return _planes(np.asarray(masks != 0).transpose(0, 2, 1).reshape(n, -1), round4(mask_words(h, w)) if stride is None else stride)


def rm_planes(masks, stride=None):
    """[n,h,w] masks -> the row-major planes of sola_mask_pack: position y*w + x."""
    n, h, w = masks.shape
    return _planes(np.asarray(masks != 0).reshape(n, -1), round4(mask_words(h, w)) if stride is None else stride)


def tracks(h, w, special=False):
    """(masks [M,T,h,w] uint8 with the missing frames zeroed, [M RLE lists with those frames None]).  ``special``: track 2 is
    all ones in every frame and track 3 all zeros."""
    # (blob_masklet's last three frames are empty, full and noise: every track takes T frames of six, a different mix each)
    masks = np.stack([np.asarray(mc.blob_masklet(6, h, w, 300 + 7 * m + h + w) != 0).astype(np.uint8)[[(m + 2 * t) % 6 for t in range(T)]]
                      for m in range(M)])
    if special:
        masks[2] = 1
        masks[3] = 0
    rles = []
    for m in range(M):
        rles.append(jc.rle_list(masks[m], missing=MISSING.get(m, ())))
        for t in MISSING.get(m, ()):
            masks[m, t] = 0
    return masks, rles


def selection_lists():
    """E = 5 lists over M = 6 tracks: empty, one id, all ids, repeated ids, one with ids outside [0, M)."""
    return [[], [4], [0, 1, 2, 3, 4, 5], [5, 1, 5, 5, 1, 0], [3, 17, 0, -2, 2]]


def level_ends(lists, K):
    """[E][K] prefix ends: spread over the list, with a decreasing and a too-long entry that the device has to clamp."""
    out = []
    for e, lst in enumerate(lists):
        n = len(lst)
        ends = [(n * (k + 1) + K - 1) // K for k in range(K)] if K > 1 else [n]
        if K >= 3:
            ends[1] = 0 if e % 2 else ends[1]       # decreasing: clamped up to the level before
            ends[K - 1] = n + 5 if e >= 2 else n    # too long: clamped to the list
        out.append(ends)
    return out


def clamp_ends(ends, n):
    prev, out = 0, []
    for v in ends:
        prev = min(max(v, prev), n)
        out.append(prev)
    return out


def nested_ors(masks, lst, ends):
    """[K,T,h,w]: level k = OR of masks[m] over the valid ids of lst[:end_k], the ends clamped as the device clamps them."""
    m_all = masks.shape[0]
    out = []
    for end in clamp_ends(ends, len(lst)):
        acc = np.zeros(masks.shape[1:], np.uint8)
        for m in lst[:end]:
            if 0 <= m < m_all:
                acc |= masks[m]
        out.append(acc)
    return np.stack(out)


def select_streams(masks, lists, ends):
    """The zlib streams in stream order (e*K + k)*T + t, and their Adler-32 values."""
    streams = []
    for lst, e_ends in zip(lists, ends):
        for level in nested_ors(masks, lst, e_ends):
            streams += [pc.zlib_stream(f) for f in level]
    return streams


def adler_of(stream):
    return int.from_bytes(stream[-4:], "big")


def raw_adler(mask):
    return zlib.adler32(pc.raw_stream(mask))
