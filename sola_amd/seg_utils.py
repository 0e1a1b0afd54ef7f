"""Drop-in for the IoU functions of ``track_generation/seg_utils.py`` (:109-142) and the greedy de-dup loop of
``generate_tokens_grid.py:252-278`` / ``generate_tokens_gdino.py:274-300`` on libsola_hip.so.

Masks are torch CUDA tensors, uint8 or float32 with values {0,1}.  Counts are exact int64; the ratio is a python
float division exactly as in the reference, so ``iou > miou_thresh`` decisions are bit-identical."""
from __future__ import annotations

import struct
import zlib

import torch

from ._lib import SolaError, check, current_stream, lib, ptr, require_cuda


def _elem_type(t):
    if t.dtype == torch.uint8 or t.dtype == torch.bool:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise SolaError(f"masks must be uint8/bool or float32, got {t.dtype}")


def _mask_kind(t, logits, who=None):
    """The library's element kind of mask tensor ``t``: 0 uint8 / bool, 1 float32 (set where != 0), 2 float32 logits (set where > 0)."""
    if logits and t.dtype != torch.float32:
        raise SolaError("logits must be float32" if who is None else f"{who}: logits must be float32, got {t.dtype}")
    return 2 if logits else _elem_type(t)


_SCRATCH = {}


def _stream_scratch(name, dev, nbytes, dtype=torch.uint8, floor=0):
    """Kernel ``name``'s scratch of at least ``nbytes`` bytes (and ``floor`` elements of ``dtype``), reused from call to call per
    device and stream: calls on one stream are ordered, and an allocation can cost as much as the kernel it serves."""
    key = (name, dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() * buf.element_size() < nbytes:
        buf = _SCRATCH[key] = torch.empty(max(-(-nbytes // dtype.itemsize), floor), device=dev, dtype=dtype)
    return buf


def _prep(t):
    require_cuda(t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.contiguous()


def pack_masks(masks, out_hw=None):
    """masks [n,h,w] -> (bits int32 [n,words], area int64 [n]) at resolution ``out_hw`` (nearest resample, as
    F.interpolate(mode='nearest') in generate_tokens_grid.py:272) or the native one."""
    masks = _prep(masks)
    n, h, w = masks.shape
    H, W = (h, w) if out_hw is None else out_hw
    words = lib().sola_mask_words(H, W)
    bits = torch.empty((n, words), device=masks.device, dtype=torch.int32)
    area = torch.empty((n,), device=masks.device, dtype=torch.int64)
    check(lib().sola_mask_pack(ptr(masks), _elem_type(masks), n, h, w, H, W, ptr(bits), ptr(area),
                               current_stream(masks.device)), "sola_mask_pack")
    return bits, area


def pair_counts(a_bits, a_area, b_bits, b_area, T=1, a_frame=None):
    """inter/union [P,R] from packed masks; ``a_frame`` [R] int32 selects, per column, the frame of each of the P
    masklets of T frames held in ``a_bits`` [P*T, words]."""
    P = a_bits.shape[0] // T
    R = b_bits.shape[0]
    words = a_bits.shape[1]
    if b_bits.shape[1] != words:
        raise SolaError("packed masks have different resolutions")
    dev = a_bits.device
    inter = torch.empty((P, R), device=dev, dtype=torch.int64)
    union = torch.empty((P, R), device=dev, dtype=torch.int64)
    if a_frame is not None:
        a_frame = a_frame.to(device=dev, dtype=torch.int32).contiguous()
    check(lib().sola_mask_pair_counts(ptr(a_bits), ptr(a_area), P, T, ptr(b_bits), ptr(b_area), R, ptr(a_frame), words,
                                      ptr(inter), ptr(union), current_stream(dev)), "sola_mask_pair_counts")
    return inter, union


def mask_iou_matrix(A, B):
    """A [P,H,W], B [R,h,w] (resampled to H x W) -> (inter, union) int64 [P,R] in one library call."""
    A, B = _prep(A), _prep(B)
    if _elem_type(A) != _elem_type(B):
        raise SolaError("A and B must have the same dtype")
    P, H, W = A.shape
    R, h, w = B.shape
    dev = A.device
    out = torch.empty((2, P, R), device=dev, dtype=torch.int64)  # one allocation for both count matrices
    inter, union = out[0], out[1]
    nb = lib().sola_mask_iou_scratch_bytes(P, R, H, W)
    # reused from call to call: the de-dup loop calls this once per SAM2 iteration with 10-35 MB of masks
    scratch = _stream_scratch("iou", dev, nb)
    check(lib().sola_mask_iou_matrix(ptr(A), ptr(B), _elem_type(A), P, R, H, W, h, w, ptr(inter), ptr(union),
                                     ptr(scratch), scratch.numel(), current_stream(dev)), "sola_mask_iou_matrix")
    return inter, union


def iou_from_counts(inter, union):
    """python-float division; an empty union counts as IoU 1.0 (seg_utils.py:139-142)."""
    if union == 0:
        return 1.0
    return inter / union


@torch.no_grad()
def compute_mask_iou(maskA, maskB):
    """seg_utils.py:128-142: maskA, maskB (H,W) {0,1} -> float."""
    inter, union = mask_iou_matrix(maskA.unsqueeze(0), maskB.unsqueeze(0))
    i, u = torch.stack([inter[0, 0], union[0, 0]]).tolist()
    return iou_from_counts(i, u)


@torch.no_grad()
def compute_masklet_iou(maskletA, maskletB, device=None):
    """seg_utils.py:109-125: one ratio over all frames of two (T,H,W) masklets."""
    if device is not None:
        maskletA, maskletB = maskletA.to(device), maskletB.to(device)
    T, H, W = maskletA.shape
    inter, union = mask_iou_matrix(maskletA.reshape(1, T * H, W), maskletB.reshape(1, T * H, W))
    i, u = torch.stack([inter[0, 0], union[0, 0]]).tolist()
    return iou_from_counts(i, u)


@torch.no_grad()
def dedup_batch(masklets, prompt_ids, prompts, miou_thresh, reshape=False):
    """Greedy filtering of untracked prompts by the newly tracked masklets (generate_tokens_grid.py:252-278).

    masklets: dict prompt_id -> (T,H,W) {0,1} CUDA tensor at the comparison resolution (after reshape_masklet), or,
    with ``reshape=True``, at the tracker's native resolution — the bilinear resample + threshold of
    generate_tokens_grid.py:248-250 is then fused into the pack launch and no resized masklet is materialised;
    prompt_ids: new tracks in batch order; prompts: list of dicts (``status``, ``frame_idx``, ``segmentation``
    (h,w) array/tensor) mutated in place exactly like the reference.  All P x R intersections come from two pack
    launches and one pair launch and a single host copy; the order-dependent greedy decision runs on the host.
    """
    todo = [r for r, info in enumerate(prompts) if info["status"] == 0]
    if not todo or not prompt_ids:
        return 0
    first = masklets[prompt_ids[0]]
    dev = first.device
    T, H, W = first.shape
    A = torch.stack([masklets[pid] for pid in prompt_ids]).reshape(len(prompt_ids) * T, H, W)
    segs = [torch.as_tensor(prompts[r]["segmentation"]) for r in todo]
    B = torch.stack(segs).to(dev)
    if B.dtype not in (torch.uint8, torch.bool, torch.float32):
        B = (B != 0).to(torch.uint8)
    if reshape:
        a_bits, a_area, (H, W) = pack_masklet_bilinear(A)
    else:
        a_bits, a_area = pack_masks(A)
    b_bits, b_area = pack_masks(B, (H, W))
    frames = torch.tensor([prompts[r]["frame_idx"] for r in todo], dtype=torch.int32, device=dev)
    inter, union = pair_counts(a_bits, a_area, b_bits, b_area, T=T, a_frame=frames)
    inter, union = inter.cpu().tolist(), union.cpu().tolist()
    n_filtered = 0
    for p, pid in enumerate(prompt_ids):
        for c, r in enumerate(todo):
            info = prompts[r]
            if info["status"] > 0:
                continue
            iou = iou_from_counts(inter[p][c], union[p][c])
            if iou > miou_thresh:
                info["status"] = 2
                info["filtered_by"] = pid
                info["filtered_iou"] = iou
                n_filtered += 1
    return n_filtered


# ----------------------------------------------------------------------------------------------------------------
# masklet rows next to the predicate: reshape_masklet, per-frame metrics, part-ness, RLE merge
# ----------------------------------------------------------------------------------------------------------------
def default_target_shape(h, w):
    """seg_utils.py:154-156."""
    return (540, 960) if h < w else (960, 540)


def pack_masklet_bilinear(masklet, target_shape=None, logits=False):
    """[N,h,w] {0,1} -> (bits int32 [N,words], area int64 [N], (H,W)): bilinear resample + `> 0.5` + bit-pack in one
    pass over the source (seg_utils.py:145-160 without the fp32 [N,H,W] intermediate).  ``logits=True``: the input is
    the tracker's float32 mask logits and `(logits > 0).float()` (generate_tokens_grid.py:215-222) is applied on read."""
    masklet = _prep(masklet)
    et = _mask_kind(masklet, logits)
    n, h, w = masklet.shape
    H, W = default_target_shape(h, w) if target_shape is None else target_shape
    words = lib().sola_mask_words(H, W)
    bits = torch.empty((n, words), device=masklet.device, dtype=torch.int32)
    area = torch.empty((n,), device=masklet.device, dtype=torch.int64)
    check(lib().sola_mask_bilinear_pack(ptr(masklet), et, n, h, w, H, W, ptr(bits), ptr(area),
                                        current_stream(masklet.device)), "sola_mask_bilinear_pack")
    return bits, area, (H, W)


def unpack_masks(bits, H, W, dtype=torch.float32):
    """bits [n,words] -> {0,1} images [n,H,W] of ``dtype`` (float32 or uint8)."""
    require_cuda(bits)
    n = bits.shape[0]
    out = torch.empty((n, H, W), device=bits.device, dtype=dtype)
    check(lib().sola_mask_unpack(ptr(bits), n, H, W, ptr(out), _elem_type(out), current_stream(bits.device)),
          "sola_mask_unpack")
    return out


def reshape_masklet(masklet, target_shape=None, logits=False):
    """seg_utils.py:145-160: (N,h,w) {0,1} -> (N,H',W') float32 {0,1}."""
    bits, _, (H, W) = pack_masklet_bilinear(masklet, target_shape, logits)
    return unpack_masks(bits, H, W, torch.float32)


@torch.no_grad()
def frame_counts(pred_masks, gt_masks):
    """(T,H,W) x (T,H,W) -> int64 [T,3] on the host: (intersection, n_pred, n_gt) per frame, from two pack launches,
    one pair launch and one copy (the reference does five .item() syncs per frame, utils.py:146-151)."""
    pred_masks, gt_masks = _prep(pred_masks), _prep(gt_masks)
    if pred_masks.shape != gt_masks.shape:
        raise SolaError(f"masklets differ in shape: {tuple(pred_masks.shape)} vs {tuple(gt_masks.shape)}")
    T = pred_masks.shape[0]
    a_bits, a_area = pack_masks(pred_masks)
    b_bits, b_area = pack_masks(gt_masks)
    frames = torch.arange(T, dtype=torch.int32, device=pred_masks.device)
    inter, _ = pair_counts(a_bits, a_area, b_bits, b_area, T=T, a_frame=frames)
    return torch.stack([inter[0], a_area, b_area], 1).cpu()


@torch.no_grad()
def masklet_counts_matrix(pred_masklets, gt_masklets):
    """(P,T,H,W) x (G,T,H,W) -> int64 [P,G,T,3] (intersection, n_pred, n_gt) for every (pred track, GT object, frame):
    the whole `for prompt_id ... for gt_anno_id ... for t` nest of generate_tokens_grid.py:252-264 in one pair launch."""
    pred_masklets, gt_masklets = _prep(pred_masklets), _prep(gt_masklets)
    P, T, H, W = pred_masklets.shape
    G = gt_masklets.shape[0]
    if tuple(gt_masklets.shape[1:]) != (T, H, W):
        raise SolaError("pred and GT masklets differ in (T,H,W)")
    a_bits, a_area = pack_masks(pred_masklets.reshape(P * T, H, W))
    b_bits, b_area = pack_masks(gt_masklets.reshape(G * T, H, W))
    frames = torch.arange(T, dtype=torch.int32, device=pred_masklets.device).repeat(G)
    inter, _ = pair_counts(a_bits, a_area, b_bits, b_area, T=T, a_frame=frames)  # [P, G*T]
    out = torch.stack([inter.view(P, G, T), a_area.view(P, 1, T).expand(P, G, T), b_area.view(1, G, T).expand(P, G, T)], -1)
    return out.cpu()


def metrics_from_counts(counts):
    """utils.py:146-168 on the integer counts [T,3] -> (precision, recall, iou) float32 [T] CPU tensors."""
    T = len(counts)
    precision, recall, iou = torch.zeros(T).float(), torch.zeros(T).float(), torch.zeros(T).float()
    for t, (intersection, n_pred, n_gt) in enumerate(counts.tolist() if hasattr(counts, "tolist") else counts):
        union = n_pred + n_gt - intersection
        iou[t] = 1.0 if union == 0 else intersection / union
        if n_pred == 0 and n_gt == 0:
            precision[t], recall[t] = 1.0, 1.0
        elif n_pred == 0 and n_gt > 0:
            precision[t], recall[t] = 1.0, 0.0
        elif n_pred > 0 and n_gt == 0:
            precision[t], recall[t] = 0.0, 1.0
        else:
            precision[t], recall[t] = intersection / n_pred, intersection / n_gt
    return precision, recall, iou


@torch.no_grad()
def compute_mask_metrics(pred_masks, gt_masks, reduction="mean"):
    """utils.py:131-174: (T,H,W) x (T,H,W) -> precision, recall, iou (0-d float32 tensors, or [T] with 'none')."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"Invalid reduction method: {reduction}")
    precision, recall, iou = metrics_from_counts(frame_counts(pred_masks, gt_masks))
    if reduction == "mean":
        return precision.mean(), recall.mean(), iou.mean()
    return precision, recall, iou


def J_from_counts(counts):
    """evaluator.py:227-237."""
    import numpy as np
    Js = []
    for intersection, n_pred, n_gt in counts.tolist():
        union = n_pred + n_gt - intersection
        Js.append(1.0 if union == 0 else intersection / union)
    return np.mean(Js)


def F_from_counts(counts):
    """evaluator.py:239-247: tp / fp / fn over all frames."""
    tp, n_pred, n_gt = counts.sum(0).tolist()
    fp, fn = n_pred - tp, n_gt - tp
    if tp == 0:
        return 0.0
    precision = tp / (tp + fp)
    recall = tp / (tp + fn)
    return 2 * precision * recall / (precision + recall)


def boundary_radius(h, w, bound_th=0.008):
    """Disk radius of the DAVIS contour measure: ``bound_th`` itself when >= 1, else ceil(bound_th * image diagonal)."""
    import numpy as np
    return int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.sqrt(np.float64(h * h + w * w))))


def F_boundary_from_counts(counts):
    """DAVIS contour F of a masklet: mean over frames of the F-measure of boundary precision and recall, from the
    [T,4] counts (n_fg, n_gt, fg_match, gt_match) of sola_mask_select_boundary_counts."""
    import numpy as np
    Fs = []
    for n_fg, n_gt, fg_match, gt_match in counts.tolist():
        if n_fg == 0 and n_gt > 0:
            precision, recall = 1, 0
        elif n_fg > 0 and n_gt == 0:
            precision, recall = 0, 1
        elif n_fg == 0 and n_gt == 0:
            precision, recall = 1, 1
        else:
            precision, recall = fg_match / n_fg, gt_match / n_gt
        Fs.append(0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall))
    return np.mean(Fs)


def _boundary_th(boundary):
    return 0.008 if boundary is True else boundary


def compute_J(pred_masklet, gt_masklet):
    return J_from_counts(frame_counts(pred_masklet, gt_masklet))


def compute_F(pred_masklet, gt_masklet):
    return F_from_counts(frame_counts(pred_masklet, gt_masklet))


def compute_JF(pred_masklet, gt_masklet):
    """J, F and (J+F)/2 from ONE counting pass (evaluator.py:196-199 runs two)."""
    c = frame_counts(pred_masklet, gt_masklet)
    J, F = float(J_from_counts(c)), float(F_from_counts(c))
    return J, F, (J + F) / 2


@torch.no_grad()
def compute_F_boundary(pred_masklet, gt_masklet, bound_th=0.008):
    """DAVIS contour F of two dense (T,h,w) masklets on the GPU (the counterpart of compute_F for the benchmark's F): the
    transposed frames go through pack_masks, which makes them the column-major planes sola_mask_select_boundary_counts
    reads, prediction t against ground truth t."""
    pred_masklet, gt_masklet = _prep(pred_masklet), _prep(gt_masklet)
    if pred_masklet.shape != gt_masklet.shape or pred_masklet.dim() != 3:
        raise SolaError(f"masklets must be (T,h,w) of one shape: {tuple(pred_masklet.shape)} vs {tuple(gt_masklet.shape)}")
    if _elem_type(pred_masklet) != _elem_type(gt_masklet):
        gt_masklet = gt_masklet.to(pred_masklet.dtype)
    T, h, w = pred_masklet.shape
    dev = pred_masklet.device
    L = lib()
    stride = L.sola_jf_plane_words(h, w)
    packed, _ = pack_masks(torch.cat([pred_masklet, gt_masklet]).transpose(1, 2).contiguous())  # [2T, ceil(h*w/32)]
    bits = torch.zeros((2 * T, stride), device=dev, dtype=torch.int32)
    bits[:, :packed.shape[1]] = packed
    # 2T masks of one frame each: "expression" t selects mask t and is scored against mask T + t
    ints = torch.arange(T + 1, dtype=torch.int32, device=dev)
    gidx = ints[:T] + T
    counts = torch.empty((T, 1, 4), device=dev, dtype=torch.int64)
    check(L.sola_mask_select_boundary_counts(ptr(bits), stride, 2 * T, 1, h, w, boundary_radius(h, w, bound_th), ptr(ints), ptr(ints),
                                             ptr(ints), ptr(gidx), T, ptr(counts), None, 0, current_stream(dev)),
          "sola_mask_select_boundary_counts")
    return F_boundary_from_counts(counts[:, 0].cpu())


@torch.no_grad()
def compute_P(part_masks, full_mask):
    """utils.py:177-192: part-ness |part & full| / |part| as float32 [N] on the masks' device (0/0 -> nan as there)."""
    part_masks, full_mask = _prep(part_masks), _prep(full_mask)
    if _elem_type(part_masks) != _elem_type(full_mask):
        full_mask = full_mask.to(part_masks.dtype)
    a_bits, a_area = pack_masks(part_masks)
    b_bits, b_area = pack_masks(full_mask.unsqueeze(0))
    inter, _ = pair_counts(a_bits, a_area, b_bits, b_area)
    return inter[:, 0].to(torch.float32) / a_area.to(torch.float32)


def _run_list_cum(counts, limit, who):
    """Inclusive prefix sums (uint32) of an uncompressed run list, which must be non-negative and cover at most ``limit`` pixels."""
    import numpy as np
    c = np.cumsum(np.asarray(counts, dtype=np.int64))
    if len(c) and (c[-1] > limit or np.any(np.diff(c) < 0) or c[0] < 0):
        raise SolaError(f"{who}: runs are negative or exceed the image")
    return c.astype(np.uint32)


def _rle_cum(rle, limit):
    """Inclusive prefix sums (uint32) of one RLE dict's run lengths; compressed strings are parsed by the library's
    host helper (sola_rle_string_to_cum), uncompressed lists by numpy."""
    import ctypes
    import numpy as np
    counts = rle["counts"]
    if isinstance(counts, str):
        counts = counts.encode("ascii")
    if isinstance(counts, (bytes, bytearray)):
        buf = np.empty(max(1, len(counts)), np.uint32)
        n = lib().sola_rle_string_to_cum(bytes(counts), len(counts), ctypes.c_void_p(buf.ctypes.data), len(buf), limit)
        if n < 0:
            check(int(n), "sola_rle_string_to_cum")
        return buf[:n]
    return _run_list_cum(counts, limit, "rle_merge_or")


@torch.no_grad()
def rle_merge_or(rle_lists, device, packed=False):
    """OR of K RLE masklets (each a list of T per-frame COCO RLE dicts, non-dict = missing frame) decoded on the GPU:
    dataloader.py:326-369 (rle_masklet_decode + np.logical_or).  Only the run-length strings are parsed on the host.
    Returns uint8 [T,h,w] (or (bits, area, (h,w)) with ``packed``)."""
    import numpy as np
    K = len(rle_lists)
    if K == 0:
        raise SolaError("rle_merge_or: no masklets")
    T = len(rle_lists[0])
    size = next((tuple(r["size"]) for rl in rle_lists for r in rl if isinstance(r, dict)), None)
    if size is None:
        raise SolaError("rle_merge_or: every frame is missing")
    h, w = size
    cums, off = [], [0]
    for f in range(T):
        for k in range(K):
            r = rle_lists[k][f] if f < len(rle_lists[k]) else None
            if isinstance(r, dict):
                if tuple(r["size"]) != (h, w):
                    raise SolaError(f"rle_merge_or: frame size {tuple(r['size'])} != {(h, w)}")
                c = _rle_cum(r, h * w)
                cums.append(c)
                off.append(off[-1] + len(c))
            else:
                off.append(off[-1])
    cum = np.concatenate(cums) if cums else np.zeros(1, np.uint32)
    if len(cum) == 0:
        cum = np.zeros(1, np.uint32)
    dev = torch.device(device)
    cum_t = torch.from_numpy(cum.view(np.int32)).to(dev)
    off_t = torch.tensor(off, dtype=torch.int64, device=dev)
    stream = current_stream(dev)
    if packed:
        words = lib().sola_mask_words(h, w)
        bits = torch.empty((T, words), device=dev, dtype=torch.int32)
        area = torch.empty((T,), device=dev, dtype=torch.int64)
        check(lib().sola_rle_fill_or(ptr(cum_t), ptr(off_t), T, K, h, w, None, ptr(bits), ptr(area), stream), "sola_rle_fill_or")
        return bits, area, (h, w)
    out = torch.empty((T, h, w), device=dev, dtype=torch.uint8)
    check(lib().sola_rle_fill_or(ptr(cum_t), ptr(off_t), T, K, h, w, ptr(out), None, None, stream), "sola_rle_fill_or")
    return out


# ----------------------------------------------------------------------------------------------------------------
# mask-level J&F of a whole video (evaluator.py:174-247): decode every referenced masklet once, count every expression
# ----------------------------------------------------------------------------------------------------------------
def rle_strings_to_cum(strings, limit=-1):
    """Compressed COCO RLE strings (str / bytes) -> (cum uint32 [runs], run_off int64 [n+1]) from one library call
    (sola_rle_strings_to_cum_batch): string i's inclusive prefix sums of its run lengths are cum[run_off[i]:run_off[i+1]].
    An empty string has no runs.  Malformed strings, and runs covering more than ``limit`` pixels, raise SolaError."""
    import numpy as np
    enc = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strings]
    str_off = np.zeros(len(enc) + 1, np.int64)
    np.cumsum([len(s) for s in enc], out=str_off[1:])
    chars = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
    cum = np.empty(max(1, int(str_off[-1])), np.uint32)  # a run takes at least one character
    run_off = np.empty(len(enc) + 1, np.int64)
    n = lib().sola_rle_strings_to_cum_batch(chars.ctypes.data, str_off.ctypes.data, len(enc), cum.ctypes.data, len(cum), limit,
                                           run_off.ctypes.data)
    if n < 0:
        check(int(n), "sola_rle_strings_to_cum_batch")
    return cum[:n], run_off


def _masklet_geometry(masklets):
    """(T, (h, w) or None) shared by every masklet (lists of RLE dicts and IndexMasklets alike); SolaError when they differ."""
    T = len(masklets[0])
    size = None
    for m in masklets:
        if len(m) != T:
            raise SolaError(f"masklet_select_counts: masklets have {len(m)} and {T} frames")
        sizes = [m.size] if isinstance(m, IndexMasklet) else [tuple(r["size"]) for r in m if isinstance(r, dict)]
        for s in sizes:
            if size is None:
                size = s
            elif s != size:
                raise SolaError(f"masklet_select_counts: frame size {s} != {size}")
    return T, size


def _planes_cum(masklets, ids, T, hw):
    """Host side of one decode launch: the run prefix sums of masks ``ids`` (plane k*T + t = frame t of ids[k]), from one
    parse of all their compressed strings; uncompressed count lists are summed by numpy and spliced in."""
    import numpy as np
    frames = [masklets[m][t] for m in ids for t in range(T)]
    lists = {}
    strings = []
    for p, r in enumerate(frames):
        c = r["counts"] if isinstance(r, dict) else ""
        if not isinstance(c, (str, bytes, bytearray)):
            lists[p] = c
            c = ""
        strings.append(c)
    cum, off = rle_strings_to_cum(strings, hw)
    if lists:
        pieces = []
        for p in range(len(frames)):
            pieces.append(_run_list_cum(lists[p], hw, "masklet_select_counts") if p in lists else cum[off[p]:off[p + 1]])
        off = np.zeros(len(frames) + 1, np.int64)
        np.cumsum([len(x) for x in pieces], out=off[1:])
        cum = np.concatenate(pieces) if pieces else cum[:0]
    return cum, off


def _plane_groups(masklets, refs, T, h, w, stride, dev, max_plane_bytes):
    """The plane-building half of masklet_select_counts / masklet_sweep_counts.  ``refs[e]`` lists the masklets expression e
    reads.  Expressions are grouped in order so that the planes of one group stay under ``max_plane_bytes`` (an expression
    that alone exceeds it runs by itself); for every group the masks it references are decoded once (one parse and one
    sola_rle_pack_cm launch for the RLE masklets, one sola_index_pack launch per index-map tensor) and
    ``(expressions, {masklet: row of the group's buffer}, bits [rows * T, stride], rows)`` is yielded.  A group that references
    no mask gets one dummy plane of 4 words and 0 rows."""
    import numpy as np
    L = lib()
    stream = current_stream(dev)
    mask_bytes = T * stride * 4
    groups, cur, cur_ids = [], [], set()
    for e, ref in enumerate(refs):
        ids = set(ref)
        if cur and len(cur_ids | ids) * mask_bytes > max_plane_bytes:
            groups.append(cur)
            cur, cur_ids = [], set()
        cur.append(e)
        cur_ids |= ids
    groups.append(cur)
    for grp in groups:
        ids = sorted(set(i for e in grp for i in refs[e]))
        # RLE masklets come first in the buffer (one decode launch over their rows), then the index masklets, those of one
        # index-map tensor next to each other (one compare launch per tensor into its objects' rows)
        by_maps = {}
        for m in ids:
            if isinstance(masklets[m], IndexMasklet):
                by_maps.setdefault(id(masklets[m].index_maps), []).append(m)
        if by_maps:
            ids = [m for m in ids if not isinstance(masklets[m], IndexMasklet)] + [m for ms in by_maps.values() for m in ms]
        n_rle = len(ids) - sum(len(ms) for ms in by_maps.values())
        local = {m: k for k, m in enumerate(ids)}
        if ids:
            bits = torch.empty((len(ids) * T, stride), device=dev, dtype=torch.int32)
            if n_rle:
                cum, off = _planes_cum(masklets, ids[:n_rle], T, h * w)
                cum_t = torch.from_numpy((cum if len(cum) else np.zeros(1, np.uint32)).view(np.int32)).to(dev)
                off_t = torch.from_numpy(off).to(dev)
                check(L.sola_rle_pack_cm(ptr(cum_t), ptr(off_t), n_rle * T, h, w, stride, ptr(bits), stream), "sola_rle_pack_cm")
            for ms in by_maps.values():
                maps = masklets[ms[0]].index_maps
                if maps.device.type != dev.type or (dev.index is not None and maps.device.index != dev.index):
                    raise SolaError(f"masklet_select_counts: index maps on {maps.device}, counting on {dev}")
                pack_index_masklets(maps, [masklets[m].obj_id for m in ms], "cm", out=bits, first_plane=[local[m] * T for m in ms])
        else:  # no expression of the group references a mask: every count is 0
            bits = torch.zeros((1, 4), device=dev, dtype=torch.int32)
        yield grp, local, bits, len(ids)


def _level_counts(who, masklets, lists, ends, K, gt_sets, device, max_plane_bytes, boundary):
    """The counting path under masklet_select_counts and masklet_sweep_counts (``who``: the caller's name in the messages):
    ``(counts, bcounts)`` on the host, counts int64 [E, K, T, 3] with ``[e, k]`` the (intersection, n_pred, n_gt) table of the
    prediction OR over ``lists[e][:ends[e][k]]`` against the OR over ``gt_sets[e]``; ``ends[e]`` holds K non-decreasing prefix
    lengths.  bcounts is None, or with ``boundary`` int64 [E, K, T, 4].  Per group of _plane_groups: one int32 upload of every
    list, one sola_mask_nested_counts call, and the K prefix lists of every expression as E*K pseudo-expressions through one
    sola_mask_select_boundary_counts launch on the same planes (with K = 1 those are the prediction lists themselves)."""
    E, M = len(lists), len(masklets)
    if M == 0:
        raise SolaError(f"{who}: no masklets")
    for s in list(lists) + list(gt_sets):
        for i in s:
            if not 0 <= int(i) < M:
                raise SolaError(f"{who}: index {i} outside the {M} masklets")
    T, size = _masklet_geometry(masklets)
    if E == 0 or size is None or T == 0:  # (no size: every frame of every masklet is missing, all masks are empty)
        return torch.zeros((E, K, T, 3), dtype=torch.int64), None if boundary is None else torch.zeros((E, K, T, 4), dtype=torch.int64)
    h, w = size
    L = lib()
    radius = None if boundary is None else boundary_radius(h, w, _boundary_th(boundary))
    stride = L.sola_jf_plane_words(h, w)
    dev = torch.device(device)
    stream = current_stream(dev)
    preds = [[int(i) for i in lists[e][:ends[e][-1]]] for e in range(E)]  # what the largest level selects
    gts = [[int(i) for i in s] for s in gt_sets]
    outs, bouts = [], []
    for grp, local, bits, n_ids in _plane_groups(masklets, [p + g for p, g in zip(preds, gts)], T, h, w, stride, dev, max_plane_bytes):
        Eg = len(grp)
        poff, pidx, goff, gidx, lend = [0], [], [0], [], []
        for e in grp:
            pidx += [local[i] for i in preds[e]]
            poff.append(len(pidx))
            gidx += [local[i] for i in gts[e]]
            goff.append(len(gidx))
            lend += ends[e]
        parts = [lend, poff, pidx + [0], goff, gidx + [0]]  # (the pad entries keep the pointers of empty lists non-null)
        if radius is not None and K > 1:  # level k of expression e as pseudo-expression e*K + k of the boundary launch
            boff, bidx, bgoff, bgidx = [0], [], [0], []
            for j, e in enumerate(grp):
                for k in range(K):
                    bidx += pidx[poff[j]:poff[j] + ends[e][k]]
                    boff.append(len(bidx))
                    bgidx += gidx[goff[j]:goff[j + 1]]
                    bgoff.append(len(bgidx))
            parts += [boff, bidx + [0], bgoff, bgidx + [0]]
        ints = torch.tensor([x for part in parts for x in part], dtype=torch.int32).to(dev)  # one copy for every list
        d, o = [], 0
        for part in parts:
            d.append(ptr(ints[o:o + len(part)]))
            o += len(part)
        counts = torch.empty((Eg, K, T, 3), device=dev, dtype=torch.int64)
        check(L.sola_mask_nested_counts(ptr(bits), stride if n_ids else 4, n_ids, T, d[1], d[2], d[0], K, d[3], d[4], Eg, ptr(counts),
                                        stream), "sola_mask_nested_counts")
        outs.append(counts)
        if radius is not None:
            bcounts = torch.empty((Eg, K, T, 4), device=dev, dtype=torch.int64)
            # (without ids no plane is read: the stride is the frame's over the dummy plane)
            check(L.sola_mask_select_boundary_counts(ptr(bits), stride, n_ids, T, h, w, radius, *d[-4:], Eg * K, ptr(bcounts), None, 0,
                                                     stream), "sola_mask_select_boundary_counts")
            bouts.append(bcounts)
    counts = (outs[0] if len(outs) == 1 else torch.cat(outs)).cpu()
    return counts, None if radius is None else (bouts[0] if len(bouts) == 1 else torch.cat(bouts)).cpu()


@torch.no_grad()
def masklet_select_counts(masklets, pred_sets, gt_sets, device, max_plane_bytes=2 << 30, boundary=None):
    """Every expression of a video against its ground truth, per frame: int64 [E, T, 3] (intersection, n_pred, n_gt) on the
    host, where expression e's prediction is the OR of ``masklets[i]`` for i in ``pred_sets[e]`` and its ground truth the OR
    over ``gt_sets[e]`` (dataloader.py:251-351 get_gt_masklet / get_sam2_masklet, evaluator.py:227-247).

    ``masklets``: M masklets of one T and (h, w), each a list of T per-frame COCO RLE dicts (a non-dict is a missing frame =
    zeros) or an IndexMasklet (``index_maps == obj_id``; those of one index-map tensor are compared by one sola_index_pack
    launch into their rows of the RLE masklets' plane buffer).  Only the masks some list references are decoded, once each,
    into column-major bit planes (sola_rle_pack_cm) and every (expression, frame) is counted by one launch (_level_counts with
    one level per expression, the whole list): one host parse, one decode launch, one count launch and one copy.  The planes
    of one launch are capped at ``max_plane_bytes``: expressions are grouped in order under that budget (an expression that
    alone exceeds it runs by itself).  An empty list is an all-zero masklet.  Counts are exact int64; the reference sums
    float32 tensors, which is exact while every count is below 2^24.

    ``boundary`` = the DAVIS ``bound_th`` (``True`` = 0.008): returns ``(counts, bcounts)`` with bcounts int64 [E, T, 4] =
    (n_fg, n_gt, fg_match, gt_match), the boundary pixels of prediction and ground truth and those within the disk of
    boundary_radius(h, w, bound_th) of the other's (sola_mask_select_boundary_counts on the planes of the same decode
    launch; F_boundary_from_counts turns a [T,4] table into the benchmark's F)."""
    if len(gt_sets) != len(pred_sets):
        raise SolaError(f"masklet_select_counts: {len(pred_sets)} prediction sets but {len(gt_sets)} GT sets")
    counts, bcounts = _level_counts("masklet_select_counts", masklets, pred_sets, [[len(s)] for s in pred_sets], 1, gt_sets, device,
                                    max_plane_bytes, boundary)
    return counts[:, 0] if boundary is None else (counts[:, 0], bcounts[:, 0])


def _jf_scores(counts, bcounts=None):
    """One expression's [T,3] table (and [T,4] boundary table) -> (J, F, JF) or (J, F, JF, F_boundary, JF_boundary)."""
    J, F = float(J_from_counts(counts)), float(F_from_counts(counts))
    if bcounts is None:
        return J, F, (J + F) / 2
    Fb = float(F_boundary_from_counts(bcounts))
    return J, F, (J + F) / 2, Fb, (J + Fb) / 2


def compute_JF_batch(masklets, pred_sets, gt_sets, device, boundary=None, **kw):
    """[(J, F, (J + F) / 2)] per expression from masklet_select_counts: evaluator.py:196-199,227-247 for every expression of
    a video in one counting pass.  J is the mean over frames of inter / union (1.0 for an empty union), F the pixel F1 over
    the whole masklet (0.0 when there is no true positive): the reference evaluator's F.  The DAVIS boundary F comes with
    ``boundary`` = its ``bound_th`` (``True`` = 0.008): every entry is then (J, F, JF, F_boundary, JF_boundary), F_boundary
    the mean over frames of the contour F-measure and JF_boundary = (J + F_boundary) / 2, the benchmark's J&F."""
    counts = masklet_select_counts(masklets, pred_sets, gt_sets, device, boundary=boundary, **kw)
    if boundary is None:
        return [_jf_scores(c) for c in counts]
    return [_jf_scores(c, b) for c, b in zip(*counts)]


# ----------------------------------------------------------------------------------------------------------------
# J&F at every selection threshold of a sweep (inference.py:104,141 / eval.py --eval_pred_threshold): the selections at
# descending thresholds are nested, so one counting pass over the largest one gives every level (sola_mask_nested_counts)
# ----------------------------------------------------------------------------------------------------------------
def sweep_levels(probs, thresholds):
    """One expression's float32 scores [n] and K thresholds (any order, duplicates allowed) -> ``(order, level_end, perm)``.
    A track is selected at a threshold when ``np.float32(prob) > np.float32(threshold)``, strict: the entry points' own
    ``prob > pred_threshold`` on float32 tensors.  With the thresholds stably sorted descending (the levels), ``order`` holds
    the indices of the tracks selected at the lowest one, stably sorted by the first level that selects them, and
    ``level_end`` (int32 [K]) the number of them selected at each level: level k's selection is ``order[:level_end[k]]``.
    ``perm`` (int64 [K]) maps the levels back: the caller's threshold j is level ``perm[j]``.  Host only."""
    import numpy as np
    p = np.asarray(probs, dtype=np.float32).reshape(-1)
    th = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    K = len(th)
    desc = np.argsort(-th, kind="stable")
    perm = np.empty(K, np.int64)
    perm[desc] = np.arange(K)
    first = K - (p[:, None] > th[desc][None, :]).sum(1) if K else np.zeros(len(p), np.int64)  # nested: the levels that select a track are a suffix
    keep = np.flatnonzero(first < K)
    order = keep[np.argsort(first[keep], kind="stable")].astype(np.int64)
    level_end = np.searchsorted(first[order], np.arange(K), side="right").astype(np.int32)
    return order, level_end, perm


@torch.no_grad()
def masklet_sweep_counts(masklets, cand_sets, probs, thresholds, gt_sets, device, max_plane_bytes=2 << 30, boundary=None):
    """masklet_select_counts at every threshold of a sweep from one decode and one counting pass: int64 [E, K, T, 3] on the
    host, ``[e, j]`` the (intersection, n_pred, n_gt) table of the prediction {``cand_sets[e][i]`` : ``probs[e][i]`` >
    ``thresholds[j]``} (the rule of sweep_levels) against the OR over ``gt_sets[e]``, levels in the caller's threshold order.

    ``cand_sets[e]`` holds the masklet indices of expression e's tracks, ``probs[e]`` their float32 scores.  The host work is
    masklet_select_counts' (_level_counts): the masks referenced are the selection at the lowest threshold plus the ground
    truth, decoded once per group of expressions under ``max_plane_bytes``; then one sola_mask_nested_counts call, in which
    every plane is read once per (expression, frame) whatever K, and one copy.  With ``boundary`` (the DAVIS bound_th,
    ``True`` = 0.008) returns ``(counts, bcounts)``, bcounts int64 [E, K, T, 4] as masklet_select_counts gives it."""
    import numpy as np
    E, K = len(cand_sets), len(thresholds)
    if K == 0:
        raise SolaError("masklet_sweep_counts: no thresholds")
    if len(gt_sets) != E or len(probs) != E:
        raise SolaError(f"masklet_sweep_counts: {E} candidate sets but {len(probs)} score vectors and {len(gt_sets)} GT sets")
    ordered, ends, perm = [], [], np.arange(K)
    for e in range(E):
        if len(probs[e]) != len(cand_sets[e]):
            raise SolaError(f"masklet_sweep_counts: expression {e} has {len(cand_sets[e])} tracks but {len(probs[e])} scores")
        order, level_end, perm = sweep_levels(probs[e], thresholds)
        rest = np.setdiff1d(np.arange(len(probs[e])), order)  # never selected: range-checked with the others, never read
        ordered.append([cand_sets[e][i] for i in order] + [cand_sets[e][i] for i in rest])
        ends.append(level_end.tolist())
    counts, bcounts = _level_counts("masklet_sweep_counts", masklets, ordered, ends, K, gt_sets, device, max_plane_bytes, boundary)
    perm = torch.from_numpy(perm)
    counts = counts[:, perm].contiguous()
    return counts if boundary is None else (counts, bcounts[:, perm].contiguous())


def compute_JF_sweep(masklets, cand_sets, probs, thresholds, gt_sets, device, boundary=None, **kw):
    """compute_JF_batch at every threshold of a sweep, from masklet_sweep_counts: per expression a list over ``thresholds`` (the
    caller's order) of the tuples compute_JF_batch returns for that threshold's selection, (J, F, JF) or, with ``boundary``,
    (J, F, JF, F_boundary, JF_boundary)."""
    counts = masklet_sweep_counts(masklets, cand_sets, probs, thresholds, gt_sets, device, boundary=boundary, **kw)
    if boundary is None:
        return [[_jf_scores(c) for c in ce] for ce in counts]
    return [[_jf_scores(c, b) for c, b in zip(ce, be)] for ce, be in zip(*counts)]


# ----------------------------------------------------------------------------------------------------------------
# masks -> COCO compressed RLE (the track writers' seg_utils.encode_rle_masklet_torch / utils.encode_rle_mask)
# ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encode_rle_masklet(masks, logits=False, return_cum=False):
    """(T,h,w) masks on the GPU -> list of T ``{"size": [h, w], "counts": str}``, byte-identical to pycocotools
    ``encode`` + ``counts.decode("utf-8")`` per frame (seg_utils.encode_rle_masklet_torch), without the host copy of the
    masklet.  uint8 / bool / float32 pixels count when != 0; ``logits=True`` takes float32 tracker logits and counts
    ``> 0`` (the ``(out_mask_logits > 0.0)`` of generate_tokens_grid.py:215).  The host reads two sizes and copies the
    characters once.  ``return_cum=True`` stops before the characters and returns the device ``(cum, run_off)``: cum
    int32 [runs] holds the uint32 inclusive prefix sums of every frame's run lengths and run_off int64 [T+1] the first
    run of each frame, which is what ``sola_rle_fill_or`` reads (offsets = run_off, K = 1)."""
    masks = _prep(masks)
    if masks.dim() != 3:
        raise SolaError(f"encode_rle_masklet: masks must be (T,h,w), got {tuple(masks.shape)}")
    et = _mask_kind(masks, logits)
    n, h, w = masks.shape
    dev = masks.device
    offs = torch.zeros((2, n + 1), device=dev, dtype=torch.int64)  # run_off, char_off
    run_off, char_off = offs[0], offs[1]
    if n == 0:
        return (torch.empty((0,), device=dev, dtype=torch.int32), run_off) if return_cum else []
    L, stream = lib(), current_stream(dev)
    nb = L.sola_rle_encode_scratch_bytes(n, h, w)
    scratch = torch.empty((max(nb, 1),), device=dev, dtype=torch.uint8)
    check(L.sola_rle_encode_runs(ptr(masks), et, n, h, w, ptr(run_off), ptr(scratch), nb, stream), "sola_rle_encode_runs")
    runs = int(run_off[n])  # host read 1: the size of cum
    cum = torch.empty((runs,), device=dev, dtype=torch.int32)
    check(L.sola_rle_encode_cum(ptr(masks), et, n, h, w, ptr(run_off), ptr(cum), ptr(char_off), ptr(scratch), nb, stream),
          "sola_rle_encode_cum")
    if return_cum:
        return cum, run_off
    coff = char_off.cpu().tolist()  # host read 2: every frame's first character, coff[n] = the size of the string buffer
    chars = torch.empty((coff[n],), device=dev, dtype=torch.uint8)
    check(L.sola_rle_encode_chars(ptr(cum), ptr(run_off), ptr(char_off), n, ptr(chars), stream), "sola_rle_encode_chars")
    text = chars.cpu().numpy().tobytes().decode("ascii")
    return [{"size": [h, w], "counts": text[coff[i]:coff[i + 1]]} for i in range(n)]


encode_rle_masklet_torch = encode_rle_masklet


def encode_rle_mask(mask, logits=False):
    """(h,w) mask on the GPU -> one ``{"size": [h, w], "counts": str}`` (utils.encode_rle_mask)."""
    if mask.dim() != 2:
        raise SolaError(f"encode_rle_mask: mask must be (h,w), got {tuple(mask.shape)}")
    return encode_rle_masklet(mask.unsqueeze(0), logits)[0]


def _split_frames(flat, masklets):
    """The per-frame list of an encode over masklets concatenated along frames -> one list per masklet."""
    out, f = [], 0
    for m in masklets:
        out.append(flat[f:f + m.shape[0]])
        f += m.shape[0]
    return out


@torch.no_grad()
def encode_rle_masklets(masklets, logits=False):
    """Every track of a SAM2 batch (list of (T_i,h,w) masklets of one size and dtype) -> list of per-track RLE lists,
    from ONE encode over the masklets concatenated along frames."""
    if len(masklets) == 0:
        return []
    return _split_frames(encode_rle_masklet(torch.cat([_prep(m) for m in masklets]), logits), masklets)


# ----------------------------------------------------------------------------------------------------------------
# masks -> PNG files (inference.py's writer: 8-bit greyscale, 255 where the mask is set)
# ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def png_deflate_masklet(masks, logits=False, out=None):
    """(T,h,w) masks on the GPU -> ``(bytes, offsets)``: every frame's zlib stream (``78 01``, one fixed-Huffman DEFLATE
    block of distance-1 matches over the filter-0 scanlines, Adler-32; include/sola_hip.h gives the format) back to back,
    frame t at ``bytes[offsets[t]:offsets[t + 1]]``.  Two library calls, one host read of the T+1 offsets between them and
    one copy of the streams; the masklet itself never leaves the device.  ``out``: a uint8 device tensor of at least
    ``offsets[T]`` bytes to write into (tests: every byte is written whatever it held)."""
    masks = _prep(masks)
    if masks.dim() != 3:
        raise SolaError(f"png_deflate_masklet: masks must be (T,h,w), got {tuple(masks.shape)}")
    et = _mask_kind(masks, logits)
    n, h, w = masks.shape
    if n == 0:
        return b"", [0]
    dev = masks.device
    L, stream = lib(), current_stream(dev)
    nb = L.sola_png_deflate_scratch_bytes(n, h, w)
    scratch = torch.empty((max(nb, 8) + 7) // 8, device=dev, dtype=torch.int64)
    byte_off = torch.empty((n + 1,), device=dev, dtype=torch.int64)
    adler = torch.empty((n,), device=dev, dtype=torch.int32)
    check(L.sola_png_deflate_sizes(ptr(masks), et, n, h, w, ptr(byte_off), ptr(adler), ptr(scratch), nb, stream),
          "sola_png_deflate_sizes")
    offs = byte_off.cpu().tolist()  # the host read: every frame's first byte, offs[n] = the size of the buffer
    if out is None:
        out = torch.empty((offs[n],), device=dev, dtype=torch.uint8)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= offs[n]):
        raise SolaError(f"png_deflate_masklet: out must be a contiguous uint8 device tensor of >= {offs[n]} bytes")
    check(L.sola_png_deflate_write(ptr(masks), et, n, h, w, ptr(byte_off), ptr(adler), ptr(out), ptr(scratch), nb, stream),
          "sola_png_deflate_write")
    return out[:offs[n]].cpu().numpy().tobytes(), offs


def _png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def encode_png_masklet(masks, logits=False):
    """(T,h,w) masks on the GPU -> list of T complete PNG files (bytes): 8-bit greyscale, 255 where the mask is set - what
    ``Image.fromarray(mask * 255).save(..., "PNG")`` stores, mode ``L`` - from png_deflate_masklet.  The host adds the
    signature, IHDR, the IDAT length and CRC-32 (over the compressed bytes only) and IEND.  uint8 / bool / float32 pixels
    count when != 0; ``logits=True`` counts float32 ``> 0``.  The files use the fixed Huffman table: larger than a general
    encoder's, equal pixels."""
    data, offs = png_deflate_masklet(masks, logits)
    if len(offs) == 1:
        return []
    h, w = masks.shape[1:]
    head = b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
    tail = _png_chunk(b"IEND", b"")
    return [head + _png_chunk(b"IDAT", data[offs[i]:offs[i + 1]]) + tail for i in range(len(offs) - 1)]


def encode_png_mask(mask, logits=False):
    """(h,w) mask on the GPU -> one PNG file (bytes)."""
    if mask.dim() != 2:
        raise SolaError(f"encode_png_mask: mask must be (h,w), got {tuple(mask.shape)}")
    return encode_png_masklet(mask.unsqueeze(0), logits)[0]


@torch.no_grad()
def encode_png_masklets(masklets, logits=False):
    """list of (T_i,h,w) masklets of one size and dtype -> list of per-masklet PNG lists, from ONE encode over the masklets
    concatenated along frames."""
    if len(masklets) == 0:
        return []
    return _split_frames(encode_png_masklet(torch.cat([_prep(m) for m in masklets]), logits), masklets)


# ----------------------------------------------------------------------------------------------------------------
# PNG files of selections of a video's masklets, at one or many thresholds, from one decode per video (inference.py)
# ----------------------------------------------------------------------------------------------------------------
def rm_plane_words(h, w):
    """Stride (uint32 words) of a row-major plane that planes_cm_to_rm writes: sola_mask_words rounded up to a multiple of 4."""
    return (lib().sola_mask_words(h, w) + 3) // 4 * 4


@torch.no_grad()
def planes_cm_to_rm(bits_cm, h, w, out=None):
    """Column-major bit planes ``[n, sola_jf_plane_words(h, w)]`` int32 (sola_rle_pack_cm / pack_index_masklets ``layout="cm"``)
    -> row-major planes ``[n, rm_plane_words(h, w)]`` int32 in the layout of pack_masks (bit y*w + x; tail and pad bits zero),
    which pair_counts and the PNG selection front-end read: RLE masklets reach them without a uint8 stage.  One launch
    (sola_planes_cm_to_rm); every word of ``out`` is written whatever it held."""
    require_cuda(bits_cm)
    if bits_cm.dim() != 2 or bits_cm.dtype != torch.int32 or not bits_cm.is_contiguous():
        raise SolaError(f"planes_cm_to_rm: planes must be a contiguous int32 [n, words] tensor, got {bits_cm.dtype} {tuple(bits_cm.shape)}")
    n, stride = bits_cm.shape
    words = rm_plane_words(h, w)
    if out is None:
        out = torch.empty((n, words), device=bits_cm.device, dtype=torch.int32)
    elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n and
              out.shape[1] >= words):
        raise SolaError(f"planes_cm_to_rm: out must be a contiguous int32 device tensor [{n}, >= {words}]")
    if n:
        check(lib().sola_planes_cm_to_rm(ptr(bits_cm), stride, n, h, w, ptr(out), out.shape[1], current_stream(bits_cm.device)),
              "sola_planes_cm_to_rm")
    return out


def _png_levels(who, masklets, lists, ends, K, device, max_plane_bytes, max_scratch_bytes):
    """The PNG path under encode_png_selections and encode_png_sweep: ``out[e][k][t]`` = the complete PNG file (bytes) of frame
    t of the OR over ``lists[e][:ends[e][k]]``; ``ends[e]`` holds K non-decreasing prefix lengths.  Per group of _plane_groups
    (every referenced track parsed and decoded once): one sola_planes_cm_to_rm, then for blocks of (expressions, at most
    SOLA_NESTED_MAX_LEVELS levels) whose scratch stays under ``max_scratch_bytes`` (a single expression's block runs alone
    whatever it needs) one int32 upload of the lists, sola_png_deflate_sizes_select, one host read of the offsets,
    sola_png_deflate_write and one copy of the streams.  A later block of levels starts from the whole prefix of its first."""
    E, M = len(lists), len(masklets)
    if M == 0:
        raise SolaError(f"{who}: no masklets")
    for s in lists:
        for i in s:
            if not 0 <= int(i) < M:
                raise SolaError(f"{who}: index {i} outside the {M} masklets")
    T, size = _masklet_geometry(masklets)
    if size is None:
        raise SolaError(f"{who}: every frame of every masklet is missing: there is no size to write a PNG at")
    if E == 0 or T == 0:
        return [[[] for _ in range(K)] for _ in range(E)]
    h, w = size
    L = lib()
    dev = torch.device(device)
    stream = current_stream(dev)
    stride_cm, stride_rm = L.sola_jf_plane_words(h, w), rm_plane_words(h, w)
    head = b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
    tail = _png_chunk(b"IEND", b"")
    preds = [[int(i) for i in lists[e][:ends[e][-1]]] for e in range(E)]  # what the largest level selects
    NL = 16  # SOLA_NESTED_MAX_LEVELS
    out = [[None] * K for _ in range(E)]
    for grp, local, bits_cm, n_ids in _plane_groups(masklets, preds, T, h, w, stride_cm, dev, max_plane_bytes):
        if n_ids:
            bits = planes_cm_to_rm(bits_cm, h, w)
        else:  # no expression of the group selects a track: no plane is read
            bits = torch.zeros((1, stride_rm), device=dev, dtype=torch.int32)
        del bits_cm
        for k0 in range(0, K, NL):
            kc = min(NL, K - k0)
            fit = 1
            while fit < len(grp) and L.sola_png_deflate_scratch_bytes((fit + 1) * kc * T, h, w) <= max_scratch_bytes:
                fit += 1
            for b0 in range(0, len(grp), fit):
                blk = grp[b0:b0 + fit]
                off, idx, lend = [0], [], []
                for e in blk:
                    idx += [local[i] for i in preds[e][:ends[e][k0 + kc - 1]]]
                    off.append(len(idx))
                    lend += ends[e][k0:k0 + kc]
                parts = [lend, off, idx + [0]]  # (the pad entry keeps the pointer of an empty list non-null)
                ints = torch.tensor([x for part in parts for x in part], dtype=torch.int32).to(dev)  # one copy for every list
                d, o = [], 0
                for part in parts:
                    d.append(ptr(ints[o:o + len(part)]))
                    o += len(part)
                n = len(blk) * kc * T
                nb = L.sola_png_deflate_scratch_bytes(n, h, w)
                scratch = _stream_scratch("png_select", dev, max(nb, 8), torch.int64)
                byte_off = torch.empty((n + 1,), device=dev, dtype=torch.int64)
                adler = torch.empty((n,), device=dev, dtype=torch.int32)
                check(L.sola_png_deflate_sizes_select(ptr(bits), stride_rm, n_ids, T, h, w, d[1], d[2], d[0], kc, len(blk), ptr(byte_off),
                                                      ptr(adler), ptr(scratch), nb, stream), "sola_png_deflate_sizes_select")
                offs = byte_off.cpu().tolist()  # the host read: every stream's first byte, offs[n] = the size of the buffer
                data = torch.empty((offs[n],), device=dev, dtype=torch.uint8)
                check(L.sola_png_deflate_write(ptr(bits), 0, n, h, w, ptr(byte_off), ptr(adler), ptr(data), ptr(scratch), nb, stream),
                      "sola_png_deflate_write")
                data = data.cpu().numpy().tobytes()
                for j, e in enumerate(blk):
                    for k in range(kc):
                        s0 = (j * kc + k) * T
                        out[e][k0 + k] = [head + _png_chunk(b"IDAT", data[offs[s0 + t]:offs[s0 + t + 1]]) + tail for t in range(T)]
    return out


@torch.no_grad()
def encode_png_selections(masklets, pred_sets, device, max_plane_bytes=2 << 30, max_scratch_bytes=1 << 30):
    """``out[e][t]``: the PNG file (bytes) of frame t of the OR of ``masklets[i]`` for i in ``pred_sets[e]`` - byte for byte the
    files of ``encode_png_masklet(rle_merge_or([masklets[i] for i in pred_sets[e]], device))``, for every expression of a video
    from ONE parse and ONE decode of the tracks some expression selects (``masklets`` as masklet_select_counts takes them).  No
    ``[T,h,w]`` masklet is materialised: the decoded bit planes are transposed to row-major once (planes_cm_to_rm) and the PNG
    encoder's bitmap front-end ORs a selection's planes while it reads them (sola_png_deflate_sizes_select).  An empty
    selection gives all-zero frames; masklets without any sized frame raise SolaError (there is nothing to size a PNG by).
    This is encode_png_sweep's path with one level that ends at the list's end."""
    lists = [list(s) for s in pred_sets]
    return [ek[0] for ek in _png_levels("encode_png_selections", masklets, lists, [[len(s)] for s in lists], 1, device, max_plane_bytes,
                                        max_scratch_bytes)]


@torch.no_grad()
def encode_png_sweep(masklets, cand_sets, probs, thresholds, device, max_plane_bytes=2 << 30, max_scratch_bytes=1 << 30):
    """encode_png_selections at every threshold of a sweep from one decode: ``out[e][j][t]`` is the PNG file (bytes) of frame t
    of the OR of {``masklets[cand_sets[e][i]]`` : ``probs[e][i]`` > ``thresholds[j]``} (float32, strict: the rule of sweep_levels
    and of ops.select), thresholds in the caller's order.  The selections at descending thresholds are nested, so each track of
    the largest one is decoded once per group of expressions and read once per (expression, frame) and 16 levels: the encoder's
    front-end carries the OR from level to level and emits every level's raw bitmap."""
    import numpy as np
    E, K = len(cand_sets), len(thresholds)
    if K == 0:
        raise SolaError("encode_png_sweep: no thresholds")
    if len(probs) != E:
        raise SolaError(f"encode_png_sweep: {E} candidate sets but {len(probs)} score vectors")
    ordered, ends, perm = [], [], np.arange(K)
    for e in range(E):
        if len(probs[e]) != len(cand_sets[e]):
            raise SolaError(f"encode_png_sweep: expression {e} has {len(cand_sets[e])} tracks but {len(probs[e])} scores")
        order, level_end, perm = sweep_levels(probs[e], thresholds)
        rest = np.setdiff1d(np.arange(len(probs[e])), order)  # never selected: range-checked with the others, never read
        ordered.append([cand_sets[e][i] for i in order] + [cand_sets[e][i] for i in rest])
        ends.append(level_end.tolist())
    levels = _png_levels("encode_png_sweep", masklets, ordered, ends, K, device, max_plane_bytes, max_scratch_bytes)
    return [[le[int(perm[j])] for j in range(K)] for le in levels]


# ----------------------------------------------------------------------------------------------------------------
# connected components, SAM2's fill_holes_in_mask_scores, small-region removal (components.hip)
# ----------------------------------------------------------------------------------------------------------------
CC_TILE = (16, 64)  # (rows, columns) of the labelling kernel's tile: include/sola_hip.h SOLA_CC_TILE_H / _W


def _cc_frames(t, what):
    """[N,1,H,W] (SAM2's layout) or [N,H,W] -> contiguous [N,H,W] on the GPU and the caller's shape."""
    shape = tuple(t.shape)
    if not (t.dim() == 3 or (t.dim() == 4 and shape[1] == 1)):
        raise SolaError(f"{what}: masks must be (N,1,H,W) or (N,H,W), got {shape}")
    t = _prep(t)
    return t.reshape(shape[0], shape[-2], shape[-1]), shape


def _cc_scratch(dev, n, h, w, scratch):
    nb = lib().sola_mask_components_scratch_bytes(n, h, w)
    if scratch is not None:  # the caller's own (tests): a contiguous uint8 device tensor
        return scratch, scratch.numel()
    scratch = _stream_scratch("cc", dev, nb, floor=256)
    return scratch, scratch.numel()


@torch.no_grad()
def connected_components(mask, connectivity=8, logits=False, scratch=None):
    """The binding for ``sam2.utils.misc.get_connected_components``: mask (N,1,H,W) or (N,H,W) on the GPU, uint8 / bool /
    float32 (set where != 0) -> ``(labels, areas)``, int32 tensors of the input's shape.  ``labels`` is 0 on clear pixels and,
    on set pixels, 1 + (y*W + x) of the component's first pixel in raster order within its own frame; ``areas`` is 0 on
    clear pixels and the pixel count of the pixel's component elsewhere.  The N frames are labelled independently in one
    library call; ``connectivity`` is 8 (SAM2's) or 4; ``logits=True`` counts float32 ``> 0``."""
    m, shape = _cc_frames(mask, "connected_components")
    et = _mask_kind(m, logits)
    n, h, w = m.shape
    dev = m.device
    out = torch.empty((2, n, h, w), device=dev, dtype=torch.int32)
    scratch, nb = _cc_scratch(dev, n, h, w, scratch)
    check(lib().sola_mask_components(ptr(m), et, n, h, w, int(connectivity), ptr(out[0]), ptr(out[1]), ptr(scratch), nb,
                                     current_stream(dev)), "sola_mask_components")
    return out[0].reshape(shape), out[1].reshape(shape)


def _fill_small(m, et, connectivity, max_area, fill_value, out, scratch):
    n, h, w = m.shape
    dev = m.device
    scratch, nb = _cc_scratch(dev, n, h, w, scratch)
    check(lib().sola_mask_fill_small(ptr(m), et, n, h, w, int(connectivity), int(max_area), float(fill_value), ptr(out), ptr(scratch),
                                     nb, current_stream(dev)), "sola_mask_fill_small")
    return out


@torch.no_grad()
def fill_holes_in_mask_scores(mask, max_area, fill_value=0.1, connectivity=8, out=None, scratch=None):
    """The binding for ``sam2.utils.misc.fill_holes_in_mask_scores``: float32 mask scores (N,1,H,W) or (N,H,W) -> a new
    tensor of the same shape in which every background component (scores <= 0, 8-connected) of at most ``max_area`` pixels
    holds ``fill_value``; every other score passes through bit for bit.  ``out``: the tensor to write instead of a new one;
    ``out=mask`` (contiguous) rewrites in place.  There is no fallback and no warning path."""
    if max_area <= 0:
        raise SolaError(f"fill_holes_in_mask_scores: max_area must be positive, got {max_area}")
    if mask.dtype != torch.float32:
        raise SolaError(f"fill_holes_in_mask_scores: scores must be float32, got {mask.dtype}")
    m, shape = _cc_frames(mask, "fill_holes_in_mask_scores")
    if out is None:
        out = torch.empty_like(m)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == m.numel()):
        raise SolaError("fill_holes_in_mask_scores: out must be a contiguous float32 device tensor of the input's size")
    return _fill_small(m, 3, connectivity, max_area, fill_value, out, scratch).reshape(shape)


@torch.no_grad()
def remove_small_regions(masks, max_area, mode, connectivity=8, scratch=None):
    """{0,1} masks (N,1,H,W) or (N,H,W), uint8 / bool / float32 -> a new tensor of the same shape and dtype.
    ``mode="islands"``: set components of at most ``max_area`` pixels are cleared.  ``mode="holes"``: clear components of
    at most ``max_area`` pixels are set to 1, those cut by the image border included; the complement is taken on read in
    the kernel.  These semantics are this library's own."""
    if mode not in ("holes", "islands"):
        raise SolaError(f"remove_small_regions: mode must be 'holes' or 'islands', got {mode!r}")
    if max_area < 0:
        raise SolaError(f"remove_small_regions: max_area must not be negative, got {max_area}")
    m, shape = _cc_frames(masks, "remove_small_regions")
    et = _elem_type(m) + (4 if mode == "holes" else 0)
    out = _fill_small(m, et, connectivity, max_area, 0.0, torch.empty_like(m), scratch).reshape(shape)
    return out.view(torch.bool) if masks.dtype == torch.bool else out


# ----------------------------------------------------------------------------------------------------------------
# the grid-prompt stage (generate_prompts_grid.py; SAM2's automatic mask generator): per-mask statistics from one read of
# the logits, box NMS, the part filter, uncompressed RLE (amg.hip; the part filter and the RLE ride on kernels above)
# ----------------------------------------------------------------------------------------------------------------
NMS_MAX_BOXES = 16384  # include/sola_hip.h SOLA_BOX_NMS_MAX_N


def _f32(x):
    """A Python double rounded once to float32: what ``tensor_f32 > python_float`` compares against in torch and numpy."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


@torch.no_grad()
def mask_logit_stats(masks, mask_threshold=0.0, threshold_offset=1.0, logits=True):
    """(N,H,W) or (N,1,H,W) on the GPU -> int64 [N,7] device tensor (n_hi, n_lo, area, x0, y0, x1, y1) from ONE read of the
    masks (sola_mask_logit_stats).  ``logits=True``: float32 mask logits; the three counts are the pixels strictly above
    mask_threshold + threshold_offset, mask_threshold - threshold_offset and mask_threshold (each sum formed in Python double
    and rounded once to float32), NaN never counting.  ``logits=False``: uint8 / bool / float32 masks set where != 0; all
    three counts are the area.  (x0, y0, x1, y1) is the inclusive box of the pixels counted in ``area``, (0, 0, 0, 0) for an
    empty mask."""
    et = _mask_kind(masks, logits, "mask_logit_stats")
    m, _ = _cc_frames(masks, "mask_logit_stats")
    n, h, w = m.shape
    stats = torch.empty((n, 7), device=m.device, dtype=torch.int64)
    check(lib().sola_mask_logit_stats(ptr(m), et, n, h, w, _f32(mask_threshold), _f32(mask_threshold + threshold_offset),
                                      _f32(mask_threshold - threshold_offset), ptr(stats), current_stream(m.device)),
          "sola_mask_logit_stats")
    return stats


def calculate_stability_score(masks, mask_threshold, threshold_offset):
    """The binding for ``sam2.utils.amg.calculate_stability_score`` (and prompt_generator.get_stability_score without its host
    copy): float32 logits (N,H,W) / (N,1,H,W) -> float32 [N] on the device = |x > thr + off| / |x > thr - off|; 0/0 is nan,
    as in SAM2."""
    stats = mask_logit_stats(masks, mask_threshold, threshold_offset)
    return stats[:, 0].float() / stats[:, 1].float()


def batched_mask_to_box(masks):
    """The binding for ``sam2.utils.amg.batched_mask_to_box``: bool / uint8 masks (N,H,W) or (N,1,H,W) -> int64 [N,4] XYXY
    (inclusive corners), (0, 0, 0, 0) for an empty mask."""
    if masks.dtype not in (torch.bool, torch.uint8):
        raise SolaError(f"batched_mask_to_box: masks must be bool or uint8, got {masks.dtype}")
    return mask_logit_stats(masks, logits=False)[:, 3:7]


def box_area(boxes):
    """torchvision.ops.boxes.box_area: [N,4] XYXY -> [N]."""
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


@torch.no_grad()
def batched_nms(boxes, scores, idxs, iou_threshold, scratch=None):
    """torchvision.ops.boxes.batched_nms on libsola_hip.so: boxes float32 [N,4] XYXY, scores [N], idxs [N] integer categories
    (None = one category) -> int64 indices of the kept boxes by decreasing score.  A box is dropped when a kept box of its
    own category with a higher score overlaps it by IoU > iou_threshold (float32, include/sola_hip.h gives the order of the
    operations); categories never interact.  The visiting order is ``torch.sort(scores, descending=True, stable=True)`` on the
    device: boxes of equal score are visited lower index first.  That tie rule is this library's own choice; torchvision
    leaves ties unspecified.  One host read (the number kept) per call; at most NMS_MAX_BOXES boxes."""
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise SolaError(f"nms: boxes must be [N,4], got {tuple(boxes.shape)}")
    if boxes.dtype != torch.float32:
        raise SolaError(f"nms: boxes must be float32, got {boxes.dtype}")
    n = boxes.shape[0]
    if scores.dim() != 1 or scores.shape[0] != n:
        raise SolaError(f"nms: scores must be [{n}], got {tuple(scores.shape)}")
    if idxs is not None:
        if idxs.dim() != 1 or idxs.shape[0] != n:
            raise SolaError(f"nms: idxs must be [{n}], got {tuple(idxs.shape)}")
        if idxs.dtype.is_floating_point or idxs.dtype == torch.bool:
            raise SolaError(f"nms: idxs must be integers, got {idxs.dtype}")
    require_cuda(boxes, scores, idxs)
    if idxs is not None:
        idxs = idxs.to(torch.int64).contiguous()
    if n > NMS_MAX_BOXES:
        raise SolaError(f"nms: {n} boxes, at most {NMS_MAX_BOXES} in one call")
    dev = boxes.device
    boxes = boxes.contiguous()
    order = torch.sort(scores, descending=True, stable=True).indices.contiguous()
    out = torch.empty((n + 1,), device=dev, dtype=torch.int64)  # n_keep, then the kept indices
    nb = lib().sola_box_nms_scratch_bytes(n)
    if scratch is None:
        scratch = _stream_scratch("nms", dev, nb, torch.int64, floor=32)
    check(lib().sola_box_nms(ptr(boxes), ptr(order), ptr(idxs), n, float(iou_threshold), ptr(out[1:]), ptr(out), ptr(scratch),
                             scratch.numel() * scratch.element_size(), current_stream(dev)), "sola_box_nms")
    return out[1:1 + int(out[0])]  # the host read


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: batched_nms with one category."""
    return batched_nms(boxes, scores, None, iou_threshold)


@torch.no_grad()
def filter_part_masks(masks, thresh=0.7):
    """The part filter of generate_prompts_grid.py:105-116: masks (N,H,W) {0,1} on the GPU, sorted by area descending by the
    caller -> bool [N] CPU tensor ``is_part``, element for element what the reference's loop of N-1 ``compute_P`` calls leaves.
    All N x N intersections come from one pack launch, one pair launch and one copy (the areas are the diagonal); the
    order-dependent loop runs on the host over the integers, with the reference's float32 ratio and comparison."""
    import numpy as np
    if masks.dim() != 3:
        raise SolaError(f"filter_part_masks: masks must be (N,H,W), got {tuple(masks.shape)}")
    _elem_type(masks)
    masks = _prep(masks)
    n = masks.shape[0]
    is_part = np.zeros(n, bool)
    if n < 2:
        return torch.from_numpy(is_part)
    bits, area = pack_masks(masks)
    inter, _ = pair_counts(bits, area, bits, area)
    inter = inter.cpu().numpy()  # inter[p, f] = |mask p & mask f|
    area = np.diagonal(inter).astype(np.float32)
    t = np.float32(thresh)
    with np.errstate(invalid="ignore", divide="ignore"):
        for full in range(n - 1):
            if is_part[full]:
                continue
            P = inter[:, full].astype(np.float32) / area  # 0/0 = nan: never marked
            is_part[P > t] = True
            is_part[full] = False
    return torch.from_numpy(is_part)


@torch.no_grad()
def mask_to_rle_uncompressed(masks, logits=False):
    """``sam2.utils.amg.mask_to_rle_pytorch``: (N,h,w) masks on the GPU -> list of ``{"size": [h, w], "counts": [int, ...]}``,
    the runs of the column-major flattening starting with a (possibly empty) run of zeros.  Built from
    encode_rle_masklet(..., return_cum=True): one copy of the prefix sums and offsets, differences on the host."""
    import numpy as np
    cum, run_off = encode_rle_masklet(masks, logits, return_cum=True)
    n, h, w = masks.shape
    if n == 0:
        return []
    both = torch.cat([run_off, cum.to(torch.int64) & 0xFFFFFFFF]).cpu().numpy()  # (cum holds uint32 in int32)
    off, c = both[:n + 1], both[n + 1:]
    out = []
    for i in range(n):
        ends = c[off[i]:off[i + 1]]  # ends with h*w: the last run closes the frame
        out.append({"size": [h, w], "counts": np.diff(ends, prepend=0).tolist()})
    return out


# ----------------------------------------------------------------------------------------------------------------
# index maps (the palette-PNG ground truth of Ref-DAVIS / Ref-YouTube-VOS: one byte per pixel = the object id) -> masklets
# ----------------------------------------------------------------------------------------------------------------
INDEX_ID_CHUNK = 8          # SOLA_INDEX_ID_CHUNK: the ids sola_index_pack compares in one pass over a staged piece
_INDEX_LAYOUTS = {"row": 0, "cm": 1}


def _index_maps(index_maps):
    require_cuda(index_maps)
    if index_maps.dtype != torch.uint8 or index_maps.dim() != 3:
        raise SolaError(f"index maps must be uint8 [T,h,w], got {index_maps.dtype} {tuple(index_maps.shape)}")
    return index_maps.contiguous()


@torch.no_grad()
def index_hist(index_maps):
    """uint8 [T,h,w] on the GPU -> int64 [T,256] on the device: the pixels of every value in every frame, from one read of
    the maps (sola_index_hist)."""
    maps = _index_maps(index_maps)
    T, h, w = maps.shape
    counts = torch.empty((T, 256), device=maps.device, dtype=torch.int64)
    check(lib().sola_index_hist(ptr(maps), T, h, w, ptr(counts), current_stream(maps.device)), "sola_index_hist")
    return counts


def object_ids_from_hist(hist, rule):
    """The object ids of a video from its [T,256] histogram (any array-like, on the host).  ``rule="davis"``: the values
    present in frame 0, minus 0 and 255 (dataloader.py:266-267, np.unique of the first annotation).  ``rule="ytbvos"``: the
    values 1..255 with a pixel in any frame (track_generation/seg_utils.py:37-48)."""
    import numpy as np
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != 256:
        raise ValueError(f"histogram must be [T,256], got {hist.shape}")
    if rule == "davis":
        return [v for v in range(1, 255) if len(hist) and hist[0, v] > 0]
    if rule == "ytbvos":
        total = hist.sum(axis=0)
        return [v for v in range(1, 256) if total[v] > 0]
    raise ValueError(f"unknown rule {rule!r}: 'davis' or 'ytbvos'")


def index_object_ids(index_maps, rule):
    """Host list of the object ids in ``index_maps`` under ``rule`` (object_ids_from_hist): one index_hist and one copy."""
    return object_ids_from_hist(index_hist(index_maps).cpu().numpy(), rule)


@torch.no_grad()
def pack_index_masklets(index_maps, ids, layout="row", out=None, first_plane=None):
    """(bits int32 [planes, words], area int64 [planes] or None): plane ``k*T + t`` (``first_plane[k] + t`` when given) is
    ``index_maps[t] == ids[k]``, every id from one read of the maps (sola_index_pack).  ``layout="row"`` is the pack_masks /
    pair_counts format and also returns the planes' areas; ``"cm"`` is the column-major format of masklet_select_counts
    (area None).  ``out``: an int32 [rows, words] buffer to write into (the rows not addressed keep their content);
    ``first_plane``: a host list of K first rows, whose ranges of T rows must be disjoint and inside ``out``.  ``ids``: a host
    list or an int32 device tensor; a value outside 0..255 gives empty planes."""
    if layout not in _INDEX_LAYOUTS:
        raise SolaError(f"layout {layout!r}: 'row' or 'cm'")
    maps = _index_maps(index_maps)
    T, h, w = maps.shape
    dev = maps.device
    L = lib()
    if torch.is_tensor(ids):
        require_cuda(ids)
        d_ids = ids.to(torch.int32).contiguous()
    else:
        d_ids = torch.tensor([int(i) for i in ids], dtype=torch.int32).to(dev)
    K = d_ids.numel()
    words = L.sola_mask_words(h, w) if layout == "row" else L.sola_jf_plane_words(h, w)
    if out is None:
        if first_plane is not None:
            raise SolaError("pack_index_masklets: first_plane needs out")
        out = torch.empty((K * T, words), device=dev, dtype=torch.int32)
    else:
        require_cuda(out)
        if out.dtype != torch.int32 or out.dim() != 2 or not out.is_contiguous() or out.shape[1] < words:
            raise SolaError(f"pack_index_masklets: out must be a contiguous int32 [rows, >= {words}] tensor")
    d_first = None
    if first_plane is not None:
        first = [int(p) for p in first_plane]
        rows = sorted(first)
        if len(first) != K or any(p < 0 or p + T > out.shape[0] for p in first) or any(b - a < T for a, b in zip(rows, rows[1:])):
            raise SolaError("pack_index_masklets: first_plane must give K disjoint ranges of T rows inside out")
        d_first = torch.tensor(first, dtype=torch.int32).to(dev)
    elif K * T > out.shape[0]:
        raise SolaError(f"pack_index_masklets: out has {out.shape[0]} rows, {K * T} needed")
    area = torch.zeros((out.shape[0],), device=dev, dtype=torch.int64) if layout == "row" else None
    check(L.sola_index_pack(ptr(maps), T, h, w, ptr(d_ids), K, ptr(d_first), _INDEX_LAYOUTS[layout], out.shape[1], ptr(out),
                            ptr(area), current_stream(dev)), "sola_index_pack")
    return out, area


@torch.no_grad()
def index_masklets(index_maps, ids=None, reshape=False, target_shape=None):
    """``get_masklets_ytbvos`` (track_generation/seg_utils.py:29-49) on the GPU: ``{str(id): float32 {0,1} [T,H,W]}`` of the
    objects in uint8 index maps [T,h,w]; objects that are empty over the whole video are dropped.  ``ids=None``: the values
    1..255 that occur (index_object_ids' "ytbvos" rule).  One histogram pass finds the objects, one pack launch compares
    every id (row-major planes), unpack_masks writes the images.  ``reshape=True``: each masklet goes through
    pack_masklet_bilinear, so the result is reshape_masklet's on ``(index_maps == id)`` bit for bit."""
    maps = _index_maps(index_maps)
    T, h, w = maps.shape
    total = index_hist(maps).sum(dim=0).cpu().numpy()
    ids = [v for v in range(1, 256) if total[v] > 0] if ids is None else [int(i) for i in ids]
    keep = list(dict.fromkeys(i for i in ids if 0 <= i <= 255 and total[i] > 0))
    if not keep or T == 0:
        return {}
    bits, _ = pack_index_masklets(maps, keep, "row")
    out = {}
    if not reshape:
        images = unpack_masks(bits, h, w, torch.float32).view(len(keep), T, h, w)
        for k, i in enumerate(keep):
            out[str(i)] = images[k]
        return out
    images = unpack_masks(bits, h, w, torch.uint8).view(len(keep), T, h, w)
    for k, i in enumerate(keep):
        out[str(i)] = reshape_masklet(images[k], target_shape)
    return out


class IndexMasklet:
    """A masklet given as ``index_maps == obj_id`` (uint8 [T,h,w] on the GPU, e.g. the frames of a Ref-DAVIS annotation
    folder): masklet_select_counts / compute_JF_batch take it as an element of ``masklets`` in place of a list of RLE dicts.
    IndexMasklets that share one ``index_maps`` tensor are compared in one sola_index_pack launch."""

    def __init__(self, index_maps, obj_id):
        self.index_maps = _index_maps(index_maps)
        self.obj_id = int(obj_id)

    def __len__(self):
        return int(self.index_maps.shape[0])

    @property
    def size(self):
        return (int(self.index_maps.shape[1]), int(self.index_maps.shape[2]))
