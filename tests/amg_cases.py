"""The grid-prompt stage's contracts (include/sola_hip.h, sola_amd/seg_utils.py) restated in plain numpy, and the cases the
tests run: per-mask statistics, greedy box NMS, the part filter, uncompressed RLE.  Written from the contracts; the GPU tests
demand equality with these."""
import numpy as np

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- statistics
def stats(maps, logits, thr=0.0, thr_hi=1.0, thr_lo=-1.0):
    """maps [n,h,w] -> int64 [n,7] = (n_hi, n_lo, area, x0, y0, x1, y1).  logits: float32 maps, a pixel counts for t when
    x > float32(t) (NaN never does); else it is set where != 0 and the three counts are the area.  The box is the inclusive
    bounding box of the pixels counted in area, (0, 0, 0, 0) when there are none."""
    maps = np.asarray(maps)
    out = np.zeros((maps.shape[0], 7), np.int64)
    for i, m in enumerate(maps):
        with np.errstate(invalid="ignore"):
            if logits:
                on, hi, lo = m > f32(thr), m > f32(thr_hi), m > f32(thr_lo)
            else:
                on = hi = lo = m != 0
        out[i, :3] = hi.sum(), lo.sum(), on.sum()
        if on.any():
            ys, xs = np.nonzero(on)
            out[i, 3:] = xs.min(), ys.min(), xs.max(), ys.max()
    return out


def f32_of(x):
    """A Python double rounded once to float32, as a Python float."""
    return float(f32(x))


def stat_masks(h, w, n_random=2, seed=0):
    """(names, uint8 [k,h,w]): empty, full, single pixels at the corners and in the last row / column, bars, random blobs,
    p = 0.5 noise."""
    rng = np.random.default_rng(seed * 1000 + h * 7 + w)
    names, ms = [], []

    def add(name, m):
        names.append(name)
        ms.append(m.astype(np.uint8))

    z = np.zeros((h, w), np.uint8)
    add("empty", z)
    add("full", z + 1)
    for name, (y, x) in (("top-left", (0, 0)), ("top-right", (0, w - 1)), ("bottom-left", (h - 1, 0)), ("bottom-right", (h - 1, w - 1)),
                         ("last-row", (h - 1, w // 2)), ("last-column", (h // 2, w - 1))):
        m = z.copy()
        m[y, x] = 1
        add(name, m)
    m = z.copy()
    m[h // 3, :] = 1
    add("row-bar", m)
    m = z.copy()
    m[:, (2 * w) // 3] = 1
    add("column-bar", m)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(n_random):
        m = z.copy()
        for _ in range(3):
            cy, cx = rng.integers(0, h), rng.integers(0, w)
            ry, rx = 1 + rng.integers(0, max(1, h // 3)), 1 + rng.integers(0, max(1, w // 3))
            m |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.uint8)
        add(f"blobs{k}", m)
    add("noise", rng.uniform(size=(h, w)) < 0.5)
    return names, np.stack(ms)


def threshold_logits(h, w, thr, thr_hi, thr_lo, seed=0):
    """One float32 map whose values sit exactly on the three thresholds, one ulp to either side of them, and on NaN, +-inf and
    both zeros."""
    t = [f32(thr), f32(thr_hi), f32(thr_lo)]
    vals = []
    for v in t:
        vals += [v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))]
    vals += [f32(np.nan), f32(np.inf), f32(-np.inf), f32(0.0), f32(-0.0)]
    rng = np.random.default_rng(seed + 31 * h + w)
    return np.asarray(vals, f32)[rng.integers(0, len(vals), size=(h, w))]


# -------------------------------------------------------------------------------------------------------------------- NMS
def visiting_order(scores):
    """Decreasing score, equal scores lower index first (a stable sort)."""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable").astype(np.int64)


def box_iou_f32(a, b):
    """The contract's IoU of two xyxy boxes: float32 scalars, every operation rounded on its own."""
    a = [f32(v) for v in a]
    b = [f32(v) for v in b]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area_a = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
        area_b = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
        iw = max(f32(0), f32(min(a[2], b[2]) - max(a[0], b[0])))
        ih = max(f32(0), f32(min(a[3], b[3]) - max(a[1], b[1])))
        inter = f32(iw * ih)
        return f32(inter / f32(f32(area_a + area_b) - inter))


def box_nms_loop(boxes, order, idxs, thr):
    """The textbook double loop, scalar by scalar: kept original indices in visiting order."""
    thr = f32(thr)
    keep = []
    for a in order:
        ok = True
        for b in keep:
            if idxs is not None and idxs[a] != idxs[b]:
                continue
            if box_iou_f32(boxes[b], boxes[a]) > thr:
                ok = False
                break
        if ok:
            keep.append(int(a))
    return keep


def box_nms(boxes, scores, idxs, thr):
    """box_nms_loop's answer from float32 ARRAY arithmetic (numpy rounds every array operation to float32, so each row of
    IoUs equals the scalar loop's): the form that is affordable at 3072 boxes."""
    boxes = np.asarray(boxes, f32)
    n = len(boxes)
    order = visiting_order(scores)
    b = boxes[order]
    cat = None if idxs is None else np.asarray(idxs)[order]
    thr = f32(thr)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        dead = np.zeros(n, bool)
        keep = []
        for i in range(n):
            if dead[i]:
                continue
            keep.append(int(order[i]))
            r = b[i + 1:]
            iw = np.maximum(f32(0), np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]))
            ih = np.maximum(f32(0), np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]))
            inter = iw * ih
            iou = inter / ((area[i] + area[i + 1:]) - inter)
            assert iou.dtype == f32
            hit = iou > thr
            if cat is not None:
                hit &= cat[i + 1:] == cat[i]
            dead[i + 1:] |= hit
    return keep


def rect_boxes(n, seed, size=2048):
    """Inclusive corner boxes of random rectangles in a size x size image (what batched_mask_to_box returns): integers, every
    product and sum of the IoU exact in float32; zero-area boxes (one row or one column) and identical boxes included."""
    rng = np.random.default_rng(seed)
    cx, cy = rng.integers(0, size, n), rng.integers(0, size, n)
    bw, bh = rng.integers(0, size // 4, n), rng.integers(0, size // 4, n)
    thin = rng.uniform(size=n) < 0.05
    bw[thin] = 0
    bh[rng.uniform(size=n) < 0.05] = 0
    b = np.stack([cx, cy, np.minimum(cx + bw, size - 1), np.minimum(cy + bh, size - 1)], 1).astype(f32)
    if n > 3:  # duplicates, and clusters of near-duplicates so that suppression chains form
        src = rng.integers(0, n, n // 3)
        dst = rng.integers(0, n, n // 3)
        b[dst] = b[src]
        jit = rng.integers(0, n, n // 3)
        b[jit] = np.clip(b[rng.integers(0, n, n // 3)] + rng.integers(-3, 4, (n // 3, 4)), 0, size - 1)
        b[:, 2] = np.maximum(b[:, 0], b[:, 2])
        b[:, 3] = np.maximum(b[:, 1], b[:, 3])
    return np.ascontiguousarray(b, f32)


def float_boxes(n, seed):
    """Finite float32 boxes in [0, 2000): clusters around a few centres, x0 <= x1 and y0 <= y1."""
    rng = np.random.default_rng(seed + 77)
    k = max(1, n // 8)
    c = rng.uniform(100, 1900, (k, 2))
    which = rng.integers(0, k, n)
    ctr = c[which] + rng.normal(0, 6, (n, 2))
    half = np.abs(rng.normal(40, 10, (n, 2))) + 0.5
    b = np.concatenate([ctr - half, ctr + half], 1)
    return np.ascontiguousarray(np.clip(b, 0, np.nextafter(f32(2000), f32(0))), f32)


def tied_scores(n, seed):
    """float32 scores on a grid of about n/4 values: many ties."""
    rng = np.random.default_rng(seed + 5)
    return (rng.integers(0, max(2, n // 4), n) / 64.0).astype(f32)


def categories(n, k, seed):
    rng = np.random.default_rng(seed + 9)
    if k >= n:
        return rng.permutation(n).astype(np.int64)
    return rng.integers(0, k, n).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ part filter
def compute_P(part_masks, full_mask):
    """float32(|part & full|) / float32(|part|) per part mask; 0/0 = nan."""
    p = np.asarray(part_masks) != 0
    g = np.asarray(full_mask) != 0
    inter = (p & g[None]).reshape(len(p), -1).sum(1).astype(f32)
    area = p.reshape(len(p), -1).sum(1).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / area


def filter_part(masks, thresh=0.7):
    """The loop of generate_prompts_grid.py's part filter, step for step: bool [N].  The N calls of compute_P read one table
    of intersections (exact integers from a float64 product) instead of the masks."""
    n = len(masks)
    flat = (np.asarray(masks) != 0).reshape(n, -1).astype(np.float64)
    inter = np.rint(flat @ flat.T).astype(np.int64)  # inter[p, f] = |mask p & mask f|
    area = np.diagonal(inter).astype(f32)
    is_part = np.zeros(n, bool)
    for idx in range(n - 1):
        if is_part[idx]:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            P = inter[:, idx].astype(f32) / area  # compute_P(masks, masks[idx])
            is_part[P > f32(thresh)] = True
        is_part[idx] = False
    return is_part


def part_masks(n, h, w, seed):
    """n {0,1} masks sorted by area descending: nested ellipses, duplicates, one empty mask, and pairs whose part-ness is
    exactly 7/10."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ms = []
    while len(ms) < n:
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        ry, rx = rng.integers(4, h // 2), rng.integers(4, w // 2)
        outer = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1)
        ms.append(outer)
        for _ in range(int(rng.integers(0, 4))):  # parts: smaller ellipses around the same centre, some sticking out
            s = rng.uniform(0.2, 0.9)
            dy, dx = rng.integers(-ry // 2, ry // 2 + 1), rng.integers(-rx // 2, rx // 2 + 1)
            ms.append((((yy - cy - dy) / (ry * s)) ** 2 + ((xx - cx - dx) / (rx * s)) ** 2 <= 1))
    ms = ms[:n]
    if n >= 4:
        ms[1] = ms[0].copy()  # a duplicate
        ms[n - 1] = np.zeros((h, w), bool)  # an empty mask
    if n >= 8:  # a 10 x 10 block and a bar of 10 pixels with exactly 7 inside it
        full = np.zeros((h, w), bool)
        full[5:15, 5:15] = True
        part = np.zeros((h, w), bool)
        part[14, 8:18] = True
        ms[2], ms[3] = full, part
    ms = np.stack(ms).astype(np.uint8)
    order = np.argsort(-ms.reshape(n, -1).sum(1, dtype=np.int64), kind="stable")
    return np.ascontiguousarray(ms[order])


# -------------------------------------------------------------------------------------------------------- uncompressed RLE
def rle_uncompressed(mask):
    """{"size": [h, w], "counts": runs of the column-major flattening, zeros first (possibly a run of 0)}."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    flat = m.T.reshape(-1)
    counts, cur, run = [], False, 0
    for v in flat.tolist():
        if v != cur:
            counts.append(run)
            cur, run = v, 0
        run += 1
    counts.append(run)
    return {"size": [h, w], "counts": counts}
