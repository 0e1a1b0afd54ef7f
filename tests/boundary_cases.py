"""The DAVIS boundary (contour) F-measure restated in numpy for the tests, for two binary masks of one size and no void
pixels:

  boundary map   B[y, x] = 1 iff m[y, x] differs from an in-image neighbour among east (y, x+1), south (y+1, x) and
                 south-east (y+1, x+1): interior pixels test three, the last row east only, the last column south only,
                 the bottom-right pixel none
  radius         bound_th itself when >= 1, else ceil(bound_th * sqrt(h*h + w*w))
  dilation       by the disk dy*dy + dx*dx <= r*r; positions outside the image contribute nothing
  counts         n_fg = |B(fg)|, n_gt = |B(gt)|, fg_match = |B(fg) & dil(B(gt))|, gt_match = |B(gt) & dil(B(fg))|
  F              precision = fg_match / n_fg, recall = gt_match / n_gt with the empty-boundary conventions below;
                 2PR / (P + R), 0 when P + R = 0; a masklet's F is the mean over its frames."""
import numpy as np


def boundary_map(m):
    m = np.asarray(m) != 0
    b = np.zeros(m.shape, bool)
    b[:, :-1] |= m[:, :-1] != m[:, 1:]       # east
    b[:-1, :] |= m[:-1, :] != m[1:, :]       # south
    b[:-1, :-1] |= m[:-1, :-1] != m[1:, 1:]  # south-east
    return b


def radius(h, w, bound_th=0.008):
    return int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.sqrt(np.float64(h * h + w * w))))


def disk(r):
    d = np.arange(-r, r + 1)
    return (d[:, None] ** 2 + d[None, :] ** 2) <= r * r


def disk_dilate(b, r):
    """OR of the shifted copies of ``b``, one per disk offset (slices: nothing wraps, nothing enters from outside)."""
    b = np.asarray(b) != 0
    h, w = b.shape
    out = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx > r * r or abs(dy) >= h or abs(dx) >= w:
                continue
            # out[y, x] |= b[y + dy, x + dx]
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            out[yd, xd] |= b[ys, xs]
    return out


def disk_dilate_rows(b, r):
    """The same dilation by row spans, for large frames: per dy one horizontally widened OR (a running sum over x)."""
    b = np.asarray(b) != 0
    h, w = b.shape
    cum = np.zeros((h, w + 1), np.int32)
    np.cumsum(b, axis=1, out=cum[:, 1:])
    xs = np.arange(w)
    out = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        if abs(dy) >= h:
            continue
        u = int(np.floor(np.sqrt(r * r - dy * dy)))
        while (u + 1) ** 2 + dy * dy <= r * r:  # (guards the float square root)
            u += 1
        while u * u + dy * dy > r * r:
            u -= 1
        wide = (cum[:, np.minimum(xs + u + 1, w)] - cum[:, np.maximum(xs - u, 0)]) > 0  # any b[y, x-u .. x+u]
        if dy >= 0:
            out[:h - dy] |= wide[dy:]
        else:
            out[-dy:] |= wide[:h + dy]
    return out


def boundary_counts(fg, gt, r, dilate=disk_dilate):
    bf, bg = boundary_map(fg), boundary_map(gt)
    return np.array([bf.sum(), bg.sum(), (bf & dilate(bg, r)).sum(), (bg & dilate(bf, r)).sum()], np.int64)


def f_from_counts(c):
    n_fg, n_gt, fg_match, gt_match = (int(v) for v in c)
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision, recall = fg_match / n_fg, gt_match / n_gt
    return 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)


def masklet_f(fg, gt, bound_th=0.008, dilate=disk_dilate):
    """Mean over the frames of two [T,h,w] masklets."""
    r = radius(fg.shape[1], fg.shape[2], bound_th)
    return float(np.mean([f_from_counts(boundary_counts(a, b, r, dilate)) for a, b in zip(fg, gt)]))
