"""The contract of sola_mask_components / sola_mask_fill_small (include/sola_hip.h) restated in numpy and plain Python, and
the frames the CPU and GPU tests share.

label(): a run-based two-pass union-find.  Pass 1 cuts every row into runs of set pixels and unions each run with the runs of
the previous row it overlaps (8-connectivity: overlaps after widening by one pixel on each side); runs are numbered in raster
order of their first pixel and a union keeps the smaller number, so a component's root is the run holding its first pixel.
Pass 2 writes, on every set pixel, 1 + the raster index of that first pixel and the component's pixel count.  Only the runs
are visited in Python, which keeps a 540x960 serpentine or noise frame within a second or two."""
import numpy as np

TILE = (16, 64)  # (rows, columns) of the GPU kernel's tile; the tests check it against seg_utils.CC_TILE
MAX_AREA = 8
SIZES = [(1, 1), (1, 70), (70, 1), (17, 33), (64, 64), (65, 129), (128, 256), (256, 256)]
BIG = (540, 960)  # serpentine and noise only


def set_mask(x, kind):
    """The set pixels of an array of an element kind of the C ABI."""
    x = np.asarray(x)
    if kind in ("uint8", "bool", "float32"):
        return x != 0
    if kind == "logits":
        return x > 0
    if kind == "scores_bg":  # background of scores: -0.0 is set, NaN is not
        return x <= 0
    raise ValueError(kind)


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def label(mask, connectivity=8):
    """(h,w) array, set where != 0 -> (labels, areas) int32 (h,w) as sola_mask_components defines them."""
    assert connectivity in (4, 8)
    m = np.asarray(mask) != 0
    h, w = m.shape
    k = 1 if connectivity == 8 else 0
    parent, run_y, run_s, run_e = [], [], [], []
    prev = []  # (start, end, id) of the previous row's runs
    for y in range(h):
        d = np.diff(np.concatenate(([0], m[y].astype(np.int8), [0])))
        starts, ends = np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()
        cur, j = [], 0
        for s, e in zip(starts, ends):  # [s, e)
            i = len(parent)
            parent.append(i)
            run_y.append(y); run_s.append(s); run_e.append(e)
            while j < len(prev) and prev[j][1] + k <= s:  # ends before this run (and does not touch it diagonally)
                j += 1
            jj = j
            while jj < len(prev) and prev[jj][0] < e + k:
                a, b = _find(parent, i), _find(parent, prev[jj][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                jj += 1
            cur.append((s, e, i))
        prev = cur
    labels, areas = np.zeros(h * w, np.int32), np.zeros(h * w, np.int32)
    if parent:
        root = np.array([_find(parent, i) for i in range(len(parent))])
        run_y, run_s, run_e = np.array(run_y), np.array(run_s), np.array(run_e)
        lens = run_e - run_s
        first = run_y * w + run_s
        area = np.bincount(root, weights=lens, minlength=len(parent)).astype(np.int64)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
        px = np.repeat(first - offs, lens) + np.arange(int(lens.sum()))
        labels[px] = np.repeat(first[root] + 1, lens)
        areas[px] = np.repeat(area[root], lens)
    return labels.reshape(h, w), areas.reshape(h, w)


def label_frames(masks, connectivity=8):
    """(n,h,w) -> stacked (labels, areas): every frame on its own."""
    out = [label(m, connectivity) for m in masks]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def fill_small(x, kind, max_area, value, connectivity=8):
    """sola_mask_fill_small: a copy of the (h,w) array x in which the pixels of set components (set_mask(x, kind)) of at most
    max_area pixels hold ``value``; everything else keeps its bits."""
    s = set_mask(x, kind)
    _, areas = label(s, connectivity)
    out = np.array(x, copy=True)
    out[s & (areas <= max_area)] = value
    return out


def fill_holes(scores, max_area, fill_value=0.1, connectivity=8):
    return fill_small(scores, "scores_bg", max_area, np.float32(fill_value), connectivity)


def remove_small(mask, max_area, mode, connectivity=8):
    """{0,1} mask: islands (set components <= max_area) cleared, or holes (clear components <= max_area) set to 1."""
    if mode == "islands":
        return fill_small(mask, "uint8", max_area, 0, connectivity)
    s = np.asarray(mask) == 0
    _, areas = label(s, connectivity)
    out = np.array(mask, copy=True)
    out[s & (areas <= max_area)] = 1
    return out


# ---- frames ------------------------------------------------------------------------------------------------------
def serpentine(h, w, vertical=False):
    """One path: every second row (column) in full, joined alternately at the right and the left (bottom and top)."""
    if vertical:
        return np.ascontiguousarray(serpentine(w, h).T)
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for i, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    m = np.zeros((h, w), np.uint8)
    t, b, l, r = 0, h - 1, 0, w - 1
    while t <= b and l <= r:
        m[t, l:r + 1] = 1
        m[t:b + 1, r] = 1
        if b - t >= 2:
            m[b, l + (2 if l else 0):r + 1] = 1
        if r - l >= 2 and b - t >= 2:
            m[t + 2:b + 1, l + 2 if l else l] = 1
        t, b, l, r = t + 2, b - 2, l + 2, r - 2
    return m


def comb(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0] = 1
    m[:, 0::2] = 1
    return m


def rings(h, w, max_area=MAX_AREA):
    """Two filled boxes, one with a hole of exactly max_area pixels (2 rows) and one of max_area + 1 (one more pixel in a third
    row); None when the frame is too small."""
    hw = (max_area + 1) // 2
    bw, bh = hw + 2, 5
    if h < bh + 1 or w < 2 * bw + 2:
        return None
    m = np.zeros((h, w), np.uint8)
    y0 = (h - bh) // 2
    for i, extra in enumerate((0, 1)):
        x0 = 1 + i * (bw + 1) if w < 4 * bw else (w // 2 - bw - 1) + i * (bw + 1)  # wide frames: astride the middle column
        m[y0:y0 + bh, x0:x0 + bw] = 1
        cells = [(y0 + 1 + j // hw, x0 + 1 + j % hw) for j in range(max_area + extra)]
        for yy, xx in cells:
            m[yy, xx] = 0
    return m


def tile_corner_pairs(h, w, tile=TILE, anti=False):
    """The only set pixels straddle a tile corner diagonally, at every corner position; None without an inner corner."""
    th, tw = tile
    ys, xs = range(th, h, th), range(tw, w, tw)
    if not ys or not xs:
        return None
    m = np.zeros((h, w), np.uint8)
    for cy in ys:
        for cx in xs:
            if anti:
                m[cy - 1, cx] = m[cy, cx - 1] = 1
            else:
                m[cy - 1, cx - 1] = m[cy, cx] = 1
    return m


def noise(h, w, p, seed=0):
    return (np.random.default_rng([h, w, seed]).uniform(size=(h, w)) < p).astype(np.uint8)


def frames(h, w, tile=TILE, max_area=MAX_AREA):
    """[(name, (h,w) uint8 {0,1})]: the shared cases at one size."""
    z = lambda: np.zeros((h, w), np.uint8)  # noqa: E731
    out = [("empty", z()), ("full", z() + 1)]
    for name, (y, x) in (("corner_tl", (0, 0)), ("corner_tr", (0, w - 1)), ("corner_bl", (h - 1, 0)), ("corner_br", (h - 1, w - 1))):
        m = z()
        m[y, x] = 1
        out.append((name, m))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checkerboard", ((yy + xx) % 2).astype(np.uint8)))
    m = z()  # two blobs that touch only diagonally, the touching corner in the middle of the frame
    cy, cx = h // 2, w // 2
    m[max(cy - 5, 0):cy, max(cx - 7, 0):cx] = 1
    m[cy:cy + 4, cx:cx + 6] = 1
    out.append(("diagonal_blobs", m))
    m = z()
    m[np.arange(min(h, w)), np.arange(min(h, w))] = 1
    out.append(("diagonal_line", m))
    m = z()
    i = np.arange(max(h, w))
    m[(i * h) // max(h, w), w - 1 - (i * w) // max(h, w)] = 1
    out.append(("anti_diagonal_line", m))
    r = rings(h, w, max_area)
    if r is not None:
        out.append(("rings", r))
    m = z() + 1  # small holes cut by the image border
    m[0:2, 0:2] = 0
    m[h // 2:h // 2 + 2, w - 1:] = 0
    m[h - 1, w // 3:w // 3 + 3] = 0
    out.append(("border_holes", m))
    out += [("comb", comb(h, w)), ("comb_flipped", np.ascontiguousarray(comb(h, w)[::-1, ::-1])), ("spiral", spiral(h, w)),
            ("serpentine", serpentine(h, w)), ("serpentine_vertical", serpentine(h, w, True)),
            ("noise_half", noise(h, w, 0.5)), ("noise_sparse", noise(h, w, 0.05))]
    for anti in (False, True):
        m = tile_corner_pairs(h, w, tile, anti)
        if m is not None:
            out.append(("tile_corners_anti" if anti else "tile_corners", m))
    return out


def big_frames(h=BIG[0], w=BIG[1]):
    return [("serpentine", serpentine(h, w)), ("serpentine_vertical", serpentine(h, w, True)), ("noise_half", noise(h, w, 0.5)),
            ("noise_sparse", noise(h, w, 0.05))]


def scores_from_mask(mask, seed=0):
    """float32 scores whose foreground (> 0) is the mask: positive and negative values, both zeros on the background side,
    NaN on both sides (a NaN is neither foreground nor background: it cuts components and passes through)."""
    rng = np.random.default_rng([seed, mask.shape[-2], mask.shape[-1]])
    r = (rng.uniform(size=mask.shape) * 4 + 0.01).astype(np.float32)
    pick = rng.integers(0, 4, size=mask.shape)
    off = np.where(pick == 0, np.float32(-0.0), np.where(pick == 1, np.float32(0.0), -r)).astype(np.float32)
    s = np.where(np.asarray(mask) != 0, r, off).astype(np.float32)
    nan = rng.uniform(size=mask.shape) < 0.01
    payload = np.array([0x7fc00000, 0xffc00001, 0x7f800123], np.uint32).view(np.float32)
    s[nan] = payload[rng.integers(0, 3, size=int(nan.sum()))]
    return s
