"""Mask IoU (sola_mask_iou_matrix: sola_amd/csrc/iou.hip, api.hip): the case table that reaches every branch of the one-launch
kernel's launcher, a plain restatement of the launcher's choice and of the two scratch sizes, the exact reference for the counts and
the seeded mask sets.  Shared by test_iou_cpu.py and test_gpu_iou_routes.py."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "id P R H W h w dtype offset switches scratch fill")
# h, w      size of the R prompt masks (resampled to H x W by the call when they differ)
# dtype     "u8" / "f32"
# offset    bytes between the start of the prompt set's storage and its first mask (0: aligned as the allocator aligns)
# switches  sola_tune keys the case runs under (a tuple of (key, value): hashable)
# scratch   "max": the larger of the two restated byte counts; "abi": what sola_mask_iou_scratch_bytes asks for and no more
# fill      "random" / "ones" (make_masks)

# the sola_tune keys of the route and their defaults (docs/tune_keys.md)
SWITCHES = {"iou_fused": 1, "iou_packed": 1, "iou_shape": 0, "pack_resample_lds": 1}

# iou.hip's constants
FUSED_MAXP = 4         # tracks per block of the one-launch kernel
OP_CHUNK = 512         # 32-pixel words per block
OP_MAX_CHUNKS = 128    # rows the group's fold walks at most
OP_TICKETS = 4096      # ticket ring; a call may take a quarter of it
OP_ACC_LINES = 16384   # pair-word ring; a call takes 4 R lines
PK_PIXELS = 1 << 19    # 19-bit count fields
PK_MAX_CHUNKS = 126    # 7-bit arrival field
RS_MAXW = 4096         # widest source row of the LDS-staged resample pack

SHAPES = ((1, 1), (1, 12), (2, 3), (2, 6), (4, 1), (4, 2), (4, 3))  # the (G, nb) block shapes the table runs through "iou_shape"
BAD_SHAPES = (16 * 3 + 1, 16 * 4 + 4, 16 * 2 + 0)                    # G = 3; G * nb = 16; nb = 0: each must route as the default

BRANCHES = ([f"onepass/G{g}/{form}" for g in (1, 2, 4) for form in ("pk", "ticket")] +
            [f"decline/{why}" for why in ("off", "dtype", "P", "resample", "hw32", "chunks", "groups", "align", "scratch")])
FALLBACKS = ("pair-stream", "resample-lds", "generic")


def _ceil(a, b):
    return -(-a // b)


def _align256(v):
    return (v + 255) & ~255


def valid_shape(G, nb):
    return G in (1, 2, 4) and nb >= 1 and G * nb <= 12


def onepass_shape(R, iou_shape=0):
    """(G, nb) = (prompt slices in flight, batches per block): iou.hip's onepass_shape."""
    G, nb = iou_shape >> 4, iou_shape & 15
    if iou_shape > 0 and valid_shape(G, nb):
        return G, nb
    return (1 if R <= 16 else 2), (1 if R <= 32 else 2 if R <= 128 else 4)


def fused_scratch_bytes(R, words):
    """mask_iou_fused_scratch_bytes (iou.hip): the one-launch kernel's count rows, bounded over every block shape."""
    return (9 * R + 64) * _ceil(words, OP_CHUNK) * 4


def abi_scratch_bytes(P, R, H, W):
    """sola_mask_iou_scratch_bytes (api.hip): the packed bits and the areas of pack + pair."""
    words = (H * W + 31) // 32
    return _align256(P * words * 4) + _align256(R * words * 4) + _align256(P * 8) + _align256(R * 8)


def route(P, R, H, W, h, w, dtype, aligned, scratch_bytes, switches=None):
    """The branch a sola_mask_iou_matrix call takes.  A restatement of onepass_shape, of launch_mask_iou_fused's decline conditions (in
    the code's order) and of its choice between the packed pair words and the ticket form (iou.hip): whoever edits one of those edits
    this.  ``aligned``: both mask pointers are multiples of 16."""
    sw = dict(SWITCHES, **dict(switches or {}))
    hw = H * W
    G, nb = onepass_shape(R, sw["iou_shape"])
    GB = G * nb
    groups, chunks = _ceil(R, GB), _ceil(hw // 32, OP_CHUNK)
    for why, declined in (("off", not sw["iou_fused"]), ("dtype", dtype != "u8"), ("P", P > FUSED_MAXP), ("resample", h != H or w != W),
                          ("hw32", hw % 32 != 0), ("chunks", chunks > OP_MAX_CHUNKS), ("groups", groups > OP_TICKETS // 4),
                          ("align", not aligned), ("scratch", scratch_bytes < fused_scratch_bytes(R, hw // 32))):
        if declined:
            return f"decline/{why}"
    pk = bool(sw["iou_packed"]) and hw < PK_PIXELS and chunks <= PK_MAX_CHUNKS and R <= OP_ACC_LINES // 16
    return f"onepass/G{G}/{'pk' if pk else 'ticket'}"


def fallback(P, R, H, W, h, w, dtype, aligned, switches=None):
    """What packs the prompt set when the one-launch kernel declines: "pair-stream" (both sets in ONE streaming launch), else the kernel
    launch_mask_pack picks for it - "stream", "resample-lds" or "generic".  A restatement of sola_mask_iou_matrix's fallback (api.hip),
    launch_mask_pack_pair, launch_mask_pack and resample_lds_ok (iou.hip): whoever edits one of those edits this."""
    sw = dict(SWITCHES, **dict(switches or {}))
    hw, identity = H * W, (h == H and w == W)
    if dtype == "u8" and identity and hw % 32 == 0 and aligned and P + R <= 65535:
        return "pair-stream"
    if dtype == "u8" and identity and hw % 32 == 0 and aligned:
        return "stream"
    lds = sw["pack_resample_lds"]
    if not identity and lds and W % 32 == 0 and w <= RS_MAXW and w <= 3 * W and \
            (lds == 2 or (w % 32 == 0 and aligned and (h * w * (1 if dtype == "u8" else 4)) % 16 == 0)):
        return "resample-lds"
    return "generic"


def launch_shape(case, switches=None):
    """(G, nb, groups, chunks) of the one-launch kernel's grid for the case: blocks of G * nb prompts x 512 words."""
    G, nb = onepass_shape(case.R, dict(case.switches, **(switches or {})).get("iou_shape", 0))
    return G, nb, _ceil(case.R, G * nb), _ceil(case.H * case.W // 32, OP_CHUNK)


def scratch_bytes(case):
    abi = abi_scratch_bytes(case.P, case.R, case.H, case.W)
    return abi if case.scratch == "abi" else max(abi, fused_scratch_bytes(case.R, case.H * case.W // 32))


def case_route(case, switches=None):
    sw = dict(case.switches, **(switches or {}))
    return route(case.P, case.R, case.H, case.W, case.h, case.w, case.dtype, case.offset % 16 == 0, scratch_bytes(case), sw)


def case_fallback(case):
    return fallback(case.P, case.R, case.H, case.W, case.h, case.w, case.dtype, case.offset % 16 == 0, dict(case.switches))


def _c(P, R, H, W, h=None, w=None, dtype="u8", offset=0, scratch="max", fill="random", **switches):
    h, w = H if h is None else h, W if w is None else w
    name = f"p{P}_r{R}_{H}x{W}" + (f"_from{h}x{w}" if (h, w) != (H, W) else "") + ("_f32" if dtype != "u8" else "") + \
        (f"_off{offset}" if offset else "") + ("_abi" if scratch == "abi" else "") + ("_ones" if fill == "ones" else "") + \
        "".join(f"_{k[4:]}{v}" for k, v in sorted(switches.items()))
    return Case(name, P, R, H, W, h, w, dtype, offset, tuple(sorted(switches.items())), scratch, fill)


def _shape_R(G, nb):
    """Prompt counts below, at and one above a multiple of the block's G * nb prompts: the first multiple above 16, where the default
    shape is (2, 1) and so none of SHAPES."""
    m = G * nb * _ceil(17, G * nb)
    return (m - 1, m, m + 1)


CASES = (
    # ---- the packed pair words, block shape by R: (1,1) up to 16 prompts, (2,1) up to 32, (2,2) up to 128, (2,4) beyond
    [_c(P, R, 64, 96) for P, R in ((1, 1), (4, 16), (3, 17), (2, 33), (4, 129))] +
    # ... one word, the last chunk almost all out of range; and 524 160 pixels, the largest common size under 2^19, every field at its top
    [_c(2, 7, 8, 4), _c(4, 5, 546, 960, fill="ones")] +
    # ---- every block shape through "iou_shape", both forms, on two chunks (the second a quarter full): ragged, full and one-over last groups
    [_c(3 + (R & 1), R, 128, 160, iou_shape=16 * G + nb, **packed)
     for G, nb in SHAPES for R in _shape_R(G, nb) for packed in ({}, {"iou_packed": 0})] +
    # ... shapes the launcher refuses: the default route
    [_c(3, 17, 64, 96, iou_shape=s) for s in BAD_SHAPES] +
    # ---- the ticket form by size: 2^19 pixels (the first off the packed form, 32 chunks), 57 chunks (not a multiple of the fold's four
    #      stripes), 128 chunks (the limit)
    [_c(3, 5, 512, 1024), _c(2, 3, 720, 1280), _c(2, 3, 1024, 2048)] +
    # ---- ... by prompt count: 129 groups of eight, the packed form declined by R > 1024
    [_c(4, 1025, 32, 32)] +
    # ---- ... under iou_packed 0: 1, 2, 3 (every chunk full) and 5 chunks
    [_c(4, 16, 64, 96, iou_packed=0), _c(3, 33, 128, 160, iou_packed=0), _c(4, 129, 192, 256, iou_packed=0), _c(2, 40, 256, 300, iou_packed=0)] +
    # ---- what the one-launch kernel declines, in the order of its tests
    [_c(4, 17, 64, 96, iou_fused=0), _c(3, 7, 64, 96, dtype="f32"), _c(5, 9, 64, 96), _c(2, 5, 64, 96, h=96, w=128), _c(2, 5, 64, 96, h=48, w=80),
     _c(3, 9, 36, 100), _c(1, 2, 1025, 2048), _c(4, 1025, 32, 32, iou_shape=17), _c(3, 9, 64, 96, offset=1), _c(4, 300, 8, 4, scratch="abi")]
)
BY_ID = {c.id: c for c in CASES}
# the ticket form at a real size, for calls that alternate two mask sets through one scratch: 57 chunks x 9 groups = 513 blocks per call
ALTERNATING = _c(4, 33, 720, 1280)
# the packed form's cases whose calls cost nothing: both forms in turn, and the library's two rings walked past their ends
RING_IDS = [f"p{P}_r{R}_64x96" for P, R in ((1, 1), (4, 16), (3, 17), (2, 33), (4, 129))]


def counts_ref(A, B):
    """Exact (inter, union) int64 [P, R] of masks A [P, H, W] and B [R, H, W] (set where != 0): ONE float64 matrix product of the
    flattened masks - every count is below 2^24 and float64 adds integers below 2^53 exactly - where oracle/iou_oracle.iou_matrix
    loops over the pairs."""
    a = (np.asarray(A) != 0).reshape(len(A), -1)
    b = (np.asarray(B) != 0).reshape(len(B), -1)
    n = a.shape[1]
    assert b.shape[1] == n and n < (1 << 24)
    inter = np.zeros((len(a), len(b)), np.float64)
    for s in range(0, n, 1 << 18):  # in slices of the pixels: the float64 copies stay small
        inter += a[:, s:s + (1 << 18)].astype(np.float64) @ b[:, s:s + (1 << 18)].astype(np.float64).T
    inter = np.rint(inter).astype(np.int64)
    union = a.sum(axis=1, dtype=np.int64)[:, None] + b.sum(axis=1, dtype=np.int64)[None, :] - inter
    return inter, union


def equal_index(case):
    """The prompt that equals track 0 in the first mask set."""
    return 2 if case.R >= 3 else case.R - 1


@functools.lru_cache(maxsize=None)
def make_masks(case, which=0):
    """(A [P, H, W], B [R, h, w]) of the case's dtype, seeded by the case.  Set 0: A at density 0.3, B at 0.5 with any non-zero byte
    for "set" (fill "ones": all set but for A[2] at 0.9 and B[1] at 0.5); prompt 0 empty (R >= 2), prompt equal_index() a copy of
    track 0 in other bytes (same-size sets), the last track's upper half empty (P >= 2).  Set 1: set 0 complemented, every mask shifted by its
    own number of pixels - another set of the same shape whose every count differs.  Computed once, shared, never modified."""
    P, R, H, W, h, w = case.P, case.R, case.H, case.W, case.h, case.w
    rng = np.random.default_rng([P, R, H, W, h, w])
    if case.fill == "ones":
        A, B = np.ones((P, H, W), np.uint8), np.full((R, h, w), 255, np.uint8)
        if P > 2:
            A[2] = rng.random((H, W), dtype=np.float32) < 0.9
        if R > 1:
            B[1] = (rng.random((h, w), dtype=np.float32) < 0.5) * np.uint8(3)
    else:
        A = (rng.random((P, H, W), dtype=np.float32) < 0.3).astype(np.uint8)
        B = (rng.random((R, h, w), dtype=np.float32) < 0.5) * rng.integers(1, 256, size=(R, h, w), dtype=np.uint8)
    if P >= 2:
        A[P - 1, : H // 2] = 0
    if (h, w) == (H, W):
        B[equal_index(case)] = A[0] * np.uint8(7)
    if R >= 2:
        B[0] = 0
    if which == 1:
        A = np.stack([np.roll(m == 0, 3 + i).astype(np.uint8) for i, m in enumerate(A)])
        B = np.stack([np.roll(m == 0, 5 + 2 * i) * np.uint8(1 + i % 255) for i, m in enumerate(B)])
    else:
        assert which == 0
    dt = np.uint8 if case.dtype == "u8" else np.float32
    A, B = np.ascontiguousarray(A.astype(dt)), np.ascontiguousarray(B.astype(dt))
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def reference(case, which=0):
    """counts_ref of the case's mask set, the prompts resampled as the call resamples them.  Computed once, shared, never modified."""
    from oracle import iou_oracle
    A, B = make_masks(case, which)
    if (case.h, case.w) != (case.H, case.W):
        B = iou_oracle.nearest_resize(B, case.H, case.W)
    inter, union = counts_ref(A, B)
    inter.setflags(write=False)
    union.setflags(write=False)
    return inter, union
