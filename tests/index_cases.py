"""Numpy restatements for the index-map tests (plain ``==``, np.packbits, np.bincount) and a small Ref-DAVIS-layout tree:
meta_expressions.json, Annotations/<video>/<frame>.png palette images, per-video grid tracks (RLE masklet JSON + tokens)."""
import json
import os

import numpy as np

import masklet_cases as mc

ID_CHUNK = 8  # SOLA_INDEX_ID_CHUNK


def hist(maps):
    """uint8 [T,h,w] -> int64 [T,256]."""
    return np.stack([np.bincount(f.reshape(-1), minlength=256) for f in maps]).astype(np.int64) if len(maps) else np.zeros((0, 256), np.int64)


def _pack(flat, stride):
    """bool [n, pixels] -> uint32 [n, stride]: bit j of word i = pixel 32*i + j, zero padded."""
    n = flat.shape[0]
    buf = np.zeros((n, stride * 32), np.uint8)
    buf[:, :flat.shape[1]] = flat
    return np.packbits(buf, axis=1, bitorder="little").view("<u4")


def rm_words(h, w):
    return (h * w + 31) // 32


def cm_words(h, w):
    return ((h * w + 31) // 32 + 3) // 4 * 4


def rm_planes(maps, ids, stride=None):
    """Plane k*T + t = (maps[t] == ids[k]) over the raster."""
    T, h, w = maps.shape
    m = np.stack([maps == k for k in ids]) if len(ids) else np.zeros((0, T, h, w), bool)
    return _pack(m.reshape(len(ids) * T, h * w), rm_words(h, w) if stride is None else stride)


def cm_planes(maps, ids, stride=None):
    """The same planes over m.T: position = x*h + y."""
    T, h, w = maps.shape
    m = np.stack([maps == k for k in ids]) if len(ids) else np.zeros((0, T, h, w), bool)
    return _pack(m.transpose(0, 1, 3, 2).reshape(len(ids) * T, h * w), cm_words(h, w) if stride is None else stride)


def object_ids(maps, rule):
    if rule == "davis":
        return [int(v) for v in np.unique(maps[0]) if v not in (0, 255)]
    return [k for k in range(1, 256) if (maps == k).sum() > 0]


def masklets_dict(maps, ids=None):
    """get_masklets_ytbvos's return value: {str(id): float32 [T,h,w]} without the objects that are empty everywhere."""
    ids = range(1, 256) if ids is None else ids
    out = {}
    for k in ids:
        m = (maps == k)
        if m.sum() > 0:
            out[str(k)] = m.astype(np.float32)
    return out


def random_maps(T, h, w, seed, values=None):
    rng = np.random.default_rng(seed)
    if values is None:
        return rng.integers(0, 256, size=(T, h, w), dtype=np.uint8)
    return np.asarray(values, np.uint8)[rng.integers(0, len(values), size=(T, h, w))]


# ----------------------------------------------------------------------------------------------------- Ref-DAVIS tree
T, H, W = 5, 23, 37
# video -> (grid track ids, object ids painted into the annotation, {expression id: (expression, obj_id)})
VIDEOS = {
    "bear": ([2, 5, 11], [1, 2, 3], {"0": ("a bear", 1), "1": ("the bear on the left", 1), "2": ("a rock", 3), "3": ("nothing here", 7)}),
    "camel": ([1, 4], [1, 2], {"0": ("a camel", 2), "1": ("the other camel", 1)}),
}


def annotation(vid):
    """uint8 [T,H,W] index maps: later objects paint over earlier ones, a few void (255) pixels."""
    _, objects, _ = VIDEOS[vid]
    maps = np.zeros((T, H, W), np.uint8)
    for k in objects:
        maps[mc.blob_masklet(T, H, W, 2000 + 10 * len(vid) + k) != 0] = k
    maps[:, 0, :3] = 255
    return maps


def make_davis_tree(root, token_dim=256, with_annotations=True, mode="P"):
    from PIL import Image
    data_root, track_root = os.path.join(root, "data"), os.path.join(root, "tracks")
    mdir = os.path.join(data_root, "ref-davis", "meta_expressions", "valid")
    os.makedirs(mdir, exist_ok=True)
    meta = {"videos": {}}
    for vid, (grid, _, exps) in VIDEOS.items():
        frames = [f"{t:05d}" for t in range(T)]
        meta["videos"][vid] = {"frames": frames, "expressions": {e: {"exp": x, "obj_id": str(o)} for e, (x, o) in exps.items()}}
        if with_annotations:
            adir = os.path.join(data_root, "ref-davis", "valid", "Annotations", vid)
            os.makedirs(adir, exist_ok=True)
            for name, frame in zip(frames, annotation(vid)):
                im = Image.fromarray(frame, mode="L")
                if mode == "P":
                    im = Image.fromarray(frame, mode="P")
                    im.putpalette([(37 * i) % 256 for i in range(768)])
                im.save(os.path.join(adir, name + ".png"))
        base = os.path.join(track_root, "grid_tracks", "ref-davis", "valid")
        tm, tt = os.path.join(base, "sam2_masklets", vid), os.path.join(base, "sam2_object_tokens", vid)
        os.makedirs(tm, exist_ok=True)
        os.makedirs(tt, exist_ok=True)
        for aid in grid:
            import jf_cases as jc
            rle = jc.rle_list(track_masks(aid))
            with open(os.path.join(tm, f"{aid:05d}.json"), "w") as f:
                json.dump({"anno_id": aid, "prompt_type": "grid", "rle": rle, "iou": {"1": 0.9} if aid % 2 else {}}, f)
            np.save(os.path.join(tt, f"{aid:05d}.npy"), np.random.default_rng(aid).standard_normal((T, token_dim)).astype(np.float32))
    with open(os.path.join(mdir, "meta_expressions.json"), "w") as f:
        json.dump(meta, f)
    split = {"data_name": "ref-davis", "data_type": "valid", "sam2_output_dirs": "grid_tracks", "batch_size": 1}
    return data_root, track_root, split


def track_masks(aid):
    return mc.blob_masklet(T, H, W, aid)
