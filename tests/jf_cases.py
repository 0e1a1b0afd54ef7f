"""A small MeViS-layout tree for the J&F tests: meta_expressions.json, mask_dict.json (optional), per-video grid tracks and
per-expression GroundingDINO tracks (RLE masklet JSON + object tokens), with blob masks from masklet_cases."""
import json
import os

import numpy as np

import masklet_cases as mc
from oracle import masklet_oracle as mo

T, H, W = 6, 23, 37  # h*w = 851: not a multiple of 32 or 128

# video -> (grid track ids, {expression id: (expression, GT anno ids, gdino track ids)})
VIDEOS = {
    "vidA": ([2, 5, 11], {"0": ("a cat", [3], [40, 41]), "1": ("two cats", [3, 7], [42]), "2": ("the dog", [9], [43, 44])}),
    "vidB": ([1, 4], {"0": ("a bird flying", [12], [50]), "1": ("the empty thing", [13], [51])}),
}


def rle_list(masks, compressed=True, missing=()):
    out = []
    for t, f in enumerate(masks):
        if t in missing:
            out.append(None)
            continue
        c = mo.mask_to_counts(f)
        out.append({"size": [int(f.shape[0]), int(f.shape[1])], "counts": mo.rle_counts_to_string(c) if compressed else c})
    return out


def gt_masks(anno_id):
    """GT object masks: object 13 is empty in every frame; object 7 has an empty frame."""
    m = mc.blob_masklet(T, H, W, 1000 + anno_id)
    if anno_id == 13:
        m[:] = 0
    if anno_id == 7:
        m[1] = 0
    return m


def make_tree(root, token_dim=256, with_mask_dict=True):
    """Writes the tree under ``root``; returns (data_root, track_root, split config dict)."""
    data_root, track_root = os.path.join(root, "data"), os.path.join(root, "tracks")
    ddir = os.path.join(data_root, "mevis", "valid_u")
    os.makedirs(ddir, exist_ok=True)
    meta, mask_dict = {"videos": {}}, {}
    for vid, (grid, exps) in VIDEOS.items():
        meta["videos"][vid] = {"frames": [f"{t:05d}" for t in range(T)],
                               "expressions": {e: {"exp": x, "anno_id": a} for e, (x, a, _) in exps.items()}}
        for e, (_, annos, gd) in exps.items():
            for a in annos:
                # object 3 has a missing frame in mask_dict, object 9 uncompressed counts
                mask_dict[str(a)] = rle_list(gt_masks(a), compressed=(a != 9), missing=(4,) if a == 3 else ())
        _write_tracks(track_root, "grid_tracks", (vid,), grid, token_dim)
        for e, (_, _, gd) in exps.items():
            _write_tracks(track_root, "gdino_tracks", (vid, e), gd, token_dim)
    with open(os.path.join(ddir, "meta_expressions.json"), "w") as f:
        json.dump(meta, f)
    if with_mask_dict:
        with open(os.path.join(ddir, "mask_dict.json"), "w") as f:
            json.dump(mask_dict, f)
    split = {"data_name": "mevis", "data_type": "valid_u", "sam2_output_dirs": "grid_tracks,gdino_tracks", "batch_size": 1}
    return data_root, track_root, split


def _write_tracks(track_root, root, tail, ids, token_dim):
    base = os.path.join(track_root, root, "mevis", "valid_u")
    mdir, tdir = os.path.join(base, "sam2_masklets", *tail), os.path.join(base, "sam2_object_tokens", *tail)
    os.makedirs(mdir, exist_ok=True)
    os.makedirs(tdir, exist_ok=True)
    for aid in ids:
        masks = mc.blob_masklet(T, H, W, aid)
        rle = rle_list(masks, missing=(0,) if aid == 41 else ())  # track 41 starts with a missing frame
        with open(os.path.join(mdir, f"{aid:05d}.json"), "w") as f:
            json.dump({"anno_id": aid, "prompt_type": "grid" if root == "grid_tracks" else "gdino", "rle": rle,
                       "iou": {"3": 0.9} if aid % 2 else {}}, f)
        rng = np.random.default_rng(aid)
        np.save(os.path.join(tdir, f"{aid:05d}.npy"), rng.standard_normal((T, token_dim)).astype(np.float32))
