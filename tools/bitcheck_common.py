"""What the bit-for-bit recorders (attn_fwd_bitcheck.py, attn_bwd_bitcheck.py) share: one SHA-256 per array, DIR/record.json, and the
comparison of two records."""
import hashlib
import json
import os


def digest(t):
    import torch

    t = t.detach().contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def switch_name(sw):
    return ",".join(f"{k}={v}" for k, v in sw.items()) or "default"


def write_record(out, rec):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "record.json"), "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print(f"{len(rec)} launches recorded in {out}/record.json")


def compare(a, b):
    """Both records hold the same launches and arrays and every digest is equal: returns the number of differences."""
    ra, rb = (json.load(open(os.path.join(d, "record.json"))) for d in (a, b))
    bad = sorted(set(ra) ^ set(rb))
    if bad:
        print("launches in one record only:", bad)
    diff = [(k, n) for k in sorted(set(ra) & set(rb)) for n in sorted(set(ra[k]) | set(rb[k])) if ra[k].get(n) != rb[k].get(n)]
    for k, n in diff:
        print(f"DIFFERENT: {k}: {n}")
    n_arrays = sum(len(v) for v in rb.values())
    print(f"{len(rb)} launches, {n_arrays} arrays: " + ("every array bit-equal" if not bad and not diff else f"{len(diff)} arrays differ, {len(bad)} launches unmatched"))
    return len(bad) + len(diff)
