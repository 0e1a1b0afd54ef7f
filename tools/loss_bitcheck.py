"""Bit-for-bit record of sola_loss / sola_loss_ragged for comparing two builds of the library (profiles/step_boundary.txt):

    SOLA_HIP_LIB=<library> python tools/loss_bitcheck.py --out A.npz        (once per build)
    python tools/loss_bitcheck.py --compare A.npz B.npz

Shapes: D = 1024 / 512 (the register kernels) and 128 (the LDS row kernel), n_neg = 32 / 3 / 1, uniform batches of (2, 9), (1, 1), (3, 16),
(37, 64) and the headline's (256, 64) tracks, a ragged batch of 1 / 8 / 17 / 64 / 3 tracks with one table of negatives per sample, and
2047 negatives (more than 64 KB of LDS).  Recorded: the three loss values and the hardest-negative indices."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def record(path):
    import torch

    from sola_amd.loss import track_selection_losses, track_selection_losses_ragged

    out = {}
    rng = np.random.Generator(np.random.PCG64(5))
    c = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()

    def uniform(key, B, N, D, n_neg):
        x, tok, y = rng.standard_normal((B, N)) * 3, rng.standard_normal((B, N, D)), (rng.uniform(size=(B, N)) < 0.3)
        pos, neg = rng.standard_normal((B, 1, D)) * 0.06, rng.standard_normal((n_neg, D)) * 0.06
        with torch.no_grad():
            l3, am = track_selection_losses(c(x), c(tok), c(y), c(pos), c(neg), 1.5, 0.07, 0.3, return_argmax=True)
        out[key + ".loss"], out[key + ".arg"] = l3.cpu().numpy(), am.cpu().numpy()

    for D in (1024, 512, 128):
        for n_neg in (32, 3, 1):
            for B, N in ((2, 9), (1, 1), (3, 16), (37, 64), (256, 64)):
                uniform(f"u.{D}.{n_neg}.{B}.{N}", B, N, D, n_neg)
            counts = [1, 8, 17, 64, 3]
            tot = sum(counts)
            x, tok, y = rng.standard_normal(tot) * 3, rng.standard_normal((tot, D)), (rng.uniform(size=tot) < 0.3)
            pos, neg = rng.standard_normal((len(counts), D)) * 0.06, rng.standard_normal((len(counts), n_neg, D)) * 0.06
            offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
            with torch.no_grad():
                l3, am = track_selection_losses_ragged(c(x), c(tok), c(y), c(pos), c(neg), offs, counts, 1.5, 0.07, 0.3, return_argmax=True)
            out[f"r.{D}.{n_neg}.loss"], out[f"r.{D}.{n_neg}.arg"] = l3.cpu().numpy(), am.cpu().numpy()
    for D in (1024, 512):
        uniform(f"big.{D}", 2, 11, D, 2047)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("wrote", path, len(out), "arrays")


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    assert sorted(za.files) == sorted(zb.files), "the two records hold different cases"
    bad = [n for n in za.files if za[n].shape != zb[n].shape or za[n].tobytes() != zb[n].tobytes()]
    for n in bad:
        print(n, za[n].shape, "DIFFERENT")
    print(f"{len(za.files)} arrays compared, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    record(args.out)
