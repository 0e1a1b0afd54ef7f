"""Bit-for-bit record of the inference forwards' results, for comparing two builds of the library (a refactor of the host-side
sequencing must not move a bit).  The training step's counterpart is tools/grad_bitcheck.py.

    SOLA_HIP_LIB=<build A>/libsola_hip.so python tools/infer_bitcheck.py --out DIR_A
    SOLA_HIP_LIB=<build B>/libsola_hip.so python tools/infer_bitcheck.py --out DIR_B
    python tools/infer_bitcheck.py --compare DIR_A DIR_B

Every seeded case (full model config) runs in the precisions f32 / f16x3 / f16 and writes score_map and score_tokens as .npy files into
DIR/<case>_<precision>/.  --compare checks that both directories hold the same cases and arrays and that every array is equal bit for
bit (numpy.array_equal on the raw 32-bit words, so a NaN equals itself); exit status 1 on any difference.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from grad_bitcheck import compare  # noqa: E402  (same directory layout, same rule)

# uniform (B, N, T, L): one sample; the split path; B * L + n_negative >= 1024 (shared negatives); N and L + n_negative above
# attn_split_min_keys (q / k / v written as split pairs); odd sizes
UNIFORM = [(1, 4, 32, 5), (8, 24, 32, 7), (64, 8, 32, 16), (2, 128, 32, 100), (3, 7, 9, 1)]
# ragged: (N, T) per video, text length per sample, sample -> video (None = one expression per video, in order)
RAGGED = [
    ("ragged_six_videos", [(5, 20), (9, 33), (12, 40), (7, 64), (16, 25), (3, 150)], [5, 7, 3, 11, 16, 1], None),
    ("ragged_3x4_gather", [(5, 20), (9, 33), (12, 40)], [5, 7, 3, 11, 16, 1, 2, 9, 4, 4, 8, 6], [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]),
]
PRECISIONS = ("f32", "f16x3", "f16")


def record(out):
    import torch

    from sola_amd import synth
    from sola_amd.module import LanguageAlignedTrackSelectionModule

    cfg = synth.DEFAULT_MODEL_CFG
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, 42).items()}, strict=True)
    m = m.cuda().eval()

    def save(case, prec, sm, st):
        torch.cuda.synchronize()
        d = os.path.join(out, f"{case}_{prec}")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "score_map.npy"), sm.detach().float().cpu().numpy())
        np.save(os.path.join(d, "score_tokens.npy"), st.detach().float().cpu().numpy())
        print(f"{case}_{prec}: score_map {tuple(sm.shape)} sum {float(sm.double().sum()):.6f}", flush=True)

    for prec in PRECISIONS:
        m.precision = prec
        for B, N, T, L in UNIFORM:
            inp = synth.make_inputs(cfg, B, N, T, L, 1)
            with torch.no_grad():
                sm, st = m(torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda())
            save(f"uniform_{B}_{N}_{T}_{L}", prec, sm, st)
        for name, videos, lens, sample_video in RAGGED:
            rng = np.random.Generator(np.random.PCG64(2024))
            objs = [torch.from_numpy(rng.standard_normal(size=(n, t, cfg["object_token_dim"])).astype(np.float32)).cuda() for n, t in videos]
            langs = [torch.from_numpy(rng.standard_normal(size=(l, cfg["lang_token_dim"])).astype(np.float32)).cuda() for l in lens]
            with torch.no_grad():
                m.forward_ragged(objs, langs, sample_video)
            save(name, prec, m.last_ragged[0], m.last_ragged[1])  # the flat buffers of all samples


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="record the cases into this directory")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(*args.compare) else 0)
    if not args.out:
        ap.error("--out DIR or --compare DIR_A DIR_B")
    record(args.out)
