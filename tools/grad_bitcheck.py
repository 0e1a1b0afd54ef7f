"""Bit-for-bit record of the training step's results, for comparing two builds of the library (a refactor of the host-side
sequencing must not move a bit: the orders of summation are fixed).

    SOLA_HIP_LIB=<build A>/libsola_hip.so python tools/grad_bitcheck.py --out DIR_A
    SOLA_HIP_LIB=<build B>/libsola_hip.so python tools/grad_bitcheck.py --out DIR_B
    python tools/grad_bitcheck.py --compare DIR_A DIR_B

Every seeded case (full model config) writes the three losses and all 83 parameter gradients as .npy files into DIR/<case>/.
--compare checks that both directories hold the same cases and arrays and that every array is equal bit for bit (numpy.array_equal on
the raw 32-bit words, so a NaN equals itself); exit status 1 on any difference.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POS_W, TEMP, ALIGN_W = 1.5, 0.07, 0.3
# (name, precision, batch B of (B, 64, 32, 16) or None = the ragged mix, sola_tune switches, dropout)
# layer rows of a uniform case = 256 * B: 256 takes the grouped few-sample route (bwd_group_rows 2048), 2304 lies above it, 9216 above the
# 8192-row split-K scratch gate; 1280 is above train_split_min_rows 1024, where the 16-bit modes start
CASES = [
    ("one_grouped", "f32", 1, {}, False),
    ("one_slabs", "f32", 1, {"bwd_group_rows": 0}, False),
    ("one_side_lane", "f32", 1, {"bwd_side_rows": 4096}, False),
    ("f32_rows2304", "f32", 9, {}, False),
    ("f32_rows9216", "f32", 36, {}, False),
    ("f16x3_rows1280", "f16x3", 5, {}, False),
    ("f16_rows1280", "f16", 5, {}, False),
    ("bf16_rows1280", "bf16", 5, {}, False),
    ("bf16_store0", "bf16", 5, {"train_bf16_store": 0}, False),
    ("bf16_store2", "bf16", 5, {"train_bf16_store": 2}, False),
    ("bf16_store1", "bf16", 5, {"train_bf16_store": 1}, False),
    ("f16x3_dw_split", "f16x3", 5, {"train_dw_f16": 0}, False),
    ("f16x3_no_dual_cast", "f16x3", 5, {"bwd_dual_cast": 0}, False),
    ("f16_no_dual_cast", "f16", 5, {"bwd_dual_cast": 0}, False),
    ("bf16_no_dual_cast", "bf16", 5, {"bwd_dual_cast": 0}, False),
    ("bf16_store0_no_dual_cast", "bf16", 5, {"train_bf16_store": 0, "bwd_dual_cast": 0}, False),
    ("bf16_no_fused_cast", "bf16", 5, {"bwd_fused_bf16_cast": 0}, False),
    ("bf16_no_x16_keep", "bf16", 5, {"train_x16_keep": 0}, False),
    ("ragged_f32", "f32", None, {}, False),
    ("ragged_f16x3", "f16x3", None, {}, False),
    ("ragged_f16", "f16", None, {}, False),
    ("ragged_bf16", "bf16", None, {}, False),
    ("dropout_f32", "f32", 9, {}, True),
    ("dropout_bf16", "bf16", 5, {}, True),
]


def record(out):
    import torch

    from sola_amd import synth
    from sola_amd._lib import tuned
    from sola_amd.loss import track_selection_losses, track_selection_losses_ragged
    from sola_amd.module import LanguageAlignedTrackSelectionModule, collate_ragged

    cfg = synth.DEFAULT_MODEL_CFG
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, 42).items()}
    for name, precision, B, switches, dropout in CASES:
        m = LanguageAlignedTrackSelectionModule(cfg)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train(dropout)
        m.precision = precision
        torch.manual_seed(7)  # the step's dropout mask seed comes from torch's CPU generator
        with tuned(**switches):
            if B is None:
                samples = synth.make_ragged_samples(cfg, 8, 2024, "cuda")
                m.forward_ragged(collate_ragged([s["obj"] for s in samples]), collate_ragged([s["lang"] for s in samples]), differentiable=True)
                flat, tok, offs, counts = m.last_ragged
                loss = track_selection_losses_ragged(flat, tok, torch.cat([s["labels"] for s in samples]), torch.stack([s["pos"] for s in samples]),
                                                     m.negative_token.weight, offs, counts, POS_W, TEMP, ALIGN_W)
                loss[:, 0].sum().backward()
                loss3 = loss.sum(0)
            else:
                inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, B, 64, 32, 16, 1).items()}
                sm, st = m(inp["object_tokens"], inp["lang_tokens"])
                neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
                loss3 = track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
                loss3[0].backward()
            torch.cuda.synchronize()
        grads = {k: p.grad for k, p in m.named_parameters()}
        assert len(grads) == 83 and all(g is not None for g in grads.values()), f"{name}: {len(grads)} gradients"
        d = os.path.join(out, name)
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "loss3.npy"), loss3.detach().cpu().numpy())
        for k, g in grads.items():
            np.save(os.path.join(d, k + ".npy"), g.detach().cpu().numpy())
        print(f"{name}: loss {[float(x) for x in loss3.detach().cpu()]}, {len(grads)} gradients", flush=True)


def compare(a, b):
    bad = 0
    cases_a, cases_b = sorted(os.listdir(a)), sorted(os.listdir(b))
    if cases_a != cases_b:
        print("different cases:", sorted(set(cases_a) ^ set(cases_b)))
        bad += 1
    for case in sorted(set(cases_a) & set(cases_b)):
        fa, fb = sorted(os.listdir(os.path.join(a, case))), sorted(os.listdir(os.path.join(b, case)))
        diff = [f for f in sorted(set(fa) ^ set(fb))]
        for f in sorted(set(fa) & set(fb)):
            x, y = np.load(os.path.join(a, case, f)), np.load(os.path.join(b, case, f))
            if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)):
                diff.append(f)
        print(f"{case}: {len(fa)} arrays, " + ("bit-equal" if not diff else f"DIFFERENT: {diff}"))
        bad += bool(diff)
    return bad


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
