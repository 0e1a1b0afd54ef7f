#!/usr/bin/env python3
"""Headline benchmark: track-selection forward + loss samples/s at (T=32, N=64, d=256) on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR   # + the last timed step's outputs as DIR/<name>.npy
    python bench.py --gpus 1 --steps 20 --warmup 3 --full               # + every leg listed below the headline's own fields

One "step" = one pass of the hot path (sola_forward + sola_loss + sola_select through the C ABI) over a batch of
``--batch`` independent synthetic (video, expression) samples already resident in HBM.  The conv weights are
re-standardised on every step, as the reference does on every forward (module/ws.py:9-13).  With N GPUs every rank
runs its own batch (per-sample sharding, no data-path collective): weak scaling, value = all samples / max-rank time.

Arithmetic of the convs/projections (98 % of the FLOPs), --precision:
  f16x3 (default) every f32 operand value is carried as an (f16 hi, f16 lo) pair in the same 4 bytes and each product is
        hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with f32 accumulation (~22-bit products), with device-side
        power-of-two scales for the caller's tokens and every weight matrix and a range guard that repeats a call on the
        exact-f32 kernels if a value leaves the format's range (include/sola_hip.h: sola_set_split_guard; the guard's
        read-back is inside the timed region).  It meets the same parity bar as exact f32 at every input scale
        (tests/test_gpu_range.py: every row of three 256-sample batches in both modes; the two sit in the same error class).
  f32   exact v_mfma_f32_32x32x2_f32.  With --full, the default mode also times the same workload on this path after the
        timed region and reports it as "exact_f32_mode" with its own roofline entries.

The ONE JSON line carries the driver's contract plus what the timed region itself yields (rank 0):
  roofline            the dominant kernel of the headline mode.  `achieved` / `frac` are ALGORITHMIC (2MNK per GEMM) against
                      the dense MFMA peak of the instruction the kernel issues; the split-f16 kernel executes 3 f16 MFMA
                      products per algorithmic product, so `achieved_executed` / `frac_executed` give the matrix-pipe view
  roofline_attention  the attention-core kernel named by the north star, against the 8 TB/s HBM peak
A plain run does nothing else: set-up, warm-up, the timed steps, --dump-outputs, the line.  Everything that takes runs of its
own comes with --full (rank 0; the legs after the timed region run at N=1 only):
  kernel_ms_per_step  per-category kernel time from an untimed pass of the same steps right behind the timed region
  max_abs_logit_err_vs_oracle / max_abs_logit_err_vs_reference
                      every row of the timed batch against the fp32 oracle / the reference's own logits (at N > 1: every rank's)
  exact_f32_mode      the same step on the exact-f32 kernels: value + roofline (f32 MFMA peak) + roofline_attention
  stress_T128_N128    BASELINE config C4 (T=128, N=128): value + roofline + roofline_attention
  ragged              sola_forward_ragged on a MeViS-like mix (N 8..80, T 20..200, L 4..24): one expression per video, and
                      four expressions per video (the text-independent half runs once per video)
  f16_storage_mode    the 16-bit activation storage mode at the headline shape and at C4 (reduced precision, stated tolerance)
  iou                 the mask-IoU de-dup predicate at its real call sizes (P=4 x R=16/64/256 at 540x960): HBM roofline + CPU
  training_step       one optimizer step at up to 64 samples, three precisions, with the per-kernel breakdown; .ragged = the same
                      step over 64 samples of DIFFERENT shapes (the MeViS-like mix); .one_sample_per_step = the reference's regime
  training_step_dist  --gpus N > 1 only: the training step on every rank with the gradient all-reduce overlapped / not overlapped /
                      left out, the all-reduce alone (ms, bus GB/s), and a ragged inference batch per rank
  cpu_baseline        the PyTorch-CPU oracle (a port of the reference path) timed on this box's host cores
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA (the 5 PF marketing figure is 2:1 sparse)
HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E spec peak
POS_W, TEMP, ALIGN_W = 1.5, 0.07, 0.3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="samples per step per GPU")
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--text-len", type=int, default=16)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, run every other leg (kernel breakdown, parity, exact f32, other shapes and modes, "
                         "training, CPU baseline); a plain run reports the timed region alone")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: budget of the cpu_baseline leg (0 = skip)")
    ap.add_argument("--train-steps", type=int, default=5, help="--full: steps of the training_step leg (rank 0, N=1, outside the timed region; 0 = skip)")
    ap.add_argument("--extra-legs", type=int, default=1, help="--full: 0 skips the stress / ragged / iou legs (profiling runs)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE", help="sola_tune switch for A/B measurements (reported in config.tune; not the default line)")
    ap.add_argument("--cached-ws", action="store_true", help="inference mode: standardise conv weights once (not the headline)")
    ap.add_argument("--precision", choices=["f32", "f16x3"], default=os.environ.get("SOLA_PRECISION", "f16x3"),
                    help="arithmetic of the convs/projections: exact f32 MFMA, or split-f16 operands (3 f16 MFMAs per product, "
                         "f32 accumulate, ~22-bit products; same 1e-3 parity bar)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) as DIR/<name>.npy, float32, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ------------------------------------------------------------------------------------------------------------ helpers
def cpu_info():
    model, phys = "unknown", None
    try:
        cores = set()
        pkg = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                pkg = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if pkg is not None and core is not None:
                    cores.add((pkg, core))
                pkg = core = None
        phys = len(cores) or None
    except OSError:
        pass
    return model, phys


def timed(fn, steps, sync, warmup=2):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def profiled(fn, steps, sync, warmup=2):
    """(seconds per step, per-category profile of the timed steps)"""
    from sola_amd import _lib

    for _ in range(warmup):
        fn()
    sync()
    _lib.profile_enable(True)
    _lib.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    dt = (time.perf_counter() - t0) / steps
    prof = _lib.profile_read(reset=True)
    _lib.profile_enable(False)
    return dt, prof


def gemm_roofline(prof, precision, step_s, steps):
    """Dominant GEMM kernel of a profiled leg, ALGORITHMIC flops (2MNK summed over its launches) / HIP-event time."""
    if precision == "f16x3":
        g256, grest = prof["gemm_split256"], prof["gemm_split"]
        g = g256 if g256["ms"] >= grest["ms"] else grest
        if g["ms"] <= 0:
            return None
        alg = g["flops"] / (g["ms"] * 1e-3) / 1e12
        name = ("gemm_nt_split_glds_persist_kernel<conv, residual, split-out> (persistent 256x256x32 blocks, 8 waves of 128x64, "
                "split-f16 operands, 3 x v_mfma_f32_32x32x16_f16 per product, direct-to-LDS staging; all plain-GEMM instantiations of a step - "
                "the launches that also apply GroupNorm + LeakyReLU in the epilogue are timed apart, kernel_ms_per_step.gemm_split256_gn)") \
            if g is g256 else "gemm_nt_split_glds_kernel<2,2,2,*> / gemm_nt_f32_kernel<64,64,1,1> (128x128 and 64x64 split-f16 blocks)"
        return {"kernel": name, "bound": "mfma", "achieved": round(alg, 2), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(alg / F16_MFMA_PEAK_TFLOPS, 4), "frac_algorithmic": round(alg / F16_MFMA_PEAK_TFLOPS, 4),
                "achieved_executed": round(3 * alg, 2), "frac_executed": round(3 * alg / F16_MFMA_PEAK_TFLOPS, 4),
                "what": "achieved/frac: algorithmic 2MNK flops per second vs the dense f16 MFMA peak; *_executed: the 3 f16 MFMA "
                        "products the kernel issues per algorithmic product (hi*hi + hi*lo + lo*hi)",
                "algorithmic_vs_f32_mfma_peak": round(alg / F32_MFMA_PEAK_TFLOPS, 3), "traffic": None,
                "launches": g["launches"], "avg_launch_us": round(1e3 * g["ms"] / max(1, g["launches"]), 2),
                "share_of_step_time": round(g["ms"] * 1e-3 / (step_s * steps), 4),
                "fused_norm_launches": {"launches": prof["gemm_split256_gn"]["launches"], "ms_per_step": round(prof["gemm_split256_gn"]["ms"] / steps, 4),
                                        "algorithmic_tflops": round(prof["gemm_split256_gn"]["flops"] / max(prof["gemm_split256_gn"]["ms"] * 1e-3, 1e-12) / 1e12, 2)}}
    g = prof["gemm128"] if prof["gemm128"]["ms"] >= prof["gemm64"]["ms"] else prof["gemm64"]
    if g["ms"] <= 0:
        return None
    ach = g["flops"] / (g["ms"] * 1e-3) / 1e12
    return {"kernel": "gemm_nt_f32_persist_kernel (persistent 256x128 tiles, buffer-load DMA to LDS, v_mfma_f32_32x32x2_f32, exact f32; launches whose grid "
                      "does not fill whole rounds: gemm_nt_f32_kernel<128,128>)" if g is prof["gemm128"] else "gemm_nt_f32_kernel<64,64>",
            "bound": "mfma", "achieved": round(ach, 2), "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / F32_MFMA_PEAK_TFLOPS, 4), "traffic": None, "launches": g["launches"],
            "avg_launch_us": round(1e3 * g["ms"] / max(1, g["launches"]), 2), "share_of_step_time": round(g["ms"] * 1e-3 / (step_s * steps), 4)}


def attn_roofline(prof):
    """Attention core of a profiled leg: algorithmic bytes (q, k, v read + o written) per second against the HBM peak, and - the
    exact-f32 kernels compute QK^T and PV on v_mfma_f32_16x16x4_f32 - the algorithmic 4*Sq*Sk*dh flops per (unit, head) against
    the f32 MFMA peak: from ~80 keys per unit on, the matrix pipe's time at its peak rate exceeds the HBM time (N = 128: 219 us vs
    134 us per inter-object launch), so `frac` alone understates those shapes; `bound` names the larger of the two fractions."""
    a = prof["attn"]
    if a["ms"] <= 0:
        return None
    gbs = a["bytes"] / (a["ms"] * 1e-3) / 1e9
    tfs = a["flops"] / (a["ms"] * 1e-3) / 1e12
    f_hbm, f_mfma = gbs / HBM_PEAK_GBS, tfs / F32_MFMA_PEAK_TFLOPS
    return {"kernel": "attention core, all launches of a step: attn_fwd_f32_simple_kernel (inter-object), attn_fwd_small_kernel / attn_fwd_f32_reg_kernel "
                      "(motion), attn_fwd_f32_res_kernel (object->language); exact f32", "bound": "hbm" if f_hbm >= f_mfma else "mfma",
            "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(f_hbm, 4), "traffic": None, "launches": a["launches"],
            "avg_launch_us": round(1e3 * a["ms"] / max(1, a["launches"]), 2),
            "f32_mfma_side": {"achieved": round(tfs, 1), "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(f_mfma, 4)}}


def kernel_ms(prof, steps):
    return {k: round(v["ms"] / steps, 4) for k, v in prof.items() if v["launches"]}


# --------------------------------------------------------------------------------------------------------------- legs
def cpu_baseline(cfg, sd, N, T, L, budget_s):
    """The oracle (PyTorch-CPU restatement of the reference path) on a bounded sample: batch-1 forward + loss
    iterations at the headline shape, all host cores, until ~budget_s seconds are used."""
    from oracle import sola_oracle
    from sola_amd import synth

    ncpu = os.cpu_count() or 1
    tsd = sola_oracle.to_torch_state(sd)
    inp = synth.make_inputs(cfg, 1, N, T, L, 0)
    neg = np.broadcast_to(sd["negative_token.weight"][None], (1,) + sd["negative_token.weight"].shape)

    def one():
        with torch.no_grad():
            sm, st = sola_oracle.forward(tsd, cfg, inp["object_tokens"], inp["lang_tokens"])
            sola_oracle.losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
            sola_oracle.select(sm)

    # torch's intra-op pool collapses when every SMT thread of a 2-socket host joins ops this small (39 s/sample at
    # 256 threads on the EPYC 9575F box), so the baseline gets the thread count that serves it best.
    cands = sorted({c for c in (1, 8, 16, 32, 64, 128, ncpu) if c <= ncpu})
    trials = {}
    for c in cands:
        torch.set_num_threads(c)
        t0 = time.perf_counter()
        one()
        if time.perf_counter() - t0 > 3.0:  # hopeless at this width; do not burn the budget
            trials[c] = time.perf_counter() - t0
            continue
        t0 = time.perf_counter()
        one()
        one()
        trials[c] = (time.perf_counter() - t0) / 2
    best = min(trials, key=trials.get)
    torch.set_num_threads(best)
    t0 = time.perf_counter()
    it = 0
    while True:
        one()
        it += 1
        el = time.perf_counter() - t0
        if el >= budget_s or it >= 2000:
            break
    sweep = ", ".join(f"{c}t:{1e3 * v:.0f}ms" for c, v in trials.items())
    model, phys = cpu_info()
    return {"value": round(it / el, 3), "unit": "samples/s", "cores": best, "kind": "port", "cpu_model": model, "physical_cores": phys,
            "logical_cpus": ncpu, "one_thread_value": round(1.0 / trials[1], 3) if 1 in trials else None,
            "sample": f"{it} batch-1 fwd+loss iterations of the PyTorch-CPU oracle at (T={T},N={N},L={L}) in {el:.1f} s, {best} threads",
            "thread_sweep": sweep}


def training_leg(cfg, sd, dev, B, N, T, L, steps, oracle_parity=None):
    """Outside the timed region, rank 0 at N=1 only: one optimizer step of the same network (sola_forward_train + losses +
    sola_backward + gradient norms / clip + AdamW) at up to 64 samples: exact f32, split-f16 GEMMs, f16-operand GEMMs."""
    from sola_amd import synth
    from sola_amd.loss import track_selection_losses
    from sola_amd.module import LanguageAlignedTrackSelectionModule, collate_ragged

    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5, fused=True)  # as train.py
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, B, N, T, L, 1).items()}

    def step():
        opt.zero_grad(set_to_none=True)
        sm, st = m(inp["object_tokens"], inp["lang_tokens"])
        neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
        loss3 = track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
        loss3[0].backward()
        m.optimizer_step(opt, 1.0)  # clip + AdamW as one launch with torch's fused arithmetic (sola_adamw_step; bit-identical to clip_grad_norm_ + opt.step())

    fl = synth.flops_per_sample(cfg, N, T, L)
    res = {"batch": B, "steps": steps, "unit": "samples/s",
           "what": "forward_train + BCE/alignment losses + backward + clip + AdamW; dropout on, one GPU",
           "gflop_per_sample_fwd_bwd": round(3 * fl["total"] / 1e9, 2)}
    sync = lambda: torch.cuda.synchronize(dev)
    for prec in ("f32", "f16x3", "f16", "bf16"):
        m.precision = prec
        dt = timed(step, steps, sync)
        _dtp, prof = profiled(step, max(2, steps // 2), sync, warmup=0)
        kms = kernel_ms(prof, max(2, steps // 2))
        gk = "gemm128" if prec == "f32" else "gemm_split256"
        g = prof[gk]
        alg = g["flops"] / (g["ms"] * 1e-3) / 1e12 if g["ms"] > 0 else 0.0
        peak = F32_MFMA_PEAK_TFLOPS if prec == "f32" else F16_MFMA_PEAK_TFLOPS
        res[prec] = {"value": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3), "model_tflops": round(3 * fl["total"] * B / dt / 1e12, 1),
                     "kernel_ms_per_step": kms,
                     "roofline": {"kernel": gk + " (forward, dX and dW GEMMs of the step)", "bound": "mfma", "achieved": round(alg, 2),
                                  "peak": peak, "unit": "TFLOP/s", "frac": round(alg / peak, 4),
                                  **({"achieved_executed": round(3 * alg, 2), "frac_executed": round(3 * alg / peak, 4)} if prec == "f16x3" else {}),
                                  "avg_launch_us": round(1e3 * g["ms"] / max(1, g["launches"]), 2)}}
        if prec == "f16":
            res[prec]["what"] = ("mixed precision (BASELINE config C2): every GEMM of the step on plain f16 casts of the f32 activations / "
                                 "gradients, f32 accumulation, ONE MFMA per product; everything else f32.  Reduced precision: losses within "
                                 "1 %, gradient cosine >= 0.95 against the exact-f32 step (tests/test_gpu_backward.py)")
        if prec == "f16x3":
            res[prec]["what"] = ("every GEMM of the step on split-f16 casts (3 f16 MFMAs per product) except the weight-gradient products dW = dY^T X, "
                                 "which sum over all token rows and take plain f16 operands (sola_tune train_dw_f16, default 1: median per-matrix error "
                                 "1e-4 against the exact-f32 step, worst tensor and gradient cosine unchanged; 0 = split pairs there too)")
        if prec == "bf16":
            res[prec]["what"] = ("the same mixed-precision step with BFLOAT16 GEMM operands (v_mfma_f32_32x32x16_bf16), the format BASELINE "
                                 "config C2 names; 8 significant bits, tolerance stated in tests/test_gpu_backward.py (LOWP_TRAIN_TOL)")
    # the reference's own regime: ONE sample per optimizer step (configs/mevis/default.yaml:37 batch_size 1), which is also what
    # train.py runs on variable-shape data (sola_forward_train takes one uniform batch)
    inp1 = {k: v[:1].contiguous() for k, v in inp.items()}

    def step1_autograd():
        opt.zero_grad(set_to_none=True)
        sm, st = m(inp1["object_tokens"], inp1["lang_tokens"])
        neg = m.negative_token.weight.clone().unsqueeze(0)
        loss3 = track_selection_losses(sm, st, inp1["labels"], inp1["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
        loss3[0].backward()
        m.clip_grad_norm_(1.0)
        opt.step()

    def step1():  # round 5: the same step with its device work enqueued by ONE library call (module.train_step -> sola_train_step; bit-identical)
        # ... and clipping + AdamW as one more launch with torch's fused arithmetic (sola_adamw_step: bit-identical parameters and moments)
        # (write_back_grads=False, as train.py calls it: an active clip does not rewrite .grad, which the loop never reads again)
        m.train_step(inp1["object_tokens"], inp1["lang_tokens"], inp1["labels"], inp1["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0, optimizer=opt,
                     write_back_grads=False)

    # variable-shape samples in ONE step (sola_forward_train_ragged / sola_backward_ragged): the MeViS-like mix of the ragged
    # inference leg (N~U[8,80], T~U[20,200], L~U[4,24]); objective = mean of the per-sample totals
    from sola_amd.loss import track_selection_losses_ragged

    S = 64
    smp = synth.make_ragged_samples(cfg, S, 2024, dev)
    objs, langs = collate_ragged([x["obj"] for x in smp]), collate_ragged([x["lang"] for x in smp])  # as a collate function hands them over: views of one buffer
    rlabels = torch.cat([x["labels"] for x in smp])
    rpos = torch.stack([x["pos"] for x in smp])
    rflops = sum(synth.flops_per_sample(cfg, int(o.shape[0]), int(o.shape[1]), int(t.shape[0]))["total"] for o, t in zip(objs, langs))

    def step_ragged():
        opt.zero_grad(set_to_none=True)
        m.forward_ragged(objs, langs)
        flat, tok, offs, counts = m.last_ragged
        loss = track_selection_losses_ragged(flat, tok, rlabels, rpos, m.negative_token.weight, offs, counts, POS_W, TEMP, ALIGN_W)
        loss[:, 0].mean().backward()
        m.optimizer_step(opt, 1.0)  # clip + AdamW as one launch with torch's fused arithmetic (sola_adamw_step; bit-identical to clip_grad_norm_ + opt.step())

    rag = {"samples_per_step": S, "shapes": "N~U[8,80], T~U[20,200], L~U[4,24], seed 2024", "unit": "samples/s",
           "object_token_rows": int(sum(o.shape[0] * o.shape[1] for o in objs)),
           "gflop_per_sample_fwd_bwd": round(3 * rflops / S / 1e9, 2),
           "what": "one optimizer step over 64 samples of different shapes: sola_forward_train_ragged + per-sample losses + "
                   "sola_backward_ragged + clip + AdamW; dropout on; a sample of this mix costs "
                   f"{rflops / S / fl['total']:.2f}x the headline shape's FLOPs"}
    for prec in ("f32", "f16x3", "f16", "bf16"):
        m.precision = prec
        dtr = timed(step_ragged, max(4, steps), sync)  # (two timed steps let one allocator hiccup move the figure by 20 %)
        _d, profr = profiled(step_ragged, 2, sync, warmup=0)
        rag[prec] = {"value": round(S / dtr, 1), "ms_per_step": round(dtr * 1e3, 3), "model_tflops": round(3 * rflops / dtr / 1e12, 1),
                     "kernel_ms_per_step": kernel_ms(profr, 2)}
    # the same leg at 128 samples per step, 16-bit GEMM operands: the per-step costs that do not scale with the rows (launches, the
    # optimizer, the weight-side casts) are halved per sample
    S2 = 128
    smp = synth.make_ragged_samples(cfg, S2, 2025, dev)
    objs, langs = collate_ragged([x["obj"] for x in smp]), collate_ragged([x["lang"] for x in smp])  # as a collate function hands them over: views of one buffer
    rlabels = torch.cat([x["labels"] for x in smp])
    rpos = torch.stack([x["pos"] for x in smp])
    rflops2 = sum(synth.flops_per_sample(cfg, int(o.shape[0]), int(o.shape[1]), int(t.shape[0]))["total"] for o, t in zip(objs, langs))
    rag["samples_per_step_128"] = {"object_token_rows": int(sum(o.shape[0] * o.shape[1] for o in objs)), "seed": 2025}
    for prec in ("f16", "bf16"):
        m.precision = prec
        dtr = timed(step_ragged, max(4, steps), sync)  # (two timed steps let one allocator hiccup move the figure by 20 %)
        rag["samples_per_step_128"][prec] = {"value": round(S2 / dtr, 1), "ms_per_step": round(dtr * 1e3, 3),
                                             "model_tflops": round(3 * rflops2 / dtr / 1e12, 1)}
    res["ragged"] = rag
    del smp, objs, langs
    m.precision = "f32"
    dt1 = timed(step1, max(steps, 50), sync, warmup=5)
    dt1a = timed(step1_autograd, max(steps, 50), sync, warmup=5)
    res["one_sample_per_step"] = {"value": round(1.0 / dt1, 1), "ms_per_step": round(dt1 * 1e3, 3), "precision": "f32",
                                  "autograd_path_ms": round(dt1a * 1e3, 3),
                                  "what": "the reference's training batch size (module.train_step: the step's device work in one library call, then "
                                          "torch's fused AdamW; autograd_path_ms: the same step call by call through autograd); below 1024 token rows "
                                          "every precision mode runs the exact-f32 kernels"}
    if oracle_parity:  # the TRAINING forward of the 64-sample ragged batch (sola_forward_train_ragged, dropout off), every logit against the fp32
        # oracle - on the ORIGINAL weights: the timed steps above have updated the module's
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m.weights_changed()
        m.eval()
        smp = synth.make_ragged_samples(cfg, S, 2024, dev)
        objs, langs = collate_ragged([x["obj"] for x in smp]), collate_ragged([x["lang"] for x in smp])  # as a collate function hands them over: views of one buffer
        bt = {"sample_video": list(range(S)), "videos": [o.cpu().numpy() for o in objs], "texts": [t.cpu().numpy() for t in langs]}
        ref = oracle_ragged_rows(cfg, oracle_parity, bt)
        rag["train_forward_logit_err_vs_oracle"] = {}
        for prec in ("f32", "f16x3"):
            m.precision = prec
            m.forward_ragged(objs, langs, differentiable=True)
            rag["train_forward_logit_err_vs_oracle"][prec] = row_errors(m.last_ragged[0].detach().cpu().numpy(), ref, m.last_ragged[3])
            if reference_logits("rag_train.2024") is not None:
                rag.setdefault("train_forward_logit_err_vs_reference", {})[prec] = row_errors(m.last_ragged[0].detach().cpu().numpy(),
                                                                                              reference_logits("rag_train.2024"), m.last_ragged[3])
        m.train()
        del smp, objs, langs
    del m, opt
    torch.cuda.empty_cache()
    return res


def dist_legs(cfg, sd, dev, world, rank, steps):
    """--gpus N > 1, after the timed region, every rank: (a) the training step with the path's ONE collective - the all-reduce of the
    131.9 MB gradient arena (train.py under torchrun; SURVEY 8e, BASELINE config C2) - with the per-bucket overlap on and off, and
    the all-reduce alone; (b) a ragged inference batch per rank (per-video sharding, no collective).  Times are max over ranks."""
    import torch.distributed as dist

    from sola_amd import dist as sdist
    from sola_amd import synth
    from sola_amd.loss import track_selection_losses, track_selection_losses_ragged
    from sola_amd.module import LanguageAlignedTrackSelectionModule, collate_ragged  # noqa: F401

    def max_over_ranks(x):
        t = torch.tensor([x], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed_all(fn, n, warmup=2):
        for _ in range(warmup):
            fn()
        dist.barrier(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        dist.barrier(); torch.cuda.synchronize(dev)
        return max_over_ranks((time.perf_counter() - t0) / n)

    B, N, T, L = 64, 64, 32, 16
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5, fused=True)
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, B, N, T, L, 7000 + rank).items()}
    state = {"overlap": True, "reduce": True}

    def step():
        opt.zero_grad(set_to_none=True)
        sm, st = m(inp["object_tokens"], inp["lang_tokens"])
        neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
        track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)[0].backward()
        if state["reduce"]:
            sdist.allreduce_gradient_arena(m, world, overlap=state["overlap"])
        m.clip_grad_norm_(1.0)
        opt.step()

    res = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "precision": m.train_precision, "samples_per_rank_per_step": B,
           "what": "forward_train + losses + backward + all-reduce (AVG) of the flat gradient arena + clip + AdamW on every rank; "
                   "the buckets of the arena are reduced in place on a side stream as sola_backward completes them (overlap) or after it"}
    for tag, ov, red in (("overlap", True, True), ("no_overlap", False, True), ("no_collective", True, False)):
        state["overlap"], state["reduce"] = ov, red
        dt = timed_all(step, steps)
        res[tag] = {"ms_per_step": round(dt * 1e3, 3), "value": round(world * B / dt, 1), "unit": "samples/s (all ranks)"}
    flat = torch.cat([b.reshape(-1) for b in m.grad_buckets()]) if getattr(m, "_grad_arena", None) is None else m._grad_arena
    nbytes = flat.numel() * 4

    def ar():
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)

    dta = timed_all(ar, max(3, steps))
    res["allreduce_alone"] = {"bytes": int(nbytes), "ms": round(dta * 1e3, 3), "algbw_GBps": round(nbytes / dta / 1e9, 2),
                              "busbw_GBps": round(2 * (world - 1) / world * nbytes / dta / 1e9, 2),
                              "exposed_ms_with_overlap": round((res["overlap"]["ms_per_step"] - res["no_collective"]["ms_per_step"]), 3),
                              "exposed_ms_without_overlap": round((res["no_overlap"]["ms_per_step"] - res["no_collective"]["ms_per_step"]), 3)}
    del opt
    # (b) ragged inference, one batch per rank
    m.eval()
    S = 64
    smp = synth.make_ragged_samples(cfg, S, 3000 + rank, dev)
    objs, langs = collate_ragged([x["obj"] for x in smp]), collate_ragged([x["lang"] for x in smp])  # as a collate function hands them over: views of one buffer
    labels = torch.cat([x["labels"] for x in smp]); pos = torch.stack([x["pos"] for x in smp])

    def rstep():
        with torch.no_grad():
            m.forward_ragged(objs, langs)
            flat_sm, tok, offs, counts = m.last_ragged
            track_selection_losses_ragged(flat_sm, tok, labels, pos, m.negative_token.weight, offs, counts, POS_W, TEMP, ALIGN_W)

    dtr = timed_all(rstep, steps)
    res["ragged_inference"] = {"samples_per_rank_per_launch": S, "shapes": "N~U[8,80], T~U[20,200], L~U[4,24], seed 3000 + rank",
                               "ms_per_launch": round(dtr * 1e3, 3), "value": round(world * S / dtr, 1), "unit": "samples/s (all ranks)"}
    del m
    torch.cuda.empty_cache()
    return res


def stress_leg(cfg, m, dev, precision, steps):
    """BASELINE config C4: long-video stress T=128, N=128 (T'=16, 2048 tokens per sample), 32 samples per step."""
    from sola_amd import ops, synth
    from sola_amd.loss import track_selection_losses

    B, N, T, L = 32, 128, 128, 16
    inp = synth.make_inputs(cfg, B, N, T, L, seed=77)
    c = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}

    def step():
        with torch.no_grad():
            sm, st = m(c["object_tokens"], c["lang_tokens"])
            track_selection_losses(sm, st, c["labels"], c["pos_tokens"], m.negative_token.weight, POS_W, TEMP, ALIGN_W)
            ops.select(sm, 0.5)

    sync = lambda: torch.cuda.synchronize(dev)
    dt, prof = profiled(step, steps, sync)
    fl = synth.flops_per_sample(cfg, N, T, L)
    out = {"workload": f"T={T} N={N} L={L}, {B} samples/step", "value": round(B / dt, 2), "unit": "samples/s", "ms_per_step": round(dt * 1e3, 3),
           "gflop_per_sample": round(fl["total"] / 1e9, 2), "model_tflops": round(B / dt * fl["total"] / 1e12, 2),
           "roofline": gemm_roofline(prof, precision, dt, steps), "roofline_attention": attn_roofline(prof),
           "kernel_ms_per_step": kernel_ms(prof, steps)}
    ref_gold = reference_logits("c4.77")
    if ref_gold is not None:  # every row of this batch against the reference's own logits
        with torch.no_grad():
            out["logit_err_vs_reference"] = uniform_row_errors(m(c["object_tokens"], c["lang_tokens"])[0].cpu().numpy(), ref_gold)
    del c
    torch.cuda.empty_cache()
    return out


def f16_storage_leg(cfg, m, dev, steps):
    """The 16-bit activation storage mode (module.precision = "f16"; BASELINE configs C2 / C4 name bf16 / fp16 runs): the same
    step at the headline shape and at C4, with the largest logit difference from the exact-f32 mode on the batch.  A
    reduced-precision mode (tolerance stated in tests/test_gpu_f16.py): reported beside the headline, never as it."""
    from sola_amd import ops, synth
    from sola_amd.loss import track_selection_losses

    out = {"what": "plain f16 between kernels (2 B per activation element), one f16 MFMA per product, f32 accumulate / softmax / statistics; "
                   "device-side scales + range guard with exact-f32 repeat",
           "tolerance": "heavy-tailed: logits (magnitude ~10) within 1.5 % rms, at most 0.5 % of them beyond 0.25, none beyond 1.0 "
                        "(tests/test_gpu_f16.py: every row of three 256-sample batches against the oracle)"}
    sync = lambda: torch.cuda.synchronize(dev)
    keep = m.precision
    for tag, (B, N, T, L) in (("NS_T32_N64", (256, 64, 32, 16)), ("C4_T128_N128", (32, 128, 128, 16))):
        c = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, B, N, T, L, seed=1000).items()}

        def step():
            with torch.no_grad():
                sm, st = m(c["object_tokens"], c["lang_tokens"])
                track_selection_losses(sm, st, c["labels"], c["pos_tokens"], m.negative_token.weight, POS_W, TEMP, ALIGN_W)
                ops.select(sm, 0.5)
            return sm

        m.precision = "f32"
        ref = step()
        m.precision = "f16"
        dt, prof = profiled(step, steps, sync)
        sm = step()
        fl = synth.flops_per_sample(cfg, N, T, L)
        a = prof["attn"]
        g = prof["gemm_split256"]
        alg = g["flops"] / (g["ms"] * 1e-3) / 1e12 if g["ms"] > 0 else 0.0
        out[tag] = {"value": round(B / dt, 1), "unit": "samples/s", "ms_per_step": round(dt * 1e3, 3), "model_tflops": round(B / dt * fl["total"] / 1e12, 1),
                    "max_abs_logit_diff_vs_f32_mode": float((sm - ref).abs().max()),
                    "rms_logit_diff_vs_f32_mode": float((sm - ref).pow(2).mean().sqrt()), "calls_repeated_in_f32": m.split_fallbacks()[0],
                    "roofline": {"kernel": "gemm_nt_split_glds_persist_kernel<*, PURE> (f16 operands, one v_mfma_f32_32x32x16_f16 per product)",
                                 "bound": "mfma", "achieved": round(alg, 1), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                 "frac": round(alg / F16_MFMA_PEAK_TFLOPS, 4)},
                    "roofline_attention": {"kernel": "attn_fwd_f16_kernel", "bound": "hbm", "achieved": round(a["bytes"] / (a["ms"] * 1e-3) / 1e9, 1),
                                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(a["bytes"] / (a["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                           "what": "algorithmic bytes at 2 B per element"},
                    "kernel_ms_per_step": kernel_ms(prof, steps)}
        del c
        torch.cuda.empty_cache()
    # the ragged path under the same mode (round 3: inference.py / eval.py call only this path): the MeViS-like mix, four
    # expressions per video, against the same call in the default split-f16 mode
    from sola_amd.loss import track_selection_losses_ragged
    from sola_amd.module import collate_ragged

    rng = np.random.Generator(np.random.PCG64(2024))
    S, per_video = 128, 4
    d, D = cfg["object_token_dim"], cfg["lang_token_dim"]
    shapes = [(int(rng.integers(8, 81)), int(rng.integers(20, 201))) for _ in range(S // per_video)]
    lens = [int(rng.integers(4, 25)) for _ in range(S)]
    sample_video = [i // per_video for i in range(S)]
    videos = collate_ragged([torch.from_numpy(rng.standard_normal((n, t, d)).astype(np.float32)) for n, t in shapes], dev)
    texts = collate_ragged([torch.from_numpy(rng.standard_normal((ln, D)).astype(np.float32)) for ln in lens], dev)
    labels = torch.cat([torch.from_numpy((rng.uniform(size=shapes[v][0]) < 0.2).astype(np.float32)) for v in sample_video]).to(dev)
    pos = torch.stack([t.mean(0) for t in texts], 0)

    def rstep():
        m.forward_ragged(videos, texts, sample_video)
        flat, tok, offs, counts = m.last_ragged
        track_selection_losses_ragged(flat, tok, labels, pos, m.negative_token.weight, offs, counts, POS_W, TEMP, ALIGN_W)
        ops.select(flat, 0.5)
        return flat

    m.precision = "f16x3"
    dt_ref = timed(rstep, steps, sync)
    ref = rstep().clone()
    m.precision = "f16"
    dt16 = timed(rstep, steps, sync)
    got = rstep()
    out["ragged_four_expressions_per_video"] = {
        "samples_per_launch": S, "value": round(S / dt16, 1), "unit": "samples/s", "ms_per_launch": round(dt16 * 1e3, 3),
        "split_f16_mode_value": round(S / dt_ref, 1), "max_abs_logit_diff_vs_split_mode": float((got - ref).abs().max()),
        "rms_logit_diff_vs_split_mode": float((got - ref).pow(2).mean().sqrt()), "calls_repeated_in_f32": m.split_fallbacks()[0]}
    del videos, texts
    torch.cuda.empty_cache()
    m.precision = keep
    return out


def ragged_leg(cfg, m, dev, steps, uniform_model_tflops, oracle_parity=None):
    """sola_forward_ragged + sola_loss_ragged + sola_select on a MeViS-like mix of shapes (N in [8,80] tracks, T in [20,200]
    frames, L in [4,24] text tokens; seeded), 128 samples per launch: (a) one expression per video, (b) four expressions per
    video.  FLOPs: `reference` = what per-sample forwards of these samples cost (the reference's batch-1 loop, and this
    library's sola_forward), `executed` = with the text-independent half computed once per video."""
    from sola_amd import ops, synth
    from sola_amd.loss import track_selection_losses_ragged
    from sola_amd.module import collate_ragged

    S = 128
    out = {"samples_per_launch": S, "shapes": "N~U[8,80], T~U[20,200], L~U[4,24], seed 2024"}
    batches = synth.make_ragged_infer_batches(cfg, S, 2024)
    for tag, bt in batches.items():
        per_video, shapes, lens, sample_video = bt["per_video"], bt["shapes"], bt["lens"], bt["sample_video"]
        V = S // per_video
        videos = collate_ragged([torch.from_numpy(v) for v in bt["videos"]], dev)  # views of one buffer (a collated batch)
        texts = collate_ragged([torch.from_numpy(t) for t in bt["texts"]], dev)
        labels = torch.cat([torch.from_numpy(l) for l in bt["labels"]]).to(dev)
        pos = torch.stack([t.mean(0) for t in texts], 0)

        def step():
            m.forward_ragged(videos, texts, sample_video)
            flat, tok, offs, counts = m.last_ragged
            track_selection_losses_ragged(flat, tok, labels, pos, m.negative_token.weight, offs, counts, POS_W, TEMP, ALIGN_W)
            ops.select(flat, 0.5)

        sync = lambda: torch.cuda.synchronize(dev)
        dt, prof = profiled(step, steps, sync)
        f_ref = f_exec = 0.0
        for i, v in enumerate(sample_video):
            n, t = shapes[v]
            fl = synth.flops_per_sample(cfg, n, t, lens[i])
            shared = fl["conv"] + synth.shared_flops_per_video(cfg, n, t)
            f_ref += fl["total"]
            f_exec += fl["total"] - shared + (shared if i % per_video == 0 else 0.0)
        rows = sum(n * t for n, t in shapes)
        out[tag] = {"videos": V, "value": round(S / dt, 1), "unit": "samples/s", "ms_per_launch": round(dt * 1e3, 3),
                    "object_token_rows": rows, "gflop_per_sample_reference": round(f_ref / S / 1e9, 2),
                    "model_tflops_reference": round(f_ref / dt / 1e12, 1), "model_tflops_executed": round(f_exec / dt / 1e12, 1),
                    "executed_vs_uniform_batch_model_tflops": round(f_exec / dt / 1e12 / uniform_model_tflops, 3) if uniform_model_tflops else None,
                    "roofline_attention": attn_roofline(prof), "kernel_ms_per_launch": kernel_ms(prof, steps)}
        if oracle_parity:  # EVERY logit of this batch against the fp32 oracle's per-sample forwards, this mode and exact f32
            ref = oracle_ragged_rows(cfg, oracle_parity, bt)
            keep = m.precision
            par = {}
            for prec in (keep, "f32"):
                m.precision = prec
                m.forward_ragged(videos, texts, sample_video)
                par[prec] = row_errors(m.last_ragged[0].cpu().numpy(), ref, m.last_ragged[3])
            m.precision = keep
            out[tag]["logit_err_vs_oracle"] = par
        ref_gold = reference_logits("rag_infer." + tag)
        if ref_gold is not None:  # the reference's own per-sample logits for this batch (no CPU work)
            keep = m.precision
            par = {}
            for prec in (keep, "f32"):
                m.precision = prec
                m.forward_ragged(videos, texts, sample_video)
                par[prec] = row_errors(m.last_ragged[0].cpu().numpy(), ref_gold, m.last_ragged[3])
            m.precision = keep
            out[tag]["logit_err_vs_reference"] = par
        del videos, texts
        torch.cuda.empty_cache()
    return out


def oracle_ragged_rows(cfg, tsd, bt):
    """fp32 oracle logits of every sample of a ragged batch (checker only): one per-sample forward each, concatenated."""
    from oracle import sola_oracle

    torch.set_num_threads(min(32, os.cpu_count() or 1))
    rows = []
    for i, v in enumerate(bt["sample_video"]):
        sm, _ = sola_oracle.forward(tsd, cfg, bt["videos"][v][None], bt["texts"][i][None])
        rows.append(np.asarray(sm)[0])
    return np.concatenate(rows)


_REF_GOLD = None


def reference_logits(key):
    """The REFERENCE's own logits for a benched batch (tests/golden/bench_golden.npz, made by tests/golden/gen_golden.py bench from
    module/module.py:130-162 called one sample per forward); None when the fixture or the key is absent.  A committed data file:
    nothing of the reference is read at run time."""
    global _REF_GOLD
    if _REF_GOLD is None:
        path = os.path.join(ROOT, "tests", "golden", "bench_golden.npz")
        _REF_GOLD = dict(np.load(path)) if os.path.exists(path) else {}
    return _REF_GOLD.get(key + ".score_map")


def uniform_row_errors(got, ref_flat):
    ref = ref_flat.reshape(got.shape).astype(np.float32)
    e_rows = np.abs(got - ref).max(axis=1)
    return {"max_abs_logit_err_vs_reference": float(e_rows.max()), "mean_row_max_err": float(e_rows.mean()), "rows_above_5e-4": int((e_rows > 5e-4).sum()),
            "rows": int(got.shape[0]), "selections_equal": bool(np.array_equal(got > 0, ref > 0))}


def row_errors(got, ref, counts):
    """Worst / mean-per-sample-worst absolute logit error, samples above 5e-4, equality of the selections (sigmoid > 0.5)."""
    e = np.abs(got - ref)
    per = np.array([e[o:o + c].max() for o, c in zip(np.cumsum([0] + list(counts[:-1])), counts)])
    return {"max": float(e.max()), "mean_sample_max": float(per.mean()), "samples_above_5e-4": int((per > 5e-4).sum()), "samples": len(counts),
            "selections_equal": bool(np.array_equal(got > 0, ref > 0))}


def call_pattern_leg(cfg, sd, dev, steps):
    """The reference's own call pattern (inference.py:58, evaluator.py:100: ONE sample per call) and the uniform BASELINE shapes besides
    the headline one (C0 (T=8, N=8), C1 (T=32, N=16) and (T=32, N=80)), each in both arithmetic modes.  S=1: wall time per call
    incl. the host side (forward + selection, the output left on the device).  Uniform shapes: samples/s at a batch of ~16 K layer tokens."""
    from sola_amd import ops, synth
    from sola_amd.module import LanguageAlignedTrackSelectionModule, collate_ragged  # noqa: F401

    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).eval()
    m.ws_policy = "always"
    sync = lambda: torch.cuda.synchronize(dev)
    out = {"one_sample_per_call_ms": {}, "uniform": {}}
    for tag, (N, T, L) in (("NS_N64_T32", (64, 32, 16)), ("N44_T110", (44, 110, 16))):
        inp = synth.make_inputs(cfg, 1, N, T, L, seed=5)
        obj, lang = torch.from_numpy(inp["object_tokens"]).to(dev), torch.from_numpy(inp["lang_tokens"]).to(dev)
        rec = {}
        for prec in ("f16x3", "f32"):
            m.precision = prec

            def call():
                with torch.no_grad():
                    sm, _ = m(obj, lang)
                    ops.select(sm, 0.5)

            rec[prec] = round(1e3 * timed(call, 50, sync, warmup=5), 4)
        out["one_sample_per_call_ms"][tag] = rec
    for tag, (N, T, B) in (("C0_T8_N8", (8, 8, 2048)), ("C1_T32_N16", (16, 32, 1024)), ("C1_T32_N80", (80, 32, 192))):
        inp = synth.make_inputs(cfg, B, N, T, 16, seed=6)
        obj, lang = torch.from_numpy(inp["object_tokens"]).to(dev), torch.from_numpy(inp["lang_tokens"]).to(dev)
        rec = {"samples": B}
        for prec in ("f16x3", "f32"):
            m.precision = prec

            def step():
                with torch.no_grad():
                    sm, _ = m(obj, lang)
                    ops.select(sm, 0.5)

            rec[prec] = round(B / timed(step, max(3, steps), sync, warmup=2), 1)
        out["uniform"][tag] = rec
        del obj, lang
    del m
    torch.cuda.empty_cache()
    return out


def iou_leg(dev, cpu_seconds):
    """The mask-IoU de-dup predicate (seg_utils.py:128-142 through generate_tokens_grid.py:266-278) at its real call sizes:
    P=4 new-track masks against R prompt masks at 540x960 uint8.  Algorithmic bytes = (P+R)*H*W (every mask read once)."""
    from oracle import iou_oracle
    from sola_amd import _lib, seg_utils

    H, W, P = 540, 960, 4
    rng = np.random.default_rng(0)

    def rects(n):
        out = np.zeros((n, H, W), np.uint8)
        for i in range(n):
            y0, x0 = rng.integers(0, H // 2), rng.integers(0, W // 2)
            out[i, y0:y0 + rng.integers(8, H // 2), x0:x0 + rng.integers(8, W // 2)] = 1
        return out

    res = {"workload": "compute_mask_iou matrix, P=4 tracks x R prompts, 540x960 uint8 masks resident in HBM", "cases": []}
    sync = lambda: torch.cuda.synchronize(dev)
    for R in (16, 64, 256):
        A, Bm = rects(P), rects(R)
        a, b = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev)
        inter, union = seg_utils.mask_iou_matrix(a, b)
        if R <= 64:
            ri, ru = iou_oracle.iou_matrix(A, Bm)
            assert np.array_equal(inter.cpu().numpy(), ri) and np.array_equal(union.cpu().numpy(), ru)
        # wall time WITHOUT the in-library event profiler (its two event records per launch cost a multi-launch call ~20 us:
        # round 2 reported 48 us for the three-launch R=64 call that takes 25 us), kernel time from a second, profiled loop
        dt = timed(lambda: seg_utils.mask_iou_matrix(a, b), 200, sync, warmup=5)
        _dtp, prof = profiled(lambda: seg_utils.mask_iou_matrix(a, b), 50, sync, warmup=2)
        k_ms = (prof["iou_pack"]["ms"] + prof["iou_pair"]["ms"]) / 50
        nbytes = (P + R) * H * W
        res["cases"].append({"R": R, "pairs": P * R, "call_us_wall": round(dt * 1e6, 1), "kernels_us": round(k_ms * 1e3, 1),
                             "launches_per_call": (prof["iou_pack"]["launches"] + prof["iou_pair"]["launches"]) // 50,
                             "pairs_per_s": round(P * R / dt),
                             "roofline": {"kernel": "mask IoU kernels of one call (pack + pair)", "bound": "hbm",
                                          "achieved": round(nbytes / (k_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "frac": round(nbytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes": nbytes,
                                          "frac_wall": round(nbytes / dt / 1e9 / HBM_PEAK_GBS, 4)}})
    if cpu_seconds > 0:
        A, Bm = rects(1), rects(8)
        t0 = time.perf_counter()
        it = 0
        while time.perf_counter() - t0 < min(3.0, cpu_seconds):
            iou_oracle.iou_matrix(A, Bm)
            it += 8
        el = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(it / el, 1), "unit": "pairs/s", "cores": 1, "kind": "port",
                               "sample": f"{it} mask pairs through the numpy oracle (oracle/iou_oracle.py) in {el:.1f} s, one thread"}
    return res


# ------------------------------------------------------------------------------------------------------ the printed line
# The driver keeps a bounded tail of stdout: the line that goes there carries NUMBERS (every leg, short keys) and stays under ~6 KB; the
# prose that explains a field lives in DESIGN.md 5 ("Fields of the bench line"), and the verbose object - every string this file
# builds - is written next to it as gpurun_out/bench_full.json (or $SOLA_BENCH_FULL).
_DROP = {"what", "tolerance", "shapes", "traffic_source", "traffic_kernel", "kernel_ms_per_step_source", "frac_algorithmic",
         "algorithmic_vs_f32_mfma_peak", "gflop_per_sample_reference", "object_token_rows", "launches_per_call", "algorithmic_bytes",
         "logical_cpus", "seed", "thread_sweep", "videos", "pairs", "gflop_per_sample_fwd_bwd", "model_tflops_reference",
         "executed_vs_uniform_batch_model_tflops", "pairs_per_s", "workload"}
_DROP_NESTED = {"model_tflops", "gflop_per_sample", "achieved", "avg_launch_us", "launches", "share_of_step_time", "steps", "dtype"}  # below the top level and its two rooflines
_KEEP_KERNEL_MS = {("kernel_ms_per_step",), ("training_step", "ragged", "f16x3", "kernel_ms_per_step"),
                   ("training_step", "ragged", "bf16", "kernel_ms_per_step"), ("training_step", "f16x3", "kernel_ms_per_step")}
_CONTRACT_ROOFLINES = {("roofline",), ("roofline_attention",)}
_OPTIONAL = [("iou", "cpu_baseline", "sample"), ("training_step", "f16x3", "kernel_ms_per_step"),
             ("f16_storage_mode", "ragged_four_expressions_per_video"), ("training_step", "ragged", "samples_per_step_128"),
             ("training_step", "ragged", "f16x3", "kernel_ms_per_step"), ("training_step", "ragged", "bf16", "kernel_ms_per_step"), ("stress_T128_N128", "kernel_ms_per_step"), ("iou", "cpu_baseline"),
             ("f16_storage_mode", "C4_T128_N128", "roofline"), ("f16_storage_mode", "NS_T32_N64", "roofline")]
_SHORT = {"max_abs_logit_err_vs_reference": "max", "max_abs_logit_err_vs_float64": "max_vs_f64", "reference_vs_float64": "ref_vs_f64",
          "train_forward_logit_err_vs_reference": "train_fwd_err_vs_reference",
          "max_abs_logit_err_vs_oracle": "max", "mean_row_max_err": "mean", "rows_above_5e-4": "gt5e-4", "samples_above_5e-4": "gt5e-4",
          "mean_sample_max": "mean", "selections_equal": "sel_eq", "max_abs_logit_diff_vs_f32_mode": "max_diff_f32",
          "rms_logit_diff_vs_f32_mode": "rms_diff_f32", "calls_repeated_in_f32": "f32_repeats", "max_abs_logit_diff_vs_split_mode": "max_diff_split",
          "rms_logit_diff_vs_split_mode": "rms_diff_split", "model_tflops_executed": "tflops_exec", "split_f16_mode_value": "split_value",
          "train_forward_logit_err_vs_oracle": "train_fwd_err_vs_oracle", "samples_per_launch": "samples", "samples_per_step": "samples",
          "max_abs_logit_diff_vs_split_mode ": "max_diff_split"}  # nested keys only (DESIGN.md 5 lists them)


def _sig(x, n=4):
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x == 0 or not np.isfinite(x):
        return x
    return float(f"{x:.{n}g}")


def compact(o, path=()):
    """The short form of the result object: explanatory strings, duplicated fields and most per-leg kernel tables dropped, kernel names cut
    at their template list, floats to four significant digits.  Contract keys of the top level and of its two rooflines are untouched."""
    if isinstance(o, dict):
        out = {}
        for k, v in o.items():
            p = path + (k,)
            if k in _DROP and p != ("config", "workload"):
                continue
            # nested legs: where every logit is compared with the REFERENCE's own (round 6), the same comparison with the oracle stays in the verbose file only
            if len(path) > 0 and ((k == "logit_err_vs_oracle" and "logit_err_vs_reference" in o) or
                                  (k == "train_forward_logit_err_vs_oracle" and "train_forward_logit_err_vs_reference" in o)):
                continue
            if k in _DROP_NESTED and len(path) > 0 and path not in _CONTRACT_ROOFLINES:
                continue
            if k in ("kernel_ms_per_step", "kernel_ms_per_launch") and p not in _KEEP_KERNEL_MS:
                continue
            if k == "f32_mfma_side" and isinstance(v, dict):
                out["mfma_frac"] = _sig(v.get("frac"))
                continue
            if k == "fused_norm_launches" and isinstance(v, dict) and not v.get("launches"):
                continue
            if k in ("unit", "peak", "bound") and len(path) > 0 and path not in _CONTRACT_ROOFLINES and path != ("cpu_baseline",):
                continue
            if k == "kernel" and isinstance(v, str):
                cut = min([i for i in (v.find("<"), v.find(" ("), v.find(",")) if i > 0] or [len(v)])
                out[k] = v[:cut][:48]
                continue
            if k == "sample" and isinstance(v, str):
                out[k] = v[:110]
                continue
            out[_SHORT.get(k, k) if len(path) > 0 else k] = compact(v, p)
        return out
    if isinstance(o, list):
        return [compact(v, path) for v in o]
    if isinstance(o, str) and len(path) > 1 and len(o) > 64 and path != ("config", "workload"):
        return o[:64]
    return _sig(o) if len(path) > 1 or path[:1] not in (("value",), ("ms_per_step",)) else o


DUMP_BYTES = 64_000_000


def dump_outputs(path, outs):
    """--dump-outputs: the arrays one timed step hands its caller, as float32 .npy files under ``path``: score_map [B,N], score_tokens
    [B,N,D], loss [total, bce, alignment], prob and pred [B,N] (ops.select).  score_tokens is written whole when everything fits in
    DUMP_BYTES, else as a fixed sample of its B*N rows (seed 0, sorted; score_tokens_rows.npy holds the flat row indices, float64)."""
    sm, st, loss3, prob, pred = (t.detach().float().cpu().numpy() for t in outs)
    small = {"score_map": sm, "loss": loss3, "prob": prob, "pred": pred}
    arrays = dict(small)
    rows = st.reshape(-1, st.shape[-1])
    room = DUMP_BYTES - sum(a.nbytes for a in small.values())
    if st.nbytes <= room:
        arrays["score_tokens"] = st
    else:
        k = (room - 1024) // (rows.shape[1] * 4 + 8)  # keep the index array inside the budget too
        idx = np.sort(np.random.default_rng(0).choice(rows.shape[0], size=k, replace=False))
        arrays["score_tokens"] = rows[idx]
        arrays["score_tokens_rows"] = idx.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def emit(out):
    full = os.environ.get("SOLA_BENCH_FULL") or os.path.join(ROOT, "gpurun_out", "bench_full.json")
    try:
        os.makedirs(os.path.dirname(full), exist_ok=True)
        with open(full, "w") as f:
            json.dump(out, f, indent=1)
    except OSError:
        pass
    line = compact(out)
    # the driver keeps a bounded tail of stdout: stay under 6 KB by dropping, in this order, what the verbose file keeps anyway
    for path in _OPTIONAL:
        if len(json.dumps(line, separators=(",", ":"))) <= 6000:
            break
        node = line
        for key in path[:-1]:
            node = node.get(key, {}) if isinstance(node, dict) else {}
        if isinstance(node, dict):
            node.pop(path[-1], None)
    print(json.dumps(line, separators=(",", ":")), flush=True)


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend_name = None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist

        # SOLA_BENCH_BACKEND=gloo lets several ranks share one GPU (functional check of this code path on a 1-GPU box;
        # RCCL refuses two ranks on one device).  The driver's runs use the default: nccl (= RCCL), one rank per GPU.
        backend = os.environ.get("SOLA_BENCH_BACKEND", "nccl")
        dev_index = local_rank % max(1, torch.cuda.device_count()) if backend != "nccl" else local_rank
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
        backend_name = dist.get_backend()
        assert dist.get_world_size() == world
    else:
        dev_index = 0
        torch.cuda.set_device(0)
    dev = torch.device("cuda", dev_index)

    from sola_amd import _lib, ops, synth
    from sola_amd.loss import track_selection_losses
    from sola_amd.module import LanguageAlignedTrackSelectionModule, collate_ragged  # noqa: F401

    for kv in args.tune:  # A/B measurements only; the line says so (config.tune)
        key, val = kv.split("=")
        _lib.check(_lib.lib().sola_tune(key.encode(), int(val)), f"sola_tune {kv}")
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = args.batch, args.tracks, args.frames, args.text_len
    sd = synth.make_state_dict(cfg, 42)
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).eval()
    m.ws_policy = "cached" if args.cached_ws else "always"
    m.precision = args.precision
    inp = synth.make_inputs(cfg, B, N, T, L, seed=1000 + rank)  # every rank owns different samples
    obj = torch.from_numpy(inp["object_tokens"]).to(dev)
    lang = torch.from_numpy(inp["lang_tokens"]).to(dev)
    labels = torch.from_numpy(inp["labels"]).to(dev)
    pos = torch.from_numpy(inp["pos_tokens"]).to(dev)

    def step():
        with torch.no_grad():
            sm, st = m(obj, lang)
            loss3 = track_selection_losses(sm, st, labels, pos, m.negative_token.weight, POS_W, TEMP, ALIGN_W)
            prob, pred = ops.select(sm, 0.5)
        return sm, st, loss3, prob, pred

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    # The interpreter's cyclic garbage collector is parked for the timed region (as timeit does): with torch imported a full
    # collection takes ~37 ms on the host, the GPU queue runs dry behind it, and where it lands is a matter of luck
    # (tools/gc_stall_probe.py: it was one 35-39 ms stall in the first timed step, +2-4 ms/step at the default 10-20 steps).
    gc.collect()
    gc.disable()
    for _ in range(args.warmup):
        step()
    barrier()
    # live kernel timing in the timed region: the launches the two rooflines are computed from (GEMMs, attention core).  Every timed
    # launch costs two event records on the stream (2.8 % of the step with all ~120 launches bracketed, tools/prof_overhead.py); the
    # complete per-category breakdown (kernel_ms_per_step, --full) comes from an UNTIMED pass of the same steps behind the timed region.
    roof_cats = ["gemm128", "gemm64", "gemm_split", "gemm_split256", "gemm_split256_gn", "attn"]
    _lib.profile_enable(True, categories=roof_cats)
    _lib.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        outs = step()
    barrier()
    elapsed = time.perf_counter() - t0
    prof = _lib.profile_read(reset=True)
    loss3 = outs[2]
    if args.dump_outputs and rank == 0:  # what the last timed step returned, written before anything else runs on the device
        dump_outputs(args.dump_outputs, outs)
    prof_all = None
    if args.full:
        _lib.profile_enable(True)
        for _ in range(args.steps):
            step()
        barrier()
        prof_all = _lib.profile_read(reset=True)
    gc.enable()
    _lib.profile_enable(False)
    assert torch.isfinite(loss3).all()
    fallbacks, guard_bits = m.split_fallbacks()

    dist_parity = None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if world > 1 and args.full:
        # parity at N > 1 (round 6): every rank that owns a batch the reference's logits are committed for (seeds 1000-1002 = ranks 0-2 at the
        # default batch) checks every row of ITS batch; the worst error over those ranks goes into the line (a 64 KB fixture, no CPU work)
        rg = reference_logits(f"u256.{1000 + rank}") if (B, N, T, L) == (256, 64, 32, 16) else None
        e = torch.tensor([-1.0, 0.0], device=dev, dtype=torch.float64)
        if rg is not None:
            with torch.no_grad():
                ur = uniform_row_errors(m(obj, lang)[0].cpu().numpy(), rg)
            e = torch.tensor([ur["max_abs_logit_err_vs_reference"] if ur["selections_equal"] else 1e9, 1.0], device=dev, dtype=torch.float64)
        emax, ecnt = e[:1].clone(), e[1:].clone()
        torch.distributed.all_reduce(emax, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(ecnt, op=torch.distributed.ReduceOp.SUM)
        dist_parity = {"max_abs_logit_err_vs_reference": float(emax.item()), "ranks_checked": int(ecnt.item())} if ecnt.item() > 0 else None
    total_samples = B * args.steps * world
    value = total_samples / elapsed
    sync = lambda: torch.cuda.synchronize(dev)

    # transparency leg (after the timed region, N=1 only): the same workload on the exact-f32 MFMA path with its own
    # roofline entries, and the largest difference between the two modes' logits on this batch
    exact = None
    parity = None
    parity_ref = None
    if args.full and args.precision == "f16x3" and world == 1:
        with torch.no_grad():
            sm_split, _ = m(obj, lang)
        m.precision = "f32"
        k = max(3, args.steps // 4)
        dt32, prof32 = profiled(step, k, sync)
        with torch.no_grad():
            sm_f32, _ = m(obj, lang)
        # parity of the benched batch itself: EVERY row of this rank-0 batch against the fp32 PyTorch-CPU oracle, both modes
        # (~8 s of host time at 256 samples; skipped with --cpu-seconds 0)
        err = None
        if args.cpu_seconds > 0 and B * N * T <= 256 * 64 * 32:
            from oracle import sola_oracle  # checker only

            torch.set_num_threads(min(32, os.cpu_count() or 1))
            tsd = sola_oracle.to_torch_state(sd)
            ref = np.concatenate([sola_oracle.forward(tsd, cfg, inp["object_tokens"][b:b + 16], inp["lang_tokens"][b:b + 16])[0].numpy()
                                  for b in range(0, B, 16)])
            err = {}
            for tag, got in (("f16x3", sm_split), ("f32", sm_f32)):
                e_rows = np.abs(got.cpu().numpy() - ref).max(axis=1)
                err[tag] = {"max_abs_logit_err_vs_oracle": float(e_rows.max()), "mean_row_max_err": float(e_rows.mean()),
                            "rows_above_5e-4": int((e_rows > 5e-4).sum()), "rows": int(B),
                            "selections_equal": bool(np.array_equal(got.cpu().numpy() > 0, ref > 0))}
        ref_gold = reference_logits(f"u256.{1000 + rank}") if (B, N, T, L) == (256, 64, 32, 16) else None
        err_ref = None
        if ref_gold is not None:  # every row against the REFERENCE's own logits (round 6); no CPU work: a 64 KB fixture
            err_ref = {tag: uniform_row_errors(got.cpu().numpy(), ref_gold) for tag, got in (("f16x3", sm_split), ("f32", sm_f32))}
            x64 = reference_logits("u256.1000.oracle_f64") if rank == 0 else None
            if x64 is not None:  # distance from exact arithmetic (float64 evaluation), next to the reference's own
                for tag, got in (("f16x3", sm_split), ("f32", sm_f32)):
                    err_ref[tag]["max_abs_logit_err_vs_float64"] = float(np.abs(got.cpu().numpy() - x64.reshape(B, N)).max())
                    err_ref[tag]["reference_vs_float64"] = float(np.abs(ref_gold.astype(np.float64) - x64).max())
        exact = {"value": round(B / dt32, 2), "unit": "samples/s", "ms_per_step": round(1e3 * dt32, 4), "steps": k, "dtype": "f32",
                 "roofline": gemm_roofline(prof32, "f32", dt32, k), "roofline_attention": attn_roofline(prof32),
                 "kernel_ms_per_step": kernel_ms(prof32, k),
                 "max_abs_logit_diff_vs_split_mode": float((sm_f32 - sm_split).abs().max()),
                 **({"max_abs_logit_err_vs_oracle": err["f32"]} if err else {}),
                 **({"max_abs_logit_err_vs_reference": err_ref["f32"]} if err_ref else {})}
        parity = err["f16x3"] if err else None
        parity_ref = err_ref["f16x3"] if err_ref else None
        m.precision = args.precision

    dist_res = None
    if args.full and world > 1 and args.train_steps > 0:  # every rank takes part (collectives); reported by rank 0
        try:  # a (symmetric) failure of this extra leg must not cost the headline line
            dist_res = dist_legs(cfg, sd, dev, world, rank, max(2, min(args.train_steps, 5)))
        except Exception as e:  # noqa: BLE001
            dist_res = {"error": f"{type(e).__name__}: {e}"[:500]}
            torch.cuda.synchronize(dev)
    if rank == 0:
        fl = synth.flops_per_sample(cfg, N, T, L)
        step_s = elapsed / args.steps
        roofline = gemm_roofline(prof, args.precision, step_s, args.steps)
        roofline_attn = attn_roofline(prof)
        # HBM traffic cannot be read from inside the run (PMC needs rocprofv3); it is the committed per-launch PMC
        # measurement of this same command line (tools/profile_bench.sh -> profiles/r0X_traffic.json), used only when the
        # batch matches the profiled one, else null
        for tname in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", tname)
            if not os.path.exists(tpath):
                continue
            tr = json.load(open(tpath))
            if tr.get("batch") == B and (N, T, L) == (64, 32, 16):
                kk = tr["kernels"]
                f32k = next((k for k in kk if k.startswith("gemm_nt_f32_persist_kernel<false, 0")), None) or \
                    next((k for k in kk if k.startswith("gemm_nt_f32_kernel<128, 128, 0, 0")), None)  # (profiles before round 5: the one-tile kernel)
                gk = tr.get("dominant_gemm") if args.precision == "f16x3" else f32k
                if roofline and gk in kk:
                    roofline["traffic_kernel"] = gk
                    roofline["traffic"] = kk[gk]["hbm_bytes_per_launch"]
                    roofline["traffic_source"] = tr["source"]
                ak = [(kk[k]["hbm_bytes_per_launch"], kk[k]["calls"]) for k in kk if k.startswith("attn_fwd")]
                if roofline_attn and ak:  # launch-weighted mean over the attention kernels of the profiled run
                    roofline_attn["traffic"] = int(sum(b * c for b, c in ak) / sum(c for _, c in ak))
                if exact and exact.get("roofline") and f32k:
                    exact["roofline"]["traffic"] = kk[f32k]["hbm_bytes_per_launch"]
            break
        out = {
            "metric": "track-selection forward+loss samples/sec at (T=32,N=64,d=256)",
            "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * step_s, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "data": "synthetic",
            "dtype": "f32" if args.precision == "f32" or B * N * T <= 4096 and not any(t.startswith("infer_f32_rows") for t in args.tune)
                     else "f32 via split-f16 (hi+lo f16 operand pairs, 3 f16 MFMAs per product, f32 accumulate)",
            "config": {"workload": f"SOLA track selection forward+BCE+alignment loss+selection, T={T} N={N} d=256 L={L}, mevis/default model "
                                   f"(32.98M params, random init), {B} samples/step/GPU, "
                                   + ("conv weights standardised once" if args.cached_ws else "conv weights re-standardised every step"),
                       "batch_per_gpu": B, "tracks": N, "frames": T, "text_len": L, "sharding": f"per-sample x{world}",
                       "collective_backend": backend_name, "world_size_reported_by_backend": world if world > 1 else None,
                       **({"tune": args.tune} if args.tune else {})},
            "gflop_per_sample": round(fl["total"] / 1e9, 3),
            "model_tflops": round(value * fl["total"] / 1e12, 2),
            "roofline": roofline, "roofline_attention": roofline_attn,
        }
        if prof_all is not None:
            out["kernel_ms_per_step"] = kernel_ms(prof_all, args.steps)
            out["kernel_ms_per_step_source"] = ("untimed pass of the same steps with every launch bracketed by events; the timed region brackets "
                                                "the GEMM and attention launches only")
        if args.precision == "f16x3":
            out["split_guard"] = {"enabled": bool(m.split_guard), "calls_repeated_in_f32": fallbacks, "guard_bits_last_call": guard_bits}
        if parity is not None:  # every row of the timed batch against the fp32 oracle (the headline mode; exact_f32_mode carries its own)
            out["max_abs_logit_err_vs_oracle"] = parity
        if parity_ref is not None:  # ... and against the reference's own logits for this batch (tests/golden/bench_golden.npz)
            out["max_abs_logit_err_vs_reference"] = parity_ref
        if world > 1 and dist_parity is not None:
            out["max_abs_logit_err_vs_reference"] = dist_parity
        if exact is not None:
            out["exact_f32_mode"] = exact
        if args.full and world == 1 and args.extra_legs:
            k = max(3, args.steps // 4)
            out["stress_T128_N128"] = stress_leg(cfg, m, dev, args.precision, k)
            tsd_par = None
            if args.cpu_seconds > 0:
                from oracle import sola_oracle  # checker only

                tsd_par = sola_oracle.to_torch_state(sd)
            out["ragged"] = ragged_leg(cfg, m, dev, k, out["model_tflops"], tsd_par)
            out["iou"] = iou_leg(dev, args.cpu_seconds)
            out["f16_storage_mode"] = f16_storage_leg(cfg, m, dev, k)
            out["call_pattern"] = call_pattern_leg(cfg, sd, dev, k)
        if dist_res is not None:
            out["training_step_dist"] = dist_res
        if args.full and world == 1 and args.train_steps > 0:
            tsd_par = None
            if args.cpu_seconds > 0:
                from oracle import sola_oracle  # checker only

                tsd_par = sola_oracle.to_torch_state(sd)
            out["training_step"] = training_leg(cfg, sd, dev, min(B, 64), N, T, L, args.train_steps, tsd_par)
        if args.full and world == 1 and args.cpu_seconds > 0:
            out["cpu_baseline"] = cpu_baseline(cfg, sd, N, T, L, args.cpu_seconds)
        emit(out)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
