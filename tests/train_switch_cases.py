"""The sola_tune switches of the TRAINING step (sola_forward_train* / sola_backward* / sola_loss_backward* / sola_train_step), as a plain table:
which keys of sola_amd/csrc/tune.h a training step can read, the non-default settings worth running, the precision modes a setting can
reach, and what docs/tune_keys.md and the comment at the global's definition promise about it.  Every other non-EXPERIMENTS key is listed
with the file that reads it and why a training step never gets there.  Shared by test_train_switch_cpu.py (the table covers tune.h exactly;
every `bits` promise quotes docs/tune_keys.md) and test_gpu_train_switches.py (every setting, alone, across a forward / backward pair and in
the coupled pairs, against the float64 oracle and the reference's golden gradients).

promise   "bits"      documented bit-identical to the default setting: the GPU test adds torch.equal on the loss and all 83 gradients
          "order"     the same products in another f32 summation order, or another kernel for the same shape
          "rounding"  moves a 16-bit rounding point (or, for the step's size gate, leaves the 16-bit arithmetic altogether)
          A dict {mode: promise} where the modes differ; "cite" is the sentence of docs/tune_keys.md behind a "bits".
modes     the precision modes in which some launch of the step reads the key.  The exact-f32 GEMM / weight-gradient / attention / GroupNorm
          keys are listed for all four: the 16-bit steps keep exact-f32 launches for shapes their kernels do not take (a K that
          is no multiple of 32 / 64) and every mode shares the f32 attention and norm kernels.
bf16      what the site flags (sola_train_site_flags) must show under "bf16" with this setting on the uniform shape of the GPU test, where
          the setting changes them BY DESIGN: qkv16 "all" / "none" / "motion" (only the motion site, whose units of <= 4 steps take the
          attention backward's register kernel) / "o2l" (only the object -> language site), o16 / prenorm16 likewise where the setting
          switches that storage off.  Unlisted = as the default (qkv16 at all six sites; o16 and prenorm16 are printed, not asserted).
          {value: {...}} where the key's settings differ (bf16_expect).
under     other switches that are on while the key's settings run, because the kernels the key is about are not reached at test sizes
          without them: "gemm_glds_force" 1 (the direct-to-LDS GEMMs for grids of any size), "attn_bwd_fused" 0 (the two-pass attention
          backward) and "bwd_group_rows" 0 (the per-matrix weight-gradient launches the side lane takes).  A `bits` promise is then held against the run under those switches alone."""

ALL = ("f32", "f16x3", "f16", "bf16")
LOWP = ("f16x3", "f16", "bf16")
P16 = ("f16", "bf16")
MODES = ALL


def _k(values, modes, promise, cite=None, bf16=None, note="", under=None):
    return {"values": tuple(values), "modes": tuple(modes), "promise": promise, "cite": cite, "bf16": bf16 or {}, "note": note, "under": under or {}}


_OFF = {"qkv16": "none", "o16": "none"}

TRAINING = {
    # ---- gemm.hip / gemm_f32p.hip / gemm_glds.hip: the forward's and the input gradients' GEMMs
    "gemm_variant": _k((0, 1), ALL, "order", note="gemm.hip launch_gemm: the exact-f32 tile kernels' staging schedule"),
    "gemm_glds": _k((0, 1, 4), LOWP, "order", under={"gemm_glds_force": 1}, note="gemm.hip launch_gemm -> gemm_glds.hip: staging / block shape of the 16-bit and split GEMMs"),
    "gemm_persist": _k((0,), LOWP, "order", under={"gemm_glds_force": 1}, note="gemm_glds.hip: 256x256 shape, one tile per block"),
    "gemm_glds_force": _k((1,), LOWP, "order", note="gemm.hip: the direct-to-LDS kernels for the small grids of the test shapes too"),
    "gemm_splitk": _k((0, 8), ALL, "order", note="gemm.hip: split-K of small grids off / from 8 tiles on"),
    "gemm_splitk_max": _k((2, 16), ALL, "order", note="gemm.hip: K ranges per tile of that split"),
    "gemm_small_rows": _k((0,), ALL, "order", note="gemm.hip: the few-row exact-f32 shape off (64 x 64 + split-K pair)"),
    "gemm_small_nw8": _k((0,), ALL, "order", note="gemm.hip: four waves per tile of the few-row shape"),
    "gemm_f32_nw8": _k((0,), ALL, "bits", cite="bit-identical outputs, bias gradients in another fixed summation order",
                       note="gemm.hip: exact-f32 128 x 128 shape with four waves (the bias-gradient clause is gemm_tn_nw8's)"),
    "gemm_f32_persist": _k((0,), ALL, "bits", cite="A/B, bit-identical: `tests/test_gpu_kernels.py`", note="gemm_f32p.hip"),
    "gemm_slack_stagger": _k((0,), ("bf16",), "bits", cite="results bit-identical", under={"gemm_glds_force": 1}, note="gemm_glds.hip: bf16 persistent launches only"),
    "train_split_min_rows": _k((1 << 30,), LOWP, "rounding", bf16={"qkv16": "none", "o16": "none", "prenorm16": "none"},
                               note="forward.hip / backward.hip size gate: above the batch, every mode runs the exact-f32 step - by design "
                                    "no 16-bit storage at all (the GPU test's fixture holds the gate at 0 otherwise)"),
    # ---- gemm_tn*.hip: weight gradients
    "gemm_tn_nw8": _k((0,), ALL, "order", note="gemm_tn.hip: dW bit-identical, bias gradients in another fixed order"),
    "gemm_tn_persist": _k((0,), ALL, "order", note="gemm_tn_f32p.hip"),
    "train_tn_tr": _k((0,), LOWP, {"f16x3": "order", "f16": "order", "bf16": "rounding"}, bf16=_OFF,
                      note="gemm_tn_tr.hip; site16 (forward.hip) keeps q / k / v as bf16 rows only while the dW products take this route: 0 "
                           "turns the bf16 q / k / v storage off by design"),
    "train_dw_f16": _k((0,), ("f16x3",), "rounding", note="backward.hip: split pairs in the weight gradients of the split-f16 step"),
    # ---- backward.hip orchestration
    "bwd_side_rows": _k((1 << 20,), ("f32",), "bits", cite="all off by default, results bit-identical", under={"bwd_group_rows": 0},
                        note="backward.hip lane_on (exact f32 only): the per-matrix weight-gradient launches on a side stream.  At the few-row "
                             "test shapes the default is the grouped launch (bwd_group_rows), which the side lane replaces, so the promise is "
                             "held against the per-matrix launches it was made for"),
    "bwd_group_rows": _k((0,), ("f32",), "order", note="backward.hip: per-matrix weight-gradient launches"),
    "bwd_dual_cast": _k((0,), LOWP, {"f16x3": "order", "f16": "order", "bf16": "rounding"}, bf16=_OFF,
                        note="backward.hip grad_w_many / stats; 0 leaves no row-major 16-bit operand behind, so site16 keeps f32 q / k / v "
                             "and gradients (off by design)"),
    "bwd_fused_bf16_cast": _k((0,), ("bf16",), "rounding",
                              note="backward.hip stats / gn16: with the storage on, the norms' bf16 dx rows and the bias sums over rounded rows go"),
    # ---- forward.hip orchestration
    "train_x16_keep": _k((0,), LOWP, {"f16x3": "bits", "f16": "bits", "bf16": "rounding"},
                         cite="the same 16-bit values either way, so the gradients of the f16x3 and f16 steps are bit-identical with 0",
                         bf16={"o16": "none", "prenorm16": "none"},
                         note="forward.hip keep16 / resid16 / attention(): the bf16 step's bfloat16 pre-norm rows and bf16-only attention "
                              "outputs live in the kept-operand arena and go with it (off by design)"),
    "train_attn_cast": _k((0, 2), LOWP, {"f16x3": "bits", "f16": "bits", "bf16": "rounding"}, cite="bit-identical to the separate cast launch",
                          bf16={0: {"o16": "none"}, 2: {}},
                          note="forward.hip attention(): 2 = the split-f16 step too (the default in the 16-bit steps); 0 in the bf16 step: no "
                               "kernel-written bf16 output rows, so o16 is off by design and D = dO . O reads the f32 rows"),
    "train_gn_cast": _k((0,), P16, "order", note="forward.hip gn_fmt: separate cast launches behind the norms"),
    "train_bf16_store": _k((0, 1, 2), ("bf16",), "rounding", note="forward.hip / backward.hip / gemm_tn_split.hip: the storage levels below the shipped 3"),
    "train_gn_stats": _k((0,), ALL, "order", note="forward.hip gn(): the object -> language norm's backward recomputes (mean, rstd)"),
    # ---- attention forward (attn.hip launch_attention and the kernels it routes to; log-sum-exp kept, dropout off in the tests)
    "attn_variant": _k((0, 2), ALL, "order", note="attn.hip"),
    "attn_target_blocks": _k((64, 4096), ALL, "order", note="attn.hip resident-K/V loop"),
    "attn_reg": _k((0, 2), ALL, "order", note="attn_reg.hip: writes the log-sum-exp, so a training forward without dropout takes it"),
    "attn_res": _k((0, 2), ALL, "order", note="attn_res.hip: as attn_reg"),
    "attn_res_tiles": _k((1, 2), ALL, "order", note="attn_res.hip"),
    "attn_res_shape": _k((1, 2), ALL, "order", note="attn_res.hip"),
    "attn_simple_train": _k((0,), ALL, "order", note="attn_simple.hip"),
    "attn_simple_db": _k((0,), ALL, "order", note="attn_simple.hip"),
    "attn_simple_remap": _k((1,), ALL, "bits", cite='"attn_simple_remap" 1 bit-identical to 0 there', note="attn_simple.hip: block order only"),
    "attn_f16_qpb": _k((1, 2), ("bf16",), "order", note="attn_f16.hip launch_h<.., TRAIN>: the bf16-MFMA training forward against <= 64 keys reads it too"),
    "attn_bf16_mfma": _k((0,), ("bf16",), "rounding", bf16={"qkv16": "o2l", "o16": "none"},
                         note="attn_f16.hip: 0 = f32 products on the widened rows (attn_simple.hip's training instantiation, which takes units of "
                              "more than 16 queries or keys only: at the uniform test shape - 8 tracks, 4 steps - that is the object -> language "
                              "site alone, by design); only the bf16-MFMA kernel writes bf16-only outputs (o16 off by design)"),
    # ---- attention backward (attn_bwd.hip)
    "attn_bwd_bf16_mfma": _k((0,), ("bf16",), "rounding", bf16={"o16": "none"},
                             note="attn_bwd.hip: 0 = f32 products; a bf16 dO / O needs the bf16 products (o16 off by design)"),
    "attn_bwd_small": _k((0,), ALL, "order", note="attn_bwd.hip: no register kernel for units of <= 4 steps"),
    "attn_bwd_blk": _k((0,), ALL, "bits", cite="block-shared double-buffered staging (bit-identical to 0: tests/test_gpu_attn_bwd.py)", under={"attn_bwd_fused": 0},
                       note="attn_bwd.hip two-pass kernels"),
    "attn_bwd_rag_wave": _k((0, 1024), ALL, "order", under={"attn_bwd_fused": 0}, note="attn_bwd.hip: ragged batches only"),
    "attn_bwd_fused": _k((0,), ALL, {"f32": "order", "f16x3": "order", "f16": "order", "bf16": "rounding"}, bf16={"qkv16": "motion", "o16": "motion"},
                         note="attn_bwd.hip: two-pass kernels; only the one-pass and the register kernel take bf16 rows, so with 0 the "
                              "inter-object and object -> language sites keep f32 q / k / v by design (the motion site's <= 4 steps stay, "
                              "with their bf16-only attention output)"),
    # ---- GroupNorm (norm.hip forward, bwd.hip backward)
    "gn_variant": _k((0,), ALL, "order", note="norm.hip"),
    "gn_wide": _k((0,), ALL, "order", note="norm.hip"),
    "gn_slices": _k((0,), ALL, "order", note="norm.hip"),
    "gn_bwd_reg": _k((0,), ALL, "order", note="bwd.hip"),
}

NOT_TRAINING = {
    "attn_stage_split_math": "api.hip: set on the descriptor of the per-stage entry point sola_attention only (tests of the split arithmetic)",
    "attn_splitm": "attn.hip / attn_simple.hip: needs AttnDesc::split_math and no log-sum-exp - the inference forward and the stage entry point",
    "attn_spin": "attn_simple.hip attention_spin_supported: split-f16 q / k / v and no log-sum-exp - the inference forward; training q / k / v are f32 or bf16 rows",
    "attn_split_min_keys": "forward_infer.hip: which units of the split-f16 INFERENCE forward take split q / k / v",
    "attn_f16_small": "attn_f16.hip launch_h<.., TRAIN = false>: the plain-f16 inference forward's streaming shape",
    "lang_shared_neg": "forward_infer.hip: the negative tokens' text-side projections of the split-f16 inference forward",
    "infer_f32_rows": "api.hip few_rows_f32: sola_forward / sola_forward_ragged only",
    "gn_h8": "norm.hip: needs 16-bit input AND output rows (GroupNormDesc::out F16), which only the plain-f16 inference forward sets",
    "bilinear_staged": "masklet.hip: mask resampling",
    "iou_fused": "iou.hip: sola_mask_iou_matrix",
    "iou_shape": "iou.hip: block shape of the one-launch IoU kernel",
    "iou_packed": "iou.hip: reduction word of the one-launch IoU kernel",
    "pack_resample_lds": "iou.hip: nearest-resampling mask pack",
}

# ---- a switch that changes between the forward and its backward (bf16 and f16).  `other` is the setting of the side that leaves the default.
# Each entry runs both orders: forward under defaults / backward under other, and forward under other / backward under defaults.  The outcome
# is gradients within the mode's bar or a SolaError that names the change; `applies` says where the key can matter at all.
ACROSS = {
    "bwd_dual_cast": {"other": 0, "applies": "bf16: the forward's bf16 q / k / v rows need the backward's row-major operand route; f16: the backward reads it alone"},
    "bwd_fused_bf16_cast": {"other": 0, "applies": "bf16: read by the backward alone (f32 rows of those gradients always exist); f16: not read"},
    "train_tn_tr": {"other": 0, "applies": "bf16: site16 and the bf16-only attention outputs need the row-major dW kernel; f16: the backward reads it alone"},
    "attn_bwd_fused": {"other": 0, "applies": "bf16: site16 asked the one-pass kernel; f16: the backward reads it alone"},
    "train_bf16_store": {"other": 0, "applies": "bf16: forward (what is kept) and backward (what is written 16-bit); f16: not read"},
    "train_x16_keep": {"other": 0, "applies": "both: read by the forward alone; the backward goes by the arena's records"},
    "attn_bwd_bf16_mfma": {"other": 0, "applies": "bf16: the forward's bf16-only attention outputs need the backward's bf16 products; f16: not read"},
    "train_attn_cast": {"other": 0, "applies": "both: read by the forward alone"},
    "train_gn_stats": {"other": 0, "applies": "both: the forward records per layer whether it wrote the statistics; the backward goes by the record"},
}
ACROSS_MODES = ("bf16", "f16")

# ---- pairs whose globals stand in one condition of forward.hip / backward.hip, under bf16: (key, value) x (key, value), every combination of
# the listed non-default values
PAIRS = (
    (("bwd_dual_cast", (0,)), ("bwd_fused_bf16_cast", (0,))),      # backward.hip: gn16, stats()
    (("train_tn_tr", (0,)), ("train_bf16_store", (0, 1, 2))),      # forward.hip site16
    (("train_x16_keep", (0,)), ("train_bf16_store", (0, 1, 2))),   # forward.hip resid16 (0: kept operand casts off with f32 storage)
    (("attn_bwd_fused", (0,)), ("train_bf16_store", (0, 1, 2))),   # forward.hip site16 / backward.hip out_proj_bwd
    (("attn_bf16_mfma", (0,)), ("train_attn_cast", (0,))),         # forward.hip attention()
)


def settings():
    """(mode, key, value) of Test A, in table order"""
    return [(m, k, v) for k, e in TRAINING.items() for v in e["values"] for m in e["modes"]]


def promise(key, mode):
    p = TRAINING[key]["promise"]
    return p[mode] if isinstance(p, dict) else p


def bf16_expect(key, value):
    e = TRAINING[key]["bf16"]
    return dict(e[value]) if e and all(isinstance(k, int) for k in e) else dict(e)


def pair_settings():
    return [((ka, va), (kb, vb)) for (ka, vas), (kb, vbs) in PAIRS for va in vas for vb in vbs]


def parse_tune_keys(tune_h_text):
    """the P(...) / S(...) rows of SOLA_TUNE_KEYS (not the EXPERIMENTS list) of sola_amd/csrc/tune.h"""
    import re
    body = tune_h_text.split("#define SOLA_TUNE_KEYS(P, S)", 1)[1].split("#define SOLA_TUNE_EXPERIMENT_KEYS", 1)[0]
    return re.findall(r"^\s*[PS]\((\w+)", body, flags=re.M)
