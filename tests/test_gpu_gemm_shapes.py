"""The 16-bit-operand (PURE) instantiations of the three direct-to-LDS GEMM kernels - one tile per block at 128x128 and at 256x256, and the
persistent 256x256 kernel - which the split-operand bit-identity tests of tests/test_gpu_fast.py do not reach: f16 and bf16 operands through
sola_gemm_nt_f16 / sola_gemm_nt_bf16 on ragged M and N (clamped DMA rows, the predicated epilogue) with 1 to 3 k-tiles of 64, and the whole
16-bit-storage forward (the conv instantiations) across the same three settings.  The kernels accumulate every output element in the same
order and agree bit for bit - with ONE exception, found by this file and recorded here as a finding, not fixed: an f16 output WITHOUT a
residual.  The persistent kernel's straight-line epilogue compiles `(_Float16)(t * osc + bias)` to v_fma_mixlo_f16, one rounding of the exact
sum; the one-tile kernels, whose output format is a run-time flag, round to f32 and then convert.  They differ on ties (the last f16 bit), so a
precision-2 forward - its convs and q/k/v projections use that epilogue - gives other bits by whether its grid is routed to the persistent
kernel or to a one-tile kernel (max |d logit| 4.278e-02 on the batch below; the mode's stated bound is 0.8).  For that epilogue and for the
forward the two one-tile kernels are held to each other bit for bit and all three to float64 within tests/test_gpu_f16.py's bounds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sola_oracle  # noqa: E402
from sola_amd import synth  # noqa: E402
from sola_amd._lib import check, current_stream, lib, ptr, tuned  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

SETTINGS = [dict(gemm_glds=1, gemm_persist=0), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=4, gemm_persist=1)]
SHAPES = [(300, 72, 128), (777, 264, 64), (520, 256, 192)]


def _gemm(kind, a, w, bias, r, r16, out, M, N, K):
    s = current_stream(out.device)
    c16 = 0 if out.dtype == torch.float32 else 1
    if kind == "f16":  # (a residual of this entry point is f16, whatever the output)
        check(lib().sola_gemm_nt_f16(ptr(a), K, ptr(w), ptr(bias), ptr(r), N, ptr(out), N, c16, M, N, K, 1.0, s), "sola_gemm_nt_f16")
    else:
        check(lib().sola_gemm_nt_bf16(ptr(a), K, ptr(w), ptr(bias), ptr(r), N, 1 if r16 else 0, ptr(out), N, c16, M, N, K, s), "sola_gemm_nt_bf16")


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_16bit_gemm_block_shapes_bit_identical(M, N, K, kind):
    """No residual into f32, a residual into f32 (f32 for bf16 operands; the f16 entry point takes its residual as f16), a 16-bit residual
    into a 16-bit output, and no residual into a 16-bit output: the three settings give the same bits, except f16 without a residual into f16
    (module docstring), where the one-tile pair agrees bit for bit and every output is held to float64 on the rounded operands within
    tests/test_gpu_f16.py's bound for an f16 output (2e-3 of the largest entry).  The f32-output variant with a residual is held to float64
    too, within that file's bound for it (2e-5 of the largest entry: only the f32 accumulation differs), under every setting.
    Which kernel the third setting (gemm_glds 4, gemm_persist 1) reaches: the PERSISTENT kernel needs two k-tiles of 64 and a residual in the
    output's format, so (777, 264, 64) and the f16 "res_f32" case (f16 residual, f32 output) run the one-tile 256x256 kernel a second time
    there; every other case of (300, 72, 128) and (520, 256, 192) runs the persistent kernel."""
    dt = torch.float16 if kind == "f16" else torch.bfloat16
    rng = np.random.default_rng(M * 7 + N)
    a = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda().to(dt).contiguous()
    w = torch.from_numpy((rng.uniform(-1, 1, size=(N, K)) / 32).astype(np.float32)).cuda().to(dt).contiguous()
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    r32 = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    r16 = r32.to(dt).contiguous()
    r_into_f32 = r16 if kind == "f16" else r32
    prod = a.cpu().double().numpy() @ w.cpu().double().numpy().T + bias.cpu().double().numpy()
    cases = [("none_f32", None, False, torch.float32), ("res_f32", r_into_f32, kind == "f16", torch.float32), ("res16_out16", r16, True, dt),
             ("none_out16", None, False, dt)]  # (the last: the convs' and the q/k/v projections' epilogue in the 16-bit storage mode)
    for name, r, r_is16, odt in cases:
        outs = []
        for st in SETTINGS:
            out = torch.empty((M, N), device="cuda", dtype=odt)
            with tuned(**st):
                _gemm(kind, a, w, bias, r, r_is16, out, M, N, K)
            outs.append(out)
        torch.cuda.synchronize()
        bits = [o.view(torch.int32 if odt == torch.float32 else torch.int16) for o in outs]
        assert torch.equal(bits[0], bits[1]), (kind, name, "128x128 vs one-tile 256x256")
        one_rounding_vs_two = kind == "f16" and name == "none_out16"
        if not one_rounding_vs_two:
            assert torch.equal(bits[0], bits[2]), (kind, name, "128x128 vs the third setting")
        if one_rounding_vs_two or name == "res_f32":
            ref = prod + (r.cpu().double().numpy() if r is not None else 0.0)
            bound = (2e-3 if odt != torch.float32 else 2e-5) * np.abs(ref).max()
            for st, o in zip(SETTINGS, outs):
                err = np.abs(o.cpu().double().numpy() - ref).max()
                print(f"{kind} {M}x{N}x{K} {name} {st}: |err| {err:.3e} of bound {bound:.3e}")
                assert err <= bound, (kind, name, st, err)


def test_f16_storage_forward_across_gemm_kernels():
    """The whole 16-bit-storage forward (module.precision "f16", library precision 2: implicit-im2col conv launches, three-problem q/k/v
    launches, f16 residual and f16 output epilogues on plain f16 operands) through the persistent kernel, the one-tile 256x256 kernel and
    the 128x128 kernel, on the model and the tiny batch of tests/test_gpu_fast.py::test_forward_identical_across_gemm_kernels.  Its convs and
    projections store f16 without a residual (module docstring): the two one-tile kernels give the same bits, the persistent kernel's logits
    are 4.278e-02 from theirs, and each of the three is held to the float64 oracle within the mode's hard bounds of tests/test_gpu_f16.py
    (0.8 on any logit, 0.9 on any token entry)."""
    from test_gpu_f16 import TOL_LOGIT, TOL_TOKEN
    cfg = synth.DEFAULT_MODEL_CFG
    sd = synth.make_state_dict(cfg, 42)
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.precision = "f16"
    inp = synth.make_inputs(cfg, 8, 40, 32, 12, 5)
    obj, lang = torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda()
    outs = []
    names = ["persistent", "one-tile 256x256", "128x128"]
    for st in [dict(gemm_glds=4, gemm_persist=1), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=1, gemm_persist=0)]:
        with tuned(**st), torch.no_grad():
            sm, tok = m(obj, lang)
        outs.append((sm.cpu(), tok.cpu()))
    print("f16 forward, max |d logit| persistent vs one-tile 256x256:", float((outs[0][0] - outs[1][0]).abs().max()))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])
    rsm, rst = sola_oracle.forward(sd, cfg, inp["object_tokens"], inp["lang_tokens"], dtype=torch.float64)
    for name, (sm, tok) in zip(names, outs):
        e_sm, e_st = float((sm.double() - rsm).abs().max()), float((tok.double() - rst).abs().max())
        print(f"f16 forward, {name}: |logit err| {e_sm:.3e} of {TOL_LOGIT}, |token err| {e_st:.3e} of {TOL_TOKEN}")
        assert e_sm <= TOL_LOGIT and e_st <= TOL_TOKEN, (name, e_sm, e_st)
