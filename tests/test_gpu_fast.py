"""Split-f16 precision mode (module.precision = "f16x3"): the convs and projections run as three f16 MFMAs per product
on (f16 hi, f16 lo) operand pairs with f32 accumulation.  It must satisfy the SAME parity bar as the exact-f32 mode:
logits/tokens within the north-star 1e-3 of the reference's golden vectors, bit-exact selections / arg-max / hardest
negatives, plus kernel-level checks of the split representation (22-bit products) against float64."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import case_dict  # noqa: E402
from oracle import sola_oracle  # noqa: E402
from sola_amd import _lib, ops, synth  # noqa: E402
from sola_amd._lib import tune_default, tuned  # noqa: E402
from sola_amd.loss import track_selection_losses  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

POS_W, TEMP, ALIGN_W = 1.5, 0.07, 0.3


def cuda(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def test_split_representation_has_22_bits():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((64, 256)) * np.exp(rng.uniform(-6, 3, size=(64, 256)))).astype(np.float32)
    for scale in (1.0, 64.0):
        dec = ops.decode_sp16(ops.cast_sp16(cuda(x), scale)).cpu().numpy().astype(np.float64)
        v = x.astype(np.float64) * scale
        err = np.abs(dec - v)
        # hi carries 11 bits, lo the next 11; once lo drops below the f16 normal range (|v| < ~0.1) its absolute
        # resolution is the subnormal spacing 2^-24, i.e. an error floor of 3e-8 regardless of |v|
        assert np.all(err <= 2.0 ** -21 * np.abs(v) + 3.1e-8), float((err - 2.0 ** -21 * np.abs(v)).max())
        assert np.abs(dec[np.abs(v) > 0.25] / v[np.abs(v) > 0.25] - 1).max() < 2.0 ** -21


@pytest.mark.parametrize("M,N,K", [(256, 1024, 1024), (100, 72, 96), (4096, 512, 768), (16384, 1024, 1024), (48, 2048, 1024)])
def test_split_gemm_vs_float64(M, N, K):
    rng = np.random.default_rng(M + N + K)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.uniform(-1, 1, size=(N, K)) / 32).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + b + r
    got = ops.gemm_nt_split(ops.cast_sp16(cuda(a)), ops.cast_sp16(cuda(w), 64.0), cuda(b), cuda(r), False, 1.0 / 64.0).cpu().numpy()
    f32 = ops.gemm_nt(cuda(a), cuda(w), cuda(b), cuda(r)).cpu().numpy()
    err_split = np.abs(got - ref).max()
    err_f32 = np.abs(f32 - ref).max()
    # same error class as exact-f32 accumulation (f32 accumulate dominates; products carry 22 bits)
    assert err_split <= max(4 * err_f32, 2e-6 * np.abs(ref).max()), (err_split, err_f32)
    # residual given in the split format
    got2 = ops.gemm_nt_split(ops.cast_sp16(cuda(a)), ops.cast_sp16(cuda(w), 64.0), cuda(b), ops.cast_sp16(cuda(r[:, : (N // 8) * 8]))
                             if N % 8 == 0 else cuda(r), N % 8 == 0, 1.0 / 64.0).cpu().numpy()
    assert np.abs(got2 - ref).max() <= max(4 * err_f32, 3e-6 * np.abs(ref).max())


def build(cfg, precision):
    m = LanguageAlignedTrackSelectionModule(cfg)
    sd = synth.make_state_dict(cfg, 42)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.precision = precision
    return m, sd


def run(m, cfg, B, N, T, L, seed):
    inp = synth.make_inputs(cfg, B, N, T, L, seed)
    c = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    with torch.no_grad():
        sm, st = m(c["object_tokens"], c["lang_tokens"])
        loss3, argmax = track_selection_losses(sm, st, c["labels"], c["pos_tokens"], m.negative_token.weight, POS_W, TEMP, ALIGN_W,
                                               return_argmax=True)
    return inp, sm, st, loss3, argmax


@pytest.fixture(scope="module")
def full_fast():
    return build(synth.DEFAULT_MODEL_CFG, "f16x3")


@pytest.fixture(scope="module")
def full_f32():
    return build(synth.DEFAULT_MODEL_CFG, "f32")


def test_few_row_calls_of_the_default_mode_run_exact_f32(full_fast, full_f32):
    """Round 4 (sola_tune "infer_f32_rows", default 4096 object-token rows - conftest.py switches it off for the other tests): one sample per
    call in the default precision runs the exact-f32 kernels (faster there since the few-row GEMM shape, no guard read-back) - the output of
    the "f16x3" module IS the "f32" module's, uniform and ragged; larger calls and the key at 0 take the split-f16 pass as before."""
    mf, _ = full_fast
    m32, _ = full_f32
    cfg = synth.DEFAULT_MODEL_CFG
    with tuned(infer_f32_rows=tune_default("infer_f32_rows")):
        _, sm_a, st_a, _, _ = run(mf, cfg, 1, 64, 32, 16, 77)      # 2048 rows: routed
        _, sm_b, st_b, _, _ = run(m32, cfg, 1, 64, 32, 16, 77)
        assert torch.equal(sm_a, sm_b) and torch.equal(st_a, st_b)
        _, sm_c, _, _, _ = run(mf, cfg, 4, 64, 32, 16, 78)          # 8192 rows: the split pass
        _, sm_d, _, _, _ = run(m32, cfg, 4, 64, 32, 16, 78)
        assert not torch.equal(sm_c, sm_d) and float((sm_c - sm_d).abs().max()) < 1e-3
        inp = synth.make_inputs(cfg, 1, 20, 50, 7, 79)
        obj, lang = torch.from_numpy(inp["object_tokens"][0]).cuda(), torch.from_numpy(inp["lang_tokens"][0]).cuda()
        with torch.no_grad():
            ra = mf.forward_ragged([obj], [lang])
            rb = m32.forward_ragged([obj], [lang])
        assert all(torch.equal(x, y) for x, y in zip(ra[0], rb[0]))
        with tuned(infer_f32_rows=0):
            _, sm_e, _, _, _ = run(mf, cfg, 1, 64, 32, 16, 77)
        assert not torch.equal(sm_e, sm_b) and float((sm_e - sm_b).abs().max()) < 1e-3


@pytest.mark.parametrize("ci", range(5))
def test_full_cases_vs_golden_in_the_shipped_routing(full_golden, full_fast, ci):
    """the golden cases through the PRODUCTION configuration of the default mode - sola_tune "infer_f32_rows" at its shipped
    4096 (conftest.py switches it off for the other tests), so the few-row cases take the exact-f32 route inside the "f16x3" module and the
    larger ones the split-f16 pass - against the reference's outputs, not against another module of this library."""
    m, _ = full_fast
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = [int(v) for v in full_golden["cases"][ci]]
    g = case_dict(full_golden, ci)
    with tuned(infer_f32_rows=tune_default("infer_f32_rows")):
        _, sm, st, loss3, argmax = run(m, cfg, B, N, T, L, 200 + ci)
    assert np.abs(sm.cpu().numpy() - g["score_map"]).max() <= 1e-3
    assert np.abs(st.cpu().numpy() - g["score_tokens"]).max() <= 1e-3
    np.testing.assert_allclose(loss3.cpu().numpy().astype(np.float64), g["loss"], rtol=2e-4, atol=2e-4)
    np.testing.assert_array_equal((torch.sigmoid(sm) > 0.5).float().cpu().numpy(), g["selected"])
    np.testing.assert_array_equal(sm.argmax(dim=1).cpu().numpy(), g["argmax_track"])
    np.testing.assert_array_equal(argmax.cpu().numpy(), g["neg_argmax"])


@pytest.mark.parametrize("ci", range(5))
def test_full_cases_vs_golden_in_split_mode(full_golden, full_fast, ci):
    m, _ = full_fast
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = [int(v) for v in full_golden["cases"][ci]]
    g = case_dict(full_golden, ci)
    _, sm, st, loss3, argmax = run(m, cfg, B, N, T, L, 200 + ci)
    assert np.abs(sm.cpu().numpy() - g["score_map"]).max() <= 1e-3
    assert np.abs(st.cpu().numpy() - g["score_tokens"]).max() <= 1e-3
    np.testing.assert_allclose(loss3.cpu().numpy().astype(np.float64), g["loss"], rtol=2e-4, atol=2e-4)
    np.testing.assert_array_equal((torch.sigmoid(sm) > 0.5).float().cpu().numpy(), g["selected"])
    np.testing.assert_array_equal(sm.argmax(dim=1).cpu().numpy(), g["argmax_track"])
    np.testing.assert_array_equal(argmax.cpu().numpy(), g["neg_argmax"])


def test_split_mode_error_is_in_the_f32_class(full_fast, full_f32):
    """Against a float64 evaluation of the oracle at the north-star shape: the split mode's error is no worse than
    twice the exact-f32 mode's (both are dominated by f32 accumulation / GroupNorm rounding)."""
    cfg = synth.DEFAULT_MODEL_CFG
    mf, sd = full_fast
    m32, _ = full_f32
    inp, sm_f, st_f, _, _ = run(mf, cfg, 2, 64, 32, 16, 4321)
    _, sm_3, st_3, _, _ = run(m32, cfg, 2, 64, 32, 16, 4321)
    rsm, rst = sola_oracle.forward(sd, cfg, inp["object_tokens"], inp["lang_tokens"], dtype=torch.float64)
    e_fast = max(np.abs(sm_f.cpu().numpy() - rsm.numpy()).max(), np.abs(st_f.cpu().numpy() - rst.numpy()).max())
    e_f32 = max(np.abs(sm_3.cpu().numpy() - rsm.numpy()).max(), np.abs(st_3.cpu().numpy() - rst.numpy()).max())
    print(f"max error vs float64: split-f16 {e_fast:.3e}, exact f32 {e_f32:.3e}")
    assert e_fast <= 5e-4 and e_fast <= 2.0 * e_f32 + 5e-5


@pytest.mark.parametrize("ci", range(6))
def test_small_cases_in_split_mode(small_golden, ci):
    cfg = synth.SMALL_MODEL_CFG
    m, _ = build(cfg, "f16x3")
    B, N, T, L = [int(v) for v in small_golden["cases"][ci]]
    g = case_dict(small_golden, ci)
    _, sm, st, loss3, argmax = run(m, cfg, B, N, T, L, 100 + ci)
    assert np.abs(sm.cpu().numpy() - g["score_map"]).max() <= 1e-3
    assert np.abs(st.cpu().numpy() - g["score_tokens"]).max() <= 1e-3
    np.testing.assert_array_equal((torch.sigmoid(sm) > 0.5).float().cpu().numpy(), g["selected"])
    np.testing.assert_array_equal(argmax.cpu().numpy(), g["neg_argmax"])
    # intermediate in the split format decodes to the reference activations
    ref = g["tap.l1_motion"]
    got = ops.decode_sp16(m.workspace_tap("l1_motion")).cpu().numpy().reshape(ref.shape)
    assert np.abs(got - ref).max() <= 3e-4 * max(1.0, np.abs(ref).max())


def _attn_ref64(q, k, v, H):
    G, Sq, D = q.shape
    dh = D // H
    qh = q.reshape(G, Sq, H, dh).transpose(0, 2, 1, 3)
    kh = k.reshape(G, -1, H, dh).transpose(0, 2, 1, 3)
    vh = v.reshape(G, -1, H, dh).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(dh)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ vh).transpose(0, 2, 1, 3).reshape(G, Sq, D)


@pytest.mark.parametrize("B,N,Tp,D", [(1, 64, 4, 1024), (2, 80, 1, 1024), (1, 130, 2, 128), (1, 20, 25, 128), (1, 128, 2, 1024), (2, 17, 3, 256),
                                      # head_dim 128: the high-occupancy shape for split inputs (attn_fwd_spin_kernel) with partial
                                      # query / key tiles and three key stages; > 128 queries: attn.hip's kernel
                                      (3, 33, 2, 1024), (1, 100, 3, 1024), (2, 47, 1, 1024)])
def test_split_attention_kernel_vs_float64(B, N, Tp, D):
    """sola_attention_split (q, k, v as split-f16 rows, three f16 MFMAs per product) in the inter-object and
    object->language layouts, f32 and split-f16 output, against float64 softmax attention: f32-class error."""
    H = 8
    rng = np.random.default_rng(N * Tp + D)
    q, k, v = (rng.standard_normal((B, N, Tp, D)).astype(np.float32) for _ in range(3))
    q64, k64, v64 = (t.astype(np.float64) for t in (q, k, v))
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    qs, ks, vs = (ops.cast_sp16(dev(t).reshape(B * N * Tp, D)) for t in (q, k, v))
    tr = lambda t: np.transpose(t, (0, 2, 1, 3)).reshape(B * Tp, N, D)
    ref = _attn_ref64(tr(q64), tr(k64), tr(v64), H).reshape(B, Tp, N, D).transpose(0, 2, 1, 3)
    got = ops.attention_split(qs, ks, vs, B * Tp, H, N, N, Tp, (N * Tp, 1, Tp), (N * Tp, 1, Tp)).reshape(B, N, Tp, D).cpu().numpy()
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
    exact = ops.attention(dev(q).reshape(-1, D), dev(k).reshape(-1, D), dev(v).reshape(-1, D), B * Tp, H, N, N, Tp,
                          (N * Tp, 1, Tp), (N * Tp, 1, Tp)).reshape(B, N, Tp, D).cpu().numpy()
    # same class as the exact-f32 MFMA kernel (whose own error depends on its summation order: the high-occupancy shape that
    # serves these sizes accumulates over 32-key tiles and is a little closer to float64 than the 64-key one was)
    assert np.abs(got - ref).max() <= max(4 * np.abs(exact - ref).max(), 1e-5), (np.abs(got - ref).max(), np.abs(exact - ref).max())
    got16 = ops.decode_sp16(ops.attention_split(qs, ks, vs, B * Tp, H, N, N, Tp, (N * Tp, 1, Tp), (N * Tp, 1, Tp), out_split=True))
    assert np.abs(got16.reshape(B, N, Tp, D).cpu().numpy() - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
    for Wn in (48, 37, 70):
        lk, lv = (rng.standard_normal((B, Wn, D)).astype(np.float32) for _ in range(2))
        ref = _attn_ref64(q64.reshape(B, N * Tp, D), lk.astype(np.float64), lv.astype(np.float64), H).reshape(B, N, Tp, D)
        got = ops.attention_split(qs, ops.cast_sp16(dev(lk).reshape(B * Wn, D)), ops.cast_sp16(dev(lv).reshape(B * Wn, D)), B, H, N * Tp,
                                  Wn, 1, (N * Tp, 0, 1), (Wn, 0, 1)).reshape(B, N, Tp, D).cpu().numpy()
        assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), (Wn, np.abs(got - ref).max())


def test_split_gemm_split_output():
    """c_is_split: the GEMM writes its result as split-f16 pairs (what the split attention reads)."""
    rng = np.random.default_rng(3)
    for (M, N, K) in [(16384, 1024, 1024), (300, 72, 96), (4096, 512, 768)]:
        a = rng.standard_normal((M, K)).astype(np.float32)
        w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        asp, wsp = ops.cast_sp16(torch.from_numpy(a).cuda()), ops.cast_sp16(torch.from_numpy(w).cuda(), 64.0)
        ref = ops.gemm_nt_split(asp, wsp, torch.from_numpy(b).cuda(), out_scale=1 / 64)
        got = ops.decode_sp16(ops.gemm_nt_split(asp, wsp, torch.from_numpy(b).cuda(), out_scale=1 / 64, out_split=True))
        err = (got - ref).abs().max().item()
        assert err <= 2.0 ** -21 * ref.abs().max().item() + 1e-7, (M, N, K, err)


def _needs_experiments():
    if not _lib.has_experiments():
        pytest.skip("closed experiment: compiled in EXPERIMENTS=1 builds of the library only (make -C sola_amd/csrc EXPERIMENTS=1)")


@pytest.mark.parametrize("M,N,K", [(1000, 520, 96), (777, 264, 64), (2048, 1024, 160), (300, 72, 96), (4100, 256, 320)])
def test_split_gemm_block_shapes_bit_identical(M, N, K):
    """The 128x128 kernel, the one-tile 256x256 kernel and the persistent 256x256 kernel accumulate every output element
    in the same order, so they must agree bit for bit - on ragged M / N (clamped DMA rows, the predicated epilogue), with
    no / f32 / split residual and with f32 / split output; one variant is also checked against float64."""
    rng = np.random.default_rng(M * 7 + N)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32)
    asp, wsp, bd, rd = ops.cast_sp16(cuda(a)), ops.cast_sp16(cuda(w), 64.0), cuda(b), cuda(r)
    rsp = ops.cast_sp16(rd) if N % 8 == 0 else None
    settings = [dict(gemm_glds=1, gemm_persist=0), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=4, gemm_persist=1)]
    with tuned(gemm_glds_force=1):  # these grids are far too small for the direct-to-LDS kernels to be chosen
        for res, res_split, out_split in [(None, False, False), (rd, False, False), (rsp, True, False), (None, False, True), (rsp, True, True)]:
            if res_split and rsp is None:
                continue
            if out_split and N % 8:
                continue
            outs = []
            for st in settings:
                with tuned(**st):
                    outs.append(ops.gemm_nt_split(asp, wsp, bd, res, res_split, 1.0 / 64.0, out_split).clone())
            torch.cuda.synchronize()
            for o in outs[1:]:
                assert torch.equal(outs[0].view(torch.int32), o.view(torch.int32)), (res is not None, res_split, out_split)
        with tuned(gemm_glds=4, gemm_persist=1):
            got = ops.gemm_nt_split(asp, wsp, bd, rd, False, 1.0 / 64.0).cpu().numpy()
        ref = ops.decode_sp16(asp).double().cpu().numpy() @ (ops.decode_sp16(wsp).double().cpu().numpy() / 64.0).T + b + r
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("seed", range(10))
def test_split_gemm_block_shapes_random(seed):
    """Seeded random shapes (ragged M, N % 8 == 0, K % 32 == 0, 2..20 k-tiles) through the three direct-to-LDS kernels: bit
    identical to each other for every epilogue flavour, and right against float64."""
    rng = np.random.default_rng(1000 + seed)
    M, N, K = int(rng.integers(1, 3000)), 8 * int(rng.integers(1, 140)), 32 * int(rng.integers(2, 21))
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32)
    asp, wsp, bd, rd = ops.cast_sp16(cuda(a)), ops.cast_sp16(cuda(w), 64.0), cuda(b), cuda(r)
    rsp = ops.cast_sp16(rd)
    with tuned(gemm_glds_force=1):
        for res, res_split, out_split in [(None, False, False), (rd, False, False), (rsp, True, False), (rsp, True, True)]:
            outs = []
            for st in [dict(gemm_glds=1, gemm_persist=0), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=4, gemm_persist=1)]:
                with tuned(**st):
                    outs.append(ops.gemm_nt_split(asp, wsp, bd, res, res_split, 1.0 / 64.0, out_split).clone())
            torch.cuda.synchronize()
            for o in outs[1:]:
                assert torch.equal(outs[0].view(torch.int32), o.view(torch.int32)), (M, N, K, res is not None, res_split, out_split)
        with tuned(gemm_glds=4, gemm_persist=1):  # (the persistent kernel, as the last of the three above)
            got = ops.gemm_nt_split(asp, wsp, bd, rd, False, 1.0 / 64.0).cpu().numpy()
        ref = ops.decode_sp16(asp).double().cpu().numpy() @ (ops.decode_sp16(wsp).double().cpu().numpy() / 64.0).T + b + r
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), (M, N, K)


def test_forward_identical_across_gemm_kernels(full_fast):
    """Whole split-mode forward (implicit-im2col conv launches, three-problem q/k/v launches, residual and split-output
    epilogues) through the persistent kernel, the one-tile kernel and the 128x128 kernel: same bits."""
    m, _ = full_fast
    inp = synth.make_inputs(synth.DEFAULT_MODEL_CFG, 8, 40, 32, 12, 5)
    obj, lang = torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda()
    outs = []
    # the norm applied in the persistent kernel's epilogue exists in that kernel only (and in EXPERIMENTS=1 builds only: the default build
    # has no such key, the experiment is off by construction)
    fuse_off = {"gemm_gn_fuse": 0} if _lib.has_experiments() else {}
    with tuned(gemm_glds_force=1, **fuse_off):
        for st in [dict(gemm_glds=4, gemm_persist=1), dict(gemm_glds=4, gemm_persist=0), dict(gemm_glds=1, gemm_persist=0)]:
            with tuned(**st), torch.no_grad():
                sm, tok = m(obj, lang)
            outs.append((sm.clone(), tok.clone()))
        torch.cuda.synchronize()
    for sm, tok in outs[1:]:
        assert torch.equal(outs[0][0], sm) and torch.equal(outs[0][1], tok)


@pytest.mark.parametrize("mag", [1e-9, 3e-6, 1e-3, 40.0, 3e4])
@pytest.mark.parametrize("M,N,K", [(300, 72, 96), (16384, 1024, 1024)])
def test_split_gemm_auto_scaled_operand(M, N, K, mag):
    """cast_sp16_auto: an operand of unknown magnitude (gradients; far below or above the f16 range) is scaled by a
    data-dependent power of two on the device and the GEMM undoes it through out_scale_dev - same relative accuracy as
    for O(1) data, for entries spanning six decades inside the tensor."""
    rng = np.random.default_rng(int(M + K))
    a = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-14, 0, size=(M, 1))) * mag).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
    asp, scal = ops.cast_sp16_auto(cuda(a))
    assert float(scal[0]) == float(np.abs(a).max())
    inv = float(scal[1])
    assert inv > 0 and math.log2(inv) == int(math.log2(inv)) and 2.0 ** 13 <= float(np.abs(a).max()) / inv < 2.0 ** 14
    got = ops.gemm_nt_split(asp, ops.cast_sp16(cuda(w), 64.0), out_scale=1.0 / 64.0, out_scale_dev=scal[1:]).cpu().numpy()
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    f32 = ops.gemm_nt(cuda(a), cuda(w)).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= max(4 * np.abs(f32 - ref).max(), 2e-6 * np.abs(ref).max())


def test_fused_norm_epilogue_is_repeatable_and_matches_the_unfused_activations():
    """The fused conv + GroupNorm + LeakyReLU epilogue at the headline shape, 12 forwards: every encoder activation it writes
    (act0..act2, split-f16 pairs) is bit-identical from run to run and within 2e-5 of the separate launches.  Regression test
    for two faults of earlier versions of the epilogue that showed up as a handful of wrong rows per launch, different ones
    each run ("fused norm"): a packed-f32 subtract behind a per-store exec-masked range check that left one
    element of a strip's last row uncentred, and SLP-vectorised statistics that returned garbage rows; tools/gnf_stress.py
    is the longer version."""
    _needs_experiments()  # round 5: the fused norm is closed (bit-repeatable, but no gain on the power-bound launch - profiles/r05_gnf_decision.txt)
    cfg = synth.DEFAULT_MODEL_CFG
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, 42).items()})
    m = m.cuda().eval(); m.precision = "f16x3"
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 128, 64, 32, 16, 31).items()}
    names = ("act0", "act1", "act2")

    def unsplit(t):  # [rows, C] floats holding [hi8|lo8] halfs per 8 values
        h = t.view(torch.float16).reshape(t.shape[0], -1, 2, 8).float()
        return (h[:, :, 0, :] + h[:, :, 1, :]).reshape(t.shape[0], -1)

    def run(fuse):
        with tuned(gemm_gn_fuse=fuse):
            with torch.no_grad():
                m(inp["object_tokens"], inp["lang_tokens"])
            torch.cuda.synchronize()
            return {nm: m.workspace_tap(nm) for nm in names}

    ref = run(0)
    first = run(1)
    for nm in names:
        assert float((unsplit(first[nm]) - unsplit(ref[nm])).abs().max()) <= 2e-5, nm
    for _ in range(11):
        t = run(1)
        for nm in names:
            assert torch.equal(t[nm].view(torch.int32), first[nm].view(torch.int32)), nm
    assert m.split_fallbacks()[1] == 0


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_forward_and_gradients_repeat_bit_for_bit(precision):
    """No kernel of the path uses float atomics: logits, tokens and every gradient of a training step repeat bit for bit from
    run to run in every precision mode (tools/repeat_stress.py is the long version, with the ragged forward)."""
    cfg = synth.DEFAULT_MODEL_CFG
    sd = synth.make_state_dict(cfg, 42)
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.cuda().eval(); m.precision = precision
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 128, 64, 32, 16, 31).items()}
    first = None
    for _ in range(5):
        with torch.no_grad():
            sm, st = m(inp["object_tokens"], inp["lang_tokens"])
        cur = (sm.view(torch.int32).clone(), st.view(torch.int32).clone())
        if first is None:
            first = cur
        assert torch.equal(cur[0], first[0]) and torch.equal(cur[1], first[1])
    from sola_amd.loss import track_selection_losses
    B = 16
    tinp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, B, 64, 32, 16, 1).items()}
    m.train()
    first = None
    for _ in range(3):
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(11)  # the dropout seed of the step is drawn from torch's generator
        sm, st = m(tinp["object_tokens"], tinp["lang_tokens"])
        neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
        track_selection_losses(sm, st, tinp["labels"], tinp["pos_tokens"], neg, 1.5, 0.07, 0.3)[0].backward()
        cur = [p.grad.view(torch.int32).clone() for p in m.parameters() if p.grad is not None]
        if first is None:
            first = cur
        assert all(torch.equal(a, b) for a, b in zip(cur, first))


def test_norm_fused_into_the_conv_epilogue_matches_the_separate_launch():
    """At GPU-filling batches the first three encoder norms (64 channels per group) are applied in the conv GEMM's epilogue
    (gemm_glds.hip, GNT).  128 samples of the headline shape: conv0 / conv1 / conv2 all qualify; the logits must agree with the
    same forward running the separate GroupNorm launches (sola_tune gemm_gn_fuse 0) to f32 summation noise, decisions equal."""
    _needs_experiments()
    cfg = synth.DEFAULT_MODEL_CFG
    m = LanguageAlignedTrackSelectionModule(cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, 42).items()})
    m = m.cuda().eval(); m.precision = "f16x3"
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 128, 64, 32, 16, 31).items()}
    outs = {}
    for fuse in (1, 0):
        with tuned(gemm_gn_fuse=fuse), torch.no_grad():
            sm, st = m(inp["object_tokens"], inp["lang_tokens"])
        outs[fuse] = (sm.clone(), st.clone())
    assert m.split_fallbacks()[1] == 0
    d_sm = float((outs[1][0] - outs[0][0]).abs().max()); d_st = float((outs[1][1] - outs[0][1]).abs().max())
    # f32 rounding noise reaches the logits amplified ~1000x (the reference itself sits 1e-4 from a float64 evaluation at this
    # shape): two correct evaluation orders differ by a few 1e-4; the absolute bar is test_batch_256_every_row_vs_oracle
    assert d_sm <= 6e-4 and d_st <= 6e-4, (d_sm, d_st)
    assert torch.equal(outs[1][0] > 0, outs[0][0] > 0) or float((outs[1][0] - outs[0][0]).abs()[(outs[1][0] > 0) != (outs[0][0] > 0)].max()) < 1e-3


@pytest.mark.parametrize("shape", [(256, 64, 32, 16), (64, 16, 32, 16), (70, 33, 40, 24), (8, 64, 32, 5)])
def test_negative_token_projections_shared_across_samples(full_fast, shape):
    """Round 5 (sola_tune "lang_shared_neg"): the 32 negative tokens appended to every sample's text (module/module.py:146-147) have the
    same key / value projections for every sample - the text-side GEMMs of the default forward take B * L + 32 rows instead of B * (L + 32)
    and the object -> language attention reads the shared rows (AttnDesc::k_private).  Same products per row: logits and tokens are
    BIT-identical to the repeated form (small batches keep the repeated form: the few-row GEMM's split over K depends on the row count)."""
    m, _ = full_fast
    B, N, T, L = shape
    inp = synth.make_inputs(synth.DEFAULT_MODEL_CFG, B, N, T, L, 17)
    obj, lang = torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda()
    outs = []
    for v in (0, 1):
        with tuned(lang_shared_neg=v), torch.no_grad():
            sm, tok = m(obj, lang)
        outs.append((sm.clone(), tok.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
