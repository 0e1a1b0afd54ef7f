"""Backward parity on the MI355X.  Per-kernel: each HIP backward against torch autograd of the float64 oracle on the
same seeded inputs.  Whole path: every parameter gradient of loss.backward() against the gradients the REAL reference
produced (tests/golden, full tensors for two small cases, per-parameter norms elsewhere) and against autograd through
the oracle evaluated here."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import case_dict  # noqa: E402
from oracle import sola_oracle  # noqa: E402
from sola_amd import ops, synth  # noqa: E402
from sola_amd._lib import tuned  # noqa: E402
from sola_amd.loss import track_selection_losses  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

POS_W, TEMP, ALIGN_W = 1.5, 0.07, 0.3


def cuda(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(size=shape) * scale).astype(np.float32)


def t64(x, grad=False):
    return torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=grad)


def assert_close(got, ref, rel=3e-5, name=""):
    got = got.detach().cpu().double().numpy()
    ref = np.asarray(ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    tol = rel * max(1e-6, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= tol, f"{name}: max err {err:.3e} > {tol:.3e} (ref max {np.abs(ref).max():.3e})"


@pytest.mark.parametrize("M,N,K", [(256, 128, 128), (1000, 70 * 4, 36), (16384, 1024, 1024), (48, 64, 128), (5, 4, 8)])
def test_gemm_tn(M, N, K):
    rng = np.random.default_rng(M + N)
    a, b = rnd(rng, M, N), rnd(rng, M, K)
    out, bias = ops.gemm_tn(cuda(a), cuda(b), want_bias_grad=True)
    assert_close(out, a.astype(np.float64).T @ b.astype(np.float64), name="gemm_tn")
    assert_close(bias, a.astype(np.float64).sum(axis=0), name="bias grad")


@pytest.mark.parametrize("mag", [1.0, 1e-7])
@pytest.mark.parametrize("M,N,K", [(256, 128, 128), (1000, 280, 40), (16384, 1024, 1024), (70, 64, 128), (5000, 520, 264)])
def test_gemm_tn_split(M, N, K, mag):
    """Weight gradient on the split-f16 path: transposing casts (zero-padded rows, ragged column tiles), device-side scale
    for gradient-sized dY, split-K persistent GEMM + ordered reduce; against float64, same bar as the f32 kernel."""
    rng = np.random.default_rng(M + N)
    a, b = rnd(rng, M, N, scale=mag), rnd(rng, M, K)
    out = ops.gemm_tn_split(cuda(a), cuda(b))
    assert_close(out, a.astype(np.float64).T @ b.astype(np.float64), name="gemm_tn_split")
    assert torch.equal(out, ops.gemm_tn_split(cuda(a), cuda(b)))  # fixed reduction order


@pytest.mark.parametrize("cout,cin,k", [(64, 32, 3), (512, 256, 3), (1024, 1024, 1), (8, 4, 3)])
def test_ws_backward(cout, cin, k):
    rng = np.random.default_rng(cout)
    w = rnd(rng, cout, cin, k, scale=0.05) + 0.01
    g = rnd(rng, cout, cin, k)
    wt = t64(w, True)
    sola_oracle.standardize_weight(wt).backward(t64(g))
    g_k = np.ascontiguousarray(np.transpose(g, (0, 2, 1)).reshape(cout, k * cin))  # GEMM layout [cout][k][cin]
    got = ops.ws_backward(cuda(w), cuda(g_k))
    assert_close(got, wt.grad, name="ws backward")


@pytest.mark.parametrize("R,T,cin,cout,k,s,p", [(5, 33, 32, 64, 3, 2, 1), (3, 8, 64, 64, 3, 1, 1), (4, 1, 32, 64, 3, 2, 1),
                                                (64, 32, 256, 512, 3, 2, 1), (7, 5, 128, 128, 1, 1, 0), (2, 200, 32, 64, 3, 2, 1)])
def test_conv1d_backward(R, T, cin, cout, k, s, p):
    rng = np.random.default_rng(R * T + cin)
    x, w, b = rnd(rng, R, T, cin), rnd(rng, cout, cin, k, scale=0.1), rnd(rng, cout)
    xt, wt, bt = t64(x, True), t64(w, True), t64(b, True)
    y = sola_oracle.conv1d_cl(xt, wt, bt, s, p)
    dy = rnd(rng, *y.shape)
    y.backward(t64(dy))
    wk = np.ascontiguousarray(np.transpose(w, (0, 2, 1)).reshape(cout, k * cin))
    dx, dw, db = ops.conv1d_cl_backward(cuda(x), cuda(wk), cuda(dy), k, s, p)
    assert_close(dx, xt.grad, name="conv dx")
    assert_close(dw.reshape(cout, k, cin).permute(0, 2, 1), wt.grad, name="conv dw")
    assert_close(db, bt.grad, name="conv db")


@pytest.mark.parametrize("mag", [1.0, 1e-6])
@pytest.mark.parametrize("R,T,cin,cout,k,s,p", [(64, 32, 256, 512, 3, 2, 1), (16, 16, 128, 128, 3, 1, 1), (9, 41, 64, 128, 3, 2, 1),
                                                (7, 20, 128, 128, 1, 1, 0), (33, 4, 512, 1024, 3, 1, 1)])
def test_conv1d_backward_split(R, T, cin, cout, k, s, p, mag):
    """The split-f16 conv backward of the training path (per-tap transposing im2col casts + split-K GEMM for dW; one GEMM
    over the output steps + col2im gather for dX), gradient-sized dY included, against float64 autograd."""
    rng = np.random.default_rng(R * T + cin)
    x, w, b = rnd(rng, R, T, cin), rnd(rng, cout, cin, k, scale=0.1), rnd(rng, cout)
    xt, wt, bt = t64(x, True), t64(w, True), t64(b, True)
    y = sola_oracle.conv1d_cl(xt, wt, bt, s, p)
    dy = rnd(rng, *y.shape, scale=mag)
    y.backward(t64(dy))
    wk = np.ascontiguousarray(np.transpose(w, (0, 2, 1)).reshape(cout, k * cin))
    dx, dw, db = ops.conv1d_cl_backward(cuda(x), cuda(wk), cuda(dy), k, s, p, split=True)
    assert_close(dx, xt.grad, name="conv dx")
    assert_close(dw.reshape(cout, k, cin).permute(0, 2, 1), wt.grad, name="conv dw")
    assert_close(db, bt.grad, name="conv db")


@pytest.mark.parametrize("B,N,Tp,C", [(2, 5, 3, 128), (1, 64, 4, 1024), (2, 3, 1, 64), (1, 7, 25, 512),
                                      # shape edges, tokens per track / per (b, t') / per sample:
                                      (1, 17, 1, 128),   # 1 / 17 / 17: wave R1, R2 with a partial last pass
                                      (1, 43, 3, 128),   # 3 / 43 / 129: wave R4; block R4 one token past the edge
                                      (1, 257, 2, 128),  # 2 / 257 / 514: block R8; 512 threads
                                      (1, 205, 5, 128),  # 5 / 205 / 1025: the 1024-thread register shape, one token past the edge
                                      (1, 683, 3, 128),  # 3 / 683 / 2049: three passes with 1024 threads
                                      (1, 5, 14, 384)])  # 48 channels per group: three passes with 256 threads, lanes with tl >= tpp idle
def test_group_norm_backward(B, N, Tp, C):
    rng = np.random.default_rng(C + N)
    x = rnd(rng, B, N, Tp, C) * 2 + 0.3
    gamma, beta = 1 + 0.1 * rnd(rng, C), 0.1 * rnd(rng, C)
    dy, dy2 = rnd(rng, B, N, Tp, C), rnd(rng, B, N, Tp, C)
    xc, dyc, dy2c = (cuda(t).reshape(B * N * Tp, C) for t in (x, dy, dy2))

    def ref(view, unview, leaky, extra):
        xt, gt, bt = t64(x, True), t64(gamma, True), t64(beta, True)
        y = sola_oracle.group_norm_tokens(view(xt), gt, bt, 8)
        if leaky:
            y = sola_oracle.leaky_relu(y)
        g = view(t64(dy)) + (view(t64(dy2)) if extra else 0)
        y.backward(g)
        return xt.grad, gt.grad, bt.grad

    # per track (encoder with LeakyReLU, and motion norm)
    for leaky in (True, False):
        rx, rg, rb = ref(lambda t: t.reshape(B * N, Tp, C), None, leaky, False)
        dx, dg, db = ops.group_norm_backward(xc, dyc, cuda(gamma), cuda(beta), 8, B * N, 1, Tp, 0, 1, Tp,
                                             leaky_slope=0.01 if leaky else None)
        assert_close(dx.reshape(B, N, Tp, C), rx, name=f"gn dx leaky={leaky}")
        assert_close(dg, rg, name="gn dgamma")
        assert_close(db, rb, name="gn dbeta")
    # per (b, t') with the second gradient stream of the x+pe output
    rx, rg, rb = ref(lambda t: t.permute(0, 2, 1, 3).reshape(B * Tp, N, C), None, False, True)
    dx, dg, db = ops.group_norm_backward(xc, dyc, cuda(gamma), cuda(beta), 8, B * Tp, Tp, N * Tp, 1, Tp, N, dy2=dy2c)
    assert_close(dx.reshape(B, N, Tp, C), rx, name="gn0 dx")
    assert_close(dg, rg, name="gn0 dgamma")
    assert_close(db, rb, name="gn0 dbeta")
    # per sample
    rx, rg, rb = ref(lambda t: t.reshape(B, N * Tp, C), None, False, False)
    dx, dg, db = ops.group_norm_backward(xc, dyc, cuda(gamma), cuda(beta), 8, B, 1, N * Tp, 0, 1, N * Tp)
    assert_close(dx.reshape(B, N, Tp, C), rx, name="gn2 dx")
    assert_close(dg, rg, name="gn2 dgamma")


def _attn_t(q, k, v, H):
    G, Sq, D = q.shape
    dh = D // H
    qh = q.reshape(G, Sq, H, dh).permute(0, 2, 1, 3)
    kh = k.reshape(G, -1, H, dh).permute(0, 2, 1, 3)
    vh = v.reshape(G, -1, H, dh).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(G, Sq, D)


@pytest.mark.parametrize("B,N,Tp,D", [(2, 5, 3, 128), (1, 64, 4, 1024), (1, 7, 16, 128), (1, 20, 25, 128), (2, 16, 4, 256), (1, 130, 2, 128),
                                      (2, 9, 2, 1024), (1, 12, 3, 1024),
                                      # the one-pass kernel (head_dim 128): one / two / four waves per unit, two key groups (70, 100, 128
                                      # keys), object -> language in 256-query chunks with a partial last chunk (360, 700 queries)
                                      (2, 40, 9, 1024), (1, 70, 10, 1024), (1, 100, 3, 1024), (1, 128, 2, 1024), (3, 20, 25, 1024)])
def test_attention_backward_three_layouts(B, N, Tp, D):
    H = 8
    rng = np.random.default_rng(N * Tp + D)
    q, k, v, do = (rnd(rng, B, N, Tp, D) for _ in range(4))
    qc, kc, vc, doc = (cuda(t).reshape(B * N * Tp, D) for t in (q, k, v, do))

    def run_ref(view):
        qt, kt, vt = t64(q, True), t64(k, True), t64(v, True)
        _attn_t(view(qt), view(kt), view(vt), H).backward(view(t64(do)))
        return qt.grad, kt.grad, vt.grad

    # inter-object
    view = lambda t: t.permute(0, 2, 1, 3).reshape(B * Tp, N, D)
    o, lse = ops.attention(qc, kc, vc, B * Tp, H, N, N, Tp, (N * Tp, 1, Tp), (N * Tp, 1, Tp), return_lse=True)
    got = ops.attention_backward(qc, kc, vc, o, doc, lse, B * Tp, H, N, N, Tp, (N * Tp, 1, Tp), (N * Tp, 1, Tp))
    for g, r, nm in zip(got, run_ref(view), "qkv"):
        assert_close(g.reshape(B, N, Tp, D), r, name=f"obj d{nm}")
    # motion
    view = lambda t: t.reshape(B * N, Tp, D)
    o, lse = ops.attention(qc, kc, vc, B * N, H, Tp, Tp, 1, (Tp, 0, 1), (Tp, 0, 1), return_lse=True)
    got = ops.attention_backward(qc, kc, vc, o, doc, lse, B * N, H, Tp, Tp, 1, (Tp, 0, 1), (Tp, 0, 1))
    for g, r, nm in zip(got, run_ref(view), "qkv"):
        assert_close(g.reshape(B, N, Tp, D), r, name=f"motion d{nm}")
    # object -> language
    Wn = 37
    lk, lv = rnd(rng, B, Wn, D), rnd(rng, B, Wn, D)
    qt, kt, vt = t64(q, True), t64(lk, True), t64(lv, True)
    _attn_t(qt.reshape(B, N * Tp, D), kt, vt, H).backward(t64(do).reshape(B, N * Tp, D))
    lkc, lvc = cuda(lk).reshape(B * Wn, D), cuda(lv).reshape(B * Wn, D)
    o, lse = ops.attention(qc, lkc, lvc, B, H, N * Tp, Wn, 1, (N * Tp, 0, 1), (Wn, 0, 1), return_lse=True)
    dq, dk, dv = ops.attention_backward(qc, lkc, lvc, o, doc, lse, B, H, N * Tp, Wn, 1, (N * Tp, 0, 1), (Wn, 0, 1))
    assert_close(dq.reshape(B, N, Tp, D), qt.grad, name="o2l dq")
    assert_close(dk.reshape(B, Wn, D), kt.grad, name="o2l dk")
    assert_close(dv.reshape(B, Wn, D), vt.grad, name="o2l dv")


def test_loss_backward_vs_oracle_autograd():
    rng = np.random.default_rng(4)
    B, N, D, n_neg = 2, 9, 128, 4
    sm, st = rnd(rng, B, N) * 3, rnd(rng, B, N, D)
    labels = (rng.uniform(size=(B, N)) < 0.3).astype(np.float32)
    pos, neg = rnd(rng, B, 1, D), rnd(rng, n_neg, D)
    for shared in (True, False):
        negv = neg if shared else np.ascontiguousarray(np.broadcast_to(neg[None], (B, n_neg, D))) + 0.01 * rnd(rng, B, n_neg, D)
        smt, stt, ngt = t64(sm, True), t64(st, True), t64(negv, True)
        ng_b = ngt.unsqueeze(0).expand(B, -1, -1) if shared else ngt
        ls = sola_oracle.losses(smt, stt, labels, pos, ng_b, POS_W, TEMP, ALIGN_W, dtype=torch.float64)
        (ls["total"] + 0.5 * ls["bce"] - 0.25 * ls["align"]).backward()
        a, b, c = cuda(sm).requires_grad_(), cuda(st).requires_grad_(), cuda(negv).requires_grad_()
        loss3 = track_selection_losses(a, b, cuda(labels), cuda(pos), c, POS_W, TEMP, ALIGN_W)
        (loss3[0] + 0.5 * loss3[1] - 0.25 * loss3[2]).backward()
        assert_close(a.grad, smt.grad, name="d score_map")
        assert_close(b.grad, stt.grad, name="d score_tokens")
        assert_close(c.grad, ngt.grad, name=f"d neg shared={shared}")


# ------------------------------------------------------------------------------------------------ whole path
def build(cfg, seed=42):
    m = LanguageAlignedTrackSelectionModule(cfg)
    sd = synth.make_state_dict(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.cuda().eval(), sd  # eval(): dropout off, as in the golden run; gradients still flow


def train_step_grads(m, cfg, B, N, T, L, seed):
    inp = synth.make_inputs(cfg, B, N, T, L, seed)
    c = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    m.zero_grad(set_to_none=True)
    sm, st = m(c["object_tokens"], c["lang_tokens"])
    # train.py:92: neg_tokens is a (cloned, repeated) view of the parameter, so it also receives gradient
    neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
    loss3 = track_selection_losses(sm, st, c["labels"], c["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
    loss3[0].backward()
    torch.cuda.synchronize()
    return inp, loss3, {k: p.grad for k, p in m.named_parameters()}


@pytest.fixture(scope="module")
def small_model():
    return build(synth.SMALL_MODEL_CFG)


@pytest.fixture(scope="module")
def full_model():
    return build(synth.DEFAULT_MODEL_CFG)


@pytest.mark.parametrize("ci", range(6))
def test_small_gradients_vs_reference(small_golden, small_model, ci):
    m, _ = small_model
    cfg = synth.SMALL_MODEL_CFG
    B, N, T, L = [int(v) for v in small_golden["cases"][ci]]
    g = case_dict(small_golden, ci)
    _, loss3, grads = train_step_grads(m, cfg, B, N, T, L, 100 + ci)
    np.testing.assert_allclose(loss3.detach().cpu().numpy().astype(np.float64), g["loss"], rtol=2e-4, atol=2e-4)
    # Some gradients are mathematically zero (a key-projection bias shifts every score of a query equally; a single
    # key when T'=1): both sides then hold fp32 noise, so the tolerance has a floor tied to the overall gradient scale.
    total = float(dict(zip([str(k) for k in g["grad_norm_keys"]], g["grad_norm_vals"]))["total_grad_norm"])
    bad = {}
    for k, gr in grads.items():
        assert gr is not None, k
        if "grad." + k in g:  # full reference gradient
            ref = g["grad." + k]
            err = float(np.abs(gr.cpu().numpy() - ref).max())
            tol = 2e-3 * float(np.abs(ref).max()) + 1e-6 * total
            if err > tol:
                bad[k] = (err, float(np.abs(ref).max()))
        else:
            ref = float(g["gradnorm." + k])
            got = float(gr.double().norm())
            if abs(got - ref) > 2e-3 * ref + 1e-5 * total:
                bad[k] = (got, ref)
    assert not bad, f"gradient mismatch: {bad}"
    gnd = m.get_grad_norm_dict()
    ref = dict(zip([str(k) for k in g["grad_norm_keys"]], g["grad_norm_vals"]))
    for k in ref:
        assert gnd[k] == pytest.approx(ref[k], rel=2e-3), k


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_full_gradient_norms_vs_reference(full_golden, full_model, ci, precision):
    """precision "f16x3": the training forward's GEMMs run on split-f16 casts of the f32 activations (the backward stays
    exact f32); same bar against the reference's losses and gradients."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = [int(v) for v in full_golden["cases"][ci]]
    g = case_dict(full_golden, ci)
    m.precision = precision
    try:
        with tuned(train_split_min_rows=0):  # these cases are below the production size gate
            _, loss3, grads = train_step_grads(m, cfg, B, N, T, L, 200 + ci)
    finally:
        m.precision = "f32"
    np.testing.assert_allclose(loss3.detach().cpu().numpy().astype(np.float64), g["loss"], rtol=2e-4, atol=2e-4)
    total = float(dict(zip([str(k) for k in g["grad_norm_keys"]], g["grad_norm_vals"]))["total_grad_norm"])
    bad = {}
    for k, gr in grads.items():
        ref = float(g["gradnorm." + k])
        got = float(gr.double().norm())
        if abs(got - ref) > 3e-3 * ref + 1e-5 * total:  # floor: exactly-zero gradients (key biases) are fp32 noise
            bad[k] = (got, ref)
    assert not bad, f"gradient-norm mismatch: {bad}"
    gnd = m.get_grad_norm_dict()
    ref = dict(zip([str(k) for k in g["grad_norm_keys"]], g["grad_norm_vals"]))
    for k in ref:
        assert gnd[k] == pytest.approx(ref[k], rel=3e-3), k


def test_split_training_gradients_match_exact_f32(full_model):
    """precision "f16x3" in training: forward GEMMs, projection and conv dX / dW GEMMs on split-f16 operands (dY cast with a
    data-dependent power-of-two scale: its entries are ~1e-4..1e-9, below the f16 normal range).  Every parameter gradient
    must agree with the exact-f32 path to 1 % in the Frobenius norm.  (Not element-wise: with ~1e6 pre-activations per
    encoder stage one of them regularly lies within rounding distance of LeakyReLU's kink, the two forwards then disagree
    on its sign and ONE output channel's weight / bias gradient moves by a few percent of the tensor's largest entry -
    either path does that against float64 autograd, at different channels: tools/train_grad_dbg.py.)"""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    grads = {}
    try:
        for prec in ("f32", "f16x3"):
            m.precision = prec
            _, _, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)  # 1280 token rows: the split kernels are taken from 1024 rows on
            grads[prec] = {k: v.clone() for k, v in g.items()}
    finally:
        m.precision = "f32"
    total = math.sqrt(sum(float(v.double().pow(2).sum()) for v in grads["f32"].values()))
    bad = {}
    for k, ref in grads["f32"].items():
        err = float((grads["f16x3"][k] - ref).double().norm())
        tol = 1e-2 * float(ref.double().norm()) + 1e-6 * total
        if err > tol:
            bad[k] = (err, float(ref.double().norm()))
    assert not bad, bad


def test_split_training_weight_gradient_products_on_f16_operands(full_model):
    """precision "f16x3" in training, sola_tune "train_dw_f16" (default 1): dW = dY^T X on plain f16 casts (one MFMA per product) while
    forward and dX keep the split pairs.  Against the exact-f32 step the weight matrices' median relative error rises from ~1e-5 to
    ~2e-4 (operand rounding averaged over >= 1024 rows), the worst tensor and the whole-gradient cosine do not move; with the switch
    off the median is back at the split level."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    out = {}
    try:
        m.precision = "f32"
        _, _, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)
        ref = {k: v.double().clone() for k, v in g.items()}
        total = math.sqrt(sum(float(v.pow(2).sum()) for v in ref.values()))
        for dw in (1, 0):
            m.precision = "f16x3"
            with tuned(train_dw_f16=dw):
                _, _, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)
            got = {k: v.double().clone() for k, v in g.items()}
            rel = sorted(float((got[k] - ref[k]).norm()) / (float(ref[k].norm()) + 1e-6 * total) for k in ref if k.endswith("weight") and ref[k].dim() >= 2)
            n = math.sqrt(sum(float(v.pow(2).sum()) for v in got.values()))
            out[dw] = (rel[len(rel) // 2], rel[-1], sum(float((got[k] * ref[k]).sum()) for k in ref) / (total * n))
    finally:
        m.precision = "f32"
    print("weight matrices, (median, worst) relative error and gradient cosine: f16 dW", out[1], "split dW", out[0])
    assert out[1][0] <= 1e-3 and out[1][1] <= 1e-2 and out[1][2] >= 0.9999, out
    assert out[0][0] <= 5e-5 and out[0][1] <= 1e-2 and out[0][2] >= 0.9999, out


# stated tolerances of the two 16-bit-operand training modes against the exact-f32 step: (loss rtol, min gradient cosine, worst
# tensor, median tensor, total-gradient-norm rtol against the REFERENCE's).  bf16 carries 8 significant bits where f16 carries 11:
# its operand rounding noise is 8x larger, so the same saturated-softmax near-ties (docstring below) move further - measured at
# this shape: loss within 0.6 %, cosine 0.744, worst tensor 73 %, median 4.8 %.  The yardstick for that error class is the textbook
# recipe on the ORACLE: autograd through oracle/sola_oracle.py under torch.autocast(bfloat16) against the same step in fp32 gives
# cosine 0.563, worst tensor 98 %, median 6.1 % (tools/bf16_autocast_oracle.py, profiles/r03_bf16_training.txt) - the library's
# mode keeps f32 storage between the GEMMs and lands inside it.
# Round 4: the bounds sit a small margin off the MEASURED statistics (profiles/r03_bf16_training.txt: f16 loss 1.3e-4,
# cosine 0.985, worst tensor 18 %, median 1.0 %; bf16 6.0e-3, 0.744, 73 %, 4.8 %), not at twice their value; the kernels are
# deterministic, so a regression of the tail shows.  (loss rtol, min cosine, worst tensor, median tensor, total-norm rtol)
LOWP_TRAIN_TOL = {"f16": (2e-3, 0.975, 0.22, 1.5e-2, 5e-2), "bf16": (1e-2, 0.73, 0.78, 6e-2, 0.15)}


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_f16_operand_training_vs_exact_f32(full_model, full_golden, mode):
    """precision "f16" in training (BASELINE config C2's 16-bit training): every GEMM of the step - forward, dX, dW - on plain
    f16 casts of the f32 activations / gradients with f32 accumulation (ONE MFMA per product; per-tensor power-of-two scales),
    everything else f32: mixed precision in the sense of torch.autocast, with f16's 11 bits instead of bf16's 8.
    A REDUCED-precision mode with a stated tolerance.  With random-init weights the first inter-object attention has scores of
    rms ~100 - a saturated softmax - so 2^-11 relative noise on its q / k flips near-ties: the logits move by up to 0.2-0.4 (as
    in the 16-bit inference mode) and the gradients of everything upstream of that attention (its q / k projections, the
    encoder) by 16-22 % in the Frobenius norm, the other tensors by 0.3-0.9 % (median), the whole gradient keeps a cosine of
    0.977-0.987 with the exact-f32 one (profiles/r02_f16_training_errors.log).  Stated: losses within 1 %, cosine >= 0.95,
    every tensor within 35 %, median within 3 %, total gradient norm within 5 % of the REFERENCE's.
    precision "bf16" (library precision 3) is the same step with bfloat16 operands (v_mfma_f32_32x32x16_bf16) - the format
    BASELINE config C2 names; its bounds are the second row of LOWP_TRAIN_TOL."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    l_rtol, min_cos, worst_tol, median_tol, norm_rtol = LOWP_TRAIN_TOL[mode]
    grads, losses = {}, {}
    try:
        for prec in ("f32", mode):
            m.precision = prec
            _, l3, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)  # 1280 token rows: above the size gate
            grads[prec] = {k: v.double().clone() for k, v in g.items()}
            losses[prec] = l3.detach().cpu().numpy().astype(np.float64)
    finally:
        m.precision = "f32"
    np.testing.assert_allclose(losses[mode], losses["f32"], rtol=l_rtol, atol=1e-3)
    ref = grads["f32"]
    total = math.sqrt(sum(float(v.pow(2).sum()) for v in ref.values()))
    n16 = math.sqrt(sum(float(v.pow(2).sum()) for v in grads[mode].values()))
    cos = sum(float((grads[mode][k] * ref[k]).sum()) for k in ref) / (total * n16)
    rel = sorted(float((grads[mode][k] - ref[k]).norm()) / (float(ref[k].norm()) + 1e-5 * total) for k in ref)
    lerr = float(np.abs(losses[mode] / losses["f32"] - 1).max())
    print(f"{mode}-operand training: loss rel {lerr:.3e}, cosine {cos:.5f}, worst tensor {rel[-1]:.3e}, median {rel[len(rel) // 2]:.3e}")
    assert cos >= min_cos and rel[-1] <= worst_tol and rel[len(rel) // 2] <= median_tol, (cos, rel[-1], rel[len(rel) // 2])
    # the same mode on a golden case: losses and total gradient norm against the reference's
    ci = 1
    B, N, T, L = [int(v) for v in full_golden["cases"][ci]]
    g = case_dict(full_golden, ci)
    m.precision = mode
    try:
        with tuned(train_split_min_rows=0):
            _, loss3, _ = train_step_grads(m, cfg, B, N, T, L, 200 + ci)
            gnd = m.get_grad_norm_dict()
    finally:
        m.precision = "f32"
    gref = dict(zip([str(k) for k in g["grad_norm_keys"]], g["grad_norm_vals"]))
    print(f"{mode}-operand training, golden case {ci}: loss {loss3.detach().cpu().numpy()} vs {g['loss']}, total gradient norm "
          f"{gnd['total_grad_norm']:.5f} vs {gref['total_grad_norm']:.5f}")
    np.testing.assert_allclose(loss3.detach().cpu().numpy().astype(np.float64), g["loss"], rtol=l_rtol, atol=1e-3)
    assert gnd["total_grad_norm"] == pytest.approx(gref["total_grad_norm"], rel=norm_rtol)


# (min cosine, worst tensor, median tensor) on weights whose first softmax is NOT saturated - measured values in the test's docstring
LOWP_TRAIN_TOL_UNSATURATED = {"f16": (0.9993, 0.055, 6e-4), "bf16": (0.994, 0.16, 4e-3)}


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_16_bit_operand_training_on_weights_with_an_unsaturated_softmax(mode):
    """VERDICT r3 item 6 / weak point 7: the bounds of LOWP_TRAIN_TOL are measured at random-init weights, where the first inter-object
    softmax is saturated (scores of rms ~100) and 2^-8 / 2^-11 operand noise flips near-ties.  Here the projection matrices are
    scaled by 1/64 (synth.make_state_dict_variant "lin_div64": attention scores x 1/4096, a nearly uniform softmax) - the regime of a
    network whose attention is not an arg-max - and the 16-bit operand steps are held to much tighter bounds against the exact-f32 step
    (measured, round 4: f16 cosine 0.99950, worst tensor 4.5 %, median 0.038 %; bf16 0.99522, 13.7 %, 0.29 %; at random init 0.985 / 0.744)."""
    cfg = synth.DEFAULT_MODEL_CFG
    m = LanguageAlignedTrackSelectionModule(cfg)
    sd = synth.make_state_dict_variant(cfg, 42, "lin_div64")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    min_cos, worst_tol, median_tol = LOWP_TRAIN_TOL_UNSATURATED[mode]
    grads, losses = {}, {}
    for prec in ("f32", mode):
        m.precision = prec
        _, l3, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)  # 1280 token rows: above the size gate
        grads[prec] = {k: v.double().clone() for k, v in g.items()}
        losses[prec] = l3.detach().cpu().numpy().astype(np.float64)
    ref = grads["f32"]
    total = math.sqrt(sum(float(v.pow(2).sum()) for v in ref.values()))
    n16 = math.sqrt(sum(float(v.pow(2).sum()) for v in grads[mode].values()))
    cos = sum(float((grads[mode][k] * ref[k]).sum()) for k in ref) / (total * n16)
    rel = sorted(float((grads[mode][k] - ref[k]).norm()) / (float(ref[k].norm()) + 1e-5 * total) for k in ref)
    lerr = float(np.abs(losses[mode] / losses["f32"] - 1).max())
    print(f"{mode}-operand training, lin_div64 weights: loss rel {lerr:.3e}, cosine {cos:.6f}, worst tensor {rel[-1]:.3e}, median {rel[len(rel) // 2]:.3e}")
    assert lerr <= 5e-3
    assert cos >= min_cos and rel[-1] <= worst_tol and rel[len(rel) // 2] <= median_tol, (cos, rel[-1], rel[len(rel) // 2])


@pytest.mark.parametrize("mode", ["f16x3", "f16", "bf16"])
def test_kept_operand_casts_give_the_same_gradients_bit_for_bit(full_model, mode):
    """Reduced-precision training modes (in "f16x3" the split operand casts write their hi halves once more as plain f16 rows - the dW
    products' operands): the forward keeps its fixed-scale operand casts in a ctx-owned arena and the backward's weight-gradient
    products read them (sola_tune "train_x16_keep", default 1) instead of casting the same f32 activations again - the same 16-bit
    values either way, so every gradient must be bit-identical with the switch off.  The arena is sized from the previous step's
    need: the SECOND step is the one that reuses the casts.  Dropout off (eval mode): the two runs see the same step.  (Round 6: the bf16
    step's bfloat16 pre-norm rows read their residual from the kept casts, so that part of the storage mode - sola_tune "train_bf16_store" 2 -
    exists only with the arena; this A/B of the arena runs at level 1.)"""
    with tuned(train_bf16_store=1):
        _kept_casts_checks(full_model, mode)


def _kept_casts_checks(full_model, mode):
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    got = {}
    try:
        m.precision = mode
        for keep in (1, 0):
            with tuned(train_x16_keep=keep):
                for _ in range(2):
                    _, l3, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)
            got[keep] = ({k: v.clone() for k, v in g.items()}, l3.detach().clone())
    finally:
        m.precision = "f32"
    assert torch.equal(got[1][1], got[0][1])
    bad = [k for k in got[1][0] if not torch.equal(got[1][0][k], got[0][0][k])]
    assert not bad, bad
    # the same with dropout ON (train mode, the masks re-seeded per step): the kept casts are the casts of the POST-dropout
    # activations, which is what the backward's own cast of the stored f32 activations reads
    got = {}
    try:
        m.train()
        m.precision = mode
        for keep in (1, 0):
            with tuned(train_x16_keep=keep):
                for _ in range(2):
                    torch.manual_seed(7)
                    _, l3, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)
            got[keep] = ({k: v.clone() for k, v in g.items()}, l3.detach().clone())
    finally:
        m.eval()
        m.precision = "f32"
    assert torch.equal(got[1][1], got[0][1])
    bad = [k for k in got[1][0] if not torch.equal(got[1][0][k], got[0][0][k])]
    assert not bad, bad


def test_bf16_statistics_pass_that_is_the_cast_gives_the_same_gradients_bit_for_bit(full_model):
    """Round 5, bf16 storage: bfloat16 has f32's exponent range, so the backward's pass over a gradient matrix (bias sums) also writes
    its UNSCALED bf16 cast - no max|x| in front, no second read by the casts of the dW / dX GEMMs (sola_tune "bwd_fused_bf16_cast",
    default 1).  The two-pass path scales by a power of two before rounding and undoes it behind the f32 accumulation: the same
    products, so every gradient must keep its bits with the switch off.  (Round 6: with the step's bf16 STORAGE on, the producers write the
    bfloat16 rows themselves and the bias sums are taken from those rounded rows - as autocast's grad_output.sum(0) is - so this A/B of
    the pass runs with sola_tune "train_bf16_store" 0.)
    The third setting, sola_tune "bwd_dual_cast" 0, is the same step once more without any row-major cast left behind for the dX GEMMs
    (neither by the statistics pass nor by the weight gradients' transposing cast): they cast the gradient matrix themselves, with the
    same scale - the same 16-bit values, so the same bits again."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    got = {}
    try:
        m.precision = "bf16"
        for fused, dual in ((1, 1), (0, 1), (1, 0)):
            with tuned(train_bf16_store=0, bwd_fused_bf16_cast=fused, bwd_dual_cast=dual):
                _, l3, g = train_step_grads(m, cfg, 8, 40, 32, 10, 77)
            got[fused, dual] = ({k: v.clone() for k, v in g.items()}, l3.detach().clone())
    finally:
        m.precision = "f32"
    for other in ((0, 1), (1, 0)):
        assert torch.equal(got[1, 1][1], got[other][1]), other
        bad = [k for k in got[1, 1][0] if not torch.equal(got[1, 1][0][k], got[other][0][k])]
        assert not bad, (other, bad)


@pytest.mark.parametrize("fused", [True, False])
def test_training_run_tracks_exact_f32_across_optimizer_steps(fused):
    """Several optimizer steps, not one: the reduced-precision modes keep derived copies of the weights (split-f16 / f16
    projection matrices + scales) that must follow every update.  torch.optim.AdamW(fused=True) changes the parameters
    without bumping Tensor._version - a run that trusted the version counter used the INITIAL projection weights in every
    forward and diverged (loss 8 -> 70 in 50 steps where exact f32 reached 1.0; profiles/r02_train_converge.log is the fixed
    behaviour).  12 steps each: the eval-mode exact-f32 loss of every mode must have dropped by a third and end within 15 %
    of the exact-f32 run's."""
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = 8, 40, 32, 10  # 1280 token rows: above the size gate of the split kernels
    sd = synth.make_state_dict(cfg, 42)
    batches = [{k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, B, N, T, L, 700 + i).items()} for i in range(2)]

    def loss_of(m, inp):
        sm, st = m(inp["object_tokens"], inp["lang_tokens"])
        neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
        return track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)

    def eval_loss(m):
        m.eval(); m.precision = "f32"
        with torch.no_grad():
            return sum(float(loss_of(m, b)[0]) for b in batches) / len(batches)

    final = {}
    for prec in ("f32", "f16x3", "f16", "bf16"):
        m = LanguageAlignedTrackSelectionModule(cfg)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m = m.cuda()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, fused=fused)
        start = eval_loss(m)
        torch.manual_seed(5)  # the dropout seeds of the steps
        for it in range(12):
            m.train(); m.precision = prec
            opt.zero_grad(set_to_none=True)
            loss_of(m, batches[it % 2])[0].backward()
            m.clip_grad_norm_(1.0)
            opt.step()
        final[prec] = eval_loss(m)
        assert final[prec] < 0.67 * start, (prec, start, final[prec])
        del m, opt
    print("eval-mode exact-f32 loss after 12 steps:", final)
    for prec in ("f16x3", "f16", "bf16"):
        assert abs(final[prec] - final["f32"]) <= 0.15 * final["f32"], final


def test_small_gradients_vs_oracle_autograd(small_model):
    """Every parameter gradient against float64 autograd through the oracle on a case with no fixture."""
    m, sd = small_model
    cfg = synth.SMALL_MODEL_CFG
    B, N, T, L = 2, 6, 24, 7
    inp, loss3, grads = train_step_grads(m, cfg, B, N, T, L, 4242)
    tsd = {k: t64(v, True) for k, v in sd.items()}
    sm, st = _oracle_forward_grad(tsd, cfg, inp)
    neg = tsd["negative_token.weight"].unsqueeze(0).expand(B, -1, -1)
    ls = sola_oracle.losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W, dtype=torch.float64)
    ls["total"].backward()
    assert abs(float(loss3[0].detach()) - float(ls["total"].detach())) < 2e-4
    gmax = max(float(t.grad.abs().max()) for t in tsd.values() if t.grad is not None)
    for k, gr in grads.items():
        ref = tsd[k].grad.numpy()
        err = float(np.abs(gr.cpu().double().numpy() - ref).max())
        assert err <= 1e-3 * float(np.abs(ref).max()) + 1e-6 * gmax, (k, err, float(np.abs(ref).max()))


def _oracle_forward_grad(tsd, cfg, inp):
    """sola_oracle.forward without the detach of to_torch_state, so autograd reaches the weights."""
    obj = t64(inp["object_tokens"])
    lang = t64(inp["lang_tokens"])
    B = obj.shape[0]
    x = sola_oracle.encoder(tsd, cfg, obj)
    pe = sola_oracle.positional_encoding(tsd, cfg, x.shape[2], torch.float64)
    lang = torch.cat([lang, tsd["negative_token.weight"].unsqueeze(0).expand(B, -1, -1)], dim=1)
    for layer in range(cfg["n_layers"]):
        x = sola_oracle.align_layer(tsd, cfg, layer, x, pe, lang)
    logits = torch.einsum("bntd,bwd->bntw", x, lang).mean(dim=-1)
    a = torch.softmax(logits, dim=-1)
    tok = (x * a.unsqueeze(-1)).sum(dim=2)
    return torch.einsum("bnd,bwd->bnw", tok, lang).mean(dim=-1), tok


def test_grad_norm_dict_and_clip_match_torch(small_model):
    """get_grad_norm_dict / clip_grad_norm_ run as multi-tensor HIP launches: same numbers as the per-parameter torch
    formulation of module/module.py:164-199 and torch.nn.utils.clip_grad_norm_ (train.py:121-122)."""
    m, _ = small_model
    cfg = synth.SMALL_MODEL_CFG
    train_step_grads(m, cfg, 2, 6, 24, 7, 9)
    ref_groups = {"short_motion_encoder": list(m.short_motion_encoder.parameters()), "negative_token": list(m.negative_token.parameters())}
    for i, layer in enumerate(m.object_lang_align_layers):
        ref_groups[f"scmola_layer_{i}"] = list(layer.parameters())
    ref = {k: math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps)) for k, ps in ref_groups.items()}
    ref["total_grad_norm"] = math.sqrt(sum(v * v for v in ref.values()))
    got = m.get_grad_norm_dict()
    assert set(got) == set(ref)
    for k in ref:
        assert got[k] == pytest.approx(ref[k], rel=1e-6), k
    before = {k: p.grad.clone() for k, p in m.named_parameters()}
    max_norm = 0.37 * ref["total_grad_norm"]
    m.clip_grad_norm_(max_norm)
    coef = max_norm / (ref["total_grad_norm"] + 1e-6)
    for k, p in m.named_parameters():
        assert torch.allclose(p.grad, before[k] * coef, rtol=1e-6, atol=0)
    assert m.get_grad_norm_dict()["total_grad_norm"] == pytest.approx(max_norm, rel=1e-5)
    m.clip_grad_norm_(10 * max_norm)  # below the threshold: untouched
    for k, p in m.named_parameters():
        assert torch.allclose(p.grad, before[k] * coef, rtol=1e-6, atol=0)


def test_side_stream_weight_gradients_are_bit_identical(full_model):
    """Round 4: in the few-sample exact-f32 backward (the reference's batch size of 1) the weight-gradient products run on a side stream
    beside the dX chain (sola_tune "bwd_side_rows").  Same kernels in the same per-gradient order: all 83 gradients, the losses and a
    second step's gradients must equal the single-stream run bit for bit."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    out = {}
    for rows in (0, 4096):  # 0 is the default (off: the lane costs the host more than it saves)
        with tuned(bwd_group_rows=0, bwd_side_rows=rows):  # the side lane runs the per-matrix slab form: compare like with like
            res = []
            for seed in (5, 6):
                _, l3, g = train_step_grads(m, cfg, 1, 64, 32, 16, seed)
                res.append((l3.detach().clone(), {k: v.clone() for k, v in g.items()}))
        out[rows] = res
    for (la, ga), (lb, gb) in zip(out[0], out[4096]):
        assert torch.equal(la, lb)
        assert set(ga) == set(gb) and len(ga) == 83
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("shape", [(1, 64, 32, 16), (1, 80, 100, 24), (2, 17, 40, 5), (3, 64, 32, 16)])
def test_grouped_few_sample_weight_gradients_equal_the_slab_form(full_model, shape):
    """Round 4 (sola_tune "bwd_group_rows", default 2048 token rows): a few-sample exact-f32 backward defers the 12 weight-gradient products
    of every layer's linear maps and runs them in ONE grouped launch (every dY in a buffer of its own until then; each block reduces over
    all rows of its problem), and - round 5 - reads the weights of its dX GEMMs where they lie (sola_gemm_nn's form: no transposed copies).  Against the per-matrix slab form (0): the same
    losses, the gradients nothing was deferred for bit for bit, the deferred ones (and what flows from the same dX chain: identical) within
    f32 summation-order noise - 2e-6 of each tensor's norm - and twice in a row the same bits (fixed order, no atomics)."""
    m, _ = full_model
    cfg = synth.DEFAULT_MODEL_CFG
    B, N, T, L = shape
    out = {}
    for rows in (0, 2048, -2048):  # -2048: the grouped form once more (repeatability)
        with tuned(bwd_group_rows=abs(rows)):
            _, l3, g = train_step_grads(m, cfg, B, N, T, L, 11)
        out[rows] = (l3.detach().clone(), {k: v.clone() for k, v in g.items()})
    (l0, g0), (l1, g1), (l2, g2) = out[0], out[2048], out[-2048]
    assert torch.equal(l0, l1) and torch.equal(l1, l2)
    assert set(g0) == set(g1) and len(g0) == 83
    worst = (0.0, "")
    total = float(torch.sqrt(sum((v.double() ** 2).sum() for v in g0.values())))
    for k in g0:
        assert torch.equal(g1[k], g2[k]), k
        # round 5: the grouped form also takes the encoder's input gradients as z = dY W + a tap gather (the weights read where they lie)
        # where the slab form of a uniform batch runs the transposed-conv gather: everything in the encoder is summation-order noise apart
        deferred = ("object_lang_align_layers" in k and "_proj." in k) or "short_motion_encoder" in k
        if not deferred:
            assert torch.equal(g0[k], g1[k]), k  # the layers' norms, negative tokens: their dX chain is the same arithmetic (the row-major
                                                 # weight form multiplies the same products in the same order as the transposed copy)
        # (the k-projection biases have a zero gradient in exact arithmetic - a constant added to every score of a query leaves its
        # softmax unchanged: what they hold is rounding noise, measured against the whole gradient)
        err = float((g0[k].double() - g1[k].double()).norm()) / (float(g0[k].double().norm()) + 1e-4 * total)
        worst = max(worst, (err, k))
    print("grouped vs slab weight gradients, worst tensor:", worst)
    assert worst[0] < 2e-6, worst


@pytest.mark.parametrize("train_mode", [False, True])
@pytest.mark.parametrize("shape", [(1, 64, 32, 16), (1, 21, 77, 9), (3, 16, 32, 12)])
def test_train_step_call_equals_the_autograd_path(shape, train_mode):
    """Round 5 (sola_train_step / module.train_step): the body of the training loop as ONE library call - forward, losses on the module's own
    negative tokens, backward, gradient norms, clipping, enqueued from C++ - against the call-by-call path through autograd
    (module(...) + track_selection_losses + .backward() + clip_grad_norm_), dropout on (the same seeds) and off.  One sample per step (the
    reference's batch size, configs/mevis/default.yaml:37): the same kernels with the same arguments in the same order - losses, every
    gradient, the norm dict and, after three clipped AdamW steps, every weight are BIT-identical.  Batches of several samples: the
    per-sample negative-token gradients are summed by torch there (repeat's backward) and by the library here - same values at 1e-6."""
    B, N, T, L = shape
    cfg = synth.DEFAULT_MODEL_CFG
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, B, N, T, L, 123).items()}
    models, opts, outs = [], [], []
    for _ in range(2):
        m, _sd = build(cfg)
        m.train(train_mode)
        m.precision = "f32"
        models.append(m)
        opts.append(torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True))
    for step in range(3):
        # (a) call by call through autograd
        m, opt = models[0], opts[0]
        torch.manual_seed(1000 + step)  # the step's dropout seed comes from torch's CPU generator
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            sm, st = m(inp["object_tokens"], inp["lang_tokens"])
            neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
            la = track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)
            la[0].backward()
        norms_a = m.get_grad_norm_dict()
        m.clip_grad_norm_(1.0)
        ga = {k: p.grad.clone() for k, p in m._params()}
        opt.step()
        # (b) one call
        m2, opt2 = models[1], opts[1]
        torch.manual_seed(1000 + step)
        lb, sm2, st2 = m2.train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0)
        norms_b = m2.step_grad_norm_dict()
        gb = {k: p.grad.clone() for k, p in m2._params()}
        opt2.step()
        torch.cuda.synchronize()
        assert torch.equal(sm, sm2) and torch.equal(st, st2) and torch.equal(la, lb), step
        if B == 1:
            for k in ga:
                assert torch.equal(ga[k], gb[k]), (step, k)
            assert norms_a == norms_b, (norms_a, norms_b)
        else:
            for k in ga:
                d = float((ga[k] - gb[k]).abs().max())
                assert d <= 1e-6 * max(1e-12, float(ga[k].abs().max())) + 1e-12, (step, k, d)
            for k in norms_a:
                assert abs(norms_a[k] - norms_b[k]) <= 1e-6 * max(norms_a[k], 1e-12), k
    if B == 1:
        for (k, p), (_k2, p2) in zip(models[0]._params(), models[1]._params()):
            assert torch.equal(p.detach(), p2.detach()), k


@pytest.mark.parametrize("max_norm", [0.0, 1.0, 1e-3])
def test_fused_clip_adamw_equals_torch(max_norm):
    """Round 5 (sola_adamw_step, module.train_step(optimizer=...)): gradient clipping + the AdamW update as ONE multi-tensor launch with torch's
    fused arithmetic (double scalars, float tensors, the expressions of ATen/native/cuda/fused_adam_utils.cuh) against
    module.train_step + torch.optim.AdamW(fused=True).step(): after four steps (weight decay on; clipping off, rarely active, always active)
    every parameter, both moments, the step counters and the gradients left in .grad are BIT-identical."""
    cfg = synth.DEFAULT_MODEL_CFG
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 1, 64, 32, 16, 5).items()}
    ms, opts = [], []
    for _ in range(2):
        m, _sd = build(cfg)
        m.train(True)
        m.precision = "f32"
        ms.append(m)
        opts.append(torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=0.05, betas=(0.9, 0.98), fused=True))
    for step in range(4):
        torch.manual_seed(77 + step)
        ms[0].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=max_norm)
        opts[0].step()
        torch.manual_seed(77 + step)
        ms[1].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=max_norm, optimizer=opts[1])
        torch.cuda.synchronize()
        for (k, p), (_k, q) in zip(ms[0]._params(), ms[1]._params()):
            assert torch.equal(p.detach(), q.detach()), (step, k, "parameter")
            assert torch.equal(p.grad, q.grad), (step, k, "gradient")
            sa, sb = opts[0].state[p], opts[1].state[q]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (step, k, "moments")
            assert float(sa["step"]) == float(sb["step"]) == step + 1, (step, k)


def test_fused_adamw_mixed_with_torch_steps_keeps_the_step_count():
    """the update's number is read from the optimizer's DEVICE step tensors, so torch's own optimizer.step() interleaved with
    module.train_step(optimizer=...) on the same optimizer - and a load_state_dict into it - cannot leave a stale count behind: model 1
    alternates the two paths (fused, torch, fused, torch, fused), model 0 takes torch's step every time; parameters, moments and step
    counters stay bit-identical, and a state dict loaded at step 5 (counters = 2) is continued from 2 by the fused path."""
    cfg = synth.DEFAULT_MODEL_CFG
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 1, 16, 32, 16, 5).items()}
    ms, opts = [], []
    for _ in range(2):
        m, _sd = build(cfg)
        m.train(True)
        m.precision = "f32"
        ms.append(m)
        opts.append(torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=0.05, fused=True))
    saved = None
    for step in range(5):
        torch.manual_seed(91 + step)
        ms[0].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0)
        opts[0].step()
        torch.manual_seed(91 + step)
        if step % 2 == 0:
            ms[1].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0, optimizer=opts[1])
        else:
            ms[1].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0)
            opts[1].step()
            ms[1].weights_changed()
        torch.cuda.synchronize()
        for (k, p), (_k, q) in zip(ms[0]._params(), ms[1]._params()):
            assert torch.equal(p.detach(), q.detach()), (step, k, "parameter")
            sa, sb = opts[0].state[p], opts[1].state[q]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (step, k, "moments")
            assert float(sa["step"]) == float(sb["step"]) == step + 1, (step, k)
        if step == 1:
            import copy
            saved = [copy.deepcopy(o.state_dict()) for o in opts], [copy.deepcopy(m.state_dict()) for m in ms]
    # rewind both to step 2 through load_state_dict, then one more step each way
    for m, o, osd, msd in zip(ms, opts, saved[0], saved[1]):
        m.load_state_dict(msd)
        o.load_state_dict(osd)
    torch.manual_seed(5)
    ms[0].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0)
    opts[0].step()
    torch.manual_seed(5)
    ms[1].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1.0, optimizer=opts[1])
    torch.cuda.synchronize()
    for (k, p), (_k, q) in zip(ms[0]._params(), ms[1]._params()):
        assert torch.equal(p.detach(), q.detach()), (k, "parameter after load_state_dict")
        assert float(opts[0].state[p]["step"]) == float(opts[1].state[q]["step"]) == 3, k


def test_grad_norm_groups_beyond_sixteen():
    """the per-group fold takes 16 groups per launch; more (a configuration with > 14 layers) run as several launches - checked on
    the multi-tensor entry point with 40 groups against float64 sums, the total in group order."""
    torch.manual_seed(3)
    tensors = [torch.randn(n, device="cuda") for n in (5, 4096, 4097, 70000) * 10]
    gids = list(range(40))
    m, _sd = build(synth.SMALL_MODEL_CFG)
    sq = m._grad_sqnorms(tensors, gids, 40).cpu()
    ref = torch.tensor([float((t.double() ** 2).sum()) for t in tensors], dtype=torch.float64)
    assert torch.allclose(sq[:40], ref, rtol=1e-6)
    tot = 0.0
    for v in sq[:40].tolist():
        tot += v
    assert float(sq[40]) == tot


def test_fused_clip_adamw_without_gradient_write_back():
    """sola_adamw_step(write_back_grads = 0) - what train.py and the bench's one-sample step pass: with the clip ACTIVE the parameters and
    both moments are bit-identical to the write-back form (and so to torch's), and .grad keeps the UNCLIPPED gradient."""
    cfg = synth.DEFAULT_MODEL_CFG
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, 1, 64, 32, 16, 5).items()}
    ms, opts = [], []
    for _ in range(2):
        m, _sd = build(cfg)
        m.train(True)
        m.precision = "f32"
        ms.append(m)
        opts.append(torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=0.05, fused=True))
    for step in range(3):
        for j, wb in enumerate((True, False)):
            torch.manual_seed(31 + step)
            ms[j].train_step(inp["object_tokens"], inp["lang_tokens"], inp["labels"], inp["pos_tokens"], POS_W, TEMP, ALIGN_W, max_grad_norm=1e-3,
                             optimizer=opts[j], write_back_grads=wb)
        torch.cuda.synchronize()
        scale = None
        for (k, p), (_k, q) in zip(ms[0]._params(), ms[1]._params()):
            assert torch.equal(p.detach(), q.detach()), (step, k, "parameter")
            sa, sb = opts[0].state[p], opts[1].state[q]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (step, k, "moments")
            if float(q.grad.abs().max()) > 0:
                assert not torch.equal(p.grad, q.grad), (step, k)  # clipped against unclipped
                if scale is None:
                    i = int(q.grad.abs().argmax())
                    scale = float(p.grad.flatten()[i] / q.grad.flatten()[i])
        assert scale is not None and 0.0 < scale < 1.0


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_optimizer_step_after_an_autograd_backward_equals_torch(max_norm):
    """module.optimizer_step(optimizer, max_grad_norm) - clip + AdamW as one launch behind a backward that went through autograd (uniform
    batch of three samples; negative_token.weight's gradient is accumulated by autograd from two contributions) - against
    clip_grad_norm_ + torch's fused AdamW: bit-identical parameters after three steps."""
    cfg = synth.DEFAULT_MODEL_CFG
    B = 3
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.make_inputs(cfg, B, 16, 32, 12, 9).items()}
    ms, opts = [], []
    for _ in range(2):
        m, _sd = build(cfg)
        m.precision = "f32"
        ms.append(m)
        opts.append(torch.optim.AdamW(m.parameters(), lr=2e-4, fused=True))
    for step in range(3):
        for i, (m, opt) in enumerate(zip(ms, opts)):
            opt.zero_grad(set_to_none=True)
            with torch.enable_grad():
                sm, st = m(inp["object_tokens"], inp["lang_tokens"])
                neg = m.negative_token.weight.clone().unsqueeze(0).repeat(B, 1, 1)
                track_selection_losses(sm, st, inp["labels"], inp["pos_tokens"], neg, POS_W, TEMP, ALIGN_W)[0].backward()
            if i == 0:
                if max_norm > 0:
                    m.clip_grad_norm_(max_norm)
                opt.step()
            else:
                m.optimizer_step(opt, max_norm)
        torch.cuda.synchronize()
        for (k, p), (_k, q) in zip(ms[0]._params(), ms[1]._params()):
            assert torch.equal(p.detach(), q.detach()), (step, k)
