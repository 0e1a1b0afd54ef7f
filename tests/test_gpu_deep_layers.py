"""A model of more than ten alignment layers through the split-f16 training forward: every layer must multiply by its OWN 16-bit copies of
the projection weights and their inverse scales (ctx.h: lin16_weight, SolaCtx::lin_inv_scale - addressed by (layer, site, projection)).

Model: synth.SMALL_MODEL_CFG with n_layers = 11, dropout off, the "lin_div64" weights.  Its 32 / 128 channels are whole k-tiles of the
split-f16 GEMMs (32), so with the row gate off every GEMM of the forward takes them - no wider object_token_dim is needed (the library's
launch counters: 83 launches in the split-f16 GEMM category, none in the f32 ones, against 83 f32 GEMM launches of the exact step).
Shape (B, N, T, L) = (4, 8, 32, 10).  One training forward in "f16x3"; yardstick: oracle/sola_oracle.py in float64, autograd-free.

Bar per output: max(1e-3 * max|score|, 8 * e32).  1e-3 of the largest entry is the project's bound for this arithmetic
(tests/test_gpu_fast.py); e32 is the largest absolute error of the EXACT-f32 training forward on the same model and inputs (it never read
the 16-bit copies) - 4x for 22-bit against 24-bit products, 2x margin.  Measured on an MI355X, largest absolute error against the oracle:

                                   score_map (max|ref| 1.0933e+01)   score_tokens (max|ref| 4.2206e+00)
  exact f32 (e32)                  6.6054e-06                        7.9332e-06
  f16x3, this library              3.8099e-06                        4.8165e-06
  f16x3, the library before it     4.4969e-03                        3.3288e-03    (layer 10 on layer 1's matrices and scales)
  bar  max(1e-3 max|ref|, 8 e32)   1.0933e-02                        4.2206e-03
  8 e32 alone                      5.2843e-05                        6.3466e-05

On these weights (every projection matrix divided by 64) a whole layer on another layer's matrices moves the scores by 4e-4 / 8e-4 of their
largest entry only: three orders of magnitude above the sound step, but BELOW the project's 1e-3 bound, whose term decides the bar.  The
first test - the bar as stated - therefore passes with the library from before the fix too.  The second test holds the same forward to
8 * e32 alone, the bar's own statement of the arithmetic's class (the split-f16 step measures 0.6 e32): the library from before the fix
misses it by 85x / 52x, this one is 13x inside.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sola_oracle  # noqa: E402
from sola_amd import synth  # noqa: E402
from sola_amd._lib import tuned  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

CFG = dict(synth.SMALL_MODEL_CFG, n_layers=11, dropout_p=0.0)
SHAPE = (4, 8, 32, 10)
E32 = {"score_map": 6.6054e-06, "score_tokens": 7.9332e-06}  # the exact-f32 training forward against the oracle (module docstring)


def forward_errors(mode):
    """one training forward in `mode` -> {output: (largest absolute error against the float64 oracle, largest reference entry)}"""
    sd = synth.make_state_dict_variant(CFG, 42, "lin_div64")
    inp = synth.make_inputs(CFG, *SHAPE, 77)
    with torch.no_grad():
        ref = sola_oracle.forward(sd, CFG, inp["object_tokens"], inp["lang_tokens"], dtype=torch.float64)
    m = LanguageAlignedTrackSelectionModule(CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()  # eval(): dropout off; the parameters still ask for gradients, so this is the TRAINING forward
    m.precision = mode
    with tuned(train_split_min_rows=0):  # the batch is below the production size gate of the reduced-precision training GEMMs
        got = m(torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda())
    torch.cuda.synchronize()
    assert got[0].requires_grad, "not the training forward"
    out = {}
    for name, g, r in zip(("score_map", "score_tokens"), got, ref):
        r = np.asarray(r, dtype=np.float64)
        out[name] = (float(np.abs(g.detach().cpu().double().numpy() - r).max()), float(np.abs(r).max()))
    return out


@pytest.fixture(scope="module")
def f16x3_errors():
    return forward_errors("f16x3")


def test_f16x3_training_forward_of_eleven_layers_against_the_oracle(f16x3_errors):
    """the bar as first stated for this model, max(1e-3 max|ref|, 8 e32): the project's bound for the arithmetic.  NOT the regression guard -
    a library that runs layer 10 on layer 1's matrices stays inside it on these weights (module docstring); the test below is the guard"""
    for name, (err, top) in f16x3_errors.items():
        bar = max(1e-3 * top, 8 * E32[name])
        print(f"deep: f16x3 {name}: max|err| {err:.3e}, max|ref| {top:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


def test_f16x3_training_forward_of_eleven_layers_stays_in_the_exact_step_s_error_class(f16x3_errors):
    """8 * e32 without the 1e-3 term: what tells layer 10's own matrices from layer 1's on these weights (module docstring)"""
    for name, (err, top) in f16x3_errors.items():
        print(f"deep: f16x3 {name}: max|err| {err:.3e}, 8 e32 {8 * E32[name]:.3e}")
        assert err <= 8 * E32[name], (name, err, 8 * E32[name])
