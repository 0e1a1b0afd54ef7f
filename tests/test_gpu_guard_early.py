"""The range guard of the 16-bit inference modes is read back BEHIND THE LAST LAUNCH THAT CAN SET IT, not behind the whole
sequence (sola_amd/csrc/forward_infer.hip: InferBuilder::read_guard; profiles/step_boundary.txt lists the launches per mode):
the call returns while its tail is still queued, and the exact-f32 repeat of a tripped call is enqueued behind that tail.

What must hold, uniform and ragged, "f16x3" (split-f16) and "f16" (16-bit storage):
* a value that leaves the f16 range at the LAST guarded launch of the mode - the last layer's object -> language attention
  under "f16x3" (a v_proj bias channel at 1e5: the attention's split-pair output overflows), the out-projection behind it under
  "f16" (an out_proj bias channel at 1e5: its f16 rows overflow) - is still seen: one fallback, outputs bit-equal to the
  exact-f32 model's;
* so is one at the FIRST guarded launch ("f16": conv0's f16 rows; "f16x3": the first encoder norm's split pairs - which only
  its own beta can push out of range, so the weight-time bit is set with it), and the weight-time bit alone (GroupNorm
  weights x3000);
* with the guard switched off the call returns the 16-bit result and counts nothing;
* a clean call reports (0, 0).

Shapes: the reduced model configuration, and the smallest batches whose B*N*T exceeds infer_f32_rows (4096 object-token rows,
below which an "f16x3" call runs the exact-f32 kernels and never consults the guard).  "f16" needs object_token_dim % 64 == 0:
its cases widen the reduced configuration's 32 to 64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sola_amd import synth  # noqa: E402
from sola_amd.module import LanguageAlignedTrackSelectionModule  # noqa: E402

CFGS = {"f16x3": synth.SMALL_MODEL_CFG, "f16": dict(synth.SMALL_MODEL_CFG, object_token_dim=64)}
UNIFORM = (2, 33, 63, 5)                      # B, N, T, L: 4158 rows
RAGGED = ([(33, 63), (20, 104)], [5, 3, 7], [0, 1, 1])  # (N_v, T_v) per video: 4159 rows; L per sample; the sample's video
LAST = 1  # n_layers - 1


def build(cfg, precision, edit=None, variant="base"):
    m = LanguageAlignedTrackSelectionModule(cfg)
    sd = synth.make_state_dict_variant(cfg, 42, variant)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    m.precision = precision
    if edit is not None:
        with torch.no_grad():
            edit(m)
    return m


def last_attention_value(m):   # "f16x3": the attention output (split pairs) is the last guarded write
    m.object_lang_align_layers[LAST].object2lang_attn.v_proj.bias[3] = 1.0e5


def last_out_projection(m):    # "f16": the out-projection's f16 rows are the last guarded write
    m.object_lang_align_layers[LAST].object2lang_attn.out_proj.bias[3] = 1.0e5


def first_conv(m):             # "f16": conv0 writes f16 rows in the scaled units of the tokens
    m.short_motion_encoder[0].bias[3] = 1.0e5


def first_norm(m):             # "f16x3": the first encoder norm writes the first split pairs
    m.short_motion_encoder[1].bias[3] = 1.0e5


def run(m, cfg, ragged):
    """-> (score_map, score_tokens) as numpy, flat over the samples"""
    with torch.no_grad():
        if not ragged:
            B, N, T, L = UNIFORM
            inp = synth.make_inputs(cfg, B, N, T, L, seed=300)
            sm, st = m(torch.from_numpy(inp["object_tokens"]).cuda(), torch.from_numpy(inp["lang_tokens"]).cuda())
        else:
            shapes, lens, sample_video = RAGGED
            rng = np.random.Generator(np.random.PCG64(301))
            videos = [torch.from_numpy(rng.standard_normal(size=(n, t, cfg["object_token_dim"])).astype(np.float32)).cuda() for n, t in shapes]
            texts = [torch.from_numpy(rng.standard_normal(size=(l, cfg["lang_token_dim"])).astype(np.float32)).cuda() for l in lens]
            m.forward_ragged(videos, texts, sample_video)
            sm, st = m.last_ragged[0], m.last_ragged[1]
        # no synchronisation here: the copy below is ordered behind the call's tail (and behind the exact-f32 repeat) by the stream alone
        return sm.cpu().numpy(), st.cpu().numpy()


def check_trip(precision, ragged, edit, bits_want, variant="base"):
    cfg = CFGS[precision]
    m = build(cfg, precision, edit, variant)
    sm, st = run(m, cfg, ragged)
    n, bits = m.split_fallbacks()
    assert n == 1 and (bits & bits_want) == bits_want, (n, bits)
    sm32, st32 = run(build(cfg, "f32", edit, variant), cfg, ragged)
    assert np.isfinite(sm32).all() and np.isfinite(st32).all()
    np.testing.assert_array_equal(sm, sm32)
    np.testing.assert_array_equal(st, st32)
    return m, sm


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_trip_at_the_last_guarded_launch_is_seen_and_repeated_in_f32(precision, ragged):
    edit = last_attention_value if precision == "f16x3" else last_out_projection
    m, sm = check_trip(precision, ragged, edit, 1)
    # guard off: the call hands back the 16-bit result (it really was out of range) and counts nothing
    m.split_guard = False
    sm_u, _ = run(m, CFGS[precision], ragged)
    assert m.split_fallbacks()[0] == 1
    assert not np.isfinite(sm_u).all() or np.abs(sm_u - sm).max() > 0


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_f16_storage_value_of_the_attention_trips_too(ragged):
    """the issue's example on the 16-bit storage mode: there the v projection's own f16 rows overflow, ahead of the attention"""
    check_trip("f16", ragged, last_attention_value, 1)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_trip_at_the_first_guarded_launch(precision, ragged):
    if precision == "f16":
        check_trip(precision, ragged, first_conv, 1)
    else:
        check_trip(precision, ragged, first_norm, 3)  # beta at 1e5: the value bit and the weight-time bit


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_weight_time_bit_travels_in_the_same_copy(precision, ragged):
    check_trip(precision, ragged, None, 2, variant="gamma_x3000")


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_clean_call_reports_nothing_and_ran_the_16_bit_path(precision, ragged):
    cfg = CFGS[precision]
    m = build(cfg, precision)
    sm, st = run(m, cfg, ragged)
    assert m.split_fallbacks() == (0, 0)
    sm2, st2 = run(m, cfg, ragged)  # the second call clears and re-reads the words behind the first one's tail
    assert m.split_fallbacks() == (0, 0)
    np.testing.assert_array_equal(sm, sm2)
    np.testing.assert_array_equal(st, st2)
    _sm32, st32 = run(build(cfg, "f32"), cfg, ragged)
    assert np.isfinite(sm).all() and np.isfinite(st).all()
    assert np.abs(st - st32).max() > 0  # the 16-bit path itself ran (these rows exceed infer_f32_rows)
