"""sola_loss / sola_loss_ragged in every kernel shape of sola_amd/csrc/head.hip, against a float64 numpy statement of
tools/loss.py:29-56 with the loss assembly of train.py:98-113:

* D = 1024 and 512: the register kernels (a wave keeps the two rows it reduces, four waves = 8 rows per block);
  D = 128: the LDS row kernel they fall back to;
* n_neg = 32, 3 and 1; the negatives as one shared table and as one table per sample;
* uniform (B, N) = (2, 9), (1, 1), (3, 16): tail blocks of 1 row (one wave with a row) and a full block beside them;
  a ragged batch with 1, 8 and 17 tracks per sample (blocks of 1, 8 and 8 + 8 + 1 rows);
* (37, 64) = 2368 tracks: the mean's single block walks its eight-loads-in-flight loop and its remainder loop;
* n_neg = 2047: the most the register kernels take, with more than 64 KB of LDS.

Tolerance: the existing loss tests' own (tests/test_gpu_forward.py: rtol 2e-4 + atol 2e-4 on the three loss values).  The
hardest-negative index must equal the float64 one wherever the two largest negative logits differ by more than that tolerance."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sola_amd.loss import track_selection_losses, track_selection_losses_ragged  # noqa: E402

POS_W, TEMP, ALIGN_W = 1.5, 0.07, 0.3
RTOL = ATOL = 2e-4


def bce(x, y):
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def sample_terms(x, tok, y, pos, neg):
    """one sample in float64: x [N] logits, tok [N, D], y [N], pos [D], neg [n_neg, D] -> per-track terms and the negative logits"""
    s = math.exp(TEMP)
    pos_logit = tok @ pos * s
    neg_logit = tok @ neg.T * s                      # [N, n_neg]
    idx = neg_logit.argmax(axis=1)                   # first maximum
    neg_label = np.zeros_like(neg_logit)
    neg_label[np.arange(len(y)), idx] = 1.0 - y
    w = np.where(y > 0, POS_W, 1.0)
    return w * bce(x, y), bce(pos_logit, y), bce(neg_logit, neg_label), idx, neg_logit


def means(t0, t1, t2):
    b = t0.mean()
    a = POS_W * t1.mean() + t2.mean()
    return np.array([b + ALIGN_W * a, b, a])


def make(counts, D, n_neg, per_sample_neg, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    total, S = sum(counts), len(counts)
    x = rng.standard_normal(total).astype(np.float32) * 3
    tok = rng.standard_normal((total, D)).astype(np.float32)
    y = (rng.uniform(size=total) < 0.3).astype(np.float32)
    pos = (rng.standard_normal((S, D)) * 2 / math.sqrt(D)).astype(np.float32)   # logits of a few units
    neg = (rng.standard_normal((S if per_sample_neg else 1, n_neg, D)) * 2 / math.sqrt(D)).astype(np.float32)
    return x, tok, y, pos, neg


def reference(counts, x, tok, y, pos, neg):
    f = lambda a: a.astype(np.float64)
    out, o = [], 0
    for i, n in enumerate(counts):
        sl = slice(o, o + n)
        out.append(sample_terms(f(x[sl]), f(tok[sl]), f(y[sl]), f(pos[i]), f(neg[i if neg.shape[0] > 1 else 0])))
        o += n
    return out


def check_argmax(got, ref):
    for g, (_t0, _t1, _t2, idx, logit) in zip(got, ref):
        if logit.shape[1] == 1:
            assert (g == 0).all()
            continue
        top2 = np.sort(logit, axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > ATOL + RTOL * np.abs(top2[:, 1])
        assert clear.any()
        np.testing.assert_array_equal(g[clear], idx[clear])


def cuda(a):
    return torch.from_numpy(a).cuda()


def run_uniform(B, N, D, n_neg, per_sample_neg, seed):
    counts = [N] * B
    x, tok, y, pos, neg = make(counts, D, n_neg, per_sample_neg, seed)
    ref = reference(counts, x, tok, y, pos, neg)
    want = means(*[np.concatenate([r[k].reshape(-1) for r in ref]) for k in range(3)])
    with torch.no_grad():
        loss3, arg = track_selection_losses(cuda(x).view(B, N), cuda(tok).view(B, N, D), cuda(y).view(B, N), cuda(pos).view(B, 1, D),
                                            cuda(neg) if per_sample_neg else cuda(neg[0]), POS_W, TEMP, ALIGN_W, return_argmax=True)
    got = loss3.cpu().numpy().astype(np.float64)
    print(f"B {B} N {N} D {D} n_neg {n_neg}: loss {got} vs float64 {want}, |diff| {np.abs(got - want).max():.2e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    check_argmax(list(arg.cpu().numpy()), ref)


@pytest.mark.parametrize("per_sample_neg", [False, True], ids=["shared_neg", "per_sample_neg"])
@pytest.mark.parametrize("BN", [(2, 9), (1, 1), (3, 16)])
@pytest.mark.parametrize("n_neg", [32, 3, 1])
@pytest.mark.parametrize("D", [1024, 512, 128])
def test_uniform(D, n_neg, BN, per_sample_neg):
    run_uniform(BN[0], BN[1], D, n_neg, per_sample_neg, seed=D + 7 * n_neg + BN[1])


@pytest.mark.parametrize("per_sample_neg", [False, True], ids=["shared_neg", "per_sample_neg"])
@pytest.mark.parametrize("n_neg", [32, 3, 1])
@pytest.mark.parametrize("D", [1024, 512, 128])
def test_ragged(D, n_neg, per_sample_neg):
    counts = [1, 8, 17]
    x, tok, y, pos, neg = make(counts, D, n_neg, per_sample_neg, seed=D + n_neg)
    ref = reference(counts, x, tok, y, pos, neg)
    want = np.stack([means(r[0], r[1], r[2]) for r in ref])
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    with torch.no_grad():
        loss, arg = track_selection_losses_ragged(cuda(x), cuda(tok), cuda(y), cuda(pos), cuda(neg) if per_sample_neg else cuda(neg[0]),
                                                  offs, counts, POS_W, TEMP, ALIGN_W, return_argmax=True)
    got = loss.cpu().numpy().astype(np.float64)
    print(f"ragged D {D} n_neg {n_neg}: |diff| {np.abs(got - want).max():.2e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    check_argmax(np.split(arg.cpu().numpy(), np.cumsum(counts)[:-1]), ref)


@pytest.mark.parametrize("D", [1024, 128])
def test_mean_over_many_tracks(D):
    run_uniform(37, 64, D, 3, False, seed=11)


@pytest.mark.parametrize("D", [1024, 512])
def test_many_negatives(D):
    """2047 negatives: the most the register kernels take - their logits (8 x 2048 floats) fill 64 KB of LDS, and with the rows'
    hardest-negative indices behind them the launch has to ask for more"""
    run_uniform(2, 11, D, 2047, False, seed=12)
