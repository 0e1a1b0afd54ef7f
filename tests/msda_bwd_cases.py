"""Multi-scale deformable attention, backward: the float64 yardstick (autograd through msda_cases.restatement), the mask of the
samples whose gradient with respect to the location is not defined to float32 precision, and the error bounds of the three
gradients, shared by test_msda_bwd_cpu.py and test_gpu_msda_bwd.py."""
import functools
import math

import torch

import msda_cases as mc

EPS = math.ldexp(1.0, -24)  # half a unit in the last place of a float32 in [1, 2)
MAX_EXCLUDED = 0.002        # near_border may leave out at most this share of a case's samples


def autograd_grads(fn, value, shapes, start, loc, w, grad_out, dtype, **kw):
    """(grad_value, grad_loc, grad_weight) of ``fn`` (mc.restatement or mc.statement) by torch autograd in ``dtype``, on the
    device the float inputs are on."""
    v, x, a = (t.detach().to(dtype).requires_grad_(True) for t in (value, loc, w))
    fn(v, shapes, start, x, a, dtype, **kw).backward(grad_out.to(dtype))
    return v.grad, x.grad, a.grad


def make_grad_out(case, seed=0):
    _, N, Lq, M, D, _ = case
    return torch.randn(N, Lq, M * D, generator=torch.Generator().manual_seed(2000 + seed))


@functools.lru_cache(maxsize=None)
def grad_reference(case):
    """(inputs of mc.make_case, grad_out float32 standard normal, (grad_value, grad_loc, grad_weight) in float64 by autograd through
    the restatement).  Computed once per case, shared, never modified."""
    inputs = mc.make_case(case)
    grad_out = make_grad_out(case)
    return inputs, grad_out, autograd_grads(mc.restatement, *inputs, grad_out, torch.float64)


def near_border(loc, shapes, delta=1e-4):
    """[N,Lq,M,L,P] bool: the sample's pixel x or y (loc * W - 0.5, float64) lies within ``delta`` of an integer.  float32
    places a sample up to W * 2^-23 pixels off (2e-5 at W = 167); one that close to a cell border may take the neighbour
    cell's slope, which is as right as its own."""
    size = shapes.flip(-1).to(torch.float64).view(1, 1, 1, -1, 1, 2)  # (W, H) next to (x, y)
    px = loc.double() * size - 0.5
    return ((px - px.round()).abs() < delta).any(-1)


def _hw(shapes):
    return max(int(h) + int(w_) for h, w_ in shapes.tolist())


def _g_abs(grad_out, M):
    N, Lq, MD = grad_out.shape
    return grad_out.double().abs().reshape(N, Lq, M, MD // M).sum(-1)  # G = sum_d |g_d|, [N,Lq,M]


def grad_weight_bound(value, shapes, grad_out):
    """[N,Lq,M,1,1]: G * Vmax * (4 hw + 32 + D) * 2^-24.  The bilinear sample of channel d is off by Vmax (4 hw + 32) 2^-24 as in
    mc.parity_bound (misplaced by W 2^-23 on a surface of slope <= 2 Vmax per pixel, plus the roundings of the coefficients
    and the 4-term sum); the product with g_d and the D-term sum add fewer than D roundings of at most G * Vmax."""
    D = value.shape[-1]
    vmax = float(value.abs().max())
    return (_g_abs(grad_out, value.shape[2]) * vmax * (4 * _hw(shapes) + 32 + D) * EPS)[..., None, None]


def grad_loc_bound(value, shapes, w, grad_out):
    """[N,Lq,M,L,P,2]: (W_l, H_l) * |w| * G * Vmax * (8 hw + 2 (32 + D)) * 2^-24, for samples that are not near_border.  Inside a
    cell the slope in x is (1-ly)(v_01 - v_00) + ly (v_11 - v_10): differences of up to 2 Vmax, linear in ly with slope up to
    4 Vmax per pixel - twice the figures of grad_weight_bound."""
    D = value.shape[-1]
    vmax = float(value.abs().max())
    size = shapes.flip(-1).to(torch.float64).view(1, 1, 1, -1, 1, 2)
    per_sample = (w.double().abs() * _g_abs(grad_out, value.shape[2])[..., None, None]).unsqueeze(-1)
    return size * per_sample * vmax * (8 * _hw(shapes) + 2 * (32 + D)) * EPS


def grad_value_bound(value, shapes, start, loc, w, grad_out, rows=None):
    """[N,M]: Tmax * (4 hw + 32 + Amax) * 2^-24.  T[n,row,m,d] is the scatter of |w| |g_d| onto every counting corner with
    coefficient 1 and Amax the largest number of hits on one row of (n, m).  A contribution w c_k g_d is off by |w g_d| times
    the coefficient's error, (H + W) 2^-23 from the misplaced sample plus a few roundings - summed over a row's hits at most
    T (4 hw + 32) 2^-24; every one of the up to Amax float32 adds into an element rounds a partial sum of at most T."""
    N, S, M, D = value.shape
    rows = S if rows is None else rows
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    T = torch.zeros(N, S, M, D, dtype=torch.float64)
    A = torch.zeros(N, S, M, dtype=torch.float64)
    n_idx = torch.arange(N).view(N, 1, 1).expand(N, Lq, M)
    m_idx = torch.arange(M).view(1, 1, M).expand(N, Lq, M)
    g = grad_out.double().abs().reshape(N, Lq, M, D)
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(start[l])
        if H <= 0 or W <= 0:
            continue
        for p in range(P):
            x0 = torch.floor(loc[:, :, :, l, p, 0].double() * W - 0.5).long()
            y0 = torch.floor(loc[:, :, :, l, p, 1].double() * H - 0.5).long()
            wg = w[:, :, :, l, p].double().abs().unsqueeze(-1) * g
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                yy, xx = y0 + dy, x0 + dx
                row = st + yy * W + xx
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & (row >= 0) & (row < rows)
                at = (n_idx[ok], row[ok], m_idx[ok])
                T.index_put_(at, wg[ok], accumulate=True)
                A.index_put_(at, torch.ones((), dtype=torch.float64).expand(int(ok.sum())), accumulate=True)
    return T.amax((1, 3)) * (4 * _hw(shapes) + 32 + A.amax(1)) * EPS


def worst_ratios(got, want, value, shapes, start, loc, w, grad_out, rows=None):
    """(grad_value, grad_loc, grad_weight) errors of ``got`` against the float64 ``want``, each as its largest multiple of its
    bound (grad_loc over the samples that are not near_border), and the excluded share of the samples.  None in ``got`` is
    passed over (its ratio is 0)."""
    gv, gl, gw = got
    ratios = [0.0, 0.0, 0.0]
    if gv is not None:
        err = (gv.double().cpu() - want[0]).abs().amax((1, 3))
        bound = grad_value_bound(value, shapes, start, loc, w, grad_out, rows)
        ratios[0] = float((err / bound.clamp_min(1e-300)).max())
    border = near_border(loc, shapes)
    if gl is not None:
        err = (gl.double().cpu() - want[1]).abs()
        bound = grad_loc_bound(value, shapes, w, grad_out)
        keep = (~border).unsqueeze(-1).expand_as(err)
        ratios[1] = float((err[keep] / bound[keep].clamp_min(1e-300)).max())
    if gw is not None:
        err = (gw.double().cpu() - want[2]).abs()
        ratios[2] = float((err / grad_weight_bound(value, shapes, grad_out).clamp_min(1e-300)).max())
    return ratios, float(border.double().mean())
