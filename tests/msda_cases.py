"""Multi-scale deformable attention: the project's own restatement of sola_ms_deform_attn's contract (the direct corner form, in
torch on the CPU, dtype selectable), the public statement it must equal (F.grid_sample per level, weighted and summed) and the
seeded case builders shared by test_msda_cpu.py and test_gpu_msda.py."""
import math

import torch
import torch.nn.functional as F

# (levels, N, Lq, M, D, P); tuples throughout: a case is a cache key
SMALL = (((7, 5), (4, 3), (2, 2), (1, 1)), 2, 37, 3, 32, 4)
CASES = [
    SMALL,
    (((16, 16),), 1, 64, 1, 16, 1),
    (((9, 13), (5, 7)), 2, 130, 8, 64, 3),
    (((100, 167), (50, 84), (25, 42), (13, 21)), 1, 900, 8, 32, 4),
] + [(SMALL[0], SMALL[1], lq, SMALL[3], SMALL[4], SMALL[5]) for lq in (1, 63, 65)]
DECODER = CASES[3]


def case_id(case):
    levels, N, Lq, M, D, P = case
    return f"L{len(levels)}x{levels[0][0]}x{levels[0][1]}-N{N}-Lq{Lq}-M{M}-D{D}-P{P}"


def level_tables(levels):
    """(spatial_shapes int64 [L,2], level_start_index int64 [L], S) of maps stored one after the other."""
    shapes = torch.tensor(levels, dtype=torch.int64).reshape(len(levels), 2)
    sizes = shapes[:, 0] * shapes[:, 1]
    start = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]])
    return shapes, start, int(sizes.sum())


def make_case(case, seed=0):
    """Float32 CPU inputs: values standard normal, locations uniform in [-0.15, 1.15] (about 40 % of the samples have a
    coordinate outside the maps), weights a softmax over L*P."""
    levels, N, Lq, M, D, P = case
    L = len(levels)
    shapes, start, S = level_tables(levels)
    g = torch.Generator().manual_seed(1000 + seed)
    value = torch.randn(N, S, M, D, generator=g)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15
    w = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).reshape(N, Lq, M, L, P)
    return value, shapes, start, loc, w


def restatement(value, shapes, start, loc, w, dtype=torch.float64, rows=None):
    """The contract, corner by corner, in ``dtype``: x = loc_x * W - 0.5, floor, four weighted corners; a corner outside its map
    or whose row is not in [0, rows) contributes nothing (rows: default S, the rows value has).  Sum over (l, p) in that order."""
    N, S, M, D = value.shape
    rows = S if rows is None else rows
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v = value.to(dtype)
    out = torch.zeros(N, Lq, M, D, dtype=dtype)
    n_idx = torch.arange(N).view(N, 1, 1).expand(N, Lq, M)
    m_idx = torch.arange(M).view(1, 1, M).expand(N, Lq, M)
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(start[l])
        if H <= 0 or W <= 0:
            continue
        for p in range(P):
            x = loc[:, :, :, l, p, 0].to(dtype) * W - 0.5
            y = loc[:, :, :, l, p, 1].to(dtype) * H - 0.5
            x0, y0 = torch.floor(x), torch.floor(y)
            lx, ly = x - x0, y - y0
            x0, y0 = x0.long(), y0.long()
            sample = torch.zeros(N, Lq, M, D, dtype=dtype)
            for dy, dx, cw in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
                yy, xx = y0 + dy, x0 + dx
                row = st + yy * W + xx
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & (row >= 0) & (row < rows)
                got = v[n_idx, row.clamp(0, S - 1), m_idx]  # [N, Lq, M, D]
                sample = sample + torch.where(ok.unsqueeze(-1), cw.unsqueeze(-1) * got, torch.zeros((), dtype=dtype))
            out = out + w[:, :, :, l, p].to(dtype).unsqueeze(-1) * sample
    return out.reshape(N, Lq, M * D)


def statement(value, shapes, start, loc, w, dtype=torch.float64):
    """The public statement (Deformable-DETR's ms_deform_attn_core_pytorch): one F.grid_sample per level on 2 * loc - 1,
    bilinear, zero padding, align_corners=False; the samples weighted and summed.  Well-formed tables only."""
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v, grids = value.to(dtype), 2 * loc.to(dtype) - 1
    sampled = []
    for l in range(L):
        H, W, st = int(shapes[l, 0]), int(shapes[l, 1]), int(start[l])
        level = v[:, st:st + H * W].flatten(2).transpose(1, 2).reshape(N * M, D, H, W)
        grid = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)  # [N*M, Lq, P, 2]
        sampled.append(F.grid_sample(level, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
    aw = w.to(dtype).transpose(1, 2).reshape(N * M, 1, Lq, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(N, M * D, Lq)
    return out.transpose(1, 2).contiguous()


def parity_bound(value, shapes, w):
    """Per output element [N, Lq, M, 1]: Vmax * sum_{l,p} |w| * (4 * max_l (H_l + W_l) + 32) * 2^-24.  loc * W - 0.5 in float32
    misplaces a sample by at most W * 2^-23 (H * 2^-23 in y); the zero-padded bilinear surface is continuous with slope at most
    2 * Vmax per pixel: 4 (H + W) 2^-24 Vmax; the corner weights, the 4-term and the 16-term sums add fewer than 32 roundings."""
    vmax = float(value.abs().max())
    hw = max(int(h) + int(w_) for h, w_ in shapes.tolist())
    return vmax * w.double().abs().sum((-1, -2)).unsqueeze(-1) * (4 * hw + 32) * math.ldexp(1.0, -24)
