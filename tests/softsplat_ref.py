"""Softmax splatting restated as explicit loops (the definition: the documentation block of include/savfi_hip.h).

softsplat(x, flow, metric, mode, gout): coordinates and taking-part decisions in `coord` (float32 as specified; float64 to compare with a
float64 composition), everything else in `acc`: float64 is the reference, float32 the sequential twin whose error against the reference
sizes the gates of the GPU suite.  Gradients are analytic (one gather per source pixel).  Sources are visited in row-major order, corners
in the order (x0, y0), (x1, y0), (x0, y1), (x1, y1), channels in order.

inputs(kind, shape): the seeded content kinds of the suites.  Metrics are multiples of 2^-8 and fractional flows multiples of 2^-10, so that
the float32 coordinate of the small test frames is exact and adding 1000 to a metric rounds nothing (`shifted` then differs from
`fractional` in M alone)."""
import functools

import numpy as np
import torch

MODES = ('sum', 'avg', 'soft')
SHAPES = [(1, 1, 4, 4), (2, 3, 7, 9), (1, 3, 33, 130), (1, 8, 5, 67), (2, 64, 8, 12)]
GATED = ('zero', 'integer', 'fractional', 'collide', 'leave')
KINDS = GATED + ('nonfinite', 'shifted', 'wide')


def corners(fx, fy, i, j, H, W, coord=np.float32, acc=np.float64):
    """-> [(k, q, bx, by)]: the corners of source (i, j) that take part, q the in-plane index, bx / by the 1-D factors in `acc`; and tx, ty"""
    with np.errstate(invalid='ignore', over='ignore'):
        X, Y = coord(j) + coord(fx), coord(i) + coord(fy)
        if not (X > -1 and X < W and Y > -1 and Y < H):          # in float, before any conversion to an integer; NaN fails
            return []
        x0, y0 = np.floor(X), np.floor(Y)
        tx, ty = X - x0, Y - y0
    wx = (acc(1) - acc(tx), acc(tx))
    wy = (acc(1) - acc(ty), acc(ty))
    out = []
    for k in range(4):
        dx, dy = k & 1, k >> 1
        xx, yy = x0 + dx, y0 + dy
        if 0 <= xx <= W - 1 and 0 <= yy <= H - 1 and (coord(1) - tx if dx == 0 else tx) > 0 and (coord(1) - ty if dy == 0 else ty) > 0:
            out.append((k, int(yy) * W + int(xx), wx[dx], wy[dy]))
    return out


def softsplat(x, flow, metric, mode, gout=None, coord=np.float32, acc=np.float64):
    """numpy / torch float32 arrays -> dict of `acc` arrays: out, hit, D, M and, with gout, g_x, g_flow, g_metric"""
    assert mode in MODES
    x, flow = (np.asarray(t, dtype=np.float32) for t in (x, flow))
    soft = mode == 'soft'
    Zs = np.asarray(metric, dtype=np.float32) if soft else None
    N, C, H, W = x.shape
    hw = H * W
    out, hit = np.zeros((N, C, hw), acc), np.zeros((N, hw), acc)
    D, M = np.zeros((N, hw), acc), np.full((N, hw), -np.inf, acc)
    taking = {}
    for n in range(N):
        for p in range(hw):
            i, j = divmod(p, W)
            if soft and not np.isfinite(Zs[n, 0, i, j]):
                continue
            cs = corners(flow[n, 0, i, j], flow[n, 1, i, j], i, j, H, W, coord, acc)
            if cs:
                taking[n, p] = cs
                for k, q, bx, by in cs:
                    hit[n, q] = 1
                    if soft:
                        M[n, q] = max(M[n, q], acc(Zs[n, 0, i, j]))
    M[hit == 0] = 0
    if not soft:
        M[:] = 0                                                  # M is 0 outside soft mode
    num = np.zeros((N, C, hw), acc)
    xs = x.reshape(N, C, hw).astype(acc)
    weights = {}
    for (n, p), cs in taking.items():                             # insertion order: samples, then sources in row-major order
        i, j = divmod(p, W)
        for k, q, bx, by in cs:
            e = np.exp(acc(Zs[n, 0, i, j]) - M[n, q]).astype(acc) if soft else acc(1)
            w = acc(e * acc(bx * by))
            weights[n, p, k] = (q, e, bx, by, w)
            D[n, q] = D[n, q] + w
            num[n, :, q] = num[n, :, q] + w * xs[n, :, p]
    with np.errstate(invalid='ignore', divide='ignore'):
        out = num if mode == 'sum' else np.where(hit[:, None] > 0, num / np.where(hit > 0, D, 1)[:, None], 0).astype(acc)
    for n in range(N):
        if not np.isfinite(x[n]).all():
            out[n] = np.nan
    res = dict(out=out.reshape(N, C, H, W), hit=hit.reshape(N, 1, H, W), D=D.reshape(N, 1, H, W), M=M.reshape(N, 1, H, W))
    if gout is None:
        return res
    g = np.asarray(gout, dtype=np.float32).reshape(N, C, hw).astype(acc)
    gx, gf, gz = np.zeros((N, C, hw), acc), np.zeros((N, 2, hw), acc), np.zeros((N, 1, hw), acc)
    for (n, p), cs in taking.items():
        for k, _, _, _ in cs:
            q, e, bx, by, w = weights[n, p, k]
            invD = acc(1) if mode == 'sum' else acc(1) / D[n, q]
            gd = g[n, :, q] * invD
            gx[n, :, p] = gx[n, :, p] + w * gd
            s = acc(np.sum(gd * (xs[n, :, p] - (0 if mode == 'sum' else out[n, :, q])), dtype=acc))
            if soft:
                gz[n, 0, p] = gz[n, 0, p] + s * w
            sgn_x, sgn_y = (1 if k & 1 else -1), (1 if k >> 1 else -1)
            gf[n, 0, p] = gf[n, 0, p] + s * e * sgn_x * by        # d b / dX = +- the vertical factor
            gf[n, 1, p] = gf[n, 1, p] + s * e * sgn_y * bx
    res.update(g_x=gx.reshape(N, C, H, W), g_flow=gf.reshape(N, 2, H, W), g_metric=gz.reshape(N, 1, H, W))
    return res


@functools.lru_cache(maxsize=None)
def inputs(kind, shape, seed=0):
    """-> x, flow, metric, gout: float32 torch tensors (shared: never modify them)"""
    N, C, H, W = shape
    if kind == 'shifted':                                                                   # `fractional` with 1000 added to the whole metric
        x, flow, metric, gout = inputs('fractional', shape, seed)
        return x, flow, metric + 1000, gout
    rng = np.random.default_rng(77 + 13 * KINDS.index(kind) + 101 * SHAPES.index(shape) + seed if shape in SHAPES else seed)
    x = rng.standard_normal((N, C, H, W))
    gout = rng.standard_normal((N, C, H, W))
    metric = np.round(rng.uniform(-10, 10, (N, 1, H, W)) * 256) / 256                       # spread <= 20
    frac = lambda size: np.clip(np.round(rng.uniform(1 / 16, 15 / 16, size) * 1024), 64, 960) / 1024
    cells = lambda lo, hi, size: rng.integers(lo, hi + 1, size).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    if kind == 'zero':
        flow = np.zeros((N, 2, H, W))
    elif kind == 'integer':
        flow = cells(-3, 3, (N, 2, H, W))
        x = cells(-255, 255, (N, C, H, W))
    elif kind == 'collide':
        flow = np.zeros((N, 2, H, W))
        for n in range(N):
            tgt = np.stack([cells(0, W - 2, 3) + frac(3), cells(0, H - 2, 3) + frac(3)])    # three targets (X, Y)
            pick = rng.integers(0, 3, (H, W))
            flow[n, 0], flow[n, 1] = tgt[0][pick] - jj, tgt[1][pick] - ii
    else:                                                                                   # fractional and what builds on it
        flow = cells(-2, 1, (N, 2, H, W)) + frac((N, 2, H, W))
    if kind == 'leave':
        gone = rng.uniform(size=(N, H, W)) < 0.5
        flow[:, 0][gone] += 2 * W
    if kind == 'wide':
        metric = np.round(rng.uniform(-200, 200, (N, 1, H, W)) * 256) / 256
    if kind == 'nonfinite':
        # a tenth of the sources; 1e30 is a FINITE metric (it would take part and own its targets), so it goes where the flow leaves too
        # (at least eight of them, so that every one of the eight corruptions occurs in the smallest frame too)
        chosen = rng.permutation(N * H * W)[:max(8, -(-N * H * W // 10))]
        which = np.zeros(N * H * W, dtype=np.int64)
        which[chosen] = 1 + np.arange(chosen.size) % 8
        which = which.reshape(N, H, W)
        for code, (plane, value) in enumerate([(0, np.nan), (1, np.inf), (0, -np.inf), (1, 1e30), (0, -1e30)], start=1):
            flow[:, plane][which == code] = value
        metric[:, 0][which == 6] = np.nan
        metric[:, 0][which == 7] = np.inf * np.where(rng.uniform(size=(which == 7).sum()) < 0.5, 1, -1)
        metric[:, 0][which == 8] = 1e30
        flow[:, 0][which == 8] = 1e30
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    return to(x), to(flow), to(metric), to(gout)


def corrupted(kind, shape):
    """[N,H,W] bool: the sources of a `nonfinite` case whose flow or metric was replaced"""
    x, flow, metric, _ = inputs(kind, shape)
    return ~(torch.isfinite(flow).all(1) & torch.isfinite(metric[:, 0]) & (flow.abs() < 1e29).all(1))
