"""Shared by the AdaCoF suites: the deformable-tap op of csrc/adacof.hip (definition: include/savfi_hip.h) restated in float64 on the CPU,
with the sums of magnitudes that scale the error bounds, the flags of samples that sit next to a cell edge, the counted rounding units
and the inputs the suites draw.

As in tests/warp_ref.py the coordinate is float32 BY DEFINITION: sy = float32(y + k d) + a is ONE float32 addition, it is clamped to
[-1, Hp] in float32, and the cell and the fraction are taken from that float32 number (the fraction sy - floor(sy) is exact).  coords()
transcribes this in numpy float32 and only then widens, so what the float64 sums below are away from the kernel's result is the kernel's
own rounding.  coord = np.float64 runs the same steps in float64: tests/test_adacof_ref_cpu.py uses it to hold the restatement to
F.grid_sample (bilinear, border, align_corners=True) per tap, and to show that the bounds tell the two coordinates apart.

Edges: the cell is [i, i + 1); both texel indices are clamped to the frame, so a coordinate beyond the border reads the border texel with
an offset gradient of exactly 0.  A NaN offset gives NaN in the pixel's out, the tap's g_w and both offset gradients of the tap."""
import numpy as np
import torch

from tests.upsample_ref import ULP, bound_ratio                 # noqa: F401
from tests.warp_ref import NEAR_CAP, NEAR_UNITS, _near, images  # noqa: F401

TILE_H, TILE_W = 4, 64             # csrc/adacof.hip: one workgroup per tile of 4 rows x 64 columns, one pixel per thread


# Units of 2^-24 * (sum of magnitudes): the roundings one term of the kernel's expression can pass through (nothing is contracted).
def fwd_units(F):
    """out = sum_t w_t * S(t), S = (1 - ty) * ((1 - tx) * x00 + tx * x01) + ty * (...): the two lower weights 1 - t (2), inner product and
    sum (2), outer product and sum (2), the product with w (1), the running sum over the F^2 taps (F^2 - 1: the first lands on 0)"""
    return 6 + 1 + (F * F - 1)


def gw_units(C):
    """g_w = sum_c g_c * S_c: the sample (6), the product with g (1), C - 1 sums over the channels"""
    return 6 + 1 + (C - 1)


def goff_units(C):
    """g_a = w * sum_c g_c * ((1 - tx) * (x10 - x00) + tx * (x11 - x01)): the texel difference (1), the lower weight (1), product and sum
    (2): the bracket; the product with g (1), C - 1 sums over the channels, the product with w (1).  g_b likewise."""
    return 4 + 1 + (C - 1) + 1


def _np(t, dtype):
    return t.detach().cpu().numpy().astype(dtype)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def coords(a, b, F, dilation, coord=np.float32):
    """(sy, sx) UNCLAMPED, [N, F^2, H, W] arrays of dtype `coord`: the exact integer base position plus the offset, one addition"""
    f = coord
    av, bv = _np(a, f), _np(b, f)
    _, F2, H, W = av.shape
    assert F2 == F * F
    k, l = np.arange(F2) // F, np.arange(F2) % F
    base_y = (np.arange(H).reshape(1, 1, H, 1) + (k * dilation).reshape(1, F2, 1, 1)).astype(f)
    base_x = (np.arange(W).reshape(1, 1, 1, W) + (l * dilation).reshape(1, F2, 1, 1)).astype(f)
    with np.errstate(invalid='ignore'):
        sy, sx = base_y + av, base_x + bv
    assert sy.dtype == f and sx.dtype == f
    return sy, sx


def _axis(s, size):
    """clamp in the coordinate's own format, floor, fraction (exact), the two clamped indices"""
    f = s.dtype.type
    with np.errstate(invalid='ignore'):
        sc = np.minimum(np.maximum(s, f(-1)), f(size))             # NaN passes
        fl = np.floor(sc)
        t = sc - fl
    assert t.dtype == f
    i = np.where(np.isnan(fl), -1, fl).astype(np.int64)
    return np.clip(i, 0, size - 1), np.clip(i + 1, 0, size - 1), t.astype(np.float64)[:, None]


def _gather(x, i, j):
    """x [N, C, Hp, Wp], i / j [N, F2, H, W] -> x[n, :, i, j] as [N, C, F2, H, W]"""
    n = np.arange(x.shape[0]).reshape(-1, 1, 1, 1)
    return x[n, :, i, j].transpose(0, 4, 1, 2, 3)


def adacof(x, w, a, b, dilation=1, gout=None, coord=np.float32):
    """x [N, C, Hp, Wp], w / a / b [N, F^2, H, W], gout [N, C, H, W] or None -> dict of float64 tensors: out, out_mag [N, C, H, W]; with
    gout also g_w, g_a, g_b and g_w_mag, g_a_mag, g_b_mag [N, F^2, H, W]; near [N, F^2, H, W] (bool: the unclamped coordinate of the
    sample lies within NEAR_UNITS * 2^-24 * size of an integer, in y or in x), nan [N, H, W] (bool: a NaN offset in some tap of the pixel)."""
    xs, ws = _np(x, np.float64), _np(w, np.float64)
    N, C, Hp, Wp = xs.shape
    _, F2, H, W = ws.shape
    F = int(round(F2 ** 0.5))
    assert F * F == F2 and Hp == H + (F - 1) * dilation and Wp == W + (F - 1) * dilation
    sy, sx = coords(a, b, F, dilation, coord)
    sy64, sx64 = coords(a, b, F, dilation, np.float64)
    res = dict(near=torch.from_numpy(_near(sy64, Hp) | _near(sx64, Wp)),
               nan=torch.from_numpy((np.isnan(sy) | np.isnan(sx)).any(1)))
    i0, i1, ty = _axis(sy, Hp)
    j0, j1, tx = _axis(sx, Wp)
    x00, x01, x10, x11 = _gather(xs, i0, j0), _gather(xs, i0, j1), _gather(xs, i1, j0), _gather(xs, i1, j1)
    wt = ws[:, None]
    with np.errstate(invalid='ignore'):
        S = (1 - ty) * ((1 - tx) * x00 + tx * x01) + ty * ((1 - tx) * x10 + tx * x11)
        Sa = (1 - ty) * ((1 - tx) * abs(x00) + tx * abs(x01)) + ty * ((1 - tx) * abs(x10) + tx * abs(x11))
        res['out'], res['out_mag'] = _t((wt * S).sum(2)), _t((abs(wt) * Sa).sum(2))
        if gout is None:
            return res
        g = _np(gout, np.float64)[:, :, None]
        poison = 0.0 * (ty + tx)[:, 0]                                  # NaN where either coordinate of the sample is NaN
        da = (1 - tx) * (x10 - x00) + tx * (x11 - x01)
        db = (1 - ty) * (x01 - x00) + ty * (x11 - x10)
        daa = (1 - tx) * (abs(x10) + abs(x00)) + tx * (abs(x11) + abs(x01))
        dba = (1 - ty) * (abs(x01) + abs(x00)) + ty * (abs(x11) + abs(x10))
        res['g_w'], res['g_w_mag'] = _t((g * S).sum(1)), _t((abs(g) * Sa).sum(1))
        res['g_a'], res['g_a_mag'] = _t(ws * ((g * da).sum(1) + poison)), _t(abs(ws) * (abs(g) * daa).sum(1))
        res['g_b'], res['g_b_mag'] = _t(ws * ((g * db).sum(1) + poison)), _t(abs(ws) * (abs(g) * dba).sum(1))
    return res


def grid_sample_statement(x, w, a, b, dilation=1):
    """The same op as F^2 calls of F.grid_sample(bilinear, border, align_corners=True) in the tensors' dtype, differentiable by autograd"""
    N, C, Hp, Wp = x.shape
    _, F2, H, W = w.shape
    F = int(round(F2 ** 0.5))
    ys = torch.arange(H, dtype=x.dtype).view(1, H, 1)
    xs = torch.arange(W, dtype=x.dtype).view(1, 1, W)
    out = 0
    for t in range(F2):
        sy = ys + (t // F) * dilation + a[:, t]
        sx = xs + (t % F) * dilation + b[:, t]
        grid = torch.stack((2 * sx / (Wp - 1) - 1, 2 * sy / (Hp - 1) - 1), -1)
        out = out + w[:, t:t + 1] * torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='border', align_corners=True)
    return out


def masked_ratio(got, ref, mag, units, keep=None):
    """bound_ratio over the elements of `keep` (bool, the arrays' shape; None: all)"""
    got = got.detach().cpu().double()
    if keep is None:
        return bound_ratio(got, ref, mag, units)
    if not keep.any():
        return 0.0
    return bound_ratio(got[keep], ref[keep], mag[keep], units)


# ------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------
KINDS = ('small', 'cross', 'outside', 'integer', 'wild')


def inputs(kind, N, C, H, W, F, d, seed=0):
    """(x, w, a, b, gout) float32 tensors.  small: |offset| < 1; cross: several pixels; outside: every tap beyond a border by a pixel or
    more, all four sides in turn (quadrants of the map); integer: integer offsets (the coordinate is exact) and a one-hot weight;
    wild: `cross` with +-inf, +-1e30 and NaN mixed into the offsets."""
    gen = torch.Generator().manual_seed(4000 + 131 * seed + 7 * H + W + 3 * F + d + 17 * KINDS.index(kind))
    F2, Hp, Wp = F * F, H + (F - 1) * d, W + (F - 1) * d
    x = images(N, C, Hp, Wp, gen)
    w = torch.randn(N, F2, H, W, generator=gen) / F
    gout = torch.randn(N, C, H, W, generator=gen)
    if kind == 'small':
        a, b = (2 * torch.rand(N, F2, H, W, generator=gen) - 1) * 0.999, (2 * torch.rand(N, F2, H, W, generator=gen) - 1) * 0.999
    elif kind in ('cross', 'wild'):
        a, b = 3 * torch.randn(N, F2, H, W, generator=gen), 3 * torch.randn(N, F2, H, W, generator=gen)
        if kind == 'wild':
            pool = torch.tensor([float('inf'), -float('inf'), 1e30, -1e30, float('nan')])
            for off in (a, b):
                hit = torch.rand(N, F2, H, W, generator=gen) < 0.02
                pick = pool[torch.randint(0, 5, (N, F2, H, W), generator=gen)]
                off[hit] = pick[hit]
    elif kind == 'outside':
        # beyond the top / bottom border in the upper / lower half of the map, beyond the left / right in the left / right half, by
        # 1 to 4 pixels past the clamp bound: base + offset <= -1 or >= size whatever the pixel and the tap
        far = 1 + 3 * torch.rand(N, F2, H, W, generator=gen)
        up = (torch.arange(H) < (H + 1) // 2).view(1, 1, H, 1)
        left = (torch.arange(W) < (W + 1) // 2).view(1, 1, 1, W)
        a = torch.where(up, -(Hp + far), Hp + far)
        b = torch.where(left, -(Wp + far), Wp + far)
    else:
        assert kind == 'integer'
        a = torch.randint(-3, 4, (N, F2, H, W), generator=gen).float()
        b = torch.randint(-3, 4, (N, F2, H, W), generator=gen).float()
        hot = torch.randint(0, F2, (N, 1, H, W), generator=gen)
        w = torch.zeros(N, F2, H, W).scatter_(1, hot, 1.0)
    return x.float(), w.float(), a.float(), b.float(), gout.float()
