"""Shared by the second-order warp suites: the backward of the two warps' first-order gradients -- savfi_voxelwarp_bwd2_f32 of
csrc/voxelwarp.hip and savfi_flowwarp_bwd2_f32 of csrc/flowwarp.hip -- restated in float64 on the CPU, with the sums of magnitudes that
scale the error bounds and the cotangent both suites draw.

Everything that decides a cell comes from tests/warp_ref.py: the float32 transcription of the coordinates (voxel_coords, flow_coords), the
clip / floor / dropped corner of a VoxelFlow tap (_voxel_tap), the parked cell of the flow warp (_flow_cell), the gather and the
near-edge flag.  So the cells, fractions and clip decisions here are the first-order reference's own, and what the float64 sums below
are away from a kernel's result is the kernel's own rounding.  coord = np.float64 runs the same steps in float64:
tests/test_warp2_ref_cpu.py uses it to hold this restatement to double autograd through the oracle's written-out statements.

With the frames constant a warp's output at a pixel depends on x3 (the flow) at that pixel alone, so the Hessian of <gO, out> is one small
block per pixel.  A bilinear cell is linear in each axis: its only second derivative is the mixed difference X = (c11 - c10) - (c01 - c00)
of its corners, and the diagonal of every block is zero.

tests/test_warp2_gpu.py holds the kernels to this."""
import numpy as np
import torch

from tests.warp_ref import (ULP, NEAR_CAP, bound_ratio, masked_ratio, voxel_coords, _voxel_tap, flow_coords, _flow_cell,      # noqa: F401
                            _gather, _near, _np, _t)

# Units of 2^-24 * (sum of magnitudes), counted as the roundings one term of the kernel's expression can pass through (a contraction to
# fma only removes roundings).  Everything tap b's factor 1 - m multiplies enters the sums with |m| + |1 - m| (warp_ref.py: 1 - m inherits
# the rounding of m, which is relative to m).
#
# d_gO[c] = 0.5 * (v0 * ((m2 * Bx) * dxb - (m * Ax) * dxa) + v1 * (...) + v2 * (o1 - o2)), dxb = sx * (wy0 * (q01 - q00) + wy1 * (q11 - q10)):
# the texel difference (1), the lower weight 1 - w1 (1), product and sum of the bracket (2), the mask 1 + t and 1 - m (2), m2 * Bx (1),
# the product with the bracket (1), the difference of the two taps (1), v0 * (1), two sums of the three v terms (2); 0.5 *, the
# slopes and dmul itself are exact.  The v2 term has 10: o as in the forward without mask and blend (6), o1 - o2 (1), v2 * (1), two sums (2).
VOXEL_DGO_UNITS = 12
# d_x3[0] = v1 * h01 + v2 * h02 (d_x3[1] likewise with h12), h01 = 0.25 * sum_c go * ((m * (Ax * Ay)) * xa + (m2 * (Bx * By)) * xb),
# xa = (sx * sy) * ((a11 - a10) - (a01 - a00)): a texel difference (1), the difference of the differences (1), the mask (2), Ax * Ay (1),
# its product with the mask (1), the product with xa (1), the sum of the two taps (1), go * (1), two sums over the channels (2), v1 * (1),
# the last sum (1) = 13; 0.25 * is exact.  The h02 term has 11: the bracket dxa (4), Ax * (1), the sum of the two taps (1), go * (1),
# two sums over the channels (2), v2 * (1), the last sum (1).
VOXEL_DFLOW_UNITS = 13
# d_x3[2] = v0 * h02 + v1 * h12: the 11 of an h02 term above
VOXEL_DMASK_UNITS = 11
# d_gout[c] = vu' * Dx_c + vv' * Dy_c, vu' = vu * (W / 2) * (2 / W), Dx_c = (ne - nw) * (1 - fy) + (se - sw) * fy: the texel difference (1),
# 1 - fy (1), product and sum (2), the product with W / 2 (1, W / 2 itself is exact), 2 / W and its product (2), vu' * (1), the sum (1)
FLOW_DGOUT_UNITS = 9


def flow_dflow_units(C):
    """d_flow[0] = s * vv' * (W / 2) * (2 / W), s = sum_c g_c * ((se - sw) - (ne - nw)), vv' = vv * (H / 2) * (2 / H): a texel difference
    (1), the difference of the differences (1), g * (1), C - 1 sums over the channels, the three roundings of vv' (3), s * vv' (1), the
    product with W / 2 (1), 2 / W and its product (2)"""
    return 9 + C


def cotangent(like, seed=0):
    """the cotangent of g_x3 / gflow: white noise of the gradient's shape from a seeded generator"""
    shape = tuple(like.shape)
    return torch.randn(shape, generator=torch.Generator().manual_seed(11000 + 17 * seed + sum((k + 1) * n for k, n in enumerate(shape))))


# ------------------------------------------------------------------------------------------------------------------------------------
# VoxelFlow tail
# ------------------------------------------------------------------------------------------------------------------------------------
def voxel2(frames, x3, gout, v, coord=np.float32, right_closed=False, clip_slope_in_x=True, corner_slope_in_x=True):
    """frames [B, 6, H, W], x3, gout, v [B, 3, H, W] -> dict of float64 tensors d_gO, d_gO_mag, d_x3, d_x3_mag [B, 3, H, W] and near
    [B, H, W] (bool, warp_ref's flag).  right_closed, clip_slope_in_x = False (X keeps (size - 1) / 2 where its coordinate is clipped)
    and corner_slope_in_x = False (X without the factors that say the upper corner exists) are WRONG conventions for the CPU suite."""
    fr, t, go, vv = (_np(a, np.float64) for a in (frames, x3, gout, v))
    B, _, H, W = fr.shape
    s, s64 = voxel_coords(x3, coord), voxel_coords(x3, np.float64)
    sizes = (W, H, W, H)
    near = torch.from_numpy(np.logical_or.reduce([_near(a, n, n == 1) for a, n in zip(s64, sizes)]))
    ax, ay, bx, by = (_voxel_tap(a, n, right_closed) for a, n in zip(s, sizes))
    m = 0.5 * (1.0 + t[:, 2:3])
    m2, m2a = 1 - m, abs(m) + abs(1 - m)
    v0, v1, v2 = vv[:, 0:1], vv[:, 1:2], vv[:, 2:3]

    taps = []
    for tx, ty, img in ((ax, ay, fr[:, 0:3]), (bx, by, fr[:, 3:6])):
        c00, c01 = _gather(img, ty['i0'], tx['i0']), _gather(img, ty['i0'], tx['i1'])
        c10, c11 = _gather(img, ty['i1'], tx['i0']), _gather(img, ty['i1'], tx['i1'])
        k00, k01, k10, k11 = abs(c00), abs(c01), abs(c10), abs(c11)
        xs = tx['slope'] * ty['slope'] if corner_slope_in_x else 1.0
        full = (0.5 * (W - 1)) * (0.5 * (H - 1))
        taps.append(dict(
            o=ty['w0'] * (tx['w0'] * c00 + tx['w1'] * c01) + ty['w1'] * (tx['w0'] * c10 + tx['w1'] * c11),
            oa=ty['w0'] * (tx['w0'] * k00 + tx['w1'] * k01) + ty['w1'] * (tx['w0'] * k10 + tx['w1'] * k11),
            dx=tx['slope'] * (ty['w0'] * (c01 - c00) + ty['w1'] * (c11 - c10)),
            dxa=tx['slope'] * (ty['w0'] * (k01 + k00) + ty['w1'] * (k11 + k10)),
            dy=ty['slope'] * (tx['w0'] * (c10 - c00) + tx['w1'] * (c11 - c01)),
            dya=ty['slope'] * (tx['w0'] * (k10 + k00) + tx['w1'] * (k11 + k01)),
            x=xs * ((c11 - c10) - (c01 - c00)), xa=xs * (k11 + k10 + k01 + k00),
            sx=tx['dmul'], sy=ty['dmul'], sxy=tx['dmul'] * ty['dmul'] if clip_slope_in_x else full))
    a, b = taps

    d_gO = 0.5 * (v0 * (m2 * b['sx'] * b['dx'] - m * a['sx'] * a['dx']) + v1 * (m2 * b['sy'] * b['dy'] - m * a['sy'] * a['dy'])
                  + v2 * (a['o'] - b['o']))
    d_gO_mag = 0.5 * (abs(v0) * (m2a * b['sx'] * b['dxa'] + abs(m) * a['sx'] * a['dxa'])
                      + abs(v1) * (m2a * b['sy'] * b['dya'] + abs(m) * a['sy'] * a['dya']) + abs(v2) * (a['oa'] + b['oa']))
    ga = abs(go)
    h01 = 0.25 * (go * (m * a['sxy'] * a['x'] + m2 * b['sxy'] * b['x'])).sum(1, keepdims=True)
    h01a = 0.25 * (ga * (abs(m) * a['sxy'] * a['xa'] + m2a * b['sxy'] * b['xa'])).sum(1, keepdims=True)
    h02 = -0.25 * (go * (a['sx'] * a['dx'] + b['sx'] * b['dx'])).sum(1, keepdims=True)
    h02a = 0.25 * (ga * (a['sx'] * a['dxa'] + b['sx'] * b['dxa'])).sum(1, keepdims=True)
    h12 = -0.25 * (go * (a['sy'] * a['dy'] + b['sy'] * b['dy'])).sum(1, keepdims=True)
    h12a = 0.25 * (ga * (a['sy'] * a['dya'] + b['sy'] * b['dya'])).sum(1, keepdims=True)
    d_x3 = np.concatenate((v1 * h01 + v2 * h02, v0 * h01 + v2 * h12, v0 * h02 + v1 * h12), 1)
    d_x3_mag = np.concatenate((abs(v1) * h01a + abs(v2) * h02a, abs(v0) * h01a + abs(v2) * h12a, abs(v0) * h02a + abs(v1) * h12a), 1)
    return dict(d_gO=_t(d_gO), d_gO_mag=_t(d_gO_mag), d_x3=_t(d_x3), d_x3_mag=_t(d_x3_mag), near=near)


# ------------------------------------------------------------------------------------------------------------------------------------
# Pixel-flow backward warp
# ------------------------------------------------------------------------------------------------------------------------------------
def flow2(img, flw, gout, v, coord=np.float32, right_closed=False):
    """img, gout [N, C, H, W], flw, v [N, 2, H, W] -> dict of float64 tensors d_gout, d_gout_mag [N, C, H, W], d_flow, d_flow_mag
    [N, 2, H, W] and near [N, H, W] (bool).  The factors (W / 2) * (2 / W) and (H / 2) * (2 / H) are one here; the units count their
    roundings.  A parked cell (warp_ref._flow_cell: cell -2, fraction 0) has four zero texels, so all of its outputs are zero."""
    a, g, vv = (_np(t, np.float64) for t in (img, gout, v))
    N, C, H, W = a.shape
    ix, iy = flow_coords(flw, coord)
    ix64, iy64 = flow_coords(flw, np.float64)
    with np.errstate(all='ignore'):
        near = torch.from_numpy(_near(ix64, W) | _near(iy64, H))
    x0, fx = _flow_cell(ix, W, right_closed)
    y0, fy = _flow_cell(iy, H, right_closed)

    def texel(yy, xx):
        inside = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H))[:, None]
        return _gather(a, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)) * inside

    nw, ne, sw, se = texel(y0, x0), texel(y0, x0 + 1), texel(y0 + 1, x0), texel(y0 + 1, x0 + 1)
    vu, vw = vv[:, 0:1], vv[:, 1:2]
    dx, dy = (ne - nw) * (1 - fy) + (se - sw) * fy, (sw - nw) * (1 - fx) + (se - ne) * fx
    dxa = (abs(ne) + abs(nw)) * (1 - fy) + (abs(se) + abs(sw)) * fy
    dya = (abs(sw) + abs(nw)) * (1 - fx) + (abs(se) + abs(ne)) * fx
    s = (g * ((se - sw) - (ne - nw))).sum(1, keepdims=True)
    sa = (abs(g) * (abs(se) + abs(sw) + abs(ne) + abs(nw))).sum(1, keepdims=True)
    return dict(d_gout=_t(vu * dx + vw * dy), d_gout_mag=_t(abs(vu) * dxa + abs(vw) * dya),
                d_flow=_t(np.concatenate((vw * s, vu * s), 1)), d_flow_mag=_t(np.concatenate((abs(vw) * sa, abs(vu) * sa), 1)), near=near)
