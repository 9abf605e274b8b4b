"""Shared by the warp suites: the VoxelFlow tail of csrc/voxelwarp.hip and the pixel-flow backward warp of csrc/flowwarp.hip restated in
float64 on the CPU, with the sums of magnitudes that scale the error bounds, the flags of samples that sit next to a cell edge, and the
inputs both suites draw.

As in tests/upsample_ref.py the ops' coordinates are float32 BY DEFINITION: the reference models build them from float32 torch ops, one
rounding each, and the cell and the fraction are taken from that float32 number.  voxel_coords / flow_cell transcribe those expressions
step by step in numpy float32 and only then widen, so what the float64 sums below are away from a kernel's result is the kernel's own
rounding.  coord = np.float64 runs the same steps in float64: tests/test_warp_ref_cpu.py uses it to hold the reference to ATen's float64
kernels and to show that the bounds tell the two coordinates apart.

Derivative convention at edges (ATen's GridSampler.h): the cell is [i, i + 1); under border clamp the coordinate gradient is zero for
s <= 0 and s >= size - 1; under zero padding the gradient comes from the corners inside the image only.

tests/test_warp_ref_cpu.py holds all of this to F.grid_sample and the oracle's statements; tests/test_warp_gpu.py holds the kernels to it."""
import numpy as np
import torch

from tests.upsample_ref import ULP, bound_ratio                 # noqa: F401  (the bound is the bilinear x2 suites')

# Units of 2^-24 * (sum of magnitudes), counted as the roundings one term of the kernel's expression can pass through:
# voxel forward m * o1 + (1 - m) * o2, o = wy0 * (wx0 * a + wx1 * a') + wy1 * (...): the two lower weights 1 - w1 (2), inner product
# and sum (2), outer product and sum (2), 1 + t and 1 - m of the mask (2), the blend's product and sum (2).
# 1 - m CANCELS where the mask saturates (tanh -> 1): it inherits the rounding of m = 0.5 * (1 + t), which is relative to m and not to
# 1 - m, so its two roundings are of |m| + |1 - m|.  Everything tap b's factor 1 - m multiplies -- o2 here, the cotangent go * (1 - m)
# of the gradients below -- therefore enters the sums of magnitudes with |m| + |1 - m| (one for a mask in [0, 1]) in place of |1 - m|.
# That is a property of the float32 expression, which is the reference model's own: ATen in float32 on the CPU shows it bit for bit.
VOXEL_FWD_UNITS = 10
# g_x3[0:2] = 0.5 * (d_b * dmul_b - d_a * dmul_a), d = sum_c g * (wy0 * (a01 - a00) + wy1 * (a11 - a10)), g = go * m: the texel
# difference (1), the lower weight (1), product and sum (2), the mask (2), go * m (1), g * (...) (1), two sums over the channels (2),
# d * dmul (1), the difference of the two taps (1); 0.5 * and dmul itself are exact
VOXEL_GFLOW_UNITS = 12
# g_x3[2] = 0.5 * sum_c go * (o1 - o2): o as in the forward without mask and blend (6), o1 - o2 (1), go * (1), two sums (2)
VOXEL_GMASK_UNITS = 10
# one contribution g * wy * wx to g_frames: the mask (2), go * m (1), two lower weights (2), two products (2); a destination that n
# non-zero contributions reach adds n - 1 roundings of the atomic sum, in any order: voxel()['g_frames_units'] = 7 + n - 1 per element
VOXEL_SCATTER_UNITS = 7
# flow forward, four taps texel * (wx * wy): 1 - fx and 1 - fy (2), the weight's product (1), the tap's product (1), three sums (3)
FLOW_FWD_UNITS = 7


def flow_bwd_units(C):
    """gflow = (sum_c g * ((ne - nw) * (1 - fy) + (se - sw) * fy)) * (W / 2) * (2 / W): the texel difference (1), 1 - fy (1), product
    and sum (2), g * (1), C - 1 sums over the channels, the product with W / 2 (1, W / 2 itself is exact), 2 / W and its product (2)"""
    return 7 + C


NEAR_UNITS = 16          # a sample is `near` where its float64 coordinate lies within 16 * 2^-24 * size of an integer or a clip bound
NEAR_CAP = 0.005         # ragged inputs: the share of flagged pixels the suites accept (measured at most 6e-4 at sizes 37 to 300)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _np(t, dtype):
    return t.detach().cpu().numpy().astype(dtype)


def mesh(n, coord=np.float32):
    """torch.linspace(-1, 1, n) in float32 -- the numbers the reference's meshgrid holds -- widened to `coord`"""
    return torch.linspace(-1.0, 1.0, n, dtype=torch.float32).numpy().astype(coord)


# ------------------------------------------------------------------------------------------------------------------------------------
# VoxelFlow: two border-clamped align_corners=True samples and a blend
# ------------------------------------------------------------------------------------------------------------------------------------
def voxel_coords(x3, coord=np.float32):
    """The four unclipped source coordinates (ax, ay, bx, by), [B, H, W] arrays of dtype `coord`: tap a = I0 at g - 0.5 t, tap b = I1 at
    g + 0.5 t, each unnormalised as ((c + 1) / 2) * (size - 1), every operation rounded on its own."""
    f = coord
    t = _np(x3, f)
    B, _, H, W = t.shape
    gx, gy = mesh(W, f).reshape(1, 1, W), mesh(H, f).reshape(1, H, 1)
    out = []
    for sign in (-1, 1):
        for g, ch, size in ((gx, 0, W), (gy, 1, H)):
            half = f(0.5) * t[:, ch]
            c = g - half if sign < 0 else g + half
            s = ((c + f(1)) / f(2)) * f(size - 1)
            assert s.dtype == f and np.isfinite(s).all()
            out.append(np.broadcast_to(s, (B, H, W)))
    return tuple(out)


def _voxel_tap(s, size, right_closed=False):
    """clip, floor, drop of the upper corner: i0, i1 (int64), w0, w1 (float64), dmul = d(clipped index) / d(normalised coordinate)"""
    f = s.dtype.type
    mx = f(size - 1)
    lo = ~(s > 0)
    hi = (s >= mx) & ~lo
    dmul = np.where(lo | hi, 0.0, 0.5 * (size - 1))
    sc = np.where(lo, f(0), np.where(hi, mx, s))
    fl = np.maximum(np.ceil(sc) - 1, 0) if right_closed else np.floor(sc)       # right_closed: the cell (i, i + 1], a WRONG convention
    i0 = fl.astype(np.int64)
    frac = sc - fl
    assert frac.dtype == f                                                      # exact in either format
    drop = i0 + 1 > size - 1
    i1 = np.where(drop, i0, i0 + 1)
    w1 = np.where(drop, 0.0, frac.astype(np.float64))
    w0 = 1.0 - frac.astype(np.float64)
    return dict(i0=i0, i1=i1, w0=w0[:, None], w1=w1[:, None], dmul=dmul[:, None], slope=(i1 != i0)[:, None].astype(np.float64))


def _near(s64, size, constant=False):
    """|s - nearest integer| <= NEAR_UNITS * 2^-24 * size (the clip bounds 0 and size - 1 are integers); constant: the coordinate of a
    border-clamped axis of one sample is 0 whatever the flow, it has no edge to cross"""
    if constant:
        return np.zeros(s64.shape, bool)
    with np.errstate(invalid='ignore'):
        return ~(np.abs(s64 - np.rint(s64)) > NEAR_UNITS * ULP * size)


def _gather(img, iy, ix):
    """img [B, C, H, W], iy / ix [B, H, W] -> img[b, :, iy, ix] as [B, C, H, W]"""
    b = np.arange(img.shape[0]).reshape(-1, 1, 1)
    return img[b, :, iy, ix].transpose(0, 3, 1, 2)


def voxel(frames, x3, gout=None, coord=np.float32, right_closed=False):
    """frames [B, 6, H, W], x3 [B, 3, H, W], gout [B, 3, H, W] or None -> dict of float64 tensors: out, out_mag; with gout also g_x3,
    g_x3_mag ([B, 3, H, W]: two flow channels and the mask), g_frames, g_frames_mag, g_frames_units ([B, 6, H, W]); and near [B, H, W]
    (bool), on_integer / clipped (the share of the 4 B H W coordinates that sit exactly on an integer / are clipped)."""
    fr, t = _np(frames, np.float64), _np(x3, np.float64)
    B, _, H, W = fr.shape
    s = voxel_coords(x3, coord)
    s64 = voxel_coords(x3, np.float64)
    sizes = (W, H, W, H)
    res = dict(near=torch.from_numpy(np.logical_or.reduce([_near(a, n, n == 1) for a, n in zip(s64, sizes)])),
               on_integer=float(np.mean([np.mean(a == np.rint(a)) for a in s])),
               clipped=float(np.mean([np.mean(~(a > 0) | (a >= a.dtype.type(n - 1))) for a, n in zip(s, sizes)])))
    ax, ay, bx, by = (_voxel_tap(a, n, right_closed) for a, n in zip(s, sizes))
    m = 0.5 * (1.0 + t[:, 2:3])

    taps = []
    for (tx, ty, img) in ((ax, ay, fr[:, 0:3]), (bx, by, fr[:, 3:6])):
        c00, c01 = _gather(img, ty['i0'], tx['i0']), _gather(img, ty['i0'], tx['i1'])
        c10, c11 = _gather(img, ty['i1'], tx['i0']), _gather(img, ty['i1'], tx['i1'])
        o = ty['w0'] * (tx['w0'] * c00 + tx['w1'] * c01) + ty['w1'] * (tx['w0'] * c10 + tx['w1'] * c11)
        oa = ty['w0'] * (tx['w0'] * abs(c00) + tx['w1'] * abs(c01)) + ty['w1'] * (tx['w0'] * abs(c10) + tx['w1'] * abs(c11))
        taps.append((tx, ty, c00, c01, c10, c11, o, oa))
    (_, _, _, _, _, _, o1, o1a), (_, _, _, _, _, _, o2, o2a) = taps
    res['out'], res['out_mag'] = _t(m * o1 + (1 - m) * o2), _t(abs(m) * o1a + (abs(m) + abs(1 - m)) * o2a)
    if gout is None:
        return res

    go = _np(gout, np.float64)
    g_x3, g_mag = np.zeros((B, 3, H, W)), np.zeros((B, 3, H, W))
    g_x3[:, 2] = 0.5 * (go * (o1 - o2)).sum(1)
    g_mag[:, 2] = 0.5 * (abs(go) * (o1a + o2a)).sum(1)
    g_fr, g_fr_mag, g_fr_n = np.zeros(B * 6 * H * W), np.zeros(B * 6 * H * W), np.zeros(B * 6 * H * W)
    plane = (np.arange(B).reshape(B, 1, 1, 1) * 6 + np.arange(3).reshape(1, 3, 1, 1)) * (H * W)
    for k, (sign, g, ga) in enumerate(((-1.0, go * m, abs(go * m)), (1.0, go * (1 - m), abs(go) * (abs(m) + abs(1 - m))))):
        tx, ty, c00, c01, c10, c11, _, _ = taps[k]
        dx = (g * tx['slope'] * (ty['w0'] * (c01 - c00) + ty['w1'] * (c11 - c10))).sum(1)
        dy = (g * ty['slope'] * (tx['w0'] * (c10 - c00) + tx['w1'] * (c11 - c01))).sum(1)
        dxa = (ga * tx['slope'] * (ty['w0'] * (abs(c01) + abs(c00)) + ty['w1'] * (abs(c11) + abs(c10)))).sum(1)
        dya = (ga * ty['slope'] * (tx['w0'] * (abs(c10) + abs(c00)) + tx['w1'] * (abs(c11) + abs(c01)))).sum(1)
        # coordinate = g -+ 0.5 t, source index = (coordinate + 1) * (size - 1) / 2 with zero slope where it is clipped
        g_x3[:, 0] += sign * 0.5 * dx * tx['dmul'][:, 0]
        g_x3[:, 1] += sign * 0.5 * dy * ty['dmul'][:, 0]
        g_mag[:, 0] += 0.5 * dxa * tx['dmul'][:, 0]
        g_mag[:, 1] += 0.5 * dya * ty['dmul'][:, 0]
        for iy, wy in ((ty['i0'], ty['w0']), (ty['i1'], ty['w1'])):
            for ix, wx in ((tx['i0'], tx['w0']), (tx['i1'], tx['w1'])):
                contrib = g * wy * wx
                idx = np.broadcast_to(plane + 3 * k * H * W + (iy * W + ix)[:, None], contrib.shape).ravel()
                np.add.at(g_fr, idx, contrib.ravel())
                np.add.at(g_fr_mag, idx, np.broadcast_to(ga * wy * wx, contrib.shape).ravel())
                np.add.at(g_fr_n, idx, (contrib != 0).ravel().astype(np.float64))
    res['g_x3'], res['g_x3_mag'] = _t(g_x3), _t(g_mag)
    res['g_frames'], res['g_frames_mag'] = _t(g_fr.reshape(B, 6, H, W)), _t(g_fr_mag.reshape(B, 6, H, W))
    res['g_frames_units'] = _t(VOXEL_SCATTER_UNITS + np.maximum(g_fr_n - 1, 0).reshape(B, 6, H, W))
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# Pixel-flow backward warp: zero padding, align_corners=False
# ------------------------------------------------------------------------------------------------------------------------------------
def flow_coords(flow, coord=np.float32):
    """(ix, iy) [N, H, W] of dtype `coord`: 2 * ((x + u) / W - 0.5) and ATen's ((n + 1) * W - 1) / 2, every operation rounded on its own"""
    f = coord
    uv = _np(flow, f)
    N, _, H, W = uv.shape
    out = []
    with np.errstate(all='ignore'):
        for ch, size, shape in ((0, W, (1, 1, W)), (1, H, (1, H, 1))):
            pos = np.arange(size).astype(f).reshape(shape)
            n = f(2) * ((pos + uv[:, ch]) / f(size) - f(0.5))
            i = ((n + f(1)) * f(size) - f(1)) / f(2)
            assert i.dtype == f
            out.append(i)
    return tuple(out)


def _flow_cell(i, size, right_closed=False):
    """floor and fraction; a target that is not finite or lies further out than one cell samples nothing (cell -2, fraction 0)"""
    with np.errstate(all='ignore'):
        fl = np.ceil(i) - 1 if right_closed else np.floor(i)
        ok = np.isfinite(fl) & (fl >= -2) & (fl <= size)
        i0 = np.where(ok, fl, -2).astype(np.int64)
        frac = np.where(ok, i - fl, 0).astype(np.float64)
    return i0, frac[:, None]


def flow(img, flw, gout=None, coord=np.float32, right_closed=False):
    """img [N, C, H, W], flw [N, 2, H, W], gout [N, C, H, W] or None -> dict of float64 tensors out, out_mag and, with gout, gflow,
    gflow_mag [N, 2, H, W]; near [N, H, W] (bool), on_integer / outside (shares of the 2 N H W coordinates)."""
    a = _np(img, np.float64)
    N, C, H, W = a.shape
    ix, iy = flow_coords(flw, coord)
    ix64, iy64 = flow_coords(flw, np.float64)
    with np.errstate(all='ignore'):
        res = dict(near=torch.from_numpy(_near(ix64, W) | _near(iy64, H)),
                   on_integer=float(np.mean([np.mean(c == np.rint(c)) for c in (ix, iy)])),
                   outside=float(np.mean([np.mean(~((c > -1) & (c < n))) for c, n in ((ix, W), (iy, H))])))
    x0, fx = _flow_cell(ix, W, right_closed)
    y0, fy = _flow_cell(iy, H, right_closed)

    def texel(yy, xx):
        inside = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H))[:, None]
        return _gather(a, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)) * inside

    nw, ne, sw, se = texel(y0, x0), texel(y0, x0 + 1), texel(y0 + 1, x0), texel(y0 + 1, x0 + 1)
    wnw, wne, wsw, wse = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
    res['out'] = _t(nw * wnw + ne * wne + sw * wsw + se * wse)
    res['out_mag'] = _t(abs(nw) * wnw + abs(ne) * wne + abs(sw) * wsw + abs(se) * wse)
    if gout is None:
        return res
    g = _np(gout, np.float64)
    gx = (g * ((ne - nw) * (1 - fy) + (se - sw) * fy)).sum(1)
    gy = (g * ((sw - nw) * (1 - fx) + (se - ne) * fx)).sum(1)
    gxa = (abs(g) * ((abs(ne) + abs(nw)) * (1 - fy) + (abs(se) + abs(sw)) * fy)).sum(1)
    gya = (abs(g) * ((abs(sw) + abs(nw)) * (1 - fx) + (abs(se) + abs(ne)) * fx)).sum(1)
    res['gflow'], res['gflow_mag'] = _t(np.stack((gx, gy), 1)), _t(np.stack((gxa, gya), 1))
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def images(N, C, H, W, gen):
    """Pictures with structure: channel c % 3 == 0 a smooth ramp plus a little noise, c % 3 == 1 one constant plane, c % 3 == 2 white
    noise.  On the ramp a wrong corner or weight shows against the magnitude bound instead of drowning in texel differences of order one."""
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    img = torch.randn(N, C, H, W, generator=gen)
    for c in range(C):
        if c % 3 == 0:
            img[:, c:c + 1] = (0.8 + 0.1 * c) * xx - (0.6 - 0.05 * c) * yy + 0.3 + 0.02 * img[:, c:c + 1]
        elif c % 3 == 1:
            img[:, c] = 0.75
    return img


def _randint(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def voxel_lattice(B, H, W, seed=0):
    """(frames, x3, gout) whose coordinates are exact in float32: size - 1 a power of two (or size 1), t = j / (size - 1) for integer
    |j| <= size - 1, which gives s = x -+ j / 4; the mask channel is k / 8.  Asserts that the float32 and float64 coordinates are bit-equal
    and, on an axis of at least two samples, that both exact clip bounds are hit."""
    gen = torch.Generator().manual_seed(9000 + 131 * seed + 7 * H + W)
    x3 = torch.zeros(B, 3, H, W, dtype=torch.float64)
    for ch, size in ((0, W), (1, H)):
        if size == 1:
            x3[:, ch] = _randint(-4, 4, (B, H, W), gen) / 4
            continue
        lim = size - 1
        assert lim & (lim - 1) == 0, "lattice sizes: size - 1 a power of two"
        wide, narrow = _randint(-lim, lim, (B, H, W), gen), _randint(-min(lim, 8), min(lim, 8), (B, H, W), gen)
        x3[:, ch] = torch.where(torch.rand(B, H, W, generator=gen) < 0.5, wide, narrow) / lim
    x3[:, 0, 0, 0], x3[:, 0, 0, W - 1], x3[:, 1, 0, 0], x3[:, 1, H - 1, 0] = 0, 0, 0, 0          # s == 0 and s == size - 1, both taps
    if W >= 5:
        x3[:, 0, 0, 1] = 4.0 / (W - 1)                                                       # tap a reaches s == 0 from x = 1
    if H >= 5:
        x3[:, 1, 1, 0] = -4.0 / (H - 1)                                                      # tap b reaches s == 0 from y = 1
    x3[:, 2] = _randint(-8, 8, (B, H, W), gen) / 8
    x3 = x3.float()
    s32, s64 = voxel_coords(x3, np.float32), voxel_coords(x3, np.float64)
    for a, b, size in zip(s32, s64, (W, H, W, H)):
        assert np.array_equal(a.astype(np.float64), b), "lattice coordinates must be exact in float32"
        assert size == 1 or ((a == 0).any() and (a == size - 1).any()), "both exact clip bounds must be hit"
    return images(B, 6, H, W, gen), x3, torch.randn(B, 3, H, W, generator=gen)


def voxel_ragged(B, H, W, amp, seed=0):
    """odd sizes, x3 = tanh(amp * randn): amp 2 pushes many samples past the border"""
    gen = torch.Generator().manual_seed(7000 + 131 * seed + 7 * H + W + int(10 * amp))
    x3 = torch.tanh(amp * torch.randn(B, 3, H, W, generator=gen))
    return images(B, 6, H, W, gen), x3, torch.randn(B, 3, H, W, generator=gen)


def flow_lattice(N, C, H, W, seed=0):
    """(img, flow, gout) with H, W powers of two and flows in multiples of 1/4 in [-(size + 2), size + 2]: x + u, the division by the
    size and everything after it are exact.  Some pixels are set so that the source cell starts at -1, W - 1, W, -2 and far outside
    (the parked cell), in x and in y.  Asserts that the float32 and float64 coordinates are bit-equal."""
    gen = torch.Generator().manual_seed(5000 + 131 * seed + 7 * H + W + C)
    flw = torch.zeros(N, 2, H, W, dtype=torch.float64)
    for ch, size in ((0, W), (1, H)):
        assert size & (size - 1) == 0, "lattice sizes: powers of two"
        wide, narrow = _randint(-4 * (size + 2), 4 * (size + 2), (N, H, W), gen), _randint(-10, 10, (N, H, W), gen)
        flw[:, ch] = torch.where(torch.rand(N, H, W, generator=gen) < 0.5, wide, narrow) / 4
    # source position = pixel + flow - 0.5; the x targets go to row 0 and the last pixel, the y targets to column W - 1 and (H - 1, 0);
    # a target that the flow range does not reach from its pixel (sizes below 8) is left to the draw
    def put(ch, y, x, value, size):
        if abs(value) <= size + 2:
            flw[:, ch, y, x] = value

    for k, target in enumerate((-1.0, W - 1.0, float(W), -2.0, -4.0)):
        put(0, 0, min(k, W - 1), target + 0.5 - min(k, W - 1), W)
        put(1, min(k, H - 1), W - 1, target + 0.5 - min(k, H - 1), H)
    put(0, H - 1, W - 1, 3.5, W)
    put(1, H - 1, 0, 3.5, H)
    assert (flw[:, 0].abs() <= W + 2).all() and (flw[:, 1].abs() <= H + 2).all()
    flw = flw.float()
    for a, b in zip(flow_coords(flw, np.float32), flow_coords(flw, np.float64)):
        assert np.array_equal(a.astype(np.float64), b), "lattice coordinates must be exact in float32"
    return images(N, C, H, W, gen), flw, torch.randn(N, C, H, W, generator=gen)


def flow_ragged(N, C, H, W, amp, seed=0):
    """odd sizes, flow = amp * randn pixels: at amp 30 most targets leave the frame"""
    gen = torch.Generator().manual_seed(3000 + 131 * seed + 7 * H + W + C + int(amp))
    flw = amp * torch.randn(N, 2, H, W, generator=gen)
    return images(N, C, H, W, gen), flw, torch.randn(N, C, H, W, generator=gen)


def masked_ratio(got, ref, mag, units, keep):
    """bound_ratio over the pixels of `keep` [B, H, W] (bool) of [B, C, H, W] maps"""
    k = keep.unsqueeze(1).expand_as(ref)
    if not k.any():
        return 0.0
    return bound_ratio(got.detach().cpu().double()[k], ref[k], mag[k], units)
