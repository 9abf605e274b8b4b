"""Float64 restatement of the census (soft ternary) term ``Census`` of --loss.  There is no reference implementation: this file IS the
definition, and the kernels of csrc/census.hip, the composed form of hip_ops and the golden fixture are held to it.

For one sample ``x`` of shape ``[C, H, W]``, ``C`` 3 or 1, ``H, W >= 3``:

* ``g = 0.2989 x_0 + 0.5870 x_1 + 0.1140 x_2`` (``C == 1``: ``g = x_0``), and ``g = 0`` outside the frame (zero padding, not reflection);
* for each of the 49 offsets ``o`` in ``{-3..3}^2``, centre included: ``d_o(p) = g(p + o) - g(p)``, ``t_o(p) = d_o / sqrt(0.81 + d_o^2)``;
* for a pair: ``delta_o = (t_o(sr) - t_o(hr))^2``, ``h_o = delta_o / (0.1 + delta_o)``, ``c(p) = sum_o h_o(p) / 49``;
* the mask ``m(p)`` is 1 for ``1 <= y <= H - 2`` and ``1 <= x <= W - 2``, otherwise 0 (pixels up to 3 from the border still read padding:
  that is intended);
* ``census = sum_p m(p) c(p) / (H W)`` per sample: masked pixels count in the divisor.

The one-value form is the mean over the batch.  Gradient for ``sr`` only.  The definition has no kink: every pair is conditioned.
"""
import torch
import torch.nn.functional as F

GRAY = (0.2989, 0.5870, 0.1140)
RADIUS = 3
VALUE_FLOOR = 4 * 2.0 ** -24
GRAD_FLOOR = 2.0 ** -20
SIZES = ((3, 3), (7, 9), (16, 21), (37, 53), (64, 64), (40, 300))
KINDS = ('noise', 'smooth', 'near')
SEED = 0


def check_shape(C, H, W):
    if C not in (1, 3):
        raise ValueError("census needs 3 or 1 channels, got %d" % C)
    if H < 3 or W < 3:
        raise ValueError("census needs H, W >= 3, got %d x %d" % (H, W))


def gray(x):
    """[N,C,H,W] -> [N,H,W]."""
    if x.shape[1] == 1:
        return x[:, 0]
    return GRAY[0] * x[:, 0] + GRAY[1] * x[:, 1] + GRAY[2] * x[:, 2]


def ternary(x):
    """[N,C,H,W] -> [N,49,H,W]: t_o for the offsets in raster order, zero padding."""
    g = gray(x)
    H, W = g.shape[1:]
    p = F.pad(g, (RADIUS,) * 4)
    side = 2 * RADIUS + 1
    d = torch.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(side) for dx in range(side)], 1) - g[:, None]
    return d / torch.sqrt(0.81 + d * d)


def census_map(sr, hr):
    """[N,H,W]: m(p) c(p)."""
    delta = (ternary(sr) - ternary(hr)) ** 2
    c = (delta / (0.1 + delta)).mean(1)
    m = torch.zeros_like(c)
    m[:, 1:-1, 1:-1] = 1
    return m * c


def census_rows(sr, hr):
    """[N,C,H,W] x [N,C,H,W] -> [N]: what N calls on the N = 1 slices give.  Any float dtype, differentiable."""
    check_shape(*sr.shape[1:])
    return census_map(sr, hr).flatten(1).mean(1)


def census(sr, hr):
    """The one-value form: the mean of census_rows."""
    return census_rows(sr, hr).mean()


def census_grad_rows(sr, hr, g):
    """d (sum_r g[r] census_rows[r]) / d sr by autograd in float64."""
    x = sr.double().clone().requires_grad_()
    rows = census_rows(x, hr.double())
    return torch.autograd.grad(rows, x, torch.as_tensor(g, dtype=torch.float64).reshape(-1))[0]


def census_and_grad(sr, hr):
    """(value, d value / d sr) of the one-value form, float64."""
    x = sr.double().clone().requires_grad_()
    v = census(x, hr.double())
    return v.detach(), torch.autograd.grad(v, x)[0]


def composed_f32(sr, hr):
    """The fp32 composition on the CPU, value per row and gradient for cotangent ones: the yardstick whose own error sets the gates."""
    x = sr.float().clone().requires_grad_()
    rows = census_rows(x, hr.float())
    return rows.detach(), torch.autograd.grad(rows.sum(), x)[0]
