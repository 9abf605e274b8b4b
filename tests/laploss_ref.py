"""Float64 restatement of the Laplacian-pyramid L1 term ``Lap`` of --loss.  There is no reference implementation: this file IS the
definition, and the kernels of csrc/laploss.hip, the composed form of hip_ops and the golden fixture are held to it.

``levels = L`` (2..5, default 5).  ``g = [1, 4, 6, 4, 1] / 16``, a 5 x 5 window ``g g^T`` per channel, borders by reflection (torch's
``reflect``, pad 2).  ``c_0 = sr - hr`` (the pyramid is linear: one pyramid of the difference, not two).  For ``s = 0 .. L - 2``:

* ``c_{s+1} = (G c_s)[::2, ::2]``, of size ``ceil(H_s / 2) x ceil(W_s / 2)``;
* ``b_s = c_s - 4 G z_s``, ``z_s`` an ``H_s x W_s`` map of zeros with ``c_{s+1}`` at the even positions;
* ``b_{L-1} = c_{L-1}``, the low-pass residual (a brightness offset is seen there).

``lap = sum_s 2^s sum |b_s| / n_0`` with ``n_0 = C H W`` per sample (``N C H W`` for the one-value form).  Gradient for ``sr`` only;
``sign(0) = 0``.  Every filtered level must have both sides >= 3 (reflection by 2): H, W >= 17 for five levels.
"""
import torch
import torch.nn.functional as F

K1 = torch.tensor([1., 4., 6., 4., 1.]) / 16
LEVELS = 5
MIN_BAND = 2.0 ** -18        # conditioning of a pair used for a gradient comparison, see min_band
VALUE_FLOOR = 4 * 2.0 ** -24
GRAD_FLOOR = 2.0 ** -20
SIZES = ((17, 17), (19, 34), (37, 53), (64, 64), (40, 300))
KINDS = ('noise', 'smooth', 'near')


def kinds_at(H, W):
    """The content kinds with a conditioned seed among 0..11 at this size (40 x 300: no smooth pair qualifies)."""
    return ('noise', 'near') if (H, W) == (40, 300) else KINDS


def level_sizes(H, W, levels=LEVELS):
    out = [(H, W)]
    for _ in range(levels - 1):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def check_shape(H, W, levels=LEVELS):
    if not 2 <= levels <= 5:
        raise ValueError("levels must be 2..5, got %r" % (levels,))
    for h, w in level_sizes(H, W, levels)[:-1]:
        if h < 3 or w < 3:
            raise ValueError("every filtered level needs both sides >= 3: %d x %d with %d levels reaches %d x %d" % (H, W, levels, h, w))


def gauss(x, scale=1.0):
    C = x.shape[1]
    k = (torch.outer(K1, K1) * scale).to(x.dtype).expand(C, 1, 5, 5)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode='reflect'), k, groups=C)


def bands(d, levels=LEVELS):
    out, c = [], d
    for s in range(levels - 1):
        down = gauss(c)[:, :, ::2, ::2]
        z = torch.zeros_like(c)
        z[:, :, ::2, ::2] = down
        out.append(c - gauss(z, 4.0))
        c = down
    return out + [c]


def lap_rows(sr, hr, levels=LEVELS):
    """[N,C,H,W] x [N,C,H,W] -> [N]: what N calls on the N = 1 slices give.  Any float dtype, differentiable."""
    check_shape(sr.shape[2], sr.shape[3], levels)
    d = sr - hr
    return sum(2.0 ** s * b.abs().flatten(1).sum(1) for s, b in enumerate(bands(d, levels))) / d[0].numel()


def lap(sr, hr, levels=LEVELS):
    """The one-value form: the mean of lap_rows (n_0 = N C H W)."""
    return lap_rows(sr, hr, levels).mean()


def lap_grad_rows(sr, hr, g, levels=LEVELS):
    """d (sum_r g[r] lap_rows[r]) / d sr by autograd in float64."""
    x = sr.double().clone().requires_grad_()
    rows = lap_rows(x, hr.double(), levels)
    return torch.autograd.grad(rows, x, torch.as_tensor(g, dtype=torch.float64).reshape(-1))[0]


def lap_and_grad(sr, hr, levels=LEVELS):
    """(value, d value / d sr) of the one-value form, float64."""
    x = sr.double().clone().requires_grad_()
    v = lap(x, hr.double(), levels)
    return v.detach(), torch.autograd.grad(v, x)[0]


def min_band(sr, hr, levels=LEVELS):
    """min |b_s| over all levels and elements / max |sr - hr|, in float64: how far the closest band element is from the kink of |.|.
    The gradient holds sign(b): an element closer to zero than fp32 rounding flips it for ANY fp32 evaluation, so pairs for gradient
    comparisons must have min_band >= MIN_BAND (about ten times the fp32 evaluation error of a band)."""
    d = sr.double() - hr.double()
    return float(min(b.abs().min() for b in bands(d, levels)) / d.abs().max())


def conditioned_pair(kind, N, C, H, W, levels=LEVELS, seeds=range(12)):
    """(seed, sr, hr): the first seed whose class-0 pair of tests/ssim_ref.make_pair meets the conditioning, None if there is none."""
    from tests.ssim_ref import make_pair
    for seed in seeds:
        sr, hr = make_pair(kind, 0, N, C, H, W, seed)
        if min_band(sr, hr, levels) >= MIN_BAND:
            return seed, sr, hr
    return None


def composed_f32(sr, hr, levels=LEVELS):
    """The fp32 composition on the CPU, value per row and gradient for cotangent ones: the yardstick whose own error sets the gates."""
    x = sr.float().clone().requires_grad_()
    rows = lap_rows(x, hr.float(), levels)
    return rows.detach(), torch.autograd.grad(rows.sum(), x)[0]
