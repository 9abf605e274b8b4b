"""Restatement of the reference's multi-scale SSIM "as implemented" (pytorch_msssim/__init__.py:78-104 over :19-75), in any float
dtype: float64 is the yardstick of the kernels, float32 repeats the reference's own arithmetic.  Written out again rather than
imported, so that it runs where the reference is absent.

* five levels; level s works on the pair pooled s times by ``avg_pool2d(., (2, 2))`` (floor: an odd last row / column is dropped);
  the reference pools once more after the fifth level, so H, W >= 32;
* the window of a level: n = min(11, H_s, W_s) taps ``exp(-(i - n // 2)^2 / 4.5)`` (double -> fp32, normalised in fp32), outer product
  in fp32, valid correlation.  These fp32 values are data: the float64 statement casts them up;
* ``cs_s = mean(v1 / v2)``, ``ssim_s = mean(map)`` over the whole tensor, ``v1 = 2 s12 + C2``, ``v2 = s1 + s2 + C2``;
* the dynamic range L is decided again on EVERY level from that level's img1 (``val_range=None``):
  ``(255 if max > 128 else 1) - (-1 if min < -0.5 else 0)``; a given ``val_range`` holds on every level;
* ``normalize``: every mean m -> (m + 1) / 2;
* result ``prod(cs[:4] ** w[:4] * ssim[4] ** w[4])`` = ``ssim_4 ** (4 w_4) * prod_{s<4} cs_s ** w_s`` with the fp32 weights
  0.0448, 0.2856, 0.3001, 0.2363, 0.1333: the last level's SSIM enters FOUR times, cs_4 and ssim_0..3 not at all.  A negative base
  gives NaN.
"""
import math

import torch
import torch.nn.functional as F

from tests import ssim_ref as R

LEVELS = 5
MIN_SIZE = 32
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
KINDS = R.KINDS
VAL_RANGES = {1: 0, 2: 1, 255: 2, 256: 3}       # val_range -> range class


def weights(dtype):
    return torch.tensor(WEIGHTS, dtype=torch.float32).to(dtype)      # fp32 values, cast up


def taps_f32(n):
    g = torch.tensor([math.exp(-(x - n // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(n)], dtype=torch.float32)
    return g / g.sum()


def window_2d(n, dtype):
    g = taps_f32(n).unsqueeze(1)
    return g.mm(g.t()).to(dtype)


def level_sizes(H, W):
    return [(H >> s, W >> s) for s in range(LEVELS)]


def level_taps(H, W):
    return [min(R.WIN, h, w) for h, w in level_sizes(H, W)]


def _level(x, y, L):
    """(mean SSIM map, mean v1 / v2) of one level."""
    C = x.shape[1]
    n = min(R.WIN, x.shape[2], x.shape[3])
    w = window_2d(n, x.dtype).expand(C, 1, n, n).contiguous()

    def conv(t):
        return F.conv2d(t, w, groups=C)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu12
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
    cs = torch.mean(v1 / v2)
    smap = ((2 * mu12 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)
    return smap.mean(), cs


def levels(img1, img2, val_range=None):
    """-> (ssim [5], cs [5], classes [5]): the plain means of every level and the range class it took (None for a given range)."""
    assert img1.dim() == 4 and img1.shape == img2.shape
    if img1.shape[2] < MIN_SIZE or img1.shape[3] < MIN_SIZE:
        raise ValueError("msssim needs H, W >= 32: the reference pools once more after its fifth level")
    ms, mc, classes = [], [], []
    for _ in range(LEVELS):
        if val_range is None:
            cls = R.range_class(img1.detach())
            L = R.CLASS_L[cls]
        else:
            cls, L = None, val_range
        s, c = _level(img1, img2, L)
        ms.append(s)
        mc.append(c)
        classes.append(cls)
        img1, img2 = F.avg_pool2d(img1, (2, 2)), F.avg_pool2d(img2, (2, 2))
    return torch.stack(ms), torch.stack(mc), classes


def combine(ms, mc, normalize=False):
    """The reference's last four lines."""
    w = weights(ms.dtype)
    if normalize:
        ms, mc = (ms + 1) / 2, (mc + 1) / 2
    return torch.prod((mc ** w)[:-1] * (ms ** w)[-1])


def combine_textbook(ms, mc, normalize=False):
    """NOT what the reference computes: Wang et al.'s product, the last SSIM entering once.  Kept to show that the tests tell them apart."""
    w = weights(ms.dtype)
    if normalize:
        ms, mc = (ms + 1) / 2, (mc + 1) / 2
    return torch.prod((mc ** w)[:-1]) * (ms ** w)[-1]


def bases(ms, mc, normalize=False):
    """The five bases that enter the product: cs_0..3 and ssim_4 (normalised if asked)."""
    b = torch.cat([mc[:-1], ms[-1:]])
    return (b + 1) / 2 if normalize else b


def msssim(img1, img2, val_range=None, normalize=False):
    """[N,C,H,W] x [N,C,H,W] -> scalar over the whole tensor (size_average=True); differentiable."""
    ms, mc, _ = levels(img1, img2, val_range)
    return combine(ms, mc, normalize)


def msssim_and_grad(img1, img2, val_range=None, normalize=False, g=1.0):
    x = img1.clone().requires_grad_()
    out = msssim(x, img2, val_range, normalize)
    grad, = torch.autograd.grad(out, x)
    return out.detach(), g * grad


def msssim_rows(img1, img2, val_range=None, normalize=False):
    """What N calls on the N = 1 slices give."""
    return torch.stack([msssim(img1[i:i + 1], img2[i:i + 1], val_range, normalize) for i in range(img1.shape[0])])


def msssim_grad_rows(img1, img2, g, val_range=None, normalize=False):
    return torch.cat([msssim_and_grad(img1[i:i + 1], img2[i:i + 1], val_range, normalize, float(g[i]))[1] for i in range(img1.shape[0])])


def quantize(x01):
    """utils.quantize(img, 1.) in the image's own precision (fp32 inputs: one fp32 multiply, ties to even)."""
    return x01.mul(255).clamp(0, 255).round()


def metric_rows(pred01, tgt01, dtype=torch.float64):
    """msssim(quantize(pred), quantize(target), val_range=255) of every row on its own."""
    return msssim_rows(quantize(pred01).to(dtype), quantize(tgt01).to(dtype), val_range=255)


def case_name(kind, cls, norm, N, H, W, seed):
    return '%s_c%d_z%d_n%d_%dx%d_s%d' % (kind, cls, int(norm), N, H, W, seed)


def parse_case(name):
    kind, cls, norm, n, size, seed = name.split('_')
    H, W = size.split('x')
    return kind, int(cls[1:]), bool(int(norm[1:])), int(n[1:]), int(H), int(W), int(seed[1:])
