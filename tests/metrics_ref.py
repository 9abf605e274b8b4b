"""Float64 restatement of the PSNR / SSIM evaluation metric, plus the seeded inputs of the metric tests.

What the reference's ``utils.calc_metrics`` computes for a pair of unit-range images (utils.py:171-204, pytorch_msssim/__init__.py:19-75),
written out again rather than imported, so that it runs where the reference is absent:

* ``q = img.mul(255).clamp(0, 255).round()`` in fp32, exactly as torch does it (one fp32 multiply, NaN passes the clamp, ties to even).
  The quantised values are integers: everything after this line is exact data.
* ``S = sum (q_p - q_t)^2``, an integer; ``mse = S / (65025 n)``, ``PSNR = -10 log10(mse + 1e-8)``.
* SSIM with ``val_range = 255``: the 11 x 11 window of tests/ssim_ref.py (its fp32 values, cast up), valid correlation, the five window sums,
  the map and its mean over C (H - 10) (W - 10) positions -- all in float64.
"""
import functools
import math

import numpy as np
import torch

from tests import ssim_ref as R

L = 255.0
KINDS = ('noise', 'smooth', 'near', 'wide', 'ties')          # the kinds with an error yardstick; 'same' is held to exact values
SEEDS = (0, 1, 2)
# (H, W): one SSIM position; two tiles across with a one-column remainder; two tile rows; ...; the two full sizes
TILE_SIZES = [(11, 11), (12, 75), (27, 75), (37, 53), (64, 64), (26, 140)]
FULL_SIZES = [(256, 448), (720, 1280)]


def quantize(x):
    """fp32 [..] in unit range -> fp32 integers 0 .. 255, torch's own arithmetic."""
    assert x.dtype == torch.float32
    return x.mul(255.0).clamp(0, 255).round()


def metric_rows(pred, tgt):
    """pred, tgt fp32 [rows,C,H,W] -> (S: list of int, mse: float64 [rows], ssim: float64 [rows]); a row with a NaN gives
    S = None, mse = ssim = NaN."""
    assert pred.dim() == 4 and pred.shape == tgt.shape and pred.shape[2] >= R.WIN and pred.shape[3] >= R.WIN
    qp, qt = quantize(pred).double(), quantize(tgt).double()
    w = R.window_2d(torch.float64)
    S, mse, ssim = [], [], []
    for r in range(pred.shape[0]):
        a, b = qp[r:r + 1], qt[r:r + 1]
        if bool(torch.isnan(a).any() | torch.isnan(b).any()):
            S.append(None)
            mse.append(float('nan'))
            ssim.append(float('nan'))
            continue
        s = int(((a - b) ** 2).to(torch.int64).sum())
        mu1, mu2, s1, s2, s12, C1, C2 = R._moments(a, b, L, w)
        smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        S.append(s)
        mse.append(s / (65025.0 * a.numel()))
        ssim.append(float(smap.mean()))
    return S, np.array(mse), np.array(ssim)


def psnr(mse):
    return -10 * math.log10(mse + 1e-8)


def _ties(rs, shape):
    """(k + 0.5) / 255 rounded to fp32 and its two fp32 neighbours: the products with 255 fall on, just below and just above a tie."""
    k = rs.randint(0, 255, size=shape)
    x = ((k + 0.5) / 255.0).astype(np.float32)
    step = rs.randint(-1, 2, size=shape)
    x = np.where(step < 0, np.nextafter(x, np.float32(-1)), np.where(step > 0, np.nextafter(x, np.float32(2)), x))
    return x.astype(np.float64)


def make_pair(kind, N, C, H, W, seed):
    """(pred, tgt) fp32 [N,C,H,W].  'noise', 'smooth', 'near', 'same': the unit-range pairs of tests/ssim_ref.make_pair;
    'wide': a smooth target stretched to [-0.25, 1.25] and a noisy copy as prediction (both clamps at work, +-inf in a corner);
    'ties': two independent images of tie values."""
    if kind in ('noise', 'smooth', 'near', 'same'):
        return R.make_pair(kind, 0, N, C, H, W, seed)
    rs = np.random.RandomState(1000 * seed + 11)
    if kind == 'wide':
        tgt = R._smooth(rs, N, C, H, W) * 1.5 - 0.25
        pred = tgt + 0.03 * rs.normal(size=(N, C, H, W))
        pred[:, 0, 0, 0], pred[:, 0, 0, 1] = np.inf, -np.inf
        tgt[:, 0, 1, 0], tgt[:, 0, 1, 1] = -np.inf, np.inf
    elif kind == 'ties':
        pred, tgt = _ties(rs, (N, C, H, W)), _ties(rs, (N, C, H, W))
    else:
        raise ValueError(kind)
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(tgt.astype(np.float32))


def case_name(kind, C, H, W, seed):
    return '%s_c%d_%dx%d_s%d' % (kind, C, H, W, seed)


@functools.lru_cache(maxsize=None)
def case(kind, N, C, H, W, seed):
    """(pred, tgt, S, mse64, ssim64) of a seeded case, computed once per process and shared: treat as read-only."""
    pred, tgt = make_pair(kind, N, C, H, W, seed)
    return (pred, tgt) + metric_rows(pred, tgt)
