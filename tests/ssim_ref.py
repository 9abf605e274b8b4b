"""Float64 restatement of the SSIM loss term and its analytic gradient, plus the seeded inputs of the SSIM tests.

What the reference's ``Loss`` computes for ``'SSIM'`` (loss.py:294 constructs ``pytorch_msssim.SSIM``; pytorch_msssim/__init__.py:7-131),
written out again rather than imported, so that it runs where the reference is absent:

* window: 11 taps of a Gaussian with sigma 1.5, exp in double precision, rounded to fp32, normalised in fp32, outer product
  in fp32 (:7-16).  The float64 statement uses exactly those fp32 window values (they are data), cast up.
* depthwise, valid correlation: an H x W plane gives (H - 10) x (W - 10) values (:40-49);
* ``map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))``, ``C1 = (0.01 L)^2``, ``C2 = (0.03 L)^2`` (:55-62);
* ``L`` from the PREDICTION's data on every call (:21-31; SSIM.forward never hands ``val_range`` on, :129):
  ``(255 if max > 128 else 1) - (-1 if min < -0.5 else 0)``;
* loss = (1 - mean(map)) / 2 (:130).

Gradient (``sr`` only), per output pixel with ``A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2``:

    b = d map / d s1  = -map / B2
    c = d map / d s12 = 2 A1 / (B1 B2)
    m = d map / d mu1 (s1, s12 fixed) = 2 mu2 A2 / (B1 B2) - 2 mu1 map / B1
    a = m - 2 mu1 b - mu2 c            (s1 = E[x^2] - mu1^2 and s12 = E[xy] - mu1 mu2 depend on mu1 too)
    d loss / d sr = -(g / (2 n_out)) * (G^T[a] + 2 sr G^T[b] + hr G^T[c])

with ``G^T`` the adjoint (full) correlation of the window.  ``ssim_loss_grad`` is held to autograd's gradcheck in
tests/test_ssim_ref_cpu.py.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIN = 11
HALO = WIN - 1
KINDS = ('noise', 'smooth', 'near')
# range class = bit 0: min(sr) < -0.5, bit 1: max(sr) > 128
CLASS_L = (1.0, 2.0, 255.0, 256.0)


def taps_f32():
    """The 11 fp32 taps (double exp -> fp32 -> normalised in fp32)."""
    g = torch.tensor([math.exp(-(x - WIN // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(WIN)], dtype=torch.float32)
    return g / g.sum()


def window_2d(dtype=torch.float64):
    g = taps_f32().unsqueeze(1)
    return g.mm(g.t()).to(dtype)      # fp32 outer product, then cast


def range_class(sr):
    return int(bool(sr.min() < -0.5)) + 2 * int(bool(sr.max() > 128))


def _conv(x, w2d):
    C = x.shape[1]
    return F.conv2d(x, w2d.expand(C, 1, WIN, WIN), groups=C)


def _conv_t(x, w2d):
    C = x.shape[1]
    return F.conv_transpose2d(x, w2d.expand(C, 1, WIN, WIN), groups=C)


def _moments(sr, hr, L, w):
    mu1, mu2 = _conv(sr, w), _conv(hr, w)
    s1 = _conv(sr * sr, w) - mu1 * mu1
    s2 = _conv(hr * hr, w) - mu2 * mu2
    s12 = _conv(sr * hr, w) - mu1 * mu2
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    return mu1, mu2, s1, s2, s12, C1, C2


def ssim_loss(sr, hr, L=None):
    """[N,C,H,W] x [N,C,H,W] -> scalar, the rule (or the given L) over the whole tensor; any float dtype, differentiable."""
    assert sr.dim() == 4 and sr.shape == hr.shape and sr.shape[2] >= WIN and sr.shape[3] >= WIN
    if L is None:
        L = CLASS_L[range_class(sr.detach())]
    mu1, mu2, s1, s2, s12, C1, C2 = _moments(sr, hr, L, window_2d(sr.dtype))
    ssim_map = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return (1 - ssim_map.mean()) / 2


def ssim_loss_grad(sr, hr, g=1.0, L=None):
    """d (g * ssim_loss(sr, hr)) / d sr by the closed form in the module docstring."""
    if L is None:
        L = CLASS_L[range_class(sr)]
    w = window_2d(sr.dtype)
    mu1, mu2, s1, s2, s12, C1, C2 = _moments(sr, hr, L, w)
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    smap = A1 * A2 / (B1 * B2)
    b = -smap / B2
    c = 2 * A1 / (B1 * B2)
    m = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * smap / B1
    a = m - 2 * mu1 * b - mu2 * c
    return -(g / (2.0 * smap.numel())) * (_conv_t(a, w) + 2 * sr * _conv_t(b, w) + hr * _conv_t(c, w))


def ssim_loss_rows(sr, hr):
    """What N calls on the N = 1 slices give: ([N] losses, [N] classes)."""
    return (torch.stack([ssim_loss(sr[i:i + 1], hr[i:i + 1]) for i in range(sr.shape[0])]),
            [range_class(sr[i]) for i in range(sr.shape[0])])


def ssim_loss_grad_rows(sr, hr, g):
    return torch.cat([ssim_loss_grad(sr[i:i + 1], hr[i:i + 1], float(g[i])) for i in range(sr.shape[0])])


# ------------------------------------------------------------------------------------------------------------------------
# seeded inputs (numpy float64 arithmetic rounded to fp32 once: the same bits wherever they are drawn)
# ------------------------------------------------------------------------------------------------------------------------
def _cubic_matrix(n_out, n_in):
    """[n_out, n_in] Keys (a = -0.5) cubic interpolation weights, align-corners sampling, border taps clamped."""
    A = np.zeros((n_out, n_in))
    for i in range(n_out):
        x = i * (n_in - 1) / max(n_out - 1, 1)
        x0 = int(np.floor(x))
        for k in range(-1, 3):
            d = abs(x - (x0 + k))
            wgt = (1.5 * d ** 3 - 2.5 * d ** 2 + 1) if d <= 1 else (-0.5 * d ** 3 + 2.5 * d ** 2 - 4 * d + 2) if d < 2 else 0.0
            A[i, min(max(x0 + k, 0), n_in - 1)] += wgt
    return A


def _smooth(rs, N, C, H, W):
    h, w = H // 8 + 3, W // 8 + 3
    low = rs.uniform(size=(N, C, h, w))
    up = np.matmul(np.matmul(_cubic_matrix(H, h), low), _cubic_matrix(W, w).T)      # rows, then columns
    lo = up.min(axis=(1, 2, 3), keepdims=True)
    hi = up.max(axis=(1, 2, 3), keepdims=True)
    return np.clip((up - lo) / (hi - lo), 0.0, 1.0)     # every sample spans exactly [0, 1]


def _to_class(x, cls):
    """[0, 1]-based data moved into range class `cls`."""
    return {0: x, 1: x * 2.0 - 1.0, 2: x * 255.0, 3: x * 256.0 - 1.0}[cls]


def make_pair(kind, classes, N, C, H, W, seed):
    """(sr, hr) fp32 [N,C,H,W]; classes: one class for all samples or one per sample.  'noise': two independent uniform images;
    'smooth': two independent smooth images; 'near': a smooth target and the target + 0.02 sigma noise (clipped to the range) as prediction;
    'same': sr == hr (smooth)."""
    if isinstance(classes, int):
        classes = [classes] * N
    rs = np.random.RandomState(1000 * seed + 7)
    if kind == 'noise':
        sr, hr = rs.uniform(size=(N, C, H, W)), rs.uniform(size=(N, C, H, W))
        sr[:, 0, 0, 0], sr[:, 0, 0, 1] = 0.0, 1.0       # the prediction spans [0, 1]: the class is the one asked for
    elif kind == 'smooth':
        sr, hr = _smooth(rs, N, C, H, W), _smooth(rs, N, C, H, W)
    elif kind == 'near':
        hr = _smooth(rs, N, C, H, W)
        sr = np.clip(hr + 0.02 * rs.normal(size=(N, C, H, W)), 0.0, 1.0)
        flat_sr, flat_hr = sr.reshape(N, -1), hr.reshape(N, -1)
        for i in range(N):        # noise-free where the target has its extremes: the prediction spans [0, 1], the class is the one asked for
            flat_sr[i, flat_hr[i].argmin()], flat_sr[i, flat_hr[i].argmax()] = 0.0, 1.0
    elif kind == 'same':
        hr = _smooth(rs, N, C, H, W)
        sr = hr.copy()
    else:
        raise ValueError(kind)
    for i, c in enumerate(classes):
        sr[i], hr[i] = _to_class(sr[i], c), _to_class(hr[i], c)
    sr, hr = torch.from_numpy(sr.astype(np.float32)), torch.from_numpy(hr.astype(np.float32))
    for i, c in enumerate(classes):
        assert range_class(sr[i]) == c, (kind, c, float(sr[i].min()), float(sr[i].max()))
    return sr, hr


def fingerprint(t):
    t = t.detach().double().reshape(-1)
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()] + t[:4].tolist())


def case_name(kind, cls, N, H, W, seed):
    return '%s_c%d_n%d_%dx%d_s%d' % (kind, cls, N, H, W, seed)
