"""Multi-scale SSIM, forward and forward + backward: the fused kernels (hip_ops.msssim) against the composition from ATen ops with
autograd (the formula of pytorch_msssim.msssim: per level five depth-wise convolutions with the outer-product window, the range of
every level decided on the host as the reference does, avg_pool2d between the levels), timed with HIP events, the two alternating in
one process.  normalize=True, as the MSSSIM term of --loss calls it.

    python tools/msssim_bench.py [--iters 100]
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meta_interpolation_amd import hip_ops  # noqa: E402

SHAPES = [(1, 3, 256, 448), (1, 3, 720, 1280)]
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(n, C, dev):
    g = torch.tensor([math.exp(-(x - n // 2) ** 2 / 4.5) for x in range(n)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(C, 1, n, n).contiguous().to(dev)


def composed(x, y, windows, wts):
    C = x.shape[1]
    ms, mc = [], []
    for _ in range(5):
        L = (255 if torch.max(x) > 128 else 1) - (-1 if torch.min(x) < -0.5 else 0)      # two host reads per level, like the reference
        w = windows[min(11, x.shape[2], x.shape[3])]
        mu1, mu2 = F.conv2d(x, w, groups=C), F.conv2d(y, w, groups=C)
        mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = F.conv2d(x * x, w, groups=C) - mu1_sq
        s2 = F.conv2d(y * y, w, groups=C) - mu2_sq
        s12 = F.conv2d(x * y, w, groups=C) - mu12
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        v1, v2 = 2.0 * s12 + C2, s1 + s2 + C2
        mc.append(torch.mean(v1 / v2))
        ms.append((((2 * mu12 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)).mean())
        x, y = F.avg_pool2d(x, (2, 2)), F.avg_pool2d(y, (2, 2))
    ms, mc = (torch.stack(ms) + 1) / 2, (torch.stack(mc) + 1) / 2
    return torch.prod((mc ** wts)[:-1] * (ms ** wts)[-1])


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    o = ap.parse_args()
    dev = 'cuda'
    wts = torch.tensor(WEIGHTS, device=dev)
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(0)
        hr = torch.rand(shape, generator=gen).to(dev)
        sr = (hr + 0.02 * torch.randn(shape, generator=gen).to(dev)).requires_grad_()
        windows = {n: window(n, shape[1], dev) for n in range(1, 12)}
        runs = {
            'fwd': (lambda: hip_ops.msssim(sr.detach(), hr, normalize=True),
                    lambda: composed(sr.detach(), hr, windows, wts)),
            'fwd+bwd': (lambda: torch.autograd.grad(hip_ops.msssim(sr, hr, normalize=True), sr)[0],
                        lambda: torch.autograd.grad(composed(sr, hr, windows, wts), sr)[0]),
        }
        dv = abs(float(runs['fwd'][0]()) - float(runs['fwd'][1]()))
        gf, gt = runs['fwd+bwd'][0](), runs['fwd+bwd'][1]()
        dg = float((gf - gt).abs().max() / gt.abs().max())
        for what, (fused, aten) in runs.items():
            for _ in range(10):
                fused(), aten()
            torch.cuda.synchronize()
            tf, tt = [], []
            for rep in range(5):          # alternate the two
                tf.append(timed(fused, o.iters))
                tt.append(timed(aten, o.iters))
            print('%-14s %-8s fused %8.1f us (min of 5; %s)   ATen ops %8.1f us (%s)   ratio %.1fx   |dvalue| %.1e  grad max-rel diff %.1e' % (
                'x'.join(map(str, shape)), what, min(tf), ' '.join('%.1f' % t for t in tf), min(tt), ' '.join('%.1f' % t for t in tt),
                min(tt) / min(tf), dv, dg), flush=True)


if __name__ == '__main__':
    main()
