"""Forward + backward of the SSIM loss term: the fused kernels (hip_ops.ssim_loss) against the composition from torch ops with
autograd (the formula of utils.ssim / pytorch_msssim with the data-dependent range decided on the host, as the reference does),
timed with HIP events, the two alternating in one process.

    python tools/ssim_loss_bench.py [--iters 200] [--trace]      # --trace: fused path only, few iterations (for rocprofv3 --kernel-trace)
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meta_interpolation_amd import hip_ops  # noqa: E402

SHAPES = [(1, 3, 256, 448), (8, 3, 256, 448), (1, 3, 720, 1280)]


def window(C, dev):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / 4.5) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(C, 1, 11, 11).contiguous().to(dev)


def composed(sr, hr, w):
    C = sr.shape[1]
    L = (255 if torch.max(sr) > 128 else 1) - (-1 if torch.min(sr) < -0.5 else 0)      # two host reads, like the reference
    mu1, mu2 = F.conv2d(sr, w, groups=C), F.conv2d(hr, w, groups=C)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(sr * sr, w, groups=C) - mu1_sq
    s2 = F.conv2d(hr * hr, w, groups=C) - mu2_sq
    s12 = F.conv2d(sr * hr, w, groups=C) - mu12
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    smap = ((2 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return (1 - smap.mean()) / 2


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
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--trace', action='store_true')
    o = ap.parse_args()
    dev = 'cuda'
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(0)
        hr = torch.rand(shape, generator=gen).to(dev)
        sr = (hr + 0.02 * torch.randn(shape, generator=gen).to(dev)).requires_grad_()
        w = window(shape[1], dev)

        def fused():
            loss = hip_ops.ssim_loss(sr, hr)
            return loss, torch.autograd.grad(loss, sr)[0]

        def torch_ops():
            loss = composed(sr, hr.clone(), w)
            return loss, torch.autograd.grad(loss, sr)[0]
        if o.trace:
            for _ in range(5):
                fused()
            torch.cuda.synchronize()
            continue
        (lf, gf), (lt, gt) = fused(), torch_ops()
        for _ in range(10):
            fused(), torch_ops()
        torch.cuda.synchronize()
        tf, tt = [], []
        for rep in range(5):          # alternate the two
            tf.append(timed(fused, o.iters))
            tt.append(timed(torch_ops, o.iters))
        print('%-18s fused %8.1f us (min of 5; %s)   torch ops %8.1f us (%s)   ratio %.1fx   |dloss| %.1e  grad max-rel diff %.1e' % (
            'x'.join(map(str, shape)), min(tf), ' '.join('%.1f' % t for t in tf), min(tt), ' '.join('%.1f' % t for t in tt),
            min(tt) / min(tf), abs(float(lf.detach()) - float(lt.detach())), float((gf - gt).abs().max() / gt.abs().max())), flush=True)


if __name__ == '__main__':
    main()
