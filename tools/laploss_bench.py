"""The Laplacian-pyramid loss term, forward and forward + backward: the fused kernels (hip_ops.lap_loss) against the composition from
ATen ops with autograd (per level: reflect pad, depth-wise 5 x 5 convolution, strided slice, zero fill, pad and convolution again,
subtraction, abs, sum -- on the difference sr - hr, the same formula as tests/laploss_ref.py in fp32), timed with HIP events, the two
alternating in one process.  Five levels, as the Lap term of --loss calls it.  Writes profiles/laploss_bench.txt.

    python tools/laploss_bench.py [--iters 100] [--out profiles/laploss_bench.txt]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from meta_interpolation_amd import hip_ops  # noqa: E402

SHAPES = [(1, 3, 256, 448), (1, 3, 720, 1280)]
LEVELS = 5


def composed(sr, hr, k1, k4):
    C = sr.shape[1]
    c = sr - hr
    n0 = c.numel()
    total = 0
    for s in range(LEVELS - 1):
        down = F.conv2d(F.pad(c, (2, 2, 2, 2), mode='reflect'), k1, groups=C)[:, :, ::2, ::2]
        z = torch.zeros_like(c)
        z[:, :, ::2, ::2] = down
        total = total + 2.0 ** s * (c - F.conv2d(F.pad(z, (2, 2, 2, 2), mode='reflect'), k4, groups=C)).abs().sum()
        c = down
    return (total + 2.0 ** (LEVELS - 1) * c.abs().sum()) / n0


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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'laploss_bench.txt'))
    o = ap.parse_args()
    dev = 'cuda'
    g = torch.tensor([1., 4., 6., 4., 1.]) / 16
    lines = []
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(0)
        hr = torch.rand(shape, generator=gen).to(dev)
        sr = (hr + 0.02 * torch.randn(shape, generator=gen).to(dev)).requires_grad_()
        k1 = torch.outer(g, g).expand(shape[1], 1, 5, 5).contiguous().to(dev)
        k4 = 4 * k1
        runs = {
            'fwd': (lambda: hip_ops.lap_loss(sr.detach(), hr), lambda: composed(sr.detach(), hr, k1, k4)),
            'fwd+bwd': (lambda: torch.autograd.grad(hip_ops.lap_loss(sr, hr), sr)[0],
                        lambda: torch.autograd.grad(composed(sr, hr, k1, k4), sr)[0]),
        }
        dv = abs(float(runs['fwd'][0]()) - float(runs['fwd'][1]()))
        gf, gt = runs['fwd+bwd'][0](), runs['fwd+bwd'][1]()
        # random content is not conditioned: a band within fp32 rounding of zero may take another sign in the two evaluations
        differ = int(((gf - gt).abs() > 2.0 ** -20 * gt.abs().max()).sum())
        for what, (fused, aten) in runs.items():
            for _ in range(10):
                fused(), aten()
            torch.cuda.synchronize()
            tf, tt = [], []
            for rep in range(5):          # alternate the two
                tf.append(timed(fused, o.iters))
                tt.append(timed(aten, o.iters))
            lines.append('%-14s %-8s fused %8.1f us (min of 5; %s)   ATen ops %8.1f us (%s)   ratio %.1fx   |dvalue| %.1e  gradient elements '
                         'apart %d of %d' % ('x'.join(map(str, shape)), what, min(tf), ' '.join('%.1f' % t for t in tf), min(tt),
                                             ' '.join('%.1f' % t for t in tt), min(tt) / min(tf), dv, differ, gt.numel()))
            print(lines[-1], flush=True)
    with open(o.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
