"""The census loss term, forward and forward + backward: the fused kernels (hip_ops.census_loss) against the composition from ATen ops
with autograd (gray, zero pad, 49 shifted slices stacked, the soft ternary, the robust distance, mean, mask, sum -- the same formula as
tests/census_ref.py in fp32), timed with HIP events, the two alternating in one process.  There is no speed gate.  Writes
profiles/census_bench.txt.

    python tools/census_bench.py [--iters 50] [--out profiles/census_bench.txt]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from meta_interpolation_amd import hip_ops  # noqa: E402

SHAPES = [(1, 3, 256, 448), (1, 3, 720, 1280)]


def composed(sr, hr):
    return hip_ops._census_composed(sr, hr).mean()


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
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'census_bench.txt'))
    o = ap.parse_args()
    dev = 'cuda'
    lines = []
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(0)
        hr = torch.rand(shape, generator=gen).to(dev)
        sr = (hr + 0.02 * torch.randn(shape, generator=gen).to(dev)).requires_grad_()
        runs = {
            'fwd': (lambda: hip_ops.census_loss(sr.detach(), hr), lambda: composed(sr.detach(), hr)),
            'fwd+bwd': (lambda: torch.autograd.grad(hip_ops.census_loss(sr, hr), sr)[0],
                        lambda: torch.autograd.grad(composed(sr, hr), sr)[0]),
        }
        dv = abs(float(runs['fwd'][0]()) - float(runs['fwd'][1]()))
        gf, gt = runs['fwd+bwd'][0](), runs['fwd+bwd'][1]()
        dg = float((gf - gt).abs().max() / gt.abs().max())
        for what, (fused, aten) in runs.items():
            for _ in range(5):
                fused(), aten()
            torch.cuda.synchronize()
            tf, tt = [], []
            for rep in range(5):          # alternate the two
                tf.append(timed(fused, o.iters))
                tt.append(timed(aten, o.iters))
            lines.append('%-14s %-8s fused %8.1f us (min of 5; %s)   ATen ops %8.1f us (%s)   ratio %.1fx   |dvalue| %.1e  max |dgrad| / max |grad| %.1e'
                         % ('x'.join(map(str, shape)), what, min(tf), ' '.join('%.1f' % t for t in tf), min(tt),
                            ' '.join('%.1f' % t for t in tt), min(tt) / min(tf), dv, dg))
            print(lines[-1], flush=True)
    with open(o.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
