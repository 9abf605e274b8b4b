"""tools/gen_golden_msssim.py -- TEST INFRASTRUCTURE.  Fixture of multi-scale SSIM, produced by IMPORTING the reference.

Runs on the CPU in the build container only (it needs the reference tree, through oracle.gen_golden's shims; nothing of the
reference is copied):

    python tools/gen_golden_msssim.py

tests/golden/msssim.npz: the reference's ``pytorch_msssim.msssim(img1, img2.clone(), normalize=...)`` in fp32 on the CPU, on the seeded
pairs of tests/ssim_ref.make_pair (the inputs are re-drawn from the seed, not stored), N = 1, C = 3.  Per case: the fp32 value, the
float64 restatement's value, a fingerprint of d value / d img1 (the whole gradient for some cases up to 64 x 64) and
``e_ref`` = |reference fp32 - float64 restatement| (value: absolute; gradient: max |diff| / max |float64 gradient|).  A case whose value is
NaN stores NaN for all of them.  ``E_<kind>_z<normalize>``: the largest finite e_ref of the kind over all sizes, classes and seeds.
(Without ``normalize`` autograd through the reference can give a NaN gradient next to a finite value: ``mssim ** weights`` is formed for
all five levels, and the zero cotangent of an unused entry with a negative base meets pow's NaN derivative.  Such a gradient e_ref is NaN.)
Further: pairs whose range class changes between levels, identical pairs, a batch of mixed classes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import msssim_ref as M  # noqa: E402
from tests import ssim_ref as R  # noqa: E402

SIZES = [(32, 32), (37, 53), (64, 64), (161, 176), (176, 176), (40, 300)]
SEEDS = (0, 1, 2)
# the whole gradient is stored for seed 0 of these (H, W) -> classes
FULL_GRAD = {(32, 32): (0, 1, 2, 3), (37, 53): (0,), (64, 64): (0,)}


def reference(fn, sr, hr, **kw):
    x = sr.clone().requires_grad_()
    out = fn(x, hr.clone(), **kw)
    grad, = torch.autograd.grad(out, x)
    return out.detach(), grad


def measure(fn, sr, hr, normalize):
    v32, g32 = reference(fn, sr, hr, normalize=normalize)
    v64, g64 = M.msssim_and_grad(sr.double(), hr.double(), None, normalize)
    if torch.isnan(v32) or torch.isnan(v64):
        return v32, g32, v64, g64, float('nan'), float('nan')
    e_v = abs(float(v32) - float(v64))
    e_g = float((g32.double() - g64).abs().max() / g64.abs().max())
    return v32, g32, v64, g64, e_v, e_g


def spike_pair(value, seed=0):
    """A `near` pair in [0, 1] at 64 x 64 with ONE element of the prediction set to `value`: its class on level 0 is the spike's, the
    pooled levels fall back to class 0."""
    sr, hr = R.make_pair('near', 0, 1, 3, 64, 64, seed)
    sr = sr.clone()
    sr[0, 1, 20, 30] = value
    return sr, hr


def main():
    torch.set_num_threads(8)
    G.install_shims()
    import pytorch_msssim
    fn = pytorch_msssim.msssim
    out = {'kinds': np.array(R.KINDS), 'seeds': np.array(SEEDS), 'sizes': np.array(SIZES)}
    names = []
    for kind in R.KINDS:
        for norm in (True, False):
            worst = np.zeros(2)
            for H, W in SIZES:
                for cls in range(4):
                    for seed in SEEDS:
                        sr, hr = R.make_pair(kind, cls, 1, 3, H, W, seed)
                        v32, g32, v64, g64, e_v, e_g = measure(fn, sr, hr, norm)
                        name = M.case_name(kind, cls, norm, 1, H, W, seed)
                        names.append(name)
                        out[name + '/value'] = np.float32(v32)
                        out[name + '/value64'] = np.float64(v64)
                        out[name + '/grad_fp'] = R.fingerprint(g32)
                        out[name + '/e_ref'] = np.array([e_v, e_g])
                        if seed == 0 and cls in FULL_GRAD.get((H, W), ()) and (norm or kind == 'near'):
                            out[name + '/grad'] = g32.numpy()
                        worst = np.fmax(worst, [e_v, e_g])      # finite figures only
                        print('  %-36s value %.8f  e_ref value %.2e grad %.2e' % (name, float(v32), e_v, e_g), flush=True)
            out['E_%s_z%d' % (kind, norm)] = worst
    # the class changes between the levels
    for tag, value, classes in (('spike200', 200.0, [2, 0, 0, 0, 0]), ('spikem06', -0.6, [1, 0, 0, 0, 0])):
        sr, hr = spike_pair(value)
        assert M.levels(sr.double(), hr.double())[2] == classes, tag
        for norm in (True, False):
            v32, g32, v64, g64, e_v, e_g = measure(fn, sr, hr, norm)
            name = '%s_z%d' % (tag, norm)
            out[name + '/value'] = np.float32(v32)
            out[name + '/value64'] = np.float64(v64)
            out[name + '/grad_fp'] = R.fingerprint(g32)
            out[name + '/e_ref'] = np.array([e_v, e_g])
            out[name + '/classes'] = np.array(classes)
            print('  %-36s value %.8f  e_ref value %.2e grad %.2e' % (name, float(v32), e_v, e_g), flush=True)
    # identical pair: the reference returns exactly 1 and a gradient that is pure rounding
    for H, W in SIZES:
        for cls in (0, 1):
            for norm in (True, False):
                sr, hr = R.make_pair('same', cls, 1, 3, H, W, 0)
                v32, g32 = reference(fn, sr, hr, normalize=norm)
                name = M.case_name('same', cls, norm, 1, H, W, 0)
                out[name + '/value'] = np.float32(v32)
                out[name + '/grad_maxabs'] = np.float64(g32.abs().max())
                print('  %-36s value %.9f  max |grad| %.3e' % (name, float(v32), float(g32.abs().max())), flush=True)
    # a batch whose rows fall in different classes: per-row values and the whole-batch value
    for seed in SEEDS:
        sr, hr = R.make_pair('near', [0, 2, 1], 3, 3, 64, 64, seed)
        for norm in (True, False):
            name = 'mixed_z%d_s%d' % (norm, seed)
            out[name + '/rows'] = np.array([float(fn(sr[i:i + 1], hr[i:i + 1].clone(), normalize=norm)) for i in range(3)], dtype=np.float32)
            out[name + '/value'] = np.float32(fn(sr, hr.clone(), normalize=norm))
    out['names'] = np.array(names)
    for kind in R.KINDS:
        for norm in (1, 0):
            e = out['E_%s_z%d' % (kind, norm)]
            print('  E_%-6s normalize %d  value %.3e  grad %.3e' % (kind, norm, e[0], e[1]))
    path = os.path.join(G.GOLD, 'msssim.npz')
    np.savez_compressed(path, **out)
    print('  msssim.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
