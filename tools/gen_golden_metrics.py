"""tools/gen_golden_metrics.py -- TEST INFRASTRUCTURE.  Fixture of the PSNR / SSIM metric, produced by IMPORTING the reference.

Runs on the CPU in the build container only (it needs the reference tree, through oracle.gen_golden's shims; nothing of the
reference is copied):

    python tools/gen_golden_metrics.py              # tests/golden/metrics.npz (scalars only)

The reference's ``utils.calc_metrics(pred, gt)`` (utils.py:195-204) in fp32 on the CPU, on the seeded pairs of
tests/metrics_ref.make_pair (the inputs are re-drawn from the seed, not stored).  Per case: the reference's fp32 PSNR and SSIM, the
float64 restatement's values and the integer S, and ``e_ref`` = |reference fp32 SSIM - float64 SSIM|.  Per kind: ``E_kind`` = the
largest ``e_ref`` over all sizes, channel counts and seeds 0..2 -- the yardstick the kernel's gate is derived from.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from tests import metrics_ref as M  # noqa: E402

# (C, H, W): every size at C = 3 (what calc_metrics is called on), the tile-boundary sizes at C = 1 too
CASES = [(3, H, W) for H, W in M.TILE_SIZES + M.FULL_SIZES] + [(1, H, W) for H, W in M.TILE_SIZES]


def cases_of_kind(kind):
    import utils as ref_utils           # the reference's (the shims put its tree first on sys.path)
    torch.set_num_threads(4)
    out, names, worst = {}, [], 0.0
    for C, H, W in CASES:
        for seed in M.SEEDS:
            pred, tgt = M.make_pair(kind, 1, C, H, W, seed)
            psnr32, ssim32 = ref_utils.calc_metrics(pred[0], tgt[0])
            S, mse64, ssim64 = M.metric_rows(pred, tgt)
            name = M.case_name(kind, C, H, W, seed)
            names.append(name)
            e_ref = abs(float(ssim32) - float(ssim64[0]))
            out[name + '/psnr'] = np.float32(psnr32)
            out[name + '/ssim'] = np.float32(ssim32)
            out[name + '/psnr64'] = np.float64(M.psnr(mse64[0]))
            out[name + '/ssim64'] = np.float64(ssim64[0])
            out[name + '/S'] = np.int64(S[0])
            out[name + '/e_ref'] = np.float64(e_ref)
            if kind != 'same':
                worst = max(worst, e_ref)
            print('  %-28s psnr %.5f ssim %.8f  S %d  e_ref %.2e' % (name, psnr32, float(ssim32), S[0], e_ref), flush=True)
    out['E_' + kind] = np.float64(worst)
    return out, names


def main():
    import multiprocessing
    G.install_shims()
    kinds = M.KINDS + ('same',)
    out = {'kinds': np.array(M.KINDS), 'seeds': np.array(M.SEEDS)}
    names = []
    with multiprocessing.get_context('fork').Pool(len(kinds)) as pool:        # one process per content kind
        for part, part_names in pool.map(cases_of_kind, kinds):
            out.update(part)
            names += part_names
    out['names'] = np.array(names)
    for kind in M.KINDS:
        print('  E_%-6s %.3e' % (kind, out['E_' + kind]))
    path = os.path.join(G.GOLD, 'metrics.npz')
    np.savez_compressed(path, **out)
    print('  metrics.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
