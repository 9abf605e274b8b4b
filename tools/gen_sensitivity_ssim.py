"""tools/gen_sensitivity_ssim.py -- TEST INFRASTRUCTURE.  The reference's own numerical spread on the SSIM-loss system fixtures.

    python tools/gen_sensitivity_ssim.py [--only case ...]      # writes tests/golden/sensitivity_ssim.npz

oracle/gen_sensitivity.py, imported, applied to the cases of tools/gen_golden_ssim.py (added to the oracle's case table at run
time): the imported reference against ITSELF under two other convolution summation orders and in float64, in the
normalisation of the GPU parity tests.  Same layout as tests/golden/sensitivity.npz; tests/test_ssim_system_gpu.py gates at
max(contract bound, K_SPREAD x this spread), as tests/test_system_gpu.py does for its cases.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402
from oracle import gen_sensitivity as S  # noqa: E402
from tools.gen_golden_ssim import SYSTEM_CASES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    opts = ap.parse_args()
    torch.set_num_threads(8)
    G.install_shims()
    G.SYSTEM_CASES.update(SYSTEM_CASES)
    path = os.path.join(G.GOLD, 'sensitivity_ssim.npz')
    out = dict(np.load(path)) if os.path.exists(path) else {}
    out['variants'] = np.array(S.VARIANTS)
    out['quantities'] = np.array(S.QUANT)
    for name in (opts.only or list(SYSTEM_CASES)):
        fx = np.load(os.path.join(G.GOLD, 'system_%s.npz' % name))
        for phase in ('train', 'val'):
            base = S.run_variant(name, 'base', phase)
            # the float32 run must BE the committed fixture
            assert abs(base['loss'] - float(fx[phase + '_loss'])) <= 1e-7 * abs(base['loss']), (name, phase, base['loss'])
            assert np.abs(base['preds'] - fx[phase + '_preds']).max() <= 1e-6, (name, phase)
            table = np.zeros((len(S.VARIANTS), len(S.QUANT)))
            for vi, variant in enumerate(S.VARIANTS):
                d = S.deviations(base, S.run_variant(name, variant, phase))
                table[vi] = [d[q] for q in S.QUANT]
                print('  %-36s %-5s %-8s ' % (name, phase, variant) + ' '.join('%s=%.2e' % (q, d[q]) for q in S.QUANT), flush=True)
            out['%s/%s' % (name, phase)] = table
        np.savez_compressed(path, **out)


if __name__ == '__main__':
    main()
