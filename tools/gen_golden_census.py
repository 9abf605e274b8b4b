"""tools/gen_golden_census.py -- TEST INFRASTRUCTURE.  Fixture of the census loss term.  CPU only; nothing is imported from the
reference (it has no such term: tests/census_ref.py is the definition).

    python tools/gen_golden_census.py

tests/golden/census.npz, on the seeded class-0 pairs of tests/ssim_ref.make_pair (re-drawn from the seed, not stored), N = 1, C = 3.
For every size of census_ref.SIZES and every content kind of census_ref.KINDS: the seed (``<case>/seed``), the float64 value
(``/value64``), the value of the fp32 composition of the same operations on the CPU (``/value``), a fingerprint of the float64 gradient
(``/grad64_fp``) and ``/e_ref`` = |fp32 composition - float64| (value: absolute; gradient: max |diff| / max |float64 gradient|).
``E_<kind>``: the largest e_ref of the kind over the sizes.  The kernels are held to max(3 E_kind, floor).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from tests import census_ref as Z  # noqa: E402
from tests import ssim_ref as R  # noqa: E402


def case_name(kind, H, W):
    return '%s_%dx%d' % (kind, H, W)


def main():
    torch.set_num_threads(8)
    out = {'sizes': np.array(Z.SIZES), 'kinds': np.array(Z.KINDS)}
    worst = {kind: np.zeros(2) for kind in Z.KINDS}
    names = []
    for H, W in Z.SIZES:
        for kind in Z.KINDS:
            sr, hr = R.make_pair(kind, 0, 1, 3, H, W, Z.SEED)
            v64, g64 = Z.census_and_grad(sr, hr)
            v32, g32 = Z.composed_f32(sr, hr)
            e_v = abs(float(v32[0]) - float(v64))
            e_g = float((g32.double() - g64).abs().max() / g64.abs().max())
            name = case_name(kind, H, W)
            names.append(name)
            out[name + '/seed'] = np.int64(Z.SEED)
            out[name + '/value64'] = np.float64(v64)
            out[name + '/value'] = np.float32(v32[0])
            out[name + '/grad64_fp'] = R.fingerprint(g64)
            out[name + '/e_ref'] = np.array([e_v, e_g])
            worst[kind] = np.fmax(worst[kind], [e_v, e_g])
            print('  %-16s seed %2d value %.8f  e_ref value %.2e grad %.2e' % (name, Z.SEED, float(v64), e_v, e_g), flush=True)
    for kind in Z.KINDS:
        out['E_' + kind] = worst[kind]
        print('  E_%-6s value %.3e  grad %.3e' % (kind, worst[kind][0], worst[kind][1]))
    out['names'] = np.array(names)
    path = os.path.join(REPO, 'tests', 'golden', 'census.npz')
    np.savez_compressed(path, **out)
    print('  census.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
