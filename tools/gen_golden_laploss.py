"""tools/gen_golden_laploss.py -- TEST INFRASTRUCTURE.  Fixture of the Laplacian-pyramid loss term.  CPU only; nothing is imported from
the reference (it has no such term: tests/laploss_ref.py is the definition).

    python tools/gen_golden_laploss.py

tests/golden/laploss.npz, on the seeded class-0 pairs of tests/ssim_ref.make_pair (re-drawn from the seed, not stored), N = 1, C = 3,
five levels.  For every size of laploss_ref.SIZES and every content kind with a conditioned seed there (laploss_ref.kinds_at): the
first seed >= 0 whose pair has min_band >= 2^-18 in float64 (``<case>/seed``, ``<case>/min_band``), the float64 value
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

from tests import laploss_ref as L  # noqa: E402
from tests import ssim_ref as R  # noqa: E402


def case_name(kind, H, W):
    return '%s_%dx%d' % (kind, H, W)


def main():
    torch.set_num_threads(8)
    out = {'sizes': np.array(L.SIZES), 'kinds': np.array(L.KINDS)}
    worst = {kind: np.zeros(2) for kind in L.KINDS}
    names = []
    for H, W in L.SIZES:
        for kind in L.KINDS:
            found = L.conditioned_pair(kind, 1, 3, H, W)
            if kind not in L.kinds_at(H, W):
                assert found is None, (kind, H, W)          # the table of the kinds is the truth about seeds 0..11
                continue
            assert found is not None, (kind, H, W)
            seed, sr, hr = found
            v64, g64 = L.lap_and_grad(sr, hr)
            v32, g32 = L.composed_f32(sr, hr)
            e_v = abs(float(v32[0]) - float(v64))
            e_g = float((g32.double() - g64).abs().max() / g64.abs().max())
            name = case_name(kind, H, W)
            names.append(name)
            out[name + '/seed'] = np.int64(seed)
            out[name + '/min_band'] = np.float64(L.min_band(sr, hr))
            out[name + '/value64'] = np.float64(v64)
            out[name + '/value'] = np.float32(v32[0])
            out[name + '/grad64_fp'] = R.fingerprint(g64)
            out[name + '/e_ref'] = np.array([e_v, e_g])
            worst[kind] = np.fmax(worst[kind], [e_v, e_g])
            print('  %-16s seed %2d min_band %.2e value %.8f  e_ref value %.2e grad %.2e'
                  % (name, seed, out[name + '/min_band'], float(v64), e_v, e_g), flush=True)
    for kind in L.KINDS:
        out['E_' + kind] = worst[kind]
        print('  E_%-6s value %.3e  grad %.3e' % (kind, worst[kind][0], worst[kind][1]))
    out['names'] = np.array(names)
    path = os.path.join(REPO, 'tests', 'golden', 'laploss.npz')
    np.savez_compressed(path, **out)
    print('  laploss.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
