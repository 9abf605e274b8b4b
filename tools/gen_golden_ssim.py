"""tools/gen_golden_ssim.py -- TEST INFRASTRUCTURE.  Fixtures of the SSIM loss term, produced by IMPORTING the reference.

Runs on the CPU in the build container only (it needs the reference tree, through oracle.gen_golden's shims; nothing of the
reference is copied):

    python tools/gen_golden_ssim.py                 # everything
    python tools/gen_golden_ssim.py --only loss     # tests/golden/ssim_loss.npz
    python tools/gen_golden_ssim.py --only sepconv_l1_ssim_2step cain_l1_ssim_1step voxelflow_mse_ssim_2step

ssim_loss.npz: the reference's ``pytorch_msssim.SSIM(val_range=1.)`` as ``Loss`` constructs it (loss.py:294), called as
``fn(sr, hr.clone())`` in fp32 on the CPU, on the seeded pairs of tests/ssim_ref.make_pair (the inputs are re-drawn from the seed,
not stored).  Per case: the fp32 loss, a fingerprint of d loss / d sr (the whole gradient for the smaller cases) and
``e_ref`` = |reference fp32 - float64 restatement| (loss: absolute; gradient: max |diff| / max |float64 gradient|), the
yardstick the kernel's gate is derived from.

system_*.npz: oracle.gen_golden.run_system_case with three cases added to its table at run time; the range class every
SSIM call took is counted and printed (and stored as ``ssim_class_counts``).
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
from tests import ssim_ref as R  # noqa: E402

SYSTEM_CASES = {
    'sepconv_l1_ssim_2step': ('sepconv', 64, 64, 2, dict(optimizer='SGD', inner_lr=1e-3, loss='1*L1+0.1*SSIM',
                                                         number_of_training_steps_per_iter=2,
                                                         number_of_evaluation_steps_per_iter=2)),
    'cain_l1_ssim_1step': ('cain', 64, 64, 1, dict(optimizer='SGD', inner_lr=1e-3, loss='1*L1+0.1*SSIM',
                                                   number_of_training_steps_per_iter=1,
                                                   number_of_evaluation_steps_per_iter=1)),
    'voxelflow_mse_ssim_2step': ('voxelflow', 64, 64, 2, dict(optimizer='SGD', inner_lr=1e-3, loss='1*MSE+0.1*SSIM',
                                                              number_of_training_steps_per_iter=2,
                                                              number_of_evaluation_steps_per_iter=2)),
}

# (N, H, W, store the whole gradient for these classes)
SMALL = [(1, 11, 11, (0, 1, 2, 3)), (1, 37, 53, (0, 1)), (1, 64, 64, ()), (2, 24, 40, (0,)), (4, 24, 40, ())]
LARGE = [(1, 256, 448), (1, 720, 1280)]
SEEDS = (0, 1, 2)


def reference_loss_and_grad(fn, sr, hr):
    sr = sr.clone().requires_grad_()
    loss = fn(sr, hr.clone())
    grad, = torch.autograd.grad(loss, sr)
    return loss.detach(), grad


def measure(fn, kind, cls, N, H, W, seed):
    sr, hr = R.make_pair(kind, cls, N, 3, H, W, seed)
    loss32, grad32 = reference_loss_and_grad(fn, sr, hr)
    srd, hrd = sr.double(), hr.double()
    loss64 = R.ssim_loss(srd, hrd)
    grad64 = R.ssim_loss_grad(srd, hrd)
    e_loss = abs(float(loss32) - float(loss64))
    e_grad = float((grad32.double() - grad64).abs().max() / grad64.abs().max())
    return sr, hr, loss32, grad32, loss64, grad64, e_loss, e_grad


def loss_cases_of_kind(kind):
    import pytorch_msssim
    torch.set_num_threads(4)
    fn = pytorch_msssim.SSIM(val_range=1.)
    out, names, worst = {}, [], np.zeros(2)
    cases = [(N, H, W, cls, store) for N, H, W, store in SMALL for cls in range(4)] + [(N, H, W, cls, ()) for N, H, W in LARGE for cls in (0, 1)]
    for N, H, W, cls, store in cases:
        for seed in SEEDS:
            sr, hr, loss32, grad32, loss64, grad64, e_loss, e_grad = measure(fn, kind, cls, N, H, W, seed)
            name = R.case_name(kind, cls, N, H, W, seed)
            names.append(name)
            out[name + '/loss'] = np.float32(loss32)
            out[name + '/loss64'] = np.float64(loss64)
            out[name + '/grad_fp'] = R.fingerprint(grad32)
            out[name + '/e_ref'] = np.array([e_loss, e_grad])
            if H > 64:
                out[name + '/grad64_fp'] = R.fingerprint(grad64)
            if seed == 0 and cls in store:
                out[name + '/grad'] = grad32.numpy()
            if N > 1 and seed == 0:
                # what N calls on the N = 1 slices give (lockstep tasks, the split support pair)
                out[name + '/loss_rows'] = np.array([float(fn(sr[i:i + 1], hr[i:i + 1].clone())) for i in range(N)], dtype=np.float32)
            worst = np.maximum(worst, [e_loss, e_grad])
            print('  %-34s loss %.8f  e_ref loss %.2e grad %.2e' % (name, float(loss32), e_loss, e_grad), flush=True)
    out['E_' + kind] = worst
    return out, names


def run_loss_cases():
    import multiprocessing
    import pytorch_msssim
    fn = pytorch_msssim.SSIM(val_range=1.)
    out = {'kinds': np.array(R.KINDS), 'seeds': np.array(SEEDS)}
    names = []
    with multiprocessing.get_context('fork').Pool(len(R.KINDS)) as pool:      # one process per content kind
        for part, part_names in pool.map(loss_cases_of_kind, R.KINDS):
            out.update(part)
            names += part_names
    # a batch whose rows fall in different classes: per-row results and the whole-batch result (the batch is class 3)
    for seed in SEEDS:
        sr, hr = R.make_pair('near', [0, 1, 2, 3], 4, 3, 24, 40, seed)
        name = 'mixed_s%d' % seed
        out[name + '/loss_rows'] = np.array([float(fn(sr[i:i + 1], hr[i:i + 1].clone())) for i in range(4)], dtype=np.float32)
        out[name + '/loss'] = np.float32(fn(sr, hr.clone()))
    # identical pair: the reference returns exactly 0 and a gradient that is pure rounding
    for N, H, W in [(1, 11, 11), (1, 37, 53), (1, 64, 64), (4, 24, 40), (1, 256, 448), (1, 720, 1280)]:
        for cls in (0, 1):
            sr, hr = R.make_pair('same', cls, N, 3, H, W, 0)
            loss32, grad32 = reference_loss_and_grad(fn, sr, hr)
            name = R.case_name('same', cls, N, H, W, 0)
            out[name + '/loss'] = np.float32(loss32)
            out[name + '/grad_maxabs'] = np.float64(grad32.abs().max())
            print('  %-34s loss %.3e  max |grad| %.3e' % (name, float(loss32), float(grad32.abs().max())), flush=True)
    out['names'] = np.array(names)
    for kind in R.KINDS:
        print('  E_%-6s loss %.3e  grad %.3e' % (kind, out['E_' + kind][0], out['E_' + kind][1]))
    path = os.path.join(G.GOLD, 'ssim_loss.npz')
    np.savez_compressed(path, **out)
    print('  ssim_loss.npz: %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


def run_system_case(name):
    import pytorch_msssim
    counts = np.zeros(4, dtype=np.int64)
    orig = pytorch_msssim.SSIM.forward

    def forward(self, img1, img2):
        counts[R.range_class(img1.detach())] += 1
        return orig(self, img1, img2)
    pytorch_msssim.SSIM.forward = forward
    G.SYSTEM_CASES[name] = SYSTEM_CASES[name]
    try:
        G.run_system_case(name)
    finally:
        pytorch_msssim.SSIM.forward = orig
    print('  %s: SSIM calls per range class L = 1 / 2 / 255 / 256: %s' % (name, counts.tolist()), flush=True)
    path = os.path.join(G.GOLD, 'system_%s.npz' % name)
    with np.load(path) as z:
        data = {k: z[k] for k in z.files}
    data['ssim_class_counts'] = counts
    np.savez_compressed(path, **data)
    print('  %s: %d bytes, parts %s' % (os.path.basename(path), os.path.getsize(path),
                                        {k: float(v) for k, v in data.items() if k.startswith('train_part_')}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*', default=None)
    opts = ap.parse_args()
    torch.set_num_threads(8)
    G.install_shims()
    for item in opts.only or (['loss'] + list(SYSTEM_CASES)):
        print('[golden ssim]', item, flush=True)
        if item == 'loss':
            run_loss_cases()
        else:
            run_system_case(item)


if __name__ == '__main__':
    main()
