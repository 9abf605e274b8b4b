"""The PSNR / SSIM evaluation metric of `rows` image pairs, three ways, timed with HIP events after a warm-up, the variants
alternating in one process:

  (a) the composition in utils.py, pair by pair (quantize twice, the squared error, utils.ssim: what ran before the fused entry);
  (b) ATen quantise + the existing fused kernels: savfi_l1_mse_f32 on q / 255 and savfi_ssim_loss_f32 at SAVFI_SSIM_RANGE_FIXED + 2;
  (c) the fused entry, hip_ops.psnr_ssim (savfi_psnr_ssim_f32).

    python tools/metrics_bench.py [--iters 200]      # calls per timed window, raised per variant to fill 50 ms

All three end in device tensors (no host read inside the timed region).  (c) must not be slower than (b) at any shape.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meta_interpolation_amd import _hip, hip_ops, utils  # noqa: E402

SHAPES = [(1, 3, 256, 448), (4, 3, 256, 448), (1, 3, 720, 1280)]


def composition(pred, tgt):
    mse, ssim = [], []
    for r in range(pred.shape[0]):
        q_p, q_t = utils.quantize(pred[r], 1.), utils.quantize(tgt[r], 1.)
        mse.append((q_p - q_t).div(255).pow(2).mean())
        ssim.append(utils.ssim(q_p.unsqueeze(0), q_t.unsqueeze(0), val_range=255))
    return torch.stack(mse), torch.stack(ssim)


def existing_kernels(pred, tgt):
    lib, st = _hip.lib(), _hip.current_stream()
    rows, C, H, W = pred.shape
    q_p, q_t = utils.quantize(pred, 1.), utils.quantize(tgt, 1.)
    mse = hip_ops.mse_loss_per_sample(q_p / 255, q_t / 255)
    loss = torch.empty(rows, device=pred.device)
    word = torch.empty(rows, dtype=torch.int32, device=pred.device)
    scratch = torch.empty(int(lib.savfi_ssim_scratch_floats(rows, C, H, W)), device=pred.device)
    _hip.check(lib.savfi_ssim_loss_f32(q_p.data_ptr(), q_t.data_ptr(), loss.data_ptr(), word.data_ptr(), scratch.data_ptr(), rows, C, H, W,
                                       _hip.SSIM_RANGE_FIXED + 2, st), "savfi_ssim_loss_f32")
    return mse, 1 - 2 * loss


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
    o = ap.parse_args()
    dev = 'cuda'
    print('%-16s %-30s %-30s %-30s %s' % ('shape', '(a) composition, us', '(b) quantise + l1_mse + ssim, us', '(c) fused entry, us', 'b/c  a/c   |d mse| |d ssim| of c vs a'))
    for shape in SHAPES:
        gen = torch.Generator().manual_seed(0)
        tgt = torch.rand(shape, generator=gen)
        pred = (tgt + 0.02 * torch.randn(shape, generator=gen)).to(dev)
        tgt = tgt.to(dev)
        variants = [lambda: composition(pred, tgt), lambda: existing_kernels(pred, tgt), lambda: hip_ops.psnr_ssim(pred, tgt)]
        first = [fn() for fn in variants]
        for _ in range(10):
            for fn in variants:
                fn()
        torch.cuda.synchronize()
        # every timed window holds at least --iters calls and at least 50 ms of work
        iters = [max(o.iters, int(5e4 / timed(fn, 20)) + 1) for fn in variants]
        times = [[], [], []]
        for rep in range(5):          # alternate the three
            for i, fn in enumerate(variants):
                times[i].append(timed(fn, iters[i]))
        best = [min(t) for t in times]
        cols = ['%8.1f (%s)' % (best[i], ' '.join('%.1f' % t for t in times[i])) for i in range(3)]
        print('%-16s %-30s %-30s %-30s %.2f %.2f  %.1e %.1e' % (
            'x'.join(map(str, shape)), cols[0], cols[1], cols[2], best[1] / best[2], best[0] / best[2],
            float((first[2][0] - first[0][0]).abs().max()), float((first[2][1] - first[0][1]).abs().max())), flush=True)


if __name__ == '__main__':
    main()
