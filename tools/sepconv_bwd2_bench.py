#!/usr/bin/env python
"""SepConv's second backward: the fused entry point against the composition from the first-order entry points, and one second-order
meta-iteration with --sepconv_second_order 0 / 1.  Writes a report (default profiles/sepconv_bwd2_bench.txt).

Kernel comparison (K = 51, frames of 8-bit images as the model feeds them, so the frames8 entry points apply):
    fused        savfi_sepconv_bwd2_f32: one launch
    composition  d_gO = fwd(in, ggV, h) + fwd(in, v, ggH); dV = the gV of bwd(in, v, ggH, gO); dH = the gH of bwd(in, ggV, h, gO):
                 savfi_sepconv_fwd_frames8_f32 x 2 + savfi_sepconv_bwd_frames8_f32 x 2 (the add of the two forwards is timed apart)
Same process, warmed, alternating; per repetition a device-event window around --calls back-to-back calls; medians and spread.
A run that finds no device fails."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from meta_interpolation_amd import _hip, synthetic                                  # noqa: E402
from meta_interpolation_amd.sepconv.sepconv_op import sepconv as S                    # noqa: E402

K = 51


def _inputs(B, C, Ho, Wo, seed=0):
    g = torch.Generator().manual_seed(seed)
    inp = torch.randint(0, 256, (B, C, Ho + K - 1, Wo + K - 1), generator=g).float() / 255
    taps = lambda: torch.randn(B, K, Ho, Wo, generator=g) / K ** 0.5
    v, h, ggV, ggH = taps(), taps(), taps(), taps()
    gO = torch.randn(B, C, Ho, Wo, generator=g)
    return [t.cuda() for t in (inp, v, h, gO, ggV, ggH)]


def _event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def kernel_comparison(shape, reps, calls, lines):
    B, C, Ho, Wo = shape
    inp, v, h, gO, ggV, ggH = _inputs(B, C, Ho, Wo)
    lib, st = _hip.lib(), _hip.current_stream()
    assert S.frames8_supported(inp, B, C, Ho, Wo, K), "the frames8 entry points must apply at the benchmark shapes"
    cls = S.frames8_classify(inp)
    d_gO, dV, dH = torch.empty_like(gO), torch.empty_like(v), torch.empty_like(h)
    o1, o2, c_dV, c_dH, junk = torch.empty_like(gO), torch.empty_like(gO), torch.empty_like(v), torch.empty_like(h), torch.empty_like(v)
    p = lambda t: t.data_ptr()

    def fused():
        _hip.check(lib.savfi_sepconv_bwd2_f32(p(inp), p(v), p(h), p(gO), p(ggV), p(ggH), p(d_gO), p(dV), p(dH), B, C, Ho, Wo, K, st), "bwd2")

    def composition():
        _hip.check(lib.savfi_sepconv_fwd_frames8_f32(p(inp), p(ggV), p(h), p(o1), p(cls), B, C, Ho, Wo, K, K, 0, st), "fwd")
        _hip.check(lib.savfi_sepconv_fwd_frames8_f32(p(inp), p(v), p(ggH), p(o2), p(cls), B, C, Ho, Wo, K, K, 0, st), "fwd")
        _hip.check(lib.savfi_sepconv_bwd_frames8_f32(p(inp), p(v), p(ggH), p(gO), p(c_dV), p(junk), p(cls), B, C, Ho, Wo, K, K, 0, st), "bwd")
        _hip.check(lib.savfi_sepconv_bwd_frames8_f32(p(inp), p(ggV), p(h), p(gO), p(junk), p(c_dH), p(cls), B, C, Ho, Wo, K, K, 0, st), "bwd")

    def composition_add():
        composition()
        torch.add(o1, o2, out=o1)

    for fn in (fused, composition, composition_add):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    diffs = (rel(d_gO, o1), rel(dV, c_dV), rel(dH, c_dH))          # o1 holds the sum after composition_add
    times = {"fused": [], "composition": [], "composition+add": []}
    for _ in range(reps):
        for name, fn in (("fused", fused), ("composition", composition), ("composition+add", composition_add)):
            times[name].append(1e3 * _event_ms(fn, calls))
    px = B * Ho * Wo
    f_bytes = S.bwd2_algorithmic_bytes(B, C, Ho, Wo, K)
    c_bytes = 2 * S.algorithmic_bytes(B, C, Ho, Wo, K) + 2 * S.algorithmic_bytes(B, C, Ho, Wo, K, grads=2)
    f_macs, c_macs = S.bwd2_macs(B, C, Ho, Wo, K), (2 * 1 + 2 * 2) * C * K * K * px
    lines.append("%dx%dx%dx%d K=%d   algorithmic: fused %.1f MB, %.2f GMAC; composition %.1f MB, %.2f GMAC"
                 % (B, C, Ho, Wo, K, f_bytes / 1e6, f_macs / 1e9, c_bytes / 1e6, c_macs / 1e9))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        macs, nbytes = (f_macs, f_bytes) if name == "fused" else (c_macs, c_bytes)
        lines.append("    %-16s median %8.1f us  (min %8.1f  max %8.1f, %d repetitions of %d calls)   %6.2f TMAC/s  %6.1f GB/s algorithmic"
                     % (name, med[name], min(ts), max(ts), len(ts), calls, macs / med[name] / 1e6, nbytes / med[name] / 1e3))
    lines.append("    fused / composition = %.3f   (fused vs composition, max|diff| / max|ref|: d_gO %.1e  dV %.1e  dH %.1e)"
                 % ((med["fused"] / med["composition"],) + diffs))
    return med


def iteration_comparison(reps, lines):
    from tests.helpers import build_system
    over = dict(optimizer='SGD', inner_lr=1e-3, loss='1*MSE', number_of_training_steps_per_iter=2, number_of_evaluation_steps_per_iter=2,
                second_order=True, first_order_to_second_order_epoch=-1)
    frames = synthetic.septuplet_batch(1, 256, 448, model='sepconv')
    systems = {flag: build_system('sepconv', dict(over, sepconv_second_order=flag)) for flag in (0, 1)}

    def step(system):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=False)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for s in systems.values():
        step(s)
        step(s)
    times = {0: [], 1: []}
    for _ in range(reps):
        for flag, s in systems.items():
            times[flag].append(step(s))
    lines.append("one meta-iteration, --model sepconv --second_order, 1 task x 2 steps, 256x448, SGD, MSE (host clock around a synchronised call)")
    for flag, ts in times.items():
        lines.append("    --sepconv_second_order %d   median %8.1f ms  (min %8.1f  max %8.1f, %d alternating repetitions)"
                     % (flag, statistics.median(ts), min(ts), max(ts), len(ts)))
    lines.append("    flag 1 does strictly more work (the second-order terms of the 51-tap op and of everything behind it): reported, no gate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--iter_reps', type=int, default=5)
    ap.add_argument('--no_iteration', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sepconv_bwd2_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("sepconv_bwd2_bench needs a GPU: nothing here is measured on a CPU")
    assert args.reps >= 20
    torch.cuda.set_device(0)
    lines = ["# python tools/sepconv_bwd2_bench.py --reps %d --calls %d   (%s; device events; fused and composition alternate in one process)"
             % (args.reps, args.calls, torch.cuda.get_device_name(0))]
    for shape in ((1, 3, 256, 448), (1, 3, 720, 1280)):
        kernel_comparison(shape, args.reps, args.calls, lines)
    if not args.no_iteration:
        iteration_comparison(args.iter_reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
