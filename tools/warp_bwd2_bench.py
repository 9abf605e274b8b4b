#!/usr/bin/env python
"""The two warps' second backward: the fused entry points against double backward through composed device ops, and one second-order
VoxelFlow meta-iteration with --warp_second_order 0 / 1.  Writes a report (default profiles/warp_bwd2_bench.txt).

Op comparison, per shape, the double backward alone (the graph of the first backward is built once, outside the timed window):
    fused      _VoxelWarpTwice / _FlowWarpTwice: grad(<g, v>, (gO, x)) is ONE launch of savfi_voxelwarp_bwd2_f32 / savfi_flowwarp_bwd2_f32
               behind the backward of the <g, v> product ("fused bwd2 ABI": that launch alone, through the C ABI)
    composed   hip_ops._voxel_warp_composed (what --warp_second_order 0 takes), and for the flow warp the same map written with
               gathers below (flow_warp_composed): grad(<g, v>, (gO, x)) through autograd's graph of ATen ops
and the whole chain forward + backward(create_graph) + double backward, which is what a second-order inner step pays.
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

from meta_interpolation_amd import _hip, hip_ops, synthetic                          # noqa: E402


def flow_warp_composed(img, flow):
    """hip_ops.flow_warp from differentiable ATen ops: F.grid_sample(bilinear, zeros, align_corners=False) behind the reference's
    2 * (x / W - 0.5) normalisation, written with gathers (ATen's grid sampler has no second derivative)"""
    N, C, H, W = img.shape
    xs = torch.arange(W, device=img.device, dtype=img.dtype).view(1, 1, W)
    ys = torch.arange(H, device=img.device, dtype=img.dtype).view(1, H, 1)
    ix = ((2 * ((xs + flow[:, 0]) / W - 0.5) + 1) * W - 1) / 2
    iy = ((2 * ((ys + flow[:, 1]) / H - 0.5) + 1) * H - 1) / 2
    x0, y0 = ix.detach().floor(), iy.detach().floor()
    fx, fy = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
    flat = img.reshape(N, C, H * W)

    def tap(yy, xx):
        inside = ((xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)).unsqueeze(1).to(img.dtype)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(N, 1, H * W).expand(N, C, H * W)
        return flat.gather(2, idx).view(N, C, H, W) * inside

    return (tap(y0, x0) * (1 - fx) * (1 - fy) + tap(y0, x0 + 1) * fx * (1 - fy) + tap(y0 + 1, x0) * (1 - fx) * fy
            + tap(y0 + 1, x0 + 1) * fx * fy)


def _event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _inputs(kind, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == 'voxel':
        a = torch.rand(1, 6, H, W, generator=g)
        x = torch.tanh(0.3 * torch.randn(1, 3, H, W, generator=g))
    else:
        a = torch.rand(1, 3, H, W, generator=g)
        x = 3.0 * torch.randn(1, 2, H, W, generator=g)
    return a.cuda(), x.cuda(), torch.randn(1, 3, H, W, generator=g).cuda(), torch.randn(x.shape, generator=g).cuda()


def op_comparison(kind, H, W, reps, calls, lines):
    a, x, gout, v = _inputs(kind, H, W)
    if kind == 'voxel':
        ops = {"fused": lambda a_, x_: hip_ops._VoxelWarpTwice.apply(a_, x_), "composed": hip_ops._voxel_warp_composed}
        nbytes = hip_ops.voxel_warp_bwd2_bytes(1, H, W)
    else:
        ops = {"fused": lambda a_, x_: hip_ops._FlowWarpTwice.apply(a_, x_), "composed": flow_warp_composed}
        nbytes = hip_ops.flow_warp_bwd2_bytes(1, 3, H, W)

    def chain(op):
        xd, gd = x.clone().requires_grad_(), gout.clone().requires_grad_()
        g, = torch.autograd.grad(op(a, xd), xd, gd, create_graph=True)
        return torch.autograd.grad((g * v).sum(), (gd, xd))

    fns, results = {}, {}
    for name, op in ops.items():
        xd, gd = x.clone().requires_grad_(), gout.clone().requires_grad_()
        g, = torch.autograd.grad(op(a, xd), xd, gd, create_graph=True)
        s = (g * v).sum()
        fns[name + " bwd2"] = (lambda s=s, gd=gd, xd=xd: torch.autograd.grad(s, (gd, xd), retain_graph=True))
        fns[name + " chain"] = (lambda op=op: chain(op))
        results[name] = chain(op)
    lib, st, p = _hip.lib(), _hip.current_stream(), (lambda t: t.data_ptr())
    d_g, d_x = torch.empty_like(gout), torch.empty_like(x)
    if kind == 'voxel':
        fns["fused bwd2 ABI"] = lambda: _hip.check(lib.savfi_voxelwarp_bwd2_f32(p(a), p(x), p(gout), p(v), p(d_g), p(d_x), 1, H, W, st), "bwd2")
    else:
        fns["fused bwd2 ABI"] = lambda: _hip.check(lib.savfi_flowwarp_bwd2_f32(p(a), p(x), p(gout), p(v), p(d_g), p(d_x), 1, 3, H, W, st), "bwd2")
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # a pixel whose coordinate the two forms round into different cells is a whole texel difference apart: max and share of such elements
    rel = lambda p, q: ((p - q).abs().max() / q.abs().max()).item()
    far = lambda p, q: ((p - q).abs() > 1e-4 * q.abs().max()).float().mean().item()
    diffs = tuple(f(p, q) for p, q in zip(results["fused"], results["composed"]) for f in (rel, far))
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(1e3 * _event_ms(fn, calls))
    lines.append("%s warp 1x3x%dx%d   fused bwd2, algorithmic: %.2f MB" % (kind, H, W, nbytes / 1e6))
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        extra = "   %6.1f GB/s algorithmic (the launch alone, through the C ABI)" % (nbytes / med[name] / 1e3) if name == "fused bwd2 ABI" else ""
        lines.append("    %-15s median %8.1f us  (min %8.1f  max %8.1f, %d repetitions of %d calls)%s"
                     % (name, med[name], min(ts), max(ts), len(ts), calls, extra))
    lines.append("    fused / composed: bwd2 %.3f, chain %.3f   (fused vs composed, max|diff| / max|ref| and share of elements over 1e-4 of max|ref|: d_gout %.1e %.1e  d_x %.1e %.1e)"
                 % ((med["fused bwd2"] / med["composed bwd2"], med["fused chain"] / med["composed chain"]) + diffs))
    return med


def iteration_comparison(reps, lines):
    from tests.helpers import build_system
    over = dict(optimizer='SGD', inner_lr=1e-3, loss='1*MSE', number_of_training_steps_per_iter=2, number_of_evaluation_steps_per_iter=2,
                second_order=True, first_order_to_second_order_epoch=-1, weight_recipe='smooth')
    frames = synthetic.septuplet_batch(1, 256, 256, model='voxelflow')
    systems = {flag: build_system('voxelflow', dict(over, warp_second_order=flag)) for flag in (0, 1)}

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
    lines.append("one meta-iteration, --model voxelflow --second_order, 1 task x 2 steps, 256x256, SGD, MSE (host clock around a synchronised call)")
    for flag, ts in times.items():
        lines.append("    --warp_second_order %d   median %8.1f ms  (min %8.1f  max %8.1f, %d alternating repetitions)"
                     % (flag, statistics.median(ts), min(ts), max(ts), len(ts)))
    lines.append("    the two flags compute the same terms (composed ATen ops against the fused kernels): reported, no gate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--calls', type=int, default=8)
    ap.add_argument('--iter_reps', type=int, default=7)
    ap.add_argument('--no_iteration', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'warp_bwd2_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("warp_bwd2_bench needs a GPU: nothing here is measured on a CPU")
    assert args.reps >= 20
    torch.cuda.set_device(0)
    lines = ["# python tools/warp_bwd2_bench.py --reps %d --calls %d   (%s; device events; fused and composed alternate in one process)"
             % (args.reps, args.calls, torch.cuda.get_device_name(0))]
    for kind in ('voxel', 'flow'):
        for H, W in ((256, 256), (256, 448)):
            op_comparison(kind, H, W, args.reps, args.calls, lines)
    if not args.no_iteration:
        iteration_comparison(args.iter_reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
