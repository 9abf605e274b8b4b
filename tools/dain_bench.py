"""HIP-event timing of the kernels of csrc/dainnet.hip and the Charbonnier loss against their ATen compositions, and of a whole DAIN
meta-iteration with the frozen front reused and with the reuse switched off, of the same iteration with --dain_task_modes 1 (tasks in
lockstep, eagerly and from captured graphs), and of front() with and without out=.

    python tools/dain_bench.py [output file] [--iteration-size H W] [--steps kernels,iteration,modes,front]        (needs the GPU)

The steps run in the order given, each after the one before it has finished: an exception in a step ends the tool with a non-zero status
and nothing further touches the GPU.  Lines are appended to the output file as each step completes.

Kernels: at the hourglass's and the rectify net's shapes for 256 x 448 and 768 x 1280 frames (one task: the depth net's batch is the two
frames of a pair), isolated launches, median and minimum of REPS launches after WARM warm-up calls; the ATen composition of the same
computation is timed the same way, alternating with the kernel.  The fraction of the 8 TB/s HBM peak is algorithmic bytes (every
operand once) over the median time.
Iteration: batch 6, one inner step, Adamax + Meta-SGD (scripts/run_dain.sh), synthetic frames, seeded weights; `reuse off` recomputes the
front on every pass -- the reference's structure and the baseline.  Both systems hold the same weights; the two are timed alternately,
ITERS iterations each after one warm-up iteration, a device synchronise around each.
Modes: the same configuration with --dain_task_modes 1 and --task_batch 8 (one lockstep group of 6), --graph_inner_loop 0 (eager
lockstep) and 1 (graphed lockstep), alternating with `front reused` (modes off, the default path), timed the same way; the graphed system
gets one more warm-up iteration (its capture).  Front: front() for 6 pairs with and without out=alloc_front(...), HIP events.
There is no speed gate anywhere: the figures say what was measured, on these shapes, nothing more.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops, synthetic
from meta_interpolation_amd.config import default_args

PEAK = 8.0e12
SIZES = ((256, 448), (768, 1280))
REPS, WARM, ITERS = 30, 5, 3


def timed_pair(f, g):
    """median, minimum (us) of f and of g, launches alternating"""
    for _ in range(WARM):
        f()
        g()
    torch.cuda.synchronize()
    evs = ([], [])
    for _ in range(REPS):
        for k, fn in enumerate((f, g)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    out = []
    for rows in evs:
        t = sorted(1e3 * a.elapsed_time(b) for a, b in rows)
        out.append((t[len(t) // 2], t[0]))
    return out


def kernels(lines):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)

    def report(op, shape, nbytes, ours, aten):
        rec = dict(op=op, shape="x".join(str(v) for v in shape), median_us=round(ours[0], 1), min_us=round(ours[1], 1),
                   aten_median_us=round(aten[0], 1), aten_min_us=round(aten[1], 1), aten_over_kernel=round(aten[0] / ours[0], 2),
                   algorithmic_MB=round(nbytes / 1e6, 2), hbm_peak_fraction=round(nbytes / (ours[0] * 1e-6) / PEAK, 4))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with torch.no_grad():
        for H, W in SIZES:
            # BatchNorm + ReLU of the hourglass: its first layer (128 channels at full size) and an inception branch one level down
            for C, h, w in ((128, H, W), (32, H // 2, W // 2), (64, H // 8, W // 8)):
                x = rnd(2, C, h, w)
                out = torch.empty(2, C + 96, h, w, device="cuda")

                def ours():
                    m, v = hip_ops.bn_stats(x, 2)
                    hip_ops.bn_apply_relu(x, m, v, 2, out=out, c_off=32)

                def aten():
                    out[:, 32:32 + C] = F.relu(F.batch_norm(x, None, None, None, None, True, 0.1, 1e-5))
                report("bn_stats+bn_apply_relu into a slice", (2, C, h, w), 4 * x.numel() * 3, *timed_pair(ours, aten))
            for C, h, w in ((128, H, W), (32, H, W)):
                x = rnd(2, C, h, w)
                report("maxpool2x2", (2, C, h, w), 5 * x.numel(), *timed_pair(lambda: hip_ops.max_pool2x2(x), lambda: F.max_pool2d(x, 2, 2)))
            low, skip = rnd(2, 64, H // 2, W // 2), rnd(2, 64, H, W)
            report("upnearest2x_add", (2, 64, H, W), 4 * (low.numel() + 2 * skip.numel()),
                   *timed_pair(lambda: hip_ops.upnearest2x_add(low, skip), lambda: skip + F.interpolate(low, scale_factor=2, mode='nearest')))
            a, r = rnd(1, 128, H, W), rnd(1, 128, H, W)
            report("add_relu", (1, 128, H, W), 12 * a.numel(), *timed_pair(lambda: hip_ops.add_relu(a, r), lambda: torch.relu(a + r)))
            p, q = rnd(1, 3, H, W), rnd(1, 3, H, W)

            def aten_loss():
                d = p - q
                return torch.mean(torch.sqrt(d * d + 1e-16))
            report("charbonnier_loss", (1, 3, H, W), 8 * p.numel(), *timed_pair(lambda: hip_ops.charbonnier_loss(p, q), aten_loss))


def _system(batch, reuse=True, **over):
    from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
    from meta_interpolation_amd.meta_learning_system import SceneAdaptiveInterpolation
    args = default_args(model='dain', num_gpu=1, loss='1*L1', optimizer='Adamax', metasgd=True, batch_size=batch, inner_lr=1e-5, outer_lr=1e-5,
                        number_of_training_steps_per_iter=1, number_of_evaluation_steps_per_iter=1, **over)
    torch.manual_seed(1)
    net = MetaDAIN()
    synthetic.load_seeded_weights(net, 'dain')
    net.reuse_front = reuse
    return SceneAdaptiveInterpolation(args, net=net)


def iteration(lines, H, W, batch=6):
    _iterations(lines, H, W, batch, {"front reused": _system(batch), "reuse off (the reference's structure)": _system(batch, reuse=False)})


def modes(lines, H, W, batch=6):
    """--dain_task_modes 1 beside the default path (`front reused` of iteration(): the parent commit's)."""
    _iterations(lines, H, W, batch, {"front reused": _system(batch),
                                     "task modes on, eager lockstep": _system(batch, dain_task_modes=1, graph_inner_loop=0, task_streams=1),
                                     "task modes on, graphed lockstep": _system(batch, dain_task_modes=1, graph_inner_loop=1, task_streams=1)},
                warm=2)


def front(lines, H, W, batch=6):
    from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
    system = _system(1)
    net = system.net
    frames = [f.cuda() for f in synthetic.septuplet_batch(batch, H, W, model='dain')]
    out = MetaDAIN.alloc_front(batch, H, W, 'cuda')
    global REPS, WARM
    keep, REPS, WARM = (REPS, WARM), 5, 1
    try:
        plain, inplace = timed_pair(lambda: net.front(frames[2], frames[4]), lambda: net.front(frames[2], frames[4], out=out))
    finally:
        REPS, WARM = keep
    lines.append(json.dumps(dict(front="%d pairs at %dx%d" % (batch, H, W), median_ms=round(plain[0] / 1e3, 2), min_ms=round(plain[1] / 1e3, 2),
                                 out_median_ms=round(inplace[0] / 1e3, 2), out_min_ms=round(inplace[1] / 1e3, 2),
                                 plain_over_out=round(plain[0] / inplace[0], 3), repetitions=5)))
    print(lines[-1], flush=True)


def _iterations(lines, H, W, batch, systems, warm=1):
    frames = [f.cuda() for f in synthetic.septuplet_batch(batch, H, W, model='dain')]
    times = {name: [] for name in systems}
    for it in range(ITERS + warm):
        for name, system in systems.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses, _, _ = system.run_train_iter(frames, 0)
            float(losses['loss'])
            torch.cuda.synchronize()
            if it >= warm:
                times[name].append(time.perf_counter() - t0)
    med = {}
    for name, t in times.items():
        t = sorted(t)
        med[name] = t[len(t) // 2]
        lines.append(json.dumps(dict(iteration=name, frames="%dx%d" % (H, W), batch=batch, inner_steps=1, median_ms=round(1e3 * med[name], 1),
                                     min_ms=round(1e3 * t[0], 1), iterations=len(t),
                                     fronts_per_iteration=systems[name].net.front_evaluations // (ITERS + warm))))
        print(lines[-1], flush=True)
    names = list(systems)
    for other in names[1:]:
        lines.append("# %dx%d: %s / %s = %.2f (medians)" % (H, W, other, names[0], med[other] / med[names[0]]))
        print(lines[-1], flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dain_bench needs the GPU: nothing is measured without one")
    argv = sys.argv[1:]
    size = (256, 448)
    if '--iteration-size' in argv:
        i = argv.index('--iteration-size')
        size = (int(argv[i + 1]), int(argv[i + 2]))
        del argv[i:i + 3]
    steps = ['kernels', 'iteration', 'modes', 'front']
    if '--steps' in argv:
        i = argv.index('--steps')
        steps = argv[i + 1].split(',')
        del argv[i:i + 2]
    out_path = argv[0] if argv else None
    table = {'kernels': lambda ls: kernels(ls), 'iteration': lambda ls: iteration(ls, *size), 'modes': lambda ls: modes(ls, *size),
             'front': lambda ls: front(ls, *size)}
    unknown = [st for st in steps if st not in table]
    if unknown:
        raise SystemExit("unknown step(s) %s: one of %s" % (unknown, sorted(table)))
    if out_path and not os.path.exists(out_path):
        with open(out_path, "w") as fh:
            fh.write("# tools/dain_bench.py on an MI355X.  Kernels: isolated launches, HIP events, %d repetitions after %d warm-up calls, alternating\n"
                     "# with the ATen composition; fraction of the 8 TB/s HBM peak = algorithmic bytes / median time / 8e12.  Iteration: host clock\n"
                     "# around run_train_iter with a device synchronise, %d iterations after the warm-up, the variants alternating.\n"
                     "# Measured on these shapes only; no speed gate.\n" % (REPS, WARM, ITERS))
    for st in steps:             # one after the other: an exception ends the tool, nothing later runs on the GPU
        lines = []
        table[st](lines)
        torch.cuda.synchronize()
        if out_path:
            with open(out_path, "a") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
