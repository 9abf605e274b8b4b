"""Softmax splatting, forward and forward + backward: the fused kernels (hip_ops.softsplat) against the composition they replace
(hip_ops.softsplat_composed: index_add scatters, a scatter_reduce and element-wise torch ops with autograd, the same definition in fp32) in
soft mode, timed with HIP events after a warm-up, the two alternating in one process, five windows each; flows `uniform` (sub-pixel to a
few pixels, every target hit by a handful of sources) and `collide` (every source of the frame lands around one of three points: the
worst case for atomics); then one `--model softsplat` meta-iteration (seeded weights, synthetic 256 x 448 septuplets, the product's
default execution mode).  The achieved bytes per second count the operands as hip_ops.softsplat_bytes does.  There is no speed gate with
one exception: at 1x3x256x448 the fused forward + backward must not be slower than the composition (the script says so in its output
file and exits non-zero if it is).  Needs a GPU.  Writes profiles/softsplat_bench.txt.

    python tools/softsplat_bench.py [--iters 50] [--tasks 4] [--steps 2] [--out profiles/softsplat_bench.txt]
"""
import argparse
import contextlib
import os
import sys
import tempfile
import time

os.environ.setdefault('MIOPEN_USER_DB_PATH', tempfile.mkdtemp(prefix='savfi_softsplat_bench_miopen_'))
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from meta_interpolation_amd import hip_ops, synthetic  # noqa: E402

SHAPES = [(1, 3, 256, 448), (1, 3, 720, 1280), (1, 64, 128, 224)]
GATED = (1, 3, 256, 448)
FLOWS = ('uniform', 'collide')


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def make_flow(kind, N, H, W, gen):
    if kind == 'uniform':
        return 4.0 * torch.rand(N, 2, H, W, generator=gen) - 2.0
    jj = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(N, H, W)
    ii = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(N, H, W)
    pick = torch.randint(0, 3, (N, H, W), generator=gen)
    tx = torch.tensor([0.25 * W + 0.3, 0.5 * W + 0.6, 0.75 * W + 0.1])[pick]
    ty = torch.tensor([0.5 * H + 0.7, 0.25 * H + 0.2, 0.75 * H + 0.4])[pick]
    return torch.stack([tx - jj, ty - ii], 1)


def op_lines(iters):
    lines, slower = [], []
    for N, C, H, W in SHAPES:
        for kind in FLOWS:
            gen = torch.Generator().manual_seed(0)
            x = torch.rand(N, C, H, W, generator=gen).cuda().requires_grad_()
            flow = make_flow(kind, N, H, W, gen).cuda().requires_grad_()
            metric = (-4.0 * torch.rand(N, 1, H, W, generator=gen)).cuda().requires_grad_()
            gout = torch.randn(N, C, H, W, generator=gen).cuda()
            leaves = (x, flow, metric)
            det = [t.detach() for t in leaves]
            runs = {
                'fwd': (lambda: hip_ops.softsplat(*det), lambda: hip_ops.softsplat_composed(*det)),
                'fwd+bwd': (lambda: torch.autograd.grad(hip_ops.softsplat(*leaves), leaves, gout),
                            lambda: torch.autograd.grad(hip_ops.softsplat_composed(*leaves), leaves, gout)),
            }
            a, b = runs['fwd'][0](), runs['fwd'][1]()
            dv = float((a - b).abs().max() / b.abs().max())
            dg = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(runs['fwd+bwd'][0](), runs['fwd+bwd'][1]()))
            nbytes = {'fwd': hip_ops.softsplat_bytes(x), 'fwd+bwd': hip_ops.softsplat_bytes(x) + hip_ops.softsplat_bytes(x, 'soft', 3)}
            for what, (fused, composed) in runs.items():
                for _ in range(5):
                    fused(), composed()
                torch.cuda.synchronize()
                tf, tc = [], []
                for rep in range(5):          # alternate the two
                    tf.append(timed(fused, iters))
                    tc.append(timed(composed, max(1, iters // 5)))
                lines.append('%-14s %-8s %-8s fused %8.1f us (min of 5; %s; %.0f GB/s of operand bytes)   composed %9.1f us (%s)   ratio %.1fx   '
                             'max |dvalue| / max |value| %.1e  max |dgrad| / max |grad| %.1e'
                             % ('x'.join(map(str, (N, C, H, W))), kind, what, min(tf), ' '.join('%.1f' % t for t in tf),
                                nbytes[what] / min(tf) / 1e3, min(tc), ' '.join('%.1f' % t for t in tc), min(tc) / min(tf), dv, dg))
                print(lines[-1], flush=True)
                if what == 'fwd+bwd' and (N, C, H, W) == GATED and min(tf) > min(tc):
                    slower.append(lines[-1])
            del runs
            torch.cuda.empty_cache()
    return lines, slower


def iteration_line(tasks, steps):
    from meta_interpolation_amd.config import default_args
    from meta_interpolation_amd.meta_learning_system import MODEL_REGISTRY, SceneAdaptiveInterpolation
    args = default_args(model='softsplat', num_gpu=1, batch_size=tasks, number_of_training_steps_per_iter=steps,
                        number_of_evaluation_steps_per_iter=steps, optimizer='SGD', inner_lr=1e-3, loss='1*L1')
    with contextlib.redirect_stdout(sys.stderr):
        net = MODEL_REGISTRY['softsplat'](args, False)
        synthetic.load_seeded_weights(net, 'softsplat')
        system = SceneAdaptiveInterpolation(args, net=net.cuda())
    frames = [f.cuda() for f in synthetic.septuplet_batch(tasks, 256, 448, model='softsplat')]
    first = None
    for _ in range(3):                # warm-up: allocator, solver choice, graph capture where the mode captures
        losses, _, _ = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=False)
        first = float(losses['loss']) if first is None else first
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        losses, _, _ = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=False)
        last = float(losses['loss'])          # the host read a logging loop does; ends in a device synchronise
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return ('--model softsplat meta-iteration: %d tasks x %d inner steps, 256 x 448, SGD, L1, default mode: %.1f ms (min of 5; %s); loss %.6f -> %.6f'
            % (tasks, steps, min(times), ' '.join('%.1f' % t for t in times), first, last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--tasks', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'softsplat_bench.txt'))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/softsplat_bench.py needs a GPU: a timing taken anywhere else says nothing")
    lines, slower = op_lines(o.iters)
    lines.append(iteration_line(o.tasks, o.steps))
    print(lines[-1], flush=True)
    gated = [l for l in lines if l.startswith('x'.join(map(str, GATED))) and ' fwd+bwd ' in l]
    lines.append('speed expectation (fused forward + backward not slower than the composition at %s): %s'
                 % ('x'.join(map(str, GATED)), 'NOT MET' if slower else 'met, by %s' % ', '.join(l.split('ratio ')[1].split()[0] + ' (' + l.split()[1] + ')'
                                                                                                  for l in gated)))
    print(lines[-1], flush=True)
    with open(o.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    if slower:
        raise SystemExit("the fused forward + backward is slower than the composition it replaces:\n" + '\n'.join(slower))


if __name__ == '__main__':
    main()
