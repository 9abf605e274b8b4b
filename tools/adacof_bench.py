"""AdaCoF's deformable-tap op, forward and forward + backward: the fused kernels (hip_ops.adacof) against the composition it replaces
(hip_ops.adacof_composed: gathers and element-wise torch ops with autograd, the same definition in fp32) at F = 5, dilation 1, timed with
HIP events after a warm-up, the two alternating in one process, five windows each; then one `--model adacof` meta-iteration (seeded
weights, synthetic 256 x 448 septuplets, the product's default execution mode).  The achieved bytes per second count every operand once
(hip_ops.adacof_bytes).  There is no speed gate with one exception: the fused forward + backward must not be slower than the composition
(the script exits non-zero if it is).  Needs a GPU.  Writes profiles/adacof_bench.txt.

    python tools/adacof_bench.py [--iters 50] [--tasks 4] [--steps 2] [--out profiles/adacof_bench.txt]
"""
import argparse
import contextlib
import os
import sys
import tempfile
import time

os.environ.setdefault('MIOPEN_USER_DB_PATH', tempfile.mkdtemp(prefix='savfi_adacof_bench_miopen_'))
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from meta_interpolation_amd import hip_ops, synthetic  # noqa: E402

SHAPES = [(1, 3, 256, 448), (1, 3, 720, 1280)]
F, D = 5, 1


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def op_lines(iters):
    lines, slower = [], []
    for N, C, H, W in SHAPES:
        gen = torch.Generator().manual_seed(0)
        rim = (F - 1) * D
        x = torch.rand(N, C, H + rim, W + rim, generator=gen).cuda()
        w = torch.softmax(torch.randn(N, F * F, H, W, generator=gen), 1).cuda().requires_grad_()
        a = (0.5 * torch.randn(N, F * F, H, W, generator=gen)).cuda().requires_grad_()
        b = (0.5 * torch.randn(N, F * F, H, W, generator=gen)).cuda().requires_grad_()
        gout = torch.randn(N, C, H, W, generator=gen).cuda()
        det = [t.detach() for t in (w, a, b)]
        runs = {
            'fwd': (lambda: hip_ops.adacof(x, *det, D), lambda: hip_ops.adacof_composed(x, *det, D)),
            'fwd+bwd': (lambda: torch.autograd.grad(hip_ops.adacof(x, w, a, b, D), (w, a, b), gout),
                        lambda: torch.autograd.grad(hip_ops.adacof_composed(x, w, a, b, D), (w, a, b), gout)),
        }
        dv = float((runs['fwd'][0]() - runs['fwd'][1]()).abs().max())
        dg = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(runs['fwd+bwd'][0](), runs['fwd+bwd'][1]()))
        nbytes = {'fwd': hip_ops.adacof_bytes(x, w), 'fwd+bwd': hip_ops.adacof_bytes(x, w) + hip_ops.adacof_bytes(x, w, 3)}
        for what, (fused, composed) in runs.items():
            for _ in range(5):
                fused(), composed()
            torch.cuda.synchronize()
            tf, tc = [], []
            for rep in range(5):          # alternate the two
                tf.append(timed(fused, iters))
                tc.append(timed(composed, max(1, iters // 5)))
            lines.append('%-14s F=%d d=%d %-8s fused %8.1f us (min of 5; %s; %.0f GB/s of operand bytes)   composed %9.1f us (%s)   ratio %.1fx   '
                         'max |dvalue| %.1e  max |dgrad| / max |grad| %.1e'
                         % ('x'.join(map(str, (N, C, H, W))), F, D, what, min(tf), ' '.join('%.1f' % t for t in tf), nbytes[what] / min(tf) / 1e3,
                            min(tc), ' '.join('%.1f' % t for t in tc), min(tc) / min(tf), dv, dg))
            print(lines[-1], flush=True)
            if what == 'fwd+bwd' and min(tf) > min(tc):
                slower.append(lines[-1])
        del runs
        torch.cuda.empty_cache()
    return lines, slower


def iteration_line(tasks, steps):
    from meta_interpolation_amd.config import default_args
    from meta_interpolation_amd.meta_learning_system import MODEL_REGISTRY, SceneAdaptiveInterpolation
    args = default_args(model='adacof', num_gpu=1, batch_size=tasks, number_of_training_steps_per_iter=steps,
                        number_of_evaluation_steps_per_iter=steps, optimizer='SGD', inner_lr=1e-3, loss='1*L1')
    with contextlib.redirect_stdout(sys.stderr):
        net = MODEL_REGISTRY['adacof'](args, False)
        synthetic.load_seeded_weights(net, 'adacof')
        system = SceneAdaptiveInterpolation(args, net=net.cuda())
    frames = [f.cuda() for f in synthetic.septuplet_batch(tasks, 256, 448, model='adacof')]
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
    return ('--model adacof meta-iteration: %d tasks x %d inner steps, 256 x 448, SGD, L1, default mode: %.1f ms (min of 5; %s); loss %.6f -> %.6f'
            % (tasks, steps, min(times), ' '.join('%.1f' % t for t in times), first, last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--tasks', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'adacof_bench.txt'))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/adacof_bench.py needs a GPU: a timing taken anywhere else says nothing")
    lines, slower = op_lines(o.iters)
    lines.append(iteration_line(o.tasks, o.steps))
    print(lines[-1], flush=True)
    with open(o.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    if slower:
        raise SystemExit("the fused forward + backward is slower than the composition it replaces:\n" + '\n'.join(slower))


if __name__ == '__main__':
    main()
