"""-m gpu: --model softsplat inside whole meta-iterations.

Two synthetic 128 x 128 tasks, SGD, LSLR with learnable rates, two inner steps, one train iteration.  There is no reference plugin and so
no fixture: the lockstep mode and the graphed lockstep mode (two calls: the second replays the captured graphs) are held to the sequential
task loop within the contract bounds tests/test_system_gpu.py holds every mode to -- loss, predictions, PSNR / SSIM and the outer
gradients' fingerprints.  One more case runs --second_order --warp_second_order 1 sequentially (the composed op, the twice-differentiable
warp under the metric): finite loss and outer gradients, and learning-rate gradients that differ from the first-order run's -- the
second-order path is live.
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops, model_utils, synthetic
from tests.helpers import assert_fp_close, build_system, fp
from tests.test_system_gpu import CONTRACT
from tests.test_system_gpu import lockstep_for  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ARGS = dict(optimizer='SGD', inner_lr=1e-3, loss='1*L1', learnable_per_layer_per_step_inner_loop_learning_rate=True,
            number_of_training_steps_per_iter=2, number_of_evaluation_steps_per_iter=2, batch_size=2)
MODES = {'sequential': dict(task_batch=0), 'lockstep': dict(task_batch=2), 'graphed_lockstep': dict(task_batch=2, graph_inner_loop=1),
         'second_order': dict(task_batch=0, second_order=True, first_order_to_second_order_epoch=-1, warp_second_order=1)}
SIZE = 128


def run(mode, lockstep_for=None, reps=1):
    system = build_system('softsplat', dict(ARGS, **MODES[mode]))
    if 'lockstep' in mode:
        lockstep_for(system, 'softsplat')
        calls = []
        body = system._lockstep_body
        system._lockstep_body = lambda *a, **k: (calls.append(len(a[1])), body(*a, **k))[1]
    system.outer_fp = {}          # the optimizer does not step: it records the outer gradients it was handed
    system.optimizer.step = lambda *a, **k: system.outer_fp.update(
        {n: fp(p.grad) for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    frames = synthetic.septuplet_batch(2, SIZE, SIZE, model='softsplat')
    flags = (hip_ops.double_backward(), model_utils.fuse_conv_act(), hip_ops.warp_second_order())   # the pass switches are per thread and
    try:                                                                   # outlive the pass: hand the later suites the thread as it was
        for _ in range(reps):          # a second call replays the captured graphs
            losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
            torch.cuda.synchronize()
    finally:
        hip_ops.set_double_backward(flags[0])
        model_utils.set_fuse_conv_act(flags[1])
        hip_ops.set_warp_second_order(flags[2])
    if mode == 'lockstep':
        assert calls == [2]
    if 'graphed' in mode:
        assert len(system._graphs) == 1 and next(iter(system._graphs.values())).T == 2
    return dict(loss=losses['loss'].item(), preds=[p.detach().cpu() for p in preds], psnr=metrics['psnr'].avg, ssim=float(metrics['ssim'].avg),
                outer=dict(system.outer_fp))


@functools.lru_cache(maxsize=None)
def sequential():
    return run('sequential')


@pytest.mark.parametrize("mode", ['lockstep', 'graphed_lockstep'])
def test_task_modes_equal_the_sequential_loop(mode, lockstep_for):
    tol = dict(CONTRACT)
    want, got = sequential(), run(mode, lockstep_for, reps=2 if 'graphed' in mode else 1)
    assert np.isfinite(want['loss']) and want['outer'] and all(np.isfinite(row).all() for row in want['outer'].values())
    assert 'net.alpha' in want['outer'] or any(k.endswith('alpha') for k in want['outer'])      # the metric's scale is meta-learned
    assert all(p.shape == (1, 3, SIZE, SIZE) or p.shape == (3, SIZE, SIZE) for p in want['preds'])
    d_loss = abs(got['loss'] - want['loss']) / abs(want['loss'])
    d_l1 = max((a - b).abs().mean().item() for a, b in zip(got['preds'], want['preds']))
    d_outer = max(max(abs(got['outer'][k][i] - row[i]) for i in (0, 1)) / max(abs(row[1]), 1e-12) for k, row in want['outer'].items())
    print('SOFTSPLAT_SYSTEM mode=%s d_loss=%.3e (bound %.0e) d_preds=%.3e (bound %.0e) d_psnr=%.3e d_ssim=%.3e d_outer=%.3e (bound %.0e)'
          % (mode, d_loss, tol['loss'], d_l1, tol['l1'], abs(got['psnr'] - want['psnr']), abs(got['ssim'] - want['ssim']), d_outer, tol['outer']))
    assert d_loss <= tol['loss'] and d_l1 < tol['l1']
    assert abs(got['psnr'] - want['psnr']) < tol['psnr'] and abs(got['ssim'] - want['ssim']) < tol['ssim']
    assert set(got['outer']) == set(want['outer'])
    for k, row in want['outer'].items():
        assert_fp_close(got['outer'][k], row, tol['outer'], (mode, 'outer', k))


def test_second_order_path_is_live():
    first, second = sequential(), run('second_order')
    assert np.isfinite(second['loss']) and all(np.isfinite(row).all() for row in second['outer'].values())
    assert set(second['outer']) == set(first['outer'])
    # the loss of the adapted weights is the same forward computation, through the composed op (float32 sums in arrival order, held to
    # 1e-4 of the scale per call in tests/test_softsplat_gpu.py) in six passes: 1e-3; the learning rates' gradients carry the second-order terms
    assert abs(second['loss'] - first['loss']) <= 1e-3 * abs(first['loss'])
    rates = [k for k in first['outer'] if 'names_learning_rates' in k and abs(first['outer'][k][1]) > 0]
    assert rates
    moved = [k for k in rates if abs(second['outer'][k][1] - first['outer'][k][1]) > 1e-3 * abs(first['outer'][k][1])]
    print('SOFTSPLAT_SYSTEM second order: loss %.8f (first order %.8f), %d of %d learning-rate gradients moved by more than 1e-3'
          % (second['loss'], first['loss'], len(moved), len(rates)))
    assert moved
