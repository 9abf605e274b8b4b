"""-m gpu: SceneAdaptiveInterpolation with --model dain on synthetic 64x64 septuplets, batch 2, Adamax + Meta-SGD (scripts/run_dain.sh),
one and two inner steps, with and without the multi-step loss.

What is checked: the iteration runs and its loss is finite; the inner-loop dictionary has the ten rectifyNet names; every tensor outside
rectifyNet is frozen and bit-unchanged by run_train_iter while the rectify tensors and their learning rates move; the frozen front is
evaluated 3 times per task and iteration whatever the number of steps; the same iteration with the reuse switched off (the reference's
structure) gives the same loss, parameters and running buffers bit for bit; the depth net's running buffers are, within the gate of
tests/test_dain_net_gpu.py, those of the float64 restatement applied once per reference forward in the reference's order; a validation
iteration returns PSNR / SSIM; a 40x72 input comes back at its own size.
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import synthetic
from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
from meta_interpolation_amd.loss import CharbonnierLoss
from meta_interpolation_amd.meta_learning_system import SceneAdaptiveInterpolation
from tests import dain_net_ref as R
from tests.test_dain_net_gpu import FLOOR, K, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCH = 2


def build(steps=1, msl=False, reuse=True, fuse=1, batch=BATCH):
    args = default_args(model='dain', num_gpu=1, loss='1*L1', optimizer='Adamax', metasgd=True, batch_size=batch,
                        number_of_training_steps_per_iter=steps, number_of_evaluation_steps_per_iter=steps,
                        use_multi_step_loss_optimization=msl, multi_step_loss_num_epochs=5, fuse_support_pairs=fuse,
                        graph_inner_loop=1, task_streams=1)         # (graph_inner_loop=1: the plugin must decline it)
    net = MetaDAIN()
    net.load_state_dict({k: v.clone() for k, v in weights().items()}, strict=True)
    net.reuse_front = reuse
    return SceneAdaptiveInterpolation(args, net=net)


@functools.lru_cache(maxsize=None)
def batch(height=64, width=64, tasks=BATCH):
    return synthetic.septuplet_batch(tasks, height, width, model='dain')


def snapshot(system):
    return {k: v.detach().clone() for k, v in system.state_dict().items()}


@pytest.mark.parametrize("steps, msl", ((1, False), (1, True), (2, False), (2, True)))
def test_train_iteration_and_its_twin_without_reuse(steps, msl):
    system = build(steps, msl)
    names = list(system.get_inner_loop_parameter_dict(system.net.named_parameters()))
    assert names == ['rectifyNet.' + k for k in R.RECTIFY_NAMES]
    assert isinstance(system.criterion, CharbonnierLoss)
    frozen = [k for k, p in system.net.named_parameters() if not k.startswith('rectifyNet.')]
    assert frozen and all(not p.requires_grad for k, p in system.net.named_parameters() if not k.startswith('rectifyNet.'))
    before = snapshot(system)
    losses, preds, _ = system.run_train_iter(batch(), 0)
    loss = float(losses['loss'])
    assert np.isfinite(loss) and set(losses) >= {'loss', 'total', 'DAIN'}
    assert len(preds) == BATCH and all(tuple(p.shape) == (1, 3, 64, 64) for p in preds)
    assert system.net.front_evaluations == 3 * BATCH                                  # two supports and the target, per task
    after = snapshot(system)
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    for k in before:
        if k.startswith('net.') and not k.startswith('net.rectifyNet.') and not k.endswith(buffers):
            assert torch.equal(before[k], after[k]), k                                  # frozen: not one bit moved
    assert all(not torch.equal(before['net.' + k], after['net.' + k]) for k in names)
    lrs = [k for k in before if not k.startswith('net.')]                               # the Meta-SGD learning rates
    assert lrs and any(not torch.equal(before[k], after[k]) for k in lrs)
    forwards = steps * 2 + (steps if msl else 1)                                        # reference forwards per task
    assert all(int(after[k]) == BATCH * forwards for k in after if k.endswith('num_batches_tracked'))

    twin = build(steps, msl, reuse=False)
    losses2, _, _ = twin.run_train_iter(batch(), 0)
    assert twin.net.front_evaluations == BATCH * forwards                              # recomputed on every pass
    assert float(losses2['loss']) == loss
    after2 = snapshot(twin)
    assert set(after2) == set(after)
    for k in after:
        assert torch.equal(after[k], after2[k]), k


def test_running_buffers_follow_the_reference_forwards_in_order():
    """One inner step, no multi-step loss: per task the reference runs support (0,4), support (2,6), then the target (2,4), each a depth-net
    forward on its two frames that moves the running buffers; then the next task."""
    system = build(1, False)
    frames = batch()
    system.run_train_iter(frames, 0)
    torch.cuda.synchronize()
    got = {k[len('net.depthNet.'):]: v.cpu() for k, v in system.state_dict().items() if k.startswith('net.depthNet.')}
    sd = {k[len('depthNet.'):]: v for k, v in weights().items() if k.startswith('depthNet.')}
    refs = []
    for dtype in (torch.float32, torch.float64):
        state = sd
        for task in range(BATCH):
            for a, b in ((0, 4), (2, 6), (2, 4)):
                _, state = R.hourglass_forward(state, torch.stack((frames[a][task], frames[b][task])), dtype, True)
        refs.append(state)
    for kind in ('running_mean', 'running_var'):
        keys = [k for k in got if k.endswith(kind)]
        cat = lambda d: torch.cat([d[k].double().flatten() for k in keys]).numpy()
        g, r32, r64 = cat(got), cat(refs[0]), cat(refs[1])
        E, scale = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
        gate, err = max(K * E, FLOOR * scale), float(np.abs(g - r64).max())
        print('DAIN_NET_PARITY system_%s err=%.3e E=%.3e scale=%.3e gate=%.3e err/gate=%.3f' % (kind, err, E, scale, gate, err / gate))
        assert err <= gate, (kind, err, gate)
    assert all(int(got[k]) == 3 * BATCH for k in got if k.endswith('num_batches_tracked'))


def test_unfused_support_passes_give_three_fronts_per_task_too():
    system = build(2, False, fuse=0)
    losses, _, _ = system.run_train_iter(batch(), 0)
    assert np.isfinite(float(losses['loss'])) and system.net.front_evaluations == 3 * BATCH


def test_validation_iteration_returns_psnr_and_ssim():
    system = build(1, False)
    before = {k: v.clone() for k, v in system.net.state_dict().items() if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
    losses, preds, metrics = system.run_validation_iter(batch())
    assert np.isfinite(float(losses['loss']))
    assert metrics['psnr'].count == BATCH and np.isfinite(metrics['psnr'].avg) and 0.0 <= float(metrics['ssim'].avg) <= 1.0
    assert all(tuple(p.shape) == (1, 3, 64, 64) for p in preds)
    assert all(torch.equal(v, system.net.state_dict()[k]) for k, v in before.items())   # validation moves no parameter


def test_padded_size_comes_back_at_the_inputs_size():
    system = build(1, False, batch=1)
    frames = batch(40, 72, 1)
    losses, preds, _ = system.run_train_iter(frames, 0)
    assert np.isfinite(float(losses['loss'])) and tuple(preds[0].shape) == (1, 3, 40, 72)
    losses, preds, metrics = system.run_validation_iter(frames)
    assert tuple(preds[0].shape) == (1, 3, 40, 72) and np.isfinite(metrics['psnr'].avg)
