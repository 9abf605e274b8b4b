"""-m gpu: --model dain --dain_task_modes 1 -- MetaDAIN's tasks adapted in lockstep (--task_batch) and from captured hipGraphs
(--graph_inner_loop) -- against the sequential eager loop, on synthetic 64 x 64 septuplets and seeded weights, with SGD (LSLR) and with
the script's configuration, Adamax + Meta-SGD.

The gates are this project's own for lockstep against sequential on plugins whose layers all run on its kernels
(tests/test_system_gpu.py::test_lockstep_equals_the_sequential_loop): loss 2e-5 relative, predictions 1e-4 mean absolute, PSNR 1e-3 dB,
every non-zero outer gradient within 2e-3 of its absolute sum (SGD) or 5e-2 (the sign-based rule) plus helpers.FP_ATOL.  SSIM, which that
test does not gate, is held to 1e-4: it is a mean in [0, 1] of the same quantised images whose pixels are held to 1e-4 mean absolute.
The depth net's running buffers and num_batches_tracked are not gated but compared bit for bit: a pair's front, and so its batch
statistics, does not depend on the batch it was computed in, and the updates are replayed in the sequential loop's order.

The outer step is recorded and not applied (as in the test the gates come from), so that a second iteration starts from the same
weights in both runs and differs only where it should: in its frames.
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import synthetic
from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
from meta_interpolation_amd.meta_learning_system import SceneAdaptiveInterpolation
from tests.helpers import FP_ATOL
from tests.test_dain_net_gpu import weights

pytestmark = pytest.mark.gpu
RULES = {'sgd': dict(optimizer='SGD', metasgd=False, inner_lr=1e-3), 'adamax_metasgd': dict(optimizer='Adamax', metasgd=True)}
BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked')


def build(rule, modes, *, steps=2, msl=False, tasks=3, task_batch=2, graph=0, reuse=True):
    args = default_args(model='dain', num_gpu=1, loss='1*L1', batch_size=tasks, number_of_training_steps_per_iter=steps,
                        number_of_evaluation_steps_per_iter=steps, use_multi_step_loss_optimization=msl, multi_step_loss_num_epochs=5,
                        graph_inner_loop=graph, task_streams=1, task_batch=task_batch,
                        **({} if modes is None else {'dain_task_modes': modes}), **RULES[rule])
    net = MetaDAIN()
    net.load_state_dict({k: v.clone() for k, v in weights().items()}, strict=True)
    net.reuse_front = reuse
    system = SceneAdaptiveInterpolation(args, net=net)
    system.lockstep_calls = []
    body = system._lockstep_body
    system._lockstep_body = lambda frames, ids, **kw: (system.lockstep_calls.append(len(ids)), body(frames, ids, **kw))[1]
    system.outer = {}
    system.optimizer.step = lambda *a, **k: system.outer.update(
        {n: p.grad.detach().clone() for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    return system


@functools.lru_cache(maxsize=None)
def batch(tasks, height=64, width=64, first=0):
    return synthetic.septuplet_batch(tasks, height, width, model='dain', first_task=first)


def train(system, frames):
    system.outer.clear()
    losses, preds, metrics = system.run_train_iter(frames, 0, do_evaluation=True)
    torch.cuda.synchronize()
    return dict(loss=float(losses['loss']), preds=torch.stack([p.squeeze(0) for p in preds]), psnr=float(metrics['psnr'].avg),
                ssim=float(metrics['ssim'].avg), outer=dict(system.outer), buffers=depth_buffers(system))


def depth_buffers(system):
    return {k: v.detach().clone() for k, v in system.net.depthNet.state_dict().items() if k.endswith(BUFFERS)}


def compare(tag, got, want, rule):
    """`got` against `want` (the sequential loop, or the eager twin) under the gates of the module's docstring; prints every ratio."""
    lim = 2e-3 if rule == 'sgd' else 5e-2
    r_loss = abs(got['loss'] - want['loss']) / abs(want['loss'])
    r_pred = (got['preds'] - want['preds']).abs().mean().item()
    r_psnr = abs(got['psnr'] - want['psnr'])
    worst, worst_key = 0.0, None
    compared = 0
    for k, v in want['outer'].items():
        total = v.abs().sum().item()
        if total == 0:
            continue
        assert k in got['outer'], k
        compared += 1
        ratio = (got['outer'][k] - v).abs().sum().item() / (lim * total + FP_ATOL)
        if ratio > worst:
            worst, worst_key = ratio, k
    moved = [k for k in want['buffers'] if not torch.equal(got['buffers'][k], want['buffers'][k])]
    print("DAIN_MODES_PARITY %s loss/gate=%.2e preds/gate=%.2e psnr/gate=%.2e outer/gate=%.2e (%s, %d tensors) buffers_differing=%d of %d"
          % (tag, r_loss / 2e-5, r_pred / 1e-4, r_psnr / 1e-3, worst, worst_key, compared, len(moved), len(want['buffers'])))
    assert np.isfinite(got['loss']) and np.isfinite(want['loss'])
    assert r_loss <= 2e-5, (tag, got['loss'], want['loss'])
    assert r_pred < 1e-4 and r_psnr < 1e-3, (tag, r_pred, r_psnr)
    assert compared >= 10 and worst <= 1.0, (tag, worst_key, worst)
    assert set(got['buffers']) == set(want['buffers']) and not moved, (tag, moved[:3])


@pytest.mark.parametrize("msl", (False, True))
@pytest.mark.parametrize("rule", list(RULES))
def test_lockstep_equals_the_sequential_loop(rule, msl):
    """3 tasks in groups of up to 2: one lockstep group of 2 and a sequential straggler, 2 inner steps."""
    frames = batch(3)
    runs = {}
    for modes in (0, 1):
        system = build(rule, modes, msl=msl)
        runs[modes] = train(system, frames)
        assert system.lockstep_calls == ([2] if modes else [])
        assert system.net.front_evaluations == 9                  # two supports and the target, per task
        assert not system._graphs
        forwards = 2 * 2 + (2 if msl else 1)
        assert all(int(v) == 3 * forwards for k, v in runs[modes]['buffers'].items() if k.endswith('num_batches_tracked'))
    assert tuple(runs[1]['preds'].shape) == (3, 3, 64, 64)
    compare("lockstep_%s_msl%d" % (rule, msl), runs[1], runs[0], rule)


def test_validation_iteration_in_lockstep():
    frames = batch(3)
    rows = {}
    for modes in (0, 1):
        system = build('adamax_metasgd', modes)
        seen = []
        metric = system._eval_metrics
        system._eval_metrics = lambda p, t: (seen.append(metric(p, t)), seen[-1])[1]
        before = {k: v.clone() for k, v in system.state_dict().items() if not k.endswith(BUFFERS)}
        losses, preds, metrics = system.run_validation_iter(frames)
        torch.cuda.synchronize()
        assert system.lockstep_calls == ([2] if modes else [])
        assert all(torch.equal(v, system.state_dict()[k]) for k, v in before.items())          # validation moves no parameter
        assert metrics['psnr'].count == 3
        mse = torch.cat([m.reshape(-1) for m, _ in seen]).double().cpu()
        ssim = torch.cat([s.reshape(-1) for _, s in seen]).double().cpu()
        rows[modes] = dict(loss=float(losses['loss']), psnr=-10 * torch.log10(mse + 1e-8), ssim=ssim,
                           preds=torch.stack([p.squeeze(0) for p in preds]), buffers=depth_buffers(system))
        assert all(int(v) == 3 * (2 * 2 + 1) for k, v in rows[modes]['buffers'].items() if k.endswith('num_batches_tracked'))
    a, b = rows[1], rows[0]
    d_psnr, d_ssim = (a['psnr'] - b['psnr']).abs().max().item(), (a['ssim'] - b['ssim']).abs().max().item()
    print("DAIN_MODES_PARITY validation loss/gate=%.2e psnr/gate=%.2e ssim/gate=%.2e preds/gate=%.2e"
          % (abs(a['loss'] - b['loss']) / abs(b['loss']) / 2e-5, d_psnr / 1e-3, d_ssim / 1e-4,
             (a['preds'] - b['preds']).abs().mean().item() / 1e-4))
    assert a['psnr'].numel() == 3 and d_psnr < 1e-3 and d_ssim < 1e-4
    assert abs(a['loss'] - b['loss']) <= 2e-5 * abs(b['loss']) and (a['preds'] - b['preds']).abs().mean().item() < 1e-4
    assert all(torch.equal(a['buffers'][k], b['buffers'][k]) for k in b['buffers'])


def test_padded_frames_in_lockstep():
    frames = batch(2, 40, 72)
    runs = {}
    for modes in (0, 1):
        system = build('adamax_metasgd', modes, steps=1, tasks=2)
        losses, preds, _ = system.run_train_iter(frames, 0)
        torch.cuda.synchronize()
        assert system.lockstep_calls == ([2] if modes else [])
        assert all(tuple(p.shape) == (1, 3, 40, 72) for p in preds)
        runs[modes] = float(losses['loss'])
    print("DAIN_MODES_PARITY padded_40x72 loss/gate=%.2e" % (abs(runs[1] - runs[0]) / abs(runs[0]) / 2e-5))
    assert np.isfinite(runs[0]) and abs(runs[1] - runs[0]) <= 2e-5 * abs(runs[0])


@pytest.mark.parametrize("rule, tasks", (('sgd', 2), ('adamax_metasgd', 2), ('adamax_metasgd', 1)))
def test_graphs_follow_changing_batches(rule, tasks):
    """Two consecutive iterations on DIFFERENT batches, replayed from graphs, against the eager twin (lockstep for 2 tasks, the task loop
    for 1) on the same two batches: the second iteration is compared -- a front left over from the first batch fails it."""
    first, second = batch(tasks), batch(tasks, first=5)
    assert not torch.equal(first[0], second[0])
    runs = {}
    for graph in (0, 1):
        system = build(rule, 1, tasks=tasks, graph=graph, msl=True)
        train(system, first)
        runs[graph] = train(system, second)
        if graph:
            assert system._graphs and all(g.T == tasks for g in system._graphs.values()) and not system.lockstep_calls
            assert all(g.sup_kw and g.tgt_kw for g in system._graphs.values())
        else:
            assert not system._graphs and system.lockstep_calls == ([2, 2] if tasks == 2 else [])
        assert system.net.front_evaluations == 2 * 3 * tasks
    compare("graphs_%s_T%d" % (rule, tasks), runs[1], runs[0], rule)


def test_reuse_switched_off_takes_the_sequential_loop():
    system = build('adamax_metasgd', 1, graph=1, reuse=False)
    got = train(system, batch(3))
    assert not system.lockstep_calls and not system._graphs
    assert system.net.front_evaluations == 3 * (2 * 2 + 1)           # tasks x forwards: a front on every pass
    assert np.isfinite(got['loss'])


def test_default_enters_neither_mode():
    system = build('adamax_metasgd', None, graph=1)               # the option is not even named: this test holds on the tree before it existed
    got = train(system, batch(3))
    assert not system.lockstep_calls and not system._graphs
    assert not getattr(system.net, 'lockstep_tasks', False) and system.net.graph_capture is False
    assert MetaDAIN.graph_capture is False and not hasattr(MetaDAIN, 'lockstep_tasks')
    assert system.net.front_evaluations == 9 and np.isfinite(got['loss'])
