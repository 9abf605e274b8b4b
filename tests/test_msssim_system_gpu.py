"""-m gpu: multi-scale SSIM inside whole meta-iterations.

* The MSSSIM term of --loss ('1*L1+0.1*MSSSIM', an addition: the reference's Loss has no such branch, so there is no reference
  fixture) on CAIN, two synthetic 64 x 64 tasks, one train iteration: the lockstep and the graphed lockstep mode agree with the
  sequential task loop within the contract bounds tests/test_system_gpu.py holds every mode to -- loss, term, predictions, metrics and
  the outer gradients' fingerprints, which carry the MSSSIM backward of every mode -- and the logged term is 0.1 (1 - float64
  restatement) of the returned predictions within 0.1 x the kernel's gate.
* The metric of --eval_msssim 1 in the three task bodies (sequential, lockstep, graphed) and in the half-split path of the
  ExperimentBuilder: `msssim` for every task, equal to the float64 restatement on the quantised frames within the gate; evaluating
  it changes nothing else; with the default the keys are as before.

Gate of the comparisons with the restatement: a network's prediction is of none of the fixture's content kinds, so these tests take
`tightest_gates`, the smallest max(3 E_kind, floor) any kind gives for the `normalize` setting.
"""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import synthetic, utils
from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.experiment_builder import ExperimentBuilder
from tests import msssim_ref as M
from tests.helpers import assert_fp_close, build_system, fp, golden, parse_case_args
from tests.test_msssim_gpu import tightest_gates
from tests.test_system_gpu import lockstep_for  # noqa: F401  (a fixture)
from tests.test_system_gpu import tolerances as contract_tolerances

pytestmark = pytest.mark.gpu

CASE = 'cain_l1_ssim_1step'          # its `args`: CAIN, SGD, one inner step; the loss string is replaced
MODES = {'sequential': dict(task_batch=0), 'lockstep': dict(task_batch=2), 'graphed_lockstep': dict(task_batch=2, graph_inner_loop=1),
         'graphed': dict(task_batch=0, graph_inner_loop=1)}


def run(mode, lockstep_for, loss='1*L1+0.1*MSSSIM', eval_msssim=0, do_evaluation=True, reps=1):
    g = golden("system_" + CASE)
    over = dict(parse_case_args(g), batch_size=2, loss=loss, eval_msssim=eval_msssim, **MODES[mode])
    system = build_system('cain', over)
    if 'lockstep' in mode:
        lockstep_for(system, 'cain')
    system.outer_fp = {}          # the optimizer does not step: it records the outer gradients it was handed
    system.optimizer.step = lambda *a, **k: system.outer_fp.update(
        {n: fp(p.grad) for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    frames = synthetic.septuplet_batch(2, 64, 64, model='cain')
    for _ in range(reps):          # a second call replays the captured graphs
        losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=do_evaluation)
        torch.cuda.synchronize()
    if 'graphed' in mode:
        assert len(system._graphs) == 1
    return system, frames, losses, preds, metrics


def test_the_loss_term_in_every_task_mode(lockstep_for):
    tol = contract_tolerances(CASE, 'train')
    runs = {mode: run(mode, lockstep_for, reps=2 if 'graphed' in mode else 1) for mode in ('sequential', 'lockstep', 'graphed_lockstep')}
    system, frames, losses, preds, metrics = runs['sequential']
    assert sorted(k for k in losses if not k.startswith('loss')) == ['L1', 'MSSSIM', 'total']
    # the logged term against the restatement on the predicted frames
    want = 0.0
    for t in range(2):
        tgt = frames[system.target_idxs[1]][t:t + 1].double()
        want += 0.1 * (1 - float(M.msssim(preds[t].double().cpu(), tgt, None, True))) / 2
    e = abs(float(losses['MSSSIM']) - want)
    print('MSSSIM_SYSTEM term=%.8f restatement=%.8f e=%.3e gate=%.3e' % (float(losses['MSSSIM']), want, e, 0.1 * tightest_gates(1)[0]))
    assert e <= 0.1 * tightest_gates(1)[0]
    assert system.outer_fp and all(np.isfinite(row).all() for row in system.outer_fp.values())
    assert abs(float(losses['total']) - float(losses['L1']) - float(losses['MSSSIM'])) <= 1e-6 * float(losses['total'])
    for mode in ('lockstep', 'graphed_lockstep'):
        other, _, l, p, m = runs[mode]
        d_loss = abs(l['loss'].item() - losses['loss'].item()) / abs(losses['loss'].item())
        d_term = abs(float(l['MSSSIM']) - float(losses['MSSSIM'])) / abs(float(losses['MSSSIM']))
        d_l1 = max((a - b).abs().mean().item() for a, b in zip(p, preds))
        print('MSSSIM_SYSTEM mode=%s d_loss=%.3e d_term=%.3e (bound %.0e) d_preds=%.3e (bound %.0e)'
              % (mode, d_loss, d_term, tol['loss'], d_l1, tol['l1']))
        assert d_loss <= tol['loss'] and d_term <= 5 * tol['loss'] and d_l1 < tol['l1']
        assert abs(m['psnr'].avg - metrics['psnr'].avg) < tol['psnr'] and abs(float(m['ssim'].avg) - float(metrics['ssim'].avg)) < tol['ssim']
        # the outer gradients: every inner and outer backward of the mode went through the MSSSIM term
        assert set(other.outer_fp) == set(system.outer_fp)
        d_outer = max(max(abs(other.outer_fp[k][i] - row[i]) for i in (0, 1)) / max(abs(row[1]), 1e-12) for k, row in system.outer_fp.items())
        print('MSSSIM_SYSTEM mode=%s d_outer=%.3e (bound %.0e)' % (mode, d_outer, tol['outer']))
        for k, row in system.outer_fp.items():
            assert_fp_close(other.outer_fp[k], row, tol['outer'], (mode, 'outer', k))


@pytest.mark.parametrize("mode", ['sequential', 'lockstep', 'graphed'])
def test_eval_flag_adds_the_metric_in_every_task_body(mode, lockstep_for):
    system, frames, losses, preds, metrics = run(mode, lockstep_for, loss='1*L1', eval_msssim=1)
    _, _, losses0, preds0, metrics0 = run(mode, lockstep_for, loss='1*L1', eval_msssim=0)
    assert sorted(metrics0) == ['psnr', 'ssim'] and sorted(metrics) == ['msssim', 'psnr', 'ssim']
    assert metrics['msssim'].count == 2 and metrics['psnr'].count == 2
    assert torch.equal(losses['loss'], losses0['loss']) and all(torch.equal(a, b) for a, b in zip(preds, preds0))
    assert metrics['psnr'].avg == metrics0['psnr'].avg and float(metrics['ssim'].avg) == float(metrics0['ssim'].avg)
    tgt = frames[system.target_idxs[1]]
    want = float(M.metric_rows(torch.cat([p.cpu() for p in preds]), tgt).mean())
    e = abs(float(metrics['msssim'].avg) - want)
    print('MSSSIM_SYSTEM metric mode=%s msssim=%.7f e=%.3e gate=%.3e' % (mode, want, e, tightest_gates(0)[0]))
    assert e <= tightest_gates(0)[0]
    _, _, _, _, none = run(mode, lockstep_for, loss='1*L1', eval_msssim=1, do_evaluation=False)
    assert none['msssim'].count == 0


class _Halves:
    """run_validation_iter of a model that returns the target frame with a little noise: what the stitched-halves path needs."""

    def __init__(self):
        self.calls = []

    def run_validation_iter(self, data_batch):
        self.calls.append(tuple(data_batch[0].shape))
        out = (data_batch[3] + 0.01 * torch.sin(torch.arange(data_batch[3].numel(), device='cuda', dtype=torch.float32)
                                                ).view_as(data_batch[3])).clamp(0, 1)
        return {'loss': (out - data_batch[3]).abs().mean(), 'total': 0.0}, [out[0]], None


def test_eval_flag_in_the_half_split_path():
    frames = [f.cuda() for f in synthetic.septuplet_batch(1, 720, 704, model='cain')]          # > 5e5 pixels: two halves, stitched
    for flag in (0, 1):
        model = _Halves()
        args = default_args(model='cain', num_gpu=1, eval_msssim=flag, synthetic=True)
        eb = ExperimentBuilder.__new__(ExperimentBuilder)
        eb.args, eb.model = args, model
        losses, outputs, metrics = eb.evaluation_iteration((frames, {}))
        assert model.calls == [(1, 3, 360, 704)] * 2 and tuple(outputs[0].shape) == (3, 720, 704)
        assert sorted(metrics) == (['msssim', 'psnr', 'ssim'] if flag else ['psnr', 'ssim'])
        if flag:
            want = float(M.metric_rows(outputs[0].unsqueeze(0).cpu(), frames[3].cpu())[0])
            assert abs(metrics['msssim'].avg - want) <= tightest_gates(0)[0]
            assert ExperimentBuilder._msssim_suffix(metrics).startswith(",  MS-SSIM: ")
        else:
            assert ExperimentBuilder._msssim_suffix(metrics) == ""
        assert utils.msssim_rows(outputs[0].unsqueeze(0).cpu(), frames[3].cpu()).shape == (1,)          # the host composition
