"""-m gpu: the census term inside whole meta-iterations.

The Census term of --loss ('1*L1+1*Census', an addition: the reference's Loss has no such branch, so there is no reference fixture) on
CAIN, two synthetic 64 x 64 tasks, one train iteration: the lockstep and the graphed lockstep mode (two calls: the second replays the
captured graphs) agree with the sequential task loop within the contract bounds tests/test_system_gpu.py holds every mode to -- loss,
term, predictions, metrics and the outer gradients' fingerprints, which carry the census backward of every mode -- and the logged term
is the float64 restatement on the returned predictions within the kernel's tightest value gate (a network's prediction is of none of
the fixture's content kinds).
"""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import synthetic
from tests import census_ref as Z
from tests.helpers import assert_fp_close, build_system, fp, golden, parse_case_args
from tests.test_census_gpu import tightest_gates
from tests.test_system_gpu import lockstep_for  # noqa: F401  (a fixture)
from tests.test_system_gpu import tolerances as contract_tolerances

pytestmark = pytest.mark.gpu

CASE = 'cain_l1_ssim_1step'          # its `args`: CAIN, SGD, one inner step; the loss string is replaced
MODES = {'sequential': dict(task_batch=0), 'lockstep': dict(task_batch=2), 'graphed_lockstep': dict(task_batch=2, graph_inner_loop=1)}


def run(mode, lockstep_for, reps=1):
    g = golden("system_" + CASE)
    over = dict(parse_case_args(g), batch_size=2, loss='1*L1+1*Census', **MODES[mode])
    system = build_system('cain', over)
    if 'lockstep' in mode:
        lockstep_for(system, 'cain')
    system.outer_fp = {}          # the optimizer does not step: it records the outer gradients it was handed
    system.optimizer.step = lambda *a, **k: system.outer_fp.update(
        {n: fp(p.grad) for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    frames = synthetic.septuplet_batch(2, 64, 64, model='cain')
    for _ in range(reps):          # a second call replays the captured graphs
        losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
        torch.cuda.synchronize()
    if 'graphed' in mode:
        assert len(system._graphs) == 1
    return system, frames, losses, preds, metrics


def test_the_loss_term_in_every_task_mode(lockstep_for):
    tol = contract_tolerances(CASE, 'train')
    runs = {mode: run(mode, lockstep_for, reps=2 if 'graphed' in mode else 1) for mode in MODES}
    system, frames, losses, preds, metrics = runs['sequential']
    assert sorted(k for k in losses if not k.startswith('loss')) == ['Census', 'L1', 'total']
    # the logged term against the restatement on the predicted frames
    want = 0.0
    for t in range(2):
        tgt = frames[system.target_idxs[1]][t:t + 1].double()
        want += float(Z.census(preds[t].double().cpu().reshape(tgt.shape), tgt)) / 2
    e = abs(float(losses['Census']) - want)
    print('CENSUS_SYSTEM term=%.8f restatement=%.8f e=%.3e gate=%.3e' % (float(losses['Census']), want, e, tightest_gates()[0]))
    assert want > 0 and e <= tightest_gates()[0]
    assert system.outer_fp and all(np.isfinite(row).all() for row in system.outer_fp.values())
    assert abs(float(losses['total']) - float(losses['L1']) - float(losses['Census'])) <= 1e-6 * float(losses['total'])
    for mode in ('lockstep', 'graphed_lockstep'):
        other, _, l, p, m = runs[mode]
        d_loss = abs(l['loss'].item() - losses['loss'].item()) / abs(losses['loss'].item())
        d_term = abs(float(l['Census']) - float(losses['Census'])) / abs(float(losses['Census']))
        d_l1 = max((a - b).abs().mean().item() for a, b in zip(p, preds))
        print('CENSUS_SYSTEM mode=%s d_loss=%.3e d_term=%.3e (bound %.0e) d_preds=%.3e (bound %.0e)'
              % (mode, d_loss, d_term, tol['loss'], d_l1, tol['l1']))
        assert d_loss <= tol['loss'] and d_term <= tol['loss'] and d_l1 < tol['l1']
        assert abs(m['psnr'].avg - metrics['psnr'].avg) < tol['psnr'] and abs(float(m['ssim'].avg) - float(metrics['ssim'].avg)) < tol['ssim']
        # the outer gradients: every inner and outer backward of the mode went through the census term
        assert set(other.outer_fp) == set(system.outer_fp)
        d_outer = max(max(abs(other.outer_fp[k][i] - row[i]) for i in (0, 1)) / max(abs(row[1]), 1e-12) for k, row in system.outer_fp.items())
        print('CENSUS_SYSTEM mode=%s d_outer=%.3e (bound %.0e)' % (mode, d_outer, tol['outer']))
        for k, row in system.outer_fp.items():
            assert_fp_close(other.outer_fp[k], row, tol['outer'], (mode, 'outer', k))
