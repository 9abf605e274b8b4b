"""-m gpu: whole meta-iterations with a combined objective that has an SSIM term ('1*L1+0.1*SSIM', '1*MSE+0.1*SSIM') against
fixtures generated from the imported reference (tools/gen_golden_ssim.py -> tests/golden/system_*_ssim_*.npz), in every
execution mode, exactly as tests/test_system_gpu.py treats its cases and with that file's tolerances: `tolerances` (the
contract bounds plus its small-map rule for SepConv's outer gradients), widened to K_SPREAD x the reference's own spread where
that is larger.  The spread of these cases is measured by tools/gen_sensitivity_ssim.py (oracle/gen_sensitivity.py applied to
them: the reference against itself under two other convolution summation orders and in float64) and stored in
tests/golden/sensitivity_ssim.npz; the rule is applied to all three cases, as that file applies its table to all of its cases.
What it changes (largest stored spread per case; gate = max(contract, K x spread)):
  voxelflow_mse_ssim_2step  loss 2.85e-4 -> gate 8.5e-4 (contract 1e-5), pixel L1 1.9e-4 -> 5.7e-4, PSNR 1.06e-3 -> 3.2e-3 dB,
                            SSIM metric 5.7e-5 -> 1.7e-4,
                            weights 1.3e-5 -> 3.9e-5, per-step gradients 1.2e-3 -> 6.1e-3, outer gradients 7.1e-3 -> 3.6e-2:
                            its flow-to-pixel map amplifies convolution rounding, as in voxelflow_lslr_sgd_2step of that file.
                            At the contract bounds this case FAILS on the GPU (loss 7.6e-5 relative off; its MSE part alone, which
                            this change does not touch, 9.6e-5; the SSIM part 2.5e-5) -- the reference is 2.85e-4 from itself.
  sepconv_l1_ssim_2step     per-step gradients 3.5e-4 -> gate 1.7e-3 (contract 1e-3), outer gradients 3.7e-4 -> 1.9e-3 (below
                            that file's 5e-3 small-map rule); every other quantity stays at its contract bound.  The case
                            passed all tests at the contract bounds before the table existed.
  cain_l1_ssim_1step        nothing: every spread is below 5e-6, all gates are the contract bounds.

Range classes the reference's SSIM calls took (stored as `ssim_class_counts`): CAIN runs in L = 1, SepConv in L = 1 (12
calls) and L = 2 (8 calls: seeded weights give predictions below -0.5 in some passes), VoxelFlow (frames normalised to
[-1, 1]) in L = 2.
"""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import synthetic
from tests.helpers import assert_fp_close, build_system, fp, golden, observe, parse_case_args
from tests.test_system_gpu import K_SPREAD, knee_allowance, lockstep_for  # noqa: F401  (lockstep_for is a fixture)
from tests.test_system_gpu import tolerances as contract_tolerances

pytestmark = pytest.mark.gpu

CASES = ['sepconv_l1_ssim_2step', 'cain_l1_ssim_1step', 'voxelflow_mse_ssim_2step']
TWO_TASK = ['sepconv_l1_ssim_2step', 'voxelflow_mse_ssim_2step']


_SENS = golden("sensitivity_ssim")
_SENS_COL = {q: i for i, q in enumerate(_SENS['quantities'].tolist())}


def tolerances(name, phase='train'):
    """tests/test_system_gpu.tolerances, its spread rule read from this file's own sensitivity table."""
    tol = contract_tolerances(name, phase)
    table = _SENS['%s/%s' % (name, phase)]                              # [variant, quantity]
    for q in tol:
        tol[q] = max(tol[q], K_SPREAD[q] * float(table[:, _SENS_COL[q]].max()))
    return tol


def check_parts(g, phase, losses, tol):
    """Every loss part of the fixture, the SSIM part included."""
    keys = [k[len(phase + '_part_'):] for k in g.files if k.startswith(phase + '_part_')]
    assert 'SSIM' in keys
    for k in keys:
        want = float(g[phase + '_part_' + k])
        assert abs(float(losses[k]) - want) <= 5 * tol['loss'] * abs(want), (phase, k, float(losses[k]), want)


def check_common(g, phase, losses, preds, metrics, tol):
    want_loss = float(g[phase + '_loss'])
    assert abs(losses['loss'].item() - want_loss) <= tol['loss'] * abs(want_loss), (losses['loss'].item(), want_loss)
    check_parts(g, phase, losses, tol)
    got = torch.stack([p.squeeze(0) for p in preds]).cpu().numpy()
    assert np.abs(got - g[phase + '_preds']).mean() < tol['l1']
    assert abs(metrics['psnr'].avg - float(g[phase + '_psnr'])) < tol['psnr']
    assert abs(float(metrics['ssim'].avg) - float(g[phase + '_ssim'])) < tol['ssim']


def check_outer(g, rec_outer, tol, name):
    rows = dict(zip(list(g['outer_grad_fp_0_keys']), g['outer_grad_fp_0']))
    for k, row in rows.items():
        if abs(row[1]) > 0:       # tensors the plugin never routes have exactly-zero lr gradients in the reference
            assert k in rec_outer, k
            assert_fp_close(rec_outer[k], row, tol['outer'], (name, 'outer', k))


def run_case(name, phase, fuse=1, check_rule=False, **modes):
    g = golden("system_" + name)
    model = str(g['model'])
    system = build_system(model, dict(parse_case_args(g), task_batch=0, **modes), fuse=fuse)
    rec = observe(system, check_rule=check_rule)
    frames = synthetic.septuplet_batch(int(g['B']), int(g['H']), int(g['W']), model=model)
    if phase == 'train':
        losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
    else:
        losses, preds, metrics = system.run_validation_iter(data_batch=frames)
    torch.cuda.synchronize()
    return g, losses, preds, metrics, rec


def test_the_fixtures_cover_both_reachable_range_classes():
    assert golden('system_cain_l1_ssim_1step')['ssim_class_counts'].tolist() == [6, 0, 0, 0]
    assert golden('system_sepconv_l1_ssim_2step')['ssim_class_counts'].tolist() == [12, 8, 0, 0]
    assert golden('system_voxelflow_mse_ssim_2step')['ssim_class_counts'].tolist() == [0, 20, 0, 0]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("phase", ["train", "val"])
def test_iteration_matches_reference_fixture(name, phase):
    tol = tolerances(name, phase)
    g, losses, preds, metrics, rec = run_case(name, phase, check_rule=True)
    assert max(rec['rule_err']) <= 1e-6, rec['rule_err']
    assert list(g[phase + '_n_live']) == rec['n_live']
    for k, row in zip(list(g['%s_grad_fp_0_keys' % phase]), g['%s_grad_fp_0' % phase]):
        assert_fp_close(rec['grad_fp'][0][k], row, 1e-3, (name, 'g0', k))
    check_common(g, phase, losses, preds, metrics, tol)
    for i, d in enumerate(rec['weight_fp']):
        keys = list(g['%s_weight_fp_%d_keys' % (phase, i)])
        assert sorted(d) == keys
        for k, row in zip(keys, g['%s_weight_fp_%d' % (phase, i)]):
            assert_fp_close(d[k], row, tol['w'], (name, 'w', i, k), extra_abs=knee_allowance(g, phase, i, k, tol['g']))
    for i, d in enumerate(rec['grad_fp']):
        for k, row in zip(list(g['%s_grad_fp_%d_keys' % (phase, i)]), g['%s_grad_fp_%d' % (phase, i)]):
            assert_fp_close(d[k], row, tol['g'], (name, 'g', i, k))
    if phase == 'train':
        rows = dict(zip(list(g['outer_grad_fp_0_keys']), g['outer_grad_fp_0']))
        assert set(rec['outer_grad_fp']) == set(rows)
        for k, row in rows.items():
            assert_fp_close(rec['outer_grad_fp'][k], row, tol['outer'], (name, 'outer', k))


@pytest.mark.parametrize("name", CASES)
def test_fused_support_pair_equals_two_single_passes(name):
    _, l1, p1, _, r1 = run_case(name, 'train', fuse=1)
    _, l0, p0, _, r0 = run_case(name, 'train', fuse=0)
    assert abs(l1['loss'].item() - l0['loss'].item()) <= (2e-4 if 'voxelflow' in name else 2e-5) * abs(l0['loss'].item())
    assert abs(float(l1['SSIM']) - float(l0['SSIM'])) <= (2e-4 if 'voxelflow' in name else 2e-5) * abs(float(l0['SSIM']))
    for a, b in zip(p1, p0):
        assert (a - b).abs().mean().item() < (1e-4 if 'voxelflow' in name else 1e-5)
    for k in r0['outer_grad_fp']:
        assert_fp_close(r1['outer_grad_fp'][k], r0['outer_grad_fp'][k], 3e-2 if 'voxelflow' in name else 1e-3, k)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("phase", ["train", "val"])
def test_graphed_inner_loop_matches_reference_fixture(name, phase):
    tol = tolerances(name, phase)
    g = golden("system_" + name)
    model = str(g['model'])
    system = build_system(model, dict(parse_case_args(g), graph_inner_loop=1, task_batch=0, task_streams=1))
    rec = {}
    system.optimizer.step = lambda *a, **k: rec.update(
        {n: fp(p.grad) for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    frames = synthetic.septuplet_batch(int(g['B']), int(g['H']), int(g['W']), model=model)
    for rep in range(2):      # the second call replays the already captured graphs
        if phase == 'train':
            losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
        else:
            losses, preds, metrics = system.run_validation_iter(data_batch=frames)
        torch.cuda.synchronize()
        assert len(system._graphs) == 1
        check_common(g, phase, losses, preds, metrics, tol)
        if phase == 'train':
            rows = dict(zip(list(g['outer_grad_fp_0_keys']), g['outer_grad_fp_0']))
            for k, row in rows.items():
                if k in rec:
                    assert_fp_close(rec[k], row, tol['outer'], (name, 'outer', k))
                else:
                    assert abs(row[1]) == 0.0, (name, 'missing outer grad', k)


def _lockstep(name, phase, lockstep_for, graphed):
    g = golden("system_" + name)
    model = str(g['model'])
    assert int(g['B']) == 2
    over = dict(parse_case_args(g), task_batch=2)
    if graphed:
        over['graph_inner_loop'] = 1
    system = build_system(model, over)
    lockstep_for(system, model)
    calls = []
    orig = system._lockstep_body
    system._lockstep_body = lambda *a, **k: (calls.append(len(a[1])), orig(*a, **k))[1]
    rec_outer = {}
    system.optimizer.step = lambda *a, **k: rec_outer.update(
        {n: fp(p.grad) for n, p in system.named_parameters() if p.requires_grad and p.grad is not None})
    frames = synthetic.septuplet_batch(2, int(g['H']), int(g['W']), model=model)
    tol = tolerances(name, phase)
    for rep in range(2 if graphed else 1):
        if phase == 'train':
            losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
        else:
            losses, preds, metrics = system.run_validation_iter(data_batch=frames)
        torch.cuda.synchronize()
        if graphed:
            assert len(system._graphs) == 1 and next(iter(system._graphs.values())).T == 2
        else:
            assert calls == [2]
        check_common(g, phase, losses, preds, metrics, tol)
        if phase == 'train':
            check_outer(g, rec_outer, tol, name)


@pytest.mark.parametrize("name", TWO_TASK)
@pytest.mark.parametrize("phase", ["train", "val"])
def test_lockstep_tasks_match_reference_fixture(name, phase, lockstep_for):
    _lockstep(name, phase, lockstep_for, graphed=False)


@pytest.mark.parametrize("name", TWO_TASK)
@pytest.mark.parametrize("phase", ["train", "val"])
def test_graphed_lockstep_tasks_match_reference_fixture(name, phase, lockstep_for):
    _lockstep(name, phase, lockstep_for, graphed=True)


def test_training_steps_with_the_combined_objective():
    """What `main.py --model sepconv --loss 1*L1+0.1*SSIM --synthetic` does per iteration, from seeded weights (the entry point itself
    loads pretrained_models/sepconv_base_l1.pth): three train iterations with the outer optimizer stepping, default execution modes."""
    system = build_system('sepconv', dict(optimizer='SGD', inner_lr=1e-5, loss='1*L1+0.1*SSIM', batch_size=2,
                                          number_of_training_steps_per_iter=2, number_of_evaluation_steps_per_iter=2,
                                          graph_inner_loop=-1, task_streams=-1))
    before = {n: p.detach().clone() for n, p in system.named_parameters() if p.requires_grad}
    frames = synthetic.septuplet_batch(2, 64, 64, model='sepconv')
    seen = []
    for it in range(3):
        losses, _, _ = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=False)
        torch.cuda.synchronize()
        seen.append((losses['loss'].item(), float(losses['L1']), float(losses['SSIM'])))
    assert all(np.isfinite(v) for row in seen for v in row) and all(row[2] > 0 for row in seen), seen
    assert abs(seen[0][0] - (seen[0][1] + seen[0][2])) <= 1e-5 * seen[0][0]
    moved = sum(float((p.detach() - before[n]).abs().sum()) for n, p in system.named_parameters() if p.requires_grad)
    assert moved > 0 and all(torch.isfinite(p).all() for p in system.parameters())
