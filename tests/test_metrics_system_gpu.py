"""-m gpu: the fused PSNR / SSIM metric inside whole meta-iterations.  One small fixture configuration each of SepConv, CAIN and
VoxelFlow (the `args` of tests/golden/system_*_ssim_*.npz, two tasks of 64 x 64), a train iteration with do_evaluation=True in the
sequential, lockstep and graphed execution modes:

* evaluating changes nothing else: loss and predictions are bit-identical to the same iteration with do_evaluation=False;
* the PSNR / SSIM meters agree with ``utils.calc_metrics`` (the composition of library ops the kernel replaces) recomputed from the
  returned predictions and the frames, within the suite's contract: CONTRACT['psnr'] = 1e-3 dB, CONTRACT['ssim'] = 1e-4
  (tests/test_fullsize_gpu.py).  The measured differences are printed (METRIC_SYSTEM lines).

That the meters also agree with the REFERENCE's fixtures is what tests/test_system_gpu.py, test_ssim_system_gpu.py and
test_fullsize_gpu.py hold, unchanged, with the kernel in the path.
"""
import pytest
import torch

from meta_interpolation_amd import hip_ops, synthetic, utils
from tests.helpers import build_system, golden, parse_case_args
from tests.test_fullsize_gpu import CONTRACT
from tests.test_system_gpu import lockstep_for  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = {'sepconv': 'sepconv_l1_ssim_2step', 'cain': 'cain_l1_ssim_1step', 'voxelflow': 'voxelflow_mse_ssim_2step'}
MODES = {'sequential': dict(task_batch=0), 'lockstep': dict(task_batch=2), 'graphed': dict(task_batch=0, graph_inner_loop=1)}


def run(model, mode, lockstep_for, do_evaluation, calls=None):
    g = golden("system_" + CASES[model])
    system = build_system(model, dict(parse_case_args(g), batch_size=2, **MODES[mode]))
    if mode == 'lockstep':
        lockstep_for(system, model)
    system.optimizer.step = lambda *a, **k: None
    if calls is not None:
        orig = hip_ops.psnr_ssim
        hip_ops.psnr_ssim = lambda p, t, **k: (calls.append(p.shape[0]), orig(p, t, **k))[1]
    try:
        frames = synthetic.septuplet_batch(2, int(g['H']), int(g['W']), model=model)
        losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=do_evaluation)
        torch.cuda.synchronize()
    finally:
        if calls is not None:
            hip_ops.psnr_ssim = orig
    if mode == 'graphed':
        assert len(system._graphs) == 1
    return system, frames, losses, preds, metrics


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("model", list(CASES))
def test_evaluation_uses_the_fused_metric_and_changes_nothing_else(model, mode, lockstep_for):
    calls = []
    system, frames, losses, preds, metrics = run(model, mode, lockstep_for, True, calls)
    _, _, losses0, preds0, metrics0 = run(model, mode, lockstep_for, False)
    assert metrics0['psnr'].count == 0 and metrics['psnr'].count == 2 and metrics['ssim'].count == 2
    # one call for the rows it is given: the two tasks together in lockstep, one by one otherwise
    assert calls == ([2] if mode == 'lockstep' else [1, 1]), calls
    assert torch.equal(losses['loss'], losses0['loss'])
    for a, b in zip(preds, preds0):
        assert torch.equal(a, b)
    # the meters against the composition, from what the iteration returned
    psnr, ssim = 0.0, 0.0
    for t in range(2):
        tgt01 = system._to_unit_range(frames[system.target_idxs[1]][t].to(preds[t].device))
        p, s = utils.calc_metrics(preds[t].squeeze(0), tgt01)
        psnr, ssim = psnr + p / 2, ssim + float(s) / 2
    d_psnr, d_ssim = abs(metrics['psnr'].avg - psnr), abs(float(metrics['ssim'].avg) - ssim)
    print('METRIC_SYSTEM model=%s mode=%s psnr=%.5f d_psnr=%.3e (bound %.0e) ssim=%.7f d_ssim=%.3e (bound %.0e)'
          % (model, mode, psnr, d_psnr, CONTRACT['psnr'], ssim, d_ssim, CONTRACT['ssim']))
    assert d_psnr <= CONTRACT['psnr'] and d_ssim <= CONTRACT['ssim']
