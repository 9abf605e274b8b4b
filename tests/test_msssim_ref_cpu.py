"""CPU: the restatement of multi-scale SSIM (tests/msssim_ref.py) against the reference's own fp32 values (tests/golden/msssim.npz,
written by tools/gen_golden_msssim.py from the imported reference), and the host surface of the feature: the Loss table, the refusal
of host tensors, the evaluation flag."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops, pytorch_msssim
from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.loss import Loss
from tests import msssim_ref as M
from tests import ssim_ref as R
from tests.helpers import golden

GOLD = golden("msssim")
NAMES = GOLD['names'].tolist()
SEED0 = [n for n in NAMES if n.endswith('_s0')]
# the fp32 restatement runs the reference's own ATen ops in the reference's order: what may differ is the association inside a
# threaded convolution or mean, a few fp32 roundings of an O(1) value (2^-24 each) resp. of the gradient's largest element
VALUE_ULPS, GRAD_REL = 4 * 2.0 ** -24, 2.0 ** -20


def _pair(name):
    kind, cls, norm, N, H, W, seed = M.parse_case(name)
    return R.make_pair(kind, cls, N, 3, H, W, seed), norm


@pytest.mark.parametrize("name", NAMES)          # every stored case: seeds 1 and 2 set most of the E_kind the GPU gates are read from
def test_restatements_match_the_reference_fp32_values(name):
    (sr, hr), norm = _pair(name)
    want, want64 = float(GOLD[name + '/value']), float(GOLD[name + '/value64'])
    e_v, e_g = GOLD[name + '/e_ref']
    v32, g32 = M.msssim_and_grad(sr, hr, None, norm)
    v64, g64 = M.msssim_and_grad(sr.double(), hr.double(), None, norm)
    # NaN exactly where the reference is, in fp32 and float64 alike
    assert np.isnan(want) == bool(torch.isnan(v32)) == bool(torch.isnan(v64)) == np.isnan(want64) == np.isnan(e_v)
    if np.isnan(want):
        assert bool(torch.isnan(g64).all())          # autograd through a NaN power: every element
        return
    assert abs(float(v32) - want) <= VALUE_ULPS
    assert abs(v64.item() - want64) <= 1e-12          # the seeded inputs reproduce
    assert abs(abs(v64.item() - want) - e_v) <= 1e-12          # float64 differs from the reference by exactly the stored e_ref
    fp = GOLD[name + '/grad_fp']
    if np.isnan(e_g):          # a finite value with a NaN gradient: an unused level's negative mean under pow (see the generator)
        assert np.isnan(fp[0]) and bool(torch.isnan(g32).any())
        return
    assert np.abs(R.fingerprint(g32)[2:] - fp[2:]).max() <= GRAD_REL * fp[2]          # the largest and the first four elements
    # the gradient's e_ref of EVERY case, the whole gradient stored or not: the fp32 restatement is within GRAD_REL of the reference's
    # gradient (asserted above on what is stored of it), so its own distance from float64 is within GRAD_REL (1 + e_g) of the stored
    # figure.  That is the floor of the GPU gate: a stored e_ref that is off by more cannot pass, one off by less cannot move a gate.
    mine = float((g32.double() - g64).abs().max() / g64.abs().max())
    assert abs(mine - e_g) <= GRAD_REL * (1 + e_g)
    if name + '/grad' in GOLD.files:
        ref = torch.from_numpy(GOLD[name + '/grad'])
        assert float((ref - g32).abs().max()) <= GRAD_REL * float(ref.abs().max())
        assert abs(float((ref.double() - g64).abs().max() / g64.abs().max()) - e_g) <= 1e-9 * e_g + 1e-15
    assert e_v <= 2e-5 and e_g <= 2e-3          # fp32 rounding of O(1) means through five powers; cancellation in E[x^2] - mu^2


def test_E_kind_is_the_largest_finite_e_ref():
    for kind in M.KINDS:
        for norm in (1, 0):
            e = np.array([GOLD[n + '/e_ref'] for n in NAMES if n.startswith('%s_c' % kind) and '_z%d_' % norm in n])
            assert e.shape[0] == 6 * 4 * 3
            assert np.array_equal(np.nanmax(e, axis=0), GOLD['E_%s_z%d' % (kind, norm)])
    # the plain form is finite for every `near` case and every normalised case
    assert all(np.isfinite(GOLD[n + '/value']) for n in NAMES if n.startswith('near_') or '_z1_' in n)


def test_the_last_ssim_enters_four_times():
    """What is pinned is ssim_4 ** (4 w_4) * prod cs_s ** w_s; Wang et al.'s product (ssim_4 once) is told apart by far more than the
    reference's own error."""
    for name in [n for n in SEED0 if n.startswith(('near_c0_z', 'noise_c0_z1', 'smooth_c0_z1'))]:
        (sr, hr), norm = _pair(name)
        ms, mc, _ = M.levels(sr.double(), hr.double())
        want, e_v = float(GOLD[name + '/value']), float(GOLD[name + '/e_ref'][0])
        assert abs(float(M.combine(ms, mc, norm)) - want) <= e_v + 1e-12
        w4 = M.WEIGHTS[4]
        base = float(M.bases(ms, mc, norm)[4])
        assert abs(float(M.combine(ms, mc, norm)) - float(M.combine_textbook(ms, mc, norm)) * base ** (3 * w4)) <= 1e-6
        # a textbook kernel would miss the GPU tests' gate max(3 E_kind, 4 * 2^-24) on every one of these pairs
        kind = name.split('_')[0]
        assert abs(float(M.combine_textbook(ms, mc, norm)) - want) > max(3 * float(GOLD['E_%s_z%d' % (kind, norm)][0]), VALUE_ULPS) + e_v


def test_class_changes_between_levels_and_mixed_batch():
    for tag, value in (('spike200', 200.0), ('spikem06', -0.6)):
        sr, hr = R.make_pair('near', 0, 1, 3, 64, 64, 0)
        sr = sr.clone()
        sr[0, 1, 20, 30] = value
        for norm in (1, 0):
            name = '%s_z%d' % (tag, norm)
            assert M.levels(sr.double(), hr.double())[2] == GOLD[name + '/classes'].tolist()
            v64 = float(M.msssim(sr.double(), hr.double(), None, bool(norm)))
            assert abs(abs(v64 - float(GOLD[name + '/value'])) - float(GOLD[name + '/e_ref'][0])) <= 1e-12
    for seed in GOLD['seeds'].tolist():
        sr, hr = R.make_pair('near', [0, 2, 1], 3, 3, 64, 64, seed)
        for norm in (1, 0):
            rows = M.msssim_rows(sr.double(), hr.double(), None, bool(norm)).numpy()
            assert np.abs(rows - GOLD['mixed_z%d_s%d/rows' % (norm, seed)]).max() <= 2e-5
            assert abs(float(M.msssim(sr.double(), hr.double(), None, bool(norm))) - float(GOLD['mixed_z%d_s%d/value' % (norm, seed)])) <= 2e-5


def test_level_geometry():
    assert M.level_taps(32, 32) == [11, 11, 8, 4, 2]
    assert M.level_taps(37, 53) == [11, 11, 9, 4, 2]
    assert M.level_taps(161, 176) == [11, 11, 11, 11, 10]
    assert M.level_taps(176, 176) == [11] * 5
    with pytest.raises(ValueError):
        M.msssim(torch.rand(1, 3, 31, 64).double(), torch.rand(1, 3, 31, 64).double())


def test_loss_table_takes_msssim():
    crit = Loss(default_args(loss='1*L1+0.1*MSSSIM'))
    assert crit.loss_keys() == ['L1', 'MSSSIM', 'total']
    assert [l['weight'] for l in crit.loss] == [1.0, 0.1]
    with pytest.raises(NotImplementedError):
        Loss(default_args(loss='1*VGG22'))
    with pytest.raises(NotImplementedError):
        Loss(default_args(loss='1*L1+0.1*Super'))


def test_host_tensors_and_bad_arguments_are_refused():
    a, b = torch.rand(2, 3, 40, 40), torch.rand(2, 3, 40, 40)
    for fn in (hip_ops.msssim, hip_ops.msssim_per_sample, hip_ops.msssim_metric, pytorch_msssim.msssim, pytorch_msssim.MSSSIM()):
        with pytest.raises(NotImplementedError):
            fn(a, b)
    crit = Loss(default_args(loss='1*L1+0.1*MSSSIM'))
    with pytest.raises(NotImplementedError):
        crit(a, b)
    with pytest.raises(NotImplementedError):
        crit.per_sample(a, b)
    with pytest.raises(ValueError):
        hip_ops.msssim(torch.rand(1, 3, 31, 64), torch.rand(1, 3, 31, 64))
    with pytest.raises(ValueError):
        hip_ops.msssim(a, b, val_range=3)
    with pytest.raises(NotImplementedError):
        pytorch_msssim.msssim(a, b, window_size=7)
    with pytest.raises(NotImplementedError):
        pytorch_msssim.msssim(a, b, size_average=False)


def test_eval_flag_defaults_to_off():
    assert default_args().eval_msssim == 0
    assert default_args(eval_msssim=1).eval_msssim == 1


def test_eval_flag_on_host_tensors_adds_the_metric_and_the_default_changes_nothing():
    """The toy plugin on the CPU: the metric comes from the host composition of utils.msssim_rows; with the default the dicts are as before."""
    from meta_interpolation_amd import synthetic, utils
    from tests.helpers import build_toy_system
    frames = synthetic.septuplet_batch(2, 32, 40, model='cain')
    seen = {}
    for flag in (0, 1):
        system = build_toy_system(batch=2, steps=1)
        system.args.eval_msssim = flag
        losses, preds, metrics = system.run_train_iter(data_batch=frames, epoch=0, do_evaluation=True)
        seen[flag] = (float(losses['loss']), {k: float(v.avg) for k, v in metrics.items()}, preds)
        assert sorted(metrics) == (['msssim', 'psnr', 'ssim'] if flag else ['psnr', 'ssim'])
        assert metrics['psnr'].count == 2 and (not flag or metrics['msssim'].count == 2)
    assert seen[0][0] == seen[1][0] and all(seen[0][1][k] == seen[1][1][k] for k in ('psnr', 'ssim'))
    pred = torch.cat([p.detach() for p in seen[1][2]])
    want = M.metric_rows(pred, frames[3], dtype=torch.float64)
    got = utils.msssim_rows(pred, frames[3])
    assert float((got.double() - want).abs().max()) <= 2e-5          # the host composition is fp32: the reference's own error
    assert torch.isfinite(want).all() and abs(seen[1][1]['msssim'] - float(want.mean())) <= 2e-5
