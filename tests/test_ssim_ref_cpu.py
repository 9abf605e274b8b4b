"""CPU: the float64 restatement of the SSIM loss term (tests/ssim_ref.py) against the reference's own fp32 values
(tests/golden/ssim_loss.npz, written by tools/gen_golden_ssim.py from the imported reference) and against autograd, and the
host surface of the new term (Loss table, CPU refusal)."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops
from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.loss import Loss
from tests import ssim_ref as R
from tests.helpers import golden

GOLD = golden("ssim_loss")
SMALL = [n for n in GOLD['names'].tolist() if int(n.split('_')[3].split('x')[0]) <= 64]


def _parse(name):
    kind, cls, n, size, seed = name.split('_')
    H, W = size.split('x')
    return kind, int(cls[1:]), int(n[1:]), int(H), int(W), int(seed[1:])


@pytest.mark.parametrize("name", SMALL)
def test_restatement_matches_the_reference_fp32_values(name):
    """The restatement is the reference's formula: its float64 value is the one the generator saw (the seeded inputs reproduce),
    and it is as close to the reference's fp32 run as that run's stored own error says."""
    kind, cls, N, H, W, seed = _parse(name)
    sr, hr = R.make_pair(kind, cls, N, 3, H, W, seed)
    loss64 = float(R.ssim_loss(sr.double(), hr.double()))
    assert abs(loss64 - float(GOLD[name + '/loss64'])) <= 1e-12
    e_loss, e_grad = GOLD[name + '/e_ref']
    assert abs(loss64 - float(GOLD[name + '/loss'])) <= e_loss + 1e-12
    # fp32 rounding (6e-8) of an O(1) loss through the cancellation in E[x^2] - mu^2: a few 1e-6 at worst (smallest maps)
    assert e_loss <= 1e-5 and e_grad <= 1e-3
    grad64 = R.ssim_loss_grad(sr.double(), hr.double())
    if name + '/grad' in GOLD.files:
        ref = torch.from_numpy(GOLD[name + '/grad']).double()
        assert float((ref - grad64).abs().max() / grad64.abs().max()) <= e_grad * (1 + 1e-9) + 1e-12
    fp = GOLD[name + '/grad_fp']
    assert abs(float(grad64.abs().sum()) - fp[1]) <= 4 * e_grad * float(grad64.abs().max()) * grad64.numel()


def test_per_row_and_batch_rules_differ_as_in_the_reference():
    for seed in GOLD['seeds'].tolist():
        sr, hr = R.make_pair('near', [0, 1, 2, 3], 4, 3, 24, 40, seed)
        rows, classes = R.ssim_loss_rows(sr.double(), hr.double())
        assert classes == [0, 1, 2, 3]
        assert np.abs(rows.numpy() - GOLD['mixed_s%d/loss_rows' % seed]).max() <= 1e-5
        assert R.range_class(sr) == 3
        assert abs(float(R.ssim_loss(sr.double(), hr.double())) - float(GOLD['mixed_s%d/loss' % seed])) <= 1e-5


@pytest.mark.parametrize("cls", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", R.KINDS)
def test_analytic_gradient_passes_gradcheck(kind, cls):
    sr, hr = R.make_pair(kind, cls, 2, 2, 12, 14, 3)
    sr, hr = sr.double(), hr.double()
    L = R.CLASS_L[cls]

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return R.ssim_loss(x, hr, L)

        @staticmethod
        def backward(ctx, g):
            x, = ctx.saved_tensors
            return g * R.ssim_loss_grad(x, hr, 1.0, L)
    # the analytic backward against finite differences of the forward, and against autograd of the forward
    assert torch.autograd.gradcheck(Fn.apply, (sr.clone().requires_grad_(),), eps=1e-6 * L, atol=1e-9, rtol=1e-5)
    x = sr.clone().requires_grad_()
    auto, = torch.autograd.grad(R.ssim_loss(x, hr, L), x)
    ana = R.ssim_loss_grad(sr, hr, 1.0, L)
    assert float((auto - ana).abs().max()) <= 1e-12 * float(auto.abs().max()) + 1e-18


def test_identical_pair_is_zero_in_float64():
    sr, hr = R.make_pair('same', 0, 1, 3, 37, 53, 0)
    assert abs(float(R.ssim_loss(sr.double(), hr.double()))) <= 1e-15
    assert float(R.ssim_loss_grad(sr.double(), hr.double()).abs().max()) <= 1e-12


def test_loss_table_takes_ssim():
    crit = Loss(default_args(loss='1*L1+0.1*SSIM'))
    assert crit.loss_keys() == ['L1', 'SSIM', 'total']
    assert [l['weight'] for l in crit.loss] == [1.0, 0.1]
    crit = Loss(default_args(loss='1*MSE+0.1*SSIM'))
    assert crit.loss_keys() == ['MSE', 'SSIM', 'total']
    with pytest.raises(NotImplementedError):
        Loss(default_args(loss='1*VGG22'))
    with pytest.raises(NotImplementedError):
        Loss(default_args(loss='1*L1+0.1*Super'))


def test_ssim_loss_refuses_cpu_tensors_and_small_frames():
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        hip_ops.ssim_loss(a, b)
    with pytest.raises(NotImplementedError):
        hip_ops.ssim_loss_per_sample(a, b)
    with pytest.raises(ValueError):
        hip_ops.ssim_loss(torch.rand(1, 3, 10, 16), torch.rand(1, 3, 10, 16))
