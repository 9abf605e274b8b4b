"""The float64 restatement of the Laplacian-pyramid loss term (tests/laploss_ref.py), the golden fixture built from it, and the
term's place in ``Loss`` -- everything that needs no GPU."""
import pytest
import torch

from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.loss import Loss
from tests import laploss_ref as L
from tests import ssim_ref as R
from tests.helpers import golden

GOLD = golden("laploss")


def test_identical_pair_is_exactly_zero():
    sr, _ = R.make_pair('smooth', 0, 2, 3, 19, 34, 0)
    assert L.lap_rows(sr.double(), sr.double().clone()).tolist() == [0.0, 0.0]
    assert float(L.lap(sr, sr.clone())) == 0.0
    assert float(L.lap_grad_rows(sr, sr.clone(), [1.0, 2.0]).abs().max()) == 0.0          # sign(0) = 0


def test_two_levels_on_the_smallest_planes():
    g = torch.Generator().manual_seed(0)
    sr, hr = torch.rand(2, 3, 3, 5, generator=g, dtype=torch.float64), torch.rand(2, 3, 3, 5, generator=g, dtype=torch.float64)
    rows = L.lap_rows(sr, hr, levels=2)
    assert rows.shape == (2,) and torch.isfinite(rows).all() and (rows > 0).all()
    assert [tuple(b.shape[2:]) for b in L.bands(sr - hr, 2)] == [(3, 5), (2, 3)]
    with pytest.raises(ValueError):
        L.lap_rows(sr, hr, levels=3)          # level 1 is 2 x 3: nothing to reflect
    with pytest.raises(ValueError):
        L.lap_rows(sr, hr, levels=6)
    with pytest.raises(ValueError):
        L.lap_rows(torch.zeros(1, 1, 16, 17), torch.zeros(1, 1, 16, 17))          # five levels need 17


def test_constant_difference_lives_in_the_residual_alone():
    """d = 0.25 at 19 x 33: the window sums to one and the up-sampling restores a constant at odd sizes too, so every Laplacian band
    is exactly 0; the residual (2 x 3 after 19 x 33 -> 10 x 17 -> 5 x 9 -> 3 x 5 -> 2 x 3) carries 16 * 0.25 * n_4 / n_0."""
    hr = (torch.rand(1, 3, 19, 33, generator=torch.Generator().manual_seed(1)) * 256).floor().double() / 256
    sr = hr + 0.25
    bs = L.bands(sr - hr)
    assert all(float(b.abs().max()) == 0.0 for b in bs[:-1])
    assert tuple(bs[-1].shape) == (1, 3, 2, 3) and bool((bs[-1] == 0.25).all())
    want = 16 * 0.25 * (2 * 3) / (19 * 33)
    assert abs(want - 0.0382775) < 1e-7
    assert abs(float(L.lap(sr, hr)) - want) <= 1e-15


def test_float64_gradient_agrees_with_central_differences():
    found = L.conditioned_pair('noise', 1, 2, 17, 19)
    assert found is not None
    _, sr, hr = found
    sr, hr = sr.double(), hr.double()
    assert L.min_band(sr, hr) >= L.MIN_BAND
    g = L.lap_grad_rows(sr, hr, [1.0])
    h = 1e-7          # far below min_band * max|d|: no band changes sign, the function is linear over the step
    flat = sr.reshape(-1)
    worst = 0.0
    for idx in list(range(0, flat.numel(), 37)) + [18, 19 * 16, flat.numel() - 1]:          # interior, corners, borders
        e = torch.zeros_like(flat)
        e[idx] = h
        fd = (L.lap_rows(sr + e.view_as(sr), hr) - L.lap_rows(sr - e.view_as(sr), hr)) / (2 * h)
        worst = max(worst, abs(float(fd) - float(g.reshape(-1)[idx])))
    assert worst <= 1e-8 * float(g.abs().max()) + 1e-9, worst
    # and the one-value form is the mean of the rows
    v, gv = L.lap_and_grad(sr, hr)
    assert abs(float(v) - float(L.lap_rows(sr, hr).mean())) <= 1e-15 and torch.allclose(gv, g, rtol=0, atol=1e-15)


def test_golden_values_and_seeds_are_reproduced():
    names = GOLD['names'].tolist()
    assert len(names) == 14
    seen = set()
    for H, W in L.SIZES:
        for kind in L.kinds_at(H, W):
            name = '%s_%dx%d' % (kind, H, W)
            seed = int(GOLD[name + '/seed'])
            for earlier in range(seed):          # the FIRST seed that qualifies
                assert L.min_band(*R.make_pair(kind, 0, 1, 3, H, W, earlier)) < L.MIN_BAND
            sr, hr = R.make_pair(kind, 0, 1, 3, H, W, seed)
            mb = L.min_band(sr, hr)
            assert mb >= L.MIN_BAND and abs(mb - float(GOLD[name + '/min_band'])) <= 1e-12
            v64, g64 = L.lap_and_grad(sr, hr)
            assert abs(float(v64) - float(GOLD[name + '/value64'])) <= 1e-12
            fpr = R.fingerprint(g64)
            assert abs(fpr - GOLD[name + '/grad64_fp']).max() <= 1e-12
            assert abs(float(GOLD[name + '/value']) - float(v64)) == pytest.approx(float(GOLD[name + '/e_ref'][0]), abs=1e-12)
            assert float(GOLD[name + '/e_ref'][0]) <= float(GOLD['E_' + kind][0]) and float(GOLD[name + '/e_ref'][1]) <= float(GOLD['E_' + kind][1])
            seen.add(name)
    assert seen == set(names)
    assert L.conditioned_pair('smooth', 1, 3, 40, 300) is None          # why 40 x 300 has two kinds
    # the fp32 composition's own error is below the floors: the floors decide the gates
    for kind in L.KINDS:
        assert 3 * float(GOLD['E_' + kind][0]) < L.VALUE_FLOOR and 3 * float(GOLD['E_' + kind][1]) < L.GRAD_FLOOR


def test_loss_wrapper_knows_the_term():
    crit = Loss(default_args(loss='1*L1+0.5*Lap'))
    assert crit.loss_keys() == ['L1', 'Lap', 'total']
    assert [(l['type'], l['weight']) for l in crit.loss] == [('L1', 1.0), ('Lap', 0.5)]
    for other in ('1*VGG22', '1*Super'):
        with pytest.raises(NotImplementedError):
            Loss(default_args(loss=other))


def test_host_tensors_and_bad_shapes_raise_before_any_launch():
    from meta_interpolation_amd import hip_ops
    a = torch.zeros(1, 3, 17, 17)
    with pytest.raises(NotImplementedError):
        hip_ops.lap_loss(a, a)
    with pytest.raises(ValueError):
        hip_ops.lap_loss(torch.zeros(1, 3, 16, 17), torch.zeros(1, 3, 16, 17))
    with pytest.raises(ValueError):
        hip_ops.lap_loss_per_sample(a, a, levels=6)
    with pytest.raises(ValueError):
        hip_ops.lap_loss(a, torch.zeros(1, 3, 17, 18))
