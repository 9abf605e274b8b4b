"""The float64 restatement of the census loss term (tests/census_ref.py), the golden fixture built from it, and the term's place in
``Loss`` -- everything that needs no GPU."""
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd.config import default_args
from meta_interpolation_amd.loss import Loss
from tests import census_ref as Z
from tests import ssim_ref as R
from tests.helpers import golden

GOLD = golden("census")


def constant_offset_pair(H=16, W=21, offset=0.25):
    """C = 1, the target on the 1 / 256 grid and the prediction `offset` above it: every difference of two gray values is exact in fp32
    and in float64, and it is the same in both images wherever both pixels lie inside the frame."""
    hr = (torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(1)) * 256).floor() / 256
    return hr + offset, hr


def test_closed_form_at_3x3():
    """hr = 0, sr = 0.9 at the centre: only the centre is unmasked, its 48 non-centre offsets have d = -0.9 against 0, t = -0.9 /
    sqrt(1.62) = -1 / sqrt(2), delta = 0.5, h = 5 / 6: the value is (48 / 49) (5 / 6) / 9 = 40 / 441."""
    sr = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    sr[0, 0, 1, 1] = 0.9
    hr = torch.zeros_like(sr)
    assert abs(float(Z.census(sr, hr)) - 40 / 441) <= 1e-15
    assert abs(float(Z.census_rows(sr, hr)[0]) - 40 / 441) <= 1e-15
    m = Z.census_map(sr, hr)
    assert float(m[0, 1, 1]) > 0 and float(m.sum()) == float(m[0, 1, 1])


def test_identical_pair_is_exactly_zero():
    sr, _ = R.make_pair('smooth', 0, 2, 3, 16, 21, 0)
    assert Z.census_rows(sr.double(), sr.double().clone()).tolist() == [0.0, 0.0]
    assert float(Z.census_grad_rows(sr, sr.clone(), [1.0, 2.0]).abs().max()) == 0.0


def test_float64_gradient_agrees_with_central_differences():
    for C in (3, 1):
        sr, hr = R.make_pair('noise', 0, 1, C, 7, 9, 0)
        sr, hr = sr.double(), hr.double()
        g = Z.census_grad_rows(sr, hr, [1.0])
        h = 1e-6
        flat = sr.reshape(-1)
        worst = 0.0
        for idx in range(flat.numel()):          # every element: corners, borders, interior
            e = torch.zeros_like(flat)
            e[idx] = h
            fd = (Z.census_rows(sr + e.view_as(sr), hr) - Z.census_rows(sr - e.view_as(sr), hr)) / (2 * h)
            worst = max(worst, abs(float(fd) - float(g.reshape(-1)[idx])))
        assert worst <= 1e-8 * float(g.abs().max()) + 1e-9, worst
        v, gv = Z.census_and_grad(sr, hr)
        assert abs(float(v) - float(Z.census_rows(sr, hr).mean())) <= 1e-15 and torch.allclose(gv, g, rtol=0, atol=1e-15)
    # the one-value form over a batch is the mean of the rows, and its gradient theirs over N
    sr, hr = R.make_pair('noise', 0, 3, 3, 7, 9, 1)
    v, gv = Z.census_and_grad(sr, hr)
    assert abs(float(v) - float(Z.census_rows(sr.double(), hr.double()).mean())) <= 1e-15
    assert torch.allclose(gv, Z.census_grad_rows(sr, hr, [1 / 3] * 3), rtol=0, atol=1e-15)


def test_padding_is_by_zeros_not_by_reflection():
    """A pair differing by a constant at 16 x 21.  Where a pixel and its whole window lie inside the frame every d_o is the same in
    both images: such pixels contribute exactly 0.  An offset that leaves the frame reads 0 in both images: d_o = -g(p), which differs
    by the constant.  The value is the sum over the border band alone, restated here pixel by pixel from the count of offsets that
    leave the frame.  Reflection padding would give 0 everywhere."""
    H, W = 16, 21
    sr, hr = constant_offset_pair(H, W)
    sr, hr = sr.double(), hr.double()
    m = Z.census_map(sr, hr)[0]
    assert float(m[3:-3, 3:-3].abs().max()) == 0.0
    band = m.clone()
    band[3:-3, 3:-3] = 0
    value = float(Z.census(sr, hr))
    assert value > 1e-3 and abs(value - float(band.sum()) / (H * W)) <= 1e-15

    def t(d):
        return d / torch.sqrt(0.81 + d * d)
    inside_y = torch.tensor([min(y, 3) + min(H - 1 - y, 3) + 1 for y in range(H)], dtype=torch.float64)
    inside_x = torch.tensor([min(x, 3) + min(W - 1 - x, 3) + 1 for x in range(W)], dtype=torch.float64)
    leaving = 49 - inside_y[:, None] * inside_x[None, :]
    delta = (t(-sr[0, 0]) - t(-hr[0, 0])) ** 2
    want = (leaving * delta / (0.1 + delta))[1:-1, 1:-1].sum() / (49 * H * W)
    assert abs(value - float(want)) <= 1e-15

    def ternary_reflected(x):
        g = Z.gray(x)
        p = F.pad(g[:, None], (3, 3, 3, 3), mode='reflect')[:, 0]
        d = torch.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(7) for dx in range(7)], 1) - g[:, None]
        return d / torch.sqrt(0.81 + d * d)
    assert float((ternary_reflected(sr) - ternary_reflected(hr)).abs().max()) == 0.0


def test_golden_values_are_reproduced():
    names = GOLD['names'].tolist()
    assert len(names) == len(Z.SIZES) * len(Z.KINDS) == 18
    seen = set()
    for H, W in Z.SIZES:
        for kind in Z.KINDS:
            name = '%s_%dx%d' % (kind, H, W)
            seed = int(GOLD[name + '/seed'])
            sr, hr = R.make_pair(kind, 0, 1, 3, H, W, seed)
            v64, g64 = Z.census_and_grad(sr, hr)
            assert abs(float(v64) - float(GOLD[name + '/value64'])) <= 1e-12
            assert abs(R.fingerprint(g64) - GOLD[name + '/grad64_fp']).max() <= 1e-12
            assert abs(float(GOLD[name + '/value']) - float(v64)) == pytest.approx(float(GOLD[name + '/e_ref'][0]), abs=1e-12)
            assert float(GOLD[name + '/e_ref'][0]) <= float(GOLD['E_' + kind][0]) and float(GOLD[name + '/e_ref'][1]) <= float(GOLD['E_' + kind][1])
            seen.add(name)
    assert seen == set(names)
    for kind in Z.KINDS:          # the fp32 composition's value error is below the floor; its gradient error is not (cancellation in t(sr) - t(hr))
        assert 3 * float(GOLD['E_' + kind][0]) < Z.VALUE_FLOOR and float(GOLD['E_' + kind][1]) > 0


def test_bad_channels_and_sizes_raise():
    for shape in ((1, 2, 8, 8), (1, 4, 8, 8), (1, 3, 2, 8), (1, 3, 8, 2)):
        with pytest.raises(ValueError):
            Z.census_rows(torch.zeros(shape), torch.zeros(shape))
    assert Z.census_rows(torch.zeros(1, 3, 3, 3), torch.zeros(1, 3, 3, 3)).tolist() == [0.0]


def test_loss_wrapper_knows_the_term():
    crit = Loss(default_args(loss='1*L1+1*Census'))
    assert crit.loss_keys() == ['L1', 'Census', 'total']
    assert [(l['type'], l['weight']) for l in crit.loss] == [('L1', 1.0), ('Census', 1.0)]
    for other in ('1*VGG22', '1*Super'):
        with pytest.raises(NotImplementedError):
            Loss(default_args(loss=other))


def test_host_tensors_and_bad_shapes_raise_before_any_launch():
    from meta_interpolation_amd import hip_ops
    a = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        hip_ops.census_loss(a, a)
    for shape in ((1, 2, 8, 8), (1, 3, 2, 8), (1, 3, 8, 2), (3, 8, 8)):
        with pytest.raises(ValueError):
            hip_ops.census_loss(torch.zeros(shape), torch.zeros(shape))
        with pytest.raises(ValueError):
            hip_ops.census_loss_per_sample(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError):
        hip_ops.census_loss(a, torch.zeros(1, 3, 8, 9))
