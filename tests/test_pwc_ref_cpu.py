"""The restatement of tests/pwc_ref.py against independent compositions of torch ops, on the host: the index-form correlation and its two
gradients against a shift / multiply / mean composition and its autograd, the warp against grid_sample(align_corners=True) times the
thresholded grid_sample of ones, the NaN semantics the kernels are held to, and the condition under which the network fixture of
tests/test_pwcnet_gpu.py is a fair one (no warp decision within reach of fp32 rounding, both decisions present at every level)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pwc_ref as R

SHAPES = [(1, 1, 1, 1), (1, 3, 3, 5), (2, 5, 9, 9), (1, 7, 12, 17)]


def _maps(shape, seed):
    rng = np.random.default_rng(seed)
    N, C, H, W = shape
    return rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal((N, 81, H, W))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_index_form_equals_the_composition(shape):
    f1, f2, gout = _maps(shape, 11)
    t1, t2 = torch.from_numpy(f1).requires_grad_(), torch.from_numpy(f2).requires_grad_()
    comp = R.correlation_composed(t1, t2)
    out = R.correlation_forward(f1, f2)
    assert out.shape == comp.shape and np.abs(out - comp.detach().numpy()).max() <= 1e-12
    g1, g2 = torch.autograd.grad(comp, (t1, t2), torch.from_numpy(gout), retain_graph=True)
    assert np.abs(R.correlation_backward_input1(f2, gout) - g1.numpy()).max() <= 1e-12
    assert np.abs(R.correlation_backward_input2(f1, gout) - g2.numpy()).max() <= 1e-12
    # with the LeakyReLU fused: autograd of leaky_relu(composition)
    act = F.leaky_relu(comp, float(np.float32(0.1)))
    outa = R.correlation_forward(f1, f2, slope=0.1)
    assert np.abs(outa - act.detach().numpy()).max() <= 1e-12
    g1, g2 = torch.autograd.grad(act, (t1, t2), torch.from_numpy(gout))
    assert np.abs(R.correlation_backward_input1(f2, gout, out=outa, slope=0.1) - g1.numpy()).max() <= 1e-12
    assert np.abs(R.correlation_backward_input2(f1, gout, out=outa, slope=0.1) - g2.numpy()).max() <= 1e-12


def test_fp32_mode_is_close_and_exact_on_integers():
    f1, f2, gout = _maps((2, 5, 9, 9), 12)
    o64 = R.correlation_forward(f1, f2)
    o32 = R.correlation_forward(f1.astype(np.float32), f2.astype(np.float32), dtype=np.float32)
    assert o32.dtype == np.float32 and 0 < np.abs(o32 - o64).max() < 1e-5
    rng = np.random.default_rng(3)
    i1, i2 = rng.integers(-4, 5, (1, 4, 6, 7)).astype(np.float64), rng.integers(-4, 5, (1, 4, 6, 7)).astype(np.float64)   # C = 4: exact division
    assert np.array_equal(R.correlation_forward(i1.astype(np.float32), i2.astype(np.float32), dtype=np.float32), R.correlation_forward(i1, i2))


@pytest.mark.parametrize("shape,scale", [((1, 1, 1, 1), 1.0), ((2, 3, 7, 9), 1.0), ((2, 3, 7, 9), 0.625), ((1, 4, 12, 1), 2.5)])
def test_warp_equals_grid_sample_with_align_corners(shape, scale):
    N, C, H, W = shape
    rng = np.random.default_rng(21)
    img = rng.standard_normal(shape)
    flow = rng.uniform(-1.0, 1.0, (N, 2, H, W)) * np.array([W / 2.0 + 1.0, H / 2.0 + 1.0])[None, :, None, None]
    ours, mask = R.pwc_warp(img, flow, scale, np.float64, np.float64, return_mask=True)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    vx, vy = xs[None] + flow[:, 0] * scale, ys[None] + flow[:, 1] * scale
    grid = torch.from_numpy(np.stack([2.0 * vx / max(W - 1, 1) - 1.0, 2.0 * vy / max(H - 1, 1) - 1.0], -1))
    t = torch.from_numpy(img)
    sampled = F.grid_sample(t, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    ones = F.grid_sample(torch.ones_like(t), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    m = ones[:, 0].numpy()
    # flows kept 1e-3 px clear of the threshold: the mask falls by at most 1 per px outside the frame, and is 1 everywhere inside it
    clear = (np.abs(m - 0.9999) > 1e-3) | (m > 1 - 1e-9)
    assert clear.mean() > 0.9
    assert np.abs(mask - ones[:, 0].numpy()).max() <= 1e-12
    expect = (sampled * (ones >= 0.9999).to(t.dtype)).numpy()
    assert np.abs(ours - expect)[np.broadcast_to(clear[:, None], ours.shape)].max() <= 1e-12
    assert (mask >= 0.9999).any() or min(H, W) == 1


def test_warp_decisions_are_taken_in_float32():
    """An exact hit on W - 1 keeps its pixel (mask == 1); a position 3e-4 px outside drops it; NaN / inf flows sample nothing."""
    img = np.arange(1, 1 + 5 * 8, dtype=np.float64).reshape(1, 1, 5, 8)
    flow = np.zeros((1, 2, 5, 8), np.float32)
    flow[0, 0, 0, :] = 7 - np.arange(8)                   # row 0: every pixel samples x = 7 exactly
    flow[0, 0, 1, :] = np.float32(7.0003) - np.arange(8)  # row 1: 3e-4 px beyond the last column
    flow[0, 0, 2, 3], flow[0, 1, 2, 4], flow[0, 0, 2, 5] = np.nan, np.inf, -np.inf
    out, mask = R.pwc_warp(img, flow, 1.0, return_mask=True)
    assert mask.dtype == np.float32
    assert np.array_equal(out[0, 0, 0], np.full(8, 8.0)) and np.array_equal(out[0, 0, 1], np.zeros(8))
    assert np.array_equal(out[0, 0, 2, 3:6], np.zeros(3)) and np.array_equal(mask[0, 2, 3:6], np.zeros(3, np.float32))
    assert np.abs(out[0, 0, 3:] - img[0, 0, 3:]).max() < 1e-5 and (mask[0, 3:] >= np.float32(0.9999)).all()     # zero flow: the fp32 chain's rounding only


def test_nan_semantics():
    f1, f2, gout = _maps((1, 3, 7, 8), 31)
    nd = 9
    a = f1.copy()
    a[0, 1, 2, 3] = np.nan                                                                  # f1: all 81 outputs of that pixel, nothing else
    nan = np.isnan(R.correlation_forward(a, f2))
    expect = np.zeros_like(nan)
    expect[0, :, 2, 3] = True
    assert np.array_equal(nan, expect)
    a[0, 1, 2, 3] = np.inf                                                                  # inf: +-inf inside the frame, inf * 0 = NaN outside
    o = R.correlation_forward(a, f2)[0, :, 2, 3].reshape(9, 9)
    assert not np.isfinite(o).any()
    assert np.isnan(o[:2]).all() and np.isnan(o[:, :1]).all() and np.isinf(o[2:, 1:]).all()  # rows y-4, y-3 and column x-4 leave the frame
    b = f2.copy()
    b[0, 2, 4, 1] = np.nan                                                                  # f2: exactly where it is read
    nan = np.isnan(R.correlation_forward(f1, b))
    expect = np.zeros_like(nan)
    for tj in range(-4, 5):
        for ti in range(-4, 5):
            y, x = 4 - tj, 1 - ti
            if 0 <= y < 7 and 0 <= x < 8:
                expect[0, (tj + 4) * nd + ti + 4, y, x] = True
    assert np.array_equal(nan, expect)
    g = gout.copy()
    tj, ti = 3, -2
    g[0, (tj + 4) * nd + ti + 4, 5, 6] = np.nan                                             # gout: g1 at its pixel, every channel ...
    nan1 = np.isnan(R.correlation_backward_input1(f2, g))
    expect = np.zeros_like(nan1)
    expect[0, :, 5, 6] = True
    assert np.array_equal(nan1, expect)
    assert not np.isnan(R.correlation_backward_input2(f1, g)).any()                         # ... its g2 target (8, 4) is outside the frame
    g = gout.copy()
    tj, ti = -3, 1
    g[0, (tj + 4) * nd + ti + 4, 5, 6] = np.nan                                             # target (2, 7): inside
    nan2 = np.isnan(R.correlation_backward_input2(f1, g))
    expect = np.zeros_like(nan2)
    expect[0, :, 2, 7] = True
    assert np.array_equal(nan2, expect)


def test_expected_state_dict_has_128_tensors():
    shapes = R.expected_state_dict_shapes()
    assert len(shapes) == 128 and sum(k.endswith('.0.weight') for k in shapes) == 49
    assert shapes['conv6_0.0.weight'] == (128, 81, 3, 3) and shapes['predict_flow6.weight'] == (2, 529, 3, 3)
    assert shapes['conv2_0.0.weight'] == (128, 117, 3, 3) and shapes['dc_conv1.0.weight'] == (128, 565, 3, 3)
    assert shapes['upfeat3.weight'] == (597, 2, 4, 4) and shapes['deconv2.weight'] == (2, 2, 4, 4) and 'upfeat2.weight' not in shapes


@functools.lru_cache(maxsize=None)
def _fixture_masks(name):
    sd, inputs = R.network_fixture()
    masks = {}
    flows = R.pwcdcnet_forward(sd, inputs[name], torch.float64, masks=masks)
    return flows, masks


@pytest.mark.parametrize("name", sorted(R.NET_INPUTS))
def test_network_fixture_condition(name):
    """A condition on the fixture, not a measurement: in the float64 run no warp mask lies within 5e-5 of 0.9999 (no fp32 implementation
    can then flip a decision), and at every level both decisions occur.  The fixture is pwc_ref.NET_SEED / FLOW_GAIN: chosen so that this
    holds (the choice is recorded there)."""
    flows, masks = _fixture_masks(name)
    assert sorted(masks) == [2, 3, 4, 5]
    for lv, mask in masks.items():
        assert np.isfinite(mask).all()
        print('PWCNET_FIXTURE %s level %d: kept %.3f of %d pixels, nearest mask to the threshold %.3e'
              % (name, lv, (mask >= 0.9999).mean(), mask.size, np.abs(mask - 0.9999).min()))
        assert np.abs(mask - 0.9999).min() > 5e-5, (name, lv)
        assert (mask >= 0.9999).any() and (mask < 0.9999).any(), (name, lv)
    for f in flows:
        assert torch.isfinite(f).all()
