"""Softmax splatting without a GPU: hip_ops.softsplat_composed in float64 held to the loop restatement (tests/softsplat_ref.py), values and
all three gradients, for every mode, shape and gated content kind; gradcheck; the premise of the GPU suite's gates (in the gated kinds
the reference's own D is at least 2^-8 wherever something landed); the invariance to a constant added to the metric; the op's routing and
argument checks; and the plugin on the CPU, float64 against float32."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops
from tests import softsplat_ref as R
from tests.helpers import build_plugin

ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def composed64(x, flow, metric, mode, gout):
    x, flow, metric = (t.double().clone().requires_grad_() for t in (x, flow, metric))
    out, hit = hip_ops.softsplat_composed(x, flow, metric if mode == 'soft' else None, mode, return_hit=True)
    assert not hit.requires_grad
    wanted = (x, flow, metric) if mode == 'soft' else (x, flow)
    grads = torch.autograd.grad(out, wanted, gout.double())
    return (out.detach(), hit) + tuple(grads)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("kind", R.GATED)
@pytest.mark.parametrize("mode", R.MODES)
def test_composed_op_in_float64_equals_the_restatement(mode, kind, shape):
    x, flow, metric, gout = R.inputs(kind, shape)
    ref = R.softsplat(x, flow, metric, mode, gout, coord=np.float64)
    got = composed64(x, flow, metric, mode, gout)
    names = ('out', 'hit', 'g_x', 'g_flow') + (('g_metric',) if mode == 'soft' else ())
    for name, t in zip(names, got):
        assert np.abs(t.numpy() - ref[name]).max() <= 1e-12, (name, np.abs(t.numpy() - ref[name]).max())
    # the coordinates of these cases are exact in float32: the float32 coordinate gives the same restatement
    ref32 = R.softsplat(x, flow, metric, mode, gout)
    for name in names:
        assert np.array_equal(ref32[name], ref[name]), name
    if kind in ('zero', 'integer'):
        assert ref['hit'].sum() > 0 and (kind != 'zero' or ref['hit'].all())
    if kind == 'leave':
        assert 0 < ref['hit'].mean() < 1


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("kind", R.GATED)
def test_the_reference_denominator_is_at_least_one_256th_wherever_something_landed(kind, shape):
    """What the GPU suite's gates rest on: with a metric spread of at most 20 the largest source at a target has e = 1 and b >= 2^-8, so
    the fixed-point step of the kernels (2^-49 of the denominator's unit at these sizes) is far below float32 rounding."""
    x, flow, metric, _ = R.inputs(kind, shape)
    assert metric.max() - metric.min() <= 20
    for mode in R.MODES:
        ref = R.softsplat(x, flow, metric, mode)
        landed = ref['hit'] > 0
        assert landed.any() and ref['D'][landed].min() >= 2.0 ** -8
        assert not ref['D'][~landed].any() and not ref['out'][np.broadcast_to(~landed, ref['out'].shape)].any()


def test_gradcheck_on_fractional_content():
    shape = (1, 1, 4, 4)
    x, flow, metric, _ = (t.double() for t in R.inputs('fractional', shape))
    x, flow, metric = (t.clone().requires_grad_() for t in (x, flow, metric))
    for mode in R.MODES:
        fn = lambda x, flow, metric: hip_ops.softsplat_composed(x, flow, metric if mode == 'soft' else None, mode)
        assert torch.autograd.gradcheck(fn, (x, flow, metric), check_undefined_grad=False), mode
    assert torch.autograd.gradgradcheck(lambda x, flow, metric: hip_ops.softsplat_composed(x, flow, metric, 'soft'), (x, flow, metric))


@pytest.mark.parametrize("shape", R.SHAPES[:4], ids=ids)
def test_a_constant_added_to_the_metric_changes_nothing(shape):
    x, flow, metric, gout = R.inputs('fractional', shape)
    moved = R.inputs('shifted', shape)
    assert all(torch.equal(a, b) for a, b in zip((x, flow, gout), (moved[0], moved[1], moved[3]))) and torch.equal(moved[2], metric + 1000)
    a, b = composed64(x, flow, metric, 'soft', gout), composed64(x, flow, moved[2], 'soft', gout)
    for p, q in zip(a, b):
        assert torch.equal(p, q)                                 # the shift is exact in these inputs: M moves, nothing else
    # ... and in float32, where the published exp(Z) form overflows: finite and the same values
    out = hip_ops.softsplat_composed(x, flow, moved[2], 'soft')
    assert torch.isfinite(out).all() and torch.equal(out, hip_ops.softsplat_composed(x, flow, metric, 'soft'))
    assert not torch.isfinite(torch.exp(moved[2])).any()


def test_wide_and_nonfinite_content_of_the_restatement():
    shape = (2, 3, 7, 9)
    x, flow, metric, gout = R.inputs('wide', shape)
    assert metric.max() - metric.min() > 300
    ref = R.softsplat(x, flow, metric, 'soft', gout)
    assert all(np.isfinite(v).all() for v in ref.values())
    x, flow, metric, gout = R.inputs('nonfinite', shape)
    bad = R.corrupted('nonfinite', shape)
    assert bad.any() and torch.isnan(flow).any() and torch.isinf(flow).any() and torch.isinf(metric).any() and (metric == 1e30).any()
    ref = R.softsplat(x, flow, metric, 'soft', gout)
    assert all(np.isfinite(v).all() for v in ref.values())
    # the same as with those sources moved out of the frame, and zero gradients for them
    flow2, metric2 = flow.clone(), metric.clone()
    flow2[:, 0][bad], flow2[:, 1][bad], metric2[:, 0][bad] = 3.0 * shape[3], 0.0, 0.0
    moved = R.softsplat(x, flow2, metric2, 'soft', gout)
    for key in ref:
        assert np.array_equal(ref[key], moved[key]), key
    mask = bad.numpy()
    assert not ref['g_x'][np.broadcast_to(mask[:, None], ref['g_x'].shape)].any()
    assert not ref['g_flow'][np.broadcast_to(mask[:, None], ref['g_flow'].shape)].any() and not ref['g_metric'][mask[:, None]].any()
    # the composed op agrees on such content (float64, the float32 coordinates of these inputs are exact)
    got = composed64(x, flow, metric, 'soft', gout)
    for name, t in zip(('out', 'hit', 'g_x', 'g_flow', 'g_metric'), got):
        assert np.abs(t.numpy() - ref[name]).max() <= 1e-12, name
    # a non-finite element of x: that whole sample of out is NaN, the other sample is untouched
    x2 = x.clone()
    x2[1, 2, 3, 4] = float('inf')
    ref2 = R.softsplat(x2, flow, metric, 'soft')
    out2 = hip_ops.softsplat_composed(x2.double(), flow.double(), metric.double(), 'soft').numpy()
    assert np.isnan(ref2['out'][1]).all() and np.isnan(out2[1]).all() and np.array_equal(ref2['out'][0], ref['out'][0])
    assert np.abs(out2[0] - ref['out'][0]).max() <= 1e-12


def test_op_arguments_are_checked_and_routed():
    x, flow, metric, _ = R.inputs('fractional', (2, 3, 7, 9))
    out = hip_ops.softsplat(x, flow, metric)                       # CPU tensors: the composed op, soft by default
    assert out.shape == x.shape and torch.equal(out, hip_ops.softsplat_composed(x, flow, metric, 'soft'))
    out, hit = hip_ops.softsplat(x.double(), flow.double(), None, 'avg', return_hit=True)
    assert out.dtype == torch.float64 and hit.shape == (2, 1, 7, 9) and set(hit.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(hip_ops.softsplat(x, flow, metric, 'sum'), hip_ops.softsplat(x, flow, None, 'sum'))      # sum and avg read no metric
    assert hip_ops.softsplat_bytes(x) > hip_ops.softsplat_bytes(x, 'avg') > 0 and hip_ops.softsplat_bytes(x, 'soft', 3) > 0
    with pytest.raises(ValueError):
        hip_ops.softsplat(x, flow, None, 'soft')
    with pytest.raises(ValueError):
        hip_ops.softsplat(x, flow, metric, 'linear')
    with pytest.raises(ValueError):
        hip_ops.softsplat(x, flow[:, :1], metric)
    with pytest.raises(ValueError):
        hip_ops.softsplat(x, flow, metric[:1])
    with pytest.raises(ValueError):
        hip_ops.softsplat(torch.zeros(1, 257, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))


def test_plugin_on_the_cpu_in_float64_against_float32():
    net = build_plugin('softsplat')
    assert type(net).__name__ == 'MetaSoftSplat' and net.lockstep_tasks and net.mode == 'soft'
    assert net.alpha.item() == -20.0 and net.alpha.requires_grad
    keys = set(net.state_dict())
    from meta_interpolation_amd.superslomo.model import MetaUNet
    assert keys == {'alpha'} | {'flowComp.' + k for k in MetaUNet(6, 4).state_dict()} | {'refine.' + k for k in MetaUNet(14, 4).state_dict()}
    from meta_interpolation_amd import synthetic
    f = synthetic.septuplet(0, 64, 64, model='softsplat')
    f0, f1 = f[2].unsqueeze(0), f[4].unsqueeze(0)
    with torch.no_grad():
        out32 = net(f0, f1, ind=3)
        out64 = net.double()(f0.double(), f1.double(), ind=3)
    assert out32.shape == (1, 3, 64, 64) and out32.dtype == torch.float32 and torch.isfinite(out32).all()
    d = (out32.double() - out64).abs()
    print('SOFTSPLAT_PLUGIN_CPU max |f32 - f64| = %.3e, mean %.3e, max |f64| = %.3e' % (d.max(), d.mean(), out64.abs().max()))
    # float32 rounding through two U-Nets of ~25 convolutions and two splats: 1e-4 of the unit range on average (a flow that rounds across
    # a cell edge moves single pixels by more, so the maximum is looser)
    assert d.mean() <= 1e-4 and d.max() <= 2e-2
    net.zero_grad()
    net.restore_backup_stats()
