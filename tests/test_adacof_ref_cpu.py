"""The AdaCoF restatement (tests/adacof_ref.py) held to F.grid_sample per tap in float64, the float32 coordinate told apart from the
float64 one by the bounds, hip_ops.adacof_composed held to the restatement and to gradcheck / gradgradcheck, and the plugin on the CPU:
its parameter names and shapes and one forward."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops
from tests import adacof_ref as R
from tests.helpers import build_plugin

SHAPES = [(1, 3, 5, 7, 5, 1), (2, 3, 9, 33, 5, 1), (1, 3, 17, 40, 3, 2), (1, 1, 8, 32, 1, 1), (1, 3, 6, 6, 11, 2)]     # N, C, H, W, F, d


def _grads64(fn, x, w, a, b, d, gout):
    w, a, b = (t.double().clone().requires_grad_() for t in (w, a, b))
    out = fn(x.double(), w, a, b, d)
    return (out.detach(),) + torch.autograd.grad(out, (w, a, b), gout.double())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["small", "cross"])
def test_float64_restatement_equals_grid_sample_per_tap(shape, kind):
    N, C, H, W, F, d = shape
    x, w, a, b, gout = R.inputs(kind, N, C, H, W, F, d)
    ref = R.adacof(x, w, a, b, d, gout, coord=np.float64)
    out, gw, ga, gb = _grads64(R.grid_sample_statement, x, w, a, b, d, gout)
    keep = ~ref['near']
    assert 1 - keep.double().mean().item() <= R.NEAR_CAP
    assert (out - ref['out']).abs().max().item() <= 1e-12
    assert (gw - ref['g_w']).abs().max().item() <= 1e-12
    assert (ga - ref['g_a'])[keep].abs().max().item() <= 1e-12
    assert (gb - ref['g_b'])[keep].abs().max().item() <= 1e-12
    # the composed op in float64 is the same statement, gradients included
    out, gw, ga, gb = _grads64(hip_ops.adacof_composed, x, w, a, b, d, gout)
    assert (out - ref['out']).abs().max().item() <= 1e-12 and (gw - ref['g_w']).abs().max().item() <= 1e-12
    assert (ga - ref['g_a'])[keep].abs().max().item() <= 1e-12 and (gb - ref['g_b'])[keep].abs().max().item() <= 1e-12


def test_the_bounds_tell_a_float64_coordinate_from_the_float32_one():
    """At W = 200 the float32 coordinate carries a rounding of up to 2^-17 = 7.6e-6 pixels; the gate of a 3 x 3 op is 14 units of
    6e-8 of a sum of magnitudes of order one.  The float32 restatement is inside its own gates (ratio 0); the float64 one is not."""
    N, C, H, W, F, d = 1, 3, 9, 200, 3, 1
    x, w, a, b, gout = R.inputs('cross', N, C, H, W, F, d)
    r32, r64 = R.adacof(x, w, a, b, d, gout, coord=np.float32), R.adacof(x, w, a, b, d, gout, coord=np.float64)
    keep = ~r32['near']
    assert R.masked_ratio(r64['out'], r32['out'], r32['out_mag'], R.fwd_units(F)) > 1
    assert R.masked_ratio(r64['g_w'], r32['g_w'], r32['g_w_mag'], R.gw_units(C)) > 1
    assert R.masked_ratio(r64['g_a'], r32['g_a'], r32['g_a_mag'], R.goff_units(C), keep) > 1
    assert R.masked_ratio(r64['g_b'], r32['g_b'], r32['g_b_mag'], R.goff_units(C), keep) > 1
    # the composed op in float32 forms the float32 coordinate: inside the gates of the float32 restatement
    wr, ar, br = (t.clone().requires_grad_() for t in (w, a, b))
    out = hip_ops.adacof_composed(x, wr, ar, br, d)
    gw, ga, gb = torch.autograd.grad(out, (wr, ar, br), gout)
    assert R.masked_ratio(out, r32['out'], r32['out_mag'], R.fwd_units(F)) <= 1
    assert R.masked_ratio(gw, r32['g_w'], r32['g_w_mag'], R.gw_units(C)) <= 1
    assert R.masked_ratio(ga, r32['g_a'], r32['g_a_mag'], R.goff_units(C), keep) <= 1
    assert R.masked_ratio(gb, r32['g_b'], r32['g_b_mag'], R.goff_units(C), keep) <= 1


def test_edge_content_of_the_restatement():
    N, C, H, W, F, d = 1, 3, 9, 33, 5, 1
    # outside: the border texel sum, offset gradients exactly 0
    x, w, a, b, gout = R.inputs('outside', N, C, H, W, F, d)
    ref = R.adacof(x, w, a, b, d, gout)
    assert not ref['g_a'].any() and not ref['g_b'].any()
    Hp, Wp = x.shape[2:]
    rows = torch.where(torch.arange(H) < (H + 1) // 2, 0, Hp - 1)
    cols = torch.where(torch.arange(W) < (W + 1) // 2, 0, Wp - 1)
    corner = x.double()[:, :, rows][:, :, :, cols]
    assert (ref['out'] - corner * w.double().sum(1, keepdim=True)).abs().max() <= 1e-13
    # integer: exact coordinates, a one-hot weight reproduces one texel
    x, w, a, b, gout = R.inputs('integer', N, C, H, W, F, d)
    ref = R.adacof(x, w, a, b, d, gout)
    s32, s64 = R.coords(a, b, F, d, np.float32), R.coords(a, b, F, d, np.float64)
    assert all(np.array_equal(p.astype(np.float64), q) for p, q in zip(s32, s64))
    assert ref['near'].all()
    assert np.isin(ref['out'].numpy(), x.double().numpy()).all()
    # wild: NaN exactly where a NaN offset is, finite elsewhere (inf and 1e30 are clamped)
    x, w, a, b, gout = R.inputs('wild', N, C, H, W, F, d)
    ref = R.adacof(x, w, a, b, d, gout)
    nan_tap = torch.isnan(a) | torch.isnan(b)
    assert nan_tap.any() and torch.isinf(a).any() and (a.abs() == 1e30).any()
    assert torch.equal(torch.isnan(ref['out']), ref['nan'].unsqueeze(1).expand_as(ref['out']))
    for key in ('g_w', 'g_a', 'g_b'):
        assert torch.equal(torch.isnan(ref[key]), nan_tap), key


def test_composed_op_passes_gradcheck_and_gradgradcheck():
    gen = torch.Generator().manual_seed(5)
    N, C, H, W, F, d = 1, 1, 4, 5, 3, 1
    x = torch.randn(N, C, H + 2, W + 2, generator=gen, dtype=torch.float64)
    w = torch.randn(N, F * F, H, W, generator=gen, dtype=torch.float64).requires_grad_()
    # offsets kept a tenth of a pixel off every cell edge: finite differences must not cross one
    frac = lambda: 0.1 + 0.8 * torch.rand(N, F * F, H, W, generator=gen, dtype=torch.float64)
    cell = lambda: torch.randint(-2, 2, (N, F * F, H, W), generator=gen).double()
    a, b = (cell() + frac()).requires_grad_(), (cell() + frac()).requires_grad_()
    fn = lambda w, a, b: hip_ops.adacof_composed(x, w, a, b, d)
    assert torch.autograd.gradcheck(fn, (w, a, b))
    assert torch.autograd.gradgradcheck(fn, (w, a, b))


def test_op_arguments_are_checked_and_routed():
    x, w, a, b, _ = R.inputs('small', 1, 3, 5, 7, 5, 1)
    out = hip_ops.adacof(x, w, a, b)                      # CPU tensors: the composed op
    assert out.shape == (1, 3, 5, 7) and torch.equal(out, hip_ops.adacof_composed(x, w, a, b, 1))
    assert hip_ops.adacof(x.double(), w.double(), a.double(), b.double()).dtype == torch.float64
    with pytest.raises(ValueError):
        hip_ops.adacof(x, w, a, b, dilation=2)            # the frame is padded for dilation 1
    with pytest.raises(ValueError):
        hip_ops.adacof(x, w[:, :16], a[:, :16], b[:, :16])
    with pytest.raises(ValueError):
        hip_ops.adacof(x, w, a[:, :9], b)
    with pytest.raises(ValueError):
        hip_ops.adacof(x[:, :2], w, a, b)
    with pytest.raises(ValueError):
        hip_ops.adacof(x, w, a, b, dilation=9)


def _expected_state(F2):
    names = {}
    chans = [(6, 32), (32, 64), (64, 128), (128, 256), (256, 512)]
    for i, (cin, cout) in enumerate(chans, start=1):
        for k, (ci, co) in zip((0, 2, 4), ((cin, cout), (cout, cout), (cout, cout))):
            names["moduleConv%d.%d" % (i, k)] = (co, ci)
    for i, (cin, cout) in zip((5, 4, 3, 2), ((512, 512), (512, 256), (256, 128), (128, 64))):
        for k, (ci, co) in zip((0, 2, 4), ((cin, cout), (cout, cout), (cout, cout))):
            names["moduleDeconv%d.%d" % (i, k)] = (co, ci)
        names["moduleUpsample%d.1" % i] = (cout, cout)
    heads = [("module%s%d" % (kind, i), F2) for i in (1, 2) for kind in ("Weight", "Alpha", "Beta")] + [("moduleOcclusion", 1)]
    for head, n in heads:
        for k, (ci, co) in zip((0, 2, 4, 7), ((64, 64), (64, 64), (64, n), (n, n))):
            names["%s.%d" % (head, k)] = (co, ci)
    out = {}
    for name, (co, ci) in names.items():
        out[name + ".weight"] = (co, ci, 3, 3)
        out[name + ".bias"] = (co,)
    return out


def test_plugin_builds_on_the_cpu_with_the_published_names():
    net = build_plugin('adacof')
    assert type(net).__name__ == 'MetaAdaCoF' and net.lockstep_tasks and net.kernel_size == 5 and net.dilation == 1
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == _expected_state(25)
    from meta_interpolation_amd.adacof.model import MetaAdaCoF
    assert {k: tuple(v.shape) for k, v in MetaAdaCoF(kernel_size=3, dilation=2).state_dict().items()} == _expected_state(9)
    gen = torch.Generator().manual_seed(1)
    f0, f1 = torch.rand(1, 3, 40, 56, generator=gen), torch.rand(1, 3, 40, 56, generator=gen)
    with torch.no_grad():
        out = net(f0, f1)
    assert out.shape == (1, 3, 40, 56) and torch.isfinite(out).all()
    # a softmax-weighted mean of texels blended by a sigmoid stays in the frames' range
    assert out.min() >= min(f0.min(), f1.min()) - 1e-5 and out.max() <= max(f0.max(), f1.max()) + 1e-5
    net.zero_grad()
    net.restore_backup_stats()


def test_sepconv_keeps_its_state_dict_after_sharing_the_unet_builders():
    from meta_interpolation_amd import kernel_unet
    from meta_interpolation_amd.sepconv import model as sm
    keys = list(build_plugin('sepconv').state_dict())
    want = []
    for i in range(1, 6):
        want += ["moduleConv%d.%d.%s" % (i, k, p) for k in (0, 2, 4) for p in ("weight", "bias")]
    for i in (5, 4, 3, 2):
        want += ["moduleDeconv%d.%d.%s" % (i, k, p) for k in (0, 2, 4) for p in ("weight", "bias")]
        want += ["moduleUpsample%d.1.%s" % (i, p) for p in ("weight", "bias")]
    for head in ("moduleVertical1", "moduleVertical2", "moduleHorizontal1", "moduleHorizontal2"):
        want += ["%s.%d.%s" % (head, k, p) for k in (0, 2, 4, 7) for p in ("weight", "bias")]
    assert keys == want
    assert not hasattr(sm, '_basic') and kernel_unet.ENCODER[0] == ("moduleConv1", 6, 32)       # one copy of the builders
