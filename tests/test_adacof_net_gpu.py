"""-m gpu: the AdaCoF plugin on the device (fused convolutions, the fused deformable-tap op) held to the same plugin on the CPU in float64
(net.double(), the op composed from torch ops): seeded weights, frames 1 x 3 x 70 x 90 -- no multiple of 32, so the mirrored padding and the
crop run -- prediction L1 and the fingerprints of every parameter gradient within the contract bounds of tests/test_system_gpu.py.  A
second test runs the same pass under hip_ops.set_double_backward(True) (the composed op on the device) against the fused pass.

The functional that is differentiated is the product's own loss, L1 to the triplet's middle frame.  A white-noise cotangent (sum(out * randn))
is NOT a usable one here: the parameter gradients of the offset heads then are cancellation residues (moduleAlpha2.4.bias: abs-sum 3.5 out of
an offset-gradient abs-sum of 428), and the one sample of this pass whose offset is -7.5e-7 at base row 52 -- float32 coordinate 52 exactly, the
float64 plugin's 51.999999: the other cell, as the float32 definition of the coordinate says -- moves that tensor's fingerprint by 1.9e-3 in ATen's
float32 on the CPU just as on the device (measured: 1.85e-3 both; under the L1 loss the same sample moves nothing above 5e-5)."""
import functools

import pytest
import torch

from meta_interpolation_amd import hip_ops, model_utils, synthetic
from tests.helpers import assert_fp_close, build_plugin, fp, record_launches
from tests.test_system_gpu import CONTRACT

pytestmark = pytest.mark.gpu

H, W = 70, 90


def frames():
    fr = synthetic.septuplet(3, H, W, model='adacof')
    return fr[2][None], fr[4][None], fr[3][None]


def run(net, f0, f1, target):
    """prediction and {name: gradient} of the L1 loss to the middle frame"""
    out = net(f0, f1)
    names, params = zip(*net.named_parameters())
    grads = torch.autograd.grad((out - target).abs().mean(), params)
    return out.detach(), dict(zip(names, grads))


@functools.lru_cache(maxsize=None)
def cpu_reference():
    net = build_plugin('adacof').double()
    out, grads = run(net, *(t.double() for t in frames()))
    return out, {k: fp(g) for k, g in grads.items()}


def device_pass(second_order=False):
    net = build_plugin('adacof', 'cuda')
    model_utils.set_fuse_conv_act(not second_order)
    hip_ops.set_double_backward(second_order)
    try:
        with record_launches() as rec:
            out, grads = run(net, *(t.cuda() for t in frames()))
        torch.cuda.synchronize()
    finally:
        model_utils.set_fuse_conv_act(False)
        hip_ops.set_double_backward(False)
    return out.cpu(), {k: g.cpu() for k, g in grads.items()}, rec.names


def test_plugin_on_the_device_matches_the_float64_plugin_on_the_cpu():
    want, want_fp = cpu_reference()
    out, grads, launches = device_pass()
    assert launches.count("adacof_fwd") == 2 and launches.count("adacof_bwd") == 2         # one launch per frame and direction
    assert out.shape == (1, 3, H, W)
    l1 = (out.double() - want).abs().mean().item()
    worst = max(max(abs(fp(g)[i] - want_fp[k][i]) for i in (0, 1)) / max(abs(want_fp[k][1]), 1e-12) for k, g in grads.items())
    print("ADACOF_NET fused l1=%.3e (bound %.0e) worst gradient fingerprint=%.3e (bound %.0e)" % (l1, CONTRACT['l1'], worst, CONTRACT['g']))
    assert l1 <= CONTRACT['l1']
    assert set(grads) == set(want_fp) and len(grads) == 118
    for k, g in grads.items():
        assert_fp_close(fp(g), want_fp[k], CONTRACT['g'], ('adacof', 'g', k))


def test_second_order_pass_on_the_device_equals_the_fused_pass():
    want, want_fp = cpu_reference()
    out, grads, launches = device_pass(second_order=True)
    assert "adacof_fwd" not in launches and "adacof_bwd" not in launches                   # the composed op
    fused_out, fused_grads, _ = device_pass()
    l1 = (out - fused_out).abs().mean().item()
    worst = max(max(abs(fp(g)[i] - fp(fused_grads[k])[i]) for i in (0, 1)) / max(abs(fp(fused_grads[k])[1]), 1e-12) for k, g in grads.items())
    print("ADACOF_NET composed vs fused l1=%.3e (bound %.0e) worst gradient fingerprint=%.3e (bound %.0e)" % (l1, CONTRACT['l1'], worst, CONTRACT['g']))
    assert l1 <= CONTRACT['l1'] and (out.double() - want).abs().mean().item() <= CONTRACT['l1']
    for k, g in grads.items():
        assert_fp_close(fp(g), fp(fused_grads[k]), CONTRACT['g'], ('adacof', 'composed vs fused', k))
        assert_fp_close(fp(g), want_fp[k], CONTRACT['g'], ('adacof', 'composed vs float64', k))
