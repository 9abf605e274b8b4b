"""-m gpu: the stages of MetaDAIN (dain/networks/DAIN.py) against the float64 restatements of tests/dain_net_ref.py, on 1x3x64x64 and
2x3x64x64 frames (64 is the smallest side the padding rule leaves alone) and one 1x3x40x72 case for the padding and its inverse.

Weights: the numpy rule of tests/dain_net_ref.py; the flow estimator's are pwc_ref.network_fixture() (its flow predictors scaled).  Each
stage is compared against the restatement fed with the DEVICE's own upstream tensors (MetaDAIN.front(..., keep_parts=True)), so a discrete
decision upstream -- a floor in the warp, a hole in the projection -- cannot turn rounding into a large difference downstream; no pixel
is left out of any comparison.  Gate per stage: |device - float64| <= max(3 E, 4 * 2^-24 * scale), E = the largest |float32 host
restatement - float64|, scale = the largest |float64|.  A run with -s prints one DAIN_NET_PARITY line per comparison.

The rectify net's ten gradients follow the same rule inside their stage: the restatement differentiates on the device's own seven ReLU
decisions.  Measured without that (1x3x64x64, default routes): a single pre-activation of block3.conv1 within rounding of 0 decided
differently put block3.conv1's gradient and every one upstream of it 12 to 139 times over a gate that those downstream met at 0.26 to
0.67 -- and on 2x3x64x64 the HOST's float32 run had such a flip of its own (E ten times the other inputs').  Frame and loss are compared
with the plain restatement.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops, model_utils
from meta_interpolation_amd.dain.networks.DAIN import MetaDAIN
from tests import dain_net_ref as R
from tests import pwc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, K = 4 * 2.0 ** -24, 3.0
SEED = 5200
INPUTS = {'1x3x64x64': (1, 3, 64, 64), '2x3x64x64': (2, 3, 64, 64), '1x3x40x72': (1, 3, 40, 72)}


def gate_check(what, got, r32, r64, failed=None):
    got, r32, r64 = (np.asarray(t.cpu() if torch.is_tensor(t) else t, np.float64) for t in (got, r32, r64))
    assert got.shape == r64.shape and np.isfinite(got).all(), what
    E, scale = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
    gate = max(K * E, FLOOR * scale)
    err = float(np.abs(got - r64).max())
    print('DAIN_NET_PARITY %s err=%.3e E=%.3e scale=%.3e gate=%.3e err/gate=%.3f' % (what, err, E, scale, gate, err / gate if gate else 0.0))
    if failed is None:
        assert err <= gate, (what, err, gate)
    elif err > gate:
        failed.append((what, err, gate))


@functools.lru_cache(maxsize=None)
def weights():
    state = R.numpy_rule_state(R.metadain_shapes(), SEED)
    flow_sd, _ = pwc_ref.network_fixture()
    state.update({'flownets.' + k: v for k, v in flow_sd.items()})
    return state


def sub_state(prefix):
    return {k[len(prefix):]: v for k, v in weights().items() if k.startswith(prefix)}


@functools.lru_cache(maxsize=None)
def network():
    net = MetaDAIN()
    net.load_state_dict({k: v.clone() for k, v in weights().items()}, strict=True)
    net.freeze_front()
    return net.to(DEV).train()


@functools.lru_cache(maxsize=None)
def frames(name):
    shape = INPUTS[name]
    return tuple(R.numpy_rule_frames(shape, SEED + 10 + i + 100 * shape[0] + shape[3]) for i in range(3))      # frame0, target, frame1


@functools.lru_cache(maxsize=None)
def front_of(name, training=True):
    """The device's front of an input, once, shared by the stage tests (the network is put back into training mode)."""
    f0, _, f1 = frames(name)
    net = network()
    net.train(training)
    try:
        fr = net.front(f0.to(DEV), f1.to(DEV), keep_parts=True)
        torch.cuda.synchronize()
    finally:
        net.train(True)
    return fr


def pair_batch(parts):
    """The depth net's batch: the two frames of a pair adjacent."""
    return torch.stack((parts['input0'], parts['input2']), 1).flatten(0, 1).cpu()


@pytest.mark.parametrize("name", ('1x3x64x64', '2x3x64x64'))
def test_hourglass_training_mode_and_running_buffers(name):
    fr = front_of(name)
    net = network()
    x = pair_batch(fr.parts)
    sd = sub_state('depthNet.')
    y32, after32 = R.hourglass_forward(sd, x, torch.float32, True, 2)
    y64, after64 = R.hourglass_forward(sd, x, torch.float64, True, 2)
    got = torch.stack(fr.parts['log_depth'], 1).flatten(0, 1)
    gate_check('hourglass_train %s' % name, got, y32, y64)
    # the running buffers after a forward on this front: one update per pair, in order
    saved = {k: v.clone() for k, v in net.depthNet.state_dict().items()}
    try:
        net.depthNet.update_running_stats(fr.bn_stats)
        torch.cuda.synchronize()
        now = {k: v.cpu() for k, v in net.depthNet.state_dict().items()}
    finally:
        net.depthNet.load_state_dict(saved)
    failed = []
    for kind in ('running_mean', 'running_var'):
        keys = [k for k in now if k.endswith(kind)]
        cat = lambda d: torch.cat([d[k].double().flatten() for k in keys])
        gate_check('hourglass_%s %s' % (kind, name), cat(now), cat(after32), cat(after64), failed)
    assert not failed, failed
    assert all(int(now[k]) == x.shape[0] // 2 for k in now if k.endswith('num_batches_tracked'))
    assert all(torch.equal(now[k], saved[k].cpu()) for k in now if k.endswith(('weight', 'bias')))


def test_hourglass_eval_mode_reads_the_running_buffers_and_updates_nothing():
    name = '1x3x64x64'
    net = network()
    before = {k: v.clone() for k, v in net.depthNet.state_dict().items()}
    fr = front_of(name, training=False)
    assert fr.bn_stats is None
    x = pair_batch(fr.parts)
    sd = sub_state('depthNet.')
    y32, _ = R.hourglass_forward(sd, x, torch.float32, False)
    y64, _ = R.hourglass_forward(sd, x, torch.float64, False)
    gate_check('hourglass_eval %s' % name, torch.stack(fr.parts['log_depth'], 1).flatten(0, 1), y32, y64)
    assert all(torch.equal(v, before[k]) for k, v in net.depthNet.state_dict().items())


@pytest.mark.parametrize("name", ('1x3x64x64', '2x3x64x64'))
def test_context_and_filter_nets(name):
    fr = front_of(name)
    p = fr.parts
    failed = []
    sd = sub_state('ctxNet.')
    for i, key in enumerate(('input0', 'input2')):
        x = p[key].cpu()
        gate_check('context%d %s' % (i, name), p['ctx'][i], R.s2df_forward(sd, x, torch.float32), R.s2df_forward(sd, x, torch.float64), failed)
    x6 = torch.cat((p['input0'], p['input2']), 1).cpu()
    r32, r64 = R.filternet_forward(weights(), x6, torch.float32), R.filternet_forward(weights(), x6, torch.float64)
    gate_check('filter_trunk %s' % name, p['filter_trunk'], r32[0], r64[0], failed)
    for i in range(2):
        gate_check('filter_head%d %s' % (i, name), p['filters'][i], r32[1 + i], r64[1 + i], failed)
    assert not failed, failed


def test_glue_depth_inverse_projection_warps_and_channel_order():
    name = '1x3x64x64'
    fr = front_of(name)
    p = fr.parts
    n = lambda t: t.cpu().numpy()
    args = (n(p['input0']), n(p['input2']), [n(t) for t in p['log_depth']], [n(t) for t in p['ctx']], [n(t) for t in p['filters']],
            [n(t) for t in p['flows']])
    offs = [n(t) for t in p['offsets']]
    g32, g64 = R.glue(*args, dtype=np.float32, warp_offsets=offs), R.glue(*args, dtype=np.float64, warp_offsets=offs)
    failed = []
    for i in range(2):
        gate_check('depth_inv%d' % i, p['depth_inv'][i], g32['depth_inv'][i], g64['depth_inv'][i], failed)
        gate_check('projection%d' % i, p['offsets'][i], g32['offsets'][i], g64['offsets'][i], failed)
        gate_check('warp_frame%d' % i, p['refs'][i], g32['refs'][i], g64['refs'][i], failed)
        gate_check('warp_context%d' % i, p['ctx_warped'][i], g32['ctx_warped'][i], g64['ctx_warped'][i], failed)
    gate_check('cur_output', fr.cur_output, g32['cur_output'], g64['cur_output'], failed)
    gate_check('rectify_input', fr.rectify_input, g32['rectify_input'], g64['rectify_input'], failed)
    assert not failed, failed
    assert fr.rectify_input.shape == (1, 437, 64, 64) and fr.padding == (0, 0, 0, 0)
    # the x4 flows: div_flow * 0.5 times the estimator's flow, bilinear x4 with align_corners=False
    net = network()
    with torch.no_grad():
        flow = net.flownets(torch.cat((p['input0'], p['input2']), 1))
    assert torch.equal(p['flows'][0], F.interpolate(20.0 * flow * 0.5, scale_factor=4, mode='bilinear', align_corners=False))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_rectify_net_loss_and_the_ten_gradients(name):
    f0, target, f1 = frames(name)
    fr = front_of(name)
    net = network()
    model_utils.set_fuse_conv_act(True)
    try:
        names = ['rectifyNet.' + k for k in R.RECTIFY_NAMES]
        params = dict(net.named_parameters())
        fast = {k: params[k].detach().clone().requires_grad_() for k in names}
        saved = {k: v.clone() for k, v in net.depthNet.state_dict().items()}
        try:
            out = net(f0.to(DEV), f1.to(DEV), params=fast, front=fr)
        finally:
            net.depthNet.load_state_dict(saved)                                    # (a training-mode forward moves the running buffers)
        loss = hip_ops.charbonnier_loss(out, target.to(DEV))
        grads = torch.autograd.grad(loss, [fast[k] for k in names])
        # the device's own seven ReLU decisions, layer by layer on the same kernels
        with torch.no_grad():
            rn = net.rectifyNet
            y = rn.block1(fr.rectify_input)
            masks = [y > 0]
            for blk in (rn.block2, rn.block3, rn.block4):
                masks.append(blk.conv1(y, act_slope=0.0) > 0)
                y = blk(y)
                masks.append(y > 0)
            assert torch.equal(MetaDAIN.unpad(rn.block5(y) + fr.cur_output, fr.padding), out)      # the same bits as the forward above
        masks = [m.cpu() for m in masks]
        torch.cuda.synchronize()
    finally:
        model_utils.set_fuse_conv_act(False)
    assert out.shape == f0.shape                                                   # the padding's inverse
    sd = sub_state('rectifyNet.')
    refs = []
    for dtype in (torch.float32, torch.float64):
        # the loss is taken on the unpadded frame
        params_t = {k: v.detach().to('cpu', dtype).requires_grad_() for k, v in sd.items()}
        x_t, cur_t = fr.rectify_input.cpu().to(dtype), fr.cur_output.cpu().to(dtype)
        with torch.no_grad():
            frame = MetaDAIN.unpad(R.rectify_forward(params_t, x_t) + cur_t, fr.padding)       # frame and loss: the plain restatement
            l = R.charbonnier(frame, target.to(dtype))
        # the gradients: the restatement on the device's ReLU decisions (tests/dain_net_ref.py rectify_forward)
        lm = R.charbonnier(MetaDAIN.unpad(R.rectify_forward(params_t, x_t, masks) + cur_t, fr.padding), target.to(dtype))
        refs.append((frame, l, torch.autograd.grad(lm, [params_t[k] for k in R.RECTIFY_NAMES])))
    failed = []
    gate_check('rectified_frame %s' % name, out.detach(), refs[0][0], refs[1][0], failed)
    gate_check('charbonnier %s' % name, loss.detach(), refs[0][1], refs[1][1], failed)
    for i, k in enumerate(R.RECTIFY_NAMES):
        gate_check('grad %s %s' % (k, name), grads[i], refs[0][2][i], refs[1][2][i], failed)
    assert not failed, failed


def test_padding_mirrors_the_frames_to_multiples_of_64():
    f0, _, f1 = frames('1x3x40x72')
    fr = front_of('1x3x40x72')
    assert fr.padding == (28, 28, 12, 12) and fr.rectify_input.shape == (1, 437, 64, 128) and fr.cur_output.shape == (1, 3, 64, 128)
    assert torch.equal(fr.parts['input0'].cpu(), F.pad(f0, (28, 28, 12, 12), mode='reflect'))
    assert torch.equal(fr.parts['input2'].cpu(), F.pad(f1, (28, 28, 12, 12), mode='reflect'))
    assert torch.equal(MetaDAIN.unpad(fr.parts['input0'], fr.padding).cpu(), f0)


def test_front_is_reproducible_and_pairs_are_independent():
    net = network()
    f0, _, f1 = (t.to(DEV) for t in frames('2x3x64x64'))
    count = net.front_evaluations
    a, b = net.front(f0, f1), net.front(f0, f1)
    assert net.front_evaluations == count + 4
    assert torch.equal(a.rectify_input, b.rectify_input) and torch.equal(a.cur_output, b.cur_output)
    assert torch.equal(a.bn_stats['mean'], b.bn_stats['mean']) and torch.equal(a.bn_stats['var'], b.bn_stats['var'])
    # the fused two-group call equals the two single calls, bit for bit
    for i in range(2):
        one = net.front(f0[i:i + 1], f1[i:i + 1])
        assert torch.equal(one.rectify_input[0], a.rectify_input[i]), i
        assert torch.equal(one.cur_output[0], a.cur_output[i]), i
        assert torch.equal(one.bn_stats['mean'][0], a.bn_stats['mean'][i]) and torch.equal(one.bn_stats['var'][0], a.bn_stats['var'][i]), i
    assert not a.rectify_input.requires_grad
