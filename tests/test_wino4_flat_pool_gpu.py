"""-m gpu: the F(4x4) kernel on flat tile lists and with the pooled output stage (csrc/winograd4.h).

Flat tile lists: workgroup tb of a sample owns tiles 32 tb .. 32 tb + 31 of the sample's row-major tile list.  Held to the block decode
(savfi_conv3x3_debug_f4_block_decode) bit for bit, and both to float64 at the gates of tests/test_conv_variants_gpu.py.  A tile's
arithmetic does not depend on the workgroup or the slot it sits in -- the reduction order over channels, the transforms and the output
stage are per tile -- so the two decodes must agree in every bit.  What can go wrong is the geometry: a group that wraps a row (left- and
right-edge tiles in one wave), the empty slots behind the last tile (loads and stores must be out of range), the division by the tile
count per row.  Maps: 22 x 38 -> 6 x 10 tiles (groups wrap rows, the last one is partial), 9 x 130 -> 3 x 33 tiles (99 of 128 slots), 7 x 5
and 4 x 4 (a handful of tiles partly outside the map); widths 37 / 38 / 40 for row stores of 1 / 2 / 4 floats.

Pooled output stage: savfi_conv3x3_tasks_pre_pool_f32 stores avgpool2x2 of the activated result from the tile it holds in registers, with
savfi_avgpool2x2_fwd_f32's expression and order: held to that kernel applied to the same launch's result, bit for bit, on even and odd
heights and widths (an odd width has no pooled stage: the launcher says so and the caller pools), and the two-output autograd function
to the convolution followed by avg_pool2x2_and_skip, gradients bit for bit."""
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import conv_ref as R
from tests.test_conv_variants_gpu import C_F4, _mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, N = 2, 4
MAPS = [(22, 38), (22, 37), (22, 40), (9, 130), (7, 5), (4, 4)]
CHANNELS = [(51, 51), (16, 40), (8, 8)]


def _both(fn):
    """fn() under the flat decode (the default) and under the block decode; asserts bit equality and returns the flat result"""
    flat = fn()
    with hip_ops.wino4_block_decode():
        block = fn()
    assert torch.equal(flat, block), (flat - block).abs().max().item()
    return flat


def _check64(got, ref, mag, Ci, Co, what):
    from tests.test_hip_ops_gpu import conv3x3_close
    got = got.cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert conv3x3_close(got.double(), ref, Ci, Co), (what, R.global_err(got, ref))
    R.assert_local(got, ref, R.pool7(mag), C_F4, "f4", what)


def _weights(Ci, Co, mode, g):
    return torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * (Ci if mode == 0 else Co) ** 0.5)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: "%dx%d" % hw)
def test_flat_equals_block_decode_and_float64(hw, pad):
    H, W = hw
    for ci, (Ci, Co) in enumerate(CHANNELS):
        g = torch.Generator().manual_seed(4100 + 100 * MAPS.index(hw) + 10 * pad + ci)
        assert hip_ops.wino4_workgroups(N, Ci, Co, H, W, pad, 0) > 0          # an F(4x4) layer
        for mode in (0, 1):
            assert hip_ops.wino4_launched_workgroups(N, Ci, Co, H, W, pad, mode) <= hip_ops.wino4_workgroups(N, Ci, Co, H, W, pad, mode)
        # forward, bias + leaky ReLU
        w = _weights(Ci, Co, 0, g)
        u_f, u_b = hip_ops.conv3x3_filters(w.to(DEV), True, True)
        if H + 2 * pad - 2 > 0 and W + 2 * pad - 2 > 0:
            x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T, Co, generator=g)
            xc, bc = x.to(DEV), b.to(DEV)
            got = _both(lambda: hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.2, pad))
            z, mag = R.conv_tasks64(x, w, pad, T, bias=b)
            _check64(got, R.act(z, 0.2), mag, Ci, Co, "fwd %s pad %d %d->%d" % (hw, pad, Ci, Co))
        # data gradient, plain and masked
        gy = torch.randn(N, Co, H, W, generator=g)
        gyc = gy.to(DEV)
        got = _both(lambda: hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad))
        ref, mag = R.dgrad_tasks64(gy, w, pad, T)
        _check64(got, ref, mag, Ci, Co, "dgrad %s pad %d %d->%d" % (hw, pad, Ci, Co))
        mask = _mask(tuple(got.shape), g)
        mc = mask.to(DEV)
        gotm = _both(lambda: hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad, mask=mc, mask_slope=0.1))
        assert torch.equal(gotm, got * R.mask_factor(mc, 0.1))
        _check64(gotm, ref * R.mask_factor(mask.double(), 0.1), mag, Ci, Co, "masked dgrad %s pad %d %d->%d" % (hw, pad, Ci, Co))


@pytest.mark.parametrize("pad", [0, 1])
def test_flat_equals_block_decode_unit_major(pad):
    """both unit-major input forms (pad 1: columns 1..4 are the 16-byte load, pad 0: columns 2..5) and the unit-major output at 20 x 48:
    5 x 12 tiles and, for the pad-0 data gradient, 6 x 13 -- groups wrap rows either way"""
    H, W, Ci, Co = 20, 48, 24, 40
    g = torch.Generator().manual_seed(4700 + pad)
    w = _weights(Ci, Co, 1, g)
    u_f, u_b = hip_ops.conv3x3_filters(w.to(DEV), True, True)
    gy = torch.randn(N, Co, H, W, generator=g)
    gyc = gy.to(DEV)
    assert hip_ops.conv3x3_in_unit16_supported(gy.shape, w, pad)
    gyu = gyc.reshape(N, Co, H, W // 16, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(N, Co, H, W)
    got = _both(lambda: hip_ops.conv3x3_dgrad_in_unit16(gyu, u_b, T, Ci, Co, pad))
    assert torch.equal(got, hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad))
    ref, mag = R.dgrad_tasks64(gy, w, pad, T)
    _check64(got, ref, mag, Ci, Co, "in16 pad %d" % pad)
    if pad == 1:
        x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T, Co, generator=g)
        xc, bc = x.to(DEV), b.to(DEV)
        got = _both(lambda: hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.0, pad, out_unit16=True))
        plain = hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.0, pad)
        assert torch.equal(got.reshape(N, H, W // 16, Co, 16).permute(0, 3, 1, 2, 4).reshape(N, Co, H, W), plain)
        z, mag = R.conv_tasks64(x, w, pad, T, bias=b)
        _check64(plain, R.act(z, 0.0), mag, Ci, Co, "out16")


def test_flat_equals_block_decode_split_reduction():
    """256 -> 256 at 8 x 8: the reduction chunks split over workgroups, partial outputs summed by wino_split_reduce"""
    H, W, Ci, Co, pad = 8, 8, 256, 256, 1
    assert R.f4_plan(N, Ci, Co, H, W, pad, 0)["nsplit"] > 1
    g = torch.Generator().manual_seed(4800)
    w = _weights(Ci, Co, 0, g)
    u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False)
    x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T, Co, generator=g)
    xc, bc = x.to(DEV), b.to(DEV)
    got = _both(lambda: hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.0, pad))
    z, mag = R.conv_tasks64(x, w, pad, T, bias=b)
    _check64(got, R.act(z, 0.0), mag, Ci, Co, "split")


class _Launches:
    """names of the launches issued inside the block (the package's launch timer)"""

    def __enter__(self):
        self.prev, _hip.TIMER = _hip.TIMER, _hip.KernelTimer()
        self.timer = _hip.TIMER
        return self

    def __exit__(self, *exc):
        _hip.TIMER = self.prev

    def count(self, name):
        return len(self.timer.records.get(name, []))


class _F4Everywhere:
    """the routing thresholds that keep small launches off F(4x4) (hip_ops.wino_form2), lowered: the shapes of a quick test then take
    the route the 256 x 448 workload takes"""

    def __enter__(self):
        self.prev = hip_ops.WINO4_MIN_WORKGROUPS, hip_ops.WINO4_MIN_PIXELS
        hip_ops.WINO4_MIN_WORKGROUPS, hip_ops.WINO4_MIN_PIXELS = 0, 0

    def __exit__(self, *exc):
        hip_ops.WINO4_MIN_WORKGROUPS, hip_ops.WINO4_MIN_PIXELS = self.prev


# Ho x Wo (pad 1: the input's size): even / even with 16-byte rows, odd height with 8-byte rows and an odd pooled width, an odd width
# (no pooled stage), and a map of several tile groups that wrap rows
POOL_MAPS = [(12, 16), (13, 18), (14, 15), (22, 38)]


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("hw", POOL_MAPS, ids=lambda hw: "%dx%d" % hw)
def test_pooled_output_stage_equals_pool_kernel(hw, slope):
    H, W = hw
    Ci, Co, pad = 16, 40, 1
    g = torch.Generator().manual_seed(4900 + 10 * POOL_MAPS.index(hw) + int(10 * slope))
    w = _weights(Ci, Co, 0, g)
    u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False)
    xc, bc = torch.randn(N, Ci, H, W, generator=g).to(DEV), torch.randn(T, Co, generator=g).to(DEV)
    plain = hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, slope, pad)
    for block in (False, True):
        with hip_ops.wino4_block_decode(block), _Launches() as seen:
            y, pooled = hip_ops.conv3x3_tasks_pre_pool(xc, u_f, T, Ci, Co, bc, slope, pad)
        assert seen.count("avgpool2x2_fwd") == (1 if W % 2 else 0)           # an odd width: the caller's pooling kernel
        assert torch.equal(y, plain)
        assert pooled.shape == (N, Co, H // 2, W // 2)
        assert torch.equal(pooled, hip_ops._avgpool2x2_fwd_launch(y)), (hw, slope, block)
        assert torch.equal(pooled, hip_ops.avg_pool2x2(y))


def test_pooled_output_stage_pad0_and_launches_without_it():
    g = torch.Generator().manual_seed(4990)
    # pad 0: 14 x 18 -> 12 x 16
    Ci, Co = 8, 8
    w = _weights(Ci, Co, 0, g)
    u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False)
    xc = torch.randn(N, Ci, 14, 18, generator=g).to(DEV)
    with _Launches() as seen:
        y, pooled = hip_ops.conv3x3_tasks_pre_pool(xc, u_f, T, Ci, Co, None, 0.0, 0)
    assert seen.count("avgpool2x2_fwd") == 0 and y.shape == (N, Co, 12, 16)
    assert torch.equal(y, hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, None, 0, 0.0, 0))
    assert torch.equal(pooled, hip_ops._avgpool2x2_fwd_launch(y))
    # a split reduction (wino_split_reduce finishes the result) and the F(2x2) form: no pooled stage, the pooling kernel runs
    Ci = Co = 256
    w = _weights(Ci, Co, 0, g)
    xc, bc = torch.randn(N, Ci, 8, 8, generator=g).to(DEV), torch.randn(T, Co, generator=g).to(DEV)
    for f2 in (False, True):
        u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False, f2=f2)
        with _Launches() as seen:
            y, pooled = hip_ops.conv3x3_tasks_pre_pool(xc, u_f, T, Ci, Co, bc, 0.0, 1, f2=f2)
        assert seen.count("avgpool2x2_fwd") == 1
        assert torch.equal(y, hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.0, 1, f2=f2))
        assert torch.equal(pooled, hip_ops._avgpool2x2_fwd_launch(y))


@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("hw", [(12, 16), (13, 18)], ids=lambda hw: "%dx%d" % hw)
def test_two_output_function_gradients_equal_conv_then_pool_and_skip(hw, slope):
    H, W = hw
    Ci, Co = 16, 40
    g = torch.Generator().manual_seed(5000 + H + int(10 * slope))
    x0, w0, b0 = torch.randn(N, Ci, H, W, generator=g), _weights(Ci, Co, 0, g), torch.randn(T, Co, generator=g)
    gs, gp = torch.randn(N, Co, H, W, generator=g).to(DEV), torch.randn(N, Co, H // 2, W // 2, generator=g).to(DEV)

    def leaves():
        return [t.to(DEV).requires_grad_() for t in (x0, w0, b0)]

    with _F4Everywhere():
        x, w, b = leaves()
        assert hip_ops.conv_pools_in_epilogue(x, w, 1, 1, 1)
        with _Launches() as seen:
            y, pooled = hip_ops.conv_bias_act_tasks_pool(x, w, b, 1, 1, 1, slope)
        assert seen.count("avgpool2x2_fwd") == 0
        got = torch.autograd.grad([y, pooled], [x, w, b], [gs, gp])
        only_skip = torch.autograd.grad(hip_ops.conv_bias_act_tasks_pool(x, w, b, 1, 1, 1, slope)[0], [x, w, b], gs)
        x2, w2, b2 = leaves()
        y2 = hip_ops.conv_bias_act_tasks(x2, w2, b2, 1, 1, 1, slope, defer=True)
        pooled2, skip2 = hip_ops.avg_pool2x2_and_skip(y2, slope)
        want = torch.autograd.grad([skip2, pooled2], [x2, w2, b2], [gs, gp])
        y3 = hip_ops.conv_bias_act_tasks(x2, w2, b2, 1, 1, 1, slope, defer=True)
        want_skip = torch.autograd.grad(hip_ops.avg_pool2x2_and_skip(y3, slope)[1], [x2, w2, b2], gs)
    assert torch.equal(y, y2) and torch.equal(pooled, pooled2)
    for a, b_, name in zip(got + only_skip, want + want_skip, ["gx", "gw", "gb"] * 2):
        assert torch.equal(a, b_), (name, (a - b_).abs().max().item())


def test_sepconv_forward_backward_equal_with_the_new_paths_on_and_off():
    """one SepConv forward and backward at 64 x 64 on the fused route (fast weights for the encoder / decoder, the four Subnets as one
    launch per layer), with the routing thresholds lowered so that its small maps run where the 256 x 448 workload's do: prediction and
    every gradient bit for bit the same with flat tile lists + the pooled output stage as with the block decode + the pooling kernel"""
    from meta_interpolation_amd import model_utils as mu, synthetic
    from meta_interpolation_amd.sepconv import model as sm
    net = sm.MetaNetwork(windowed=True)
    synthetic.load_seeded_weights(net, 'sepconv')
    net = net.cuda()
    frames = synthetic.septuplet_batch(2, 64, 64, model='sepconv')
    f0, f1, tgt = frames[2].cuda(), frames[4].cuda(), frames[3].cuda()
    routed = {n: p for n, p in net.named_parameters() if n.startswith(('moduleConv', 'moduleDeconv'))}
    own = [(n, p) for n, p in net.named_parameters() if n not in routed]

    def run():
        # stacked fast weights [T = 1, ...]: the lockstep form the meta-learning loop runs
        fast = {n: p.detach().clone()[None].requires_grad_() for n, p in routed.items()}
        with _Launches() as seen:
            out = net(f0, f1, params=fast)
        loss = (out - tgt).abs().mean()
        grads = torch.autograd.grad(loss, list(fast.values()) + [p for _, p in own])
        return out.detach(), dict(zip(list(fast) + [n for n, _ in own], grads)), seen.count("avgpool2x2_fwd")

    mu.set_fuse_conv_act(True)
    prev = sm.POOL_EPILOGUE
    try:
        with _F4Everywhere():
            sm.POOL_EPILOGUE = True
            o_new, g_new, pools_new = run()
            sm.POOL_EPILOGUE = False
            with hip_ops.wino4_block_decode():
                o_old, g_old, pools_old = run()
    finally:
        sm.POOL_EPILOGUE = prev
        mu.set_fuse_conv_act(False)
    assert pools_old == 5 and pools_new < pools_old, (pools_new, pools_old)        # (conv5 splits its reduction: its pooling stays a kernel)
    assert torch.equal(o_new, o_old)
    assert len(g_new) == len(g_old) > 0
    for n, ref in g_old.items():
        assert torch.equal(g_new[n], ref), n
