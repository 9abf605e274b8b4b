"""-m gpu: the launch manifest of the op layer -- for every op, the ordered (timer name, checked symbols, nbytes, flops) of the launches
one call issues through _hip.launch, compared exactly with tests/golden/launch_manifest.json.

bench.py selects the kernels it times by the name and computes its roofline lines from nbytes / flops; the `what` string a return code is
checked with is the symbol an error message names.  No other test looks at the byte and flop counts, so a change of the host code that
moves one of them, renames a launch, reorders two or checks a code under another symbol's name fails here.

The fixture was recorded ONCE, by `python -m tests.test_launch_manifest_gpu <path>` on an MI355X, from the commit before the op layer
moved to _hip.call (this file and the recorder of tests/helpers.py placed on that tree).  It is not regenerated from the code under test:
a case that legitimately changes gets its entry edited by hand, with the reason in the commit.  The two adacof entries were written by
hand in that way (the op came after the recording): adacof_bytes of the case's shapes, each operand once.

Every case returns the tensors it produced (outputs, gradients, buffers updated in place) as a flat list: this file drops them,
tests/test_launch_guards_gpu.py compares two runs of each case through them.

Shapes: the warps, SepConv and the loss terms at the smallest size that reaches each path; every other op at the smallest shape its own
GPU test uses (the convolution routes: the cases of tests/test_conv_dispatch_gpu.py).  Module knobs stay at their defaults except where a
case names one, and that case restores it."""
import contextlib
import json
import os
import sys
import types

import pytest
import torch

from meta_interpolation_amd import _hip, graph_inner_loop, hip_ops
from meta_interpolation_amd.sepconv.sepconv_op import sepconv as S
from tests import test_conv_dispatch_gpu as D
from tests.helpers import GOLDEN, record_launches

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIXTURE = os.path.join(GOLDEN, "launch_manifest.json")


def _gen(seed=0):
    return torch.Generator(device=DEV).manual_seed(seed)


def _flat(*results):
    """Every tensor in `results` (tensors, None, scalars, nested lists / tuples / dicts of them), detached, in order: what a case
    returns, so that a caller can compare two runs of it."""
    out = []
    for r in results:
        if isinstance(r, torch.Tensor):
            out.append(r.detach())
        elif isinstance(r, dict):
            out += _flat(*r.values())
        elif isinstance(r, (list, tuple)):
            out += _flat(*r)
    return out


def _randn(g, *shape, grad=False):
    return torch.randn(shape, device=DEV, generator=g).requires_grad_(grad)


def _rand(g, *shape, grad=False):
    return torch.rand(shape, device=DEV, generator=g).requires_grad_(grad)


@contextlib.contextmanager
def _knob(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


# ---------------------------------------------------------------------------------------------
# the two warps
# ---------------------------------------------------------------------------------------------
def _warp_once(fn, a_shape, b_shape, a_grad):
    g = _gen(1)
    a, b = _randn(g, *a_shape, grad=a_grad), _randn(g, *b_shape, grad=True)
    out = fn(a, b)
    return [out, *torch.autograd.grad(out, [a, b] if a_grad else [b], _randn(g, *out.shape))]


def _warp_twice(fn, a_shape, b_shape, both):
    """create_graph=True, then a second backward: w.r.t. the cotangent and the flow (`both`) or the flow alone."""
    g = _gen(2)
    a, b = _randn(g, *a_shape), _randn(g, *b_shape, grad=True)
    out = fn(a, b)
    gO = _randn(g, *out.shape, grad=both)
    gb, = torch.autograd.grad(out, b, gO, create_graph=True)
    return [out, gb, *torch.autograd.grad(gb, [b, gO] if both else [b], _randn(g, *gb.shape))]


VOX, FLOW = ((2, 6, 5, 7), (2, 3, 5, 7)), ((2, 3, 5, 7), (2, 2, 5, 7))


# ---------------------------------------------------------------------------------------------
# SepConv: B = 1, C = 3, Ho = 4, Wo = 8, K = 51
# ---------------------------------------------------------------------------------------------
def _sepconv_inputs(frames8):
    g = _gen(3)
    inp = (torch.randint(0, 256, (1, 3, 54, 58), device=DEV, generator=g).float() / 255) if frames8 else _rand(g, 1, 3, 54, 58)
    return g, inp, _randn(g, 1, 51, 4, 8) / 7, _randn(g, 1, 51, 4, 8) / 7


def _needs_frames8(frames8):
    if frames8 and not S.frames8_supported(torch.empty(1, device=DEV), 1, 3, 4, 8, 51):
        pytest.skip("the library does not take the 8-bit-frame kernels in this process (frames8_supported says no)")


def _sepconv_once(frames8, want_gI):
    _needs_frames8(frames8)
    g, inp, v, h = _sepconv_inputs(frames8)
    inp.requires_grad_(want_gI)
    v.requires_grad_(), h.requires_grad_()
    out = S.FunctionSepconv.apply(inp, v, h)
    return [out, *torch.autograd.grad(out, ([inp] if want_gI else []) + [v, h], _randn(g, *out.shape))]


def _sepconv_twice(frames8):
    _needs_frames8(frames8)
    g, inp, v, h = _sepconv_inputs(frames8)
    v.requires_grad_(), h.requires_grad_()
    out = S.FunctionSepconvTwice.apply(inp, v, h)
    gO = _randn(g, *out.shape, grad=True)
    gV, gH = torch.autograd.grad(out, [v, h], gO, create_graph=True)
    return [out, gV, gH, *torch.autograd.grad([gV, gH], [v, h, gO], [_randn(g, *gV.shape), _randn(g, *gH.shape)])]


def _sepconv_pair(frames8=True, one_launch=True):
    _needs_frames8(frames8)
    g = _gen(4)
    f0, f1 = (torch.randint(0, 256, (1, 3, 54, 58), device=DEV, generator=g).float() / 255 for _ in range(2))
    taps = (_randn(g, 4, 51, 4, 8) / 7).requires_grad_()
    with _knob(S, "FRAMES8", frames8), _knob(S, "PAIR_ONE_LAUNCH", one_launch):
        out = S.FunctionSepconvPair.apply(f0, f1, taps)
        return [out, *torch.autograd.grad(out, taps, _randn(g, *out.shape))]


# ---------------------------------------------------------------------------------------------
# the loss terms and the metrics: sr, hr [2, 3, 33, 35]
# ---------------------------------------------------------------------------------------------
def _loss(fn, **kw):
    g = _gen(5)
    sr, hr = _rand(g, 2, 3, 33, 35, grad=True), _rand(g, 2, 3, 33, 35)
    out = fn(sr, hr, **kw)
    return [out, *torch.autograd.grad(out, sr, torch.ones_like(out))]


def _metric(fn):
    g = _gen(6)
    return _flat(fn(_rand(g, 2, 3, 33, 35), _rand(g, 2, 3, 33, 35)))


# ---------------------------------------------------------------------------------------------
# everything else
# ---------------------------------------------------------------------------------------------
def _fwd_bwd(fn, *shapes, seed=7):
    """fn of seeded leaves of `shapes`, then the gradient of the (first) result for all of them."""
    g = _gen(seed)
    leaves = [_randn(g, *s, grad=True) for s in shapes]
    outs = fn(*leaves)
    out = outs[0] if isinstance(outs, (tuple, list)) else outs
    return _flat(outs, torch.autograd.grad(out, leaves, _randn(g, *out.shape), allow_unused=True))


def _both_outputs(fn, *shapes, seed=8):
    """The same for an op with two results that both carry a cotangent."""
    g = _gen(seed)
    leaves = [_randn(g, *s, grad=True) for s in shapes]
    a, b = fn(*leaves)
    return _flat(a, b, torch.autograd.grad([a, b], leaves, [_randn(g, *a.shape), _randn(g, *b.shape)], allow_unused=True))


def _avgpool_second_order():
    g = _gen(9)
    x = _randn(g, 1, 5, 7, 9, grad=True)
    gO = _randn(g, 1, 5, 3, 4, grad=True)
    gx, = torch.autograd.grad(hip_ops.avg_pool2x2(x), x, gO, create_graph=True)
    return [gx, *torch.autograd.grad(gx, gO, _randn(g, *gx.shape))]


def _mt_tensors(g, grad=False):
    shapes = [(6, 7), (5,), (2, 3, 3, 3)]
    return [_randn(g, *s, grad=grad) for s in shapes], [_randn(g, *s) for s in shapes]


def _mt_update(rule, lr_mode, lr_grad):
    g = _gen(10)
    ws, gs = _mt_tensors(g, grad=True)
    lrs = [(torch.full_like(w, 0.1) if lr_mode == _hip.LR_ELEMENT else torch.tensor(0.1, device=DEV)).requires_grad_(lr_grad) for w in ws]
    kw = {}
    if rule != _hip.RULE_SGD:
        kw = dict(m=[torch.zeros_like(w) for w in ws], s=[torch.zeros_like(w) for w in ws], bc1=[0.1] * 3, sqrt_bc2=[0.1] * 3)
    outs = hip_ops.mt_update(rule, lr_mode, ws, gs, lrs, **kw)
    grads = torch.autograd.grad(outs, ws + (lrs if lr_grad else []), [torch.ones_like(o) for o in outs])
    hip_ops.filters_after_update([])
    return _flat(outs, grads, kw.get('m'), kw.get('s'))


def _mt_update_nograd():
    g = _gen(11)
    ws, gs = _mt_tensors(g)
    lrs = [torch.tensor(0.1, device=DEV) for _ in ws]
    m, s = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    res = hip_ops.mt_update_nograd(_hip.RULE_ADAM, _hip.LR_SCALAR, ws, gs, lrs, m, s, [0.1] * 3, [0.1] * 3, 0.9, 0.99, 1e-8, True)
    hip_ops.filters_after_update([])
    return _flat(res, ws, m, s)


def _mt_scale():
    g = _gen(12)
    ws, gs = _mt_tensors(g, grad=True)
    gamma = _rand(g, 3, grad=True)
    outs = hip_ops.mt_scale(gamma, ws)
    res = [outs, torch.autograd.grad(outs, [gamma] + ws, gs)]
    res.append(torch.autograd.grad(hip_ops.mt_scale(gamma, ws)[1], [gamma, ws[1]], gs[1]))   # one live output: the compacted gamma
    res += [hip_ops.mt_scale_grads(gamma, ws, gs), hip_ops.mt_mean(ws)]
    hip_ops.filters_after_update([])
    return _flat(res)


def _mt_copy():
    g = _gen(13)
    srcs, dsts = _mt_tensors(g)
    hip_ops.mt_copy(dsts, srcs)
    first = [d.clone() for d in dsts]
    hip_ops.MtCopy(dsts, srcs).run()
    return _flat(first, dsts, hip_ops.mt_clone(srcs))


def _graph_loop_lr_grads():
    g = _gen(14)
    suffix, dirs = _mt_tensors(g)
    rule = types.SimpleNamespace(lr_mode=_hip.LR_SCALAR, names_learning_rates_dict={"w%d" % i: torch.zeros(2) for i in range(3)})
    gl = types.SimpleNamespace(rule=rule, step_out=[{'dir': dirs}], rule_id=_hip.RULE_ADAM, routed=["w0", "w1", "w2"], T=1)
    acc = graph_inner_loop.OuterGradAccumulator(None, {})
    acc.add_lr_grads(gl, 0, suffix)
    return _flat(acc.lr_rows)


def _dain_warp():
    g = _gen(15)
    x, flow, filt = _randn(g, 2, 3, 7, 9, grad=True), (4 * _randn(g, 2, 2, 7, 9)).requires_grad_(), (_randn(g, 2, 16, 7, 9) / 4).requires_grad_()
    out = hip_ops.filter_interpolation(x, flow, filt)
    grads = torch.autograd.grad(out, [x, flow, filt], _randn(g, *out.shape))
    with torch.no_grad():
        into = torch.zeros(2, 5, 7, 9, device=DEV)
        res = hip_ops.filter_interpolation_into(into, 2, x, flow, filt)
    return _flat(out, grads, into, res)


def _dain_projection():
    g = _gen(16)
    flow, wgt = (3 * _randn(g, 2, 2, 7, 9)).requires_grad_(), _rand(g, 2, 1, 7, 9, grad=True)
    out = hip_ops.depth_flow_projection(flow, wgt, 0)
    grads = torch.autograd.grad(out, [flow, wgt], _randn(g, *out.shape))
    return _flat(out, grads, hip_ops.depth_flow_projection(flow.detach(), wgt.detach(), 1))


def _pwc():
    g = _gen(17)
    f1, f2 = _randn(g, 1, 3, 3, 5, grad=True), _randn(g, 1, 3, 3, 5, grad=True)
    res = []
    for slope in (1.0, 0.1):
        out = hip_ops.correlation(f1, f2, 4, slope)
        res += [out, torch.autograd.grad(out, [f1, f2], _randn(g, *out.shape))]
    with torch.no_grad():
        res.append(hip_ops.pwc_warp(_randn(g, 2, 3, 7, 9), 2 * _randn(g, 2, 2, 7, 9), 0.625))
    return _flat(res)


def _dain_net():
    g = _gen(18)
    with torch.no_grad():
        x = _randn(g, 4, 3, 5, 7)
        mean, var = hip_ops.bn_stats(x, 2)
        running = [torch.zeros(3, device=DEV), torch.ones(3, device=DEV)]
        res = [mean, var, hip_ops.bn_apply_relu(x, mean, var, 2, _rand(g, 3), _randn(g, 3)), x]
        res.append(hip_ops.bn_running_update(running, [mean[0].contiguous(), var[0].contiguous()], [1.0, 1.5]))
        res += [running, hip_ops.max_pool2x2(_randn(g, 2, 3, 5, 7)), hip_ops.upnearest2x_add(_randn(g, 2, 3, 3, 5), _randn(g, 2, 3, 6, 10))]
    return _flat(res, _fwd_bwd(hip_ops.add_relu, (2, 3, 5, 7), (2, 3, 5, 7), seed=19))


def _conv_case(name):
    """One forward + backward of a case of tests/test_conv_dispatch_gpu.py (its shapes, its call), nothing compared."""
    c = D.CASES[name]
    T, N, Ci, Co, K = c["T"], c["N"], c["Ci"], c["Co"], c["K"]
    g = _gen(20)
    x = _randn(g, N, Ci, c["H"], c["W"])
    if c["in_slope"] is not None:
        x = torch.relu(x)
    x.requires_grad_(c["need_x"])
    w = (_randn(g, *(((T,) if T else ()) + (Co, Ci, K, K))) / (K * Ci ** 0.5)).requires_grad_()
    b = (0.1 * _randn(g, *(((T,) if T else ()) + (Co,)))).requires_grad_() if c["bias"] else None
    hip_ops.set_weight_gradient_overlap(c["overlap"])
    try:
        if T:
            y = hip_ops.conv_bias_act_tasks(x, w, b, c["stride"], c["pad"], 1, c["slope"], direct=c["direct"], in_slope=c["in_slope"],
                                            defer=c["defer"], out_unit16=c["out_unit16"])
        else:
            y = hip_ops.conv_bias_act(x, w, b, c["stride"], c["pad"], 1, 1, c["slope"], direct=c["direct"], reflect=c["reflect"],
                                      in_slope=c["in_slope"], defer=c["defer"])
        grads = torch.autograd.grad(y, ([x] if c["need_x"] else []) + [w] + ([b] if b is not None else []), _randn(g, *y.shape))
        hip_ops.join_weight_gradients()
        return _flat(y, grads)
    finally:
        hip_ops.set_weight_gradient_overlap(False)


def _conv_unit16_cotangent():
    """tasks-unit16 of the dispatch cases with a unit-major cotangent as well (out_unit16 = 2): the data gradient alone."""
    c = D.CASES["tasks-unit16"]
    g = _gen(21)
    x = _randn(g, c["N"], c["Ci"], c["H"], c["W"], grad=True)
    w, b = _randn(g, c["T"], c["Co"], c["Ci"], 3, 3) / 21, _randn(g, c["T"], c["Co"])
    assert hip_ops.conv3x3_in_unit16_supported((c["N"], c["Co"], c["H"] - 2, c["W"] - 2), w, 0)
    y =hip_ops.conv_bias_act_tasks(x, w, b, 1, 0, 1, 1.0, out_unit16=2)
    return _flat(y, torch.autograd.grad(y, x, hip_ops.tag_layout(_randn(g, *y.shape), hip_ops.UNIT16)))


def _conv_plain_entries():
    """The entry points without autograd: conv3x3, conv3x3_tasks (both forms), conv3x3_wgrad in its direct and its Winograd form."""
    g = _gen(22)
    x, w, b = _randn(g, 1, 8, 16, 64), _randn(g, 64, 8, 3, 3) / 8, _randn(g, 64)
    y = hip_ops.conv3x3(x, w, b, 0, 0.2, 1)
    res = [y, hip_ops.conv3x3(_randn(g, *y.shape), w, None, 1, 1.0, 1)]
    xt, wt, bt = _randn(g, 4, 64, 16, 64), _randn(g, 2, 32, 64, 3, 3) / 24, _randn(g, 2, 32)
    for f2 in (False, True):
        yt = hip_ops.conv3x3_tasks(xt, wt, bt, 0, 0.2, 0, f2=f2)
        res += [yt, hip_ops.conv3x3_tasks(_randn(g, *yt.shape), wt, None, 1, 1.0, 0, f2=f2)]
    res.append(hip_ops.conv3x3_wgrad(_randn(g, 1, 32, 16, 64), _randn(g, 1, 32, 16, 64), 1))
    with _knob(hip_ops, "WGRAD_WINO_MIN_GFLOP", 0.0):
        res.append(hip_ops.conv3x3_wgrad(_randn(g, 2, 32, 16, 16), _randn(g, 2, 32, 16, 16), 1))
        res.append(hip_ops.conv3x3_wgrad_tasks(_randn(g, 2, 20, 37, 53), _randn(g, 2, 70, 37, 53), 2, 1, want_bias=True))
    res.append(hip_ops.conv3x3_wgrad_tasks(_randn(g, 8, 64, 24, 32), _randn(g, 8, 64, 24, 32), 4, 1))
    return _flat(res)


def _conv_pool():
    g = _gen(23)
    x, w, b = _randn(g, 4, 16, 12, 16, grad=True), (_randn(g, 2, 40, 16, 3, 3) / 12).requires_grad_(), _randn(g, 2, 40, grad=True)
    y, pooled = hip_ops.conv_bias_act_tasks_pool(x, w, b, 1, 1, 1, 0.2)
    return _flat(y, pooled, torch.autograd.grad([y, pooled], [x, w, b], [_randn(g, *y.shape), _randn(g, *pooled.shape)]))


def _convk_masked():
    """The masked epilogue of the direct kernel's data gradient, the precise form of its weight gradient, and the filters in one
    many-layer launch per kind."""
    g = _gen(24)
    w = _randn(g, 64, 64, 3, 3) / 24
    _, packed = hip_ops.convk_filters(w, False, True)
    gz, mask = _randn(g, 1, 64, 32, 32), _randn(g, 1, 64, 32, 32)
    res = [packed, hip_ops.convk_tasks_pre(gz, packed, 1, 64, 64, 3, None, 1, 1.0, 1, mask=mask, mask_slope=0.2)]
    res.append(hip_ops.convk_wgrad_tasks(_randn(g, 1, 64, 32, 32), gz, 1, 3, 1, precise=True))
    res.append(hip_ops._filters_multi('convk', [(w, True, True)]))
    res.append(hip_ops._filters_multi('wino', [(w, True, False)]))
    res.append(hip_ops._filters_multi('wino2', [(w, False, True)]))
    res.append(hip_ops.conv3x3_filters(w, True, True, f2=True))
    return _flat(res)


def _reflect_pads():
    return (_fwd_bwd(lambda x: hip_ops.reflect_pad(x, 2), (1, 3, 7, 9), seed=25)
            + _both_outputs(lambda x: hip_ops.reflect_pad_with_skip(x, 2), (1, 3, 7, 9), seed=26))


def _upsample():
    return (_fwd_bwd(lambda x: hip_ops.upsample_bilinear2x(x, True), (2, 7, 5, 9), seed=27)
            + _fwd_bwd(lambda x: hip_ops.upsample_bilinear2x(x, False, 0.2), (2, 7, 5, 9), seed=28)
            + _fwd_bwd(lambda x: hip_ops.upsample_bilinear2x_window(x, (24, 32), (2, 3), (6, 8, 20, 30), True), (1, 3, 16, 20), seed=29)
            + _fwd_bwd(lambda x: hip_ops.mask_grad(x, 0.2), (2, 3, 5, 7), seed=30))


def _channel_attention(N, T, C, Cr, H, W):
    shapes = [(N, C, H, W), (N, C, H, W), (T, Cr, C, 1, 1), (T, Cr), (T, C, Cr, 1, 1), (T, C)]
    return _fwd_bwd(hip_ops.channel_attention_residual, *shapes, seed=31)


def _adacof(grads):
    """N = 1, C = 3, F = 3, dilation 1, 5x7 outputs (the frame [1,3,7,9]); `grads`: which of w, a, b require grad (the others' gradient
    pointers go as NULL)."""
    g = _gen(33)
    x = _rand(g, 1, 3, 7, 9)
    w, a, b = (_randn(g, 1, 9, 5, 7, grad=need) for need in grads)
    out = hip_ops.adacof(x, w, a, b)
    return _flat(out, torch.autograd.grad(out, [t for t, need in zip((w, a, b), grads) if need], _randn(g, *out.shape)))


def _charbonnier(fn):
    return _fwd_bwd(fn, (2, 3, 33, 35), (2, 3, 33, 35), seed=32)


CASES = {
    "voxelwarp": lambda: _warp_once(hip_ops.voxel_warp_blend, *VOX, False),
    "voxelwarp+g_frames": lambda: _warp_once(hip_ops.voxel_warp_blend, *VOX, True),
    "voxelwarp-twice": lambda: _warp_twice(hip_ops._VoxelWarpTwice.apply, *VOX, True),
    "voxelwarp-twice-d_x3": lambda: _warp_twice(hip_ops._VoxelWarpTwice.apply, *VOX, False),
    "flowwarp": lambda: _warp_once(hip_ops.flow_warp, *FLOW, False),
    "flowwarp-twice": lambda: _warp_twice(hip_ops._FlowWarpTwice.apply, *FLOW, True),
    "flowwarp-twice-d_flow": lambda: _warp_twice(hip_ops._FlowWarpTwice.apply, *FLOW, False),
    "sepconv-fp32": lambda: _sepconv_once(False, False),
    "sepconv-fp32+gI": lambda: _sepconv_once(False, True),
    "sepconv-fp32-twice": lambda: _sepconv_twice(False),
    "sepconv-frames8": lambda: _sepconv_once(True, False),
    "sepconv-frames8+gI": lambda: _sepconv_once(True, True),
    "sepconv-frames8-twice": lambda: _sepconv_twice(True),
    "sepconv-pair": lambda: _sepconv_pair(),
    "sepconv-pair-two-launches": lambda: _sepconv_pair(one_launch=False),
    "sepconv-pair-strided": lambda: _sepconv_pair(frames8=False),
    "l1": lambda: _loss(hip_ops.l1_loss),
    "l1-per-sample": lambda: _loss(hip_ops.l1_loss_per_sample),
    "mse": lambda: _loss(hip_ops.mse_loss),
    "mse-per-sample": lambda: _loss(hip_ops.mse_loss_per_sample),
    "ssim": lambda: _loss(hip_ops.ssim_loss),
    "ssim-per-sample": lambda: _loss(hip_ops.ssim_loss_per_sample),
    "msssim": lambda: _loss(hip_ops.msssim, normalize=True),
    "msssim-per-sample": lambda: _loss(hip_ops.msssim_per_sample, normalize=True),
    "msssim-255": lambda: _loss(hip_ops.msssim, val_range=255, normalize=True),
    "msssim-255-per-sample": lambda: _loss(hip_ops.msssim_per_sample, val_range=255, normalize=True),
    "lap": lambda: _loss(hip_ops.lap_loss),
    "lap-per-sample": lambda: _loss(hip_ops.lap_loss_per_sample),
    "census": lambda: _loss(hip_ops.census_loss),
    "census-per-sample": lambda: _loss(hip_ops.census_loss_per_sample),
    "charbonnier": lambda: _charbonnier(hip_ops.charbonnier_loss),
    "charbonnier-per-sample": lambda: _charbonnier(hip_ops.charbonnier_loss_per_sample),
    "psnr_ssim": lambda: _metric(hip_ops.psnr_ssim),
    "psnr_ssim+sq": lambda: _metric(lambda a, b: hip_ops.psnr_ssim(a, b, want_sq_sum=True)),
    "msssim_metric": lambda: _metric(hip_ops.msssim_metric),
    "frames_to_u8": lambda: _flat(hip_ops.frames_to_u8(_rand(_gen(6), 2, 3, 33, 35))),
    "avgpool": lambda: _fwd_bwd(hip_ops.avg_pool2x2, (1, 5, 7, 9)),
    "avgpool-second-order": _avgpool_second_order,
    "avgpool-and-skip": lambda: _both_outputs(lambda x: hip_ops.avg_pool2x2_and_skip(x, 0.2), (2, 5, 12, 16)),
    "pixel_shuffle": lambda: (_fwd_bwd(lambda x: hip_ops.pixel_shuffle(x, 0.5), (2, 3, 16, 24))
                              + _fwd_bwd(lambda x: hip_ops.pixel_shuffle(x, 2), (2, 12, 8, 12))),
    "sub_mean": lambda: _both_outputs(hip_ops.sub_mean, (2, 3, 37, 45)),
    "mt_update-sgd": lambda: _mt_update(_hip.RULE_SGD, _hip.LR_SCALAR, True),
    "mt_update-adam-element": lambda: _mt_update(_hip.RULE_ADAM, _hip.LR_ELEMENT, True),
    "mt_update-nograd": _mt_update_nograd,
    "mt_scale": _mt_scale,
    "mt_copy": _mt_copy,
    "graph-loop-lr-grads": _graph_loop_lr_grads,
    "dain-warp": _dain_warp,
    "dain-projection": _dain_projection,
    "pwc": _pwc,
    "dain-net": _dain_net,
    "conv-plain-entries": _conv_plain_entries,
    "conv-pool": _conv_pool,
    "conv-unit16-cotangent": _conv_unit16_cotangent,
    "convk-masked-precise-multi": _convk_masked,
    "reflect_pad": _reflect_pads,
    "upsample2x": _upsample,
    "channel-attention-fused": lambda: _channel_attention(3, 3, 16, 2, 5, 7),
    "channel-attention-three-launches": lambda: _channel_attention(2, 1, 320, 20, 8, 8),
    "adacof": lambda: _adacof((True, True, True)),
    "adacof-null-grads": lambda: _adacof((True, False, False)),
}
CASES.update({"conv-" + name: (lambda name=name: _conv_case(name)) for name in D.CASES})


def run_case(name):
    """[[timer name, [checked symbols], nbytes, flops], ...] of one case, from an empty filter store."""
    hip_ops.filters_after_update([])
    hip_ops._pack_plans.clear()
    torch.cuda.synchronize()
    with record_launches() as rec:
        CASES[name]()
        torch.cuda.synchronize()
    return [[n, what, nbytes, flops] for n, nbytes, flops, what in rec.launches]


def record(path):
    """The recording mode: every case once, written to `path` (a case the machine cannot run is left out and named)."""
    manifest = {}
    for name in CASES:
        try:
            manifest[name] = run_case(name)
        except pytest.skip.Exception as exc:
            print("skipped %s: %s" % (name, exc))
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(manifest.items())) + "\n}\n")
    names = sorted({launch[0] for launches in manifest.values() for launch in launches})
    print("%d cases, %d launches, %d timer names: %s" % (len(manifest), sum(map(len, manifest.values())), len(names), " ".join(names)))


@pytest.fixture(scope="module")
def manifest():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_names_every_case(manifest):
    assert sorted(manifest) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launches_are_the_recorded_ones(name, manifest):
    got = run_case(name)
    want = manifest[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: launch %d is %r, recorded %r" % (name, i, g, w)
    assert len(got) == len(want), "%s: %d launches, recorded %d: %r" % (name, len(got), len(want), [g[0] for g in got])


if __name__ == "__main__":
    record(sys.argv[1])
