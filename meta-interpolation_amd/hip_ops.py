"""torch.autograd wrappers over the non-sepconv entry points of libsavfi_hip.so.

Every function here launches a hand-written gfx950 kernel through the C ABI (include/savfi_hip.h)
on torch's current stream.  Device tensors only -- there is no CPU or eager-PyTorch fallback.
"""
import collections
import contextlib
import functools
import ctypes
import os
import threading

import torch
from torch.autograd.function import once_differentiable

from . import _hip

# Set by the meta system for the duration of a forward with --second_order: ops whose hand-written backward
# is not itself differentiable switch to composed device ops (losses) or refuse (voxel warp) instead of
# silently dropping second-order terms.  (FunctionSepconv does drop them, exactly like the reference: SURVEY.md
# section 0, fact 9; --sepconv_second_order 1 makes the SepConv plugin use FunctionSepconvTwice in such passes, and
# --warp_second_order 1 makes voxel_warp_blend / flow_warp use the fused twice-differentiable _VoxelWarpTwice / _FlowWarpTwice.)
# Per THREAD (tasks may be adapted on concurrent threads; two systems in one process must not flip each other's ops):
# worker threads get the caller's value through meta_learning_system._run_tasks.
_PASS = threading.local()


def set_double_backward(value):
    _PASS.double_backward = bool(value)


def double_backward():
    return getattr(_PASS, 'double_backward', False)


# --------------------------------------------------------------------------------------------
# VoxelFlow warp + blend            (reference: voxelflow/core/models/voxel_flow.py:471-509)
# --------------------------------------------------------------------------------------------
def _voxelwarp_fwd(frames, x3):
    """savfi_voxelwarp_fwd_f32: the one forward launch of _VoxelWarp and _VoxelWarpTwice."""
    _hip.require_cuda(frames, x3)
    B, six, H, W = frames.shape
    assert six == 6 and x3.shape == (B, 3, H, W)
    out = torch.empty((B, 3, H, W), dtype=frames.dtype, device=frames.device)
    _hip.call("voxelwarp_fwd", "savfi_voxelwarp_fwd_f32", frames, x3, out, B, H, W, nbytes=4 * 12 * B * H * W)
    return out


def _voxelwarp_grads(frames, x3, gO, want_frames):
    """savfi_voxelwarp_bwd_f32: the one first-order gradient launch of _VoxelWarp and _VoxelWarpGrad -> (g_x3, g_frames or None)."""
    B, _, H, W = frames.shape
    gO = gO.contiguous()
    _hip.require_cuda(gO)
    g_x3 = torch.empty_like(x3)
    g_fr = torch.zeros_like(frames) if want_frames else None
    _hip.call("voxelwarp_bwd", "savfi_voxelwarp_bwd_f32", frames, x3, gO, g_x3, g_fr, B, H, W, nbytes=4 * 15 * B * H * W)
    return g_x3, g_fr


class _VoxelWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames, x3):
        out = _voxelwarp_fwd(frames, x3)
        ctx.save_for_backward(frames, x3)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gO):
        frames, x3 = ctx.saved_tensors
        need_f, need_x = ctx.needs_input_grad
        g_x3, g_fr = _voxelwarp_grads(frames, x3, gO, need_f)
        return g_fr, (g_x3 if need_x else None)


def _bilinear_border(img, cx, cy):
    """F.grid_sample(img, stack(cx, cy), bilinear, padding_mode='border', align_corners=True) written with gathers (ATen
    GridSampler.h: unnormalise, clip the coordinate, four corners): differentiable in `img`, `cx`, `cy` to any order --
    ATen's grid_sampler_2d_backward has no derivative, so the fused op and F.grid_sample alike stop at first order.
    The clip has ATen's slope (clip_coordinates_set_grad), which is also the fused kernel's: zero for s <= 0 and s >= size - 1, the
    bounds included, where clamp() alone would pass the gradient of a coordinate that sits exactly on a bound.  Inside the open interval
    the coordinate itself goes on, so values and derivatives of every order there are what clamp() gave."""
    N, C, H, W = img.shape

    def clip(s, size):
        return torch.where((s > 0) & (s < size - 1), s, s.detach().clamp(0, size - 1))

    ix = clip((cx + 1.0) * 0.5 * (W - 1), W)
    iy = clip((cy + 1.0) * 0.5 * (H - 1), H)
    x0, y0 = ix.detach().floor(), iy.detach().floor()
    fx, fy = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
    x0i, y0i = x0.long().clamp(0, W - 1), y0.long().clamp(0, H - 1)
    x1i, y1i = (x0i + 1).clamp(max=W - 1), (y0i + 1).clamp(max=H - 1)
    flat = img.reshape(N, C, H * W)

    def corner(yi, xi):
        return flat.gather(2, (yi * W + xi).reshape(N, 1, H * W).expand(N, C, H * W)).reshape(N, C, H, W)

    top = corner(y0i, x0i) * (1 - fx) + corner(y0i, x1i) * fx
    bot = corner(y1i, x0i) * (1 - fx) + corner(y1i, x1i) * fx
    return top * (1 - fy) + bot * fy


def _voxel_warp_composed(frames, x3):
    """The VoxelFlow tail (voxelflow/core/models/voxel_flow.py:471-507, syn_type 'inter') from differentiable ATen ops: what
    --second_order takes (set_double_backward(True)), like pixel shuffle / up-sampling / the losses."""
    B, _, H, W = frames.shape
    gx = torch.linspace(-1.0, 1.0, W, device=frames.device, dtype=frames.dtype).view(1, 1, W).expand(B, H, W)
    gy = torch.linspace(-1.0, 1.0, H, device=frames.device, dtype=frames.dtype).view(1, H, 1).expand(B, H, W)
    fx, fy = 0.5 * x3[:, 0], 0.5 * x3[:, 1]
    o1 = _bilinear_border(frames[:, 0:3], gx - fx, gy - fy)
    o2 = _bilinear_border(frames[:, 3:6], gx + fx, gy + fy)
    mask = (0.5 * (1.0 + x3[:, 2:3])).expand(B, 3, H, W)
    return mask * o1 + (1.0 - mask) * o2


class _VoxelWarpGrad(torch.autograd.Function):
    """(frames, x3, gO) -> g_x3: the backward of _VoxelWarpTwice as a function of its own, through the launch _VoxelWarp.backward
    runs (_voxelwarp_grads).  Its backward is savfi_voxelwarp_bwd2_f32 (csrc/voxelwarp.hip) and is once differentiable: a third derivative raises."""

    @staticmethod
    def forward(ctx, frames, x3, gO):
        gO = gO.contiguous()
        g_x3, _ = _voxelwarp_grads(frames, x3, gO, False)
        ctx.save_for_backward(frames, x3, gO)
        return g_x3

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        frames, x3, gO = ctx.saved_tensors
        B, _, H, W = frames.shape
        _, need_x, need_g = ctx.needs_input_grad
        if not (need_x or need_g):
            return None, None, None
        v = v.contiguous()
        _hip.require_cuda(v)
        d_x3 = torch.empty_like(x3) if need_x else None
        d_gO = torch.empty_like(gO) if need_g else None
        _hip.call("voxelwarp_bwd2", "savfi_voxelwarp_bwd2_f32", frames, x3, gO, v, d_gO, d_x3, B, H, W,
                  nbytes=voxel_warp_bwd2_bytes(B, H, W, need_g, need_x))
        return None, d_x3, d_gO


def voxel_warp_bwd2_bytes(B, H, W, want_gO=True, want_x3=True):
    """HBM bytes of savfi_voxelwarp_bwd2_f32 if every operand is read / written exactly once: frames (6), x3, gO, v (3 each) and 3
    floats per requested output"""
    return 4 * B * H * W * (15 + 3 * int(want_gO) + 3 * int(want_x3))


class _VoxelWarpTwice(torch.autograd.Function):
    """_VoxelWarp for frames WITHOUT gradient, twice differentiable in x3 (--warp_second_order 1).  The forward and the first-order
    gradient are the launches of _VoxelWarp (_voxelwarp_fwd, _voxelwarp_grads): same bits.  The backward is itself an autograd.Function (_VoxelWarpGrad), so under
    create_graph=True g_x3 carries a graph and the second-order terms of MAML reach the outer gradient through savfi_voxelwarp_bwd2_f32.
    Frames that require grad are refused: the second-order terms of g_frames are not built, and a graph-less g_frames would drop them
    silently."""

    @staticmethod
    def forward(ctx, frames, x3):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("_VoxelWarpTwice: the frames require grad, and the second-order terms of their gradient are not "
                                      "implemented (they would be dropped silently); the composed op differentiates them")
        out = _voxelwarp_fwd(frames, x3)
        ctx.save_for_backward(frames, x3)
        return out

    @staticmethod
    def backward(ctx, gO):
        frames, x3 = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        return None, _VoxelWarpGrad.apply(frames, x3, gO)


def set_warp_second_order(value):
    """--warp_second_order 1: in second-order passes (double_backward()) the two warps are the fused twice-differentiable ops.  Per thread,
    like set_double_backward."""
    _PASS.warp_second_order = bool(value)


def warp_second_order():
    return getattr(_PASS, 'warp_second_order', False)


def voxel_warp_blend(frames, x3):
    """frames [B,6,H,W] (I0|I1), x3 [B,3,H,W] = tanh(conv4) -> interpolated frame [B,3,H,W]."""
    if double_backward():
        if warp_second_order() and x3.is_cuda:
            return _VoxelWarpTwice.apply(frames.contiguous(), x3.contiguous())
        return _voxel_warp_composed(frames, x3)
    return _VoxelWarp.apply(frames.contiguous(), x3.contiguous())


# --------------------------------------------------------------------------------------------
# 2x2 average pooling          (reference: sepconv/model.py:176-187, rrin/unet.py:146, superslomo/model.py:66)
# --------------------------------------------------------------------------------------------
def _avgpool2x2_fwd_launch(x):
    """savfi_avgpool2x2_fwd_f32 on a contiguous device map, no autograd"""
    N, C, H, W = x.shape
    out = torch.empty((N, C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    _hip.call("avgpool2x2_fwd", "savfi_avgpool2x2_fwd_f32", x, out, N * C, H, W, nbytes=4 * N * C * (H * W + (H // 2) * (W // 2)))
    return out


class _AvgPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _hip.require_cuda(x)
        ctx.hw = tuple(x.shape[2:])
        return _avgpool2x2_fwd_launch(x)

    @staticmethod
    def backward(ctx, g):
        # linear op: its adjoint goes through a Function too, so double-backward keeps working
        return _AvgPool2x2Adjoint.apply(g, ctx.hw)


class _AvgPool2x2Adjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, hw):
        g = g.contiguous()
        _hip.require_cuda(g)
        N, C = g.shape[:2]
        H, W = hw
        gin = torch.empty((N, C, H, W), dtype=g.dtype, device=g.device)
        _hip.call("avgpool2x2_bwd", "savfi_avgpool2x2_bwd_f32", g, gin, N * C, H, W, nbytes=4 * N * C * (H * W + (H // 2) * (W // 2)))
        return gin

    @staticmethod
    def backward(ctx, gg):
        return _AvgPool2x2.apply(gg.contiguous()), None


def _avgpool2x2_skip_adjoint(g_pool, g_skip, x, in_slope):
    """gin = (pool^T(g_pool) + g_skip) * (x > 0 ? 1 : in_slope): the one backward pass of "pool AND keep" (savfi_avgpool2x2_bwd_fused_f32);
    either cotangent may be None, in_slope None = no activation derivative"""
    N, C, H, W = x.shape
    g_pool = None if g_pool is None else g_pool.contiguous()
    g_skip = None if g_skip is None else g_skip.contiguous()
    gin = torch.empty_like(x)
    _hip.call("avgpool2x2_bwd", "savfi_avgpool2x2_bwd_fused_f32", g_pool, g_skip, None if in_slope is None else x,
              1.0 if in_slope is None else float(in_slope), gin, N * C, H, W,
              nbytes=4 * N * C * (H * W * (2 + (g_skip is not None)) + (H // 2) * (W // 2)))
    return gin


class _AvgPool2x2AndSkip(torch.autograd.Function):
    """(pool(x), x): an encoder block's activated output feeds the pooling and a skip connection.  backward: ONE pass
    gin = (pool^T(g_pool) + g_skip) * (x > 0 ? 1 : in_slope) -- the pooling's adjoint, autograd's accumulation of the two consumers'
    cotangents and the producer's deferred activation derivative (conv_bias_act `defer`).  First-order passes only."""

    @staticmethod
    def forward(ctx, x, in_slope):
        _hip.require_cuda(x)
        out = _avgpool2x2_fwd_launch(x)
        ctx.in_slope = in_slope
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        return out, x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pool, g_skip):
        if g_pool is None and g_skip is None:
            return None, None
        x, = ctx.saved_tensors
        return _avgpool2x2_skip_adjoint(g_pool, g_skip, x, ctx.in_slope), None


def avg_pool2x2_and_skip(x, in_slope=None):
    """(avg_pool2x2(x), x) with ONE element-wise pass in backward (see _AvgPool2x2AndSkip); in_slope: x is the activated output of a
    fused convolution that left its activation derivative to this op.  GPU float32 [N,C,H>=2,W>=2] tensors in first-order passes; anything
    else takes the plain ops (with the derivative as an identity node)."""
    if (x.is_cuda and x.dim() == 4 and x.shape[2] >= 2 and x.shape[3] >= 2 and x.dtype == torch.float32 and not double_backward()
            and torch.is_grad_enabled()):
        return _AvgPool2x2AndSkip.apply(x.contiguous(), None if in_slope is None else float(in_slope))
    if in_slope is not None:
        x = mask_grad(x, in_slope)
    return avg_pool2x2(x), x


def avg_pool2x2(x):
    """F.avg_pool2d(x, 2) == nn.AvgPool2d(2, 2): [N,C,H,W] -> [N,C,H//2,W//2]; plain ATen on CPU tensors (host-logic tests)."""
    if not x.is_cuda or x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2 or x.dtype != torch.float32:
        return torch.nn.functional.avg_pool2d(x, 2)
    return _AvgPool2x2.apply(x.contiguous())


class AvgPool2x2(torch.nn.Module):
    """Parameter-free stand-in for torch.nn.AvgPool2d(kernel_size=2, stride=2)."""

    def forward(self, x):
        return avg_pool2x2(x)

    def extra_repr(self):
        return 'kernel_size=2, stride=2'


# --------------------------------------------------------------------------------------------
# Backward warp by a pixel-unit flow    (reference: superslomo/model.py:231-307, rrin/model.py:8-20)
# --------------------------------------------------------------------------------------------
def _flowwarp_fwd(img, flow):
    """savfi_flowwarp_fwd_f32: the one forward launch of _FlowWarp and _FlowWarpTwice (which check their arguments themselves)."""
    N, C, H, W = img.shape
    out = torch.empty_like(img)
    _hip.call("flowwarp_fwd", "savfi_flowwarp_fwd_f32", img, flow, out, N, C, H, W, nbytes=4 * N * H * W * (2 * C + 2))
    return out


def _flowwarp_grad(img, flow, gout):
    """savfi_flowwarp_bwd_f32: the one first-order gradient launch of _FlowWarp and _FlowWarpGrad -> gflow (gout contiguous)."""
    N, C, H, W = img.shape
    _hip.require_cuda(gout)
    gflow = torch.empty_like(flow)
    _hip.call("flowwarp_bwd", "savfi_flowwarp_bwd_f32", img, flow, gout, gflow, N, C, H, W, nbytes=4 * N * H * W * (2 * C + 4))
    return gflow


class _FlowWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, flow):
        _hip.require_cuda(img, flow)
        N, C, H, W = img.shape
        assert flow.shape == (N, 2, H, W), (img.shape, flow.shape)
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("flow_warp differentiates w.r.t. the flow only: on the reference's path the warped "
                                      "images are network inputs (superslomo/model.py:600-624, rrin/model.py:99-100)")
        out = _flowwarp_fwd(img, flow)
        ctx.save_for_backward(img, flow)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        img, flow = ctx.saved_tensors
        return None, _flowwarp_grad(img, flow, gout.contiguous())


class _FlowWarpGrad(torch.autograd.Function):
    """(img, flow, gout) -> gflow: the backward of _FlowWarpTwice as a function of its own, through the launch _FlowWarp.backward
    runs (_flowwarp_grad).  Its backward is savfi_flowwarp_bwd2_f32 (csrc/flowwarp.hip) and is once differentiable: a third derivative
    raises."""

    @staticmethod
    def forward(ctx, img, flow, gout):
        gout = gout.contiguous()
        gflow = _flowwarp_grad(img, flow, gout)
        ctx.save_for_backward(img, flow, gout)
        return gflow

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        img, flow, gout = ctx.saved_tensors
        N, C, H, W = img.shape
        _, need_f, need_g = ctx.needs_input_grad
        if not (need_f or need_g):
            return None, None, None
        v = v.contiguous()
        _hip.require_cuda(v)
        d_flow = torch.empty_like(flow) if need_f else None
        d_gout = torch.empty_like(gout) if need_g else None
        _hip.call("flowwarp_bwd2", "savfi_flowwarp_bwd2_f32", img, flow, gout, v, d_gout, d_flow, N, C, H, W,
                  nbytes=flow_warp_bwd2_bytes(N, C, H, W, need_g, need_f))
        return None, d_flow, d_gout


def flow_warp_bwd2_bytes(N, C, H, W, want_gout=True, want_flow=True):
    """HBM bytes of savfi_flowwarp_bwd2_f32 if every operand is read / written exactly once: img and gout (C each), flow and v (2
    each), C floats of d_gout and 2 of d_flow where requested"""
    return 4 * N * H * W * (2 * C + 4 + C * int(want_gout) + 2 * int(want_flow))


class _FlowWarpTwice(torch.autograd.Function):
    """_FlowWarp, twice differentiable in the flow (--warp_second_order 1).  The forward and the first-order gradient are the launches
    of _FlowWarp (_flowwarp_fwd, _flowwarp_grad): same bits.  The backward is itself an autograd.Function (_FlowWarpGrad), so under create_graph=True gflow carries
    a graph and the second-order terms of MAML reach the outer gradient through savfi_flowwarp_bwd2_f32.  An image that requires grad is
    refused, as _FlowWarp refuses it."""

    @staticmethod
    def forward(ctx, img, flow):
        _hip.require_cuda(img, flow)
        N, C, H, W = img.shape
        assert flow.shape == (N, 2, H, W), (img.shape, flow.shape)
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("flow_warp differentiates w.r.t. the flow only: on the reference's path the warped "
                                      "images are network inputs (superslomo/model.py:600-624, rrin/model.py:99-100)")
        out = _flowwarp_fwd(img, flow)
        ctx.save_for_backward(img, flow)
        return out

    @staticmethod
    def backward(ctx, gout):
        img, flow = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        return None, _FlowWarpGrad.apply(img, flow, gout)


def flow_warp(img, flow):
    """img [N,C,H,W] sampled at (x + u - 0.5, y + v - 0.5), flow = (u, v) [N,2,H,W] in pixels: exactly what
    backWarp / warp of the reference compute (their normalisation under grid_sample's align_corners=False)."""
    if double_backward() and warp_second_order() and flow.is_cuda:
        return _FlowWarpTwice.apply(img.contiguous(), flow.contiguous())
    return _FlowWarp.apply(img.contiguous(), flow.contiguous())


# --------------------------------------------------------------------------------------------
# Pixel (un)shuffle                                   (reference: model_utils.py:202-217)
# --------------------------------------------------------------------------------------------
def _launch_shuffle(x, r, down):
    _hip.require_cuda(x)
    B, C, H, W = x.shape
    if down:
        assert H % r == 0 and W % r == 0
        out = torch.empty((B, C * r * r, H // r, W // r), dtype=x.dtype, device=x.device)
        _hip.call("pixel_unshuffle", "savfi_pixel_unshuffle_f32", x, out, B, C, H, W, r, nbytes=8 * x.numel())
    else:
        assert C % (r * r) == 0
        out = torch.empty((B, C // (r * r), H * r, W * r), dtype=x.dtype, device=x.device)
        _hip.call("pixel_shuffle", "savfi_pixel_shuffle_f32", x, out, B, C, H, W, r, nbytes=8 * x.numel())
    return out


class _PixelShuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, down):
        ctx.r, ctx.down = r, down
        return _launch_shuffle(x.contiguous(), r, down)

    @staticmethod
    def backward(ctx, g):
        # the permutation's adjoint is its inverse; applied through the Function so that it stays
        # differentiable (second-order MAML through CAIN)
        return _PixelShuffle.apply(g, ctx.r, not ctx.down), None, None


def pixel_shuffle(input, scale_factor):
    """Same call surface as the reference's pixel_shuffle: scale<1 packs space into channels
    (block 1/scale), scale>=1 unpacks."""
    if scale_factor >= 1:
        return _PixelShuffle.apply(input, int(scale_factor), False)
    return _PixelShuffle.apply(input, int(round(1 / scale_factor)), True)


# --------------------------------------------------------------------------------------------
# Per-plane mean removal                              (reference: model_utils.py:11-15 sub_mean)
# --------------------------------------------------------------------------------------------
class _SubMean(torch.autograd.Function):
    """x [N,C,H,W] -> (x - mean_hw(x), mean_hw(x) [N,C,1,1]) on savfi_sub_mean_f32: two launches that add in a fixed order and need
    no cleared memory.  ATen's mean switches to several workgroups per output plus a hipMemsetAsync'ed semaphore array on large
    frames, and a memset node of a captured hipGraph only clears in the first replay on ROCm 7.2 (csrc/submean.hip)."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _hip.require_cuda(x)
        N, C, H, W = x.shape
        ctx.hw, ctx.shape = H * W, tuple(x.shape)
        out = torch.empty_like(x)
        mean = torch.empty((N, C, 1, 1), dtype=x.dtype, device=x.device)
        ws = torch.empty(_workspace_floats("savfi_sub_mean_workspace_floats", N * C, H * W), dtype=x.dtype, device=x.device)
        _hip.call("sub_mean", "savfi_sub_mean_f32", x, out, mean, ws, N * C, H * W, nbytes=12 * x.numel())
        return out, mean

    @staticmethod
    def backward(ctx, g_out, g_mean):
        # out = x - m(x), mean = m(x), m linear and self-adjoint up to 1/hw: gx = g_out - m(g_out) + g_mean / hw  (differentiable:
        # the same Function and ATen arithmetic)
        gx = None
        if g_out is not None:
            gx = _SubMean.apply(g_out)[0]
        if g_mean is not None:
            share = (g_mean / ctx.hw).expand(ctx.shape)
            gx = share if gx is None else gx + share
        return gx


def sub_mean(x):
    """(x - mean, mean): the per-channel spatial mean removed (reference model_utils.py:11-15)."""
    return _SubMean.apply(x)


# --------------------------------------------------------------------------------------------
# Fused multi-tensor inner-loop update            (reference: inner_loop_optimizers.py)
# --------------------------------------------------------------------------------------------
class _MtUpdate(torch.autograd.Function):
    """(w_1..w_n, lr_1..lr_n) -> (w'_1..w'_n); g, moments and hyper-parameters ride in `spec`.

    First-order MAML semantics: the gradients g are constants.  d w'/d w = I, and d w'/d lr is the
    per-element update direction, saved by the forward kernel when some lr requires grad.
    """

    @staticmethod
    def forward(ctx, spec, *tensors):
        ctx.set_materialize_grads(False)   # unused outputs (e.g. SepConv's subnet copies) stay None
        n = spec["n"]
        ws, lrs = tensors[:n], tensors[n:]
        gs = spec["grads"]
        rule, lr_mode = spec["rule"], spec["lr_mode"]
        outs = [torch.empty_like(w) for w in ws]
        need_lr = any(ctx.needs_input_grad[1 + n + i] for i in range(n))
        save_dir = need_lr and rule != _hip.RULE_SGD
        coefs = [torch.empty_like(w) for w in ws] if save_dir else None
        ms, ss = spec.get("m"), spec.get("s")
        _launch_mt_update(rule, lr_mode, ws, gs, lrs, ms, ss, outs, coefs, spec.get("bc1"), spec.get("sqrt_bc2"),
                          spec["beta1"], spec["beta2"], spec["eps"])
        numel = [w.numel() for w in ws]
        ctx.n, ctx.lr_mode, ctx.numel = n, lr_mode, numel
        ctx.lr_shapes = [lr.shape for lr in lrs]
        ctx.w_shapes = [w.shape for w in ws]
        if need_lr:
            ctx.dirs = coefs if save_dir else list(gs)
            ctx.dir_scale = 1.0 if save_dir else -1.0
        else:
            ctx.dirs = None
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        n = ctx.n
        g_ws = [g if ctx.needs_input_grad[1 + i] else None for i, g in enumerate(g_outs)]
        g_lrs = [None] * n
        if ctx.dirs is not None:
            idx = [i for i in range(n) if ctx.needs_input_grad[1 + n + i] and g_outs[i] is not None]
            if idx:
                gos = [g_outs[i].contiguous() for i in idx]
                dirs = [ctx.dirs[i] for i in idx]
                dev = gos[0].device
                if ctx.lr_mode == _hip.LR_SCALAR:      # (one zero fill for all of them: 0-dim views of one buffer)
                    dst = list(torch.zeros(len(idx), dtype=torch.float32, device=dev).unbind(0))
                else:
                    dst = [torch.empty_like(go) for go in gos]
                numel = [ctx.numel[i] for i in idx]
                _hip.call("mt_update_bwd", "savfi_mt_update_bwd_f32", ctx.lr_mode, len(idx), _hip.ptr_array(gos), _hip.ptr_array(dirs),
                          _hip.ptr_array(dst), _hip.i64_array(numel), ctx.dir_scale)
                for j, i in enumerate(idx):
                    if ctx.lr_mode == _hip.LR_ELEMENT and tuple(ctx.w_shapes[i]) != tuple(ctx.lr_shapes[i]):
                        g_lrs[i] = dst[j].sum(0)         # weights stacked over tasks, ONE element-wise lr table: add the tasks
                    else:
                        g_lrs[i] = dst[j].reshape(ctx.lr_shapes[i])
        return (None, *g_ws, *g_lrs)


def _launch_mt_update(rule, lr_mode, ws, gs, lrs, ms, ss, outs, coefs, bc1, sqrt_bc2, beta1, beta2, eps):
    """One savfi_mt_update_f32 call.  Weights stacked over tasks ([T, *shape], tasks adapted in lockstep) with an element-wise
    learning-rate table of shape `shape` (Meta-SGD) go in as T entries, one per task slice, that share the lr pointer; with a
    scalar lr (LSLR) a stacked tensor is just a tensor of T x numel elements."""
    if lr_mode == _hip.LR_ELEMENT and any(w.shape != lr.shape for w, lr in zip(ws, lrs)):
        def cut(ts):
            if ts is None:
                return None
            out = []
            for t, w, lr in zip(ts, ws, lrs):
                out.extend([t] if w.shape == lr.shape else list(t.unbind(0)))
            return out
        rep = lambda vals: None if vals is None else [v for v, w, lr in zip(vals, ws, lrs)
                                                      for _ in range(1 if w.shape == lr.shape else w.shape[0])]
        lrs = rep(list(lrs))
        bc1, sqrt_bc2 = rep(bc1), rep(sqrt_bc2)
        ws_, gs, ms, ss, outs, coefs = cut(ws), cut(gs), cut(ms), cut(ss), cut(outs), cut(coefs)
        ws = ws_
    per_el = 12 + (4 if lr_mode == _hip.LR_ELEMENT else 0) + (8 if ms is not None else 0) + (8 if ss is not None else 0) + (4 if coefs is not None else 0)
    _hip.call("mt_update", "savfi_mt_update_f32", rule, lr_mode, len(ws), _hip.ptr_array(ws), _hip.ptr_array(gs), _hip.ptr_array(lrs),
              _hip.ptr_array(ms) if ms is not None else None, _hip.ptr_array(ss) if ss is not None else None,
              _hip.ptr_array(outs), _hip.ptr_array(coefs) if coefs is not None else None,
              _hip.i64_array([w.numel() for w in ws]),
              _hip.f32_array(bc1) if bc1 is not None else None, _hip.f32_array(sqrt_bc2) if sqrt_bc2 is not None else None,
              beta1, beta2, eps, nbytes=per_el * sum(w.numel() for w in ws))


def mt_update(rule, lr_mode, weights, grads, lrs, m=None, s=None, bc1=None, sqrt_bc2=None,
              beta1=0.9, beta2=0.99, eps=1e-8):
    """Fused update of a list of tensors.  `lrs[i]` is a 0-dim tensor (LR_SCALAR) or a tensor shaped
    like weights[i] (LR_ELEMENT).  m / s are updated in place by the kernel.  Returns new tensors.
    The kernel reads every operand as a dense array: strided weights, gradients (a transposed or expanded view) and learning-rate
    tables are made dense here -- the learning rates differentiably; the moments cannot be copied and are refused."""
    n = len(weights)
    if n == 0:
        return []
    dense = lambda ts: [t if t.is_contiguous() else t.contiguous() for t in ts]
    ws, gs, lrs = dense(weights), dense([g.detach() for g in grads]), dense(lrs)
    _hip.require_cuda(*ws, *gs, *lrs)
    for name, mom in (("m", m), ("s", s)):
        if mom is None:
            continue
        if any(not t.is_contiguous() for t in mom):
            raise ValueError("mt_update: the moments `%s` are updated in place and must be contiguous (a dense copy would take the "
                             "update with it)" % name)
        _hip.require_cuda(*mom)
    spec = dict(n=n, rule=rule, lr_mode=lr_mode, grads=gs, m=m, s=s, bc1=bc1,
                sqrt_bc2=sqrt_bc2, beta1=beta1, beta2=beta2, eps=eps)
    outs = list(_MtUpdate.apply(spec, *ws, *lrs))
    filters_after_update(outs)
    return outs


def mt_update_nograd(rule, lr_mode, weights, grads, lrs, m, s, bc1, sqrt_bc2, beta1, beta2, eps, want_coef):
    """The fused update without the autograd wrapper (used inside captured hipGraphs, where the outer gradient
    is assembled by hand): returns (new weights, coef or None) with coef = d w' / d lr per element."""
    outs = [torch.empty_like(w) for w in weights]
    coefs = [torch.empty_like(w) for w in weights] if want_coef else None
    _launch_mt_update(rule, lr_mode, list(weights), list(grads), list(lrs), m, s, outs, coefs, bc1, sqrt_bc2, beta1, beta2, eps)
    filters_after_update(outs)
    return outs, coefs


# --------------------------------------------------------------------------------------------
# L2F: per-tensor mean of gradients, per-tensor attenuation   (meta_learning_system.py:249-268)
# --------------------------------------------------------------------------------------------
def mt_mean(tensors):
    """[t_1..t_n] -> float32[n] of per-tensor means (no autograd: inputs are first-order grads)."""
    ts = [t.detach().contiguous() for t in tensors]
    _hip.require_cuda(*ts)
    out = torch.zeros(len(ts), dtype=torch.float32, device=ts[0].device)
    _hip.call("mt_mean", "savfi_mt_mean_f32", len(ts), _hip.ptr_array(ts), _hip.i64_array([t.numel() for t in ts]), out)
    return out


class _MtScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gamma, *ws):
        ctx.set_materialize_grads(False)
        _hip.require_cuda(gamma, *ws)
        outs = [torch.empty_like(w) for w in ws]
        _hip.call("mt_scale", "savfi_mt_scale_f32", len(ws), _hip.ptr_array(ws), gamma, _hip.ptr_array(outs),
                  _hip.i64_array([w.numel() for w in ws]))
        ctx.save_for_backward(gamma, *ws)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        gamma, *ws = ctx.saved_tensors
        n = len(ws)
        live = [i for i in range(n) if g_outs[i] is not None]
        g_ws = [None] * n
        g_gamma = torch.zeros_like(gamma) if ctx.needs_input_grad[0] else None
        if live:
            # gamma / g_gamma are indexed by tensor position: run the live tensors through a compacted
            # gamma vector and scatter the per-tensor reductions back
            gos = [g_outs[i].contiguous() for i in live]
            wl = [ws[i] for i in live]
            gw_l = [torch.empty_like(ws[i]) if ctx.needs_input_grad[1 + i] else None for i in live]
            full = len(live) == n
            gam_l = gamma if full else gamma[live].contiguous()
            gg_l = None if g_gamma is None else (g_gamma if full else torch.zeros_like(gam_l))
            _hip.call("mt_scale_bwd", "savfi_mt_scale_bwd_f32", len(live), _hip.ptr_array(gos), _hip.ptr_array(wl), gam_l,
                      _hip.ptr_array(gw_l), gg_l, _hip.i64_array([w.numel() for w in wl]))
            for j, i in enumerate(live):
                g_ws[i] = gw_l[j]
            if g_gamma is not None and not full:
                g_gamma[live] = gg_l
        return (g_gamma, *g_ws)


def mt_scale_grads(gamma, weights, g_outs):
    """The backward of mt_scale without autograd (hipGraph loop, where the outer gradient is assembled by hand):
    returns (g_gamma float32[n] = <g_outs[i], weights[i]>, [gamma[i] * g_outs[i]])."""
    ws = [w.detach().contiguous() for w in weights]
    gos = [g.contiguous() for g in g_outs]
    gamma = gamma.detach().contiguous()
    _hip.require_cuda(gamma, *ws, *gos)
    gws = [torch.empty_like(w) for w in ws]
    gg = torch.zeros_like(gamma)
    _hip.call("mt_scale_bwd", "savfi_mt_scale_bwd_f32", len(ws), _hip.ptr_array(gos), _hip.ptr_array(ws), gamma, _hip.ptr_array(gws), gg,
              _hip.i64_array([w.numel() for w in ws]))
    return gg, gws


def mt_scale(gamma, weights):
    """gamma float32[n] (device), weights list of n tensors -> [gamma[i] * weights[i]]."""
    ws = [w if w.is_contiguous() else w.contiguous() for w in weights]
    outs = list(_MtScale.apply(gamma.contiguous(), *ws))
    # L2F's attenuated weights are born together like an update's fast weights: their filters in one launch per kind (config C5: 254
    # single-layer transforms of ~9 us per meta-iteration otherwise); defined further down, with the plan it keeps per list of shapes
    filters_after_update([o.detach() for o in outs])
    return outs


_ONES = {}


def _ones(n, device):
    t = _ONES.get(device)
    if t is None or t.numel() < n:
        t = _ONES[device] = torch.ones(max(int(n), 1024), dtype=torch.float32, device=device)
    return t


def mt_scale_into(gamma, weights, outs):
    """outs[i] <- gamma[i] * weights[i] without autograd, into tensors the caller owns (the static W_0 buffers of the hipGraph loop)."""
    ws = [w.detach() if w.is_contiguous() else w.detach().contiguous() for w in weights]
    outs = [o.detach() for o in outs]
    gamma = gamma.detach().contiguous()
    _hip.require_cuda(gamma, *ws, *outs)
    assert len(ws) == len(outs) and all(o.is_contiguous() and o.numel() == w.numel() and o.dtype == w.dtype for o, w in zip(outs, ws))
    _hip.call("mt_scale", "savfi_mt_scale_f32", len(ws), _hip.ptr_array(ws), gamma, _hip.ptr_array(outs), _hip.i64_array([w.numel() for w in ws]))


def mt_copy(dsts, srcs):
    """dsts[i] <- srcs[i] for lists of float32 CUDA tensors of equal sizes: ceil(n / 48) launches of the multi-tensor scale kernel
    with gamma = 1 (x * 1.0f is x, bit for bit) where torch._foreach_copy_ issues one device memcpy per tensor -- 494 of them per
    task for CAIN, twice per meta-iteration of the hipGraph loop (theta -> W_0, first gradient -> accumulator): ~1000 host-bound
    launches of a 26 ms iteration at 64 x 64."""
    dsts, srcs = list(dsts), list(srcs)
    if not dsts:
        return
    plain = all(d.is_cuda and d.dtype == torch.float32 and s.dtype == torch.float32 and s.device == d.device and d.is_contiguous()
                and d.numel() == s.numel() and d.numel() > 0 for d, s in zip(dsts, srcs))
    if not plain:
        with torch.no_grad():
            torch._foreach_copy_(dsts, [s.view_as(d) if s.shape != d.shape and s.numel() == d.numel() else s for d, s in zip(dsts, srcs)])
        return
    mt_scale_into(_ones(len(dsts), dsts[0].device), srcs, dsts)


class MtCopy:
    """mt_copy between two FIXED lists (the parameters and the static W_0 buffers of a hipGraph set: neither is ever re-allocated):
    the pointer tables are built once -- 2 x 494 ctypes stores per call for CAIN otherwise -- and run() re-checks the addresses."""

    def __init__(self, dsts, srcs):
        # the LIVE objects are kept (a `.detach()` alias would keep pointing at the old storage after `p.data = ...` --
        # module.to() / .float() -- and the address check below could never fail)
        self.dsts, self.srcs = list(dsts), list(srcs)
        self.plain = bool(self.dsts) and all(
            d.is_cuda and d.dtype == torch.float32 and s.dtype == torch.float32 and s.device == d.device and d.is_contiguous()
            and s.is_contiguous() and d.numel() == s.numel() and d.numel() > 0 for d, s in zip(self.dsts, self.srcs))
        if self.plain:
            self.ptrs = [t.data_ptr() for t in self.dsts + self.srcs]
            self.args = (len(self.dsts), _hip.ptr_array(self.srcs), None, _hip.ptr_array(self.dsts),
                         _hip.i64_array([d.numel() for d in self.dsts]))

    def run(self):
        if not self.dsts:
            return
        if not self.plain or any(t.data_ptr() != p for t, p in zip(self.dsts + self.srcs, self.ptrs)):
            with torch.no_grad():
                mt_copy([d.detach() for d in self.dsts], [s.detach() for s in self.srcs])
            return
        n, pw, _, po, numel = self.args
        _hip.call("mt_scale", "savfi_mt_scale_f32", n, pw, _ones(n, self.dsts[0].device), po, numel)


def mt_clone(srcs):
    """[s.clone() for s in srcs] through mt_copy."""
    srcs = list(srcs)
    outs = [torch.empty_like(s, memory_format=torch.contiguous_format) for s in srcs]
    mt_copy(outs, srcs)
    return outs


# --------------------------------------------------------------------------------------------
# Fused L1 / MSE                                                     (loss.py:287-290)
# --------------------------------------------------------------------------------------------
def _row_means_buffers(a, b):
    """(rows, n, result [rows], scratch) of a per-row mean over a, b [rows, ...] (_L1Mse, _Charbonnier: one scratch rule)."""
    _hip.require_cuda(a, b)
    assert a.shape == b.shape
    rows = a.shape[0]
    n = a.numel() // rows
    res = torch.empty(rows, dtype=torch.float32, device=a.device)
    scratch = torch.empty(_workspace_floats("savfi_l1_mse_scratch_floats", rows, n), dtype=torch.float32, device=a.device)
    return rows, n, res, scratch


class _L1Mse(torch.autograd.Function):
    """a, b [rows, ...] -> float32[rows] of per-row mean |a-b| (kind 0) / mean (a-b)^2 (kind 1); deterministic."""

    @staticmethod
    def forward(ctx, kind, a, b):
        rows, n, res, scratch = _row_means_buffers(a, b)
        _hip.call("l1_mse", "savfi_l1_mse_f32", kind, a, b, res, scratch, rows, n)
        ctx.kind = kind
        ctx.save_for_backward(a, b)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = torch.empty_like(a)
        rows = a.shape[0]
        _hip.call("l1_mse_bwd", "savfi_l1_mse_bwd_f32", ctx.kind, a, b, g, ga, rows, a.numel() // rows)
        gb = -ga if ctx.needs_input_grad[2] else None
        return None, ga, gb


def _loss_rows(kind, a, b):
    a, b = a.contiguous(), b.contiguous()
    return _L1Mse.apply(kind, a.reshape(1, -1) if a.dim() < 2 else a, b.reshape(1, -1) if b.dim() < 2 else b)


def l1_loss(a, b):
    """nn.L1Loss(): mean over everything (loss.py:287)."""
    if double_backward():
        return torch.nn.functional.l1_loss(a, b)
    return _L1Mse.apply(0, a.contiguous().reshape(1, -1), b.contiguous().reshape(1, -1)).reshape(())


def mse_loss(a, b):
    if double_backward():
        return torch.nn.functional.mse_loss(a, b)
    return _L1Mse.apply(1, a.contiguous().reshape(1, -1), b.contiguous().reshape(1, -1)).reshape(())


def l1_loss_per_sample(a, b):
    """[N,...] x [N,...] -> [N]: nn.L1Loss() of every sample on its own (tasks adapted in lockstep), one launch."""
    if double_backward():
        return (a - b).abs().flatten(1).mean(1)
    return _loss_rows(0, a, b)


def mse_loss_per_sample(a, b):
    if double_backward():
        return (a - b).pow(2).flatten(1).mean(1)
    return _loss_rows(1, a, b)


# --------------------------------------------------------------------------------------------
# Fused SSIM loss term                      (loss.py:294 -> pytorch_msssim/__init__.py:7-131)
# --------------------------------------------------------------------------------------------
class _SsimLoss(torch.autograd.Function):
    """sr, hr [N,C,H,W] -> float32[N] of (1 - mean SSIM) / 2 per sample (range rule per sample), or float32[1] over the whole
    batch (range rule over the batch); the range class stays on the device (capturable); deterministic."""

    @staticmethod
    def forward(ctx, sr, hr, mode):
        _hip.require_cuda(sr, hr)
        assert sr.dim() == 4 and sr.shape == hr.shape, (sr.shape, hr.shape)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("ssim_loss differentiates w.r.t. the prediction only: on the reference's path the target is a "
                                      "clone of a data frame (loss.py:340)")
        N, C, H, W = sr.shape
        out_rows = 1 if mode == _hip.SSIM_RANGE_BATCH else N
        res = torch.empty(out_rows, dtype=torch.float32, device=sr.device)
        word = torch.empty(out_rows, dtype=torch.int32, device=sr.device)
        scratch = torch.empty(_workspace_floats("savfi_ssim_scratch_floats", N, C, H, W), dtype=torch.float32, device=sr.device)
        _hip.call("ssim_loss", "savfi_ssim_loss_f32", sr, hr, res, word, scratch, N, C, H, W, mode, nbytes=8 * sr.numel())
        ctx.batch = mode == _hip.SSIM_RANGE_BATCH
        ctx.save_for_backward(sr, hr, word)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sr, hr, word = ctx.saved_tensors
        N, C, H, W = sr.shape
        rows, ch = (1, N * C) if ctx.batch else (N, C)      # one loss over the batch: the samples are further channel planes
        g = g.contiguous()
        gsr = torch.empty_like(sr)
        _hip.call("ssim_loss_bwd", "savfi_ssim_loss_bwd_f32", sr, hr, g, word, gsr, rows, ch, H, W, nbytes=12 * sr.numel())
        return gsr, None, None


@functools.lru_cache(maxsize=None)
def _gauss_taps(n, device):
    """The n fp32 taps of pytorch_msssim.gaussian(n, 1.5) on `device` (built once per size and device); n = 11: create_window's."""
    import math
    g = torch.tensor([math.exp(-(x - n // 2) ** 2 / 4.5) for x in range(n)], dtype=torch.float32)
    return (g / g.sum()).to(device)


def _ssim_level(img1, img2, extremes, fixed_cls=None):
    """One level of the composed SSIM / MS-SSIM from differentiable device ops -> (SSIM map, v1, v2) with v1 / v2 the contrast map
    (divided by the caller that wants it): the separable window of min(11, H, W) taps, the dynamic range by the reference's rule from
    `extremes` = (max, min) of the detached first image as device tensors (torch.where: no host read; the caller reduces them, whole
    batch or per sample) or the fixed class `fixed_cls`, the five windowed moments."""
    C = img1.shape[1]
    n = min(11, img1.shape[2], img1.shape[3])
    taps = _gauss_taps(n, img1.device)
    wr, wc = taps.view(1, 1, 1, n).expand(C, 1, 1, n), taps.view(1, 1, n, 1).expand(C, 1, n, 1)

    def win(x):
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, wr, groups=C), wc, groups=C)
    if fixed_cls is None:
        hi, lo = extremes
        one = torch.ones_like(hi)
        L = torch.where(hi > 128, 255 * one, one) + torch.where(lo < -0.5, one, 0 * one)
    else:
        L = (1.0, 2.0, 255.0, 256.0)[fixed_cls]
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu1, mu2 = win(img1), win(img2)
    s1, s2, s12 = win(img1 * img1) - mu1 * mu1, win(img2 * img2) - mu2 * mu2, win(img1 * img2) - mu1 * mu2
    v1, v2 = 2 * s12 + C2, s1 + s2 + C2
    return ((2 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2), v1, v2


def _ssim_composed(sr, hr, per_sample):
    """The same formula from differentiable device ops (what --second_order takes): one _ssim_level with the 11-tap window."""
    d = sr.detach()
    smap, _, _ = _ssim_level(sr, hr, (d.amax((1, 2, 3), keepdim=True), d.amin((1, 2, 3), keepdim=True)) if per_sample else (d.max(), d.min()))
    return (1 - (smap.flatten(1).mean(1) if per_sample else smap.mean())) / 2


def _ssim_args(sr, hr):
    if sr.dim() != 4 or sr.shape != hr.shape or sr.shape[2] < 11 or sr.shape[3] < 11:
        raise ValueError("ssim_loss needs two [N,C,H,W] tensors of one shape with H, W >= 11 (the window is always 11 wide), got %s, %s"
                         % (tuple(sr.shape), tuple(hr.shape)))
    sr, hr = sr.contiguous(), hr.contiguous()
    _hip.require_cuda(sr, hr)
    return sr, hr


def ssim_loss(sr, hr):
    """pytorch_msssim.SSIM() as the reference's Loss constructs and calls it (loss.py:294, :340): (1 - mean SSIM) / 2 over the
    whole batch, dynamic range from the prediction's data.  Gradient for `sr` only."""
    sr, hr = _ssim_args(sr, hr)
    if double_backward():
        return _ssim_composed(sr, hr, False)
    return _SsimLoss.apply(sr, hr, _hip.SSIM_RANGE_BATCH).reshape(())


def ssim_loss_per_sample(sr, hr):
    """[N,C,H,W] x [N,C,H,W] -> [N]: the same term for every sample on its own (tasks adapted in lockstep), one launch."""
    sr, hr = _ssim_args(sr, hr)
    if double_backward():
        return _ssim_composed(sr, hr, True)
    return _SsimLoss.apply(sr, hr, _hip.SSIM_RANGE_PER_ROW)


# --------------------------------------------------------------------------------------------
# PSNR / SSIM evaluation metric and the frame writer          (utils.py:171-204, :276-285)
# --------------------------------------------------------------------------------------------
def psnr_ssim(pred01, tgt01, want_sq_sum=False):
    """pred01, tgt01 [rows,C,H,W] in unit range -> (mse [rows], ssim [rows]) of the 0..255-quantised images, every row on its own:
    what utils.quantize(., 1.) + ((q_p - q_t) / 255)^2 .mean() + utils.ssim(val_range=255) give per pair, in two launches for all
    rows.  PSNR = -10 log10(mse + 1e-8).  No gradient; capturable; deterministic.  want_sq_sum: also the exact integer sums of
    squared differences, int64 [rows] (-1 for a row that holds a NaN)."""
    if pred01.dim() != 4 or pred01.shape != tgt01.shape or pred01.shape[2] < 11 or pred01.shape[3] < 11:
        raise ValueError("psnr_ssim needs two [rows,C,H,W] tensors of one shape with H, W >= 11 (the window is always 11 wide), got %s, %s"
                         % (tuple(pred01.shape), tuple(tgt01.shape)))
    pred01, tgt01 = pred01.detach().contiguous(), tgt01.detach().contiguous()
    _hip.require_cuda(pred01, tgt01)
    rows, C, H, W = pred01.shape
    res = torch.empty((rows, 2), dtype=torch.float32, device=pred01.device)
    sq = torch.empty(rows, dtype=torch.int64, device=pred01.device) if want_sq_sum else None
    scratch = torch.empty(_workspace_floats("savfi_psnr_ssim_scratch_bytes", rows, C, H, W), dtype=torch.uint8, device=pred01.device)
    _hip.call("psnr_ssim", "savfi_psnr_ssim_f32", pred01, tgt01, res, sq, scratch, rows, C, H, W, nbytes=8 * pred01.numel())
    return (res[:, 0], res[:, 1]) + ((sq,) if want_sq_sum else ())


# --------------------------------------------------------------------------------------------
# Multi-scale SSIM                      (pytorch_msssim/__init__.py:78-142; no branch of the reference's Loss uses it)
# --------------------------------------------------------------------------------------------
_MSSSIM_LEVELS = 5
_MSSSIM_VAL_RANGES = {1: 0, 2: 1, 255: 2, 256: 3}


def _fold_dims(img, fold):
    """The (rows, C, H, W) a loss kernel is called with; fold: one value over the batch (MS-SSIM: under a FIXED class) -- the samples
    are further channel planes of one row."""
    N, C, H, W = img.shape
    return (1, N * C, H, W) if fold else (N, C, H, W)


def _msssim_launch(img1, img2, mode, normalize, quantize=False, fold=False):
    """-> (result [rows], scratch): the forward launches of savfi_msssim_f32; `scratch` is what the backward needs."""
    N, C, H, W = _fold_dims(img1, fold)
    res = torch.empty(1 if mode == _hip.SSIM_RANGE_BATCH else N, dtype=torch.float32, device=img1.device)
    scratch = torch.empty(_workspace_floats("savfi_msssim_scratch_bytes", N, C, H, W) // 4, dtype=torch.float32, device=img1.device)
    _hip.call("msssim", "savfi_msssim_f32", img1, img2, res, scratch, N, C, H, W, mode, int(bool(normalize)), int(bool(quantize)),
              nbytes=int(8 * img1.numel() * 1.6))
    return res, scratch


class _MsSsim(torch.autograd.Function):
    """img1, img2 [N,C,H,W] -> float32[N] (every sample an N = 1 call of the reference) or float32[1] (one call on the batch); the range
    classes and the factors of the backward stay on the device (capturable); deterministic."""

    @staticmethod
    def forward(ctx, img1, img2, mode, normalize, fold):
        _hip.require_cuda(img1, img2)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("msssim differentiates w.r.t. the first image (the prediction) only")
        res, scratch = _msssim_launch(img1, img2, mode, normalize, fold=fold)
        ctx.mode, ctx.fold = mode, fold
        ctx.scratch = scratch      # holds the backward's work area too: not a saved tensor (the backward writes into it)
        ctx.save_for_backward(img1, img2)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        img1, img2 = ctx.saved_tensors
        N, C, H, W = _fold_dims(img1, ctx.fold)
        g = g.contiguous()
        g1 = torch.empty_like(img1)
        _hip.call("msssim_bwd", "savfi_msssim_bwd_f32", img1, img2, g, ctx.scratch, g1, N, C, H, W, ctx.mode,
                  nbytes=int(12 * img1.numel() * 1.6))
        return g1, None, None, None, None


def _msssim_composed(img1, img2, per_sample, fixed_cls, normalize):
    """The same value from differentiable device ops (what --second_order takes): one _ssim_level per level, its range decided from
    that level's image, avg_pool2d between the levels."""
    dims = (1, 2, 3) if per_sample else (0, 1, 2, 3)
    ms, mc = [], []
    for _ in range(_MSSSIM_LEVELS):
        d = img1.detach()
        extremes = (d.amax(dims, keepdim=True), d.amin(dims, keepdim=True)) if fixed_cls is None else None
        smap, v1, v2 = _ssim_level(img1, img2, extremes, fixed_cls)
        ms.append(smap.mean(dims))
        mc.append((v1 / v2).mean(dims))
        img1, img2 = torch.nn.functional.avg_pool2d(img1, (2, 2)), torch.nn.functional.avg_pool2d(img2, (2, 2))
    w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    last = (ms[-1] + 1) / 2 if normalize else ms[-1]
    out = last ** (4 * w[-1])
    for s in range(_MSSSIM_LEVELS - 1):
        out = out * ((mc[s] + 1) / 2 if normalize else mc[s]) ** w[s]
    return out


def _msssim_args(img1, img2, val_range, what="msssim"):
    if img1.dim() != 4 or img1.shape != img2.shape or img1.shape[2] < 32 or img1.shape[3] < 32:
        raise ValueError("%s needs two [N,C,H,W] tensors of one shape with H, W >= 32 (five levels, and the reference pools once more "
                         "after the fifth), got %s, %s" % (what, tuple(img1.shape), tuple(img2.shape)))
    if val_range is not None and val_range not in _MSSSIM_VAL_RANGES:
        raise ValueError("%s: val_range must be None (decided from the data on every level) or one of 1, 2, 255, 256, got %r"
                         % (what, val_range))
    img1, img2 = img1.contiguous(), img2.contiguous()
    _hip.require_cuda(img1, img2)
    return img1, img2, None if val_range is None else _MSSSIM_VAL_RANGES[val_range]


def msssim(img1, img2, val_range=None, normalize=False):
    """pytorch_msssim.msssim(img1, img2, size_average=True, val_range=..., normalize=...) as implemented: one value over the whole
    batch, ssim_4 ** (4 w_4) * prod cs_s ** w_s, NaN for a negative base.  Gradient for `img1` only."""
    img1, img2, cls = _msssim_args(img1, img2, val_range)
    if double_backward():
        return _msssim_composed(img1, img2, False, cls, normalize).reshape(())
    if cls is not None:
        return _MsSsim.apply(img1, img2, _hip.SSIM_RANGE_FIXED + cls, normalize, True).reshape(())
    return _MsSsim.apply(img1, img2, _hip.SSIM_RANGE_BATCH, normalize, False).reshape(())


def msssim_per_sample(img1, img2, val_range=None, normalize=False):
    """[N,C,H,W] x [N,C,H,W] -> [N]: msssim of every sample on its own (tasks adapted in lockstep)."""
    img1, img2, cls = _msssim_args(img1, img2, val_range, "msssim_per_sample")
    if double_backward():
        return _msssim_composed(img1, img2, True, cls, normalize)
    return _MsSsim.apply(img1, img2, _hip.SSIM_RANGE_PER_ROW if cls is None else _hip.SSIM_RANGE_FIXED + cls, normalize, False)


def msssim_metric(pred01, tgt01):
    """pred01, tgt01 [rows,C,H,W] in unit range -> [rows]: msssim(quantize(pred), quantize(target), val_range=255) of every row on its
    own, the plain definition (NaN where a base is negative); the images are quantised as they are loaded.  No gradient; capturable."""
    pred01, tgt01, _ = _msssim_args(pred01.detach(), tgt01.detach(), None, "msssim_metric")
    return _msssim_launch(pred01, tgt01, _hip.SSIM_RANGE_FIXED + 2, False, quantize=True)[0]


# --------------------------------------------------------------------------------------------
# Laplacian-pyramid L1, the term 'Lap' of --loss          (no counterpart in the reference; definition: include/savfi_hip.h)
# --------------------------------------------------------------------------------------------
LAP_LEVELS = 5


class _LapLoss(torch.autograd.Function):
    """sr, hr [N,C,H,W] -> float32[N] (every sample on its own) or float32[1] (fold: one value over the batch); capturable; deterministic."""

    @staticmethod
    def forward(ctx, sr, hr, levels, fold):
        _hip.require_cuda(sr, hr)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("lap_loss differentiates w.r.t. the prediction only")
        rows, C, H, W = _fold_dims(sr, fold)
        res = torch.empty(rows, dtype=torch.float32, device=sr.device)
        scratch = torch.empty(_workspace_floats("savfi_laploss_scratch_bytes", rows, C, H, W, levels) // 4, dtype=torch.float32,
                              device=sr.device)
        _hip.call("laploss", "savfi_laploss_f32", sr, hr, res, scratch, rows, C, H, W, levels, nbytes=int(4 * sr.numel() * (2 + 2 / 3)))
        ctx.levels, ctx.fold = levels, fold
        ctx.scratch = scratch      # the pyramid of the difference, and the backward's work area: not a saved tensor (the backward writes into it)
        ctx.save_for_backward(sr, hr)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sr, hr = ctx.saved_tensors
        rows, C, H, W = _fold_dims(sr, ctx.fold)
        g = g.contiguous()
        gsr = torch.empty_like(sr)
        _hip.call("laploss_bwd", "savfi_laploss_bwd_f32", sr, hr, g, ctx.scratch, gsr, rows, C, H, W, ctx.levels,
                  nbytes=int(4 * sr.numel() * (4 + 1 / 3)))
        return gsr, None, None, None


@functools.lru_cache(maxsize=None)
def _lap_window(device):
    g = torch.tensor([1., 4., 6., 4., 1.]) / 16
    return torch.outer(g, g).to(device)


def _lap_composed(sr, hr, levels):
    """[N]: the same value from differentiable device ops in fp32 (what --second_order takes)."""
    C = sr.shape[1]
    k = _lap_window(sr.device).expand(C, 1, 5, 5)

    def gauss(x, scale):
        return torch.nn.functional.conv2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode='reflect'), k * scale, groups=C)
    c = sr - hr
    n0 = c[0].numel()
    total = 0
    for s in range(levels - 1):
        down = gauss(c, 1.0)[:, :, ::2, ::2]
        z = torch.zeros_like(c)
        z[:, :, ::2, ::2] = down
        total = total + 2.0 ** s * (c - gauss(z, 4.0)).abs().flatten(1).sum(1)
        c = down
    return (total + 2.0 ** (levels - 1) * c.abs().flatten(1).sum(1)) / n0


def _lap_args(sr, hr, levels, what):
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError("%s needs two [N,C,H,W] tensors of one shape, got %s, %s" % (what, tuple(sr.shape), tuple(hr.shape)))
    if not isinstance(levels, int) or not 2 <= levels <= 5:
        raise ValueError("%s: levels must be 2..5, got %r" % (what, levels))
    h, w = sr.shape[2], sr.shape[3]
    for _ in range(levels - 1):
        if h < 3 or w < 3:
            raise ValueError("%s: every filtered level needs both sides >= 3 (reflection by 2; H, W >= 17 for five levels), got %s with "
                             "levels=%d" % (what, tuple(sr.shape), levels))
        h, w = (h + 1) // 2, (w + 1) // 2
    sr, hr = sr.contiguous(), hr.contiguous()
    _hip.require_cuda(sr, hr)
    return sr, hr


def lap_loss(sr, hr, levels=LAP_LEVELS):
    """Laplacian-pyramid L1 over the whole batch: sum_s 2^s sum |b_s(sr - hr)| / (N C H W), 5-tap binomial window, reflected borders,
    the last level the low-pass residual.  Gradient for `sr` only."""
    sr, hr = _lap_args(sr, hr, levels, "lap_loss")
    if double_backward():
        return _lap_composed(sr, hr, levels).mean()
    return _LapLoss.apply(sr, hr, levels, True).reshape(())


def lap_loss_per_sample(sr, hr, levels=LAP_LEVELS):
    """[N,C,H,W] x [N,C,H,W] -> [N]: the same term for every sample on its own (tasks adapted in lockstep)."""
    sr, hr = _lap_args(sr, hr, levels, "lap_loss_per_sample")
    if double_backward():
        return _lap_composed(sr, hr, levels)
    return _LapLoss.apply(sr, hr, levels, False)


# --------------------------------------------------------------------------------------------
# Census (soft ternary) loss, the term 'Census' of --loss   (no counterpart in the reference; definition: include/savfi_hip.h)
# --------------------------------------------------------------------------------------------
class _CensusLoss(torch.autograd.Function):
    """sr, hr [N,C,H,W] -> float32[N] (every sample on its own) or float32[1] (fold: the mean over the batch); capturable; deterministic."""

    @staticmethod
    def forward(ctx, sr, hr, fold):
        _hip.require_cuda(sr, hr)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("census_loss differentiates w.r.t. the prediction only")
        N, C, H, W = sr.shape
        rows, n = (1, N) if fold else (N, 1)
        res = torch.empty(rows, dtype=torch.float32, device=sr.device)
        scratch = torch.empty(_workspace_floats("savfi_census_scratch_bytes", rows, n, C, H, W) // 8, dtype=torch.float64, device=sr.device)
        _hip.call("census", "savfi_census_f32", sr, hr, res, scratch, rows, n, C, H, W, nbytes=8 * sr.numel())
        ctx.fold = fold
        ctx.save_for_backward(sr, hr)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sr, hr = ctx.saved_tensors
        N, C, H, W = sr.shape
        rows, n = (1, N) if ctx.fold else (N, 1)
        g = g.contiguous()
        gsr = torch.empty_like(sr)
        _hip.call("census_bwd", "savfi_census_bwd_f32", sr, hr, g, gsr, rows, n, C, H, W, nbytes=12 * sr.numel())
        return gsr, None, None


_CENSUS_GRAY = (0.2989, 0.5870, 0.1140)


def _census_composed(sr, hr):
    """[N]: the same value from differentiable device ops in fp32 (what --second_order takes): 49-channel tensors, as the definition reads."""
    H, W = sr.shape[2], sr.shape[3]

    def ternary(x):
        g = x[:, 0] if x.shape[1] == 1 else _CENSUS_GRAY[0] * x[:, 0] + _CENSUS_GRAY[1] * x[:, 1] + _CENSUS_GRAY[2] * x[:, 2]
        p = torch.nn.functional.pad(g, (3, 3, 3, 3))
        d = torch.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(7) for dx in range(7)], 1) - g[:, None]
        return d / torch.sqrt(0.81 + d * d)
    delta = (ternary(sr) - ternary(hr)) ** 2
    c = (delta / (0.1 + delta)).mean(1)
    return c[:, 1:-1, 1:-1].flatten(1).sum(1) / (H * W)


def _census_args(sr, hr, what):
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError("%s needs two [N,C,H,W] tensors of one shape, got %s, %s" % (what, tuple(sr.shape), tuple(hr.shape)))
    if sr.shape[1] not in (1, 3):
        raise ValueError("%s needs 3 channels (gray = 0.2989 R + 0.5870 G + 0.1140 B) or 1, got %s" % (what, tuple(sr.shape)))
    if sr.shape[2] < 3 or sr.shape[3] < 3:
        raise ValueError("%s needs H, W >= 3, got %s" % (what, tuple(sr.shape)))
    sr, hr = sr.contiguous(), hr.contiguous()
    _hip.require_cuda(sr, hr)
    return sr, hr


def census_loss(sr, hr):
    """Census (soft ternary) loss as one value, the mean over the batch: per sample, with g the gray image (zero outside the frame),
    d_o = g(p + o) - g(p) for the 49 offsets of the 7 x 7 window, t_o = d_o / sqrt(0.81 + d_o^2), delta_o = (t_o(sr) - t_o(hr))^2,
    sum over the pixels off the outermost ring of mean_o delta_o / (0.1 + delta_o), divided by H W.  The constants presume unit-range
    frames; the term is applied to whatever tensors it is handed (Super SloMo's mean-subtracted and VoxelFlow's normalised frames
    included), as the other terms are.  Gradient for `sr` only."""
    sr, hr = _census_args(sr, hr, "census_loss")
    if double_backward():
        return _census_composed(sr, hr).mean()
    return _CensusLoss.apply(sr, hr, True).reshape(())


def census_loss_per_sample(sr, hr):
    """[N,C,H,W] x [N,C,H,W] -> [N]: the same term for every sample on its own (tasks adapted in lockstep)."""
    sr, hr = _census_args(sr, hr, "census_loss_per_sample")
    if double_backward():
        return _census_composed(sr, hr)
    return _CensusLoss.apply(sr, hr, False)


# --------------------------------------------------------------------------------------------
# AdaCoF's deformable-tap op, the tail of --model adacof   (no counterpart in the reference; definition: include/savfi_hip.h)
# --------------------------------------------------------------------------------------------
def adacof_bytes(x, w, grads=0):
    """HBM bytes of one launch if every operand is read / written exactly once: the frame, the three parameter stacks, the output (or
    its cotangent) and `grads` gradient stacks"""
    N, C = x.shape[0], x.shape[1]
    return 4 * (x.numel() + (3 + grads) * w.numel() + N * C * w.shape[2] * w.shape[3])


class _AdaCoF(torch.autograd.Function):
    """x [N,C,Hp,Wp] (no gradient), w, a, b [N,F^2,H,W] -> [N,C,H,W]: one launch forward, one launch backward for whichever of the
    three parameter gradients are needed; capturable; deterministic."""

    @staticmethod
    def forward(ctx, x, w, a, b, F, dilation):
        _hip.require_cuda(x, w, a, b)
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("adacof: the frame requires grad, and the fused op builds no frame gradient (it would be dropped "
                                      "silently); hip_ops.adacof_composed differentiates it")
        N, C = x.shape[0], x.shape[1]
        H, W = w.shape[2], w.shape[3]
        out = torch.empty((N, C, H, W), dtype=x.dtype, device=x.device)
        _hip.call("adacof_fwd", "savfi_adacof_fwd_f32", x, w, a, b, out, N, C, H, W, F, dilation, nbytes=adacof_bytes(x, w))
        ctx.geom = (N, C, H, W, F, dilation)
        ctx.save_for_backward(x, w, a, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w, a, b = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:4]
        if not any(needs):
            return None, None, None, None, None, None
        g = g.contiguous()
        _hip.require_cuda(g)
        gw, ga, gb = (torch.empty_like(w) if need else None for need in needs)
        _hip.call("adacof_bwd", "savfi_adacof_bwd_f32", x, w, a, b, g, gw, ga, gb, *ctx.geom, nbytes=adacof_bytes(x, w, sum(needs)))
        return None, gw, ga, gb, None, None


def _adacof_args(x, w, a, b, dilation, what):
    """-> F, after the checks of the C entry that shapes decide (a ValueError names the argument instead of an error code)"""
    if x.dim() != 4 or w.dim() != 4 or a.shape != w.shape or b.shape != w.shape:
        raise ValueError("%s needs a frame [N,C,Hp,Wp] and three [N,F*F,H,W] tensors of one shape, got %s, %s, %s, %s"
                         % (what, tuple(x.shape), tuple(w.shape), tuple(a.shape), tuple(b.shape)))
    F = int(round(w.shape[1] ** 0.5))
    if F * F != w.shape[1] or F % 2 == 0 or F > 11:
        raise ValueError("%s needs F * F taps with F odd and at most 11, got %d planes" % (what, w.shape[1]))
    dilation = int(dilation)
    if not 1 <= dilation <= 8:
        raise ValueError("%s needs a dilation of 1 to 8, got %d" % (what, dilation))
    if x.shape[1] not in (1, 3):
        raise ValueError("%s needs 3 channels or 1, got %s" % (what, tuple(x.shape)))
    N, _, H, W = w.shape
    rim = (F - 1) * dilation
    if x.shape[0] != N or x.shape[2] != H + rim or x.shape[3] != W + rim:
        raise ValueError("%s needs the frame padded by (F - 1) * dilation = %d in all: [%d,C,%d,%d], got %s"
                         % (what, rim, N, H + rim, W + rim, tuple(x.shape)))
    return F


def adacof_composed(x, w, a, b, dilation=1):
    """The definition of adacof() from differentiable torch ops, on any device and in any floating dtype: what second-order passes
    (set_double_backward(True)), CPU tensors and non-fp32 tensors take.  The coordinate is formed in the tensors' dtype (one addition to
    an exact integer), clamped to [-1, size] before the cell is taken; differentiable to any order in w, a, b and x."""
    F = _adacof_args(x, w, a, b, dilation, "adacof_composed")
    dilation = int(dilation)
    N, C, Hp, Wp = x.shape
    _, F2, H, W = w.shape
    tap = torch.arange(F2, device=x.device)
    base_y = (torch.arange(H, device=x.device).view(1, 1, H, 1) + (tap // F * dilation).view(1, F2, 1, 1)).to(a.dtype)
    base_x = (torch.arange(W, device=x.device).view(1, 1, 1, W) + (tap % F * dilation).view(1, F2, 1, 1)).to(b.dtype)

    def axis(s, size):
        s = s.clamp(-1, size)                                          # NaN passes
        cell = s.detach().floor()
        t = s - cell
        i = torch.nan_to_num(cell, nan=-1.0).long()
        return i.clamp(0, size - 1), (i + 1).clamp(0, size - 1), t.unsqueeze(1)

    i0, i1, ty = axis(base_y + a, Hp)
    j0, j1, tx = axis(base_x + b, Wp)
    flat = x.reshape(N, C, Hp * Wp)

    def texel(i, j):
        return flat.gather(2, (i * Wp + j).reshape(N, 1, -1).expand(N, C, -1)).reshape(N, C, F2, H, W)

    top = (1 - tx) * texel(i0, j0) + tx * texel(i0, j1)
    bot = (1 - tx) * texel(i1, j0) + tx * texel(i1, j1)
    return (w.unsqueeze(1) * ((1 - ty) * top + ty * bot)).sum(2)


def adacof(x, w, a, b, dilation=1):
    """AdaCoF's op: x [N,C,Hp,Wp] the frame padded by (F - 1) * dilation in all, w / a / b [N,F*F,H,W] a weight, a vertical and a horizontal
    offset per output pixel and tap -> [N,C,H,W], out = sum_t w_t * bilinear(x, (y + k d + a_t, x + l d + b_t)) with border replicate
    (include/savfi_hip.h).  fp32 device tensors take the fused kernels: one launch forward, one backward, gradients for w, a, b only (a
    frame that requires grad is refused).  Second-order passes, CPU tensors and other dtypes take adacof_composed."""
    F = _adacof_args(x, w, a, b, dilation, "adacof")
    tensors = (x, w, a, b)
    if double_backward() or not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return adacof_composed(x, w, a, b, dilation)
    x, w, a, b = (t.contiguous() for t in tensors)
    _hip.require_cuda(x, w, a, b)
    return _AdaCoF.apply(x, w, a, b, F, int(dilation))


# --------------------------------------------------------------------------------------------
# Softmax splatting (forward warping), the op of --model softsplat   (no counterpart in the reference; definition: include/savfi_hip.h)
# --------------------------------------------------------------------------------------------
SOFTSPLAT_MODES = _hip.SOFTSPLAT_MODES


def softsplat_bytes(x, mode='soft', grads=0):
    """Algorithmic HBM bytes of one call if every operand moves once per launch that touches it.  Forward (grads=0): x twice (scan,
    scatter), flow and metric twice in soft mode (once otherwise), the C + 1 64-bit accumulators cleared, added to and read, the keys
    likewise, out + hit + D + M written.  Backward (grads = number of gradient tensors wanted, each counted at the size of the mean of
    the three): x, out, g_out, flow, metric, D, M read, the gradients written."""
    N, C, H, W = x.shape
    px, soft = N * H * W, mode == 'soft'
    if not grads:
        return px * (8 * C + (2 if soft else 1) * (8 + (4 if soft else 0)) + 3 * 8 * (C + 1) + 3 * 4 + 4 * C + 12)
    return px * (12 * C + 8 + (4 if soft else 0) + 8 + grads * (4 * C + 12) // 3)


class _SoftSplat(torch.autograd.Function):
    """x [N,C,H,W], flow [N,2,H,W], metric [N,1,H,W] or None -> out [N,C,H,W], hit [N,1,H,W] (no gradient): four launches forward, one
    backward for whichever of the three gradients are needed; capturable; bit-reproducible."""

    @staticmethod
    def forward(ctx, x, flow, metric, mode):
        _hip.require_cuda(x, flow, metric)
        N, C, H, W = x.shape
        out = torch.empty_like(x)
        hit, den, mx = (torch.empty((N, 1, H, W), dtype=x.dtype, device=x.device) for _ in range(3))
        scratch = torch.empty(_workspace_floats("savfi_softsplat_scratch_bytes", N, C, H, W), dtype=torch.uint8, device=x.device)
        _hip.call("softsplat_fwd", "savfi_softsplat_fwd_f32", x, flow, metric, out, hit, den, mx, scratch, N, C, H, W, SOFTSPLAT_MODES[mode],
                  nbytes=softsplat_bytes(x, mode))
        ctx.mode = mode
        ctx.has_metric = metric is not None
        ctx.save_for_backward(*((x, flow, out, den, mx) + ((metric,) if metric is not None else ())))
        ctx.mark_non_differentiable(hit)
        return out, hit

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _ghit):
        x, flow, out, den, mx = ctx.saved_tensors[:5]
        metric = ctx.saved_tensors[5] if ctx.has_metric else None
        needs = ctx.needs_input_grad[:3]
        if not any(needs):
            return None, None, None, None
        g = g.contiguous()
        _hip.require_cuda(g)
        N, C, H, W = x.shape
        gx = torch.empty_like(x) if needs[0] else None
        gf = torch.empty_like(flow) if needs[1] else None
        gm = torch.empty_like(metric) if needs[2] else None
        _hip.call("softsplat_bwd", "savfi_softsplat_bwd_f32", x, flow, metric, out, den, mx, g, gx, gf, gm, N, C, H, W,
                  SOFTSPLAT_MODES[ctx.mode], nbytes=softsplat_bytes(x, ctx.mode, sum(needs)))
        return gx, gf, gm, None


def _softsplat_args(x, flow, metric, mode, what):
    """The checks of the C entry that shapes decide (a ValueError names the argument instead of an error code) -> the metric the mode reads"""
    if mode not in SOFTSPLAT_MODES:
        raise ValueError("%s: mode must be one of %s, got %r (a linear mode is soft with metric = log w)" % (what, sorted(SOFTSPLAT_MODES), mode))
    if x.dim() != 4 or flow.dim() != 4 or flow.shape != (x.shape[0], 2, x.shape[2], x.shape[3]):
        raise ValueError("%s needs x [N,C,H,W] and flow [N,2,H,W], got %s, %s" % (what, tuple(x.shape), tuple(flow.shape)))
    if x.shape[1] > 256 or 0 in x.shape:
        raise ValueError("%s needs 1 to 256 channels and a non-empty tensor, got %s" % (what, tuple(x.shape)))
    if mode != 'soft':
        return None                      # sum and avg read no metric
    if metric is None:
        raise ValueError("%s: mode 'soft' needs a metric [N,1,H,W]" % what)
    if metric.shape != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise ValueError("%s needs a metric [N,1,H,W] for x %s, got %s" % (what, tuple(x.shape), tuple(metric.shape)))
    return metric


def softsplat_composed(x, flow, metric=None, mode='soft', return_hit=False):
    """The definition of softsplat() from differentiable torch ops, on any device and in any floating dtype: what second-order passes
    (set_double_backward(True)), CPU tensors and non-fp32 tensors take.  The coordinate is formed in the tensors' dtype (one addition to an
    exact integer); the sums are index_add scatters (on a device: float atomics, not bit-reproducible), M is a scatter_reduce(amax) of
    detached values; differentiable to any order in x, flow and metric."""
    metric = _softsplat_args(x, flow, metric, mode, "softsplat_composed")
    N, C, H, W = x.shape
    dt, dev, hw = x.dtype, x.device, H * W
    X = torch.arange(W, device=dev, dtype=dt).view(1, 1, W) + flow[:, 0]
    Y = torch.arange(H, device=dev, dtype=dt).view(1, H, 1) + flow[:, 1]
    src = (X > -1) & (X < W) & (Y > -1) & (Y < H)                   # NaN, +-inf and 1e30 fail; what any corner taking part needs
    if metric is not None:
        src = src & torch.isfinite(metric[:, 0])
    zero = torch.zeros((), dtype=dt, device=dev)
    X, Y = torch.where(src, X, zero), torch.where(src, Y, zero)     # a source taking no part: finite stand-ins, masked out below
    x0, y0 = X.detach().floor(), Y.detach().floor()
    tx, ty = X - x0, Y - y0
    wx, wy = (1 - tx, tx), (1 - ty, ty)
    base = (torch.arange(N, device=dev) * hw).view(N, 1, 1)
    idx, ok, b = [], [], []
    for k in range(4):
        dx, dy = k & 1, k >> 1
        xx, yy = x0 + dx, y0 + dy
        take = src & (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1) & (wx[dx].detach() > 0) & (wy[dy].detach() > 0)
        ok.append(take)
        idx.append((base + torch.where(take, yy * W + xx, zero).long()).reshape(-1))
        b.append(torch.where(take, wx[dx] * wy[dy], zero).reshape(-1))
    if metric is not None:
        Z = torch.where(src, metric[:, 0], zero).reshape(-1)
        low = torch.full((), float('-inf'), dtype=dt, device=dev)
        M = torch.full((N * hw,), float('-inf'), dtype=dt, device=dev)
        for k in range(4):
            M = M.scatter_reduce(0, idx[k], torch.where(ok[k].reshape(-1), Z.detach(), low), 'amax', include_self=True)
        w = [b[k] * torch.exp(Z - torch.where(ok[k].reshape(-1), M[idx[k]], Z.detach())) for k in range(4)]
    else:
        w = b
    xs = x.permute(0, 2, 3, 1).reshape(N * hw, C)
    num = torch.zeros((N * hw, C), dtype=dt, device=dev)
    den = torch.zeros((N * hw,), dtype=dt, device=dev)
    cnt = torch.zeros((N * hw,), dtype=dt, device=dev)
    for k in range(4):
        num = num.index_add(0, idx[k], w[k].unsqueeze(1) * xs)
        den = den.index_add(0, idx[k], w[k])
        cnt = cnt.index_add(0, idx[k], ok[k].reshape(-1).to(dt))
    hit = cnt > 0
    if mode == 'sum':
        out = num
    else:
        out = torch.where(hit.unsqueeze(1), num / torch.where(hit, den, torch.ones((), dtype=dt, device=dev)).unsqueeze(1), zero)
    out = out.reshape(N, H, W, C).permute(0, 3, 1, 2)
    bad = ~torch.isfinite(x.detach()).flatten(1).all(1)
    out = torch.where(bad.view(N, 1, 1, 1), torch.full((), float('nan'), dtype=dt, device=dev), out).contiguous()
    return (out, hit.reshape(N, 1, H, W).to(dt)) if return_hit else out


def softsplat(x, flow, metric=None, mode='soft', return_hit=False):
    """Softmax splatting (forward warping): the source pixel p of x [N,C,H,W] lands at p + flow(p) (flow [N,2,H,W], x then y) and is shared
    bilinearly among the four pixels around it.  mode 'sum': the plain sum of the shares; 'avg': divided by the sum of the weights;
    'soft': weighted by exp(metric) [N,1,H,W] as a per-target softmax, finite for every finite metric (include/savfi_hip.h).  Where
    nothing lands the result is 0; return_hit: also hit [N,1,H,W], 1 where something landed (no gradient).  fp32 device tensors take the
    fused kernels (four launches forward, one backward; gradients for x, flow and metric; bit-reproducible).  Second-order passes, CPU
    tensors and other dtypes take softsplat_composed."""
    metric = _softsplat_args(x, flow, metric, mode, "softsplat")
    tensors = (x, flow) + (() if metric is None else (metric,))
    if double_backward() or not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return softsplat_composed(x, flow, metric, mode, return_hit)
    x, flow = x.contiguous(), flow.contiguous()
    metric = None if metric is None else metric.contiguous()
    out, hit = _SoftSplat.apply(x, flow, metric, mode)
    return (out, hit) if return_hit else out


def frames_to_u8(x):
    """x [N,C,H,W] (or [C,H,W], [H,W]) in unit range, C = 1 or 3 -> uint8 [N,H,W,C] ([H,W,C], [H,W]) on the device, quantised as
    utils.save_image does (the metric's device function): a frame leaves the device as bytes."""
    shape = x.shape
    if x.dim() not in (2, 3, 4):
        raise ValueError("frames_to_u8 needs [N,C,H,W], [C,H,W] or [H,W], got %s" % (tuple(shape),))
    x4 = x.detach().reshape((1,) * (4 - x.dim()) + tuple(shape)).contiguous()
    _hip.require_cuda(x4)
    N, C, H, W = x4.shape
    if C not in (1, 3):
        raise ValueError("frames_to_u8 writes 1 or 3 channels, got %d" % C)
    out = torch.empty((N, H, W, C), dtype=torch.uint8, device=x.device)
    if out.numel():
        _hip.call("frames_to_u8", "savfi_frames_f32_to_u8", x4, out, N, C, H, W, nbytes=5 * x4.numel())
    return out if x.dim() == 4 else out[0] if x.dim() == 3 else out[0, :, :, 0]


# --------------------------------------------------------------------------------------------
# DAIN's adaptive warping layer and depth-aware flow projection
#   (dain/my_package/FilterInterpolation/FilterInterpolationLayer.py, dain/my_package/DepthFlowProjection/DepthFlowProjectionLayer.py)
# --------------------------------------------------------------------------------------------
def filterinterp_bytes(B, C, H, W, grads=0):
    """Algorithmic HBM bytes of one adaptive-warping call (each operand once): forward in + flow + filt + out; backward (grads=1)
    in + flow + filt + gout and the three gradients (g_in is written twice: cleared, then accumulated)."""
    px = B * H * W
    return 4 * px * ((2 * C + 18) if not grads else (2 * C + 18 + 2 * C + 18))


def depthflowproj_bytes(B, H, W, grads=0):
    """Algorithmic HBM bytes of one flow-projection call: forward flow + w read twice (maximum pass, scatter), three 64-bit
    accumulators cleared and read, count + out written; backward flow + w + count + out + gout read, g_flow + g_w written."""
    px = B * H * W
    return px * ((2 * 12 + 2 * 24 + 12) if not grads else 4 * 11)


class _FilterInterpolation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input1, input2, input3):
        _hip.require_cuda(input1, input2, input3)
        B, C, H, W = input1.shape
        if input2.shape != (B, 2, H, W) or input3.shape != (B, 16, H, W):
            raise ValueError("filter_interpolation needs input [B,C,H,W], flow [B,2,H,W] and a 4 x 4 filter [B,16,H,W], got %s, %s, %s"
                             % (tuple(input1.shape), tuple(input2.shape), tuple(input3.shape)))
        out = torch.empty_like(input1)
        _hip.call("filterinterp_fwd", "savfi_filterinterp_fwd_f32", input1, input2, input3, out, B, C, H, W, 4,
                  nbytes=filterinterp_bytes(B, C, H, W))
        ctx.save_for_backward(input1, input2, input3)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, input2, input3 = ctx.saved_tensors
        B, C, H, W = input1.shape
        gradoutput = gradoutput.contiguous()
        need = ctx.needs_input_grad
        # every gradient the entry writes is written completely (g_in is cleared by the entry itself)
        g1 = torch.empty_like(input1) if need[0] else None
        g2 = torch.empty_like(input2) if need[1] else None
        g3 = torch.empty_like(input3) if need[2] else None
        _hip.call("filterinterp_bwd", "savfi_filterinterp_bwd_f32", input1, input2, input3, gradoutput, g1, g2, g3, B, C, H, W, 4,
                  nbytes=filterinterp_bytes(B, C, H, W, grads=1))
        return g1, g2, g3


def filter_interpolation(input, flow, filt):
    """DAIN's adaptive warping layer (FilterInterpolationLayer.apply): input [B,C,H,W], flow [B,2,H,W], filt [B,16,H,W] -> [B,C,H,W].
    First order only (the backward is once_differentiable: a second derivative raises).  g_input is accumulated with fp32 atomics
    and is the one result that is not bit-reproducible; everything else is."""
    return _FilterInterpolation.apply(input.contiguous(), flow.contiguous(), filt.contiguous())


def filter_interpolation_into(out, c_off, input, flow, filt):
    """filter_interpolation(input, flow, filt) written into channels [c_off, c_off + C) of ``out`` [B,C_total,H,W] (contiguous): the
    same bits, no other channel touched, one launch and no temporary.  Forward only, as the frozen front of MetaDAIN needs it."""
    input, flow, filt = input.contiguous(), flow.contiguous(), filt.contiguous()
    _hip.require_cuda(out, input, flow, filt)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (out, input, flow, filt)):
        raise NotImplementedError("filter_interpolation_into has no backward: it fills the rectify input of DAIN's frozen front "
                                  "(meta_learning_system.py:96-101); call it under torch.no_grad()")
    B, C, H, W = input.shape
    if flow.shape != (B, 2, H, W) or filt.shape != (B, 16, H, W) or out.dim() != 4 or (out.shape[0], out.shape[2], out.shape[3]) != (B, H, W):
        raise ValueError("filter_interpolation_into needs input [B,C,H,W], flow [B,2,H,W], a 4 x 4 filter [B,16,H,W] and out "
                         "[B,C_total,H,W], got %s, %s, %s, %s" % (tuple(input.shape), tuple(flow.shape), tuple(filt.shape), tuple(out.shape)))
    _hip.call("filterinterp_fwd_slice", "savfi_filterinterp_fwd_slice_f32", input, flow, filt, out, B, C, H, W, 4, out.shape[1], int(c_off),
              nbytes=filterinterp_bytes(B, C, H, W))
    return out


class _DepthFlowProjection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input1, input2, fillhole):
        _hip.require_cuda(input1, input2)
        B, two, H, W = input1.shape
        if two != 2 or input2.shape != (B, 1, H, W):
            raise ValueError("depth_flow_projection needs flow [B,2,H,W] and a depth inverse [B,1,H,W], got %s, %s"
                             % (tuple(input1.shape), tuple(input2.shape)))
        count = torch.empty((B, 1, H, W), dtype=input1.dtype, device=input1.device)
        output = torch.empty_like(input1)
        scratch = torch.empty(_workspace_floats("savfi_depthflowproj_scratch_bytes", B, H, W), dtype=torch.uint8, device=input1.device)
        _hip.call("depthflowproj_fwd", "savfi_depthflowproj_fwd_f32", input1, input2, count, output, scratch, B, H, W, int(bool(fillhole)),
                  nbytes=depthflowproj_bytes(B, H, W))
        # as the reference saves them (DepthFlowProjectionLayer.py:47): the output AFTER the hole fill
        ctx.save_for_backward(input1, input2, count, output)
        ctx.mark_non_differentiable(count)
        return output, count

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput, _gcount):
        input1, input2, count, output = ctx.saved_tensors
        B, _, H, W = input1.shape
        gradoutput = gradoutput.contiguous()
        need = ctx.needs_input_grad
        g1 = torch.empty_like(input1) if need[0] else None       # a gradient that is not needed goes to the C ABI as NULL
        g2 = torch.empty_like(input2) if need[1] else None
        _hip.call("depthflowproj_bwd", "savfi_depthflowproj_bwd_f32", input1, input2, count, output, gradoutput, g1, g2, B, H, W,
                  nbytes=depthflowproj_bytes(B, H, W, grads=1))
        return g1, g2, None


def depth_flow_projection(flow, depth_inv, fillhole, return_count=False):
    """DAIN's depth-aware flow projection (DepthFlowProjectionLayer.apply): flow [B,2,H,W], depth_inv [B,1,H,W] -> projected flow
    [B,2,H,W]; fillhole: fill pixels nothing landed on from their nearest valid neighbours in four directions (the reference sets
    it when the flow needs no gradient).  Bit-reproducible, forward and backward.  return_count: also the accumulated depth
    inverses [B,1,H,W] (no gradient)."""
    out, count = _DepthFlowProjection.apply(flow.contiguous(), depth_inv.contiguous(), fillhole)
    return (out, count) if return_count else out


# --------------------------------------------------------------------------------------------
# PWC-Net's cost-volume correlation and warp     (dain/PWCNet/correlation_package_pytorch1_0/correlation.py, dain/PWCNet/PWCNet.py:158-198)
# --------------------------------------------------------------------------------------------
def correlation_bytes(N, C, H, W, md=4, grads=0):
    """Algorithmic HBM bytes of one correlation call (each operand once): forward f1 + f2 + out; backward (grads=1) f1 + f2 + gout + out
    and both gradients."""
    px, nt = N * H * W, (2 * md + 1) ** 2
    return 4 * px * ((2 * C + nt) if not grads else (4 * C + 2 * nt))


def pwc_warp_bytes(N, C, H, W):
    """Algorithmic HBM bytes of one PWC warp: img + flow + out."""
    return 4 * N * H * W * (2 * C + 2)


class _Correlation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, md, slope):
        _hip.require_cuda(f1, f2)
        N, C, H, W = f1.shape
        if f2.shape != f1.shape:
            raise ValueError("correlation needs two feature maps of one shape [N,C,H,W], got %s, %s" % (tuple(f1.shape), tuple(f2.shape)))
        out = torch.empty((N, (2 * md + 1) ** 2, H, W), dtype=f1.dtype, device=f1.device)       # written completely by the kernel
        _hip.call("correlation_fwd", "savfi_correlation_fwd_f32", f1, f2, out, N, C, H, W, md, slope, nbytes=correlation_bytes(N, C, H, W, md))
        ctx.md, ctx.slope = md, slope
        ctx.save_for_backward(f1, f2, out if slope != 1.0 else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        f1, f2, out = ctx.saved_tensors
        N, C, H, W = f1.shape
        gout = gout.contiguous()
        need = ctx.needs_input_grad
        g1 = torch.empty_like(f1) if need[0] else None          # a gradient that is not needed goes to the C ABI as NULL
        g2 = torch.empty_like(f2) if need[1] else None
        _hip.call("correlation_bwd", "savfi_correlation_bwd_f32", f1, f2, gout, out, ctx.slope, g1, g2, N, C, H, W, ctx.md,
                  nbytes=correlation_bytes(N, C, H, W, ctx.md, grads=1))
        return g1, g2, None, None


def correlation(f1, f2, md=4, slope=1.0):
    """PWC-Net's cost volume: out[n, (tj+md)(2md+1) + ti+md, y, x] = mean_c f1[n,c,y,x] f2[n,c,y+tj,x+ti] over zero-padded maps, then
    LeakyReLU(slope) in the same kernel (slope = 1: none).  [N,C,H,W] x 2 -> [N,(2md+1)^2,H,W]; md = 4 is the one the library builds.
    First order only (once_differentiable); forward and both gradients are bit-reproducible."""
    return _Correlation.apply(f1.contiguous(), f2.contiguous(), int(md), float(slope))


def pwc_warp(img, flow, scale=1.0):
    """PWCDCNet.warp(img, flow * scale): img [N,C,H,W] sampled bilinearly at (x + scale u, y + scale v) with zeros outside -- grid_sample
    with align_corners=True, as the torch the reference pins for DAIN ran it -- and zeroed where the same sample of an all-ones image is
    below 0.9999.  One launch; forward only, as the frozen flow estimator needs it."""
    img, flow = img.contiguous(), flow.contiguous()
    _hip.require_cuda(img, flow)
    if torch.is_grad_enabled() and (img.requires_grad or flow.requires_grad):
        raise NotImplementedError("pwc_warp has no backward: PWC-Net is frozen on every path of the reference's system "
                                  "(meta_learning_system.py:96-101); call it under torch.no_grad()")
    N, C, H, W = img.shape
    if flow.shape != (N, 2, H, W):
        raise ValueError("pwc_warp needs img [N,C,H,W] and flow [N,2,H,W], got %s, %s" % (tuple(img.shape), tuple(flow.shape)))
    out = torch.empty_like(img)
    _hip.call("pwcwarp_fwd", "savfi_pwcwarp_fwd_f32", img, flow, float(scale), out, N, C, H, W, nbytes=pwc_warp_bytes(N, C, H, W))
    return out


# --------------------------------------------------------------------------------------------
# DAIN's frozen front and rectify net: BatchNorm per task, max-pool, nearest x2 + add, add + ReLU, Charbonnier   (csrc/dainnet.hip)
# --------------------------------------------------------------------------------------------
CHARBONNIER_EPS = 1e-8          # dain/networks/DAIN.py:638


def _frozen(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError("%s has no backward: DAIN's front is frozen on every path of the reference's system "
                                  "(meta_learning_system.py:96-101); call it under torch.no_grad()" % what)


def _stat_view(t, C, what):
    """A [G, C] view of per-group statistics whose channels are adjacent (a column slice of a flat [G, total] buffer) -> (G, stride)."""
    if not t.is_cuda:
        raise NotImplementedError("savfi HIP ops need device tensors (%s)" % what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != C or (C > 1 and t.stride(1) != 1):
        raise ValueError("%s must be a float32 [groups, %d] view with adjacent channels, got %s %s stride %s"
                         % (what, C, t.dtype, tuple(t.shape), t.stride()))
    return t.shape[0], (t.stride(0) if t.shape[0] > 1 else 0)


def bn_stats(x, n_per_group, mean=None, var=None):
    """Per (group, channel) mean and biased variance of x [N,C,H,W] over the n_per_group * H * W values of each group of n_per_group
    consecutive samples: what train-mode BatchNorm2d normalises with when a group is a call of its own.  A group's results do not depend,
    bit for bit, on what else is in the batch.  mean / var: [N / n_per_group, C] views to write into (column slices of a flat buffer
    are fine), allocated when None.  Returns (mean, var).  Forward only."""
    x = x.contiguous()
    _hip.require_cuda(x)
    _frozen("bn_stats", x)
    N, C, H, W = x.shape
    n_per_group = int(n_per_group)
    if n_per_group <= 0 or N % n_per_group:
        raise ValueError("a batch of %d samples is no multiple of n_per_group = %d" % (N, n_per_group))
    if n_per_group * H * W == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (list(x.shape),))
    G = N // n_per_group
    if mean is None:
        mean, var = x.new_empty(G, C), x.new_empty(G, C)
    (gm, sm), (gv, sv) = _stat_view(mean, C, "mean"), _stat_view(var, C, "var")
    if gm != G or gv != G or sm != sv:
        raise ValueError("mean and var must be [%d, %d] views with one group stride" % (G, C))
    nscratch = _workspace_floats("savfi_bn_stats_scratch_floats", N, C, H, W, n_per_group)
    scratch = x.new_empty(nscratch) if nscratch else None
    _hip.call("bn_stats", "savfi_bn_stats_f32", x, mean, var, sm, scratch, N, C, H, W, n_per_group, nbytes=8 * x.numel())
    return mean, var


def bn_apply_relu(x, mean, var, n_per_group, gamma=None, beta=None, eps=1e-5, out=None, c_off=0):
    """relu((x - mean) / sqrt(var + eps) * gamma + beta) with the statistics of each sample's group (mean / var: [groups, C] views, see
    bn_stats; eval mode: the running buffers as [1, C] with n_per_group = N), written into channels [c_off, c_off + C) of `out`
    [N, C_total, H, W] (allocated with C_total = C when None): the branches of an inception block land in their concatenation.
    Forward only."""
    x = x.contiguous()
    _hip.require_cuda(x, gamma, beta, out)
    _frozen("bn_apply_relu", x, gamma, beta)
    N, C, H, W = x.shape
    n_per_group = int(n_per_group)
    if n_per_group <= 0 or N % n_per_group:
        raise ValueError("a batch of %d samples is no multiple of n_per_group = %d" % (N, n_per_group))
    (gm, sm), (gv, sv) = _stat_view(mean, C, "mean"), _stat_view(var, C, "var")
    if gm != N // n_per_group or gv != gm or sm != sv:
        raise ValueError("mean and var must be [%d, %d] views with one group stride" % (N // n_per_group, C))
    if out is None:
        out = x.new_empty(N, C, H, W)
    if out.dim() != 4 or out.shape[0] != N or tuple(out.shape[2:]) != (H, W) or c_off < 0 or c_off + C > out.shape[1]:
        raise ValueError("out %s cannot take channels [%d, %d) of %s" % (tuple(out.shape), c_off, c_off + C, tuple(x.shape)))
    _hip.call("bn_apply_relu", "savfi_bn_apply_relu_f32", x, mean, var, sm, gamma, beta, float(eps), out, N, C, H, W, n_per_group,
              int(c_off), out.shape[1], nbytes=8 * x.numel())
    return out


def bn_running_update(running, stats, unbias, momentum=0.1):
    """running[i] <- (1 - momentum) running[i] + momentum * (stats[i] * unbias[i]) for lists of float32 device vectors (the running
    means and variances of every BatchNorm of a network, the statistics of one forward): ceil(n / 48) launches."""
    running, stats = list(running), list(stats)
    if not running:
        return
    for r, s in zip(running, stats):
        if not (r.is_cuda and s.is_cuda):
            raise NotImplementedError("savfi HIP ops need device tensors (bn_running_update)")
        assert r.dtype == s.dtype == torch.float32 and r.is_contiguous() and s.is_contiguous() and r.numel() == s.numel()
    _hip.call("bn_running_update", "savfi_bn_running_update_f32", len(running), _hip.ptr_array(running), _hip.ptr_array(stats),
              _hip.i64_array([r.numel() for r in running]), _hip.f32_array([float(u) for u in unbias]), float(momentum))


def max_pool2x2(x):
    """nn.MaxPool2d(2, 2) of [N,C,H,W]: odd sides floor, NaN propagates as in torch.max_pool2d.  Forward only."""
    x = x.contiguous()
    _hip.require_cuda(x)
    _frozen("max_pool2x2", x)
    N, C, H, W = x.shape
    out = x.new_empty(N, C, H // 2, W // 2)
    _hip.call("maxpool2x2", "savfi_maxpool2x2_f32", x, out, N * C, H, W, nbytes=5 * out.numel() * 4)
    return out


def upnearest2x_add(low, skip):
    """skip + UpsamplingNearest2d(scale_factor=2)(low): the hourglass's upsample and CAddTable in one pass.  Forward only."""
    low, skip = low.contiguous(), skip.contiguous()
    _hip.require_cuda(low, skip)
    _frozen("upnearest2x_add", low, skip)
    N, C, h, w = low.shape
    if tuple(skip.shape) != (N, C, 2 * h, 2 * w):
        raise ValueError("skip %s is not exactly twice low %s on both sides" % (tuple(skip.shape), tuple(low.shape)))
    out = torch.empty_like(skip)
    _hip.call("upnearest2x_add", "savfi_upnearest2x_add_f32", low, skip, out, N * C, h, w, 2 * h, 2 * w, nbytes=9 * low.numel() * 4)
    return out


class _AddRelu(torch.autograd.Function):
    """relu(a + r); the derivative, taken from the result, goes to both inputs."""

    @staticmethod
    def forward(ctx, a, r):
        _hip.require_cuda(a, r)
        assert a.shape == r.shape
        y = torch.empty_like(a)
        _hip.call("add_relu", "savfi_add_relu_f32", a, r, y, a.numel(), nbytes=12 * a.numel())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, = ctx.saved_tensors
        shape = g.shape
        g = mask_by_activation(g.reshape(1, 1, -1), y.reshape(1, 1, -1), 0.0).reshape(shape)
        return g, g


def add_relu(a, r):
    """relu(a + r), the tail of a residual block (dain/Resblock/BasicBlock.py:146-147), one pass; first order."""
    if double_backward():
        return torch.relu(a + r)
    return _AddRelu.apply(a.contiguous(), r.contiguous())


class _Charbonnier(torch.autograd.Function):
    """a, b [rows, ...] -> float32[rows] of per-row mean sqrt((a - b)^2 + eps^2); deterministic."""

    @staticmethod
    def forward(ctx, a, b, eps):
        rows, n, res, scratch = _row_means_buffers(a, b)
        _hip.call("charbonnier", "savfi_charbonnier_f32", a, b, res, scratch, rows, n, eps, nbytes=8 * a.numel())
        ctx.eps = eps
        ctx.save_for_backward(a, b)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = torch.empty_like(a)
        rows = a.shape[0]
        _hip.call("charbonnier_bwd", "savfi_charbonnier_bwd_f32", a, b, g, ga, rows, a.numel() // rows, ctx.eps, nbytes=12 * a.numel())
        gb = -ga if ctx.needs_input_grad[1] else None
        return ga, gb, None


def charbonnier_loss(a, b, eps=CHARBONNIER_EPS):
    """mean(sqrt((a - b)^2 + eps^2)) over everything (dain/loss_function.py:14-16)."""
    if double_backward():
        d = a - b
        return torch.mean(torch.sqrt(d * d + eps * eps))
    return _Charbonnier.apply(a.contiguous().reshape(1, -1), b.contiguous().reshape(1, -1), float(eps)).reshape(())


def charbonnier_loss_per_sample(a, b, eps=CHARBONNIER_EPS):
    """[N,...] x [N,...] -> [N]: the Charbonnier loss of every sample on its own, one launch."""
    if double_backward():
        d = a - b
        return torch.sqrt(d * d + eps * eps).flatten(1).mean(1)
    a, b = a.contiguous(), b.contiguous()
    return _Charbonnier.apply(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1), float(eps))


# --------------------------------------------------------------------------------------------
# conv + bias + (leaky) ReLU with fused epilogues   (sepconv/model.py:172-194, model_utils.py:957-990)
# --------------------------------------------------------------------------------------------
# 3x3 / stride 1 convolutions run on savfi_conv3x3_f32 (Winograd on the fp32 matrix cores, bias + activation in its
# epilogue) wherever it beats MIOpen; tiles = N * ceil(Ho/2) * ceil(Wo/2).  Thresholds from tools/conv_bench.py with the
# late round-2 kernel (profiles/r02_conv_bench.jsonl: filter transform included): at N >= 2 it is 1.15-2.1x faster forward and
# 1.1-1.9x for the data gradient on every layer shape of the four plugins down to 24x32 maps (12x16 / 16x16 stay on MIOpen:
# forward 1.27x, data gradient 0.87x, on ~40 us kernels); at N = 1 it wins from 48x64 maps up (1.05-1.9x) and loses on 24x32 (0.86-1.04x).  (Round 1 needed 6000-
# 20000 tiles: the corner-tile tail and the output stage's store stalls, DESIGN.md 4b, weighed most on small maps.)
WINOGRAD_CONV = True            # (routing knobs are module attributes: tools and tests set them, no environment variable is read)
WINO_MIN_TILES_FWD = 700
WINO_MIN_TILES_BWD = 700
WINO_MIN_TILES_FWD_BATCHED = 100      # N >= 2 (support pairs, lockstep batches of shared weights): 16x16 maps and up -- with the filters of all
                                      # layers transformed in one launch per inner step (round 3) the forward is 16.5 vs 31.5 us on CAIN's
                                      # 192 -> 192 layers at 16x16, N = 2 and the data gradient 16.1 vs 22.0 (profiles/r03_convk_bench.jsonl);
                                      # config C1: forward 33.7 -> 38.4 steps/s, data gradient another +3 %.  Single samples at that size
                                      # (64 tiles) measured 1 % slower than MIOpen in the loop: they keep the 700 above
WINO_MIN_TILES_BWD_BATCHED = 100
# The weight gradient of the same layers runs on savfi_conv3x3_wgrad_f32 (NCHW-native MFMA kernel, deterministic) when a
# map has >= 3000 output pixels and >= 16 input channels: 1.2-1.8x faster than MIOpen's igemm kernel + its two layout
# transposes there (tools/wgrad_bench.py, profiles/r01_wgrad_bench.jsonl); the deep 24x32 / 12x16 layers stay on MIOpen.
WGRAD_MIN_PIXELS = 3000
WGRAD_MIN_CI = 16
# Winograd form of the weight gradient (savfi_conv3x3_wgrad_wino_tasks_f32, F(3x3, 2x2)): 1.4-1.6x faster than the direct kernel
# on the large layers and 1.2-1.5x faster than MIOpen (grouped or not) on the deep 24x32 / 12x16 ones once a call carries enough
# work; below ~5 GFLOP the three launches (kernel + two reduction levels) are the cost and the old routing stays.
WGRAD_WINO = True
WGRAD_WINO_MIN_GFLOP = 5.0
WGRAD_WINO_MIN_PIXELS = 192


def _wgrad_wino(N, Ci, Co, Ho, Wo):
    # the Winograd form indexes a sample's channels with 28-bit element offsets (SAVFI_E_TOOBIG beyond): oversize layers fall back
    if Ci * (Ho + 2) * (Wo + 2) >= (1 << 28) or Co * Ho * Wo >= (1 << 28):
        return False
    return WGRAD_WINO and Ho * Wo >= WGRAD_WINO_MIN_PIXELS and 18e-9 * Ci * Co * Ho * Wo * N >= WGRAD_WINO_MIN_GFLOP


# Direct K x K convolution on split-bf16 MFMAs (savfi_convk_*: csrc/convk.hip, csrc/convk_wgrad.hip).  fp32-equivalent arithmetic
# (six bf16 products per fp32 product, fp32 accumulate; as close to fp64 as an fp32 fmaf chain, tools/bf16_split_probe.hip) at
# up to 2.4x the fp32 matrix rate.  Routing (tools/convk_bench.py, profiles/r03_convk_bench.txt):
#   5x5 / 7x7 (VoxelFlow, Super SloMo): always -- forward / data gradient 1.8-3x MIOpen's igemm kernels, weight gradient 1.4-1.7x;
#   3x3: where it beats the Winograd kernel -- layers of >= 64 -> 64 channels in whole 64-channel blocks on maps of >= 700 pixels
#        (220-240 vs 200-208 direct-equivalent TFLOP/s) and the <= 8-channel input layers -- or where a plugin asks for the
#        direct form because it amplifies Winograd rounding (VoxelFlow: `direct=True`).
CONVK = True
CONVK_3X3_MIN_PIXELS = 700


CONVK_WGRAD3_RING_MIN_PIXELS = 3000
CONVK_WGRAD3_RING_SMALL_MIN_PIXELS = 64
CONVK_WGRAD3 = True             # A/B: False = every 3 x 3 weight gradient on the Winograd form
CONVK_WGRAD3_RING = True        # A/B: False = no all-taps kernel (the tap-split kernel's rules alone)


def convk_wgrad_preferred(K, Ci, Co, Ho, Wo, direct=False, N=None):
    """Weight gradient of a stride-1 K x K layer on csrc/convk_wgrad.hip rather than the Winograd / MIOpen forms?  5x5 / 7x7 and
    `direct` layers always; 3x3 where the split-bf16 kernels measured faster than savfi_conv3x3_wgrad_wino:
    * >= 48 -> 48 channels on maps of >= 3000 pixels -- the all-taps kernel on the row ring (round 5; tools/wgrad3_forms_time.py,
      profiles/r05_wgrad3_forms.txt: 160-167 vs 181-184 us on 64 -> 64 @192x256 / 128 -> 128 @96x128, 82 vs 99 on 128 -> 64 @96x128, 57 vs 69 on
      64 -> 64 @96x128 at T = 4 x 2 samples; CAIN 192 -> 192 @96x160: 127 vs 164; the deep 24x32 / 12x16 layers stay on Winograd: 215 vs 180);
    * the wide shallow layers (<= 32 input channels: 89 vs 167 us for 6 -> 32 and 195 vs 252 us for 32 -> 32 at 384 x 512, T = 4)
      and >= 192 output channels on maps of >= 4096 pixels on the tap-split kernel (profiles/r03_convk_bench.jsonl)."""
    if not CONVK or K not in (3, 5, 7):
        return False
    if K != 3 or direct:
        return True
    if not CONVK_WGRAD3:
        return False
    if Ci >= 48 and Co >= 48 and Ho * Wo >= CONVK_WGRAD3_RING_MIN_PIXELS and CONVK_WGRAD3_RING:
        return True
    # ... and the small maps the Winograd form does not take either (N samples; CAIN at 64x64: 192 -> 192 @16x16, where MIOpen's
    # weight gradient is im2col + two GEMMs + col2im, 33 us in four launches against 12 + 5: config C1 45.5 -> 47.1 steps/s)
    if N is not None and Ci >= 48 and Co >= 48 and Ho * Wo >= CONVK_WGRAD3_RING_SMALL_MIN_PIXELS and CONVK_WGRAD3_RING \
            and not _wgrad_wino(N, Ci, Co, Ho, Wo):
        return True
    return (Ci <= 32 and Ho * Wo >= 16384) or (Co >= 192 and Ho * Wo >= 4096)


def _conv_geometry(w_shape, stride, padding, dilation, groups=1):
    """(K, pad) if the layer is a square K x K / stride 1 / undilated / ungrouped convolution with symmetric padding, else None.
    (The one parser of a layer's geometry: which K and pad a kernel family takes is said where the route is chosen, conv_route.)"""
    one = lambda v: v == 1 if isinstance(v, int) else all(t == 1 for t in v)
    K = int(w_shape[-1])
    if int(w_shape[-2]) != K or not one(stride) or not one(dilation) or groups != 1:
        return None
    pad = padding if isinstance(padding, int) else (padding[0] if padding[0] == padding[1] else -1)
    return (K, int(pad)) if pad >= 0 else None


# Winograd F(4x4, 3x3) (csrc/winograd4.h; round 6): the 3x3 layers of at most 512 -> 512 channels, wherever its launch fills the chip --
# measured against the direct split-bf16 kernel on one box (tools/r6/wino4_time.py deep|small convk, profiles/r06_wino4_vs_convk.txt;
# forward / data gradient in us, T = 4 x 2 samples): 64 -> 64 @192x256 95 / 94 vs 142 / 147, 128 -> 128 @96x128 94 / 92 vs 128 / 128,
# 256 -> 256 @48x64 118 / 115 vs 133 / 132, 64 -> 64 @137x236 N = 32 324 / 320 vs 385 / 393, 64 -> 64 @96x128 35 / 34 vs 47 / 46, 128 -> 128
# @48x64 (192 workgroups) 37 / 36 vs 42 / 42; with the reduction split over workgroups (from 256 channels): 512 -> 512 @24x32 138 / 141 vs
# 164 / 160, 256 -> 256 @24x32 46 / 44 vs 57 / 56, 512 -> 512 @12x16 64 / 62 (F(2x2): 53; direct: 107).  Below ~180 workgroups (of 2 per CU x
# 256 CUs = 512 slots) the direct kernel keeps the layer.
WINO4_MIN_WORKGROUPS = 180
WINO4_MIN_PIXELS = 400


@functools.lru_cache(maxsize=None)
def _conv3x3_name(Ci, Co, what):
    """Timer name of a savfi_conv3x3_* launch: 'conv3x3f4_*' for the layers the library runs on its F(4x4) kernel (by channel counts)."""
    f4 = int(_hip.lib().savfi_conv3x3_f4_workgroups(1, int(Ci), int(Co), 8, 8, 1, 0)) > 0
    return ("conv3x3f4_" if f4 else "conv3x3_") + what


@functools.lru_cache(maxsize=4096)
def wino4_workgroups(N, Ci, Co, H, W, pad, mode=0):
    """Workgroups savfi_conv3x3_* would launch on its F(4x4) kernel for this call; 0: the layer's channel counts keep it on F(2x2).
    (Cached per shape: the routing asks once per convolution call, and a 64 x 64 CAIN iteration is host-bound.)"""
    n = int(_hip.lib().savfi_conv3x3_f4_workgroups(int(N), int(Ci), int(Co), int(H), int(W), int(pad), int(mode)))
    return max(n, 0)


def wino4_launched_workgroups(N, Ci, Co, H, W, pad, mode=0):
    """The grid an F(4x4) launch of this call really has: ceil(tiles / 32) workgroups per sample, split and channel block (flat tile
    lists) -- routing keeps counting tile blocks, wino4_workgroups.  Not cached: it follows wino4_block_decode."""
    n = int(_hip.lib().savfi_conv3x3_f4_launched_workgroups(int(N), int(Ci), int(Co), int(H), int(W), int(pad), int(mode)))
    return max(n, 0)


@contextlib.contextmanager
def wino4_block_decode(on=True):
    """Test hook: inside the block, F(4x4) launches decode their tiles by 2^(5-s) x 2^s blocks (the grid wino4_workgroups counts) instead of
    flat tile lists.  Same results bit for bit; the previous setting comes back on exit."""
    prev = ctypes.c_int(0)
    _hip.check(_hip.lib().savfi_conv3x3_debug_f4_block_decode(1 if on else 0, ctypes.byref(prev)), "savfi_conv3x3_debug_f4_block_decode")
    try:
        yield
    finally:
        _hip.check(_hip.lib().savfi_conv3x3_debug_f4_block_decode(prev.value, None), "savfi_conv3x3_debug_f4_block_decode")


def _layer(x_shape, w_shape, stride, padding, dilation, groups=1):
    """(N, Ci, Co, H, W, K, pad) of a layer with a _conv_geometry on [N,C,H,W] maps, else None: what the threshold rules below take."""
    geo = _conv_geometry(w_shape, stride, padding, dilation, groups)
    if geo is None or len(x_shape) != 4:
        return None
    return (int(x_shape[0]), int(w_shape[-3]), int(w_shape[-4]), int(x_shape[2]), int(x_shape[3])) + geo


def _form2(N, Ci, Co, H, W, pad):
    """wino_form2 over integers."""
    n = wino4_workgroups(int(N), int(Ci), int(Co), int(H), int(W), int(pad))
    if n <= 0:
        return False
    # ... and on maps below ~400 pixels: a 12 x 16 map is 12 of a workgroup's 32 tiles, and the 36-point filter transform of a deep layer
    # (2.25x F(2x2)'s: 151 MB per 512 -> 512 layer, direction and inner step at T = 4) costs more than the kernel saves there:
    # 512 -> 512 @12x16, T = 4 x 2: 67 + 67 us + 92 us of transforms on F(4x4) against 53 + 52 + 41 on F(2x2)
    return n < WINO4_MIN_WORKGROUPS or (H + 2 * pad - 2) * (W + 2 * pad - 2) < WINO4_MIN_PIXELS


def _convk_admits(N, Ci, Co, H, W, K, pad, direct):
    """Forward and data gradient of a layer on the direct split-bf16 kernel?  K in (3, 5, 7), 0 <= pad <= K - 1."""
    if not CONVK or K not in (3, 5, 7) or pad > K - 1:
        return False
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    if Ho < 1 or Wo < 1 or Ci * H * W >= (1 << 29) or Co * Ho * Wo >= (1 << 29):
        return False
    if K != 3 or direct:
        return True
    if not (Ho * Wo >= CONVK_3X3_MIN_PIXELS and (Ci <= 8 or (Ci >= 64 and Co >= 64 and Co % 64 == 0))):
        return False
    # (the <= 8-channel input layers stay here: an F(4x4) chunk is 8 reduction channels, half of them padding for 6 -> 32)
    return Ci <= 8 or pad > 1 or not WINOGRAD_CONV or wino4_workgroups(N, Ci, Co, H, W, pad) < WINO4_MIN_WORKGROUPS


def _wino_admits(N, Ci, Co, H, W, K, pad, tasks, backward):
    """A direction of a layer on the Winograd kernels by its tile count?  K == 3, pad in (0, 1).  Shared weights: WINO_MIN_TILES_* and
    its batched variant; per-task weights: TASKS_MIN_TILES_*."""
    if not WINOGRAD_CONV or K != 3 or pad not in (0, 1):
        return False
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if Ho < 1 or Wo < 1 or H * W < 4:
        return False
    tiles = N * ((Ho + 1) // 2) * ((Wo + 1) // 2)
    if tasks:
        return tiles >= (TASKS_MIN_TILES_BWD if backward else TASKS_MIN_TILES_FWD)
    if N >= 2 and tiles >= (WINO_MIN_TILES_BWD_BATCHED if backward else WINO_MIN_TILES_FWD_BATCHED):
        return True
    return tiles >= (WINO_MIN_TILES_BWD if backward else WINO_MIN_TILES_FWD)


def _wgrad3_admits(N, Ci, Co, H, W, K, pad, tasks):
    """Weight gradient of a layer on savfi_conv3x3_wgrad*?  K == 3, pad in (0, 1); wherever its Winograd form runs (_wgrad_wino), else
    shared weights: WGRAD_MIN_CI, WGRAD_MIN_PIXELS and the fill of the 64-pixel segments; per-task weights: TASKS_WGRAD_MIN_PIXELS."""
    if not WINOGRAD_CONV or K != 3 or pad not in (0, 1):
        return False
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if Ho > 0 and Wo > 0 and _wgrad_wino(N, Ci, Co, Ho, Wo):
        return True
    if tasks:
        return Ho * Wo >= TASKS_WGRAD_MIN_PIXELS
    # the kernel works on 64-pixel row segments: a mostly empty last segment (CAIN's 160-wide maps: 83 % used) loses
    fill = Wo / (64.0 * ((Wo + 63) // 64)) if Wo > 0 else 0.0
    return Ci >= WGRAD_MIN_CI and Ho * Wo >= WGRAD_MIN_PIXELS and fill >= 0.85


Route = collections.namedtuple("Route", "K pad fwd dgrad wgrad")
_ATEN_ROUTE = Route(None, None, 'aten', 'aten', 'aten')


def conv_route(x_shape, w_shape, stride, padding, dilation, groups=1, direct=False, reflect=False):
    """Which kernels run a fused convolution of float32 maps on the device: the one place where that is decided, over integers (the knobs
    of this module are read at every call).  w_shape [Co,Ci,K,K]: shared weights, [T,Co,Ci,K,K]: per-task weights.  Route:
      fwd    'convk' (direct split-bf16), 'wino' (the Winograd form of the library's channel rule: F(4x4) up to 512 channels), 'wino2'
             (F(2x2) although the channels say F(4x4): wino_form2), 'aten';
      dgrad  the same on the filters transformed with the forward's, or 'conv3x3': the forward stayed on ATen but the backward thresholds
             admit the Winograd kernel, which then transforms its own filter (conv3x3 / conv3x3_tasks);
      wgrad  'convk' (csrc/convk_wgrad.hip), 'conv3x3' (savfi_conv3x3_wgrad*; Winograd or direct form: _wgrad_wino, in the launcher), 'aten';
      K, pad of the square / stride 1 / undilated / ungrouped layer; None where it is not one (every direction on ATen)."""
    layer = _layer(x_shape, w_shape, stride, padding, dilation, groups)
    if layer is None:
        return _ATEN_ROUTE
    N, Ci, Co, H, W, K, pad = layer
    tasks = len(w_shape) == 5
    fwd = dgrad = wgrad = 'aten'
    if _convk_admits(*layer, direct):
        fwd = dgrad = 'convk'
    else:
        if _wino_admits(*layer, tasks, False):
            fwd = 'wino2' if _form2(N, Ci, Co, H, W, pad) else 'wino'
        if _wino_admits(*layer, tasks, True):
            dgrad = fwd if fwd != 'aten' else 'conv3x3'
    # 5x5 / 7x7 layers and plugins that asked for the direct form: weight gradient on the split-bf16 kernel as well; a mirrored border
    # (shared weights, forward on the direct kernel: convk_reflect_eligible) exists there only
    if reflect or (K in (3, 5, 7) and pad <= K - 1 and (fwd == 'convk' or K == 3)
                   and convk_wgrad_preferred(K, Ci, Co, H + 2 * pad - K + 1, W + 2 * pad - K + 1, direct, N)):
        wgrad = 'convk'
    elif _wgrad3_admits(*layer, tasks):
        wgrad = 'conv3x3'
    return Route(K, pad, fwd, dgrad, wgrad)


def _f32_map(x):
    """The fused kernels take float32 [N,C,H,W] maps on the device: the precondition of every route but ATen's."""
    return bool(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4)


def _layer_of(x, weight, stride, padding, dilation, groups=1):
    """_layer of tensors, for the predicates that ask one threshold rule of conv_route on its own; None also where x is no float32 map."""
    return _layer(x.shape, weight.shape, stride, padding, dilation, groups) if _f32_map(x) else None


def convk_eligible(x, weight, stride, padding, dilation, groups=1, direct=False):
    """Does this convolution (and its data gradient) run on the direct split-bf16 kernel?  weight [Co,Ci,K,K] or [T,Co,Ci,K,K]."""
    layer = _layer_of(x, weight, stride, padding, dilation, groups)
    return layer is not None and _convk_admits(*layer, direct)


def wino_form2(x, weight, pad):
    """Does a layer on the Winograd route run the F(2x2) kernel although its channel counts would put it on F(4x4)?  Yes where the F(4x4)
    launch would not fill the chip (small maps: the 64 x 64 fixtures, config C1): F(2x2) splits its reduction from 128 workgroups down and
    rounds 5x finer (an Adam-type inner rule turns F(4x4)'s rounding into flipped steps of the elements whose gradient is rounding
    noise: CAIN 64 x 64 + Adam).  The filters of such a layer are kind 'wino2' (savfi_conv3x3_*_form_f32 / bit 1 of `mode`)."""
    return _form2(x.shape[0], weight.shape[-3], weight.shape[-4], x.shape[2], x.shape[3], pad)


def conv3x3_eligible(x, weight, stride, padding, dilation, groups, backward=False):
    """Do the Winograd thresholds admit this shared-weight layer (whatever the direct kernel says of it)?"""
    layer = _layer_of(x, weight, stride, padding, dilation, groups)
    return layer is not None and _wino_admits(*layer, False, backward)


def conv3x3_wgrad_eligible(x, weight, stride, padding, dilation, groups):
    layer = _layer_of(x, weight, stride, padding, dilation, groups)
    return layer is not None and _wgrad3_admits(*layer, False)


# Weight gradients on a side stream.  In the backward of a first-order support pass the data-gradient chain (layer L's gx
# feeds layer L-1) is the critical path; the weight gradients hang off it and are only consumed by the update after the whole
# backward.  While overlap is switched on (per thread, by the caller that owns the autograd.grad() call) every fused conv
# op remembers the side stream at FORWARD time (its backward runs on autograd's device thread, where a thread-local flag
# would not be visible) and queues its weight gradient there; the caller joins before it touches the gradients.
_WG = threading.local()


_WG_SIDE = {}              # compute stream handle -> its side stream (persistent: streams and the library handles bound
_WG_LOCK = threading.Lock()    # to them are not created per pass or per worker thread)


def set_weight_gradient_overlap(on):
    _WG.stream = None
    if on:
        key = (torch.cuda.current_device(), _hip.current_stream())
        with _WG_LOCK:
            side = _WG_SIDE.get(key)
            if side is None:
                side = _WG_SIDE[key] = torch.cuda.Stream()
        _WG.stream = side
    _WG.on = bool(on)
    _WG.uses = {}          # id(weight) -> [number of fused conv ops that read it in this pass]


def _weight_use_counter(w):
    """A weight read by more than one op of the pass (the unfused support triplets, a plugin that shares layers) gets
    its contributions ADDED by autograd on the compute stream as soon as the second one is returned - before the caller's
    join.  Such weights keep their gradient on the compute stream (decided in backward, when the count is final)."""
    holder = _WG.uses.setdefault(id(w), [0])
    holder[0] += 1
    return holder


def weight_gradient_stream():
    return getattr(_WG, 'stream', None) if getattr(_WG, 'on', False) else None


def join_weight_gradients():
    """Make the current stream wait for every weight gradient queued on its side stream."""
    if not _WG_SIDE:
        return
    with _WG_LOCK:
        side = _WG_SIDE.get((torch.cuda.current_device(), _hip.current_stream()))
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)


def _aten_conv(x, w, stride, padding, dilation, groups, T):
    """The layers no savfi kernel takes, on ATen (MIOpen), result [N,Co,Ho,Wo] contiguous.  Per-task weights (T not None, x contiguous):
    ONE grouped convolution on small maps -- [n*T,C,H,W] viewed as [n,T*C,H,W] with groups = T --, one call per task on large ones."""
    if T is None:
        z = torch.nn.functional.conv2d(x, w, None, stride, padding, dilation, groups)
        return z if z.is_contiguous() else z.contiguous()
    N, Ci, H, W = x.shape
    Co, n = w.shape[1], N // T
    if _grouped_ok(x):
        z = torch.nn.functional.conv2d(x.view(n, T * Ci, H, W), w.reshape(T * Co, Ci, *w.shape[3:]), None, stride, padding, dilation, T)
        if not z.is_contiguous():
            z = z.contiguous()
    else:           # large map, no savfi kernel (5x5 / 7x7 / strided): one MIOpen call per task, results interleaved
        xs = x.view(n, T, Ci, H, W)
        z = torch.stack([torch.nn.functional.conv2d(xs[:, t], w[t], None, stride, padding, dilation) for t in range(T)], 1)
    return z.view(N, Co, z.shape[-2], z.shape[-1])


def _aten_conv_backward(gz, x, w, stride, padding, dilation, groups, T, need_x, need_w):
    """(gx, gw) of _aten_conv (None where not asked for)."""
    pair = lambda v: [v, v] if isinstance(v, int) else list(v)
    conf = (None, pair(stride), pair(padding), pair(dilation), False, [0, 0])
    if T is None:
        gx, gw, _ = torch.ops.aten.convolution_backward(gz, x, w, *conf, groups, [need_x, need_w, False])
        return (gx if need_x else None), (gw if need_w else None)
    N, Ci, H, W = x.shape
    Co, n = w.shape[1], N // T
    Ho, Wo = gz.shape[2:]
    if _grouped_ok(x):
        gx, gw, _ = torch.ops.aten.convolution_backward(gz.view(n, T * Co, Ho, Wo), x.view(n, T * Ci, H, W), w.reshape(T * Co, Ci, *w.shape[3:]),
                                                        *conf, T, [need_x, need_w, False])
        return (gx.contiguous().view(N, Ci, H, W) if need_x else None), (gw.view(w.shape) if need_w else None)
    gzs, xs = gz.view(n, T, Co, Ho, Wo), x.view(n, T, Ci, H, W)
    per = [torch.ops.aten.convolution_backward(gzs[:, t].contiguous(), xs[:, t].contiguous(), w[t], *conf, 1, [need_x, need_w, False])
           for t in range(T)]
    return (torch.stack([p[0] for p in per], 1).view(N, Ci, H, W) if need_x else None), (torch.stack([p[1] for p in per], 0) if need_w else None)


def _conv_forward(ctx, x, w, b, stride, padding, dilation, groups, slope, direct, cache, reflect, in_slope, defer, out_unit16, T, pool=False):
    """The forward of both fused convolutions.  T = None: shared weights w [Co,Ci,K,K], b [Co] (_ConvBiasAct: `groups`, the module-owned
    filter `cache`, the mirrored border `reflect`); else per-task weights w [T,Co,Ci,K,K], b [T,Co], sample s on task s % T
    (_ConvBiasActTasks: `out_unit16`).  The route is decided here, once, and kept on ctx for the backward."""
    # conv -> ReLU -> conv chains (model_utils.MetaSequential): `defer` -- the consumer of y applies THIS layer's activation
    # derivative (the gradient arriving here is already d/dz); `in_slope` -- x is the activated output of a layer that deferred
    # its derivative to this one: it is folded into this layer's data gradient (kernel epilogue where there is one)
    if T is not None:
        x = x.contiguous()          # (the grouped ATen call views it; the shared form leaves a strided x to ATen and the launchers)
    route = conv_route(x.shape, w.shape, stride, padding, dilation, groups, direct, reflect) if _f32_map(x) else _ATEN_ROUTE
    K, pad = route.K, route.pad
    Co, Ci = w.shape[-4], w.shape[-3]
    need_x = bool(ctx.needs_input_grad[0])
    assert not reflect or route.fwd == 'convk', "mirrored borders: direct kernel only"
    # out_unit16: the result's MEMORY is unit-major (its only consumer is FunctionSepconvPair(taps_unit16=True)); the cotangent that comes back
    # is laid out like the shape says, so nothing changes in backward.  The caller has asked conv3x3_unit16_supported.
    # out_unit16 == 2: the cotangent that comes back is unit-major as well (FunctionSepconvPair(..., grads_unit16=True)): only the
    # data gradient may be asked for (the caller has checked conv3x3_in_unit16_supported and that w, b carry no gradient)
    assert not out_unit16 or (slope == 1.0 and not defer and conv3x3_unit16_supported(x, w, pad)), \
        "unit-major output: Winograd route (not the F(2x2) form of a small launch), no activation"
    ctx.u_bwd = None
    if route.fwd == 'convk':
        u_fwd, ctx.u_bwd = filter_lookup('convk', w, True, need_x, cache)
        z = convk_tasks_pre(x, u_fwd, T or 1, Ci, Co, K, b, 0, slope, pad, direct, reflect)
    elif route.fwd in ('wino', 'wino2'):
        # both filter transforms of this layer in one launch: the data gradient of the same step will want the other one
        u_fwd, ctx.u_bwd = filter_lookup(route.fwd, w, True, need_x and route.dgrad == route.fwd, cache)
        if pool:          # the 2 x 2 average of z from the kernel's output stage where the launch has one for it, else from the pooling kernel
            z, pooled = conv3x3_tasks_pre_pool(x, u_fwd, T or 1, Ci, Co, b, slope, pad, f2=route.fwd == 'wino2')
        else:
            z = conv3x3_tasks_pre(x, u_fwd, T or 1, Ci, Co, b, 0, slope, pad, out_unit16=bool(out_unit16), f2=route.fwd == 'wino2')
    else:
        z = _aten_conv(x, w, stride, padding, dilation, groups, T)
        if b is not None or slope != 1.0:
            zb = b if b is not None else torch.zeros(w.shape[:-3], dtype=z.dtype, device=z.device)
            _hip.require_cuda(z, zb)
            rows, chans, hw = z.shape[0] // (T or 1), (T or 1) * Co, z.shape[2] * z.shape[3]      # [n*T,Co] maps = n rows of T*Co channels
            _hip.call("bias_act_fwd", "savfi_bias_act_fwd_f32", z, zb, rows, chans, hw, slope)
    ctx.route, ctx.T, ctx.conf = route, T, (stride, padding, dilation, groups, slope)
    ctx.in_slope, ctx.defer, ctx.reflect, ctx.gy_unit16 = in_slope, bool(defer), bool(reflect), int(out_unit16) == 2
    ctx.direct, ctx.cache, ctx.w_version, ctx.has_bias = direct, cache, w._version, b is not None
    ctx.wg_stream = weight_gradient_stream() if x.is_cuda else None
    ctx.wg_uses = _weight_use_counter(w) if ctx.wg_stream is not None else None
    ctx.save_for_backward(x, w, z)
    if out_unit16:
        tag_layout(z, UNIT16)           # the tensor's shape does not say how its memory is laid out: its consumer checks the tag
    if pool:
        return z, (pooled if route.fwd in ('wino', 'wino2') else _avgpool2x2_fwd_launch(z))
    return z


def _conv_backward(ctx, gy):
    """(gx, gw, gb) of _conv_forward, on the route it kept: bias / activation backward, data gradient, weight gradient."""
    x, w, y = ctx.saved_tensors
    stride, padding, dilation, groups, slope = ctx.conf
    route, T, direct = ctx.route, ctx.T, ctx.direct
    K, pad = route.K, route.pad
    Co, Ci = w.shape[-4], w.shape[-3]
    N, _, Ho, Wo = y.shape
    tasks = T or 1
    need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
    # the filter packed / transformed at forward time is only valid for the weight version the forward saw
    u_bwd = ctx.u_bwd if w._version == ctx.w_version else None
    ctx.u_bwd = None
    if T is not None:
        # the cotangent's memory layout is a contract between two autograd functions that its shape cannot carry: the producer tags the
        # tensor, and anything in between (a hook, an accumulation of two consumers' gradients, a clone) loses or contradicts the tag
        require_layout(gy, UNIT16 if ctx.gy_unit16 else None, "the cotangent of conv_bias_act_tasks(out_unit16=%d)" % (2 if ctx.gy_unit16 else 1))
    gy = gy.contiguous()
    if ctx.gy_unit16:
        assert not need_w and not need_b and slope == 1.0 and ctx.in_slope is None and route.fwd == 'wino', \
            "a unit-major cotangent: data gradient of the Winograd route only"
        if not need_x:
            return None, None, None
        if u_bwd is None:
            u_bwd = filter_lookup('wino', w, False, True, None)[1]
        return conv3x3_dgrad_in_unit16(gy, u_bwd, T, Ci, Co, pad), None, None
    identity = slope == 1.0 or ctx.defer     # no activation, or its derivative already applied by the consumer: gz is gy itself,
    gz = gy if identity else torch.empty_like(gy)        # only the bias gradient is computed
    mask, mslope = (x, ctx.in_slope) if (ctx.in_slope is not None and need_x) else (None, 1.0)
    wgrad = route.wgrad if need_w else None
    # a weight read by one op of the pass only: its gradient beside the data-gradient chain (decided here: the use count is final now)
    side = ctx.wg_stream if (ctx.wg_stream is not None and ctx.wg_uses[0] == 1) else None
    # the bias gradient rides on the weight gradient's read of gz where that is the all-taps direct kernel -- or, per-task weights only, the
    # Winograd form -- and this function has nothing else to do with the cotangent (no activation, or its derivative left to the consumer):
    # one pass over the map and two launches less per layer
    # (not beside the Winograd weight gradient on the SIDE stream: a bias gradient autograd consumes on the compute stream -- stacked
    # biases, a bias shared between ops -- must be produced there; the side-stream guard counts uses of the WEIGHT only)
    fuse_b = bool(need_b and identity and (
        (wgrad == 'convk' and convk_wgrad_tasks_sums_bias(x.shape, Co, tasks, K, pad, direct))
        or (wgrad == 'conv3x3' and T is not None and side is None and conv3x3_wgrad_tasks_sums_bias(x.shape, Co, T, pad))))
    gb = torch.empty(w.shape[:-3], dtype=gy.dtype, device=gy.device) if (need_b and not fuse_b) else None
    if gb is not None or not identity:
        rows, chans = N // tasks, tasks * Co                # [n*T,Co] maps = n rows of T*Co channels
        scratch = (torch.empty(_workspace_floats("savfi_bias_act_scratch_floats", rows, chans, Ho * Wo), dtype=gy.dtype, device=gy.device)
                   if gb is not None else None)
        _hip.call("bias_act_bwd", "savfi_bias_act_bwd_f32", gy, gy if identity else y, None if identity else gz, gb, scratch,
                  rows, chans, Ho * Wo, 1.0 if identity else slope)
    gx = gw = None
    if need_x and route.dgrad == 'convk':
        if u_bwd is None:
            u_bwd = filter_lookup('convk', w, False, True, ctx.cache)[1]
        if ctx.reflect:     # gradient of the mirrored (padded) extent = the full data gradient of the unpadded convolution, folded
            gx = reflect_pad_bwd(convk_tasks_pre(gz, u_bwd, tasks, Ci, Co, K, None, 1, 1.0, 0, direct), pad)
        else:
            gx = convk_tasks_pre(gz, u_bwd, tasks, Ci, Co, K, None, 1, 1.0, pad, direct, mask=mask, mask_slope=mslope)
            mask = None
    elif need_x and route.dgrad in ('wino', 'wino2') and u_bwd is not None:
        gx = conv3x3_tasks_pre(gz, u_bwd, tasks, Ci, Co, None, 1, 1.0, pad, mask=mask, mask_slope=mslope, f2=route.dgrad == 'wino2')
        mask = None
    elif need_x and route.dgrad != 'aten':
        # the forward stayed on ATen ('conv3x3'), or the weight has changed since: the entry points that transform the filter themselves
        # (shared weights: the form is the library's channel rule; per-task weights keep the forward's)
        gx = conv3x3(gz, w, None, 1, 1.0, pad) if T is None else conv3x3_tasks(gz, w, None, 1, 1.0, pad, f2=route.dgrad == 'wino2')
    if wgrad == 'convk':
        gw = convk_wgrad_tasks(x, gz, tasks, K, pad, direct, ctx.reflect, want_bias=fuse_b)
        if fuse_b:
            gw, gb = gw
        if T is None:
            gw, gb = gw[0], (gb[0] if fuse_b else gb)
    # the side stream: the shared form also runs the ATen weight gradient there, the per-task form the savfi one only
    on_side = side is not None and (wgrad == 'conv3x3' or (wgrad == 'aten' and T is None))
    if on_side:
        # gz was produced on this stream just above: the side stream picks up from here
        ready = torch.cuda.Event()
        ready.record()
        side.wait_event(ready)
    if wgrad == 'conv3x3':
        where = dict(stream=side.cuda_stream, extra_stream=side) if on_side else {}
        if T is None:
            gw = conv3x3_wgrad(x, gz, pad, **where)
        else:
            gw = conv3x3_wgrad_tasks(x, gz, T, pad, want_bias=fuse_b, **where)
            if fuse_b:
                gw, gb = gw
    elif wgrad == 'aten' and on_side:
        with torch.cuda.stream(side):
            gw = _aten_conv_backward(gz, x, w, stride, padding, dilation, groups, None, False, True)[1]
        gw.record_stream(torch.cuda.current_stream())      # consumed on this stream after the caller's join
    if on_side:
        x.record_stream(side)
        gz.record_stream(side)
    aten_x, aten_w = bool(need_x and route.dgrad == 'aten'), wgrad == 'aten' and not on_side
    if aten_x or aten_w:
        gx2, gw2 = _aten_conv_backward(gz, x, w, stride, padding, dilation, groups, T, aten_x, aten_w)
        gx, gw = (gx2 if aten_x else gx), (gw2 if aten_w else gw)
    if mask is not None and gx is not None:      # a route without the fused epilogue: the deferred derivative as its own pass
        gx = mask_by_activation(gx, mask, mslope)
    return gx, gw, gb


class _ConvBiasAct(torch.autograd.Function):
    """y = act(conv2d(x, w) + b).  Large 3x3 convolutions run on the savfi Winograd/MFMA kernel with bias and
    activation in its epilogue; the others stay on MIOpen with the bias add and activation as ONE in-place kernel
    on the output.  The backward computes act' * gy and the bias gradient in one pass, then the data gradient
    (savfi kernel or MIOpen) and the weight gradient (MIOpen).  First-order only (the backward is not
    differentiable): callers use the unfused ops under --second_order."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, dilation, groups, slope, direct=False, cache=None, reflect=False, in_slope=None, defer=False):
        return _conv_forward(ctx, x, w, b, stride, padding, dilation, groups, slope, direct, cache, reflect, in_slope, defer, 0, None)

    @staticmethod
    def backward(ctx, gy):
        return _conv_backward(ctx, gy) + (None,) * 10


# --------------------------------------------------------------------------------------------
# The same fused conv for T tasks adapted in LOCKSTEP (reference: the sequential task loop meta_learning_system.py:366).
# Activations [n*T, C, H, W] are ordered sample-major (sample s = j*T + t belongs to task t), fast weights are stacked
# [T, Co, Ci, kh, kw] / [T, Co]: one launch per layer for the whole meta-batch.  Large-enough 3x3 layers run on the savfi
# kernels with a task index on the grid (per-task filter sets); everything else is ONE grouped MIOpen convolution --
# [n*T, C, H, W] viewed as [n, T*C, H, W] with groups = T, which the sample-major order makes a free view in and out.
# --------------------------------------------------------------------------------------------
# Thresholds from tools/tasks_bench.py (profiles/r02_tasks_bench_*.jsonl; T = 4 tasks x 2 samples).  Forward / data gradient:
# the savfi kernel wins or ties everywhere down to 24x32 maps (against 4 MIOpen calls: 1.1-2x); ONE grouped MIOpen call is
# ~15 % ahead on the 24x32 / 12x16 layers only (2 % of a step), not worth a second code path.  Weight gradient: the savfi
# kernel works on 64-pixel row segments and loses on maps under ~3000 px (512->512 @12x16: 311 us vs 111 us grouped);
# MIOpen's grouped weight gradient collapses on LARGE maps (10.5 ms at 384x512), so those always stay here, whatever Ci.
TASKS_MIN_TILES_FWD = 1          # N * ceil(Ho/2) * ceil(Wo/2) tiles over all tasks
TASKS_MIN_TILES_BWD = 1
TASKS_WGRAD_MIN_PIXELS = 3000


def conv3x3_tasks_eligible(x, weight, stride, padding, dilation, backward=False):
    layer = _layer_of(x, weight, stride, padding, dilation)
    return layer is not None and _wino_admits(*layer, True, backward)


def conv3x3_wgrad_tasks_eligible(x, weight, stride, padding, dilation):
    layer = _layer_of(x, weight, stride, padding, dilation)
    return layer is not None and _wgrad3_admits(*layer, True)


def _conv3x3_out(N, Ci, Co, H, W, pad, mode):
    """(shape of the result, flops) of a savfi_conv3x3_* launch on an [N,*,H,W] map; mode 0: forward, 1: data gradient (of the cotangent)."""
    grow = 2 * (pad if mode == 0 else 2 - pad) - 2
    Ho, Wo = H + grow, W + grow
    return (N, Co if mode == 0 else Ci, Ho, Wo), 18.0 * Ci * Co * N * (Ho * Wo if mode == 0 else H * W)


def conv3x3_tasks(x, weight, bias=None, mode=0, slope=1.0, pad=1, f2=False):
    """savfi_conv3x3_tasks_f32 without autograd: weight [T,Co,Ci,3,3], bias [T,Co] or None; sample n uses task n % T.  f2: the F(2x2) form."""
    fbit = 2 if f2 else 0
    x, weight = x.contiguous(), weight.contiguous()
    _hip.require_cuda(x, weight)
    N, _, H, W = x.shape
    T, Co, Ci = weight.shape[:3]
    assert N % T == 0 and tuple(weight.shape[3:]) == (3, 3) and x.shape[1] == (Ci if mode == 0 else Co), (x.shape, weight.shape, mode)
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, mode)
    ws = torch.empty(_workspace_floats("savfi_conv3x3_tasks_workspace_floats", N, T, Ci, Co, H, W, int(pad), mode | fbit), dtype=x.dtype, device=x.device)
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _hip.call(_conv3x3_name(Ci, Co, "fwd" if mode == 0 else "bwd_data"), "savfi_conv3x3_tasks_f32", x, weight, bias, out, ws,
              N, T, Ci, Co, H, W, int(pad), mode | fbit, float(slope), flops=flops)
    return out


# --------------------------------------------------------------------------------------------
# The filter store: where a fused convolution gets its packed ('convk') or Winograd-transformed ('wino', 'wino2') filters from.
#
# The fused kernels read a weight through such a copy; made per layer and pass that is 270 launches of ~9 us in a SepConv meta-iteration,
# 760 in a CAIN one (profiles/r03_*_one_iteration.txt).  filter_lookup therefore asks three stores before it launches:
#   the module's cache: a module's OWN parameter is read in every support and target pass of a first-order meta-iteration (SepConv's
#     Subnets: 11 passes) and only the outer optimizer step changes it.  The dict is OWNED BY THE MODULE (MetaConv2dLayer passes its own):
#     it dies with the module, so a parameter of a later module that happens to reuse the address can never alias an entry.
#     refresh_module_filters re-makes the entries of all modules after that step in one launch per kind.
#   the prepacked filters: the fast weights of a step are born together in an update (mt_update, mt_scale).  The first step records which
#     of its outputs were packed, and how (the "plan" of that list of shapes); from then on every update packs those outputs straight away
#     with one launch per kind (filters_after_update).  An entry keeps its weight tensor alive, so a data pointer cannot come back as another
#     tensor while the entry exists; the weight's version is part of the match.
#   the constant weights: long-lived tensors that are no module's parameter (sepconv/model.py: the four sub-networks' own parameters
#     stacked into one task-batched layer; rebuilt when a parameter changes) are registered, and their filters are made once per tensor,
#     kind and stream.  Keyed on the data pointer of a tensor the registry keeps alive, so the pointer cannot be recycled meanwhile.
# While a hipGraph is captured, filters that live outside the capture are neither read nor stored: a replay runs no Python, so it must
# recompute the filters from the live weights (a kernel captured on a cached filter would read the transform of an old weight after the
# next in-place step).  The module's cache and the constant weights skip while capturing.  The prepacked filters and the plan do not:
# graph_inner_loop calls filters_after_update INSIDE the capture, so the many-layer launch and the convolutions that read its slices are
# nodes of one graph.  The state is shared by the per-task threads of --task_streams (a key that holds device memory names its stream).
# --------------------------------------------------------------------------------------------
PREPACK = True
_FILTER_CACHE_PER_MODULE = 6
_CONST_WEIGHTS_MAX = 64     # a model that goes away without unregistering leaves its entries behind: oldest out (16 per SepConv net and stream)
_pack_plans = {}            # tuple of the update's weight shapes -> {index: [kind, fwd, bwd]}
_last_update = None         # (signature, {data_ptr: index}, outputs) of the newest update
_prepacked = {}             # (kind, data_ptr) -> (weight, version, filters_fwd, filters_bwd)
_const_weights = {}         # data_ptr -> [weight, version, {(kind, stream): [filters_fwd, filters_bwd]}]
_const_weights_lock = threading.Lock()      # --task_streams: the per-task Python threads register / evict concurrently

# what the store asks of the process, through these names at call time (a host test puts its own in their place)
_on_device, _capturing, _raw_stream = (lambda t: t.is_cuda), torch.cuda.is_current_stream_capturing, _hip.current_stream

# One descriptor per kind, in the order the many-layer launches are issued.  form: None for the direct kernel's packed bf16 triples, whose
# entry points take K where those of the Winograd transforms take the form (bit 1 of the C ABI's `mode`; 0: by the library's channel rule,
# 2: F(2x2) whatever the channel counts).  floats: the size query of one filter; timer: the name of the single-layer launch, with "_multi"
# that of the many-layer launch; single, multi: their C entry points.
FilterKind = collections.namedtuple('FilterKind', 'form floats timer single multi')
_WINO = ("savfi_conv3x3_filter_floats", "conv3x3_filters", "savfi_conv3x3_filters_form_f32", "savfi_conv3x3_filters_multi_form_f32")
_KINDS = {'convk': FilterKind(None, "savfi_convk_filter_floats", "convk_filters", "savfi_convk_filters_f32", "savfi_convk_filters_multi_f32"),
          'wino': FilterKind(0, *_WINO), 'wino2': FilterKind(2, *_WINO)}


def _filter_shape(weight):
    """(T, Co, Ci, K) of a weight [Co,Ci,K,K] (T = 1) or [T,Co,Ci,K,K]."""
    T, Co, Ci = (1,) + tuple(weight.shape[:2]) if weight.dim() == 4 else tuple(weight.shape[:3])
    return int(T), int(Co), int(Ci), int(weight.shape[-1])


def _filter_floats(k, T, Ci, Co, K, mode):
    """Floats of one filter of kind k; mode 0: forward, 1: data gradient."""
    return _workspace_floats(k.floats, T, Ci, Co, *((K, mode) if k.form is None else (mode | k.form,)))


def _make_filters(kind, weight, fwd, bwd):
    """The single-layer launch: (filters_fwd, filters_bwd) of `weight`, both in ONE launch; None where not wanted."""
    k = _KINDS[kind]
    T, Co, Ci, K = _filter_shape(weight)
    us = [torch.empty(_filter_floats(k, T, Ci, Co, K, mode), dtype=torch.float32, device=weight.device) if want else None
          for mode, want in ((0, fwd), (1, bwd))]
    # (a direction that is not wanted goes to the C ABI as NULL)
    _hip.call(k.timer, k.single, weight, us[0], us[1], T, Ci, Co, K if k.form is None else k.form, stream=_raw_stream())
    return us[0], us[1]


def _filters_multi(kind, jobs):
    """The many-layer launch: [(weight, want_fwd, want_bwd)] -> [(filters_fwd, filters_bwd)] with ONE launch per 56 (layer, mode) jobs; the
    results are slices of one buffer, each rounded up to 64 floats (256-byte aligned)."""
    if not jobs:
        return []
    k, n = _KINDS[kind], len(jobs)
    IA = ctypes.c_int * n
    aT, aCi, aCo, aK = IA(), IA(), IA(), IA()
    cuts, total = [], 0
    for j, (w, f, b) in enumerate(jobs):
        T, Co, Ci, K = aT[j], aCo[j], aCi[j], aK[j] = _filter_shape(w)
        nf, nb = ((_filter_floats(k, T, Ci, Co, K, mode) + 63) // 64 * 64 if want else 0 for mode, want in ((0, f), (1, b)))
        cuts.append((total, total + nf, total + nf + nb))
        total += nf + nb
    flat = torch.empty(total, dtype=torch.float32, device=jobs[0][0].device)
    made = [((flat[start:mid] if mid > start else None), (flat[mid:end] if end > mid else None)) for start, mid, end in cuts]
    _hip.call(k.timer + "_multi", k.multi, _hip.ptr_array([w for w, _, _ in jobs]), _hip.ptr_array([tf for tf, _ in made]),
              _hip.ptr_array([tb for _, tb in made]), aT, aCi, aCo, aK if k.form is None else IA(*([k.form] * n)), n, stream=_raw_stream())
    return made


_ModuleKey = collections.namedtuple('_ModuleKey', 'kind ptr version shape device stream')


def _module_key(kind, weight):
    """The key of a module's cache (a plain tuple: it is built on every lookup; _ModuleKey names its fields)."""
    return (kind, weight.data_ptr(), weight._version, tuple(weight.shape), weight.device.index, _raw_stream())


def filter_lookup(kind, weight, fwd, bwd, cache=None):
    """(filters_fwd, filters_bwd) of `weight` ([Co,Ci,K,K] or [T,Co,Ci,K,K]) for the kernels of `kind`; an entry is None when not asked
    for.  `cache`: the dict of the module whose own parameter `weight` is, None for every other weight.  The first level that answers wins:

    1. The module's cache -- only with `cache`, and not while capturing.  Keyed (kind, data pointer, version, shape, device, stream), at
       most _FILTER_CACHE_PER_MODULE entries, oldest out.  An entry that lacks a wanted direction is made again by the levels below with
       the wanted directions plus those it held, and becomes the newest; only the wanted directions are returned.
    2. The prepacked filters of the newest update -- keyed (kind, data pointer); a hit needs the same version, the same shape and EVERY
       wanted direction, else it is a miss.  Also while capturing (see above).
    3. The registered constant weights -- not while capturing.  An entry is valid for the version and shape it was registered with; its
       filters are kept per (kind, stream), only the missing directions are made, both are kept.
    4. A single-layer launch.  If the weight is an output of the newest update, the plan of that update learns it first."""
    wanted, key = (fwd, bwd), None
    if cache is not None and not _capturing():                                      # 1
        key = _module_key(kind, weight)
        hit = cache.get(key)
        if hit is not None:
            if (hit[0] is not None or not fwd) and (hit[1] is not None or not bwd):
                return (hit[0] if fwd else None), (hit[1] if bwd else None)
            fwd, bwd = fwd or hit[0] is not None, bwd or hit[1] is not None
    weight = weight.contiguous()
    _hip.require_cuda(weight)
    assert weight.shape[-2] == weight.shape[-1] and (kind == 'convk' or weight.shape[-1] == 3) and (fwd or bwd), (kind, weight.shape)
    made = _prepacked_filters(kind, weight, fwd, bwd)                               # 2
    if made is None:
        made = _const_filters(kind, weight, fwd, bwd)                               # 3
    if made is None:
        _learn_plan(kind, weight, fwd, bwd)                                         # 4
        made = _make_filters(kind, weight, fwd, bwd)
    if key is not None:
        cache.pop(key, None)
        while len(cache) >= _FILTER_CACHE_PER_MODULE:
            cache.pop(next(iter(cache)))
        cache[key] = made
    return (made[0] if wanted[0] else None), (made[1] if wanted[1] else None)


def convk_filters(weight, fwd=True, bwd=True):
    """savfi_convk_filters_f32: weight [T,Co,Ci,K,K] (or [Co,Ci,K,K]) packed as bf16 triples in MFMA fragment order for the
    forward pass and / or the data gradient of the direct K x K convolution, in one call.  Returns (p_fwd, p_bwd)."""
    return filter_lookup('convk', weight, fwd, bwd)


def conv3x3_filters(weight, fwd=True, bwd=True, f2=False):
    """savfi_conv3x3_filters_form_f32: the Winograd transforms of weight [T,Co,Ci,3,3] (or [Co,Ci,3,3]) for the forward pass and / or
    the data gradient, in ONE launch.  Returns (u_fwd, u_bwd); an entry is None when not asked for.  f2: the F(2x2) form whatever the
    channel counts (kind 'wino2': wino_form2) -- such filters go with conv3x3_tasks_pre(..., f2=True) only."""
    return filter_lookup('wino2' if f2 else 'wino', weight, fwd, bwd)


def _prepacked_filters(kind, weight, fwd, bwd):
    hit = _prepacked.get((kind, weight.data_ptr())) if _prepacked else None
    if hit is None or hit[1] != weight._version or hit[0].shape != weight.shape or (fwd and hit[2] is None) or (bwd and hit[3] is None):
        return None
    return (hit[2] if fwd else None), (hit[3] if bwd else None)


def _const_filters(kind, weight, fwd, bwd):
    e = _const_weights.get(weight.data_ptr()) if _const_weights else None
    if e is None or e[1] != weight._version or e[0].shape != weight.shape or _capturing():
        return None
    have = e[2].setdefault((kind, _raw_stream()), [None, None])
    need_f, need_b = fwd and have[0] is None, bwd and have[1] is None
    if need_f or need_b:
        pf, pb = _make_filters(kind, weight, need_f, need_b)
        if need_f:
            have[0] = pf
        if need_b:
            have[1] = pb
    return (have[0] if fwd else None), (have[1] if bwd else None)


def _learn_plan(kind, weight, fwd, bwd):
    """A layer makes its own filters from `weight`: if that is an output of the newest update, the plan of that update learns it.  The
    first kind seen for an output stays; directions are added for that kind only."""
    if _last_update is None:
        return
    sig, index, _ = _last_update
    i = index.get(weight.data_ptr())
    if i is None or tuple(weight.shape) != sig[i]:
        return
    entry = _pack_plans.setdefault(sig, {}).get(i)
    if entry is None:
        _pack_plans[sig][i] = [kind, bool(fwd), bool(bwd)]
    elif entry[0] == kind:
        entry[1], entry[2] = entry[1] or bool(fwd), entry[2] or bool(bwd)


def register_const_weight(w):
    with _const_weights_lock:
        while len(_const_weights) >= _CONST_WEIGHTS_MAX:
            _const_weights.pop(next(iter(_const_weights)), None)
        _const_weights[w.data_ptr()] = [w, w._version, {}]
    return w


def unregister_const_weight(w):
    with _const_weights_lock:
        _const_weights.pop(w.data_ptr(), None)


def filters_after_update(outs):
    """Called with the fast weights an update just produced: pack / transform the ones the plan of this list names, one many-layer
    launch per kind.  What the previous update prepared is dropped in any case."""
    global _last_update
    _prepacked.clear()
    if not PREPACK or not outs or not _on_device(outs[0]):
        _last_update = None
        return
    sig = tuple(tuple(o.shape) for o in outs)
    _last_update = (sig, {o.data_ptr(): i for i, o in enumerate(outs)}, outs)
    plan = _pack_plans.get(sig)
    if not plan:
        return
    for kind in _KINDS:
        jobs = [(outs[i], e[1], e[2]) for i, e in sorted(plan.items()) if e[0] == kind]
        for (w, _, _), (tf, tb) in zip(jobs, _filters_multi(kind, jobs)):
            _prepacked[(kind, w.data_ptr())] = (w, w._version, tf, tb)


def refresh_module_filters(modules):
    """After an in-place update of the modules' OWN weights (the outer optimizer step): re-make, in one launch per kind, the
    filters each module's cache holds for the previous version of its weight (CAIN: 500 single-layer packs per meta-iteration)."""
    if not PREPACK or _capturing():
        return
    st = _raw_stream()
    jobs = {kind: [] for kind in _KINDS}
    for m in modules:
        cache, w = getattr(m, '_filters', None), getattr(m, 'weight', None)
        if not cache or w is None or not _on_device(w) or not w.is_contiguous():
            continue
        for key in reversed(list(cache)):           # the newest entry of this weight on this stream, if it is of another version
            k = _ModuleKey(*key)
            if k.ptr == w.data_ptr() and k.shape == tuple(w.shape) and k.stream == st:
                if k.version != w._version:
                    old = cache[key]
                    jobs[k.kind].append((m, key, (w.detach(), old[0] is not None, old[1] is not None)))
                break
    for kind, items in jobs.items():
        for (m, key, (w, _, _)), made in zip(items, _filters_multi(kind, [it[2] for it in items])):
            m._filters.pop(key, None)
            m._filters[_module_key(kind, w)] = made


# Memory-layout tags.  Two tensors of the SepConv tail keep the shape [4N, 51, H, W] while their MEMORY is unit-major, [H][W / 16][51][16]
# per sample: the taps between the last Subnet convolution and FunctionSepconvPair, and their cotangent on the way back.
# The layout travels as an attribute of the tensor object; producer and consumer name what they write / expect, and a tensor that reaches
# a consumer with another tag -- or a unit-major one that reaches a consumer which knows nothing of tags after a hook, a clone or a sum
# replaced the object -- fails here instead of being read as scrambled numbers.
UNIT16 = "unit16"


def tag_layout(t, layout):
    t._savfi_layout = layout
    return t


def layout_of(t):
    return getattr(t, "_savfi_layout", None)


def require_layout(t, layout, what):
    got = layout_of(t)
    if got != layout:
        raise SavfiLayoutError("%s: memory layout %r expected, the tensor is tagged %r (a unit-major tensor keeps the shape [N,51,H,W] "
                               "while its memory is [N][H][W/16][51][16]; only its producer's partner may read it)" % (what, layout, got))


class SavfiLayoutError(RuntimeError):
    pass


def conv3x3_unit16_supported(x, w, pad):
    """Can the 3x3 layer (x [N,Ci,H,W], task weights w [T,Co,Ci,3,3], zero padding `pad`) write its result unit-major
    (savfi_conv3x3_tasks_pre_unit16_f32)?  It runs on the Winograd kernel, its width is a multiple of 16, no reduction split."""
    # ('wino2' no: a small launch runs the F(2x2) form, whose unit-major entry points are the form-0 ones)
    if not (_f32_map(x) and w.dim() == 5 and conv_route(x.shape, w.shape, 1, pad, 1).fwd == 'wino'):
        return False
    N, Ci, H, W = x.shape
    return int(_hip.lib().savfi_conv3x3_unit16_supported(N, w.shape[0], Ci, w.shape[1], H, W, int(pad))) == 1


def conv3x3_in_unit16_supported(gy_shape, w, pad):
    """Can the data gradient of the 3x3 layer (cotangent of shape gy_shape, task weights w [T,Co,Ci,3,3]) read a unit-major cotangent
    (savfi_conv3x3_dgrad_in_unit16_f32)?"""
    N, Co, H, W = gy_shape
    return int(_hip.lib().savfi_conv3x3_in_unit16_supported(N, w.shape[0], w.shape[2], Co, H, W, int(pad))) == 1


def conv3x3_dgrad_in_unit16(gy, u, T, Ci, Co, pad):
    """savfi_conv3x3_dgrad_in_unit16_f32: the data gradient on a cotangent whose MEMORY is unit-major ([N][H][W/16][Co][16])."""
    gy = gy.contiguous()
    _hip.require_cuda(gy, u)
    N, _, H, W = gy.shape
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, 1)
    out = torch.empty(shape, dtype=gy.dtype, device=gy.device)
    _hip.call(_conv3x3_name(Ci, Co, "bwd_data"), "savfi_conv3x3_dgrad_in_unit16_f32", gy, u, out, N, T, Ci, Co, H, W, int(pad), flops=flops)
    return out


def conv3x3_tasks_pre(x, u, T, Ci, Co, bias=None, mode=0, slope=1.0, pad=1, mask=None, mask_slope=1.0, out_unit16=False, f2=False):
    """savfi_conv3x3_tasks_pre_f32: conv3x3_tasks on a filter already transformed by conv3x3_filters (same mode).  `mask` (mode 1):
    the result is multiplied by (mask > 0 ? 1 : mask_slope) in the kernel's output stage (savfi_conv3x3_dgrad_masked_f32).
    `out_unit16` (mode 0): the result tensor has the usual shape [N,Co,Ho,Wo] but its MEMORY is unit-major, [N][Ho][Wo/16][Co][16]
    (savfi_conv3x3_tasks_pre_unit16_f32) -- for FunctionSepconvPair(..., taps_unit16=True) only.  `f2`: `u` is a kind-'wino2' filter
    (conv3x3_filters(..., f2=True)): the F(2x2) kernel (bit 1 of the C ABI's `mode`)."""
    x = x.contiguous()
    _hip.require_cuda(x, u)
    fbit = 2 if f2 else 0
    if mask is not None:
        assert mode == 1 and bias is None and slope == 1.0
        return _conv3x3_dgrad_masked(x, u, T, Ci, Co, pad, mask.contiguous(), mask_slope, fbit)
    N, _, H, W = x.shape
    assert N % T == 0 and x.shape[1] == (Ci if mode == 0 else Co), (x.shape, T, Ci, Co, mode)
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, mode)
    if out_unit16:
        assert mode == 0 and not f2
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
        _hip.call(_conv3x3_name(Ci, Co, "fwd"), "savfi_conv3x3_tasks_pre_unit16_f32", x, u, bias, out, N, T, Ci, Co, H, W, int(pad),
                  float(slope), flops=flops)
        return out
    nws = _workspace_floats("savfi_conv3x3_tasks_pre_workspace_floats", N, T, Ci, Co, H, W, int(pad), mode | fbit)
    ws = torch.empty(nws, dtype=x.dtype, device=x.device) if nws else None
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    name = ("conv3x3_" + ("fwd" if mode == 0 else "bwd_data")) if f2 else _conv3x3_name(Ci, Co, "fwd" if mode == 0 else "bwd_data")
    _hip.call(name, "savfi_conv3x3_tasks_pre_f32", x, u, bias, out, ws, N, T, Ci, Co, H, W, int(pad), mode | fbit, float(slope), flops=flops)
    return out


def conv3x3_tasks_pre_pool(x, u, T, Ci, Co, bias=None, slope=1.0, pad=1, f2=False):
    """(y, avg_pool2x2(y)) of conv3x3_tasks_pre's forward (savfi_conv3x3_tasks_pre_pool_f32): the pooled map comes from the convolution's
    output stage where the launch has one for it (F(4x4), an even unsplit output) and from savfi_avgpool2x2_fwd_f32 on y otherwise --
    the same values bit for bit."""
    x = x.contiguous()
    _hip.require_cuda(x, u)
    fbit = 2 if f2 else 0
    N, _, H, W = x.shape
    assert N % T == 0 and x.shape[1] == Ci, (x.shape, T, Ci, Co)
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, 0)
    assert shape[2] >= 2 and shape[3] >= 2, shape
    nws = _workspace_floats("savfi_conv3x3_tasks_pre_workspace_floats", N, T, Ci, Co, H, W, int(pad), fbit)
    ws = torch.empty(nws, dtype=x.dtype, device=x.device) if nws else None
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    pooled = torch.empty(shape[:2] + (shape[2] // 2, shape[3] // 2), dtype=x.dtype, device=x.device)
    did = ctypes.c_int(0)
    name = "conv3x3_fwd" if f2 else _conv3x3_name(Ci, Co, "fwd")
    _hip.call(name, "savfi_conv3x3_tasks_pre_pool_f32", x, u, bias, out, pooled, ws, N, T, Ci, Co, H, W, int(pad), fbit, float(slope),
              ctypes.byref(did), flops=flops)
    if not did.value:
        pooled = _avgpool2x2_fwd_launch(out)
    return out, pooled


def _conv3x3_dgrad_masked(gy, u, T, Ci, Co, pad, mask, mask_slope, fbit=0):
    N, _, H, W = gy.shape
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, 1)
    out = torch.empty(shape, dtype=gy.dtype, device=gy.device)
    assert mask.shape == out.shape, (mask.shape, out.shape)
    nws = _workspace_floats("savfi_conv3x3_tasks_pre_workspace_floats", N, T, Ci, Co, H, W, int(pad), 1 | fbit)
    ws = torch.empty(nws, dtype=gy.dtype, device=gy.device) if nws else None
    _hip.call("conv3x3_bwd_data" if fbit else _conv3x3_name(Ci, Co, "bwd_data"), "savfi_conv3x3_dgrad_masked_form_f32", gy, u, mask,
              float(mask_slope), out, ws, N, T, Ci, Co, H, W, int(pad), fbit, flops=flops)
    return out


def mask_by_activation(g, y, slope):
    """g * (y > 0 ? 1 : slope): the (leaky) ReLU derivative from the activated output, one element-wise pass (savfi_bias_act_bwd_f32
    without the bias sums) -- the unfused form of the masked data-gradient epilogues."""
    g, y = g.contiguous(), y.contiguous()
    _hip.require_cuda(g, y)
    out = torch.empty_like(g)
    N, C = g.shape[:2]
    hw = g.numel() // (N * C)
    _hip.call("bias_act_bwd", "savfi_bias_act_bwd_f32", g, y, out, None, None, N, C, hw, float(slope))
    return out


class _MaskGrad(torch.autograd.Function):
    """identity whose backward multiplies by the activation derivative taken from the (activated) tensor itself: the consumer side of
    a deferred activation derivative when the consumer is not one of the fused convolutions."""

    @staticmethod
    def forward(ctx, x, slope):
        ctx.slope = slope
        ctx.save_for_backward(x)
        return x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return mask_by_activation(g, x, ctx.slope), None


def mask_grad(x, slope):
    return _MaskGrad.apply(x, float(slope))


def convk_tasks_pre(x, packed, T, Ci, Co, K, bias=None, mode=0, slope=1.0, pad=1, precise=False, reflect=False, mask=None, mask_slope=1.0):
    """savfi_convk_tasks_pre_f32: direct K x K convolution (mode 0, + bias + activation) or its data gradient (mode 1) on a
    filter packed by convk_filters (same mode); sample n uses filter set n % T.  `mask` (mode 1): the result is multiplied by
    (mask > 0 ? 1 : mask_slope) in the kernel's epilogue (savfi_convk_dgrad_masked_f32)."""
    x = x.contiguous()
    _hip.require_cuda(x, packed)
    N, _, H, W = x.shape
    assert N % T == 0 and x.shape[1] == (Ci if mode == 0 else Co), (x.shape, T, Ci, Co, mode)
    I = Co if mode == 0 else Ci
    p_eff = pad if mode == 0 else K - 1 - pad
    out = torch.empty((N, I, H + 2 * p_eff - K + 1, W + 2 * p_eff - K + 1), dtype=x.dtype, device=x.device)
    if mask is not None and (K != 3 or precise):
        # the masked epilogue exists for the 3 x 3 kernels of the conv chains; the same multiplication as a separate pass elsewhere
        return mask_by_activation(convk_tasks_pre(x, packed, T, Ci, Co, K, bias, mode, slope, pad, precise, reflect), mask, mask_slope)
    if mask is not None:
        assert mode == 1 and bias is None and slope == 1.0 and not reflect
        mask = mask.contiguous()
        assert mask.shape == out.shape, (mask.shape, out.shape)
        _hip.call("convk_bwd_data", "savfi_convk_dgrad_masked_f32", x, packed, mask, float(mask_slope), out, N, T, Ci, Co, H, W, K, int(pad),
                  int(bool(precise)), flops=2.0 * K * K * Ci * Co * N * H * W)
        return out
    _hip.call("convk_fwd" if mode == 0 else "convk_bwd_data", "savfi_convk_tasks_pre_reflect_f32", x, packed, bias, out, N, T, Ci, Co, H, W,
              K, int(pad), mode, float(slope), int(bool(precise)), int(bool(reflect)),
              flops=2.0 * K * K * Ci * Co * N * (out.shape[2] * out.shape[3] if mode == 0 else H * W))
    return out


def convk_wgrad_tasks_sums_bias(x_shape, co, T, K, pad, precise=False):
    """Will convk_wgrad_tasks(..., want_bias=True) hand out the bias gradient with the weight gradient (the all-taps 3 x 3 kernel does)?"""
    N, Ci, H, W = x_shape
    return bool(WGRAD_FUSE_BIAS and not precise and _hip.lib().savfi_convk_wgrad_sums_bias(N, T, Ci, co, H, W, K, int(pad)))


def convk_wgrad_tasks(x, gz, T, K, pad, precise=False, reflect=False, want_bias=False):
    """savfi_convk_wgrad_tasks_f32: gw [T,Co,Ci,K,K], gw[t] over the samples n % T == t (direct K x K form, split-bf16 MFMAs).
    want_bias (only where convk_wgrad_tasks_sums_bias says yes): returns (gw, gb [T,Co]) -- the sums of gz ride on the kernel's staging of it."""
    x, gz = x.contiguous(), gz.contiguous()
    _hip.require_cuda(x, gz)
    N, Ci, H, W = x.shape
    Co = gz.shape[1]
    assert N % T == 0 and tuple(gz.shape) == (N, Co, H + 2 * pad - K + 1, W + 2 * pad - K + 1), (x.shape, gz.shape, K, pad, T)
    ws = torch.empty(_workspace_floats("savfi_convk_wgrad_workspace_floats", N, T, Ci, Co, H, W, K, int(pad)), dtype=x.dtype, device=x.device)
    gw = torch.empty((T, Co, Ci, K, K), dtype=x.dtype, device=x.device)
    flops = 2.0 * K * K * Ci * Co * N * gz.shape[2] * gz.shape[3]
    if want_bias:
        assert not precise and convk_wgrad_tasks_sums_bias(x.shape, Co, T, K, pad), "ask convk_wgrad_tasks_sums_bias first"
        gb = torch.empty((T, Co), dtype=x.dtype, device=x.device)
        _hip.call("convk_wgrad", "savfi_convk_wgrad_tasks_bias_f32", x, gz, gw, gb, ws, N, T, Ci, Co, H, W, K, int(pad), int(bool(reflect)),
                  flops=flops)
        return gw, gb
    _hip.call("convk_wgrad", "savfi_convk_wgrad_tasks_reflect_f32", x, gz, gw, ws, N, T, Ci, Co, H, W, K, int(pad), int(bool(precise)),
              int(bool(reflect)), flops=flops)
    return gw


def reflect_pad_bwd(gp, pad, add=None):
    """savfi_reflect_pad_bwd_f32: the adjoint of nn.ReflectionPad2d(pad) as a gather; gp [N,C,H+2p,W+2p] -> [N,C,H,W].
    add [N,C,H,W]: a second cotangent of the unpadded map, added in the same pass (savfi_reflect_pad_bwd_add_f32)."""
    gp = gp.contiguous()
    _hip.require_cuda(gp)
    N, C, Hp, Wp = gp.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    gx = torch.empty((N, C, H, W), dtype=gp.dtype, device=gp.device)
    if add is not None:
        add = add.contiguous()
        _hip.require_cuda(add)
        assert tuple(add.shape) == (N, C, H, W) and add.dtype == gp.dtype, (add.shape, gp.shape, pad)
        _hip.call("reflect_pad_bwd", "savfi_reflect_pad_bwd_add_f32", gp, add, gx, N * C, H, W, int(pad), nbytes=4 * (gp.numel() + 2 * gx.numel()))
        return gx
    _hip.call("reflect_pad_bwd", "savfi_reflect_pad_bwd_f32", gp, gx, N * C, H, W, int(pad), nbytes=4 * (gp.numel() + gx.numel()))
    return gx


class _ReflectPad(torch.autograd.Function):
    """nn.ReflectionPad2d(pad): savfi_reflect_pad_fwd_f32, the adjoint as ONE gather launch (savfi_reflect_pad_bwd_f32) where ATen's
    reflection_pad2d_backward zero-fills its result and scatters with atomics (two launches, order-dependent sums) -- the layers
    whose maps are too small for the mirrored staging of the direct kernels (CAIN at 64x64: 252 pads per meta-iteration)."""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad = int(pad)
        return _reflect_pad_fwd(x, ctx.pad)

    @staticmethod
    def backward(ctx, g):
        return reflect_pad_bwd(g, ctx.pad), None


def _reflect_pad_fwd(x, p):
    x = x.contiguous()
    _hip.require_cuda(x)
    N, C, H, W = x.shape
    assert 0 <= p < H and p < W, (x.shape, p)
    if N * C > 65535:          # beyond the launch grid's plane axis: ATen's kernel
        return torch.nn.functional.pad(x, (p,) * 4, mode='reflect')
    xp = torch.empty((N, C, H + 2 * p, W + 2 * p), dtype=x.dtype, device=x.device)
    _hip.call("reflect_pad", "savfi_reflect_pad_fwd_f32", x, xp, N * C, H, W, p, nbytes=4 * (x.numel() + xp.numel()))
    return xp


class _ReflectPadSkip(torch.autograd.Function):
    """(nn.ReflectionPad2d(pad)(x), x): the padded map for a convolution and the map itself for a connection round it (CAIN's RCAB,
    reference model_utils.py:957-990).  The two cotangents of x arrive in ONE backward call and leave as one pass, fold(g_pad) + g_skip
    (savfi_reflect_pad_bwd_add_f32), where autograd would add the fold's result and the skip gradient in an element-wise kernel of its own."""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad = int(pad)
        ctx.set_materialize_grads(False)
        return _reflect_pad_fwd(x, ctx.pad), x.view_as(x)

    @staticmethod
    def backward(ctx, g_pad, g_skip):
        if g_pad is None:
            return g_skip, None
        return reflect_pad_bwd(g_pad, ctx.pad, add=g_skip), None


def reflect_pad_with_skip(x, pad):
    """(nn.ReflectionPad2d(pad)(x), x) with the two gradients of x added inside the fold (_ReflectPadSkip); passes that need a
    differentiable backward, CPU tensors and other dtypes: ATen's pad and x itself."""
    if double_backward() or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        return torch.nn.functional.pad(x, (int(pad),) * 4, mode='reflect'), x
    return _ReflectPadSkip.apply(x, int(pad))


def reflect_pad(x, pad):
    """nn.ReflectionPad2d(pad)(x).  First-order passes on CUDA tensors take the gather adjoint; --second_order (whose backward
    must itself be differentiable) and CPU tensors stay on ATen."""
    if double_backward() or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        return torch.nn.functional.pad(x, (int(pad),) * 4, mode='reflect')
    return _ReflectPad.apply(x, int(pad))


def convk_reflect_eligible(x, weight, pad):
    """MetaConvNorm (ReflectionPad2d(pad) + K x K convolution, K = 2 pad + 1) as ONE direct convolution that mirrors the border
    while it stages its tile?  Where the layer would take the direct kernel anyway (forward, data gradient and weight gradient
    all live in csrc/convk*.hip there) and the fast weight is a plain [Co,Ci,K,K] tensor."""
    if weight.dim() != 4 or x.dim() != 4 or pad < 1 or int(weight.shape[-1]) != 2 * pad + 1:
        return False
    if pad >= x.shape[2] or pad >= x.shape[3]:
        return False
    return convk_eligible(x, weight, 1, pad, 1, 1, False)


WGRAD_FUSE_BIAS = True     # A/B: False = the bias sums as a pass of their own (rounds 2-4)


def conv3x3_wgrad_tasks_sums_bias(x_shape, co, T, pad):
    """Will conv3x3_wgrad_tasks(..., want_bias=True) hand out the bias gradient with the weight gradient (the Winograd form does)?"""
    N, Ci, H, W = x_shape
    return WGRAD_FUSE_BIAS and _wgrad_wino(N, Ci, co, H + 2 * pad - 2, W + 2 * pad - 2)


def conv3x3_wgrad_tasks(x, gz, T, pad=1, stream=None, extra_stream=None, want_bias=False):
    """savfi_conv3x3_wgrad_tasks_f32: gw [T,Co,Ci,3,3], gw[t] over the samples n % T == t.  `stream` / `extra_stream`: as in
    conv3x3_wgrad (launch on a side stream, buffers from the current stream's pool).  want_bias (only where
    conv3x3_wgrad_tasks_sums_bias says yes): returns (gw, gb [T,Co]) -- the sums of gz ride on the weight gradient's read of it."""
    x, gz = x.contiguous(), gz.contiguous()
    _hip.require_cuda(x, gz)
    N, Ci, H, W = x.shape
    Co = gz.shape[1]
    assert N % T == 0 and tuple(gz.shape) == (N, Co, H + 2 * pad - 2, W + 2 * pad - 2), (x.shape, gz.shape, pad, T)
    form = "wino_" if _wgrad_wino(N, Ci, Co, H + 2 * pad - 2, W + 2 * pad - 2) else ""
    gw = torch.empty((T, Co, Ci, 3, 3), dtype=x.dtype, device=x.device)
    if want_bias:
        assert form == "wino_" and WGRAD_FUSE_BIAS, "ask conv3x3_wgrad_tasks_sums_bias first"
        ws = torch.empty(_workspace_floats("savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats", N, T, Ci, Co, H, W, int(pad)), dtype=x.dtype, device=x.device)
        gb = torch.empty((T, Co), dtype=x.dtype, device=x.device)
        if extra_stream is not None:
            for t in (ws, gw, gb):
                t.record_stream(extra_stream)
        _hip.call("conv3x3_wgrad", "savfi_conv3x3_wgrad_wino_tasks_bias_f32", x, gz, gw, gb, ws, N, T, Ci, Co, H, W, int(pad),
                  stream=stream, flops=18.0 * Ci * Co * gz.shape[2] * gz.shape[3] * N)
        return gw, gb
    ws = torch.empty(_workspace_floats("savfi_conv3x3_wgrad_%stasks_workspace_floats" % form, N, T, Ci, Co, H, W, int(pad)), dtype=x.dtype, device=x.device)
    if extra_stream is not None:
        ws.record_stream(extra_stream)
        gw.record_stream(extra_stream)
    _hip.call("conv3x3_wgrad", "savfi_conv3x3_wgrad_%stasks_f32" % form, x, gz, gw, ws, N, T, Ci, Co, H, W, int(pad),
              stream=stream, flops=18.0 * Ci * Co * gz.shape[2] * gz.shape[3] * N)
    return gw


TASKS_GROUPED_MAX_PIXELS = 3000      # MIOpen's grouped solvers: fine on small maps, 5-30x slower than T plain calls on large ones


def _grouped_ok(x):
    return x.shape[2] * x.shape[3] < TASKS_GROUPED_MAX_PIXELS


def conv2d_tasks(x, weight, bias, stride=1, padding=0, dilation=1):
    """conv2d of [n*T, Ci, H, W] (sample-major) with per-task weights [T, Co, Ci, kh, kw] / bias [T, Co], composed of
    differentiable torch ops (second order, bias-free layers, CPU host-logic tests): ONE grouped convolution on small maps,
    one plain convolution per task on large ones (tools/tasks_bench.py: MIOpen's grouped kernels take 1.5-10 ms there)."""
    T, Co, Ci = weight.shape[:3]
    N, _, H, W = x.shape
    n = N // T
    if _grouped_ok(x) or not x.is_cuda:
        z = torch.nn.functional.conv2d(x.reshape(n, T * Ci, H, W), weight.reshape(T * Co, Ci, *weight.shape[3:]),
                                       None if bias is None else bias.reshape(T * Co), stride, padding, dilation, T)
        return z.reshape(N, Co, z.shape[2], z.shape[3])
    xs = x.reshape(n, T, Ci, H, W)
    zs = [torch.nn.functional.conv2d(xs[:, t], weight[t], None if bias is None else bias[t], stride, padding, dilation)
          for t in range(T)]
    z = torch.stack(zs, 1)                                     # [n, T, Co, Ho, Wo]: sample-major again
    return z.reshape(N, Co, z.shape[3], z.shape[4])


class _ConvBiasActTasks(torch.autograd.Function):
    """y = act(conv2d(x[s], w[s % T]) + b[s % T]) for every sample s.  First-order only (like _ConvBiasAct)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, dilation, slope, direct=False, in_slope=None, defer=False, out_unit16=False):
        return _conv_forward(ctx, x, w, b, stride, padding, dilation, 1, slope, direct, None, False, in_slope, defer, int(out_unit16), w.shape[0])

    @staticmethod
    def backward(ctx, gy):
        return _conv_backward(ctx, gy) + (None,) * 8


class _ConvBiasActTasksPool(torch.autograd.Function):
    """(y, avg_pool2x2(y)) with y = act(conv2d(x[s], w[s % T]) + b[s % T]): an encoder block's last layer, whose activated output feeds the
    pooling and a skip connection.  Forward: the F(4x4) kernel's output stage stores the pooled map from the tile it holds in registers
    (csrc/winograd4.h, POOL; savfi_avgpool2x2_fwd_f32's expression and order, so the same bits) -- the pooling kernel read the whole map
    back for it; launches without that epilogue run the pooling kernel as before.  backward(g_skip, g_pool): _AvgPool2x2AndSkip's one
    pass, gz = (pool^T(g_pool) + g_skip) * act'(y), then _ConvBiasActTasks's backward on gz as the cotangent of a layer that deferred its
    activation derivative -- the kernels, in the order, of conv_bias_act_tasks(defer=True) -> avg_pool2x2_and_skip.  First-order only."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, dilation, slope, direct=False, in_slope=None):
        ctx.set_materialize_grads(False)
        return _conv_forward(ctx, x, w, b, stride, padding, dilation, 1, slope, direct, None, False, in_slope, True, 0, w.shape[0], pool=True)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_skip, g_pool):
        if g_skip is None and g_pool is None:
            return (None,) * 9
        y = ctx.saved_tensors[2]
        slope = ctx.conf[4]
        gz = _avgpool2x2_skip_adjoint(g_pool, g_skip, y, None if slope == 1.0 else slope)
        return _conv_backward(ctx, gz) + (None,) * 6


def conv_bias_act_tasks_pool(x, weight, bias, stride=1, padding=0, dilation=1, slope=0.0, direct=False, in_slope=None):
    """(y, avg_pool2x2(y)) of conv_bias_act_tasks -- see _ConvBiasActTasksPool.  y's activation derivative is applied by this op's own
    backward: its consumers see an ordinary tensor (nothing is deferred to them).  Maps of at least 2 x 2 pixels."""
    return _ConvBiasActTasksPool.apply(x, weight, bias, stride, padding, dilation, float(slope), bool(direct),
                                       None if in_slope is None else float(in_slope))


def conv_pools_in_epilogue(x, weight, stride, padding, dilation):
    """Does conv_bias_act_tasks's forward of this per-task layer run on the F(4x4) kernel with an output stage that can pool (an even,
    unsplit output of at least 2 rows)?  Where MetaNetwork's encoder uses conv_bias_act_tasks_pool."""
    if not (_f32_map(x) and weight.dim() == 5):
        return False
    route = conv_route(x.shape, weight.shape, stride, padding, dilation)
    if route.fwd != 'wino':
        return False
    N, Ci, H, W = x.shape
    Ho, Wo = H + 2 * route.pad - 2, W + 2 * route.pad - 2
    if Ho < 2 or Wo < 2 or Wo % 2 != 0 or wino4_workgroups(N, Ci, weight.shape[1], H, W, route.pad, 0) <= 0:
        return False
    return _workspace_floats("savfi_conv3x3_tasks_pre_workspace_floats", N, weight.shape[0], Ci, weight.shape[1], H, W, route.pad, 0) == 0


def conv_bias_act_tasks(x, weight, bias, stride=1, padding=0, dilation=1, slope=0.0, direct=False, in_slope=None, defer=False,
                        out_unit16=False):
    """act(conv2d(x[s], weight[s % T]) + bias[s % T]): the lockstep form of conv_bias_act (`in_slope`, `defer`: conv_bias_act).
    `out_unit16`: the result's memory is unit-major (conv3x3_tasks_pre; only after conv3x3_unit16_supported said yes, slope 1)."""
    z = _ConvBiasActTasks.apply(x, weight, bias, stride, padding, dilation, float(slope), bool(direct),
                                None if in_slope is None else float(in_slope), bool(defer), int(out_unit16))
    return tag_layout(z, UNIT16) if out_unit16 else z


@functools.lru_cache(maxsize=None)
def _workspace_floats(query, *shape):
    """Size queries of the C ABI are pure functions of the shape: ask once per shape."""
    n = int(getattr(_hip.lib(), query)(*shape))
    if n < 0:
        _hip.check(n, query)
    return n


def conv3x3(x, weight, bias=None, mode=0, slope=1.0, pad=1):
    """savfi_conv3x3_f32 without autograd.  mode 0: act(conv2d(x, weight, padding=pad) + bias); mode 1: the data
    gradient of that convolution (x = gy [N,Co,H,W] -> gx [N,Ci,H+2-2pad,W+2-2pad])."""
    x = x.contiguous()
    weight = weight.contiguous()
    _hip.require_cuda(x, weight)
    N, _, H, W = x.shape
    Co, Ci = weight.shape[:2]
    assert tuple(weight.shape[2:]) == (3, 3) and x.shape[1] == (Ci if mode == 0 else Co), (x.shape, weight.shape, mode)
    shape, flops = _conv3x3_out(N, Ci, Co, H, W, pad, mode)
    ws = torch.empty(_workspace_floats("savfi_conv3x3_workspace_floats", N, Ci, Co, H, W, int(pad), mode), dtype=x.dtype, device=x.device)
    out = torch.empty(shape, dtype=x.dtype, device=x.device)
    _hip.call(_conv3x3_name(Ci, Co, "fwd" if mode == 0 else "bwd_data"), "savfi_conv3x3_f32", x, weight, bias, out, ws,
              N, Ci, Co, H, W, int(pad), mode, float(slope), flops=flops)
    return out


def conv3x3_wgrad(x, gz, pad=1, stream=None, extra_stream=None):
    """savfi_conv3x3_wgrad_f32: weight gradient [Co,Ci,3,3] of conv2d(x, w, padding=pad) for the cotangent gz.
    `stream` (raw handle) launches on another stream than torch's current one; the result and the workspace are still
    allocated from the current stream's pool (safe: that stream has been made to wait for this one) and registered with
    `extra_stream` so that they are not recycled while it still uses them."""
    x, gz = x.contiguous(), gz.contiguous()
    _hip.require_cuda(x, gz)
    N, Ci, H, W = x.shape
    Co = gz.shape[1]
    assert tuple(gz.shape) == (N, Co, H + 2 * pad - 2, W + 2 * pad - 2), (x.shape, gz.shape, pad)
    if _wgrad_wino(N, Ci, Co, H + 2 * pad - 2, W + 2 * pad - 2):
        return conv3x3_wgrad_tasks(x, gz, 1, pad, stream, extra_stream)[0]
    ws = torch.empty(_workspace_floats("savfi_conv3x3_wgrad_workspace_floats", N, Ci, Co, H, W, int(pad)), dtype=x.dtype, device=x.device)
    gw = torch.empty((Co, Ci, 3, 3), dtype=x.dtype, device=x.device)
    if extra_stream is not None:
        ws.record_stream(extra_stream)
        gw.record_stream(extra_stream)
    _hip.call("conv3x3_wgrad", "savfi_conv3x3_wgrad_f32", x, gz, gw, ws, N, Ci, Co, H, W, int(pad), stream=stream,
              flops=18.0 * Ci * Co * gz.shape[2] * gz.shape[3] * N)
    return gw


def conv_bias_act(x, weight, bias, stride=1, padding=0, dilation=1, groups=1, slope=0.0, direct=False, cache=None, reflect=False,
                  in_slope=None, defer=False):
    """act(conv2d(x, weight) + bias) with act = LeakyReLU(slope) (0 -> ReLU, 1 -> identity); bias may be None.  `direct`: a 3x3
    layer wants the direct split-bf16 kernel whatever its size (no Winograd rounding); `cache`: a dict owned by the module whose
    own parameter `weight` is (its packed filters are kept there per weight version), None for fast weights.
    conv -> act -> conv chains whose intermediate has ONE consumer (model_utils.MetaSequential): `defer` = that consumer applies this
    layer's activation derivative, `in_slope` = x is the activated output of a producer that deferred its derivative to this layer
    (folded into this layer's data gradient: one element-wise pass over the map less per chain link)."""
    return _ConvBiasAct.apply(x, weight, bias, stride, padding, dilation, groups, float(slope), bool(direct), cache, bool(reflect),
                              None if in_slope is None else float(in_slope), bool(defer))


# --------------------------------------------------------------------------------------------
# Channel attention + residual of CAIN's RCAB        (reference model_utils.py:931-953, :957-990)
# --------------------------------------------------------------------------------------------
CA_FUSE_MLP = True       # A/B and tests: False = pool, MLP and apply as three launches per direction


class _ChannelAttentionResidual(torch.autograd.Function):
    """out = t * sigmoid(W2 relu(W1 mean_hw(t) + b1) + b2) + x, also returns the attention y [N,C,1,1] (not differentiable on
    its own).  w1 [T,Cr,C] / b1 [T,Cr] / w2 [T,C,Cr] / b2 [T,C]: sample n uses set n % T.  First-order only."""

    @staticmethod
    def forward(ctx, t, x, w1, b1, w2, b2):
        t, x = t.contiguous(), x.contiguous()
        w1, b1, w2, b2 = w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
        _hip.require_cuda(t, x, w1, b1, w2, b2)
        N, C, H, W = t.shape
        T, Cr = w1.shape[0], w1.shape[1]
        assert x.shape == t.shape and N % T == 0 and tuple(w1.shape) == (T, Cr, C) and tuple(w2.shape) == (T, C, Cr), (t.shape, w1.shape, w2.shape)
        s = torch.empty((N, C), dtype=t.dtype, device=t.device)
        y = torch.empty((N, C), dtype=t.dtype, device=t.device)
        a1 = torch.empty((N, Cr), dtype=t.dtype, device=t.device)
        out = torch.empty_like(t)
        hw = H * W
        _hip.call("ca_pool", "savfi_ca_pool_f32", t, None, s, N * C, hw, 1.0 / hw, nbytes=4 * t.numel())
        if CA_FUSE_MLP and Cr <= 16 and C <= 256:       # the MLP inside the apply launch (every workgroup repeats it for its sample: the same y, bit for bit)
            _hip.call("ca_apply", "savfi_ca_apply_mlp_f32", t, s, w1, b1, w2, b2, x, out, y, a1, N, T, C, Cr, hw, nbytes=12 * t.numel())
        else:
            _hip.call("ca_mlp", "savfi_ca_mlp_fwd_f32", s, w1, b1, w2, b2, y, a1, N, T, C, Cr)
            _hip.call("ca_apply", "savfi_ca_apply_f32", t, y, x, None, out, N * C, hw, nbytes=12 * t.numel())
        ctx.save_for_backward(t, s, y, a1, w1, w2)
        ctx.mark_non_differentiable(y)
        ctx.set_materialize_grads(False)        # (else autograd fills a zero tensor for the attention's cotangent on every backward call)
        return out, y.view(N, C, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gy):
        if g is None:
            return (None,) * 6
        t, s, y, a1, w1, w2 = ctx.saved_tensors
        g = g.contiguous()
        N, C, H, W = t.shape
        T, Cr = w1.shape[0], w1.shape[1]
        hw = H * W
        r = torch.empty((N, C), dtype=t.dtype, device=t.device)
        ds = torch.empty((N, C), dtype=t.dtype, device=t.device)
        gw1, gb1 = torch.empty_like(w1), torch.empty((T, Cr), dtype=t.dtype, device=t.device)
        gw2, gb2 = torch.empty_like(w2), torch.empty((T, C), dtype=t.dtype, device=t.device)
        gt = torch.empty_like(t)
        _hip.call("ca_pool", "savfi_ca_pool_f32", g, t, r, N * C, hw, 1.0, nbytes=8 * t.numel())
        if CA_FUSE_MLP and Cr <= 16 and C <= 256:       # the MLP's backward inside the apply launch: ds per workgroup, the parameter gradients from T workgroups
            _hip.call("ca_apply", "savfi_ca_apply_bwd_mlp_f32", g, r, s, y, a1, w1, w2, gt, gw1, gb1, gw2, gb2, N, T, C, Cr, hw,       # at the front of its grid
                      nbytes=8 * t.numel())
        else:
            _hip.call("ca_mlp_bwd", "savfi_ca_mlp_bwd_f32", r, s, y, a1, w1, w2, ds, gw1, gb1, gw2, gb2, N, T, C, Cr, 1.0 / hw)
            _hip.call("ca_apply", "savfi_ca_apply_f32", g, y, None, ds, gt, N * C, hw, nbytes=8 * t.numel())
        need = ctx.needs_input_grad
        return (gt if need[0] else None, g if need[1] else None, gw1 if need[2] else None, gb1 if need[3] else None,
                gw2 if need[4] else None, gb2 if need[5] else None)


def channel_attention_residual(t, x, w1, b1, w2, b2):
    """RCAB tail: (t * CA(t) + x, CA(t)).  Weights of the two 1x1 convolutions as [Cr,C,1,1] / [Cr] / [C,Cr,1,1] / [C], or with a
    leading task axis T (tasks in lockstep: sample n uses set n % T)."""
    stacked = w1.dim() == 5
    T = w1.shape[0] if stacked else 1
    Cr, C = (w1.shape[1], w1.shape[2]) if stacked else (w1.shape[0], w1.shape[1])
    out, y = _ChannelAttentionResidual.apply(t, x, w1.reshape(T, Cr, C), b1.reshape(T, Cr), w2.reshape(T, C, Cr), b2.reshape(T, C))
    return out, y


# --------------------------------------------------------------------------------------------
# Bilinear x2 up-sampling      (sepconv/model.py:191, :213-234; voxel_flow.py:400-414)
# --------------------------------------------------------------------------------------------
class _Upsample2x(torch.autograd.Function):
    """geom = (H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww): x is the crop [sy0:sy0+Hs, sx0:sx0+Ws] of a virtual
    [H, W] map, the result the window [oy0:oy0+Hw, ox0:ox0+Ww] of its x2 up-sampling (full op: crop = window = all)."""

    @staticmethod
    def forward(ctx, x, align_corners, geom, in_slope=None):
        """in_slope: x is the activated output of a fused convolution that left its (leaky) ReLU derivative to this op (its single
        consumer; conv_bias_act `defer`): the adjoint multiplies by it in its store (first-order passes only)."""
        _hip.require_cuda(x)
        N, C = x.shape[:2]
        H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
        assert tuple(x.shape[2:]) == (Hs, Ws), (x.shape, geom)
        out = torch.empty((N, C, Hw, Ww), dtype=x.dtype, device=x.device)
        _hip.call("upsample2x_fwd", "savfi_upsample2x_window_fwd_f32", x, out, N * C, *geom, int(align_corners),
                  nbytes=4 * N * C * (Hs * Ws + Hw * Ww))
        ctx.align, ctx.geom, ctx.in_slope = bool(align_corners), geom, in_slope
        if in_slope is not None:
            ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.in_slope is not None:
            # a raw kernel without a graph: under create_graph=True it would hand out zero second-order terms silently -- refuse instead
            # (the callers pass in_slope in first-order passes only: hip_ops.double_backward() is checked at forward time)
            if torch.is_grad_enabled() and g.requires_grad:
                raise RuntimeError("upsample2x with a deferred activation derivative (in_slope) is first-order only")
            x, = ctx.saved_tensors
            g = g.contiguous()
            N, C = g.shape[:2]
            H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = ctx.geom
            gin = torch.empty((N, C, Hs, Ws), dtype=g.dtype, device=g.device)
            _hip.call("upsample2x_bwd", "savfi_upsample2x_window_bwd_masked_f32", g, x, float(ctx.in_slope), gin, N * C, *ctx.geom,
                      int(ctx.align), nbytes=4 * N * C * (2 * Hs * Ws + Hw * Ww))
            return gin, None, None, None
        # linear op: its adjoint goes through the Function too, so double-backward keeps working
        return _Upsample2xAdjoint.apply(g, ctx.align, ctx.geom), None, None, None


class _Upsample2xAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, align_corners, geom):
        g = g.contiguous()
        _hip.require_cuda(g)
        N, C = g.shape[:2]
        H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
        assert tuple(g.shape[2:]) == (Hw, Ww), (g.shape, geom)
        gin = torch.empty((N, C, Hs, Ws), dtype=g.dtype, device=g.device)
        _hip.call("upsample2x_bwd", "savfi_upsample2x_window_bwd_f32", g, gin, N * C, *geom, int(align_corners),
                  nbytes=4 * N * C * (Hs * Ws + Hw * Ww))
        ctx.align, ctx.geom = bool(align_corners), geom
        return gin

    @staticmethod
    def backward(ctx, gg):
        return _Upsample2x.apply(gg.contiguous(), ctx.align, ctx.geom, None), None, None


def upsample_window_sources(o0, o1, size_in, align_corners):
    """First / last source index the outputs [o0, o1) of a x2 up-sampling of `size_in` samples read
    (float32 arithmetic of the kernel, which is ATen's area_pixel_compute_source_index)."""
    import numpy as np
    f = np.float32
    if align_corners:
        scale = f(size_in - 1) / f(2 * size_in - 1) if size_in > 0 else f(0)
        src = lambda d: scale * f(d)
    else:
        src = lambda d: max((f(d) + f(0.5)) * f(0.5) - f(0.5), f(0))
    lo = min(int(src(o0)), size_in - 1)
    hi = min(int(src(o1 - 1)), size_in - 1)
    return lo, min(hi + 1, size_in - 1)


def upsample_bilinear2x_window(x, full_hw, crop_origin, out_window, align_corners, in_slope=None):
    """x = crop of a virtual [N,C,*full_hw] map starting at crop_origin (y, x); returns rows/cols
    out_window = (oy0, ox0, Hw, Ww) of its bilinear x2 up-sampling.  in_slope: see _Upsample2x.forward."""
    H, W = full_hw
    geom = (int(H), int(W), int(crop_origin[0]), int(crop_origin[1]), int(x.shape[2]), int(x.shape[3]),
            int(out_window[0]), int(out_window[1]), int(out_window[2]), int(out_window[3]))
    return _Upsample2x.apply(x.contiguous(), bool(align_corners), geom, None if in_slope is None else float(in_slope))


def upsample_bilinear2x(x, align_corners, in_slope=None):
    """[N,C,H,W] -> [N,C,2H,2W], bilinear, ATen-identical source indices.  in_slope: see _Upsample2x.forward."""
    H, W = int(x.shape[2]), int(x.shape[3])
    return _Upsample2x.apply(x.contiguous(), bool(align_corners), (H, W, 0, 0, H, W, 0, 0, 2 * H, 2 * W),
                             None if in_slope is None else float(in_slope))


class Upsample2x(torch.nn.Module):
    """Parameter-free stand-in for torch.nn.Upsample(scale_factor=2, mode='bilinear', align_corners=...)."""

    def __init__(self, align_corners=True):
        super().__init__()
        self.align_corners = align_corners

    def forward(self, x, in_slope=None):
        if not x.is_cuda:    # CPU tensors (host-logic tests): the plain ATen op
            assert in_slope is None, "a deferred activation derivative is a GPU path"
            return torch.nn.functional.interpolate(x, scale_factor=2, mode='bilinear', align_corners=self.align_corners)
        return upsample_bilinear2x(x, self.align_corners, in_slope)

    def extra_repr(self):
        return 'scale_factor=2, mode=bilinear, align_corners=%s' % self.align_corners
