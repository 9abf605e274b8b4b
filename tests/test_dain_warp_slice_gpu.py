"""-m gpu: hip_ops.filter_interpolation_into / savfi_filterinterp_fwd_slice_f32, the adaptive warp written into a channel slice.

The slice must hold the bits of hip_ops.filter_interpolation and every other channel of the wider tensor must keep what it held, for slice
bases and planes that are not 16-byte aligned (7 x 9 planes, c_off = 3 and 45), one and several channel chunks, and inputs that take
both branches of the kernel (valid pixels and the pass-through; some flows NaN).  Bad slice arguments and NULL pointers are refused
without a launch, and the call is capturable: a graph replayed on changed inputs gives the eager result.
"""
import functools

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.5
SHAPES = {(2, 3, 7, 9): 4.0, (1, 5, 16, 16): 8.0, (2, 196, 12, 20): 8.0}          # (B, C, H, W) -> the flows are uniform in +- this
SLICES = ((0, 2), (3, 0), (45, 1))                                                 # (c_off, channels after the slice)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=0):
    B, C, H, W = shape
    torch.manual_seed(seed)
    x = torch.randn(B, C, H, W)
    flow = (torch.rand(B, 2, H, W) * 2 - 1) * SHAPES[shape]
    filt = torch.randn(B, 16, H, W) / 4
    flow.view(-1)[torch.randperm(flow.numel())[:3]] = float('nan')
    return x.to(DEV), flow.to(DEV), filt.to(DEV)


def valid_share(flow):
    """The kernel's validity rule (include/savfi_hip.h), in fp32 on the host."""
    flow = flow.cpu()
    B, _, H, W = flow.shape
    fx, fy = flow[:, 0], flow[:, 1]
    x2 = torch.arange(W, dtype=torch.float32).view(1, 1, W) + fx
    y2 = torch.arange(H, dtype=torch.float32).view(1, H, 1) + fy
    ok = (x2 >= 0) & (y2 >= 0) & (x2 <= W - 1) & (y2 <= H - 1) & (fx.abs() < W / 2.0) & (fy.abs() < H / 2.0)
    return ok.float().mean().item()


@functools.lru_cache(maxsize=None)
def reference(shape):
    with torch.no_grad():
        return hip_ops.filter_interpolation(*inputs(shape))


@pytest.mark.parametrize("c_off, extra", SLICES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_slice_holds_the_warp_and_nothing_else_moves(shape, c_off, extra):
    B, C, H, W = shape
    x, flow, filt = inputs(shape)
    share = valid_share(flow)
    print("DAIN_WARP_SLICE %s valid share %.2f" % (shape, share))
    assert 0.2 <= share <= 0.8, share                      # both branches
    assert torch.isnan(flow).any()
    out = torch.full((B, c_off + C + extra, H, W), SENTINEL, device=DEV)
    with torch.no_grad():
        got = hip_ops.filter_interpolation_into(out, c_off, x, flow, filt)
    assert got is out
    assert torch.equal(out[:, c_off:c_off + C], reference(shape))
    assert (out[:, :c_off] == SENTINEL).all() and (out[:, c_off + C:] == SENTINEL).all()


def test_bad_arguments_are_refused_without_a_launch():
    shape = (2, 3, 7, 9)
    B, C, H, W = shape
    x, flow, filt = inputs(shape)
    out = torch.full((B, C + 2, H, W), SENTINEL, device=DEV)
    lib = _hip.lib()
    call = lambda i, f, k, o, c_total, c_off: lib.savfi_filterinterp_fwd_slice_f32(i, f, k, o, B, C, H, W, 4, c_total, c_off,
                                                                                   _hip.current_stream())
    ptrs = (x.data_ptr(), flow.data_ptr(), filt.data_ptr(), out.data_ptr())
    for c_total, c_off in ((C + 2, -1), (C + 2, 3), (C - 1, 0), (0, 0)):
        assert call(*ptrs, c_total, c_off) == -2, (c_total, c_off)                  # SAVFI_E_SHAPE
    for k in range(4):
        assert call(*[None if j == k else p for j, p in enumerate(ptrs)], C + 2, 1) == -1        # SAVFI_E_NULL
    assert lib.savfi_filterinterp_fwd_slice_f32(*ptrs, B, C, H, W, 3, C + 2, 1, _hip.current_stream()) == -3     # as its sibling
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(ValueError):
        hip_ops.filter_interpolation_into(out[:1], 0, x, flow, filt)
    with pytest.raises(_hip.SavfiHipError):
        with torch.no_grad():
            hip_ops.filter_interpolation_into(out, 3, x, flow, filt)
    with pytest.raises(NotImplementedError):
        hip_ops.filter_interpolation_into(out, 1, x.clone().requires_grad_(), flow, filt)


def test_captured_call_follows_changed_inputs():
    shape = (1, 5, 16, 16)
    B, C, H, W = shape
    c_off = 3
    static = [t.clone() for t in inputs(shape)]
    out = torch.full((B, c_off + C + 1, H, W), SENTINEL, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        hip_ops.filter_interpolation_into(out, c_off, *static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        hip_ops.filter_interpolation_into(out, c_off, *static)
    for seed in (1, 2):
        fresh = inputs(shape, seed)
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        out.fill_(SENTINEL)
        graph.replay()
        with torch.no_grad():
            want = hip_ops.filter_interpolation(*fresh)
        assert torch.equal(out[:, c_off:c_off + C], want)
        assert (out[:, :c_off] == SENTINEL).all() and (out[:, c_off + C:] == SENTINEL).all()
