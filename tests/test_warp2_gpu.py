"""-m gpu: the second backward of the VoxelFlow tail (savfi_voxelwarp_bwd2_f32, csrc/voxelwarp.hip) and of the pixel-flow warp
(savfi_flowwarp_bwd2_f32, csrc/flowwarp.hip) against the float64 restatement of tests/warp2_ref.py, inside bounds that count the
roundings of the kernels' expressions (the constants of warp2_ref, nothing measured), on the shapes of tests/test_warp_gpu.py.

Lattice inputs put the coordinates exactly on integers, quarter cells, the clip bounds and outside: every pixel is compared.  Ragged
inputs have odd sizes and continuous flows: the pixels whose coordinate lies next to a cell edge are left out, under a cap.
tests/test_warp2_ref_cpu.py holds the restatement itself to double autograd in float64."""
import functools

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import warp_ref as R
from tests import warp2_ref as R2

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_NULL, E_SHAPE, E_TOOBIG = -1, -2, -4
CANARY, PAD = 7777.0, 4096

VOXEL_LATTICE = [(2, 5, 9), (1, 9, 17), (1, 2, 3), (1, 1, 9), (1, 5, 1), (1, 2, 513)]      # B, H, W; 513: a second 256-wide block, lanes past W
VOXEL_RAGGED = [(2, 33, 47), (1, 6, 70), (1, 3, 300)]
FLOW_LATTICE = [(2, 3, 8, 16), (1, 1, 1, 1), (1, 2, 4, 128), (1, 5, 2, 64)]                # N, C, H, W; the last two span two x tiles
FLOW_RAGGED = [(1, 3, 6, 70), (2, 5, 3, 300), (1, 3, 37, 53)]


@pytest.fixture
def second_order_pass():
    """the switches the meta system sets for a second-order pass with --warp_second_order 1, on this thread"""
    hip_ops.set_double_backward(True)
    hip_ops.set_warp_second_order(True)
    yield
    hip_ops.set_double_backward(False)
    hip_ops.set_warp_second_order(False)


@functools.lru_cache(maxsize=None)
def _voxel_case(shape, amp):
    """inputs and their reference, computed once and shared; amp None: the lattice"""
    frames, x3, gout = R.voxel_lattice(*shape) if amp is None else R.voxel_ragged(*shape, amp)
    v = R2.cotangent(x3)
    return frames, x3, gout, v, R2.voxel2(frames, x3, gout, v)


@functools.lru_cache(maxsize=None)
def _flow_case(shape, amp):
    img, flw, gout = R.flow_lattice(*shape) if amp is None else R.flow_ragged(*shape, amp)
    v = R2.cotangent(flw)
    return img, flw, gout, v, R2.flow2(img, flw, gout, v)


def _keep(ref, amp):
    """lattice: every pixel; ragged: the pixels that are not flagged, and the flagged share is under the cap"""
    if amp is None:
        return torch.ones_like(ref['near'])
    share = ref['near'].float().mean().item()
    print("  flagged share %.2e" % share)
    assert share <= R.NEAR_CAP, share
    return ~ref['near']


def _abi(entry, operands, shapes, dims, want=(True, True)):
    """one launch of a bwd2 entry with each output inside a canary-padded, NaN-filled buffer: the requested outputs (None for the
    other); an output that was not requested must come back untouched, NaN for NaN"""
    lib, st = _hip.lib(), _hip.current_stream()
    dev = [t.to(DEV).contiguous() for t in operands]
    bufs, views = [], []
    for shape in shapes:
        n = 1
        for k in shape:
            n *= k
        buf = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        buf[PAD:PAD + n] = float('nan')
        bufs.append((buf, n))
        views.append(buf[PAD:PAD + n].view(*shape))
    ptrs = [views[k].data_ptr() if want[k] else None for k in range(2)]
    _hip.check(getattr(lib, entry)(*[t.data_ptr() for t in dev], *ptrs, *dims, st), entry)
    torch.cuda.synchronize()
    for k, (buf, n) in enumerate(bufs):
        assert torch.all(buf[:PAD] == CANARY) and torch.all(buf[PAD + n:] == CANARY), (entry, k)
        if want[k]:
            assert not torch.isnan(views[k]).any(), (entry, k, "an element was not written")
        else:
            assert torch.isnan(views[k]).all(), (entry, k, "an output that was not requested was written")
    return [views[k] if want[k] else None for k in range(2)]


def _voxel_abi(frames, x3, gout, v, want=(True, True)):
    B, _, H, W = frames.shape
    return _abi("savfi_voxelwarp_bwd2_f32", (frames, x3, gout, v), [(B, 3, H, W), (B, 3, H, W)], (B, H, W), want)


def _flow_abi(img, flw, gout, v, want=(True, True)):
    N, C, H, W = img.shape
    return _abi("savfi_flowwarp_bwd2_f32", (img, flw, gout, v), [(N, C, H, W), (N, 2, H, W)], (N, C, H, W), want)


def _twice(fn, a, x, gout, v, third=False):
    """(d_gout, d_x) of <grad_x <gout, fn(a, x)>, v> through autograd on the device"""
    ad, xd, gd = a.to(DEV), x.to(DEV).requires_grad_(), gout.to(DEV).requires_grad_()
    g, = torch.autograd.grad(fn(ad, xd), xd, gd, create_graph=True)
    assert g.requires_grad
    if third:
        d_x, = torch.autograd.grad((g * v.to(DEV)).sum(), xd, create_graph=True)
        return d_x, xd
    return torch.autograd.grad((g * v.to(DEV)).sum(), (gd, xd))


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,amp", [(s, None) for s in VOXEL_LATTICE] + [(s, a) for s in VOXEL_RAGGED for a in (0.3, 2.0)])
def test_voxelwarp_bwd2_against_float64(shape, amp, second_order_pass):
    """d_gO and d_x3 through the C ABI inside the counted bounds; through hip_ops.voxel_warp_blend and two autograd.grad calls the
    same bits; a second launch the same bits; with one output pointer null the other output's bits and nothing written for the null one"""
    frames, x3, gout, v, ref = _voxel_case(shape, amp)
    print("\nvoxel %s amp %s" % (shape, amp))
    keep = _keep(ref, amp)
    d_gO, d_x3 = _voxel_abi(frames, x3, gout, v)
    ratios = dict(d_gO=R.masked_ratio(d_gO, ref['d_gO'], ref['d_gO_mag'], R2.VOXEL_DGO_UNITS, keep),
                  d_flow=R.masked_ratio(d_x3[:, 0:2], ref['d_x3'][:, 0:2], ref['d_x3_mag'][:, 0:2], R2.VOXEL_DFLOW_UNITS, keep),
                  d_mask=R.masked_ratio(d_x3[:, 2:3], ref['d_x3'][:, 2:3], ref['d_x3_mag'][:, 2:3], R2.VOXEL_DMASK_UNITS, keep))
    print("  of the bound", " ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    o_gO, o_x3 = _twice(hip_ops.voxel_warp_blend, frames, x3, gout, v)
    assert torch.equal(o_gO, d_gO) and torch.equal(o_x3, d_x3)
    again = _voxel_abi(frames, x3, gout, v)
    assert torch.equal(again[0], d_gO) and torch.equal(again[1], d_x3)
    only_g, none = _voxel_abi(frames, x3, gout, v, want=(True, False))
    assert none is None and torch.equal(only_g, d_gO)
    none, only_x = _voxel_abi(frames, x3, gout, v, want=(False, True))
    assert none is None and torch.equal(only_x, d_x3)


@pytest.mark.parametrize("shape,amp", [(s, None) for s in FLOW_LATTICE] + [(s, a) for s in FLOW_RAGGED for a in (1.0, 6.0, 30.0)])
def test_flowwarp_bwd2_against_float64(shape, amp, second_order_pass):
    img, flw, gout, v, ref = _flow_case(shape, amp)
    print("\nflow %s amp %s" % (shape, amp))
    keep = _keep(ref, amp)
    d_gout, d_flow = _flow_abi(img, flw, gout, v)
    ratios = dict(d_gout=R.masked_ratio(d_gout, ref['d_gout'], ref['d_gout_mag'], R2.FLOW_DGOUT_UNITS, keep),
                  d_flow=R.masked_ratio(d_flow, ref['d_flow'], ref['d_flow_mag'], R2.flow_dflow_units(shape[1]), keep))
    print("  of the bound", " ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    o_gout, o_flow = _twice(hip_ops.flow_warp, img, flw, gout, v)
    assert torch.equal(o_gout, d_gout) and torch.equal(o_flow, d_flow)
    again = _flow_abi(img, flw, gout, v)
    assert torch.equal(again[0], d_gout) and torch.equal(again[1], d_flow)
    only_g, none = _flow_abi(img, flw, gout, v, want=(True, False))
    assert none is None and torch.equal(only_g, d_gout)
    none, only_f = _flow_abi(img, flw, gout, v, want=(False, True))
    assert none is None and torch.equal(only_f, d_flow)


def test_flowwarp_bwd2_gives_zeros_where_the_flow_is_not_finite_or_far_away(second_order_pass):
    """NaN, +-inf and +-1e30 flows: d_gout, d_flow (and the first-order gflow the autograd path computes on its way) are exactly zero
    there, not NaN; every other pixel is what it is without them, and all of it is inside the bounds of the reference"""
    shape = (2, 3, 8, 16)
    img, flw, gout, v, clean = _flow_case(shape, None)
    bad = flw.clone()
    spots = [(0, 0, 1, 2), (0, 1, 3, 5), (1, 0, 7, 15), (1, 1, 0, 0), (1, 0, 4, 4), (0, 1, 7, 0)]
    for (n, ch, y, x), value in zip(spots, (float('nan'), float('inf'), float('-inf'), 1e30, -1e30, float('nan'))):
        bad[n, ch, y, x] = value
    hit = torch.zeros(2, 8, 16, dtype=torch.bool)
    for n, _, y, x in spots:
        hit[n, y, x] = True
    d_gout, d_flow = _flow_abi(img, bad, gout, v)
    d_gout0, d_flow0 = _flow_abi(img, flw, gout, v)
    fd = bad.to(DEV).requires_grad_()
    gflow, = torch.autograd.grad(hip_ops.flow_warp(img.to(DEV), fd), fd, gout.to(DEV), create_graph=True)
    fd0 = flw.to(DEV).requires_grad_()
    gflow0, = torch.autograd.grad(hip_ops.flow_warp(img.to(DEV), fd0), fd0, gout.to(DEV))
    for got, base in ((d_gout.cpu(), d_gout0.cpu()), (d_flow.cpu(), d_flow0.cpu()), (gflow.detach().cpu(), gflow0.cpu())):
        k = hit.unsqueeze(1).expand_as(got)
        assert not torch.isnan(got).any() and (got[k] == 0).all() and torch.equal(got[~k], base[~k])
    ref = R2.flow2(img, bad, gout, v)
    assert R.bound_ratio(d_gout, ref['d_gout'], ref['d_gout_mag'], R2.FLOW_DGOUT_UNITS) <= 1.0
    assert R.bound_ratio(d_flow, ref['d_flow'], ref['d_flow_mag'], R2.flow_dflow_units(3)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
def test_a_third_derivative_raises(second_order_pass):
    frames, x3, gout, v, _ = _voxel_case((2, 5, 9), None)
    d_x, xd = _twice(hip_ops.voxel_warp_blend, frames, x3, gout, v, third=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(d_x.sum(), xd)
    img, flw, gout, v, _ = _flow_case((2, 3, 8, 16), None)
    d_f, fd = _twice(hip_ops.flow_warp, img, flw, gout, v, third=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(d_f.sum(), fd)


def test_frames_that_require_grad_are_refused(second_order_pass):
    frames, x3, _, _, _ = _voxel_case((2, 5, 9), None)
    with pytest.raises(NotImplementedError):
        hip_ops.voxel_warp_blend(frames.to(DEV).requires_grad_(), x3.to(DEV).requires_grad_())
    with pytest.raises(NotImplementedError):
        hip_ops._VoxelWarpTwice.apply(frames.to(DEV).requires_grad_(), x3.to(DEV))
    img, flw, _, _, _ = _flow_case((2, 3, 8, 16), None)
    with pytest.raises(NotImplementedError):
        hip_ops.flow_warp(img.to(DEV).requires_grad_(), flw.to(DEV).requires_grad_())
    with pytest.raises(NotImplementedError):
        hip_ops._FlowWarpTwice.apply(img.to(DEV).requires_grad_(), flw.to(DEV))


def test_first_order_through_the_twice_differentiable_ops_is_the_fused_ops_bits(second_order_pass):
    """forward and first-order gradient of _VoxelWarpTwice / _FlowWarpTwice go through the entry points of _VoxelWarp / _FlowWarp"""
    frames, x3, gout, _, _ = _voxel_case((1, 9, 17), None)
    outs = []
    for op in (hip_ops._VoxelWarpTwice, hip_ops._VoxelWarp):
        xd = x3.to(DEV).requires_grad_()
        out = op.apply(frames.to(DEV), xd)
        outs.append((out.detach(), torch.autograd.grad(out, xd, gout.to(DEV))[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    img, flw, gout, _, _ = _flow_case((2, 3, 8, 16), None)
    outs = []
    for op in (hip_ops._FlowWarpTwice, hip_ops._FlowWarp):
        fd = flw.to(DEV).requires_grad_()
        out = op.apply(img.to(DEV), fd)
        outs.append((out.detach(), torch.autograd.grad(out, fd, gout.to(DEV))[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_with_the_switch_off_the_ops_are_what_they_were():
    """second-order pass, --warp_second_order 0: voxel_warp_blend is the composed form (its graph has no _VoxelWarp node of either kind
    and differentiates twice), flow_warp is _FlowWarp and raises at the second backward; first-order pass with the switch on: both are
    the once-differentiable fused ops"""
    frames, x3, gout, v, ref = _voxel_case((2, 5, 9), None)
    img, flw, fgout, fv, _ = _flow_case((2, 3, 8, 16), None)
    assert not hip_ops.double_backward() and not hip_ops.warp_second_order()
    hip_ops.set_double_backward(True)
    try:
        out = hip_ops.voxel_warp_blend(frames.to(DEV), x3.to(DEV).requires_grad_())
        assert "VoxelWarp" not in type(out.grad_fn).__name__
        d_gO, d_x3 = _twice(hip_ops.voxel_warp_blend, frames, x3, gout, v)
        assert torch.isfinite(d_x3).all() and torch.isfinite(d_gO).all()
        fd = flw.to(DEV).requires_grad_()
        fout = hip_ops.flow_warp(img.to(DEV), fd)
        assert type(fout.grad_fn).__name__ == "_FlowWarpBackward"
        g, = torch.autograd.grad(fout, fd, fgout.to(DEV), create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad((g * fv.to(DEV)).sum(), fd)
    finally:
        hip_ops.set_double_backward(False)
    hip_ops.set_warp_second_order(True)
    try:
        out = hip_ops.voxel_warp_blend(frames.to(DEV), x3.to(DEV).requires_grad_())
        fout = hip_ops.flow_warp(img.to(DEV), flw.to(DEV).requires_grad_())
        assert type(out.grad_fn).__name__ == "_VoxelWarpBackward" and type(fout.grad_fn).__name__ == "_FlowWarpBackward"
    finally:
        hip_ops.set_warp_second_order(False)


def test_bwd2_entry_points_refuse_null_pointers_and_bad_extents():
    lib, st = _hip.lib(), _hip.current_stream()
    P = torch.zeros(64, device=DEV).data_ptr()
    vb2, fb2 = lib.savfi_voxelwarp_bwd2_f32, lib.savfi_flowwarp_bwd2_f32
    for k in range(4):
        assert vb2(*[None if i == k else P for i in range(4)], P, P, 1, 2, 2, st) == E_NULL
        assert fb2(*[None if i == k else P for i in range(4)], P, P, 1, 1, 2, 2, st) == E_NULL
    assert vb2(P, P, P, P, None, None, 1, 2, 2, st) == E_NULL and fb2(P, P, P, P, None, None, 1, 1, 2, 2, st) == E_NULL
    for outs in ((P, P), (P, None), (None, P)):
        for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2), (1, -3, 2), (1, 2, -3), (1, 65536, 1)):
            assert vb2(P, P, P, P, *outs, *dims, st) == E_SHAPE
        for dims in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 0, 2), (1, 1, 2, 0), (-1, 1, 2, 2), (1, -1, 2, 2), (1, 1, -2, 2), (1, 1, 2, -2)):
            assert fb2(P, P, P, P, *outs, *dims, st) == E_SHAPE
        assert fb2(P, P, P, P, *outs, 65536, 1, 1, 1, st) == E_TOOBIG
    torch.cuda.synchronize()
