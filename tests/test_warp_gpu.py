"""-m gpu: the VoxelFlow tail (csrc/voxelwarp.hip) and the pixel-flow backward warp (csrc/flowwarp.hip) against the float64 restatement
of tests/warp_ref.py, inside bounds that count the roundings of the kernels' expressions (the constants of warp_ref, nothing measured).

Lattice inputs put the coordinates exactly on integers, quarter cells, the clip bounds and outside; no order of operations can move a
cell there, so every pixel is compared.  Ragged inputs have odd sizes and continuous flows; the reference takes the cell from the same
float32 coordinate as the kernel, gradients leave out the few pixels whose coordinate lies next to a cell edge (under a cap).
tests/test_warp_ref_cpu.py holds the reference itself to ATen in float64."""
import functools

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from oracle import torch_ops as O
from tests import warp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_NULL, E_SHAPE = -1, -2
CANARY, PAD = 7777.0, 4096

VOXEL_LATTICE = [(2, 5, 9), (1, 9, 17), (1, 2, 3), (1, 1, 9), (1, 5, 1), (1, 2, 513)]      # B, H, W; 513: a second 256-wide block, lanes past W
VOXEL_RAGGED = [(2, 33, 47), (1, 6, 70), (1, 3, 300)]
FLOW_LATTICE = [(2, 3, 8, 16), (1, 1, 1, 1), (1, 2, 4, 128), (1, 5, 2, 64)]                # N, C, H, W; the last two span two x tiles
FLOW_RAGGED = [(1, 3, 6, 70), (2, 5, 3, 300), (1, 3, 37, 53)]


@functools.lru_cache(maxsize=None)
def _voxel_case(shape, amp):
    """inputs and their reference, computed once and shared; amp None: the lattice"""
    frames, x3, gout = R.voxel_lattice(*shape) if amp is None else R.voxel_ragged(*shape, amp)
    return frames, x3, gout, R.voxel(frames, x3, gout)


@functools.lru_cache(maxsize=None)
def _flow_case(shape, amp):
    img, flw, gout = R.flow_lattice(*shape) if amp is None else R.flow_ragged(*shape, amp)
    return img, flw, gout, R.flow(img, flw, gout)


def _keep(ref, amp):
    """lattice: every pixel; ragged: the pixels that are not flagged, and the flagged share is under the cap"""
    if amp is None:
        return torch.ones_like(ref['near'])
    share = ref['near'].float().mean().item()
    print("  flagged share %.2e" % share)
    assert share <= R.NEAR_CAP, share
    return ~ref['near']


def _voxel_op(frames, x3, gout, frames_grad=True):
    fd, xd = frames.to(DEV).requires_grad_(frames_grad), x3.to(DEV).requires_grad_()
    out = hip_ops.voxel_warp_blend(fd, xd)
    out.backward(gout.to(DEV))
    return out.detach(), xd.grad, fd.grad


def _voxel_abi(frames, x3, gout, want_frames):
    """savfi_voxelwarp_{fwd,bwd}_f32 with every output inside a canary-filled buffer: (out, g_x3, g_frames or None)"""
    B, _, H, W = frames.shape
    lib, st = _hip.lib(), _hip.current_stream()
    fd, xd, gd = frames.to(DEV).contiguous(), x3.to(DEV).contiguous(), gout.to(DEV).contiguous()
    sizes = dict(out=B * 3 * H * W, g_x3=B * 3 * H * W, g_fr=B * 6 * H * W)
    bufs = {k: torch.full((n + 2 * PAD,), CANARY, device=DEV) for k, n in sizes.items()}
    bufs['g_fr'][PAD:PAD + sizes['g_fr']] = 0                      # the frame gradient is accumulated into a zeroed buffer
    _hip.check(lib.savfi_voxelwarp_fwd_f32(fd.data_ptr(), xd.data_ptr(), bufs['out'][PAD:].data_ptr(), B, H, W, st), "voxelwarp fwd")
    _hip.check(lib.savfi_voxelwarp_bwd_f32(fd.data_ptr(), xd.data_ptr(), gd.data_ptr(), bufs['g_x3'][PAD:].data_ptr(),
                                           bufs['g_fr'][PAD:].data_ptr() if want_frames else None, B, H, W, st), "voxelwarp bwd")
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert torch.all(bufs[k][:PAD] == CANARY) and torch.all(bufs[k][PAD + n:] == CANARY), k
    if not want_frames:
        assert torch.all(bufs['g_fr'][PAD:PAD + sizes['g_fr']] == 0)
    return (bufs['out'][PAD:PAD + sizes['out']].view(B, 3, H, W), bufs['g_x3'][PAD:PAD + sizes['g_x3']].view(B, 3, H, W),
            bufs['g_fr'][PAD:PAD + sizes['g_fr']].view(B, 6, H, W) if want_frames else None)


def _hold_voxel(tag, out, g_x3, g_fr, ref, keep):
    ratios = dict(fwd=R.bound_ratio(out, ref['out'], ref['out_mag'], R.VOXEL_FWD_UNITS),
                  g_flow=R.masked_ratio(g_x3[:, 0:2], ref['g_x3'][:, 0:2], ref['g_x3_mag'][:, 0:2], R.VOXEL_GFLOW_UNITS, keep),
                  g_mask=R.masked_ratio(g_x3[:, 2:3], ref['g_x3'][:, 2:3], ref['g_x3_mag'][:, 2:3], R.VOXEL_GMASK_UNITS, keep),
                  g_frames=R.bound_ratio(g_fr, ref['g_frames'], ref['g_frames_mag'] * ref['g_frames_units'], 1))
    print("  %s: of the bound" % tag, " ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("shape,amp", [(s, None) for s in VOXEL_LATTICE] + [(s, a) for s in VOXEL_RAGGED for a in (0.3, 2.0)])
def test_voxelwarp_fused_op_against_float64(shape, amp):
    """forward, g_x3 and g_frames of the fused op inside the counted bounds; bit-identical on a second run; and the production backward
    -- the frames are inputs there, so the kernel instance is voxelwarp_bwd<false> with g_frames == nullptr -- gives the g_x3 of the
    instance that also scatters, bit for bit, through the C ABI and through hip_ops when only x3 requires grad."""
    frames, x3, gout, ref = _voxel_case(shape, amp)
    print("\nvoxel %s amp %s: on integers %.2f, clipped %.2f" % (shape, amp, ref['on_integer'], ref['clipped']))
    keep = _keep(ref, amp)
    out, g_x3, g_fr = _voxel_op(frames, x3, gout)
    _hold_voxel("fused", out, g_x3, g_fr, ref, keep)
    out2, g_x3_2, _ = _voxel_op(frames, x3, gout)
    assert torch.equal(out2, out) and torch.equal(g_x3_2, g_x3)
    out3, g_x3_3, none = _voxel_op(frames, x3, gout, frames_grad=False)
    assert none is None and torch.equal(out3, out) and torch.equal(g_x3_3, g_x3)
    a_out, a_gx, a_gf = _voxel_abi(frames, x3, gout, want_frames=True)
    b_out, b_gx, _ = _voxel_abi(frames, x3, gout, want_frames=False)
    assert torch.equal(a_out, out) and torch.equal(a_gx, g_x3) and torch.equal(b_out, out) and torch.equal(b_gx, g_x3)
    assert R.bound_ratio(a_gf, ref['g_frames'], ref['g_frames_mag'] * ref['g_frames_units'], 1) <= 1.0


def test_voxelwarp_composed_op_agrees_with_the_fused_op_at_every_exact_bound():
    """_voxel_warp_composed (what --second_order takes) on the device: forward and first-order gradients inside the same bounds of the
    same reference as the fused op, so the two passes of one model hand the same derivative to a coordinate on a clip bound.  Its
    expression has the fused kernel's counts: 10 for the forward; for g_x3's flow channels the mask (2), g * mask (1), 1 - fy and its
    product (2), the product with a texel (1), two sums over the channels (2), three sums of the four corner terms (3, where the kernel
    has a texel difference, a sum and the tap difference), the product with size - 1 (1) = 12, the sum of the two taps being the
    kernel's difference."""
    frames, x3, gout, ref = _voxel_case((2, 5, 9), None)
    fd, xd = frames.to(DEV).requires_grad_(), x3.to(DEV).requires_grad_()
    out = hip_ops._voxel_warp_composed(fd, xd)
    g_fr, g_x3 = torch.autograd.grad(out, (fd, xd), gout.to(DEV))
    _hold_voxel("composed", out, g_x3, g_fr, ref, torch.ones_like(ref['near']))


def test_voxelwarp_composed_op_hessian_vector_product():
    """One Hessian-vector product of sum(gout * out) in x3 on a ragged 5x9 map, against float64 CPU autograd through the oracle's
    written-out statement.  Relative to max |Hv| of the float64 result, float32 on the CPU is 1.4e-7 away for this input (the oracle's
    statement; the composed op 1.3e-7) and at most 2.7e-7 over twelve other draws: the bound is 1e-6, four times the worst of them (the device: 1.3e-7)."""
    frames, x3, gout = R.voxel_ragged(1, 5, 9, 1.0)
    v = torch.randn(x3.shape, generator=torch.Generator().manual_seed(1))

    def hvp(fn, fr, x, go, vec):
        x = x.clone().requires_grad_()
        g, = torch.autograd.grad(fn(fr, x), x, go, create_graph=True)
        return torch.autograd.grad((g * vec).sum(), x)[0]

    want = hvp(O.voxel_warp_blend_written_out, frames.double(), x3.double(), gout.double(), v.double())
    got = hvp(hip_ops._voxel_warp_composed, frames.to(DEV), x3.to(DEV), gout.to(DEV), v.to(DEV)).cpu().double()
    err = ((got - want).abs().max() / want.abs().max()).item()
    print("\nHVP: %.2e of max |Hv| = %.3g" % (err, want.abs().max().item()))
    assert (want != 0).float().mean() > 0.5 and err <= 1e-6, err


# ------------------------------------------------------------------------------------------------------------------------------------
def _flow_op(img, flw, gout):
    fd = flw.to(DEV).requires_grad_()
    out = hip_ops.flow_warp(img.to(DEV), fd)
    out.backward(gout.to(DEV))
    return out.detach(), fd.grad


def _flow_abi(img, flw, gout):
    """savfi_flowwarp_{fwd,bwd}_f32 with both outputs inside canary-filled buffers"""
    N, C, H, W = img.shape
    lib, st = _hip.lib(), _hip.current_stream()
    im, fd, gd = img.to(DEV).contiguous(), flw.to(DEV).contiguous(), gout.to(DEV).contiguous()
    sizes = dict(out=N * C * H * W, gflow=N * 2 * H * W)
    bufs = {k: torch.full((n + 2 * PAD,), CANARY, device=DEV) for k, n in sizes.items()}
    _hip.check(lib.savfi_flowwarp_fwd_f32(im.data_ptr(), fd.data_ptr(), bufs['out'][PAD:].data_ptr(), N, C, H, W, st), "flowwarp fwd")
    _hip.check(lib.savfi_flowwarp_bwd_f32(im.data_ptr(), fd.data_ptr(), gd.data_ptr(), bufs['gflow'][PAD:].data_ptr(), N, C, H, W, st),
               "flowwarp bwd")
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert torch.all(bufs[k][:PAD] == CANARY) and torch.all(bufs[k][PAD + n:] == CANARY), k
    return bufs['out'][PAD:PAD + sizes['out']].view(N, C, H, W), bufs['gflow'][PAD:PAD + sizes['gflow']].view(N, 2, H, W)


@pytest.mark.parametrize("shape,amp", [(s, None) for s in FLOW_LATTICE] + [(s, a) for s in FLOW_RAGGED for a in (1.0, 6.0, 30.0)])
def test_flowwarp_against_float64(shape, amp):
    """forward and gflow inside the counted bounds, bit-identical on a second run and through the C ABI with canaries around the outputs"""
    img, flw, gout, ref = _flow_case(shape, amp)
    print("\nflow %s amp %s: on integers %.2f, outside %.2f" % (shape, amp, ref['on_integer'], ref['outside']))
    keep = _keep(ref, amp)
    out, gflow = _flow_op(img, flw, gout)
    ratios = dict(fwd=R.bound_ratio(out, ref['out'], ref['out_mag'], R.FLOW_FWD_UNITS),
                  gflow=R.masked_ratio(gflow, ref['gflow'], ref['gflow_mag'], R.flow_bwd_units(shape[1]), keep))
    print("  of the bound", " ".join("%s %.3f" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    out2, gflow2 = _flow_op(img, flw, gout)
    assert torch.equal(out2, out) and torch.equal(gflow2, gflow)
    a_out, a_g = _flow_abi(img, flw, gout)
    assert torch.equal(a_out, out) and torch.equal(a_g, gflow)


def test_flowwarp_samples_nothing_where_the_flow_is_not_finite_or_far_away():
    """NaN, +-inf and +-1e30 flows: the output AND the flow gradient are exactly zero there (not NaN), every other pixel is what it is
    without them, and all of it is inside the bounds of the reference"""
    shape = (2, 3, 8, 16)
    img, flw, gout, clean = _flow_case(shape, None)
    bad = flw.clone()
    spots = [(0, 0, 1, 2), (0, 1, 3, 5), (1, 0, 7, 15), (1, 1, 0, 0), (1, 0, 4, 4), (0, 1, 7, 0)]
    for (n, ch, y, x), value in zip(spots, (float('nan'), float('inf'), float('-inf'), 1e30, -1e30, float('nan'))):
        bad[n, ch, y, x] = value
    hit = torch.zeros(2, 8, 16, dtype=torch.bool)
    for n, _, y, x in spots:
        hit[n, y, x] = True
    out, gflow = _flow_op(img, bad, gout)
    out0, gflow0 = _flow_op(img, flw, gout)
    for got, base in ((out.cpu(), out0.cpu()), (gflow.cpu(), gflow0.cpu())):
        k = hit.unsqueeze(1).expand_as(got)
        assert not torch.isnan(got).any() and (got[k] == 0).all() and torch.equal(got[~k], base[~k])
    ref = R.flow(img, bad, gout)
    assert R.bound_ratio(out, ref['out'], ref['out_mag'], R.FLOW_FWD_UNITS) <= 1.0
    assert R.bound_ratio(gflow, ref['gflow'], ref['gflow_mag'], R.flow_bwd_units(3)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
def test_warp_entry_points_refuse_null_pointers_and_bad_extents():
    lib, st = _hip.lib(), _hip.current_stream()
    P = torch.zeros(64, device=DEV).data_ptr()
    vf, vb, ff, fb = lib.savfi_voxelwarp_fwd_f32, lib.savfi_voxelwarp_bwd_f32, lib.savfi_flowwarp_fwd_f32, lib.savfi_flowwarp_bwd_f32
    for k in range(3):
        assert vf(*[None if i == k else P for i in range(3)], 1, 2, 2, st) == E_NULL
        assert ff(*[None if i == k else P for i in range(3)], 1, 1, 2, 2, st) == E_NULL
    for k in range(4):                                                              # g_frames alone may be null
        assert vb(*[None if i == k else P for i in range(4)], P, 1, 2, 2, st) == E_NULL
        assert fb(*[None if i == k else P for i in range(4)], 1, 1, 2, 2, st) == E_NULL
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2), (1, -3, 2), (1, 2, -3), (1, 65536, 1)):
        assert vf(P, P, P, *dims, st) == E_SHAPE and vb(P, P, P, P, P, *dims, st) == E_SHAPE and vb(P, P, P, P, None, *dims, st) == E_SHAPE
    for dims in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 0, 2), (1, 1, 2, 0), (-1, 1, 2, 2), (1, -1, 2, 2), (1, 1, -2, 2), (1, 1, 2, -2)):
        assert ff(P, P, P, *dims, st) == E_SHAPE and fb(P, P, P, P, *dims, st) == E_SHAPE
    torch.cuda.synchronize()
