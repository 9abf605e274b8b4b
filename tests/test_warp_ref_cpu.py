"""CPU: the float64 restatement of the VoxelFlow tail and of the pixel-flow backward warp (tests/warp_ref.py).

The GPU suite (tests/test_warp_gpu.py) holds csrc/voxelwarp.hip and csrc/flowwarp.hip to this reference inside bounds that are counted,
not measured.  Here the reference is held to ATen's F.grid_sample in float64 -- values and autograd gradients, border clamp with
align_corners=True and zero padding with align_corners=False -- on inputs whose coordinates sit exactly on integers, half cells, the clip
bounds and outside (lattice) and on odd sizes with continuous flows (ragged); the oracle's statements and the composed op that
--second_order takes are held to it in the same way, which is where a coordinate exactly on the lower clip bound used to pass a gradient
that ATen and the fused kernel do not; and references with one wrong convention are shown to MISS the bounds, so that the bounds are
known to be able to fail."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import hip_ops
from oracle import torch_ops as O
from tests import warp_ref as R

VOXEL_LATTICE = [(2, 5, 9), (1, 9, 17), (1, 2, 3), (1, 1, 9), (1, 5, 1), (1, 2, 513)]          # B, H, W
VOXEL_RAGGED = [(2, 33, 47), (1, 6, 70), (1, 3, 300)]
FLOW_LATTICE = [(2, 3, 8, 16), (1, 1, 1, 1), (1, 2, 4, 128), (1, 5, 2, 64)]                    # N, C, H, W
FLOW_RAGGED = [(1, 3, 6, 70), (2, 5, 3, 300), (1, 3, 37, 53)]
# float64 against float64: ATen's vectorised kernels and autograd associate differently from the reference and may fuse a product and a
# sum of the coordinate, which moves a coordinate of up to 512 px by a few times 2^-53 * 512 = 2^-44 px.  2^-40 of the sum of magnitudes
# covers both with room: 13 bits above float64's rounding, 16 bits below the float32 bounds the kernels are held to -- no wrong convention
# fits in there.  (In bound_ratio's units of 2^-24.)
F64_UNITS = 2.0 ** -16


def _voxel_autograd(fn, frames, x3, gout):
    fr, xr = frames.double().requires_grad_(), x3.double().requires_grad_()
    out = fn(fr, xr)
    g_fr, g_x3 = torch.autograd.grad(out, (fr, xr), gout.double())
    return out.detach(), g_x3, g_fr


def _hold_voxel(fn, frames, x3, gout, ref, keep):
    """values, g_frames at every pixel and g_x3 at the pixels of `keep` inside the float64 bound; returns the largest ratio"""
    out, g_x3, g_fr = _voxel_autograd(fn, frames, x3, gout)
    ratios = (R.bound_ratio(out, ref['out'], ref['out_mag'], F64_UNITS),
              R.masked_ratio(g_x3, ref['g_x3'], ref['g_x3_mag'], F64_UNITS, keep),
              R.bound_ratio(g_fr, ref['g_frames'], ref['g_frames_mag'] * ref['g_frames_units'], F64_UNITS))
    assert max(ratios) <= 1.0, ratios
    return max(ratios)


def _hold_flow(fn, img, flw, gout, ref, keep):
    fl = flw.double().requires_grad_()
    out = fn(img.double(), fl)
    g, = torch.autograd.grad(out, fl, gout.double())
    ratios = (R.bound_ratio(out.detach(), ref['out'], ref['out_mag'], F64_UNITS),
              R.masked_ratio(g, ref['gflow'], ref['gflow_mag'], F64_UNITS, keep))
    assert max(ratios) <= 1.0, ratios
    return max(ratios)


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VOXEL_LATTICE)
def test_voxel_lattice_coordinates_are_exact_and_sit_on_the_edges(shape):
    frames, x3, gout = R.voxel_lattice(*shape)                   # asserts float32 == float64 bit for bit and that both bounds are hit
    ref = R.voxel(frames, x3)
    assert ref['on_integer'] >= 0.2 and ref['clipped'] >= 0.07, (ref['on_integer'], ref['clipped'])
    assert x3.abs().max() <= 1 and frames.dtype == torch.float32 and gout.shape == x3.shape
    B, H, W = shape
    ax, ay, bx, by = R.voxel_coords(x3)
    assert (ax[:, 0, 0] == 0).all() and (bx[:, 0, W - 1] == W - 1).all() and (ay[:, 0, 0] == 0).all() and (by[:, H - 1, 0] == H - 1).all()
    if W >= 5:
        assert (ax[:, 0, 1] == 0).all() and (bx[:, 0, 1] == 2).all()             # the lower bound reached from inside


@pytest.mark.parametrize("shape", FLOW_LATTICE)
def test_flow_lattice_coordinates_are_exact_and_sit_on_the_edges(shape):
    img, flw, gout = R.flow_lattice(*shape)                      # asserts float32 == float64 bit for bit
    ref = R.flow(img, flw)
    assert ref['on_integer'] >= 0.2 and ref['outside'] >= 0.07, (ref['on_integer'], ref['outside'])
    N, C, H, W = shape
    ix, iy = R.flow_coords(flw)
    assert (flw[:, 0].abs() <= W + 2).all() and (flw[:, 1].abs() <= H + 2).all()
    for c, size in ((ix, W), (iy, H)):
        if size >= 8:                                            # the cells -1, size - 1, size, -2 and the parked ones on either side
            for want in (-1, size - 1, size, -2, -4, size + 2):
                assert (c == want).any(), want


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference against ATen
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VOXEL_LATTICE)
def test_voxel_reference_matches_aten_float64_on_the_lattice(shape):
    """F.grid_sample(border, align_corners=True) and the blend in float64, every pixel: values, g_x3 (exact zeros where a coordinate
    is clipped, the bounds included) and g_frames"""
    frames, x3, gout = R.voxel_lattice(*shape)
    ref = R.voxel(frames, x3, gout)
    _hold_voxel(O.voxel_warp_blend, frames, x3, gout, ref, torch.ones(shape, dtype=torch.bool))
    s = R.voxel_coords(x3)
    both_x = (~(s[0] > 0) | (s[0] >= shape[2] - 1)) & (~(s[2] > 0) | (s[2] >= shape[2] - 1))
    assert both_x.any() and (ref['g_x3'][:, 0][torch.from_numpy(both_x)] == 0).all()


@pytest.mark.parametrize("amp", [0.3, 2.0])
@pytest.mark.parametrize("shape", VOXEL_RAGGED)
def test_voxel_reference_matches_aten_float64_on_ragged_inputs(shape, amp):
    """with the coordinates in float64 on both sides; gradients at the pixels that are not flagged, and few are flagged"""
    frames, x3, gout = R.voxel_ragged(*shape, amp)
    ref = R.voxel(frames, x3, gout, coord=np.float64)
    share = ref['near'].float().mean().item()
    print("voxel ragged %s amp %g: flagged share %.2e" % (shape, amp, share))
    assert share <= R.NEAR_CAP
    _hold_voxel(O.voxel_warp_blend, frames, x3, gout, ref, ~ref['near'])
    _hold_voxel(O.voxel_warp_blend_written_out, frames, x3, gout, ref, ~ref['near'])


@pytest.mark.parametrize("amp", [0.3, 2.0])
@pytest.mark.parametrize("shape", VOXEL_RAGGED)
def test_voxel_float32_statements_are_inside_the_kernel_bounds(shape, amp):
    """ATen and the written-out statement in float32 on the CPU against the reference with the op's float32 coordinates, inside the
    bounds the kernel is held to (their expressions have the kernel's roundings or fewer).  amp 2 saturates the mask: with |1 - m| in
    place of |m| + |1 - m| in the sums of magnitudes these inputs are 3 (forward), 1000 (g_x3) and 4400 (g_frames) times outside."""
    frames, x3, gout = R.voxel_ragged(*shape, amp)
    ref = R.voxel(frames, x3, gout)
    keep = ~ref['near']
    for fn in (O.voxel_warp_blend, O.voxel_warp_blend_written_out):
        fr, xr = frames.clone().requires_grad_(), x3.clone().requires_grad_()
        out = fn(fr, xr)
        g_fr, g_x3 = torch.autograd.grad(out, (fr, xr), gout)
        ratios = (R.bound_ratio(out.detach(), ref['out'], ref['out_mag'], R.VOXEL_FWD_UNITS),
                  R.masked_ratio(g_x3[:, 0:2], ref['g_x3'][:, 0:2], ref['g_x3_mag'][:, 0:2], R.VOXEL_GFLOW_UNITS, keep),
                  R.masked_ratio(g_x3[:, 2:3], ref['g_x3'][:, 2:3], ref['g_x3_mag'][:, 2:3], R.VOXEL_GMASK_UNITS, keep),
                  R.bound_ratio(g_fr, ref['g_frames'], ref['g_frames_mag'] * ref['g_frames_units'], 1))
        print("float32 %s %s amp %g: of the bounds %s" % (fn.__name__, shape, amp, " ".join("%.2f" % r for r in ratios)))
        assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("shape", FLOW_LATTICE)
def test_flow_reference_matches_aten_float64_on_the_lattice(shape):
    """F.grid_sample(zeros, align_corners=False) behind the reference's normalisation, every pixel; the oracle's written-out statement too"""
    img, flw, gout = R.flow_lattice(*shape)
    ref = R.flow(img, flw, gout)
    keep = torch.ones(shape[0], shape[2], shape[3], dtype=torch.bool)
    _hold_flow(O.flow_warp_reference_ops, img, flw, gout, ref, keep)
    _hold_flow(O.flow_warp, img, flw, gout, ref, keep)


@pytest.mark.parametrize("amp", [1.0, 6.0, 30.0])
@pytest.mark.parametrize("shape", FLOW_RAGGED)
def test_flow_reference_matches_aten_float64_on_ragged_inputs(shape, amp):
    img, flw, gout = R.flow_ragged(*shape, amp)
    ref = R.flow(img, flw, gout, coord=np.float64)
    share = ref['near'].float().mean().item()
    print("flow ragged %s amp %g: flagged share %.2e" % (shape, amp, share))
    assert share <= R.NEAR_CAP
    _hold_flow(O.flow_warp_reference_ops, img, flw, gout, ref, ~ref['near'])
    _hold_flow(O.flow_warp, img, flw, gout, ref, ~ref['near'])


def test_flow_reference_samples_nothing_at_targets_that_are_not_finite_or_far_away():
    img, flw, gout = R.flow_lattice(2, 3, 8, 16)
    clean = R.flow(img, flw, gout)
    bad = flw.clone()
    spots = [(0, 0, 1, 2), (0, 1, 3, 5), (1, 0, 7, 15), (1, 1, 0, 0), (1, 0, 4, 4)]
    for (n, ch, y, x), v in zip(spots, (float('nan'), float('inf'), float('-inf'), 1e30, -1e30)):
        bad[n, ch, y, x] = v
    ref = R.flow(img, bad, gout)
    hit = torch.zeros(2, 8, 16, dtype=torch.bool)
    for n, _, y, x in spots:
        hit[n, y, x] = True
    for key in ('out', 'out_mag', 'gflow', 'gflow_mag'):
        k = hit.unsqueeze(1).expand_as(ref[key])
        assert (ref[key][k] == 0).all() and torch.equal(ref[key][~k], clean[key][~k]), key


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle's statements and the composed op
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [O.voxel_warp_blend, O.voxel_warp_blend_written_out, hip_ops._voxel_warp_composed],
                         ids=["aten", "written_out", "composed"])
@pytest.mark.parametrize("shape", VOXEL_LATTICE)
def test_voxel_statements_agree_with_the_reference_at_every_exact_bound(fn, shape):
    """The first-order pass (ATen, like the fused kernel) and the twice-differentiable statements that --second_order takes must hand the
    same derivative to a coordinate that sits exactly on a clip bound: zero.  clamp() alone gives slope one there, which showed as
    column 0 of d/dx3[:, 0] = [0.57, -0.05, -0.51, -0.54, -0.49] on a 5x9 map with x3 = 0 where ATen gives exact zeros."""
    frames, x3, gout = R.voxel_lattice(*shape)
    ref = R.voxel(frames, x3, gout)
    _hold_voxel(fn, frames, x3, gout, ref, torch.ones(shape, dtype=torch.bool))


@pytest.mark.parametrize("fn", [O.voxel_warp_blend_written_out, hip_ops._voxel_warp_composed], ids=["written_out", "composed"])
def test_voxel_border_gradient_is_zero_for_a_zero_flow(fn):
    frames, _, gout = R.voxel_lattice(1, 5, 9)
    for dtype in (torch.float32, torch.float64):
        x3 = torch.zeros(1, 3, 5, 9, dtype=dtype, requires_grad=True)
        g, = torch.autograd.grad(fn(frames.to(dtype), x3), x3, gout.to(dtype))
        assert (g[0, 0, :, 0] == 0).all() and (g[0, 0, :, 8] == 0).all() and (g[0, 1, 0, :] == 0).all() and (g[0, 1, 4, :] == 0).all()
        assert (g[0, 0, :, 1:8] != 0).any() and (g[0, 1, 1:4, :] != 0).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# the bounds can fail
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_bounds_tell_float64_coordinates_from_float32_ones():
    """at the largest width a coordinate computed in float64 is up to 2 * 2^-24 * 300 px away from the op's: many times the bounds"""
    frames, x3, gout = R.voxel_ragged(1, 3, 300, 0.3)
    ref, wrong = R.voxel(frames, x3, gout), R.voxel(frames, x3, gout, coord=np.float64)
    keep = ~ref['near']
    assert R.bound_ratio(wrong['out'], ref['out'], ref['out_mag'], R.VOXEL_FWD_UNITS) > 4
    assert R.masked_ratio(wrong['g_x3'][:, 2:3], ref['g_x3'][:, 2:3], ref['g_x3_mag'][:, 2:3], R.VOXEL_GMASK_UNITS, keep) > 4
    assert R.bound_ratio(wrong['g_frames'], ref['g_frames'], ref['g_frames_mag'] * ref['g_frames_units'], 1) > 4
    img, flw, gout = R.flow_ragged(2, 5, 3, 300, 6.0)
    ref, wrong = R.flow(img, flw, gout), R.flow(img, flw, gout, coord=np.float64)
    assert R.bound_ratio(wrong['out'], ref['out'], ref['out_mag'], R.FLOW_FWD_UNITS) > 4
    assert R.masked_ratio(wrong['gflow'], ref['gflow'], ref['gflow_mag'], R.flow_bwd_units(5), ~ref['near']) > 4


def test_the_bounds_tell_a_right_closed_cell_and_a_clamp_slope_from_the_convention():
    """on the lattice the values of a cell (i, i + 1] are the same (the op is continuous) and its gradients are not"""
    frames, x3, gout = R.voxel_lattice(2, 5, 9)
    ref, wrong = R.voxel(frames, x3, gout), R.voxel(frames, x3, gout, right_closed=True)
    assert R.bound_ratio(wrong['out'], ref['out'], ref['out_mag'], R.VOXEL_FWD_UNITS) <= 1
    assert R.bound_ratio(wrong['g_x3'][:, :2], ref['g_x3'][:, :2], ref['g_x3_mag'][:, :2], R.VOXEL_GFLOW_UNITS) > 100
    img, flw, gout = R.flow_lattice(2, 3, 8, 16)
    ref, wrong = R.flow(img, flw, gout), R.flow(img, flw, gout, right_closed=True)
    assert R.bound_ratio(wrong['out'], ref['out'], ref['out_mag'], R.FLOW_FWD_UNITS) <= 1
    assert R.bound_ratio(wrong['gflow'], ref['gflow'], ref['gflow_mag'], R.flow_bwd_units(3)) > 100
    # the slope of a bare clamp at the bounds: what the written-out statements computed before they took ATen's convention
    frames, x3, gout = R.voxel_lattice(2, 5, 9)
    ref = R.voxel(frames, x3, gout)

    def bare_clamp(fr, x):
        B, _, H, W = fr.shape
        gx, gy = (torch.from_numpy(R.mesh(n, np.float64)) for n in (W, H))
        out = 0
        for sign, img, m in ((-1, fr[:, 0:3], 0.5 * (1 + x[:, 2:3])), (1, fr[:, 3:6], 1 - 0.5 * (1 + x[:, 2:3]))):
            ix = ((gx.view(1, 1, W) + sign * 0.5 * x[:, 0] + 1) / 2 * (W - 1)).clamp(0, W - 1)
            iy = ((gy.view(1, H, 1) + sign * 0.5 * x[:, 1] + 1) / 2 * (H - 1)).clamp(0, H - 1)
            x0, y0 = ix.detach().floor().clamp(max=max(W - 2, 0)), iy.detach().floor().clamp(max=max(H - 2, 0))
            fx, fy = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
            flat = img.reshape(B, 3, H * W)

            def px(yy, xx):
                idx = (yy.long().clamp(max=H - 1) * W + xx.long().clamp(max=W - 1)).reshape(B, 1, H * W).expand(B, 3, H * W)
                return flat.gather(2, idx).reshape(B, 3, H, W)
            out = out + m * ((px(y0, x0) * (1 - fx) + px(y0, x0 + 1) * fx) * (1 - fy) + (px(y0 + 1, x0) * (1 - fx) + px(y0 + 1, x0 + 1) * fx) * fy)
        return out

    out, g_x3, _ = _voxel_autograd(bare_clamp, frames, x3, gout)
    assert R.bound_ratio(out, ref['out'], ref['out_mag'], R.VOXEL_FWD_UNITS) <= 1
    assert R.bound_ratio(g_x3[:, :2], ref['g_x3'][:, :2], ref['g_x3_mag'][:, :2], R.VOXEL_GFLOW_UNITS) > 100
