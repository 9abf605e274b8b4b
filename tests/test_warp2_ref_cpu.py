"""CPU: the float64 restatement of the two warps' second backward (tests/warp2_ref.py) against double autograd through the oracle's
written-out statements; references with one wrong convention shown to MISS the bounds the kernels are held to; the flag; the two entry
points of the C ABI as far as they go without a device; and the conditioning of the second-order system comparisons of
tests/test_warp2_system_gpu.py (the oracle in float32 against the oracle in float64)."""
import re
import subprocess

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, config
from meta_interpolation_amd.config import default_args
from oracle import torch_ops as O
from tests import warp_ref as R
from tests import warp2_ref as R2

VOXEL_LATTICE = [(2, 5, 9), (1, 9, 17), (1, 2, 3), (1, 1, 9), (1, 5, 1), (1, 2, 513)]          # B, H, W
VOXEL_RAGGED = [(2, 33, 47), (1, 6, 70), (1, 3, 300)]
FLOW_LATTICE = [(2, 3, 8, 16), (1, 1, 1, 1), (1, 2, 4, 128), (1, 5, 2, 64)]                    # N, C, H, W
FLOW_RAGGED = [(1, 3, 6, 70), (2, 5, 3, 300), (1, 3, 37, 53)]
# float64 against float64, as in tests/test_warp_ref_cpu.py: autograd associates differently from the restatement and may move a
# coordinate of up to 512 px by a few times 2^-53 * 512 = 2^-44 px.  2^-40 of the sum of magnitudes covers both with room and is 16 bits
# below the float32 bounds the kernels are held to.  (In bound_ratio's units of 2^-24.)
F64_UNITS = 2.0 ** -16
E_NULL, E_SHAPE, E_TOOBIG = -1, -2, -4


def _double_autograd(fn, a, x, gout, v):
    """(d_gout, d_x): the gradients of <grad_x <gout, fn(a, x)>, v> by gout and by x, all in float64"""
    x, gout = x.double().requires_grad_(), gout.double().requires_grad_()
    g, = torch.autograd.grad(fn(a.double(), x), x, gout, create_graph=True)
    return torch.autograd.grad((g * v.double()).sum(), (gout, x))


def _hold_voxel(frames, x3, gout, v, ref, keep):
    d_gO, d_x3 = _double_autograd(O.voxel_warp_blend_written_out, frames, x3, gout, v)
    ratios = (R.masked_ratio(d_gO, ref['d_gO'], ref['d_gO_mag'], F64_UNITS, keep),
              R.masked_ratio(d_x3, ref['d_x3'], ref['d_x3_mag'], F64_UNITS, keep))
    assert max(ratios) <= 1.0, ratios
    assert (ref['d_gO'] != 0).float().mean() > 0.3 and (ref['d_x3'] != 0).float().mean() > 0.1        # there is something to compare


def _hold_flow(img, flw, gout, v, ref, keep):
    d_gout, d_flow = _double_autograd(O.flow_warp, img, flw, gout, v)
    ratios = (R.masked_ratio(d_gout, ref['d_gout'], ref['d_gout_mag'], F64_UNITS, keep),
              R.masked_ratio(d_flow, ref['d_flow'], ref['d_flow_mag'], F64_UNITS, keep))
    assert max(ratios) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement against double autograd
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VOXEL_LATTICE)
def test_voxel_restatement_equals_double_autograd_on_the_lattice(shape):
    """every pixel: coordinates on integers, quarter cells and both clip bounds, where the cell and the clip slope are conventions"""
    frames, x3, gout = R.voxel_lattice(*shape)
    v = R2.cotangent(x3)
    ref = R2.voxel2(frames, x3, gout, v)
    _hold_voxel(frames, x3, gout, v, ref, torch.ones(shape, dtype=torch.bool))


@pytest.mark.parametrize("amp", [0.3, 2.0])
@pytest.mark.parametrize("shape", VOXEL_RAGGED)
def test_voxel_restatement_equals_double_autograd_on_ragged_inputs(shape, amp):
    frames, x3, gout = R.voxel_ragged(*shape, amp)
    v = R2.cotangent(x3)
    ref = R2.voxel2(frames, x3, gout, v, coord=np.float64)
    share = ref['near'].float().mean().item()
    assert share <= R.NEAR_CAP, share
    _hold_voxel(frames, x3, gout, v, ref, ~ref['near'])


@pytest.mark.parametrize("shape", FLOW_LATTICE)
def test_flow_restatement_equals_double_autograd_on_the_lattice(shape):
    """every pixel: cells that start at -2, -1, W - 1, W and parked cells included"""
    img, flw, gout = R.flow_lattice(*shape)
    v = R2.cotangent(flw)
    ref = R2.flow2(img, flw, gout, v)
    _hold_flow(img, flw, gout, v, ref, torch.ones(shape[0], shape[2], shape[3], dtype=torch.bool))
    if shape[2] * shape[3] > 1:
        assert (ref['d_gout'] != 0).any() and (ref['d_flow'] != 0).any()


@pytest.mark.parametrize("amp", [1.0, 6.0, 30.0])
@pytest.mark.parametrize("shape", FLOW_RAGGED)
def test_flow_restatement_equals_double_autograd_on_ragged_inputs(shape, amp):
    img, flw, gout = R.flow_ragged(*shape, amp)
    v = R2.cotangent(flw)
    ref = R2.flow2(img, flw, gout, v, coord=np.float64)
    share = ref['near'].float().mean().item()
    assert share <= R.NEAR_CAP, share
    _hold_flow(img, flw, gout, v, ref, ~ref['near'])


def test_flow_restatement_gives_zeros_at_targets_that_are_not_finite_or_far_away():
    img, flw, gout = R.flow_lattice(2, 3, 8, 16)
    v = R2.cotangent(flw)
    clean = R2.flow2(img, flw, gout, v)
    bad = flw.clone()
    spots = [(0, 0, 1, 2), (0, 1, 3, 5), (1, 0, 7, 15), (1, 1, 0, 0), (1, 0, 4, 4)]
    for (n, ch, y, x), value in zip(spots, (float('nan'), float('inf'), float('-inf'), 1e30, -1e30)):
        bad[n, ch, y, x] = value
    ref = R2.flow2(img, bad, gout, v)
    hit = torch.zeros(2, 8, 16, dtype=torch.bool)
    for n, _, y, x in spots:
        hit[n, y, x] = True
    for key in ('d_gout', 'd_gout_mag', 'd_flow', 'd_flow_mag'):
        k = hit.unsqueeze(1).expand_as(ref[key])
        assert (ref[key][k] == 0).all() and torch.equal(ref[key][~k], clean[key][~k]), key


# ------------------------------------------------------------------------------------------------------------------------------------
# the bounds can fail
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_bounds_tell_a_right_closed_cell_from_the_convention():
    """on the lattice a cell (i, i + 1] has other corners wherever a coordinate sits on an integer: other brackets, another X"""
    frames, x3, gout = R.voxel_lattice(2, 5, 9)
    v = R2.cotangent(x3)
    ref, wrong = R2.voxel2(frames, x3, gout, v), R2.voxel2(frames, x3, gout, v, right_closed=True)
    assert R.bound_ratio(wrong['d_gO'], ref['d_gO'], ref['d_gO_mag'], R2.VOXEL_DGO_UNITS) > 100
    assert R.bound_ratio(wrong['d_x3'][:, :2], ref['d_x3'][:, :2], ref['d_x3_mag'][:, :2], R2.VOXEL_DFLOW_UNITS) > 100
    assert R.bound_ratio(wrong['d_x3'][:, 2:], ref['d_x3'][:, 2:], ref['d_x3_mag'][:, 2:], R2.VOXEL_DMASK_UNITS) > 100
    img, flw, gout = R.flow_lattice(2, 3, 8, 16)
    v = R2.cotangent(flw)
    ref, wrong = R2.flow2(img, flw, gout, v), R2.flow2(img, flw, gout, v, right_closed=True)
    assert R.bound_ratio(wrong['d_gout'], ref['d_gout'], ref['d_gout_mag'], R2.FLOW_DGOUT_UNITS) > 100
    assert R.bound_ratio(wrong['d_flow'], ref['d_flow'], ref['d_flow_mag'], R2.flow_dflow_units(3)) > 100


def test_the_bounds_tell_a_slope_dropped_from_the_mixed_difference():
    """X carries the slopes of BOTH coordinates of its tap.  Without the clip slope -- (size - 1) / 2 kept where the coordinate is
    clipped, the derivative of a bare clamp taken twice -- H01 is far outside its bound on the lattice, where both clip bounds are hit.
    The other slope, the one that says the upper corner exists, is implied: a dropped upper corner IS the lower corner (i1 == i0, the
    same texel), so both differences of X vanish there and a restatement without that factor is the same numbers bit for bit.  (It
    stays in the formula, as in the first-order brackets: it is what makes the expression right for any way of filling a dropped corner.)"""
    frames, x3, gout = R.voxel_lattice(2, 5, 9)
    v = R2.cotangent(x3)
    ref = R2.voxel2(frames, x3, gout, v)
    wrong = R2.voxel2(frames, x3, gout, v, clip_slope_in_x=False)
    assert torch.equal(wrong['d_gO'], ref['d_gO']) and torch.equal(wrong['d_x3'][:, 2:], ref['d_x3'][:, 2:])      # no X in these
    assert R.bound_ratio(wrong['d_x3'][:, :2], ref['d_x3'][:, :2], ref['d_x3_mag'][:, :2], R2.VOXEL_DFLOW_UNITS) > 100
    same = R2.voxel2(frames, x3, gout, v, corner_slope_in_x=False)
    assert torch.equal(same['d_x3'], ref['d_x3']) and torch.equal(same['d_x3_mag'], ref['d_x3_mag'])
    s = R.voxel_coords(x3)
    assert any((a >= a.dtype.type(n - 1)).any() for a, n in zip(s, (9, 5, 9, 5)))                # upper corners were dropped


def test_the_bounds_tell_float64_coordinates_from_float32_ones():
    frames, x3, gout = R.voxel_ragged(1, 3, 300, 0.3)
    v = R2.cotangent(x3)
    ref, wrong = R2.voxel2(frames, x3, gout, v), R2.voxel2(frames, x3, gout, v, coord=np.float64)
    assert R.masked_ratio(wrong['d_gO'], ref['d_gO'], ref['d_gO_mag'], R2.VOXEL_DGO_UNITS, ~ref['near']) > 4
    img, flw, gout = R.flow_ragged(2, 5, 3, 300, 6.0)
    v = R2.cotangent(flw)
    ref, wrong = R2.flow2(img, flw, gout, v), R2.flow2(img, flw, gout, v, coord=np.float64)
    assert R.masked_ratio(wrong['d_gout'], ref['d_gout'], ref['d_gout_mag'], R2.FLOW_DGOUT_UNITS, ~ref['near']) > 4


def test_cotangent_is_seeded():
    a, b = R2.cotangent(torch.empty(2, 3, 5, 9)), R2.cotangent(torch.empty(2, 3, 5, 9))
    assert torch.equal(a, b) and a.shape == (2, 3, 5, 9) and not torch.equal(a, R2.cotangent(torch.empty(2, 3, 5, 9), seed=1))


# ------------------------------------------------------------------------------------------------------------------------------------
# the flag
# ------------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults_to_zero():
    parser = config.build_parser()
    assert parser.parse_args([]).warp_second_order == 0
    assert parser.parse_args(['--warp_second_order', '1']).warp_second_order == 1
    with pytest.raises(SystemExit):
        parser.parse_args(['--warp_second_order', '2'])
    assert default_args().warp_second_order == 0
    assert default_args(warp_second_order=1).warp_second_order == 1
    assert 'warp_second_order' in config.__doc__


def test_switch_is_per_thread_and_off_by_default():
    import threading
    from meta_interpolation_amd import hip_ops
    assert hip_ops.warp_second_order() is False
    hip_ops.set_warp_second_order(True)
    try:
        seen = []
        th = threading.Thread(target=lambda: seen.append(hip_ops.warp_second_order()))
        th.start()
        th.join()
        assert seen == [False] and hip_ops.warp_second_order() is True
    finally:
        hip_ops.set_warp_second_order(False)


# ------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device: every call below returns before a launch, the "device pointers" are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------------------
NAMES = ("savfi_voxelwarp_bwd2_f32", "savfi_flowwarp_bwd2_f32")
PTRS = tuple(0x10000 * (k + 1) for k in range(6))


def test_library_exports_both_symbols_under_abi_24():
    lib = _hip.lib()
    assert lib.savfi_version() == 24 and _hip.ABI_VERSION == 24
    dyn = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    with open(_hip.HEADER_PATH) as fh:
        text = fh.read()
    comment = text[:text.index("#define SAVFI_ABI_VERSION 24")].rsplit("/*", 1)[1]
    assert "Added under 24" in comment
    for name, nargs in zip(NAMES, (10, 11)):
        assert name in _hip.declared_symbols() and name in _hip._PROTOTYPES and len(_hip._PROTOTYPES[name]) == nargs
        assert getattr(lib, name) is not None and name in exported
        assert re.search(r"\b%s\b" % name, comment)


def test_null_and_shape_errors_are_returned_before_any_launch():
    vb2, fb2 = _hip.lib().savfi_voxelwarp_bwd2_f32, _hip.lib().savfi_flowwarp_bwd2_f32
    for k in range(4):                                                              # frames / img, x3 / flow, gO / gout, v
        args = [None if i == k else p for i, p in enumerate(PTRS)]
        assert vb2(*args, 1, 2, 2, None) == E_NULL and fb2(*args, 1, 1, 2, 2, None) == E_NULL, k
    assert vb2(*PTRS[:4], None, None, 1, 2, 2, None) == E_NULL and fb2(*PTRS[:4], None, None, 1, 1, 2, 2, None) == E_NULL
    for outs in ((PTRS[4], None), (None, PTRS[5]), (PTRS[4], PTRS[5])):             # one null output is fine: the shape is looked at
        for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2), (1, -3, 2), (1, 2, -3), (1, 65536, 1), (65536, 1, 1)):
            assert vb2(*PTRS[:4], *outs, *dims, None) == E_SHAPE, dims
        for dims in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 0, 2), (1, 1, 2, 0), (-1, 1, 2, 2), (1, -1, 2, 2), (1, 1, -2, 2), (1, 1, 2, -2)):
            assert fb2(*PTRS[:4], *outs, *dims, None) == E_SHAPE, dims
        for dims in ((65536, 1, 1, 1), (1, 1, 4 * 65535 + 1, 1), (1, 1 << 10, 1 << 15, 1 << 15)):
            assert fb2(*PTRS[:4], *outs, *dims, None) == E_TOOBIG, dims
            assert _hip.lib().savfi_flowwarp_bwd_f32(*PTRS[:4], *dims, None) == E_TOOBIG, dims       # the first-order entry's limits
    assert vb2(None, *PTRS[1:], 0, 2, 2, None) == E_NULL and fb2(*PTRS[:3], None, *PTRS[4:], 0, 1, 2, 2, None) == E_NULL   # NULL first


# ------------------------------------------------------------------------------------------------------------------------------------
# the system comparisons of tests/test_warp2_system_gpu.py are well conditioned
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["rrin", "superslomo"])
def test_the_oracle_in_float32_and_in_float64_agree_within_a_quarter_of_the_gate(model):
    """the second-order meta-iteration the device is compared with, on the weights of tests/warp2_system.py (flow heads scaled): the
    oracle's float32 run against its float64 run, loss and every outer-gradient fingerprint inside a quarter of the gate"""
    from tests import warp2_system as S
    from tests.helpers import assert_fp_close
    loss32, fp32 = S.oracle_run(model, torch.float32)
    loss64, fp64 = S.oracle_run(model, torch.float64)
    assert abs(loss32 - loss64) <= 0.25 * S.LOSS_GATE * abs(loss64)
    assert set(fp32) == set(fp64) and len(fp64) >= 90
    worst = 0.0
    for name, want in fp64.items():
        assert_fp_close(fp32[name], want, 0.25 * S.FP_GATE, ('float32 against float64', model, name))
        worst = max(worst, max(abs(fp32[name][k] - want[k]) for k in (0, 1)) / max(abs(want[1]), 1e-12))
    print("%s: float32 against float64, loss %.1e, fingerprints at most %.1e of the abs-sum" % (model, abs(loss32 - loss64) / abs(loss64), worst))
    # the flow heads carry a gradient: the flows are not scaled away
    for head in S.FLOW_HEADS[model]:
        assert fp64[head + '.weight'][1] > 0
