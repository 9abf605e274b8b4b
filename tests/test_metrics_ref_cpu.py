"""CPU (-m "not gpu"): the yardstick of the PSNR / SSIM metric tests is itself pinned.  tests/metrics_ref.py (float64) against the
values tools/gen_golden_metrics.py stored from the reference's ``utils.calc_metrics``; and the host side of the feature that needs no
launch: the symbols, the path selection for tensors the kernel does not take.

PSNR bound: the reference's mse is an fp32 mean (pairwise sums, relative error of a few 2^-24) plus an fp32 ``+ 1e-8``; 16 ulp
relative = 9.5e-7 is 4.1e-6 dB (d PSNR = 4.34 d mse / mse).  The restatement's S is exact, so PSNR_TOL = 1e-5 dB.
"""
import math

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops, utils
from tests import metrics_ref as M
from tests.helpers import golden

GOLD = golden("metrics")
PSNR_TOL = 1e-5

SMALL = [(kind, C, H, W, seed) for kind in M.KINDS + ('same',) for C in (1, 3) for H, W in M.TILE_SIZES for seed in M.SEEDS]
LARGE = [(kind, 3, 256, 448, 0) for kind in M.KINDS] + [('near', 3, 720, 1280, 0)]


def _check(kind, C, H, W, seed):
    name = M.case_name(kind, C, H, W, seed)
    _, _, S, mse64, ssim64 = M.case(kind, 1, C, H, W, seed)
    assert S[0] == int(GOLD[name + '/S'])                                      # the inputs are the ones the reference saw
    assert abs(ssim64[0] - float(GOLD[name + '/ssim64'])) <= 1e-12
    e_ref = abs(float(GOLD[name + '/ssim']) - ssim64[0])
    assert abs(e_ref - float(GOLD[name + '/e_ref'])) <= 1e-12
    if kind == 'same':
        assert S[0] == 0 and ssim64[0] == 1.0 and float(GOLD[name + '/ssim']) == 1.0
    else:
        assert e_ref <= float(GOLD['E_' + kind])
    assert abs(M.psnr(mse64[0]) - float(GOLD[name + '/psnr'])) <= PSNR_TOL + 2.0 ** -24 * abs(float(GOLD[name + "/psnr"]))      # + the fp32 store


def test_restatement_matches_the_reference_at_the_tile_boundary_sizes():
    for c in SMALL:
        _check(*c)


@pytest.mark.parametrize("case", LARGE, ids=lambda c: M.case_name(*c))
def test_restatement_matches_the_reference_at_full_size(case):
    _check(*case)


def test_the_yardstick_is_the_largest_reference_error_of_its_kind():
    names = GOLD['names'].tolist()
    for kind in M.KINDS:
        worst = max(float(GOLD[n + '/e_ref']) for n in names if n.startswith(kind + '_'))
        assert worst == float(GOLD['E_' + kind]) and 0 < worst < 1e-4
    assert sorted(GOLD['kinds'].tolist()) == sorted(M.KINDS) and GOLD['seeds'].tolist() == list(M.SEEDS)


def test_quantisation_inputs_exercise_ties_and_both_clamps():
    pred, tgt = M.make_pair('ties', 1, 3, 37, 53, 0)
    v = (pred * 255).double()              # the fp32 product, as quantize forms it
    assert float(((v - v.floor()) == 0.5).double().mean()) > 0.2             # exact ties in fp32 ...
    q = M.quantize(pred)
    assert bool(((q % 2 == 0) | ((pred * 255 - (pred * 255).floor()) != 0.5)).all())      # ... go to even
    pred, tgt = M.make_pair('wide', 1, 3, 37, 53, 0)
    assert float(pred.min()) == -math.inf and float(pred.max()) == math.inf
    finite = pred[torch.isfinite(pred)]
    assert float(finite.min()) < -0.1 and float(finite.max()) > 1.1
    q = M.quantize(pred)
    assert float(q.min()) == 0 and float(q.max()) == 255


def test_nan_rows_are_nan_in_the_restatement_only_where_they_are():
    pred, tgt = M.make_pair('near', 3, 1, 24, 40, 0)
    pred = pred.clone()
    pred[1, 0, 20, 33] = float('nan')
    S, mse, ssim = M.metric_rows(pred, tgt)
    assert S[1] is None and math.isnan(mse[1]) and math.isnan(ssim[1])
    assert all(np.isfinite([mse[0], mse[2], ssim[0], ssim[2]]))
    assert math.isnan(float(utils.quantize(pred, 1.)[1, 0, 20, 33]))          # torch.clamp lets the NaN through


def test_library_declares_the_metric_and_the_writer():
    declared = _hip.declared_symbols()
    for name in ("savfi_psnr_ssim_scratch_bytes", "savfi_psnr_ssim_f32", "savfi_frames_f32_to_u8"):
        assert name in declared and hasattr(_hip.lib(), name)
    lib = _hip.lib()
    assert lib.savfi_psnr_ssim_scratch_bytes(1, 3, 10, 16) == -2 and lib.savfi_psnr_ssim_scratch_bytes(1, 3, 16, 10) == -2
    assert lib.savfi_psnr_ssim_scratch_bytes(30000, 3, 16, 16) == -4
    # 8 bytes per workgroup; 256 x 448: 16 x 7 tiles of 16 x 64 SSIM positions
    assert lib.savfi_psnr_ssim_scratch_bytes(1, 3, 11, 11) == 3 * 8
    assert lib.savfi_psnr_ssim_scratch_bytes(4, 3, 256, 448) == 4 * 3 * 16 * 7 * 8


def test_host_tensors_and_short_images_take_the_composition():
    """The selection is made from the tensors: CPU tensors (and images shorter than the window) get utils' composition, row by row."""
    pred, tgt = M.make_pair('near', 3, 3, 24, 40, 0)
    mse, ssim = utils.psnr_ssim_rows(pred, tgt)
    assert mse.shape == (3,) and ssim.shape == (3,)
    for r in range(3):
        q_p, q_t = utils.quantize(pred[r], 1.), utils.quantize(tgt[r], 1.)
        assert float(mse[r]) == float((q_p - q_t).div(255).pow(2).mean())
        psnr, s = utils.calc_metrics(pred[r], tgt[r])
        assert float(ssim[r]) == float(s) and abs(-10 * math.log10(float(mse[r]) + 1e-8) - psnr) <= 1e-5
    mse, ssim = utils.psnr_ssim_rows(pred[:, :, :9, :30], tgt[:, :, :9, :30])          # 9 rows: the window shrinks (utils.ssim)
    assert float(ssim[0]) == float(utils.calc_metrics(pred[0, :, :9, :30], tgt[0, :, :9, :30])[1])
    with pytest.raises(NotImplementedError):
        hip_ops.psnr_ssim(pred, tgt)
    with pytest.raises(NotImplementedError):
        hip_ops.frames_to_u8(pred)
    with pytest.raises(ValueError):
        hip_ops.psnr_ssim(pred[:, :, :9], tgt[:, :, :9])
