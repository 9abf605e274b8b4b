"""-m gpu: the bits of the SSIM family (csrc/ssim.hip: SSIM loss, PSNR / SSIM metric, multi-scale SSIM) through the C ABI.

A.  The three users run the same tile arithmetic.  On one image pair the per-workgroup SSIM partial sums and the published range class
    of savfi_ssim_loss_f32 equal those of level 0 of savfi_msssim_f32, and the partial sums of savfi_psnr_ssim_f32 equal those of
    savfi_msssim_f32(quantize=1, FIXED + 2), bit for bit.  That is what lets the kernels share one forward tile.

B.  Every output byte is the one recorded in tests/golden/ssim_family_bits.json: result, class words, gradient and the whole scratch as
    the forward (and, for multi-scale SSIM, the backward) left it in a NaN-filled buffer, as sha256.  The fixture was recorded ONCE, by
    `python -m tests.test_ssim_family_bits_gpu --record` on an MI355X, with this module placed on the tree and the library of the
    commit before the kernels were merged into one tile (where msssim_level restated fwd_tile and msssim_bwd_level restated ssim_bwd).
    It is not regenerated from the code under test.  A case whose input hash differs fails ("inputs differ"): the fixture then has to
    be recorded again from that parent, not from the code under test.

Shapes: 11 x 11 (one position), 12 x 75 (one row of positions, two tiles across, W % 4 != 0), 27 x 75 (two tiles down, the second with
one row), 37 x 53 (odd sizes: the floor pooling drops a row and a column), 33 x 140 (2 x 3 forward tiles, W % 4 == 0: the float4 path;
windows of 11, 11, 8, 4, 2 taps down the levels); 32 x 32 is the smallest multi-scale size (windows 11, 11, 8, 4, 2).
"""
import hashlib
import json
import os
import sys

import pytest
import torch

from meta_interpolation_amd import _hip
from tests import ssim_ref as R
from tests.helpers import GOLDEN
from tests.test_ssim_gpu import offset_copy

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(GOLDEN, "ssim_family_bits.json")
PER_ROW, BATCH, FIXED = _hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH, _hip.SSIM_RANGE_FIXED
HEAD, LEVELS, TH, TW, HALO = 16, 5, 16, 64, 10


def up4(n):
    return (n + 3) & ~3


def tiles(H, W):
    """Forward workgroups of one plane at 11 taps: (across, down)."""
    return -(-(W - HALO) // TW), -(-(H - HALO) // TH)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------------
# the entry points on raw pointers, every output into a poisoned buffer
# ------------------------------------------------------------------------------------------------------------------------
def ssim_call(sr, hr, mode, g=None, off=(0, 0)):
    """-> {result, words, scratch (as the forward left it), grad}"""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    rows, ch = (1, N * C) if mode == BATCH else (N, C)
    res = torch.full((rows,), float('nan'), device=DEV)
    word = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.full((int(lib.savfi_ssim_scratch_floats(N, C, H, W)),), float('nan'), device=DEV)
    _hip.check(lib.savfi_ssim_loss_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), word.data_ptr(), scratch.data_ptr(), N, C, H, W,
                                       mode, st), "savfi_ssim_loss_f32")
    gl = torch.ones(rows, device=DEV) if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
    grad = torch.full(sr.shape, float('nan'), device=DEV)
    _hip.check(lib.savfi_ssim_loss_bwd_f32(srd.data_ptr(), hrd.data_ptr(), gl.data_ptr(), word.data_ptr(), grad.data_ptr(), rows, ch, H, W,
                                           st), "savfi_ssim_loss_bwd_f32")
    torch.cuda.synchronize()
    return {'result': res.cpu(), 'words': word.cpu(), 'scratch': scratch.cpu(), 'grad': grad.cpu()}


def metric_call(pred, tgt, off=(0, 0)):
    """-> {result [rows, 2], sq_sum, scratch (32-bit words)}"""
    lib, st = _hip.lib(), _hip.current_stream()
    rows, C, H, W = pred.shape
    p, t = offset_copy(pred, off[0]), offset_copy(tgt, off[1])
    res = torch.full((rows, 2), float('nan'), device=DEV)
    sq = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(lib.savfi_psnr_ssim_scratch_bytes(rows, C, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    scratch = torch.full((nbytes // 4,), float('nan'), device=DEV)
    _hip.check(lib.savfi_psnr_ssim_f32(p.data_ptr(), t.data_ptr(), res.data_ptr(), sq.data_ptr(), scratch.data_ptr(), rows, C, H, W, st),
               "savfi_psnr_ssim_f32")
    torch.cuda.synchronize()
    return {'result': res.cpu(), 'sq_sum': sq.cpu(), 'scratch': scratch.cpu()}


def msssim_call(sr, hr, mode, normalize, quantize=False, g=None, off=(0, 0), backward=True):
    """-> {result, scratch (as the forward left it), and with `backward`: grad, scratch_bwd (the coarser levels' gradients are in it)}"""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    rows = 1 if mode == BATCH else N
    res = torch.full((rows,), float('nan'), device=DEV)
    nbytes = int(lib.savfi_msssim_scratch_bytes(N, C, H, W))
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.full((nbytes // 4,), float('nan'), device=DEV)
    _hip.check(lib.savfi_msssim_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), scratch.data_ptr(), N, C, H, W, mode, int(normalize),
                                    int(quantize), st), "savfi_msssim_f32")
    out = {'result': res, 'scratch': scratch.clone()}
    if backward:
        go = torch.ones(rows, device=DEV) if g is None else torch.tensor(g, dtype=torch.float32, device=DEV)
        grad = torch.full(sr.shape, float('nan'), device=DEV)
        _hip.check(lib.savfi_msssim_bwd_f32(srd.data_ptr(), hrd.data_ptr(), go.data_ptr(), scratch.data_ptr(), grad.data_ptr(), N, C, H, W,
                                            mode, st), "savfi_msssim_bwd_f32")
        out.update(grad=grad, scratch_bwd=scratch)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def msssim_level0(scratch, N, C, H, W, mode):
    """(the SSIM partial sums of level 0, its class word per row) out of a multi-scale scratch, by msssim_plan's layout: the head, the
    pooled pair and the gradient of levels 1 .. 4, then the partial sums level by level."""
    at = up4(N * HEAD)
    for s in range(1, LEVELS):
        at += 3 * up4(N * C * (H >> s) * (W >> s))
    tx, ty = tiles(H, W)
    rows = 1 if mode == BATCH else N
    words = scratch[:rows * HEAD].view(torch.int32).view(rows, HEAD)[:, 2 * LEVELS]
    return scratch[at:at + N * C * tx * ty], words


# ------------------------------------------------------------------------------------------------------------------------
# A. the families agree
# ------------------------------------------------------------------------------------------------------------------------
FAMILY_SIZES = [(37, 53), (33, 140)]


@pytest.mark.parametrize("size", FAMILY_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("mode,classes", [(PER_ROW, [1, 2]), (BATCH, [0, 3]), (FIXED + 0, [0, 0]), (FIXED + 2, [0, 0])],
                         ids=['per_row', 'batch', 'fixed0', 'fixed2'])
def test_ssim_loss_and_msssim_level_0_give_the_same_partial_sums(mode, classes, size):
    H, W = size
    N, C = 2, 3
    sr, hr = R.make_pair('near', classes, N, C, H, W, 3)
    tx, ty = tiles(H, W)
    one = ssim_call(sr, hr, mode)
    many = msssim_call(sr, hr, mode, True, backward=False)
    want = one['scratch'][:N * C * tx * ty]
    got, words = msssim_level0(many['scratch'], N, C, H, W, mode)
    assert torch.isfinite(want).all()
    differ = (want.view(torch.int32) != got.view(torch.int32)).nonzero().flatten().tolist()
    assert not differ, "workgroups %s: ssim_fwd %s, msssim_level %s" % (differ, want[differ].tolist(), got[differ].tolist())
    assert torch.equal(want, got)
    assert one['words'].tolist() == words.tolist()
    if mode >= FIXED:
        assert words.tolist() == [mode - FIXED] * N
    elif mode == PER_ROW:
        assert words.tolist() == classes


@pytest.mark.parametrize("size", FAMILY_SIZES, ids=lambda s: '%dx%d' % s)
def test_metric_and_quantised_msssim_level_0_give_the_same_partial_sums(size):
    H, W = size
    N, C = 2, 3
    pred, tgt = R.make_pair('near', 0, N, C, H, W, 4)
    tx, ty = tiles(H, W)
    one = metric_call(pred, tgt)
    many = msssim_call(pred, tgt, FIXED + 2, False, quantize=True, backward=False)
    want = one['scratch'][:N * C * tx * ty]
    got, words = msssim_level0(many['scratch'], N, C, H, W, FIXED + 2)
    assert torch.isfinite(want).all()
    differ = (want.view(torch.int32) != got.view(torch.int32)).nonzero().flatten().tolist()
    assert not differ, "workgroups %s: metric_tile %s, msssim_level %s" % (differ, want[differ].tolist(), got[differ].tolist())
    assert torch.equal(want, got) and words.tolist() == [2] * N


# ------------------------------------------------------------------------------------------------------------------------
# B. the recorded bits
# ------------------------------------------------------------------------------------------------------------------------
def _spiked(sr):
    sr = sr.clone()
    sr[0, sr.shape[1] // 2, 20, 30] = 200.0          # one element: class 2 on level 0, the pooled value (about 50) is back in class 0
    return sr


def _ssim_case(size, mode, classes, g, N=2, C=3, kind='near', off=(0, 0), seed=5):
    def run():
        sr, hr = R.make_pair(kind, classes, N, C, size[0], size[1], seed)
        gt = torch.tensor(g, dtype=torch.float32)
        return sha(sr, hr, gt), ssim_call(sr, hr, mode, g, off)
    return run


def _metric_case(size, rows=2, C=3, off=(0, 0), nan_row=None, seed=6):
    def run():
        pred, tgt = R.make_pair('near', 0, rows, C, size[0], size[1], seed)
        if nan_row is not None:
            pred[nan_row, C - 1, size[0] // 2, size[1] - 1] = float('nan')
        return sha(pred, tgt), metric_call(pred, tgt, off)
    return run


def _msssim_case(size, mode, classes, normalize, g, N=2, C=3, off=(0, 0), quantize=False, spike=False, seed=7):
    def run():
        sr, hr = R.make_pair('near', classes, N, C, size[0], size[1], seed)
        if spike:
            sr = _spiked(sr)
        gt = torch.tensor(g, dtype=torch.float32)
        return sha(sr, hr, gt), msssim_call(sr, hr, mode, normalize, quantize, g, off, backward=not quantize)
    return run


G2 = [0.25, 0.75]
CASES = {
    # SSIM loss + backward: every size per row with unequal cotangents, the four classes spread over them
    "ssim-11x11-rows-c01": _ssim_case((11, 11), PER_ROW, [0, 1], G2),
    "ssim-12x75-rows-c23": _ssim_case((12, 75), PER_ROW, [2, 3], G2),
    "ssim-27x75-rows-c12": _ssim_case((27, 75), PER_ROW, [1, 2], G2),
    "ssim-37x53-rows-c30": _ssim_case((37, 53), PER_ROW, [3, 0], G2),
    "ssim-33x140-rows-c02": _ssim_case((33, 140), PER_ROW, [0, 2], G2),
    "ssim-33x140-rows-noise": _ssim_case((33, 140), PER_ROW, [1, 3], G2, kind='noise'),
    "ssim-11x11-batch": _ssim_case((11, 11), BATCH, [0, 0], [1.75]),
    "ssim-37x53-batch-c01": _ssim_case((37, 53), BATCH, [0, 1], [1.75]),
    "ssim-33x140-batch-c20": _ssim_case((33, 140), BATCH, [2, 0], [1.75]),
    "ssim-12x75-fixed2": _ssim_case((12, 75), FIXED + 2, [0, 0], G2),
    "ssim-33x140-fixed2": _ssim_case((33, 140), FIXED + 2, [0, 0], G2),
    "ssim-27x75-n1c1-c1": _ssim_case((27, 75), PER_ROW, [1], [0.5], N=1, C=1),
    "ssim-33x140-off13": _ssim_case((33, 140), PER_ROW, [0, 2], G2, off=(1, 3)),
    "ssim-37x53-off31": _ssim_case((37, 53), PER_ROW, [3, 0], G2, off=(3, 1)),
    # the metric: rows = 2, sq_sum requested
    "metric-11x11": _metric_case((11, 11)),
    "metric-12x75": _metric_case((12, 75)),
    "metric-27x75": _metric_case((27, 75)),
    "metric-37x53": _metric_case((37, 53)),
    "metric-33x140": _metric_case((33, 140)),
    "metric-37x53-nan-row1": _metric_case((37, 53), nan_row=1),
    "metric-33x140-off13": _metric_case((33, 140), off=(1, 3)),
    # multi-scale SSIM forward + backward
    "msssim-32x32-rows-z1": _msssim_case((32, 32), PER_ROW, [0, 1], True, G2),
    "msssim-32x32-rows-z0": _msssim_case((32, 32), PER_ROW, [2, 3], False, G2),
    "msssim-37x53-rows-z1": _msssim_case((37, 53), PER_ROW, [1, 2], True, G2),
    "msssim-37x53-rows-z0": _msssim_case((37, 53), PER_ROW, [3, 0], False, G2),
    "msssim-33x140-rows-z1": _msssim_case((33, 140), PER_ROW, [0, 2], True, G2),
    "msssim-33x140-rows-z0": _msssim_case((33, 140), PER_ROW, [1, 0], False, G2),
    "msssim-37x53-batch-z1": _msssim_case((37, 53), BATCH, [0, 1], True, [1.75]),
    "msssim-33x140-fixed2-z1": _msssim_case((33, 140), FIXED + 2, [0, 0], True, G2),
    "msssim-32x32-n1c1-z1": _msssim_case((32, 32), PER_ROW, [0], True, [0.5], N=1, C=1),
    "msssim-33x140-n1c1-z0": _msssim_case((33, 140), PER_ROW, [1], False, [0.5], N=1, C=1),
    "msssim-37x53-quant-fixed2": _msssim_case((37, 53), FIXED + 2, [0, 0], False, G2, quantize=True),
    "msssim-33x140-quant-fixed2": _msssim_case((33, 140), FIXED + 2, [0, 0], False, G2, quantize=True),
    "msssim-37x53-spike200-z1": _msssim_case((37, 53), PER_ROW, [0, 0], True, G2, spike=True),
    "msssim-33x140-spike200-batch-z0": _msssim_case((33, 140), BATCH, [0, 0], False, [1.75], spike=True),
    "msssim-33x140-off13": _msssim_case((33, 140), PER_ROW, [0, 2], True, G2, off=(1, 3)),
    "msssim-32x32-off31": _msssim_case((32, 32), PER_ROW, [0, 1], True, G2, off=(3, 1)),
}


def run_case(name):
    inputs, out = CASES[name]()
    return {"inputs": inputs, "outputs": {k: sha(v) for k, v in sorted(out.items())}}


def record(path):
    bits = {name: run_case(name) for name in CASES}
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(bits.items())) + "\n}\n")
    print("%d cases -> %s" % (len(bits), path))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_names_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_are_the_recorded_ones(name, recorded):
    got, want = run_case(name), recorded[name]
    assert got["inputs"] == want["inputs"], "%s: inputs differ, re-record from the parent" % name
    wrong = [k for k in want["outputs"] if got["outputs"].get(k) != want["outputs"][k]]
    assert not wrong and sorted(got["outputs"]) == sorted(want["outputs"]), "%s: %s differ from the recorded bytes" % (name, wrong)


def test_the_spiked_pairs_change_class_between_levels():
    """What the two spike200 cases are there for, asserted: class 2 on level 0, class 0 below."""
    for size, mode in (((37, 53), PER_ROW), ((33, 140), BATCH)):
        sr, hr = R.make_pair('near', [0, 0], 2, 3, size[0], size[1], 7)
        out = msssim_call(_spiked(sr), hr, mode, True, backward=False)
        rows = 1 if mode == BATCH else 2
        words = out['scratch'][:rows * HEAD].view(torch.int32).view(rows, HEAD)[:, 2 * LEVELS:3 * LEVELS].tolist()
        assert words[0] == [2, 0, 0, 0, 0] and words[1:] == [[0] * 5] * (rows - 1)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python -m tests.test_ssim_family_bits_gpu --record [path]")
    record(sys.argv[2] if len(sys.argv) == 3 else FIXTURE)
