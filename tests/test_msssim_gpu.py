"""-m gpu: the multi-scale SSIM kernels (csrc/ssim.hip) through the C ABI and through hip_ops, against the float64 restatement of
tests/msssim_ref.py.

Gate.  The convention of tests/test_ssim_gpu.py: tools/gen_golden_msssim.py measured, for every stored case, ``e_ref`` =
|reference fp32 - float64| (value: absolute; gradient: max |diff| / max |float64 gradient|) and ``E_kind`` = the largest finite
``e_ref`` of a content kind and ``normalize`` setting over all sizes, classes and seeds 0..2.  The kernel must satisfy
``e_kernel <= max(3 E_kind, floor)``; floor = 4 ulp of a value of order 1 (2.4e-7) resp. 2^-20 of the gradient's maximum.

MEASURED (MI355X; worst e_kernel per kind over the single-sample and row cases of this file, against the gate; every line of that
run is in profiles/msssim_parity.txt):
  kind    normalize  value error  gate       gradient error  gate
  noise   1          5.47e-06     4.40e-05   3.64e-05        6.86e-04
  smooth  1          9.79e-07     3.79e-06   6.06e-06        5.43e-05
  near    1          8.00e-07     6.14e-06   8.94e-05        5.63e-04
  near    0          1.60e-06     1.27e-05   8.91e-05        5.70e-04
Error over gate, in table order: value 0.12, 0.26, 0.13, 0.13 (worst: `smooth` at 176 x 176, whose last level is a single position
per channel); gradient 0.05, 0.11, 0.16, 0.16.  The two pairs whose class changes between levels are held to their own e_ref:
value error 6.3e-07 .. 1.9e-06 against gates 3.9e-06 .. 8.8e-06, gradient error 3.4e-05 .. 5.1e-05 against 9.9e-05 .. 1.5e-04
(up to 0.37 of the gate).  Identical pairs: value exactly 1 and gradient exactly 0 in every run.  Metric on quantised `near` frames:
8.3e-08 .. 7.6e-07 (gate 1.27e-05).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops
from tests import msssim_ref as M
from tests import ssim_ref as R
from tests.helpers import golden
from tests.test_ssim_gpu import offset_copy

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = golden("msssim")
VALUE_FLOOR, GRAD_FLOOR, K = 4 * 2.0 ** -24, 2.0 ** -20, 3.0
SIZES = [(32, 32), (37, 53), (64, 64), (161, 176), (176, 176), (40, 300)]
HEAD, LEVELS = 16, 5
# (kind, normalize): (worst value error, value gate, worst gradient error, gradient gate) as printed by the run in profiles/msssim_parity.txt
MEASURED = {('noise', 1): (5.466e-06, 4.398e-05, 3.637e-05, 6.862e-04), ('smooth', 1): (9.788e-07, 3.787e-06, 6.061e-06, 5.430e-05),
            ('near', 1): (8.000e-07, 6.140e-06, 8.943e-05, 5.629e-04), ('near', 0): (1.596e-06, 1.271e-05, 8.906e-05, 5.696e-04)}
MIN_BASE = 0.05          # every base that enters the product: away from the singular derivative of the power
FIXED = _hip.SSIM_RANGE_FIXED


def gates(kind, norm, e_ref=None):
    e_v, e_g = GOLD['E_%s_z%d' % (kind, norm)] if e_ref is None else e_ref
    return max(K * float(e_v), VALUE_FLOOR), max(K * float(e_g), GRAD_FLOOR)


def tightest_gates(norm):
    """For content of none of the fixture's kinds (a network's prediction): the smallest gate any kind gives."""
    return tuple(min(gates(kind, norm)[i] for kind in R.KINDS) for i in (0, 1))


def up4(n):
    return (n + 3) & ~3


def run_abi(sr, hr, mode, normalize, g=None, off=(0, 0), quantize=False, backward=True):
    """The entry points on raw pointers, results into NaN-filled buffers.
    -> (value [rows or 1] cpu, classes [rows][5], gradient cpu or None, the scratch as the forward left it)"""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    rows = 1 if mode == _hip.SSIM_RANGE_BATCH else N
    res = torch.full((rows,), float('nan'), device=DEV)
    nbytes = int(lib.savfi_msssim_scratch_bytes(N, C, H, W))
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.full((nbytes // 4,), float('nan'), device=DEV)
    assert scratch.data_ptr() % 16 == 0
    _hip.check(lib.savfi_msssim_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), scratch.data_ptr(), N, C, H, W, mode, int(normalize),
                                    int(quantize), st), "savfi_msssim_f32")
    fwd_scratch = scratch.clone()
    classes = scratch[:rows * HEAD].view(torch.int32).view(rows, HEAD)[:, 2 * LEVELS:3 * LEVELS].cpu().tolist()
    grad = None
    if backward:
        go = torch.ones(rows, device=DEV) if g is None else torch.as_tensor(g, dtype=torch.float32).to(DEV)
        grad = torch.full(sr.shape, float('nan'), device=DEV)
        _hip.check(lib.savfi_msssim_bwd_f32(srd.data_ptr(), hrd.data_ptr(), go.data_ptr(), scratch.data_ptr(), grad.data_ptr(), N, C, H, W,
                                            mode, st), "savfi_msssim_bwd_f32")
        grad = grad.cpu()
    torch.cuda.synchronize()
    return res.cpu(), classes, grad, fwd_scratch


def check(kind, norm, what, value, grad, value64, grad64, e_ref=None):
    """Print the figures, then hold them to the gate."""
    g_v, g_g = gates(kind, norm, e_ref)
    e_v = float((value.double() - value64).abs().max())
    e_g = float((grad.double() - grad64).abs().max() / grad64.abs().max())
    print('MSSSIM_PARITY kind=%s normalize=%d case=%s e_value=%.3e gate=%.3e e_grad=%.3e gate=%.3e' % (kind, norm, what, e_v, g_v, e_g, g_g))
    assert torch.isfinite(grad).all()
    assert e_v <= g_v, (what, e_v, g_v)
    assert e_g <= g_g, (what, e_g, g_g)


def bases_ok(sr, hr, norm, val_range=None):
    ms, mc, classes = M.levels(sr.double(), hr.double(), val_range)
    return float(M.bases(ms, mc, norm).min()) >= MIN_BASE, classes


@pytest.mark.parametrize("size", SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_sample_matches_float64_in_every_range_class(kind, size):
    H, W = size
    for norm in ((True, False) if kind == 'near' else (True,)):
        for cls in range(4):
            sr, hr = R.make_pair(kind, cls, 1, 3, H, W, 0)
            ok, classes = bases_ok(sr, hr, norm)
            assert ok
            value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), None, norm)
            name = M.case_name(kind, cls, norm, 1, H, W, 0)
            assert abs(float(value64) - float(GOLD[name + '/value64'])) <= 1e-12          # the inputs are the ones the reference saw
            for mode in (_hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH):
                value, words, grad, scratch = run_abi(sr, hr, mode, norm)
                assert words == [classes]
                check(kind, norm, '%s mode%d' % (name, mode), value, grad, value64.reshape(1), grad64)
            # the reference's fp32 value is as far away as its own error plus ours allows
            assert abs(float(value) - float(GOLD[name + '/value'])) <= gates(kind, norm)[0] + float(GOLD[name + '/e_ref'][0])
        # the pooled pair of the first two levels, where the scratch keeps them: avg_pool2d's bits
        at = up4(HEAD)
        x, y = sr.to(DEV), hr.to(DEV)
        for s in (1, 2):
            x, y = F.avg_pool2d(x, (2, 2)), F.avg_pool2d(y, (2, 2))
            n = x.numel()
            assert torch.equal(scratch[at:at + n].view(x.shape), x) and torch.equal(scratch[at + up4(n):at + up4(n) + n].view(y.shape), y)
            at += 3 * up4(n)


@pytest.mark.parametrize("size", [(37, 53), (64, 64)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("kind,norm", [('near', True), ('near', False), ('noise', True)])
def test_rows_per_row_and_whole_batch_with_unequal_cotangents(kind, norm, size):
    H, W = size
    g = [0.25, 0.75, 1.25]
    for cl in (0, [0, 2, 1]):          # a batch whose rows fall in different range classes
        sr, hr = R.make_pair(kind, cl, 3, 3, H, W, 1)
        assert bases_ok(sr, hr, norm)[0] and all(bases_ok(sr[i:i + 1], hr[i:i + 1], norm)[0] for i in range(3))
        # per row: what three calls on the N = 1 slices give, bit for bit
        value, words, grad, _ = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, norm, g)
        for i in range(3):
            v1, w1, g1, _ = run_abi(sr[i:i + 1], hr[i:i + 1], _hip.SSIM_RANGE_PER_ROW, norm, g[i:i + 1])
            assert torch.equal(v1, value[i:i + 1]) and torch.equal(g1, grad[i:i + 1]) and w1 == words[i:i + 1]
            assert w1[0] == M.levels(sr[i:i + 1].double(), hr[i:i + 1].double())[2]
        check(kind, norm, 'rows %dx%d classes %s' % (H, W, cl), value, grad, M.msssim_rows(sr.double(), hr.double(), None, norm),
              M.msssim_grad_rows(sr.double(), hr.double(), g, None, norm))
        # whole batch: one call on the N = 3 tensor, the rule and the means over everything
        value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), None, norm, 1.75)
        value, words, grad, _ = run_abi(sr, hr, _hip.SSIM_RANGE_BATCH, norm, [1.75])
        assert words == [M.levels(sr.double(), hr.double())[2]]
        check(kind, norm, 'batch %dx%d classes %s' % (H, W, cl), value, grad, value64.reshape(1), grad64)
    # a fixed class ignores the data: class-0 data under L = 2 and L = 255 on every level
    sr, hr = R.make_pair(kind, 0, 3, 3, H, W, 1)
    for k, L in ((1, 2), (2, 255)):
        assert all(bases_ok(sr[i:i + 1], hr[i:i + 1], norm, L)[0] for i in range(3))
        value, words, grad, _ = run_abi(sr, hr, FIXED + k, norm, g)
        assert words == [[k] * 5] * 3
        check(kind, norm, 'fixed%d %dx%d' % (k, H, W), value, grad, M.msssim_rows(sr.double(), hr.double(), L, norm),
              M.msssim_grad_rows(sr.double(), hr.double(), g, L, norm))


@pytest.mark.parametrize("tag,spike,classes", [('spike200', 200.0, [2, 0, 0, 0, 0]), ('spikem06', -0.6, [1, 0, 0, 0, 0])])
def test_the_range_class_changes_between_levels(tag, spike, classes):
    sr, hr = R.make_pair('near', 0, 1, 3, 64, 64, 0)
    sr = sr.clone()
    sr[0, 1, 20, 30] = spike          # one element: the pooled value (about spike / 4) is back in class 0
    for norm in (True, False):
        name = '%s_z%d' % (tag, norm)
        assert GOLD[name + '/classes'].tolist() == classes
        ok, cls64 = bases_ok(sr, hr, norm)
        assert ok and cls64 == classes
        value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), None, norm)
        assert abs(float(value64) - float(GOLD[name + '/value64'])) <= 1e-12
        for mode in (_hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH):
            value, words, grad, _ = run_abi(sr, hr, mode, norm)
            assert words == [classes]          # what the forward stored
            check('near', norm, '%s mode%d' % (name, mode), value, grad, value64.reshape(1), grad64, e_ref=GOLD[name + '/e_ref'])


def test_negative_base_gives_nan_like_the_reference():
    sr, hr = R.make_pair('noise', 0, 1, 3, 32, 32, 1)          # seed 1: the reference's value is NaN (seed 0 happens to stay positive)
    name = M.case_name('noise', 0, False, 1, 32, 32, 1)
    value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), None, False)
    assert torch.isnan(value64) and torch.isnan(grad64).all() and np.isnan(GOLD[name + '/value'])
    value, _, grad, _ = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, False)
    assert torch.isnan(value).all() and torch.isnan(grad).all()
    value, _, grad, _ = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, True)
    assert torch.isfinite(value).all() and torch.isfinite(grad).all()
    # in a batch of rows only the row with the negative base is NaN
    sr2, hr2 = R.make_pair('near', 0, 1, 3, 32, 32, 0)
    value, _, grad, _ = run_abi(torch.cat([sr, sr2]), torch.cat([hr, hr2]), _hip.SSIM_RANGE_PER_ROW, False, [1.0, 1.0])
    assert torch.isnan(value[0]) and torch.isnan(grad[0]).all() and torch.isfinite(value[1]) and torch.isfinite(grad[1]).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: '%dx%d' % s)
def test_identical_pair_is_exactly_one(size):
    H, W = size
    for cls in (0, 1):
        sr, hr = R.make_pair('same', cls, 1, 3, H, W, 0)
        for norm in (True, False):
            name = M.case_name('same', cls, norm, 1, H, W, 0)
            assert float(GOLD[name + '/value']) == 1.0
            for mode in (_hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH):
                value, _, grad, _ = run_abi(sr, hr, mode, norm)
                assert value.tolist() == [1.0]
                worst = float(grad.abs().max())
                print('MSSSIM_SAME case=%s mode%d max|grad|=%.3e reference %.3e' % (name, mode, worst, float(GOLD[name + '/grad_maxabs'])))
                assert worst <= 3 * float(GOLD[name + '/grad_maxabs'])


def test_alignment_and_reproducibility():
    for H, W in ((37, 53), (64, 64), (40, 300)):
        sr, hr = R.make_pair('near', [0, 1], 2, 3, H, W, 2)
        base = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, True, [0.5, 1.5])
        for off in ((0, 0), (1, 0), (0, 2), (1, 2), (2, 1)):          # operands 4 and 8 bytes off a 16-byte boundary
            again = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, True, [0.5, 1.5], off=off)
            assert torch.equal(again[0], base[0]) and torch.equal(again[2], base[2]) and again[1] == base[1]


def test_one_capture_replays_the_eager_result():
    """Forward and backward in ONE capture on a single stream; the replay after the inputs were refilled in place equals the eager
    result of the new inputs bit for bit (no host read, no cleared memory, nothing left from the capture's data)."""
    first = R.make_pair('near', [0, 1], 2, 3, 37, 53, 0)
    second = R.make_pair('near', [2, 0], 2, 3, 37, 53, 1)
    go = torch.tensor([0.5, 1.5], device=DEV)

    def eager(pair):
        x = pair[0].to(DEV).requires_grad_()
        v = hip_ops.msssim_per_sample(x, pair[1].to(DEV), normalize=True)
        gx, = torch.autograd.grad(v, x, go)
        return v.detach().clone(), gx.clone()
    want1, want2 = eager(first), eager(second)
    x = first[0].to(DEV).requires_grad_()
    y = first[1].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(hip_ops.msssim_per_sample(x, y, normalize=True), x, go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = hip_ops.msssim_per_sample(x, y, normalize=True)
        gx, = torch.autograd.grad(v, x, go)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(v.detach(), want1[0]) and torch.equal(gx, want1[1])
    with torch.no_grad():
        x.copy_(second[0])
        y.copy_(second[1])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(v.detach(), want2[0]) and torch.equal(gx, want2[1])
    assert not torch.equal(want1[0], want2[0])


def test_hip_ops_autograd_and_the_composed_form():
    sr, hr = R.make_pair('near', [0, 2, 1], 3, 3, 37, 53, 1)
    g = torch.tensor([0.25, 0.75, 1.25])
    for norm in (True, False):
        # one value over the batch
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.msssim(x, hr.to(DEV), normalize=norm)
        assert v.shape == ()
        gx, = torch.autograd.grad(2.0 * v, x)
        value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), None, norm, 2.0)
        check('near', norm, 'hip_ops.msssim', v.detach().cpu().reshape(1), gx.cpu(), value64.reshape(1), grad64)
        # every sample on its own
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.msssim_per_sample(x, hr.to(DEV), normalize=norm)
        assert v.shape == (3,)
        gx, = torch.autograd.grad(v, x, g.to(DEV))
        rows64 = M.msssim_rows(sr.double(), hr.double(), None, norm)
        grows64 = M.msssim_grad_rows(sr.double(), hr.double(), g.tolist(), None, norm)
        check('near', norm, 'hip_ops.msssim_per_sample', v.detach().cpu(), gx.cpu(), rows64, grows64)
        # a given range: one value under L = 2 on every level
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.msssim(x, hr.to(DEV), val_range=2, normalize=norm)
        gx, = torch.autograd.grad(v, x)
        value64, grad64 = M.msssim_and_grad(sr.double(), hr.double(), 2, norm)
        check('near', norm, 'hip_ops.msssim val_range=2', v.detach().cpu().reshape(1), gx.cpu(), value64.reshape(1), grad64)
        # the composed form of --second_order: the same numbers within the gate, and differentiable twice
        hip_ops.set_double_backward(True)
        try:
            x = sr.to(DEV).requires_grad_()
            v = hip_ops.msssim_per_sample(x, hr.to(DEV), normalize=norm)
            gx, = torch.autograd.grad(v, x, g.to(DEV), create_graph=True)
            check('near', norm, 'composed per_sample', v.detach().cpu(), gx.detach().cpu(), rows64, grows64)
            assert gx.requires_grad
            ggx, = torch.autograd.grad(gx.pow(2).sum(), x)
            assert torch.isfinite(ggx).all() and float(ggx.abs().max()) > 0
            v = hip_ops.msssim(x, hr.to(DEV), normalize=norm)
            value64, _ = M.msssim_and_grad(sr.double(), hr.double(), None, norm)
            assert abs(float(v) - float(value64)) <= gates('near', norm)[0]
        finally:
            hip_ops.set_double_backward(False)
    with pytest.raises(NotImplementedError):
        hip_ops.msssim(sr.to(DEV), hr.to(DEV).requires_grad_())


def test_metric_is_the_plain_definition_on_quantised_frames():
    for H, W in ((37, 53), (64, 64), (161, 176)):
        # frames of kind `near` in unit range, which the metric quantises into class 2: E_near without `normalize` is their yardstick
        pred, tgt = R.make_pair('near', 0, 3, 3, H, W, 4)
        # row 2 is equal after quantisation: the target on the grid, the prediction less than half a step away
        tgt[2] = (tgt[2] * 255).round() / 255
        pred[2] = tgt[2] + 0.4 / 255
        want = M.metric_rows(pred, tgt)
        got = hip_ops.msssim_metric(pred.to(DEV), tgt.to(DEV)).cpu()
        assert torch.equal(M.quantize(pred[2]), M.quantize(tgt[2])) and float(got[2]) == 1.0
        e = float((got.double() - want).abs().max())
        print('MSSSIM_METRIC %dx%d values %s e=%.3e gate=%.3e' % (H, W, got.tolist(), e, gates('near', 0)[0]))
        assert torch.isfinite(want).all() and e <= gates('near', 0)[0]
    # NaN is reported as NaN: a frame against its negative has negative contrast means
    a, _ = R.make_pair('noise', 0, 1, 3, 32, 32, 0)
    b = 1 - a
    assert torch.isnan(M.metric_rows(a, b)).all() and torch.isnan(hip_ops.msssim_metric(a.to(DEV), b.to(DEV))).all()
