"""-m gpu: the fused SSIM loss kernels (csrc/ssim.hip) through the C ABI and through hip_ops, against the float64 restatement
of tests/ssim_ref.py.

Gate.  The yardstick is the reference's own fp32 arithmetic against float64: tools/gen_golden_ssim.py measured, for every
stored case, ``e_ref`` = |reference fp32 - float64| (loss: absolute; gradient: max |diff| / max |float64 gradient|) and
``E_kind`` = the largest ``e_ref`` of a content kind over all sizes, classes and seeds 0..2.  The kernel must satisfy
``e_kernel <= max(3 E_kind, floor)`` in every case of the kind; 3 is the factor the suite grants over reference spread
(K_SPREAD in tests/test_fullsize_gpu.py); floor = 4 ulp of a loss of order 1 (2.4e-7) resp. 2^-20 of the gradient's maximum.

MEASURED (MI355X; worst e_kernel per kind over every kernel case of this file, against the gate; every line of that run is in
profiles/ssim_parity.txt):
  kind     loss error   gate        gradient error   gate
  noise    9.3e-08      1.82e-06    1.09e-06         9.56e-06
  smooth   1.21e-06     8.48e-06    2.43e-05         2.25e-04
  near     8.3e-07      8.74e-06    4.83e-05         3.52e-04
The kernel uses a seventh to a tenth of the gate; the loss errors are worst at 11 x 11 (one SSIM position per channel, where the
cancellation in E[x^2] - mu^2 is not averaged), the gradient errors at the full-size frames.  Identical pairs: loss and gradient
exactly 0 in every run.
"""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import ssim_ref as R
from tests.helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = golden("ssim_loss")
LOSS_FLOOR, GRAD_FLOOR, K = 4 * 2.0 ** -24, 2.0 ** -20, 3.0

# kind: (worst loss error, loss gate, worst gradient error, gradient gate) as printed by the run in profiles/ssim_parity.txt
MEASURED = {'noise': (9.266e-08, 1.820e-06, 1.093e-06, 9.560e-06),
            'smooth': (1.209e-06, 8.480e-06, 2.432e-05, 2.251e-04),
            'near': (8.348e-07, 8.743e-06, 4.831e-05, 3.519e-04)}


def gates(kind):
    e_loss, e_grad = GOLD['E_' + kind]
    return max(K * float(e_loss), LOSS_FLOOR), max(K * float(e_grad), GRAD_FLOOR)


def offset_copy(t, off):
    """A contiguous device copy of `t` whose first element sits `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


def run_abi(sr, hr, mode, g=None, off=(0, 0)):
    """The three entry points on raw pointers.  -> (loss [rows or 1] cpu float32, range words, gradient cpu)"""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    out_rows = 1 if mode == _hip.SSIM_RANGE_BATCH else N
    res = torch.full((out_rows,), float('nan'), device=DEV)
    word = torch.full((out_rows,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.full((int(lib.savfi_ssim_scratch_floats(N, C, H, W)),), float('nan'), device=DEV)
    _hip.check(lib.savfi_ssim_loss_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), word.data_ptr(), scratch.data_ptr(), N, C, H, W,
                                       mode, st), "savfi_ssim_loss_f32")
    gl = torch.ones(out_rows, device=DEV) if g is None else torch.as_tensor(g, dtype=torch.float32).to(DEV)
    gsr = torch.full(sr.shape, float('nan'), device=DEV)
    rows, ch = (1, N * C) if mode == _hip.SSIM_RANGE_BATCH else (N, C)
    _hip.check(lib.savfi_ssim_loss_bwd_f32(srd.data_ptr(), hrd.data_ptr(), gl.data_ptr(), word.data_ptr(), gsr.data_ptr(), rows, ch, H, W,
                                           st), "savfi_ssim_loss_bwd_f32")
    torch.cuda.synchronize()
    return res.cpu(), word.cpu().tolist(), gsr.cpu()


def check(kind, what, loss, grad, loss64, grad64):
    """Print the figures, then hold them to the kind's gate."""
    g_loss, g_grad = gates(kind)
    e_loss = float((loss.double() - loss64).abs().max())
    e_grad = float((grad.double() - grad64).abs().max() / grad64.abs().max())
    print('SSIM_PARITY kind=%s case=%s e_loss=%.3e gate=%.3e e_grad=%.3e gate=%.3e' % (kind, what, e_loss, g_loss, e_grad, g_grad))
    assert torch.isfinite(grad).all()
    assert e_loss <= g_loss, (what, e_loss, g_loss)
    assert e_grad <= g_grad, (what, e_grad, g_grad)


SIZES = [(11, 11), (12, 75), (37, 53), (64, 64), (256, 448), (720, 1280)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_sample_matches_float64_in_every_range_class(kind, size):
    H, W = size
    for cls in ((0, 1, 2, 3) if H <= 64 else (0, 1)):
        sr, hr = R.make_pair(kind, cls, 1, 3, H, W, 0)
        loss64 = R.ssim_loss(sr.double(), hr.double()).reshape(1)
        grad64 = R.ssim_loss_grad(sr.double(), hr.double())
        name = R.case_name(kind, cls, 1, H, W, 0)
        if name + '/loss64' in GOLD.files:        # the inputs are the ones the reference saw
            assert abs(float(loss64) - float(GOLD[name + '/loss64'])) <= 1e-12
        if name + '/grad64_fp' in GOLD.files:
            assert np.allclose(R.fingerprint(grad64), GOLD[name + '/grad64_fp'], rtol=1e-9, atol=1e-18)
        for mode in (_hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH):
            loss, word, grad = run_abi(sr, hr, mode)
            assert word == [cls]
            check(kind, '%s mode%d' % (name, mode), loss, grad, loss64, grad64)
        if name + '/loss' in GOLD.files:           # and the reference's fp32 value is as far away as its own error plus ours allows
            assert abs(float(loss) - float(GOLD[name + '/loss'])) <= gates(kind)[0] + float(GOLD[name + '/e_ref'][0])


@pytest.mark.parametrize("N,size", [(4, (24, 40)), (8, (37, 53)), (4, (64, 64)), (8, (12, 75))])
@pytest.mark.parametrize("kind", R.KINDS)
def test_rows_per_row_and_whole_batch_with_unequal_cotangents(kind, N, size):
    H, W = size
    classes = [(i + (0 if kind == 'noise' else 1)) % 4 for i in range(N)]          # a batch whose rows fall in different classes
    for cl in (0, 1, classes):
        sr, hr = R.make_pair(kind, cl, N, 3, H, W, 1)
        g = [0.25 + 0.5 * i for i in range(N)]
        # per row: what N calls on the N = 1 slices give
        loss64, cls64 = R.ssim_loss_rows(sr.double(), hr.double())
        grad64 = R.ssim_loss_grad_rows(sr.double(), hr.double(), g)
        loss, word, grad = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, g)
        assert word == cls64
        check(kind, 'rows n%d %dx%d classes %s' % (N, H, W, cl), loss, grad, loss64, grad64)
        # whole batch: one call on the N > 1 tensor
        loss64 = R.ssim_loss(sr.double(), hr.double()).reshape(1)
        grad64 = R.ssim_loss_grad(sr.double(), hr.double(), 1.75)
        loss, word, grad = run_abi(sr, hr, _hip.SSIM_RANGE_BATCH, [1.75])
        assert word == [R.range_class(sr)]
        check(kind, 'batch n%d %dx%d classes %s' % (N, H, W, cl), loss, grad, loss64, grad64)


def test_mixed_class_batch_matches_the_reference_fixture():
    for seed in GOLD['seeds'].tolist():
        sr, hr = R.make_pair('near', [0, 1, 2, 3], 4, 3, 24, 40, seed)
        loss, word, _ = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW)
        assert word == [0, 1, 2, 3]
        assert np.abs(loss.numpy() - GOLD['mixed_s%d/loss_rows' % seed]).max() <= gates('near')[0] + float(GOLD['E_near'][0])
        loss, word, _ = run_abi(sr, hr, _hip.SSIM_RANGE_BATCH)
        assert word == [3]
        assert abs(float(loss) - float(GOLD['mixed_s%d/loss' % seed])) <= gates('near')[0] + float(GOLD['E_near'][0])


@pytest.mark.parametrize("off", [(1, 0), (2, 3), (3, 1), (0, 2)])
@pytest.mark.parametrize("size", [(37, 53), (64, 64), (40, 76)], ids=lambda s: '%dx%d' % s)
def test_operands_off_16_byte_alignment(off, size):
    H, W = size
    sr, hr = R.make_pair('smooth', 0, 2, 3, H, W, 2)
    loss0, _, grad0 = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW)
    loss1, _, grad1 = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, off=off)
    # the scalar tail loads the same values and every sum keeps its association: identical bits
    assert torch.equal(loss0, loss1) and torch.equal(grad0, grad1)
    loss64, _ = R.ssim_loss_rows(sr.double(), hr.double())
    check('smooth', 'offset %s %dx%d' % (off, H, W), loss1, grad1, loss64, R.ssim_loss_grad_rows(sr.double(), hr.double(), [1.0, 1.0]))


def test_fixed_range_mode_ignores_the_data():
    sr, hr = R.make_pair('near', 0, 1, 3, 40, 56, 0)
    for k, L in enumerate(R.CLASS_L):
        loss, word, grad = run_abi(sr, hr, _hip.SSIM_RANGE_FIXED + k)
        assert word == [k]
        loss64 = R.ssim_loss(sr.double(), hr.double(), L).reshape(1)
        check('near', 'fixed L=%g' % L, loss, grad, loss64, R.ssim_loss_grad(sr.double(), hr.double(), 1.0, L))


def test_results_are_bit_reproducible_and_survive_graph_capture():
    sr, hr = R.make_pair('near', [0, 1, 0, 1], 4, 3, 64, 96, 0)
    a = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, [1.0, 2.0, 3.0, 4.0])
    b = run_abi(sr, hr, _hip.SSIM_RANGE_PER_ROW, [1.0, 2.0, 3.0, 4.0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[1] == b[1]
    srd, hrd = sr.to(DEV), hr.to(DEV)
    w = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV)

    def fwd_bwd(x):
        loss = hip_ops.ssim_loss_per_sample(x, hrd)
        g, = torch.autograd.grad((loss * w).sum(), x)
        return loss.detach(), g
    static = srd.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd_bwd(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = fwd_bwd(static)
    for it, classes in enumerate(([0, 1, 0, 1], [1, 0, 3, 2])):           # the second replay changes every row's class: no host decision
        sr2, _ = R.make_pair('near', classes, 4, 3, 64, 96, 0)
        with torch.no_grad():
            static.copy_(sr2.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        loss_e, grad_e = fwd_bwd(static.detach().clone().requires_grad_())
        assert torch.equal(loss_g, loss_e) and torch.equal(grad_g, grad_e), it
        if it == 0:
            assert torch.equal(loss_g.cpu(), a[0]) and torch.equal(grad_g.cpu(), a[2])


@pytest.mark.parametrize("N,size", [(1, (11, 11)), (1, (37, 53)), (1, (64, 64)), (4, (24, 40)), (1, (256, 448)), (1, (720, 1280))])
def test_identical_pair_gives_zero(N, size):
    """sr == hr: the reference returns exactly 0.0; the float64 gradient is 0, so the gradient is held to 3 x the largest element
    of the reference's own fp32 gradient on that pair (pure rounding)."""
    H, W = size
    for cls in (0, 1):
        sr, hr = R.make_pair('same', cls, N, 3, H, W, 0)
        name = R.case_name('same', cls, N, H, W, 0)
        for mode in (_hip.SSIM_RANGE_PER_ROW, _hip.SSIM_RANGE_BATCH):
            loss, _, grad = run_abi(sr, hr, mode)
            print('SSIM_IDENTICAL case=%s mode=%d |loss|=%.3e max|grad|=%.3e reference max|grad|=%.3e' % (
                name, mode, float(loss.abs().max()), float(grad.abs().max()), float(GOLD[name + '/grad_maxabs'])))
            assert float(loss.abs().max()) <= 2.0 ** -23
            assert float(grad.abs().max()) <= 3 * float(GOLD[name + '/grad_maxabs'])


def test_argument_errors():
    lib, st = _hip.lib(), _hip.current_stream()
    t = torch.zeros(3 * 16 * 16, device=DEV)
    w = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    assert lib.savfi_ssim_loss_f32(p, p, p, w.data_ptr(), p, 1, 3, 10, 16, 0, st) == -2          # SAVFI_E_SHAPE
    assert lib.savfi_ssim_loss_f32(p, p, p, w.data_ptr(), p, 1, 3, 16, 10, 0, st) == -2
    assert lib.savfi_ssim_loss_bwd_f32(p, p, p, w.data_ptr(), p, 1, 3, 10, 16, st) == -2
    assert lib.savfi_ssim_scratch_floats(1, 3, 10, 16) == -2
    assert lib.savfi_ssim_loss_f32(None, p, p, w.data_ptr(), p, 1, 3, 16, 16, 0, st) == -1       # SAVFI_E_NULL
    assert lib.savfi_ssim_loss_f32(p, p, p, None, p, 1, 3, 16, 16, 0, st) == -1
    assert lib.savfi_ssim_loss_bwd_f32(p, p, None, w.data_ptr(), p, 1, 3, 16, 16, st) == -1
    assert lib.savfi_ssim_loss_f32(p, p, p, w.data_ptr(), p, 30000, 3, 16, 16, 0, st) == -4      # SAVFI_E_TOOBIG
    assert lib.savfi_ssim_loss_f32(p, p, p, w.data_ptr(), p, 1, 3, 16, 16, 9, st) == -3          # SAVFI_E_UNSUPPORTED
    torch.cuda.synchronize()


def test_hip_ops_surface():
    sr, hr = R.make_pair('near', [0, 1], 2, 3, 48, 64, 0)
    x = sr.to(DEV).requires_grad_()
    loss = hip_ops.ssim_loss(x, hr.to(DEV))
    assert loss.shape == ()
    (2.5 * loss).backward()
    check('near', 'hip_ops.ssim_loss', loss.detach().cpu().reshape(1), x.grad.cpu(), R.ssim_loss(sr.double(), hr.double()).reshape(1),
          R.ssim_loss_grad(sr.double(), hr.double(), 2.5))
    x = sr.to(DEV).requires_grad_()
    rows = hip_ops.ssim_loss_per_sample(x, hr.to(DEV))
    assert rows.shape == (2,)
    (rows * torch.tensor([1.0, 3.0], device=DEV)).sum().backward()
    loss64, _ = R.ssim_loss_rows(sr.double(), hr.double())
    check('near', 'hip_ops.ssim_loss_per_sample', rows.detach().cpu(), x.grad.cpu(), loss64,
          R.ssim_loss_grad_rows(sr.double(), hr.double(), [1.0, 3.0]))
    with pytest.raises(NotImplementedError):
        hip_ops.ssim_loss(sr.to(DEV), hr.to(DEV).requires_grad_())
    # --second_order: the composed device ops give the same numbers and are differentiable twice
    hip_ops.set_double_backward(True)
    try:
        x = sr.to(DEV).requires_grad_()
        rows2 = hip_ops.ssim_loss_per_sample(x, hr.to(DEV))
        g, = torch.autograd.grad(rows2.sum(), x, create_graph=True)
        assert g.requires_grad
        check('near', 'composed per sample', rows2.detach().cpu(), g.detach().cpu(), loss64,
              R.ssim_loss_grad_rows(sr.double(), hr.double(), [1.0, 1.0]))
        tot = hip_ops.ssim_loss(sr.to(DEV), hr.to(DEV))
        assert abs(float(tot) - float(R.ssim_loss(sr.double(), hr.double()))) <= gates('near')[0]
    finally:
        hip_ops.set_double_backward(False)
