"""-m gpu: the census loss kernels (csrc/census.hip) through the C ABI and through hip_ops, against the float64 restatement of
tests/census_ref.py.

Gate.  The convention of tests/test_laploss_gpu.py: tools/gen_golden_census.py measured, for every stored case, ``e_ref`` =
|fp32 composition on the CPU - float64| (value: absolute; gradient: max |diff| / max |float64 gradient|) and ``E_kind`` = the largest
``e_ref`` of a content kind.  The kernel must satisfy ``e_kernel <= max(3 E_kind, floor)``; floor = 4 * 2^-24 (2.4e-7) for the value
and 2^-20 (9.5e-7) of the gradient's maximum.  E_kind is at most 4.3e-8 for the value: the floor decides.  For the gradient it is
5.7e-7 (noise), 1.2e-6 (smooth) and 4.2e-6 (near) -- cancellation in t(sr) - t(hr), inherent to any fp32 evaluation -- so 3 E_kind
decides: 1.7e-6, 3.5e-6, 1.3e-5.  Content of none of the fixture's kinds (the closed form, the constant offset) is held to the
smallest gate any kind gives.  The definition has no kink: no pair and no element is left out of any comparison.

MEASURED (MI355X; worst e_kernel per kind over the parity cases of this file, against the gate; every line of that run is in
profiles/census_parity.txt):
  kind      value error  gate       gradient error  gate
  noise     1.62e-08     2.38e-07   4.80e-07        1.72e-06
  smooth    5.11e-09     2.38e-07   1.10e-06        3.49e-06
  near      5.79e-10     2.38e-07   4.63e-06        1.27e-05      (the gradient's worst: near_7x9)
  closed    3.94e-09     2.38e-07   4.17e-08        1.72e-06      (0.9 at the centre of 3 x 3)
  constant  4.39e-10     2.38e-07   1.60e-07        1.72e-06      (d = 0.25 at 16 x 21)
Error over gate: value 0.07, 0.02, 0.00, 0.02, 0.00; gradient 0.28, 0.31, 0.36, 0.02, 0.09.  The composed form of --second_order:
value 2.8e-10, gradient 2.8e-06 (`near`, 37 x 53, gate 1.27e-05).  Identical pairs: value and gradient exactly 0 in every run.  Rows
against single calls, operand offsets, repeats and the replayed capture: equal bits.
"""
import functools

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import census_ref as Z
from tests import ssim_ref as R
from tests.helpers import golden
from tests.test_census_ref_cpu import constant_offset_pair
from tests.test_ssim_gpu import offset_copy

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = golden("census")
K = 3.0
# kind: (worst value error, value gate, worst gradient error, gradient gate) as printed by the run in profiles/census_parity.txt
MEASURED = {'noise': (1.623e-08, 2.384e-07, 4.803e-07, 1.724e-06), 'smooth': (5.105e-09, 2.384e-07, 1.097e-06, 3.486e-06),
            'near': (5.785e-10, 2.384e-07, 4.629e-06, 1.271e-05), 'closed': (3.941e-09, 2.384e-07, 4.167e-08, 1.724e-06),
            'constant': (4.392e-10, 2.384e-07, 1.598e-07, 1.724e-06)}


def gates(kind):
    e_v, e_g = GOLD['E_' + kind]
    return max(K * float(e_v), Z.VALUE_FLOOR), max(K * float(e_g), Z.GRAD_FLOOR)


def tightest_gates():
    """For content of none of the fixture's kinds (a network's prediction): the smallest gate any kind gives."""
    return tuple(min(gates(kind)[i] for kind in Z.KINDS) for i in (0, 1))


@functools.lru_cache(maxsize=None)
def pair(kind, N, C, H, W, seed=Z.SEED):
    return R.make_pair(kind, 0, N, C, H, W, seed)


@functools.lru_cache(maxsize=None)
def rows64(kind, N, C, H, W, g=None, seed=Z.SEED):
    """(float64 values [N], float64 gradient for the cotangent g, default ones) of a pair of `pair`; computed once, never changed."""
    sr, hr = pair(kind, N, C, H, W, seed)
    return Z.census_rows(sr.double(), hr.double()), Z.census_grad_rows(sr, hr, [1.0] * N if g is None else list(g))


def run_abi(sr, hr, rows=None, n=1, g=None, off=(0, 0), backward=True):
    """The entry points on raw pointers, results into NaN-filled buffers -> (value [rows] cpu, gradient cpu or None, the scratch as
    the forward left it).  rows * n = N."""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    rows = N // n if rows is None else rows
    assert rows * n == N
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    res = torch.full((rows,), float('nan'), device=DEV)
    nbytes = int(lib.savfi_census_scratch_bytes(rows, n, C, H, W))
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.full((nbytes // 8,), float('nan'), device=DEV, dtype=torch.float64)
    assert scratch.data_ptr() % 16 == 0
    _hip.check(lib.savfi_census_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), scratch.data_ptr(), rows, n, C, H, W, st),
               "savfi_census_f32")
    grad = None
    if backward:
        go = torch.ones(rows, device=DEV) if g is None else torch.as_tensor(g, dtype=torch.float32).to(DEV)
        grad = torch.full(sr.shape, float('nan'), device=DEV)
        _hip.check(lib.savfi_census_bwd_f32(srd.data_ptr(), hrd.data_ptr(), go.data_ptr(), grad.data_ptr(), rows, n, C, H, W, st),
                   "savfi_census_bwd_f32")
        grad = grad.cpu()
    torch.cuda.synchronize()
    return res.cpu(), grad, scratch.cpu()


def check(kind, what, value, grad, value64, grad64, gate=None):
    """Print the figures, then hold them to the gate."""
    g_v, g_g = gates(kind) if gate is None else gate
    e_v = float((value.double() - value64).abs().max())
    e_g = float((grad.double() - grad64).abs().max() / grad64.abs().max())
    print('CENSUS_PARITY kind=%s case=%s e_value=%.3e gate=%.3e e_grad=%.3e gate=%.3e' % (kind, what, e_v, g_v, e_g, g_g))
    assert torch.isfinite(grad).all() and torch.isfinite(value).all()
    assert e_v <= g_v, (what, e_v, g_v)
    assert e_g <= g_g, (what, e_g, g_g)


def through_hip_ops(sr, hr, per_sample, g=None):
    x = sr.to(DEV).requires_grad_()
    v = (hip_ops.census_loss_per_sample if per_sample else hip_ops.census_loss)(x, hr.to(DEV))
    go = torch.ones_like(v) if g is None else torch.as_tensor(g, dtype=torch.float32).to(DEV).reshape(v.shape)
    gx, = torch.autograd.grad(v, x, go)
    return v.detach().cpu(), gx.cpu()


@pytest.mark.parametrize("size", Z.SIZES, ids=lambda s: '%dx%d' % s)
def test_single_sample_matches_float64(size):
    H, W = size
    for kind in Z.KINDS:
        name = '%s_%dx%d' % (kind, H, W)
        sr, hr = pair(kind, 1, 3, H, W, int(GOLD[name + '/seed']))
        value64, grad64 = rows64(kind, 1, 3, H, W)
        assert abs(float(value64) - float(GOLD[name + '/value64'])) <= 1e-12          # the pair the generator measured
        value, grad, scratch = run_abi(sr, hr)
        check(kind, name, value, grad, value64, grad64)
        # the fp32 composition's value is as far away as its own error plus ours allows
        assert abs(float(value) - float(GOLD[name + '/value'])) <= gates(kind)[0] + float(GOLD[name + '/e_ref'][0])
        # the scratch: one finite partial per workgroup, and their sum is the value
        groups = -(-H // 8) * -(-W // 32)
        assert torch.isfinite(scratch[:groups]).all() and bool((scratch[:groups] >= 0).all())
        assert abs(float(scratch[:groups].sum()) / (49 * H * W) - float(value64)) <= gates(kind)[0]
        # through hip_ops
        v, gx = through_hip_ops(sr, hr, False)
        assert v.shape == () and torch.equal(v.reshape(1), value) and torch.equal(gx, grad)
        v, gx = through_hip_ops(sr, hr, True)
        assert v.shape == (1,) and torch.equal(v, value) and torch.equal(gx, grad)


@pytest.mark.parametrize("kind", Z.KINDS)
def test_rows_equal_single_calls_bit_for_bit_and_the_batch_forms(kind):
    H, W = 37, 53          # 2 x 2 workgroups, odd sides
    g = (0.25, 0.75, 1.25)
    sr, hr = pair(kind, 3, 3, H, W)
    value, grad, _ = run_abi(sr, hr, rows=3, n=1, g=g)
    for i in range(3):
        v1, g1, _ = run_abi(sr[i:i + 1], hr[i:i + 1], g=g[i:i + 1])
        assert torch.equal(v1, value[i:i + 1]) and torch.equal(g1, grad[i:i + 1])
    check(kind, 'rows3 n1 %dx%d' % (H, W), value, grad, *rows64(kind, 3, 3, H, W, g))
    v, gx = through_hip_ops(sr, hr, True, g)
    assert v.shape == (3,) and torch.equal(v, value) and torch.equal(gx, grad)
    # rows = 1, n = 3: the mean over the batch, one call
    value64, grad64 = Z.census_and_grad(sr, hr)
    value, grad, _ = run_abi(sr, hr, rows=1, n=3, g=[1.75])
    check(kind, 'rows1 n3 %dx%d' % (H, W), value, grad, value64.reshape(1), 1.75 * grad64)
    v, gx = through_hip_ops(sr, hr, False, 1.75)
    assert v.shape == () and torch.equal(v.reshape(1), value) and torch.equal(gx, grad)
    # rows = 2, n = 2: each row the mean of its two samples, on its own cotangent
    sr4, hr4 = pair(kind, 4, 3, H, W)
    g2 = (0.5, 1.5)
    r64 = Z.census_rows(sr4.double(), hr4.double()).view(2, 2).mean(1)
    g64 = Z.census_grad_rows(sr4, hr4, [g2[0] / 2, g2[0] / 2, g2[1] / 2, g2[1] / 2])
    value, grad, _ = run_abi(sr4, hr4, rows=2, n=2, g=g2)
    check(kind, 'rows2 n2 %dx%d' % (H, W), value, grad, r64, g64)
    for r in range(2):          # a row of two samples is the rows = 1, n = 2 call on them
        v1, g1, _ = run_abi(sr4[2 * r:2 * r + 2], hr4[2 * r:2 * r + 2], rows=1, n=2, g=g2[r:r + 1])
        assert torch.equal(v1, value[r:r + 1]) and torch.equal(g1, grad[2 * r:2 * r + 2])


def test_one_channel():
    H, W = 7, 9
    for kind in Z.KINDS:
        sr, hr = pair(kind, 2, 1, H, W)
        value, grad, _ = run_abi(sr, hr, g=(0.5, 1.5))
        check(kind, 'C1 %dx%d' % (H, W), value, grad, *rows64(kind, 2, 1, H, W, (0.5, 1.5)))
        v, gx = through_hip_ops(sr, hr, True, (0.5, 1.5))
        assert torch.equal(v, value) and torch.equal(gx, grad)


@pytest.mark.parametrize("size", Z.SIZES, ids=lambda s: '%dx%d' % s)
def test_identical_pair_is_exactly_zero(size):
    H, W = size
    sr, hr = R.make_pair('same', 0, 2, 3, H, W, 0)
    value, grad, _ = run_abi(sr, hr, g=[0.5, 1.5])
    assert value.tolist() == [0.0, 0.0] and float(grad.abs().max()) == 0.0
    value, grad, _ = run_abi(sr, hr, rows=1, n=2)
    assert value.tolist() == [0.0] and float(grad.abs().max()) == 0.0
    value, grad, _ = run_abi(sr[:, :1].contiguous(), hr[:, :1].contiguous(), g=[0.5, 1.5])
    assert value.tolist() == [0.0, 0.0] and float(grad.abs().max()) == 0.0


def test_the_closed_form_at_3x3():
    """hr = 0, sr = 0.9 at the centre: 40 / 441 (tests/test_census_ref_cpu.py)."""
    sr = torch.zeros(1, 1, 3, 3)
    sr[0, 0, 1, 1] = 0.9
    hr = torch.zeros_like(sr)
    value64, grad64 = Z.census_and_grad(sr, hr)          # of the fp32 0.9
    assert abs(float(value64) - 40 / 441) <= 1e-8
    value, grad, _ = run_abi(sr, hr)
    check('closed', '0.9 at the centre of 3x3', value, grad, value64.reshape(1), grad64, gate=tightest_gates())
    assert abs(float(value) - 40 / 441) <= Z.VALUE_FLOOR


def test_constant_offset_lives_in_the_border_band():
    """sr = hr + 0.25 at 16 x 21, C = 1, the target on the 1 / 256 grid: every pixel at least 3 from the border contributes exactly 0,
    the value is the border band's, where offsets read the zero padding.  Reflection padding would give value and gradient 0."""
    sr, hr = constant_offset_pair(16, 21)
    assert bool(((sr - hr) == 0.25).all())
    value64, grad64 = Z.census_and_grad(sr, hr)
    assert float(value64) > 1e-3 and float(grad64.abs().max()) > 0
    value, grad, _ = run_abi(sr, hr)
    check('constant', 'd=0.25 16x21', value, grad, value64.reshape(1), grad64, gate=tightest_gates())
    # pixels at least 6 from the border: every neighbour's window lies inside the frame too, and the kernel's differences are exact
    assert float(grad64[:, :, 6:-6, 6:-6].abs().max()) == 0.0 and float(grad[:, :, 6:-6, 6:-6].abs().max()) == 0.0


def test_alignment_and_reproducibility():
    for H, W in ((37, 53), (64, 64), (40, 300)):
        sr, hr = pair('near', 2, 3, H, W, 2)
        base = run_abi(sr, hr, g=[0.5, 1.5])
        for off in ((0, 0), (1, 0), (0, 2), (1, 2), (2, 1)):          # operands 4 and 8 bytes off a 16-byte boundary; (0, 0): a repeat
            again = run_abi(sr, hr, g=[0.5, 1.5], off=off)
            assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
            # the partial sums too, as bits (what the forward does not write keeps the NaN fill)
            assert torch.equal(again[2].view(torch.int64), base[2].view(torch.int64))
        again = run_abi(sr, hr, rows=1, n=2, g=[0.5])
        assert torch.equal(again[0], run_abi(sr, hr, rows=1, n=2, g=[0.5])[0])


def test_one_capture_replays_the_eager_result():
    """Forward and backward in ONE capture on a single stream; the replay after the inputs were refilled in place equals the eager
    result of the new inputs bit for bit (no host read, no cleared memory, nothing left from the capture's data)."""
    first = pair('near', 2, 3, 37, 53, 0)
    second = pair('noise', 2, 3, 37, 53, 1)
    go = torch.tensor([0.5, 1.5], device=DEV)

    def eager(p):
        x = p[0].to(DEV).requires_grad_()
        v = hip_ops.census_loss_per_sample(x, p[1].to(DEV))
        gx, = torch.autograd.grad(v, x, go)
        return v.detach().clone(), gx.clone()
    want1, want2 = eager(first), eager(second)
    x = first[0].to(DEV).requires_grad_()
    y = first[1].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(hip_ops.census_loss_per_sample(x, y), x, go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = hip_ops.census_loss_per_sample(x, y)
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


def test_the_composed_form_and_a_target_with_grad():
    kind = 'near'
    g = (0.25, 0.75, 1.25)
    sr, hr = pair(kind, 3, 3, 37, 53)
    hip_ops.set_double_backward(True)
    try:
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.census_loss_per_sample(x, hr.to(DEV))
        gx, = torch.autograd.grad(v, x, torch.tensor(g, device=DEV), create_graph=True)
        check(kind, 'composed per_sample', v.detach().cpu(), gx.detach().cpu(), *rows64(kind, 3, 3, 37, 53, g))
        assert gx.requires_grad
        ggx, = torch.autograd.grad((gx * torch.linspace(0, 1, gx.numel(), device=DEV).view_as(gx)).sum() + v.pow(2).sum(), x)
        assert torch.isfinite(ggx).all() and float(ggx.abs().max()) > 0
        v = hip_ops.census_loss(x, hr.to(DEV))
        value64, grad64 = Z.census_and_grad(sr, hr)
        gx, = torch.autograd.grad(v, x)
        check(kind, 'composed one value', v.detach().cpu().reshape(1), gx.cpu(), value64.reshape(1), grad64)
    finally:
        hip_ops.set_double_backward(False)
    with pytest.raises(NotImplementedError):
        hip_ops.census_loss(sr.to(DEV), hr.to(DEV).requires_grad_())
    with pytest.raises(NotImplementedError):
        hip_ops.census_loss_per_sample(sr.to(DEV), hr.to(DEV).requires_grad_())
