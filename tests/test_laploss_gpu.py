"""-m gpu: the Laplacian-pyramid loss kernels (csrc/laploss.hip) through the C ABI and through hip_ops, against the float64
restatement of tests/laploss_ref.py.

Gate.  The convention of tests/test_msssim_gpu.py: tools/gen_golden_laploss.py measured, for every stored case, ``e_ref`` =
|fp32 composition on the CPU - float64| (value: absolute; gradient: max |diff| / max |float64 gradient|) and ``E_kind`` = the largest
``e_ref`` of a content kind.  The kernel must satisfy ``e_kernel <= max(3 E_kind, floor)``; floor = 4 * 2^-24 (2.4e-7) for the value
and 2^-20 (9.5e-7) of the gradient's maximum.  E_kind is at most 2.9e-8 (value) and 1.7e-7 (gradient): the floors decide.

Conditioning.  The gradient holds sign(b_s); a band element closer to zero than fp32 rounding flips its sign for any fp32 evaluation.
Every pair used for a gradient comparison has min_band >= 2^-18 in float64 (asserted on the CPU before it is used); no element is
left out of a comparison.

MEASURED (MI355X; worst e_kernel per kind over the parity cases of this file, against the gate; every line of that run is in
profiles/laploss_parity.txt):
  kind      value error  gate       gradient error  gate
  noise     1.40e-08     2.38e-07   1.15e-07        9.54e-07
  smooth    1.30e-08     2.38e-07   1.29e-07        9.54e-07
  near      1.34e-09     2.38e-07   1.17e-07        9.54e-07
  constant  1.41e-09     2.38e-07   9.84e-08        9.54e-07      (d = 0.25 at 19 x 33)
Error over gate: value 0.06, 0.05, 0.01, 0.01; gradient 0.12, 0.13, 0.12, 0.10.  The composed form of --second_order: value 1.3e-09, gradient
1.1e-07 (`near`, 37 x 53).  Identical pairs: value and gradient exactly 0 in every run.  Rows against single calls, operand offsets and the
replayed capture: equal bits.
"""
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import laploss_ref as L
from tests import ssim_ref as R
from tests.helpers import golden
from tests.test_ssim_gpu import offset_copy

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = golden("laploss")
K = 3.0
# kind: (worst value error, value gate, worst gradient error, gradient gate) as printed by the run in profiles/laploss_parity.txt
MEASURED = {'noise': (1.404e-08, 2.384e-07, 1.152e-07, 9.537e-07), 'smooth': (1.295e-08, 2.384e-07, 1.287e-07, 9.537e-07),
            'near': (1.344e-09, 2.384e-07, 1.165e-07, 9.537e-07), 'constant': (1.408e-09, 2.384e-07, 9.843e-08, 9.537e-07)}


def gates(kind):
    e_v, e_g = GOLD['E_' + kind]
    return max(K * float(e_v), L.VALUE_FLOOR), max(K * float(e_g), L.GRAD_FLOOR)


def tightest_gates():
    """For content of none of the fixture's kinds (a network's prediction): the smallest gate any kind gives."""
    return tuple(min(gates(kind)[i] for kind in L.KINDS) for i in (0, 1))


def run_abi(sr, hr, levels=5, g=None, off=(0, 0), fold=False, backward=True):
    """The entry points on raw pointers, results into NaN-filled buffers -> (value [rows] cpu, gradient cpu or None, the scratch as
    the forward left it).  fold: one value over the batch, the samples as further planes of one row."""
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = sr.shape
    rows, ch = (1, N * C) if fold else (N, C)
    srd, hrd = offset_copy(sr, off[0]), offset_copy(hr, off[1])
    res = torch.full((rows,), float('nan'), device=DEV)
    nbytes = int(lib.savfi_laploss_scratch_bytes(rows, ch, H, W, levels))
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.full((nbytes // 4,), float('nan'), device=DEV)
    assert scratch.data_ptr() % 16 == 0
    _hip.check(lib.savfi_laploss_f32(srd.data_ptr(), hrd.data_ptr(), res.data_ptr(), scratch.data_ptr(), rows, ch, H, W, levels, st),
               "savfi_laploss_f32")
    fwd_scratch = scratch.clone()
    grad = None
    if backward:
        go = torch.ones(rows, device=DEV) if g is None else torch.as_tensor(g, dtype=torch.float32).to(DEV)
        grad = torch.full(sr.shape, float('nan'), device=DEV)
        _hip.check(lib.savfi_laploss_bwd_f32(srd.data_ptr(), hrd.data_ptr(), go.data_ptr(), scratch.data_ptr(), grad.data_ptr(), rows, ch,
                                             H, W, levels, st), "savfi_laploss_bwd_f32")
        grad = grad.cpu()
    torch.cuda.synchronize()
    return res.cpu(), grad, fwd_scratch


def check(kind, what, value, grad, value64, grad64, gate=None):
    """Print the figures, then hold them to the gate."""
    g_v, g_g = gates(kind) if gate is None else gate
    e_v = float((value.double() - value64).abs().max())
    e_g = float((grad.double() - grad64).abs().max() / grad64.abs().max())
    print('LAPLOSS_PARITY kind=%s case=%s e_value=%.3e gate=%.3e e_grad=%.3e gate=%.3e' % (kind, what, e_v, g_v, e_g, g_g))
    assert torch.isfinite(grad).all() and torch.isfinite(value).all()
    assert e_v <= g_v, (what, e_v, g_v)
    assert e_g <= g_g, (what, e_g, g_g)


def conditioned(kind, N, H, W, levels=5):
    found = L.conditioned_pair(kind, N, 3, H, W, levels)
    assert found is not None, (kind, N, H, W, levels)
    seed, sr, hr = found
    assert L.min_band(sr, hr, levels) >= L.MIN_BAND
    return seed, sr, hr


@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: '%dx%d' % s)
def test_single_sample_matches_float64(size):
    H, W = size
    for kind in L.kinds_at(H, W):
        name = '%s_%dx%d' % (kind, H, W)
        seed = int(GOLD[name + '/seed'])
        sr, hr = R.make_pair(kind, 0, 1, 3, H, W, seed)
        assert L.min_band(sr, hr) >= L.MIN_BAND
        value64, grad64 = L.lap_and_grad(sr, hr)
        assert abs(float(value64) - float(GOLD[name + '/value64'])) <= 1e-12          # the pair the generator measured
        value, grad, scratch = run_abi(sr, hr)
        check(kind, name, value, grad, value64.reshape(1), grad64)
        # the fp32 composition's value is as far away as its own error plus ours allows
        assert abs(float(value) - float(GOLD[name + '/value'])) <= gates(kind)[0] + float(GOLD[name + '/e_ref'][0])
        # level 1 of the difference's pyramid, where the scratch keeps it first (ten fp32 roundings of at most 2^-24 max|c| each)
        c1 = L.gauss(sr.double() - hr.double())[:, :, ::2, ::2]
        got = scratch[:c1.numel()].view(c1.shape).cpu().double()
        assert float((got - c1).abs().max()) <= 2.0 ** -20 * float((sr - hr).abs().max())
        # through hip_ops
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.lap_loss(x, hr.to(DEV))
        gx, = torch.autograd.grad(v, x)
        assert v.shape == () and torch.equal(v.detach().cpu().reshape(1), value) and torch.equal(gx.cpu(), grad)


@pytest.mark.parametrize("kind", L.KINDS)
def test_rows_equal_single_calls_bit_for_bit_and_the_folded_form(kind):
    H, W = 37, 53          # 2 x 2 workgroups on level 0, odd sizes on every level
    g = [0.25, 0.75, 1.25]
    _, sr, hr = conditioned(kind, 3, H, W)
    value, grad, _ = run_abi(sr, hr, g=g)
    for i in range(3):
        v1, g1, _ = run_abi(sr[i:i + 1], hr[i:i + 1], g=g[i:i + 1])
        assert torch.equal(v1, value[i:i + 1]) and torch.equal(g1, grad[i:i + 1])
    check(kind, 'rows3 %dx%d' % (H, W), value, grad, L.lap_rows(sr.double(), hr.double()), L.lap_grad_rows(sr, hr, g))
    # one value over the batch: the samples folded into the planes of one row
    value64, grad64 = L.lap_and_grad(sr, hr)
    value, grad, _ = run_abi(sr, hr, g=[1.75], fold=True)
    check(kind, 'folded %dx%d' % (H, W), value, grad, value64.reshape(1), 1.75 * grad64)
    x = sr.to(DEV).requires_grad_()
    v = hip_ops.lap_loss(x, hr.to(DEV))
    gx, = torch.autograd.grad(1.75 * v, x)
    assert v.shape == () and torch.equal(v.detach().cpu().reshape(1), value) and torch.equal(gx.cpu(), grad)
    x = sr.to(DEV).requires_grad_()
    v = hip_ops.lap_loss_per_sample(x, hr.to(DEV))
    gx, = torch.autograd.grad(v, x, torch.tensor(g, device=DEV))
    rows, grows, _ = run_abi(sr, hr, g=g)
    assert v.shape == (3,) and torch.equal(v.detach().cpu(), rows) and torch.equal(gx.cpu(), grows)


@pytest.mark.parametrize("size", [(7, 9), (9, 7)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize("levels", [2, 3])
def test_fewer_levels_on_small_planes(levels, size):
    H, W = size
    for kind in L.KINDS:
        _, sr, hr = conditioned(kind, 1, H, W, levels)
        value64, grad64 = L.lap_and_grad(sr, hr, levels)
        value, grad, _ = run_abi(sr, hr, levels=levels)
        check(kind, 'levels%d %dx%d' % (levels, H, W), value, grad, value64.reshape(1), grad64)
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.lap_loss_per_sample(x, hr.to(DEV), levels=levels)
        gx, = torch.autograd.grad(v, x, torch.ones(1, device=DEV))
        assert torch.equal(v.detach().cpu(), value) and torch.equal(gx.cpu(), grad)
    with pytest.raises(ValueError):
        hip_ops.lap_loss(sr.to(DEV), hr.to(DEV), levels=4)          # level 2 is 2 x 3 or 3 x 2


@pytest.mark.parametrize("size", L.SIZES, ids=lambda s: '%dx%d' % s)
def test_identical_pair_is_exactly_zero(size):
    H, W = size
    sr, hr = R.make_pair('same', 0, 2, 3, H, W, 0)
    value, grad, _ = run_abi(sr, hr, g=[0.5, 1.5])
    assert value.tolist() == [0.0, 0.0] and float(grad.abs().max()) == 0.0
    value, grad, _ = run_abi(sr, hr, fold=True)
    assert value.tolist() == [0.0] and float(grad.abs().max()) == 0.0


def test_constant_difference_lives_in_the_residual_alone():
    """d = 0.25 at 19 x 33 with the target on the 1 / 256 grid: every Laplacian band is exactly zero in float64, the value is
    16 * 0.25 * n_4 / n_0.  A wrong parity at a reflected border makes non-zero bands there: the value and, through their signs,
    the gradient leave the floors."""
    hr = (torch.rand(1, 3, 19, 33, generator=torch.Generator().manual_seed(1)) * 256).floor() / 256
    sr = hr + 0.25
    assert bool(((sr - hr) == 0.25).all())
    value64, grad64 = L.lap_and_grad(sr, hr)
    assert abs(float(value64) - 16 * 0.25 * 6 / (19 * 33)) <= 1e-15
    value, grad, _ = run_abi(sr, hr)
    check('constant', 'd=0.25 19x33', value, grad, value64.reshape(1), grad64, gate=(L.VALUE_FLOOR, L.GRAD_FLOOR))


def test_alignment_and_reproducibility():
    for H, W in ((37, 53), (64, 64), (40, 300)):
        sr, hr = R.make_pair('near', 0, 2, 3, H, W, 2)
        base = run_abi(sr, hr, g=[0.5, 1.5])
        for off in ((0, 0), (1, 0), (0, 2), (1, 2), (2, 1)):          # operands 4 and 8 bytes off a 16-byte boundary
            again = run_abi(sr, hr, g=[0.5, 1.5], off=off)
            assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
            # the pyramid and the partial sums too, as bits (what the forward does not write keeps the NaN fill)
            assert torch.equal(again[2].view(torch.int32), base[2].view(torch.int32))


def test_one_capture_replays_the_eager_result():
    """Forward and backward in ONE capture on a single stream; the replay after the inputs were refilled in place equals the eager
    result of the new inputs bit for bit (no host read, no cleared memory, nothing left from the capture's data)."""
    first = R.make_pair('near', 0, 2, 3, 37, 53, 0)
    second = R.make_pair('noise', 0, 2, 3, 37, 53, 1)
    go = torch.tensor([0.5, 1.5], device=DEV)

    def eager(pair):
        x = pair[0].to(DEV).requires_grad_()
        v = hip_ops.lap_loss_per_sample(x, pair[1].to(DEV))
        gx, = torch.autograd.grad(v, x, go)
        return v.detach().clone(), gx.clone()
    want1, want2 = eager(first), eager(second)
    x = first[0].to(DEV).requires_grad_()
    y = first[1].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(hip_ops.lap_loss_per_sample(x, y), x, go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = hip_ops.lap_loss_per_sample(x, y)
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
    _, sr, hr = conditioned(kind, 3, 37, 53)
    g = torch.tensor([0.25, 0.75, 1.25])
    rows64, grows64 = L.lap_rows(sr.double(), hr.double()), L.lap_grad_rows(sr, hr, g.tolist())
    hip_ops.set_double_backward(True)
    try:
        x = sr.to(DEV).requires_grad_()
        v = hip_ops.lap_loss_per_sample(x, hr.to(DEV))
        gx, = torch.autograd.grad(v, x, g.to(DEV), create_graph=True)
        check(kind, 'composed per_sample', v.detach().cpu(), gx.detach().cpu(), rows64, grows64)
        assert gx.requires_grad
        ggx, = torch.autograd.grad((gx * torch.linspace(0, 1, gx.numel(), device=DEV).view_as(gx)).sum() + v.pow(2).sum(), x)
        assert torch.isfinite(ggx).all() and float(ggx.abs().max()) > 0
        v = hip_ops.lap_loss(x, hr.to(DEV))
        value64, grad64 = L.lap_and_grad(sr, hr)
        gx, = torch.autograd.grad(v, x)
        check(kind, 'composed one value', v.detach().cpu().reshape(1), gx.cpu(), value64.reshape(1), grad64)
    finally:
        hip_ops.set_double_backward(False)
    with pytest.raises(NotImplementedError):
        hip_ops.lap_loss(sr.to(DEV), hr.to(DEV).requires_grad_())
    with pytest.raises(NotImplementedError):
        hip_ops.lap_loss_per_sample(sr.to(DEV), hr.to(DEV).requires_grad_())
