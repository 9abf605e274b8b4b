"""-m gpu: the kernels of csrc/adacof.hip held to the float64 restatement (tests/adacof_ref.py) inside the counted gates, through the C ABI
into NaN-filled buffers between canaries and through hip_ops.adacof.

Shapes: the five of the definition's CPU suite plus H, W one below, at and one above the tile (4 rows x 64 columns).  Content kinds of the
offsets: small (|offset| < 1), cross (several pixels), outside (every tap beyond a border: the border texel sum exactly, offset gradients
exactly 0), integer (exact coordinates, nothing flagged out, a one-hot weight reproduces the texel bit for bit), wild (+-inf, +-1e30 and
NaN mixed in: finite pixels inside their gates, NaN pixels NaN, canaries intact -- csrc/adacof.hip clamps in float before every
conversion to an integer, and converts fmaxf(floor, -1), which is -1 for a NaN).

Every case prints its ratios to the gates (ADACOF_PARITY ...; profiles/adacof_parity.txt holds a run's worst)."""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import adacof_ref as R
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

BASE = [(1, 3, 5, 7, 5, 1), (2, 3, 9, 33, 5, 1), (1, 3, 17, 40, 3, 2), (1, 1, 8, 32, 1, 1), (1, 3, 6, 6, 11, 2)]          # N, C, H, W, F, d
TILE = [(1, 3, H, W, 3, 1) for H in (R.TILE_H - 1, R.TILE_H, R.TILE_H + 1) for W in (R.TILE_W - 1, R.TILE_W, R.TILE_W + 1)]
SHAPES = BASE + TILE
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
NAN = float('nan')


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """The inputs and the restatement of one case, computed once and shared (never modified)."""
    N, C, H, W, F, d = shape
    x, w, a, b, gout = R.inputs(kind, N, C, H, W, F, d)
    return (x, w, a, b, gout), R.adacof(x, w, a, b, d, gout)


def bits(t):
    return t.contiguous().view(torch.int32)


def shifted(t, off):
    """A device copy of t whose first element sits `off` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def run_abi(shape, tensors, off=0, want=(True, True, True), fwd=True):
    """-> (out, g_w, g_a, g_b) device tensors (None where not asked for) written by the C entries into guarded NaN-filled buffers"""
    N, C, H, W, F, d = shape
    x, w, a, b, gout = (shifted(t, off) for t in tensors)
    G = Guarded()
    new = lambda name, *s: G.new(name, int(np.prod(s)) + off, fill=NAN)[off:].view(*s)
    out = new('out', N, C, H, W) if fwd else None
    gs = [new(n, N, F * F, H, W) if k else None for n, k in zip(('g_w', 'g_a', 'g_b'), want)]
    if fwd:
        assert out.data_ptr() % 16 == 4 * off
        _hip.call("adacof_fwd", "savfi_adacof_fwd_f32", x, w, a, b, out, N, C, H, W, F, d)
    _hip.call("adacof_bwd", "savfi_adacof_bwd_f32", x, w, a, b, gout, *gs, N, C, H, W, F, d)
    torch.cuda.synchronize()
    G.check("adacof %s" % (shape,))
    return (out, *gs)


def ratios(shape, got, ref, keep_pixels=None, mask_near=True):
    """The four ratios to the gates; keep_pixels [N, H, W]: the pixels / taps of pixels that count (wild: the finite ones)"""
    N, C, H, W, F, d = shape
    out, gw, ga, gb = (t.cpu() for t in got)
    taps = None if keep_pixels is None else keep_pixels.unsqueeze(1).expand(N, F * F, H, W)
    chans = None if keep_pixels is None else keep_pixels.unsqueeze(1).expand(N, C, H, W)
    off = ~ref['near'] if mask_near else torch.ones_like(ref['near'])
    off = off if taps is None else off & taps
    return (R.masked_ratio(out, ref['out'], ref['out_mag'], R.fwd_units(F), chans),
            R.masked_ratio(gw, ref['g_w'], ref['g_w_mag'], R.gw_units(C), taps),
            R.masked_ratio(ga, ref['g_a'], ref['g_a_mag'], R.goff_units(C), off),
            R.masked_ratio(gb, ref['g_b'], ref['g_b_mag'], R.goff_units(C), off))


def report(shape, kind, r, extra=""):
    print("ADACOF_PARITY shape=%s kind=%s out=%.3f g_w=%.3f g_a=%.3f g_b=%.3f%s" % (ids(shape), kind, *r, extra))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("kind", ["small", "cross"])
def test_values_and_gradients_inside_the_counted_gates(shape, kind):
    tensors, ref = case(shape, kind)
    share = ref['near'].double().mean().item()
    got = run_abi(shape, tensors)
    r = ratios(shape, got, ref)
    report(shape, kind, r, " near=%.2e" % share)
    assert share <= R.NEAR_CAP
    assert max(r) <= 1.0
    # a second run, and operands / outputs 4 bytes past a 16-byte boundary: the same bits
    again, moved = run_abi(shape, tensors), run_abi(shape, tensors, off=1)
    for p, q, s in zip(got, again, moved):
        assert torch.equal(bits(p), bits(q)) and torch.equal(bits(p), bits(s))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_tap_beyond_a_border(shape):
    N, C, H, W, F, d = shape
    tensors, ref = case(shape, 'outside')
    x, w = tensors[0].numpy(), tensors[1].numpy()
    got = run_abi(shape, tensors)
    r = ratios(shape, got, ref)
    report(shape, 'outside', r)
    assert max(r) <= 1.0
    assert not got[2].any() and not got[3].any()                       # exactly 0, both offset gradients
    # the border texel sum in float32, taps in order, product first
    Hp, Wp = x.shape[2:]
    rows = np.where(np.arange(H) < (H + 1) // 2, 0, Hp - 1)
    cols = np.where(np.arange(W) < (W + 1) // 2, 0, Wp - 1)
    corner = x[:, :, rows][:, :, :, cols]
    acc = np.zeros((N, C, H, W), np.float32)
    for t in range(F * F):
        acc = acc + w[:, t:t + 1] * corner
    assert acc.dtype == np.float32 and np.array_equal(got[0].cpu().numpy(), acc)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_integer_offsets_and_a_one_hot_weight(shape):
    N, C, H, W, F, d = shape
    tensors, ref = case(shape, 'integer')
    x, w, a, b, _ = tensors
    got = run_abi(shape, tensors)
    r = ratios(shape, got, ref, mask_near=False)                       # the coordinate is exact: nothing is flagged out
    report(shape, 'integer', r)
    assert max(r) <= 1.0
    Hp, Wp = x.shape[2:]
    hot = w.argmax(1)                                                  # [N, H, W]
    pick = lambda o: o.gather(1, hot.unsqueeze(1)).squeeze(1).long()
    iy = (torch.arange(H).view(1, H, 1) + (hot // F) * d + pick(a)).clamp(0, Hp - 1)
    ix = (torch.arange(W).view(1, 1, W) + (hot % F) * d + pick(b)).clamp(0, Wp - 1)
    texel = x[torch.arange(N).view(N, 1, 1), :, iy, ix].permute(0, 3, 1, 2)
    assert torch.equal(bits(got[0].cpu()), bits(texel + 0.0))           # (+ 0.0: the running sum turns a -0 into +0)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_wild_offsets_stay_inside_the_frame(shape):
    N, C, H, W, F, d = shape
    tensors, ref = case(shape, 'wild')
    nan_tap = torch.isnan(tensors[2]) | torch.isnan(tensors[3])
    got = run_abi(shape, tensors)                                      # (checks the canaries)
    out, gw, ga, gb = (t.cpu() for t in got)
    assert torch.equal(torch.isnan(out), ref['nan'].unsqueeze(1).expand_as(out))
    for g in (gw, ga, gb):
        assert torch.equal(torch.isnan(g), nan_tap)
    clean = lambda t: torch.nan_to_num(t, nan=0.0)
    finite = dict(ref, **{k: clean(ref[k]) for k in ('out', 'out_mag', 'g_w', 'g_w_mag', 'g_a', 'g_a_mag', 'g_b', 'g_b_mag')})
    finite['near'] = ref['near'] | nan_tap
    r = ratios(shape, (clean(out), clean(gw), clean(ga), clean(gb)), finite, keep_pixels=~ref['nan'])
    # g_w of a finite tap of a NaN pixel is finite and checked too
    r_gw = R.masked_ratio(clean(gw), finite['g_w'], finite['g_w_mag'], R.gw_units(C), ~nan_tap)
    report(shape, 'wild', r, " g_w(all finite taps)=%.3f" % r_gw)
    assert max(r) <= 1.0 and r_gw <= 1.0


@pytest.mark.parametrize("shape", [BASE[1], BASE[2], TILE[8]], ids=ids)
def test_autograd_equals_the_abi_and_gradient_outputs_may_be_null(shape):
    N, C, H, W, F, d = shape
    tensors, ref = case(shape, 'cross')
    full = run_abi(shape, tensors)
    x, w, a, b, gout = (t.cuda() for t in tensors)
    w, a, b = (t.requires_grad_() for t in (w, a, b))
    out = hip_ops.adacof(x, w, a, b, d)
    gw, ga, gb = torch.autograd.grad(out, (w, a, b), gout)
    for p, q in zip(full, (out.detach(), gw, ga, gb)):
        assert torch.equal(bits(p), bits(q))
    # every subset of the three gradients: the same bits, one launch
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)):
        part = run_abi(shape, tensors, want=tuple(map(bool, want)), fwd=False)
        for k, p, q in zip(want, part[1:], full[1:]):
            assert (p is None) == (not k) and (p is None or torch.equal(bits(p), bits(q)))
    names = []
    launch = _hip.launch
    try:
        _hip.launch = lambda name, fn, nbytes=0, flops=0: (names.append((name, nbytes)), launch(name, fn, nbytes=nbytes, flops=flops))
        w2 = w.detach().clone().requires_grad_()
        out = hip_ops.adacof(x, w2, a.detach(), b.detach(), d)
        (g2,) = torch.autograd.grad(out, (w2,), gout)
    finally:
        _hip.launch = launch
    floats = lambda k: 4 * (x.numel() + (3 + k) * w.numel() + out.numel())
    assert names == [("adacof_fwd", floats(0)), ("adacof_bwd", floats(1))] and torch.equal(bits(g2), bits(full[1]))


def test_a_frame_that_requires_grad_is_refused_and_second_order_passes_take_the_composed_op():
    shape = BASE[0]
    tensors, ref = case(shape, 'small')
    x, w, a, b, gout = (t.cuda() for t in tensors)
    with pytest.raises(NotImplementedError, match="frame requires grad"):
        hip_ops.adacof(x.clone().requires_grad_(), w, a, b, 1)
    hip_ops.set_double_backward(True)
    try:
        w, a, b = (t.requires_grad_() for t in (w, a, b))
        out = hip_ops.adacof(x, w, a, b, 1)
        got = (out.detach(),) + torch.autograd.grad(out, (w, a, b), gout, create_graph=True)
        assert all(g.requires_grad for g in got[1:])                     # the gradients carry a graph
    finally:
        hip_ops.set_double_backward(False)
    r = ratios(shape, [g.detach() for g in got], ref)
    report(shape, 'small(composed)', r)
    assert max(r) <= 1.0
