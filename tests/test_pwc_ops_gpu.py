"""-m gpu: PWC-Net's correlation (forward, both gradients) and warp (csrc/correlation.hip) through the C ABI and through hip_ops, against
the float64 restatement of tests/pwc_ref.py.

Inputs go through the C ABI into NaN-poisoned buffers between canaries, with every pointer at 0 and at 4 bytes past a 16-byte boundary.
The restatement multiplies by the padded zeros and takes the warp's coordinate chain and threshold decision in float32 as the kernels do,
so no case is excluded.

Gates.
  values       |kernel - float64| <= max(3 E, 4 * 2^-24 * scale) for every output and gradient: E = the largest |fp32-mode restatement -
               float64| of the same case and tensor (sequential fp32 sums in raster order: the reference's own fp32 error), scale = the
               largest finite |float64| of that tensor; factor and floor as in tests/test_dain_ops_gpu.py.  The backward with a fused
               slope reads the forward's `out` as an INPUT: kernel and both restatement modes are given the kernel forward's values.
  exact        the `integer` and `onehot` kinds have exact products and sums: forward and unmasked gradients equal the fp32-mode
               restatement bit for bit and, without a slope, the float64 result rounded once.
  positions    NaN, +inf and -inf positions equal the restatement's.  Outputs start as NaN: every element was written.
  decisions    the pixels the warp zeroes are the restatement's exactly.
  reproducible two launches give identical bits for every output and gradient, the two pointer offsets too, and a gradient asked for
               alone equals the one asked for with the other.
  capture      each forward recorded in a torch.cuda.graph and replayed three times on new inputs equals the eager result bit for bit.
  canaries     intact around every buffer.
  autograd     hip_ops.correlation through autograd equals the ABI call bit for bit.

MEASURED: not yet -- this file has not run on an MI355X.  A run with -s prints one PWC_PARITY line per comparison and the worst per op
and tensor as PWC_PARITY_SUMMARY; that table belongs here and the whole run in profiles/pwc_ops_parity.txt.
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import pwc_ref as R
from tests.test_dain_ops_gpu import make_flow

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, K = 4 * 2.0 ** -24, 3.0
CANARY = -12345.678
GUARD = 64

CORR_SHAPES = [(1, 1, 1, 1), (1, 3, 3, 5), (2, 5, 9, 9), (1, 32, 17, 70), (1, 33, 37, 19), (2, 196, 4, 7)]
CORR_KINDS = ['normal', 'integer', 'onehot', 'nonfinite']
WARP_SHAPES = [(1, 1, 1, 1), (2, 3, 7, 9), (1, 32, 17, 70), (2, 196, 4, 7)]
FLOW_KINDS = ['zero', 'integer', 'uniform', 'edge', 'nonfinite', 'hits']
SCALES = [1.0, 0.625]
SLOPE = 0.1


def sid(s):
    return 'x'.join(str(v) for v in s)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references (computed once per case, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def corr_case(shape, kind):
    N, C, H, W = shape
    rng = np.random.default_rng(3000 + 7 * CORR_SHAPES.index(shape) + CORR_KINDS.index(kind))
    if kind in ('normal', 'nonfinite'):
        f1, f2 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        gout = rng.standard_normal((N, 81, H, W)).astype(np.float32)
    elif kind == 'integer':
        f1, f2 = (rng.integers(-3, 4, size=shape).astype(np.float32) for _ in range(2))
        gout = rng.integers(-3, 4, size=(N, 81, H, W)).astype(np.float32)
    else:                                                        # onehot: out[tc, y, x] = f2[(y W + x) % C, y + tj, x + ti] / C
        f1 = np.zeros(shape, np.float32)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        f1[:, (ys * W + xs) % C, ys, xs] = 1.0
        f2 = (1.0 + np.arange(N * C * H * W, dtype=np.float32)).reshape(shape)
        gout = rng.integers(-3, 4, size=(N, 81, H, W)).astype(np.float32)
    if kind == 'nonfinite':
        f1[0, C // 2, H // 2, W // 2] = np.nan
        f1[N - 1, 0, H - 1, 0] = np.inf
        f2[0, C - 1, 0, W - 1] = np.nan
        f2[N - 1, 0, H // 3, W // 3] = -np.inf
        gout[0, 40, H // 2, 0] = np.nan
        gout[N - 1, 7, 0, W // 2] = np.inf
    x = dict(f1=f1, f2=f2, gout=gout)
    _frozen(f1, f2, gout)
    ref = {}
    for slope in (1.0, SLOPE):
        ref['out', slope] = _frozen(R.correlation_forward(f1, f2, slope=slope, dtype=np.float32),
                                    R.correlation_forward(f1.astype(np.float64), f2.astype(np.float64), slope=slope))
    return x, ref


def corr_bwd_ref(x, out, slope):
    """(g1, g2) -> (fp32 mode, float64); `out`: the kernel forward's result (None: no mask)"""
    ref = {}
    for name, fn, other in (('g1', R.correlation_backward_input1, 'f2'), ('g2', R.correlation_backward_input2, 'f1')):
        ref[name] = (fn(x[other], x['gout'], out=out, slope=slope, dtype=np.float32),
                     fn(x[other].astype(np.float64), x['gout'].astype(np.float64), out=out, slope=slope))
    return ref


def hits_flow(B, H, W, scale):
    """Positions that land on column 0 / W - 1 and row 0 / H - 1: exactly where the distance is representable after the multiply by
    `scale` (always for scale 1; the multiples of 5 for 0.625 = 5 / 8), within an ulp elsewhere."""
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    f = np.empty((B, 2, H, W))
    f[:, 0, 0::2, :] = ((0 - xs) / scale)[None, None, :]
    f[:, 0, 1::2, :] = ((W - 1 - xs) / scale)[None, None, :]
    f[:, 1, :, 0::2] = ((0 - ys) / scale)[None, :, None]
    f[:, 1, :, 1::2] = ((H - 1 - ys) / scale)[None, :, None]
    return f.astype(np.float32)


@functools.lru_cache(maxsize=None)
def warp_case(shape, kind, scale):
    B, C, H, W = shape
    rng = np.random.default_rng(4000 + 7 * WARP_SHAPES.index(shape) + FLOW_KINDS.index(kind))
    img = rng.standard_normal(shape).astype(np.float32)
    flow = hits_flow(B, H, W, scale) if kind == 'hits' else make_flow(kind, B, H, W, rng)
    r32 = R.pwc_warp(img, flow, scale, np.float32)
    r64, mask = R.pwc_warp(img, flow, scale, np.float64, return_mask=True)
    _frozen(img, flow, r32, r64, mask)
    return dict(img=img, flow=flow), (r32, r64), mask


# ---------------------------------------------------------------------------------------------------------------------------------
# buffers between canaries
# ---------------------------------------------------------------------------------------------------------------------------------
class Arena:
    def __init__(self):
        self.bufs = []

    def _place(self, n, off):
        buf = torch.full((GUARD + off + n + GUARD,), CANARY, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[GUARD + off:GUARD + off + n]
        assert view.data_ptr() % 16 == 4 * off
        self.bufs.append((buf, GUARD + off, n))
        return view

    def put(self, a, off):
        """a host array -> a contiguous device view `off` floats past a 16-byte boundary"""
        v = self._place(a.size, off)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1))
        return v.view(a.shape)

    def out(self, shape, off):
        """an output buffer poisoned with NaN"""
        v = self._place(int(np.prod(shape)), off)
        v.fill_(float('nan'))
        return v.view(shape)

    def check(self):
        for buf, start, n in self.bufs:
            assert bool((buf[:start] == CANARY).all()) and bool((buf[start + n:] == CANARY).all()), "a canary was overwritten"


WORST = {}                      # (op, tensor) -> (err / gate, err, gate, case, lines): the worst PWC_PARITY line of the session


@pytest.fixture(scope="module", autouse=True)
def _parity_summary():
    """After the last test of this file: the measured worst error per op and tensor, as the MEASURED table prints it (run with -s)."""
    yield
    print()
    print('PWC_PARITY_SUMMARY  op           tensor  lines  worst err/gate  err         gate        case')
    for (op, name), (ratio, e, gate, case, n) in sorted(WORST.items()):
        print('PWC_PARITY_SUMMARY  %-12s %-6s %6d  %-14.3f  %.3e   %.3e   %s' % (op, name, n, ratio, e, gate, case))


def gate_check(op, case, name, got, r32, r64):
    """Print the figures, then hold them to the gates."""
    got = got.detach().cpu().numpy()
    finite = np.isfinite(r64)
    with np.errstate(invalid='ignore'):
        E = float(np.abs(r32.astype(np.float64) - r64)[finite & np.isfinite(r32)].max(initial=0.0))
        scale = float(np.abs(r64[finite]).max(initial=0.0))
        gate = max(K * E, FLOOR * scale)
        for what, test in (('NaN', np.isnan), ('+inf', np.isposinf), ('-inf', np.isneginf)):
            assert np.array_equal(test(got), test(r64)), (op, case, name, what + ' positions differ')
        e = float(np.abs(got.astype(np.float64) - r64)[finite].max(initial=0.0))
    print('PWC_PARITY op=%s tensor=%s case=%s err=%.3e E=%.3e scale=%.3e gate=%.3e' % (op, name, case, e, E, scale, gate))
    ratio = e / gate if gate > 0 else (0.0 if e == 0 else float('inf'))
    prev = WORST.get((op, name))
    WORST[op, name] = (ratio, e, gate, case, 1) if prev is None else ((ratio, e, gate, case) if ratio > prev[0] else prev[:4]) + (prev[4] + 1,)
    assert e <= gate, (op, case, name, e, gate)


# ---------------------------------------------------------------------------------------------------------------------------------
# correlation
# ---------------------------------------------------------------------------------------------------------------------------------
def corr_abi(x, off, slope, with_out, want=(True, True)):
    lib, st = _hip.lib(), _hip.current_stream()
    N, C, H, W = x['f1'].shape
    ar = Arena()
    f1, f2, gout = (ar.put(x[k], off) for k in ('f1', 'f2', 'gout'))
    out = ar.out((N, 81, H, W), off)
    _hip.check(lib.savfi_correlation_fwd_f32(f1.data_ptr(), f2.data_ptr(), out.data_ptr(), N, C, H, W, 4, slope, st),
               "savfi_correlation_fwd_f32")
    g = [ar.out((N, C, H, W), off) if w else None for w in want]
    _hip.check(lib.savfi_correlation_bwd_f32(f1.data_ptr(), f2.data_ptr(), gout.data_ptr(), out.data_ptr() if with_out else None, slope,
                                             *(None if t is None else t.data_ptr() for t in g), N, C, H, W, 4, st),
               "savfi_correlation_bwd_f32")
    torch.cuda.synchronize()
    ar.check()
    return dict(out=out, g1=g[0], g2=g[1])


@pytest.mark.parametrize("kind", CORR_KINDS)
@pytest.mark.parametrize("shape", CORR_SHAPES, ids=sid)
def test_correlation_abi_matches_float64(shape, kind):
    x, ref = corr_case(shape, kind)
    case = '%s/%s' % (sid(shape), kind)
    exact = kind in ('integer', 'onehot')
    # no slope, no mask
    a = corr_abi(x, 0, 1.0, False)
    bref = corr_bwd_ref(x, None, 1.0)
    gate_check('correlation', case, 'out', a['out'], *ref['out', 1.0])
    for name in ('g1', 'g2'):
        gate_check('correlation', case, name, a[name], *bref[name])
    if exact:
        for name, (r32, r64) in (('out', ref['out', 1.0]), ('g1', bref['g1']), ('g2', bref['g2'])):
            got = a[name].cpu().numpy()
            assert np.array_equal(got, r32) and np.array_equal(got, r64.astype(np.float32)), (case, name, 'not exact')
    b = corr_abi(x, 1, 1.0, False)                                   # 4 bytes past a 16-byte boundary; and a second launch
    u = corr_abi(x, 1, SLOPE, False)                                 # a slope without `out`: no mask in the backward
    for name in ('out', 'g1', 'g2'):
        assert bits_equal(a[name], b[name]), (case, name)
    assert bits_equal(a['g1'], u['g1']) and bits_equal(a['g2'], u['g2'])
    # LeakyReLU fused, its derivative taken from `out`
    c = corr_abi(x, 0, SLOPE, True)
    gate_check('correlation', case + '/slope', 'out', c['out'], *ref['out', SLOPE])
    if exact:
        assert np.array_equal(c['out'].cpu().numpy(), ref['out', SLOPE][0]), (case, 'slope: not exact')
    assert bits_equal(c['out'], u['out'])
    mref = corr_bwd_ref(x, c['out'].cpu().numpy(), SLOPE)
    for name in ('g1', 'g2'):
        gate_check('correlation', case + '/slope', name, c[name], *mref[name])
    d = corr_abi(x, 1, SLOPE, True, want=(True, False))              # each gradient alone (the other NULL), other offset
    e = corr_abi(x, 1, SLOPE, True, want=(False, True))
    assert d['g2'] is None and e['g1'] is None
    assert bits_equal(c['g1'], d['g1']) and bits_equal(c['g2'], e['g2']) and bits_equal(c['out'], d['out']), case


@pytest.mark.parametrize("kind", ['normal', 'nonfinite'])
@pytest.mark.parametrize("shape", CORR_SHAPES, ids=sid)
def test_correlation_autograd_matches_the_abi(shape, kind):
    x, _ = corr_case(shape, kind)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    for slope, with_out in ((1.0, False), (SLOPE, True)):
        a = corr_abi(x, 0, slope, with_out)
        f1, f2 = t['f1'].clone().requires_grad_(), t['f2'].clone().requires_grad_()
        out = hip_ops.correlation(f1, f2, 4, slope)
        g1, g2 = torch.autograd.grad(out, (f1, f2), t['gout'])
        assert bits_equal(out.detach(), a['out']) and bits_equal(g1, a['g1']) and bits_equal(g2, a['g2']), (shape, kind, slope)
        f2b = t['f2'].clone().requires_grad_()                       # pruning by needs_input_grad: f2 alone
        (g2b,) = torch.autograd.grad(hip_ops.correlation(t['f1'], f2b, 4, slope), (f2b,), t['gout'])
        assert bits_equal(g2b, a['g2'])


def test_correlation_module_views_second_order_and_bad_arguments():
    from meta_interpolation_amd.dain.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    x, _ = corr_case((2, 5, 9, 9), 'normal')
    a = corr_abi(x, 0, SLOPE, True)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    corr = Correlation(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1)
    wide = torch.zeros(2, 5, 9, 12, device=DEV)
    wide[..., 2:11] = t['f1']
    assert bits_equal(corr(wide[..., 2:11], t['f2'], SLOPE), a['out'])                 # a view that is not contiguous is made so
    assert bits_equal(corr(t['f1'], t['f2']), corr_abi(x, 0, 1.0, False)['out'])       # the reference's call: no activation
    f1 = t['f1'].clone().requires_grad_()
    (g,) = torch.autograd.grad(hip_ops.correlation(f1, t['f2']), (f1,), t['gout'], create_graph=True)
    with pytest.raises(RuntimeError):                                                  # once_differentiable: second order raises
        torch.autograd.grad(g.sum(), (f1,))
    with pytest.raises(ValueError):
        hip_ops.correlation(t['f1'], t['f2'][:, :3])
    with pytest.raises(TypeError):
        hip_ops.correlation(t['f1'].double(), t['f2'].double())
    with pytest.raises(_hip.SavfiHipError, match="UNSUPPORTED"):
        hip_ops.correlation(t['f1'], t['f2'], md=3)


# ---------------------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------------------
def warp_abi(x, off, scale):
    lib, st = _hip.lib(), _hip.current_stream()
    B, C, H, W = x['img'].shape
    ar = Arena()
    img, flow = ar.put(x['img'], off), ar.put(x['flow'], off)
    out = ar.out((B, C, H, W), off)
    _hip.check(lib.savfi_pwcwarp_fwd_f32(img.data_ptr(), flow.data_ptr(), scale, out.data_ptr(), B, C, H, W, st), "savfi_pwcwarp_fwd_f32")
    torch.cuda.synchronize()
    ar.check()
    return out


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind", FLOW_KINDS)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=sid)
def test_warp_abi_matches_float64(shape, kind, scale):
    x, ref, mask = warp_case(shape, kind, scale)
    case = '%s/%s/s%g' % (sid(shape), kind, scale)
    a = warp_abi(x, 0, scale)
    gate_check('pwcwarp', case, 'out', a, *ref)
    got = a.cpu().numpy()
    zeroed = ~got.any(axis=1)
    assert np.array_equal(zeroed, ~(mask >= np.float32(0.9999))), (case, 'the zeroed pixels differ from the float32 decision')
    assert np.array_equal(zeroed, ~ref[1].any(axis=1))
    if kind == 'zero':
        assert not zeroed.any()
    if kind == 'nonfinite':
        bad = ~np.isfinite(x['flow']).all(axis=1)
        assert bad.any() and zeroed[bad].all()                                          # NaN / inf flows sample nothing
    if kind == 'hits' and min(shape[2:]) > 1:
        assert (mask == 1).any() and not zeroed.all()                                   # exact hits keep their pixel
    b = warp_abi(x, 1, scale)                                                           # other offset; and a second launch
    assert bits_equal(a, b), case
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    assert bits_equal(hip_ops.pwc_warp(t['img'], t['flow'], scale), a)


def test_warp_refuses_gradients_and_bad_shapes():
    x, _, _ = warp_case((2, 3, 7, 9), 'uniform', 1.0)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    for name in ('img', 'flow'):
        args = dict(t)
        args[name] = t[name].clone().requires_grad_()
        with pytest.raises(NotImplementedError):
            hip_ops.pwc_warp(args['img'], args['flow'], 1.0)
        with torch.no_grad():
            assert bits_equal(hip_ops.pwc_warp(args['img'], args['flow'], 1.0), warp_abi(x, 0, 1.0))
    with pytest.raises(ValueError):
        hip_ops.pwc_warp(t['img'], t['flow'][:, :1], 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------------------------------------------
def _capture(fn, static):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(*static)                                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fn(*static)
    return graph, res


@pytest.mark.parametrize("slope", [1.0, SLOPE])
def test_correlation_forward_replays_bit_for_bit_in_a_graph(slope):
    shape = (1, 33, 37, 19)
    x0, _ = corr_case(shape, 'integer')
    static = [torch.from_numpy(x0[k]).to(DEV) for k in ('f1', 'f2')]
    graph, out_g = _capture(lambda a, b: hip_ops.correlation(a, b, 4, slope), static)
    for it, kind in enumerate(('normal', 'nonfinite', 'onehot')):
        x, ref = corr_case(shape, kind)
        for s, k in zip(static, ('f1', 'f2')):
            s.copy_(torch.from_numpy(x[k]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out_g, hip_ops.correlation(*(s.clone() for s in static), 4, slope)), (it, kind)
        gate_check('correlation', '%s/%s/slope%g/graph' % (sid(shape), kind, slope), 'out', out_g, *ref['out', slope])


def test_warp_forward_replays_bit_for_bit_in_a_graph():
    shape, scale = (1, 32, 17, 70), 0.625
    x0, _, _ = warp_case(shape, 'zero', scale)
    static = [torch.from_numpy(x0[k]).to(DEV) for k in ('img', 'flow')]
    graph, out_g = _capture(lambda a, b: hip_ops.pwc_warp(a, b, scale), static)
    for it, kind in enumerate(('uniform', 'nonfinite', 'hits')):
        x, ref, _ = warp_case(shape, kind, scale)
        for s, k in zip(static, ('img', 'flow')):
            s.copy_(torch.from_numpy(x[k]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out_g, hip_ops.pwc_warp(*(s.clone() for s in static), scale)), (it, kind)
        gate_check('pwcwarp', '%s/%s/s%g/graph' % (sid(shape), kind, scale), 'out', out_g, *ref)
