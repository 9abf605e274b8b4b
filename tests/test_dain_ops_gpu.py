"""-m gpu: DAIN's adaptive warping layer and depth-aware flow projection (csrc/dainwarp.hip) through the C ABI and through hip_ops with
autograd, against the float64 restatement of tests/dain_ops_ref.py.

Inputs go through the C ABI into NaN-poisoned buffers between canaries, with every pointer at 0 and at 4 bytes past a 16-byte boundary
(the projection's scratch, which holds 64-bit words, at 0 and 8).  The restatement takes its index and validity decisions in float32 as
the kernels do, so no case is excluded.

Gates.
  values       |kernel - float64| <= max(3 E, 4 * 2^-24 * scale) for every output and gradient: E = the largest |fp32-mode restatement -
               float64| of the same case and tensor (sequential fp32 in raster order: the reference's own fp32 error), scale = the
               largest |float64| of that tensor, 3 = the factor the suite grants over reference spread (K_SPREAD), the floor the one
               of tests/test_metrics_gpu.py.  The projection backward reads the forward's `count` and `out` as INPUTS: kernel and
               both restatement modes are given the same (the kernel forward's) values.
  positions    NaN positions equal the restatement's.  Outputs start as NaN, so this also says that every element was written.
  decisions    the pixels with count > 0 are the restatement's exactly; a hole that cannot be filled is exactly 0.
  reproducible two launches give identical bits for the warping forward, g_flow, g_filt and the projection forward (both fillhole
               values) and backward; the two pointer offsets give identical bits too.  g_in (fp32 atomics) is held to the value gate.
  capture      each forward recorded in a torch.cuda.graph and replayed three times on new inputs equals the eager result bit for bit
               (a cleared accumulator that is only cleared in the first replay would show here).
  canaries     intact around every buffer.

MEASURED (MI355X; the worst DAIN_PARITY line per op and tensor of one run of this file, 505 lines in all; the run is in
profiles/dain_ops_parity.txt):
 op             tensor   lines  worst err/gate  err         gate        case
 depthflowproj  count       76  0.191           3.016e-06   1.576e-05   1x4x4/zero/fill0
 depthflowproj  g_flow      70  0.333           3.630e-07   1.089e-06   2x7x9/nonfinite/fill0
 depthflowproj  g_w         70  0.538           5.000e-04   9.299e-04   1x16x64/converge/fill0
 depthflowproj  out         76  0.170           1.884e-06   1.106e-05   1x16x64/uniform/fill0
 filterinterp   g_filt      30  0.551           9.094e-07   1.649e-06   1x3x16x64/nonfinite
 filterinterp   g_flow      30  0.489           5.360e-07   1.096e-06   1x3x16x64/uniform
 filterinterp   g_in       120  0.828           8.097e-07   9.784e-07   1x3x16x64/edge
 filterinterp   out         33  0.620           6.202e-07   1.001e-06   1x3x33x130/edge
"""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import dain_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, K = 4 * 2.0 ** -24, 3.0
CANARY = -12345.678
GUARD = 64

SHAPES = [(1, 1, 4, 4), (2, 3, 7, 9), (2, 5, 17, 33), (1, 3, 16, 64), (1, 3, 33, 130)]
WARP_SHAPES = SHAPES + [(1, 196, 8, 12)]
FLOW_KINDS = ['zero', 'integer', 'uniform', 'edge', 'nonfinite']
PROJ_KINDS = FLOW_KINDS + ['converge', 'leave']


def sid(s):
    return 'x'.join(str(v) for v in s)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references (computed once per case, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------------------
def make_flow(kind, B, H, W, rng):
    if kind == 'zero':
        return np.zeros((B, 2, H, W), np.float32)
    if kind == 'integer':                                             # alpha = beta = 0
        return rng.integers(-3, 4, size=(B, 2, H, W)).astype(np.float32)
    if kind == 'uniform':                                             # reaches every validity clause and every border clamp
        f = rng.uniform(-1.0, 1.0, size=(B, 2, H, W))
        f[:, 0] *= W / 2.0 + 1.0
        f[:, 1] *= H / 2.0 + 1.0
        return f.astype(np.float32)
    if kind == 'edge':                                                # exact hits on W - 1 and H - 1 (and on 0)
        f = rng.uniform(-1.5, 1.5, size=(B, 2, H, W)).astype(np.float32)
        xs, ys = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
        f[:, 0, 0::3, :] = (W - 1) - xs[None, None, :]
        f[:, 1, :, 1::3] = ((H - 1) - ys)[None, :, None]
        f[:, 0, 1::3, 0::2] = -xs[None, None, 0::2]
        f[:, 1, 0::2, 2::3] = -ys[None, 0::2, None]
        return f
    if kind == 'nonfinite':
        f = rng.uniform(-2.5, 2.5, size=(B, 2, H, W)).astype(np.float32)
        f[0, 0, H // 2, W // 2] = np.nan
        f[B - 1, 1, H - 1, 0] = np.inf
        f[0, 1, 0, W - 1] = -np.inf
        return f
    if kind == 'converge':                                            # everything moves towards the centre: holes along the border
        xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
        f = np.empty((B, 2, H, W))
        f[:, 0] = 0.7 * ((W - 1) / 2.0 - xs)[None, None, :] + rng.uniform(-0.3, 0.3, size=(B, H, W))
        f[:, 1] = 0.7 * ((H - 1) / 2.0 - ys)[None, :, None] + rng.uniform(-0.3, 0.3, size=(B, H, W))
        return f.astype(np.float32)
    if kind == 'leave':                                               # sample 0: every source leaves the frame
        f = rng.uniform(-2.5, 2.5, size=(B, 2, H, W)).astype(np.float32)
        f[0] = np.float32(W + H) * np.where(rng.uniform(size=(2, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
        return f
    raise ValueError(kind)


def errs(a32, a64):
    return float(np.nanmax(np.abs(a32.astype(np.float64) - a64), initial=0.0)), float(np.nanmax(np.abs(a64), initial=0.0))


@functools.lru_cache(maxsize=None)
def warp_case(shape, kind):
    B, C, H, W = shape
    rng = np.random.default_rng(1000 + 7 * WARP_SHAPES.index(shape) + FLOW_KINDS.index(kind))
    inp = rng.standard_normal((B, C, H, W)).astype(np.float32)
    filt = (rng.standard_normal((B, 16, H, W)) * 0.25).astype(np.float32)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32)
    flow = make_flow(kind, B, H, W, rng)
    ref = {'out': (R.filterinterp_forward(inp, flow, filt, np.float32), R.filterinterp_forward(inp, flow, filt))}
    b32, b64 = R.filterinterp_backward(inp, flow, filt, gout, np.float32), R.filterinterp_backward(inp, flow, filt, gout)
    for i, name in enumerate(('g_in', 'g_flow', 'g_filt')):
        ref[name] = (b32[i], b64[i])
    for v in ref.values():
        for a in v:
            a.setflags(write=False)
    return dict(inp=inp, flow=flow, filt=filt, gout=gout), ref


@functools.lru_cache(maxsize=None)
def proj_case(shape, kind):
    B, _, H, W = shape
    rng = np.random.default_rng(2000 + 7 * SHAPES.index(shape) + PROJ_KINDS.index(kind))
    flow = make_flow(kind, B, H, W, rng)
    wgt = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), size=(B, 1, H, W))).astype(np.float32)        # depth inverses in [1e-3, 1e2]
    gout = rng.standard_normal((B, 2, H, W)).astype(np.float32)
    ref = {}
    for fill in (0, 1):
        o32, c32 = R.depthflowproj_forward(flow, wgt, fill, np.float32)
        o64, c64 = R.depthflowproj_forward(flow, wgt, fill)
        ref['out%d' % fill], ref['count%d' % fill] = (o32, o64), (c32, c64)
    return dict(flow=flow, wgt=wgt, gout=gout), ref


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

    def scratch(self, nbytes, off_bytes):
        buf = torch.full((nbytes + 2 * 256 + 16,), 0xa5, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        self.raw = (buf, 256 + off_bytes, nbytes)
        return buf[256 + off_bytes:256 + off_bytes + nbytes]

    def check(self):
        for buf, start, n in self.bufs:
            assert bool((buf[:start] == CANARY).all()) and bool((buf[start + n:] == CANARY).all()), "a canary was overwritten"
        if hasattr(self, 'raw'):
            buf, start, n = self.raw
            assert bool((buf[:start] == 0xa5).all()) and bool((buf[start + n:] == 0xa5).all()), "a scratch canary was overwritten"


WORST = {}                      # (op, tensor) -> (err / gate, err, gate, case, lines): the worst DAIN_PARITY line of the session


@pytest.fixture(scope="module", autouse=True)
def _parity_summary():
    """After the last test of this file: the measured worst error per op and tensor, as the MEASURED table prints it (run with -s)."""
    yield
    print()
    print('DAIN_PARITY_SUMMARY  op             tensor   lines  worst err/gate  err         gate        case')
    for (op, name), (ratio, e, gate, case, n) in sorted(WORST.items()):
        print('DAIN_PARITY_SUMMARY  %-14s %-8s %5d  %-14.3f  %.3e   %.3e   %s' % (op, name, n, ratio, e, gate, case))


def gate_check(op, case, name, got, r32, r64):
    """Print the figures, then hold them to the gates."""
    got = got.detach().cpu().numpy()
    E, scale = errs(r32, r64)
    gate = max(K * E, FLOOR * scale)
    assert np.array_equal(np.isnan(got), np.isnan(r64)), (op, case, name, 'NaN positions differ')
    e = float(np.nanmax(np.abs(got.astype(np.float64) - r64), initial=0.0))
    print('DAIN_PARITY op=%s tensor=%s case=%s err=%.3e E=%.3e scale=%.3e gate=%.3e' % (op, name, case, e, E, scale, gate))
    ratio = e / gate if gate > 0 else (0.0 if e == 0 else float('inf'))
    key = (op, name.rstrip('01'))
    prev = WORST.get(key)
    WORST[key] = (ratio, e, gate, case, 1) if prev is None else ((ratio, e, gate, case) if ratio > prev[0] else prev[:4]) + (prev[4] + 1,)
    assert e <= gate, (op, case, name, e, gate)


# ---------------------------------------------------------------------------------------------------------------------------------
# adaptive warping
# ---------------------------------------------------------------------------------------------------------------------------------
def warp_abi(x, off, want=(True, True, True)):
    lib, st = _hip.lib(), _hip.current_stream()
    B, C, H, W = x['inp'].shape
    ar = Arena()
    inp, flow, filt, gout = (ar.put(x[k], off) for k in ('inp', 'flow', 'filt', 'gout'))
    out = ar.out((B, C, H, W), off)
    _hip.check(lib.savfi_filterinterp_fwd_f32(inp.data_ptr(), flow.data_ptr(), filt.data_ptr(), out.data_ptr(), B, C, H, W, 4, st),
               "savfi_filterinterp_fwd_f32")
    g = [ar.out(s, off) if w else None for s, w in zip(((B, C, H, W), (B, 2, H, W), (B, 16, H, W)), want)]
    _hip.check(lib.savfi_filterinterp_bwd_f32(inp.data_ptr(), flow.data_ptr(), filt.data_ptr(), gout.data_ptr(),
                                              *(None if t is None else t.data_ptr() for t in g), B, C, H, W, 4, st),
               "savfi_filterinterp_bwd_f32")
    torch.cuda.synchronize()
    ar.check()
    return dict(out=out, g_in=g[0], g_flow=g[1], g_filt=g[2])


@pytest.mark.parametrize("kind", FLOW_KINDS)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=sid)
def test_warp_abi_matches_float64(shape, kind):
    x, ref = warp_case(shape, kind)
    case = '%s/%s' % (sid(shape), kind)
    a = warp_abi(x, 0)
    for name in ('out', 'g_in', 'g_flow', 'g_filt'):
        gate_check('filterinterp', case, name, a[name], *ref[name])
    b = warp_abi(x, 1)                                               # 4 bytes past a 16-byte boundary; and a second launch
    c = warp_abi(x, 0, want=(False, True, True))                     # without g_in
    for name in ('out', 'g_flow', 'g_filt'):
        assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name]), (case, name)
    gate_check('filterinterp', case + '/off4', 'g_in', b['g_in'], *ref['g_in'])
    d = warp_abi(x, 1, want=(True, False, False))
    gate_check('filterinterp', case + '/g_in only', 'g_in', d['g_in'], *ref['g_in'])


@pytest.mark.parametrize("kind", FLOW_KINDS)
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=sid)
def test_warp_autograd_matches_the_abi(shape, kind):
    x, ref = warp_case(shape, kind)
    case = '%s/%s/autograd' % (sid(shape), kind)
    a = warp_abi(x, 0)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    inp, flow, filt = (t[k].clone().requires_grad_() for k in ('inp', 'flow', 'filt'))
    out = hip_ops.filter_interpolation(inp, flow, filt)
    g_in, g_flow, g_filt = torch.autograd.grad(out, (inp, flow, filt), t['gout'])
    assert torch.equal(out.detach(), a['out']) and torch.equal(g_flow, a['g_flow']) and torch.equal(g_filt, a['g_filt'])
    gate_check('filterinterp', case, 'g_in', g_in, *ref['g_in'])
    # pruning by needs_input_grad: the flow alone
    flow2 = t['flow'].clone().requires_grad_()
    out2 = hip_ops.filter_interpolation(t['inp'], flow2, t['filt'])
    (g2,) = torch.autograd.grad(out2, (flow2,), t['gout'])
    assert torch.equal(g2, a['g_flow']) and torch.equal(out2.detach(), a['out'])


def test_warp_module_views_and_second_order():
    from meta_interpolation_amd.dain.my_package.FilterInterpolation import FilterInterpolationModule
    x, ref = warp_case((2, 3, 7, 9), 'uniform')
    a = warp_abi(x, 0)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    wide = torch.zeros(2, 3, 7, 12, device=DEV)
    wide[..., 2:11] = t['inp']
    out = FilterInterpolationModule()(wide[..., 2:11], t['flow'], t['filt'])           # a view that is not contiguous is made so
    assert torch.equal(out, a['out'])
    flow = t['flow'].clone().requires_grad_()
    out = hip_ops.filter_interpolation(t['inp'], flow, t['filt'])
    (g,) = torch.autograd.grad(out, (flow,), t['gout'], create_graph=True)
    with pytest.raises(RuntimeError):                                                  # once_differentiable: second order raises
        torch.autograd.grad(g.sum(), (flow,))
    with pytest.raises(ValueError):
        hip_ops.filter_interpolation(t['inp'], t['flow'], t['filt'][:, :9])
    with pytest.raises(TypeError):
        hip_ops.filter_interpolation(t['inp'].double(), t['flow'].double(), t['filt'].double())


# ---------------------------------------------------------------------------------------------------------------------------------
# depth-aware flow projection
# ---------------------------------------------------------------------------------------------------------------------------------
def proj_abi(x, off, fill, scratch_off=0):
    lib, st = _hip.lib(), _hip.current_stream()
    B, _, H, W = x['flow'].shape
    ar = Arena()
    flow, wgt, gout = (ar.put(x[k], off) for k in ('flow', 'wgt', 'gout'))
    count, out = ar.out((B, 1, H, W), off), ar.out((B, 2, H, W), off)
    scratch = ar.scratch(int(lib.savfi_depthflowproj_scratch_bytes(B, H, W)), scratch_off)
    _hip.check(lib.savfi_depthflowproj_fwd_f32(flow.data_ptr(), wgt.data_ptr(), count.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                               B, H, W, fill, st), "savfi_depthflowproj_fwd_f32")
    g_flow, g_w = ar.out((B, 2, H, W), off), ar.out((B, 1, H, W), off)
    _hip.check(lib.savfi_depthflowproj_bwd_f32(flow.data_ptr(), wgt.data_ptr(), count.data_ptr(), out.data_ptr(), gout.data_ptr(),
                                               g_flow.data_ptr(), g_w.data_ptr(), B, H, W, st), "savfi_depthflowproj_bwd_f32")
    torch.cuda.synchronize()
    ar.check()
    return dict(out=out, count=count, g_flow=g_flow, g_w=g_w)


def proj_bwd_ref(x, got):
    cnt, out = got['count'].cpu().numpy(), got['out'].cpu().numpy()
    b32 = R.depthflowproj_backward(x['flow'], x['wgt'], cnt, out, x['gout'], np.float32)
    b64 = R.depthflowproj_backward(x['flow'], x['wgt'], cnt, out, x['gout'])
    return {'g_flow': (b32[0], b64[0]), 'g_w': (b32[1], b64[1])}


@pytest.mark.parametrize("kind", PROJ_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_proj_abi_matches_float64(shape, kind):
    x, ref = proj_case(shape, kind)
    for fill in (0, 1):
        case = '%s/%s/fill%d' % (sid(shape[:1] + shape[2:]), kind, fill)
        a = proj_abi(x, 0, fill)
        o64, c64 = ref['out%d' % fill][1], ref['count%d' % fill][1]
        gate_check('depthflowproj', case, 'out', a['out'], *ref['out%d' % fill])
        gate_check('depthflowproj', case, 'count', a['count'], *ref['count%d' % fill])
        cnt, out = a['count'].cpu().numpy(), a['out'].cpu().numpy()
        assert np.array_equal(cnt > 0, c64 > 0), (case, 'the set of pixels something landed on differs')
        assert np.array_equal(cnt == 0, c64 == 0)
        unfilled = (c64[:, 0] <= 0) & (o64[:, 0] == 0) & (o64[:, 1] == 0)               # with fill = 0: every hole
        assert not out.transpose(0, 2, 3, 1)[unfilled].any(), (case, 'a hole that cannot be filled is not exactly 0')
        if kind == 'leave':
            assert not cnt[0].any() and not out[0].any()
        if kind in ('converge', 'leave') and min(shape[2:]) > 4:
            assert (c64 <= 0).any()                                                     # the case does have holes
        bref = proj_bwd_ref(x, a)
        for name in ('g_flow', 'g_w'):
            gate_check('depthflowproj', case, name, a[name], *bref[name])
        b = proj_abi(x, 1, fill, scratch_off=8)                                         # other offsets; and a second launch
        for name in ('out', 'count', 'g_flow', 'g_w'):
            assert torch.equal(a[name], b[name]) or (torch.isnan(a[name]).any() and
                                                     np.array_equal(a[name].cpu().numpy(), b[name].cpu().numpy(), equal_nan=True)), (case, name)


@pytest.mark.parametrize("kind", PROJ_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_proj_autograd_matches_the_abi(shape, kind):
    from meta_interpolation_amd.dain.my_package.DepthFlowProjection import DepthFlowProjectionModule
    x, ref = proj_case(shape, kind)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    for fill in (0, 1):
        a = proj_abi(x, 0, fill)
        flow, wgt = t['flow'].clone().requires_grad_(), t['wgt'].clone().requires_grad_()
        out, count = hip_ops.depth_flow_projection(flow, wgt, fill, return_count=True)
        assert not count.requires_grad
        g_flow, g_w = torch.autograd.grad(out, (flow, wgt), t['gout'])
        for got, name in ((out.detach(), 'out'), (count, 'count'), (g_flow, 'g_flow'), (g_w, 'g_w')):
            assert np.array_equal(got.cpu().numpy(), a[name].cpu().numpy(), equal_nan=True), (shape, kind, fill, name)
        # the module: fillhole = not requires_grad
        assert torch.equal(DepthFlowProjectionModule(requires_grad=not fill)(t['flow'], t['wgt']), a['out'])
    wgt = t['wgt'].clone().requires_grad_()                                             # pruning: the depth inverse alone
    (g,) = torch.autograd.grad(hip_ops.depth_flow_projection(t['flow'], wgt, 0), (wgt,), t['gout'])
    assert np.array_equal(g.cpu().numpy(), proj_abi(x, 0, 0)['g_w'].cpu().numpy(), equal_nan=True)


def test_proj_second_order_raises_and_bad_shapes():
    x, ref = proj_case((2, 3, 7, 9), 'uniform')
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    flow = t['flow'].clone().requires_grad_()
    (g,) = torch.autograd.grad(hip_ops.depth_flow_projection(flow, t['wgt'], 0), (flow,), t['gout'], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), (flow,))
    with pytest.raises(ValueError):
        hip_ops.depth_flow_projection(t['flow'], t['wgt'].expand(2, 2, 7, 9), 0)


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


def test_warp_forward_replays_bit_for_bit_in_a_graph():
    shape = (2, 5, 17, 33)
    x0, _ = warp_case(shape, 'uniform')
    static = [torch.from_numpy(x0[k]).to(DEV) for k in ('inp', 'flow', 'filt')]
    graph, out_g = _capture(lambda a, b, c: hip_ops.filter_interpolation(a, b, c), static)
    for it, kind in enumerate(('edge', 'nonfinite', 'uniform')):
        x, ref = warp_case(shape, kind)
        for s, k in zip(static, ('inp', 'flow', 'filt')):
            s.copy_(torch.from_numpy(x[k]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        eager = hip_ops.filter_interpolation(*(s.clone() for s in static))
        assert torch.equal(out_g, eager), (it, kind)
        gate_check('filterinterp', '%s/%s/graph' % (sid(shape), kind), 'out', out_g, *ref['out'])


@pytest.mark.parametrize("fill", [0, 1])
def test_proj_forward_replays_bit_for_bit_in_a_graph(fill):
    shape = (2, 5, 17, 33)
    x0, _ = proj_case(shape, 'uniform')
    static = [torch.from_numpy(x0[k]).to(DEV) for k in ('flow', 'wgt')]
    graph, (out_g, cnt_g) = _capture(lambda a, b: hip_ops.depth_flow_projection(a, b, fill, return_count=True), static)
    for it, kind in enumerate(('converge', 'leave', 'edge')):                          # accumulators must be cleared in EVERY replay
        x, ref = proj_case(shape, kind)
        for s, k in zip(static, ('flow', 'wgt')):
            s.copy_(torch.from_numpy(x[k]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        out_e, cnt_e = hip_ops.depth_flow_projection(*(s.clone() for s in static), fill, return_count=True)
        assert torch.equal(out_g, out_e) and torch.equal(cnt_g, cnt_e), (it, kind)
        gate_check('depthflowproj', '%s/%s/fill%d/graph' % (sid(shape[:1] + shape[2:]), kind, fill), 'out', out_g, *ref['out%d' % fill])
        gate_check('depthflowproj', '%s/%s/fill%d/graph' % (sid(shape[:1] + shape[2:]), kind, fill), 'count', cnt_g, *ref['count%d' % fill])
