"""-m gpu: the kernels of csrc/softsplat.hip held to the float64 loop restatement (tests/softsplat_ref.py), through the C ABI into NaN-filled
buffers between canaries and through hip_ops.softsplat.

Values and the three gradients must lie within max(K * E, FLOOR * scale) of the float64 restatement, K = 3 and FLOOR = 4 * 2^-24 as for the
scatter ops of tests/test_dain_ops_gpu.py, E the error of the float32 sequential twin against float64 on the same inputs, scale the largest
magnitude of the float64 tensor; no element is left out and NaN positions must be identical.  hit is compared bit for bit in every kind,
`integer` content in sum mode bit for bit.  Content kinds: tests/softsplat_ref.py.  `nonfinite` puts 1e30 into the metric only where the
flow leaves the frame as well: 1e30 is a finite metric and by the definition would take part.

Every gated case prints its ratios (SOFTSPLAT_PARITY ...; profiles/softsplat_parity.txt holds a run's worst)."""
import functools

import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import softsplat_ref as R
from tests.helpers import Guarded, record_launches

pytestmark = pytest.mark.gpu

FLOOR, K = 4 * 2.0 ** -24, 3.0
NAN = float('nan')
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
NAMES = ('out', 'g_x', 'g_flow', 'g_metric')
# sum and avg read no metric: the kinds that differ in the metric alone are run in soft mode only
CASES = [(mode, kind) for mode in R.MODES for kind in R.GATED + ('nonfinite',)] + [('soft', 'shifted')]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_summary():
    yield
    print()
    print('SOFTSPLAT_PARITY_SUMMARY tensor    lines  worst err/gate  err         gate        case')
    for name, (ratio, e, gate, case, n) in sorted(WORST.items()):
        print('SOFTSPLAT_PARITY_SUMMARY %-9s %5d  %-14.3f  %.3e   %.3e   %s' % (name, n, ratio, e, gate, case))


@functools.lru_cache(maxsize=None)
def case(shape, kind, mode):
    """The inputs, the float64 restatement and its float32 twin of one case, computed once and shared (never modified)."""
    x, flow, metric, gout = R.inputs(kind, shape)
    return (x, flow, metric, gout), R.softsplat(x, flow, metric, mode, gout), R.softsplat(x, flow, metric, mode, gout, acc=np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all((p is None and q is None) or torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def run_abi(tensors, mode, want=(True, True, True), fwd=None):
    """-> dict of device tensors written by the C entries into guarded NaN-filled buffers: out, hit, den, mx and the gradients asked for.
    fwd: the (out, den, mx) of an earlier forward, to run the backward alone."""
    x, flow, metric, gout = (t.cuda() for t in tensors)
    N, C, H, W = x.shape
    z = metric if mode == 'soft' else None
    G = Guarded()
    res = {}
    if fwd is None:
        for name, c in (('out', C), ('hit', 1), ('den', 1), ('mx', 1)):
            res[name] = G.new(name, N, c, H, W, fill=NAN)
        nbytes = _hip.lib().savfi_softsplat_scratch_bytes(N, C, H, W)
        assert nbytes > 0 and nbytes % 16 == 0
        scratch = G.new('scratch', nbytes // 4, fill=NAN)
        _hip.call("softsplat_fwd", "savfi_softsplat_fwd_f32", x, flow, z, res['out'], res['hit'], res['den'], res['mx'], scratch, N, C, H, W,
                  _hip.SOFTSPLAT_MODES[mode])
    else:
        res.update(zip(('out', 'den', 'mx'), fwd))
    if any(want):
        for name, c, k in (('g_x', C, want[0]), ('g_flow', 2, want[1]), ('g_metric', 1, want[2])):
            res[name] = G.new(name, N, c, H, W, fill=NAN) if k else None
        _hip.call("softsplat_bwd", "savfi_softsplat_bwd_f32", x, flow, z, res['out'], res['den'], res['mx'], gout, res['g_x'], res['g_flow'],
                  res['g_metric'], N, C, H, W, _hip.SOFTSPLAT_MODES[mode])
    torch.cuda.synchronize()
    G.check("softsplat %s %s" % (tuple(x.shape), mode))
    return res


def gate_check(what, name, got, r32, r64):
    """Print the figures, then hold them to the gate; every element counts."""
    got = got.detach().cpu().numpy()
    E = float(np.nanmax(np.abs(r32.astype(np.float64) - r64), initial=0.0))
    scale = float(np.nanmax(np.abs(r64), initial=0.0))
    gate = max(K * E, FLOOR * scale)
    assert np.array_equal(np.isnan(got), np.isnan(r64)), (what, name, 'NaN positions differ')
    e = float(np.nanmax(np.abs(got.astype(np.float64) - r64), initial=0.0))
    ratio = e / gate if gate > 0 else (0.0 if e == 0 else float('inf'))
    print('SOFTSPLAT_PARITY tensor=%s case=%s err=%.3e E=%.3e scale=%.3e gate=%.3e ratio=%.3f' % (name, what, e, E, scale, gate, ratio))
    prev = WORST.get(name)
    WORST[name] = (ratio, e, gate, what, 1) if prev is None else ((ratio, e, gate, what) if ratio > prev[0] else prev[:4]) + (prev[4] + 1,)
    assert e <= gate, (what, name, e, gate)


def check_case(shape, kind, mode, got):
    _, r64, r32 = case(shape, kind, mode)
    what = '%s/%s/%s' % (ids(shape), kind, mode)
    assert np.array_equal(got['hit'].cpu().numpy(), r64['hit'].astype(np.float32)), (what, 'hit')
    for name in NAMES:
        gate_check(what, name, got[name], r32[name], r64[name])
    gate_check(what, 'D', got['den'], r32['D'], r64['D'])
    assert np.array_equal(got['mx'].cpu().numpy(), r64['M'].astype(np.float32)), (what, 'M')


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
@pytest.mark.parametrize("mode,kind", CASES)
def test_values_and_gradients_inside_the_gates(mode, kind, shape):
    tensors, r64, _ = case(shape, kind, mode)
    got = run_abi(tensors, mode)
    check_case(shape, kind, mode, got)
    if kind == 'integer' and mode == 'sum':                    # integer shares of integers: exact in every format
        assert np.array_equal(got['out'].cpu().numpy(), r64['out'].astype(np.float32))
    if mode != 'soft':
        assert not got['g_metric'].any() and not got['mx'].any()


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_two_runs_of_collide_are_bit_identical(shape):
    tensors, r64, _ = case(shape, 'collide', 'soft')
    assert r64['hit'].sum() <= 3 * 4 * shape[0]                # every source lands on one of three targets per sample
    a, b = run_abi(tensors, 'soft'), run_abi(tensors, 'soft')
    assert same_bits(a.values(), b.values())


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[0] == 2], ids=ids)
@pytest.mark.parametrize("mode", R.MODES)
def test_a_batch_of_two_equals_its_samples_run_alone(mode, shape):
    tensors = case(shape, 'fractional', mode)[0]
    both = run_abi(tensors, mode)
    for n in range(2):
        alone = run_abi(tuple(t[n:n + 1].contiguous() for t in tensors), mode)
        assert same_bits([v[n:n + 1] for v in both.values()], alone.values()), n


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_nonfinite_sources_equal_sources_moved_out_of_the_frame(shape):
    (x, flow, metric, gout), _, _ = case(shape, 'nonfinite', 'soft')
    bad = R.corrupted('nonfinite', shape)
    assert bad.any()
    flow2, metric2 = flow.clone(), metric.clone()
    flow2[:, 0][bad], flow2[:, 1][bad], metric2[:, 0][bad] = 3.0 * shape[3], 0.0, 0.0
    got, moved = run_abi((x, flow, metric, gout), 'soft'), run_abi((x, flow2, metric2, gout), 'soft')
    assert same_bits(got.values(), moved.values())
    for name, c in (('g_x', shape[1]), ('g_flow', 2), ('g_metric', 1)):
        assert not got[name].cpu()[bad.unsqueeze(1).expand(-1, c, -1, -1)].any(), name      # exactly zero


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_shifted_metric_is_within_the_gate_of_fractional(shape):
    tensors = case(shape, 'shifted', 'soft')[0]
    assert float(tensors[2].min()) > 980 and not torch.isfinite(torch.exp(tensors[2])).any()      # the published form overflows here
    got = run_abi(tensors, 'soft')
    _, r64, r32 = case(shape, 'fractional', 'soft')
    for name in NAMES:
        gate_check('%s/shifted-vs-fractional/soft' % ids(shape), name, got[name], r32[name], r64[name])


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_wide_metric_is_finite_and_reproducible(shape):
    tensors = R.inputs('wide', shape)
    assert float(tensors[2].max() - tensors[2].min()) > 300 or shape == R.SHAPES[0]
    a, b = run_abi(tensors, 'soft'), run_abi(tensors, 'soft')
    assert all(bool(torch.isfinite(v).all()) for v in a.values())
    assert same_bits(a.values(), b.values())
    ref = R.softsplat(*tensors[:3], 'soft')
    assert np.array_equal(a['hit'].cpu().numpy(), ref['hit'].astype(np.float32))


@pytest.mark.parametrize("shape", R.SHAPES[1:], ids=ids)
@pytest.mark.parametrize("mode", R.MODES)
def test_a_hole_has_zero_output_and_sources_that_left_have_zero_gradients(mode, shape):
    tensors, r64, _ = case(shape, 'leave', mode)
    got = run_abi(tensors, mode)
    hole = got['hit'].cpu() == 0
    assert hole.any() and not hole.all()
    assert not got['out'].cpu()[hole.expand(-1, shape[1], -1, -1)].any() and not got['den'].cpu()[hole].any()
    left = (tensors[1][:, 0:1] > shape[3])                     # the sources that were sent out of the frame
    assert left.any()
    for name, c in (('g_x', shape[1]), ('g_flow', 2), ('g_metric', 1)):
        assert not got[name].cpu()[left.expand(-1, c, -1, -1)].any(), name


def test_a_nonfinite_element_of_x_makes_its_whole_sample_nan():
    shape = (2, 3, 7, 9)
    x, flow, metric, gout = case(shape, 'fractional', 'soft')[0]
    clean = run_abi((x, flow, metric, gout), 'soft', want=(False, False, False))
    for value in (float('inf'), NAN):
        x2 = x.clone()
        x2[1, 2, 3, 4] = value
        got = run_abi((x2, flow, metric, gout), 'soft', want=(False, False, False))
        assert bool(torch.isnan(got['out'][1]).all()) and torch.equal(bits(got['out'][0]), bits(clean['out'][0]))
        assert same_bits([got[k] for k in ('hit', 'den', 'mx')], [clean[k] for k in ('hit', 'den', 'mx')])


def op_run(tensors, mode, needs=(True, True, True)):
    """hip_ops.softsplat and autograd.grad on device copies -> out, hit, g_x, g_flow, g_metric (None where not asked for / not read)"""
    x, flow, metric, gout = (t.cuda() for t in tensors)
    leaves = [t.clone().requires_grad_(k) for t, k in zip((x, flow, metric), needs)]
    out, hit = hip_ops.softsplat(leaves[0], leaves[1], leaves[2] if mode == 'soft' else None, mode, return_hit=True)
    assert not hit.requires_grad
    wanted = [t for t, k in zip(leaves, needs) if k and (mode == 'soft' or t is not leaves[2])]
    grads = iter(torch.autograd.grad(out, wanted, gout))
    return [out.detach(), hit] + [next(grads) if (k and (mode == 'soft' or i < 2)) else None for i, k in enumerate(needs)]


@pytest.mark.parametrize("shape", [R.SHAPES[1], R.SHAPES[3]], ids=ids)
@pytest.mark.parametrize("mode", R.MODES)
def test_autograd_equals_the_abi_and_gradient_outputs_may_be_null(mode, shape):
    tensors = case(shape, 'fractional', mode)[0]
    full = run_abi(tensors, mode)
    want = [full[k] for k in ('out', 'hit', 'g_x', 'g_flow', 'g_metric')]
    with record_launches() as rec:
        got = op_run(tensors, mode)
    if mode != 'soft':
        want[4] = None
    assert same_bits(got, want)
    x = tensors[0]
    assert [(l[0], l[1]) for l in rec.launches] == [("softsplat_fwd", hip_ops.softsplat_bytes(x, mode)),
                                                    ("softsplat_bwd", hip_ops.softsplat_bytes(x, mode, 3 if mode == 'soft' else 2))]
    # every subset of the three gradients: the same bits from the C entry and from autograd
    fwd = (full['out'], full['den'], full['mx'])
    for sub in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)):
        part = run_abi(tensors, mode, want=tuple(map(bool, sub)), fwd=fwd)
        for k, name in zip(sub, ('g_x', 'g_flow', 'g_metric')):
            assert (part[name] is None) == (not k) and (part[name] is None or torch.equal(bits(part[name]), bits(full[name])))
        if mode == 'soft' or any(sub[:2]):
            got = op_run(tensors, mode, needs=tuple(map(bool, sub)))
            for k, g, name in zip(sub, got[2:], ('g_x', 'g_flow', 'g_metric')):
                assert g is None or torch.equal(bits(g), bits(full[name])), (sub, name)


@pytest.mark.parametrize("mode", ['soft', 'avg'])
def test_eager_equals_a_graph_replay(mode):
    shape = (2, 3, 7, 9)
    first, second = case(shape, 'fractional', mode)[0], case(shape, 'collide', mode)[0]
    eager = [op_run(t, mode) for t in (first, second, first)]
    static = [t.cuda().clone() for t in first]
    leaves = [t.requires_grad_() for t in static[:3]]
    wanted = leaves if mode == 'soft' else leaves[:2]

    def step():
        out, hit = hip_ops.softsplat(leaves[0], leaves[1], leaves[2] if mode == 'soft' else None, mode, return_hit=True)
        return [out, hit] + list(torch.autograd.grad(out, wanted, static[3]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for tensors, want in zip((first, second, first), eager):      # three replays: the accumulators are cleared by the op's own kernel
        with torch.no_grad():
            for dst, src in zip(static, tensors):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits([t.detach() for t in held], [w for w in want if w is not None])


def test_second_order_passes_take_the_composed_op():
    shape = (2, 3, 7, 9)
    tensors, r64, r32 = case(shape, 'fractional', 'soft')
    x, flow, metric, gout = (t.cuda() for t in tensors)
    hip_ops.set_double_backward(True)
    try:
        leaves = [t.clone().requires_grad_() for t in (x, flow, metric)]
        out = hip_ops.softsplat(*leaves)
        grads = torch.autograd.grad(out, leaves, gout, create_graph=True)
        assert all(g.requires_grad for g in grads)                 # the gradients carry a graph
    finally:
        hip_ops.set_double_backward(False)
    # the composition is float32 throughout and adds in arrival order: not held to the counted gates.  With D >= 2^-8 a float32 rounding
    # of D or of a numerator is amplified at most 256-fold: 256 * 2^-24 * a handful of operations stays below 1e-4 of the scale
    for name, t in zip(NAMES, (out,) + grads):
        err = float(np.abs(t.detach().cpu().numpy().astype(np.float64) - r64[name]).max())
        print('SOFTSPLAT_COMPOSED tensor=%s err=%.3e scale=%.3e' % (name, err, np.abs(r64[name]).max()))
        assert err <= 1e-4 * np.abs(r64[name]).max(), name
