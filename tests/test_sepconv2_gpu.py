"""-m gpu: SepConv's second backward -- savfi_sepconv_bwd2_f32 (csrc/sepconv_bwd2.hip) through the C ABI and FunctionSepconvTwice through
autograd -- against the float64 restatement of tests/sepconv2_ref.py on identical seeded inputs."""
import functools
import math

import pytest
import torch

from meta_interpolation_amd import _hip
from meta_interpolation_amd.sepconv.sepconv_op.sepconv import FunctionSepconv, FunctionSepconvTwice
from tests import sepconv2_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the shapes of SEPCONV_CASES in tests/test_hip_ops_gpu.py without its 128 x 128: the K = 51 fast path, ragged in both directions with
# batch > 1, C = 1, small K, C = 4 with K = 3, the smallest possible, K = 13
CASES = [(1, 3, 16, 32, 51), (2, 3, 37, 45, 51), (1, 1, 9, 70, 51), (1, 3, 7, 5, 5), (2, 4, 10, 33, 3), (1, 2, 1, 1, 1), (1, 3, 20, 20, 13)]
ABI_CASE = (1, 3, 19, 41, 51)
OUTPUTS = ("d_gO", "dV", "dH")


@functools.lru_cache(maxsize=None)
def _case(B, C, Ho, Wo, K):
    """inputs, the float64 restatement and the same loops in fp32 -- computed once per shape, never modified"""
    t = R.bwd2_inputs(B, C, Ho, Wo, K, seed=B * 1000 + Ho * 10 + K)
    return t, R.sepconv_bwd2_f64(*t), R.sepconv_bwd2_f64(*t, dtype=torch.float32)


def gate(ref64, ref32):
    """max error over max|ref|: the project's bound for these sums (tests/test_hip_ops_gpu.py:51) or 3 x the reference's own fp32 error"""
    return max(1e-5, 3 * R.rel(ref32, ref64))


def bwd2(inp, v, h, gO, ggV, ggH, want=(True, True, True), outs=None):
    """one call of the entry point on device tensors (None = NULL); returns (d_gO, dV, dH), None where not wanted"""
    B, C, Ho, Wo = gO.shape
    K = v.shape[1]
    if outs is None:
        outs = [torch.full_like(t, float('nan')) if w else None for t, w in zip((gO, v, h), want)]
    p = lambda t: None if t is None else t.data_ptr()
    _hip.check(_hip.lib().savfi_sepconv_bwd2_f32(p(inp), p(v), p(h), p(gO), p(ggV), p(ggH), *(p(o) for o in outs), B, C, Ho, Wo, K,
                                                 _hip.current_stream()), "savfi_sepconv_bwd2_f32")
    return outs


def measure(case):
    """{output: (error ratio, gate)} of the entry point on a case"""
    t, ref64, ref32 = _case(*case)
    got = bwd2(*(x.to(DEV) for x in t))
    torch.cuda.synchronize()
    return {n: (R.rel(g.cpu(), r64), gate(r64, r32)) for n, g, r64, r32 in zip(OUTPUTS, got, ref64, ref32)}


@pytest.mark.parametrize("B,C,Ho,Wo,K", CASES)
def test_entry_point_against_the_restatement(B, C, Ho, Wo, K):
    res = measure((B, C, Ho, Wo, K))
    for n, (err, bound) in res.items():
        print("%s %s: max err / max|ref| %.3e (gate %.3e)" % ((B, C, Ho, Wo, K), n, err, bound))
    for n, (err, bound) in res.items():
        assert err <= bound, (n, err, bound)


def test_outputs_between_canaries_and_null_subsets():
    t, ref64, ref32 = _case(*ABI_CASE)
    dt = [x.to(DEV) for x in t]
    inp, v, h, gO, ggV, ggH = dt
    PAD, CANARY = 1024, 12345.0

    def guarded(like):
        buf = torch.full((like.numel() + 2 * PAD,), float('nan'), device=DEV)
        buf[:PAD] = CANARY
        buf[-PAD:] = CANARY
        return buf, buf[PAD:PAD + like.numel()].view(like.shape)

    bufs, outs = zip(*[guarded(x) for x in (gO, v, h)])
    bwd2(*dt, outs=list(outs))
    torch.cuda.synchronize()
    for n, buf, out, r64, r32 in zip(OUTPUTS, bufs, outs, ref64, ref32):
        assert torch.equal(buf[:PAD], torch.full((PAD,), CANARY, device=DEV)) and torch.equal(buf[-PAD:], torch.full((PAD,), CANARY, device=DEV)), n
        assert not torch.isnan(out).any(), n
        assert R.rel(out.cpu(), r64) <= gate(r64, r32), n
    full_g, full_v, full_h = outs
    # each NULL subset is the corresponding part of the full call, bit for bit
    only_g, _, _ = bwd2(*dt, want=(True, False, False))
    assert torch.equal(only_g, full_g)
    g_h, dv_h, none = bwd2(inp, v, h, gO, None, ggH, want=(True, True, False))
    assert none is None and torch.equal(dv_h, full_v)
    g_v, none, dh_v = bwd2(inp, v, h, gO, ggV, None, want=(True, False, True))
    assert none is None and torch.equal(dh_v, full_h)
    # ... and an absent cotangent is a zero one
    zero = torch.zeros_like(ggV)
    assert torch.equal(g_h, bwd2(inp, v, h, gO, zero, ggH)[0])
    assert torch.equal(g_v, bwd2(inp, v, h, gO, ggV, zero)[0])
    _, only_v, _ = bwd2(*dt, want=(False, True, False))
    _, _, only_h = bwd2(*dt, want=(False, False, True))
    assert torch.equal(only_v, full_v) and torch.equal(only_h, full_h)


@pytest.mark.parametrize("case", [ABI_CASE, (2, 4, 10, 33, 3)])
def test_reproducible_and_capturable(case):
    t, _, _ = _case(*case)
    dt = [x.to(DEV) for x in t]
    first = bwd2(*dt)
    second = bwd2(*dt)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    outs = [torch.full_like(x, float('nan')) for x in (dt[3], dt[1], dt[2])]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bwd2(*dt, outs=outs)
    for o in outs:
        o.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def _leaves(case, need=(True, True)):
    t, ref64, ref32 = _case(*case)
    inp, v, h, gO, ggV, ggH = (x.to(DEV) for x in t)
    return inp, v.requires_grad_(need[0]), h.requires_grad_(need[1]), gO.requires_grad_(), ggV, ggH, ref64, ref32


@pytest.mark.parametrize("case", [(2, 3, 37, 45, 51), (1, 3, 16, 32, 51), (1, 3, 7, 5, 5)])
def test_first_order_is_function_sepconv_bit_for_bit(case):
    inp, v, h, gO, _, _, _, _ = _leaves(case)
    out1 = FunctionSepconv.apply(inp, v, h)
    gv1, gh1 = torch.autograd.grad(out1, (v, h), gO.detach())
    out2 = FunctionSepconvTwice.apply(inp, v, h)
    gv2, gh2 = torch.autograd.grad(out2, (v, h), gO.detach())
    assert torch.equal(out1, out2) and torch.equal(gv1, gv2) and torch.equal(gh1, gh2)
    for need in ((True, False), (False, True)):
        _, v1, h1, _, _, _, _, _ = _leaves(case, need)
        x = v1 if need[0] else h1
        (a,) = torch.autograd.grad(FunctionSepconv.apply(inp, v1, h1), x, gO.detach())
        (b,) = torch.autograd.grad(FunctionSepconvTwice.apply(inp, v1, h1), x, gO.detach())
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [(2, 3, 37, 45, 51), (1, 3, 7, 5, 5)])
def test_double_backward_matches_the_restatement(case):
    inp, v, h, gO, ggV, ggH, ref64, ref32 = _leaves(case)
    out = FunctionSepconvTwice.apply(inp, v, h)
    gV, gH = torch.autograd.grad(out, (v, h), gO, create_graph=True)
    assert gV.requires_grad and gH.requires_grad
    s = (gV * ggV).sum() + (gH * ggH).sum()
    d_gO, dV, dH = torch.autograd.grad(s, (gO, v, h), create_graph=True)
    for n, g, r64, r32 in zip(OUTPUTS, (d_gO, dV, dH), ref64, ref32):
        assert R.rel(g.detach().cpu(), r64) <= gate(r64, r32), n
    # a third derivative raises; it never drops terms
    with pytest.raises(RuntimeError):
        torch.autograd.grad(dV.sum(), h)


def test_plain_function_sepconv_still_hands_out_graphless_gradients():
    inp, v, h, gO, _, _, _, _ = _leaves((1, 3, 7, 5, 5))
    gV, gH = torch.autograd.grad(FunctionSepconv.apply(inp, v, h), (v, h), gO, create_graph=True)
    assert not gV.requires_grad and not gH.requires_grad and gV.grad_fn is None and gH.grad_fn is None


def test_frame_with_gradient_is_refused():
    inp, v, h, _, _, _, _, _ = _leaves((1, 3, 7, 5, 5))
    with pytest.raises(NotImplementedError, match="second-order"):
        FunctionSepconvTwice.apply(inp.requires_grad_(), v, h)


def test_only_v_requires_grad():
    case = (1, 3, 16, 32, 51)
    inp, v, h, gO, ggV, _, _, _ = _leaves(case, need=(True, False))
    t = _case(*case)[0]
    want64 = R.sepconv_bwd2_f64(t[0], t[1], t[2], t[3], t[4], None)
    want32 = R.sepconv_bwd2_f64(t[0], t[1], t[2], t[3], t[4], None, dtype=torch.float32)
    out = FunctionSepconvTwice.apply(inp, v, h)
    (gV,) = torch.autograd.grad(out, v, gO, create_graph=True)
    d_gO, dV = torch.autograd.grad((gV * ggV).sum(), (gO, v), allow_unused=True)
    # gH was never computed, so ggH is absent: d_gO = sep(in, ggV, h), and dV -- whose only term needs ggH -- is no gradient at all
    assert R.rel(d_gO.cpu(), want64[0]) <= gate(want64[0], want32[0])
    assert dV is None and want64[1] is None
