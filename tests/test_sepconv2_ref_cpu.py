"""The float64 restatement of SepConv's second backward (tests/sepconv2_ref.py) against double autograd through the oracle's
differentiable op, the stored second-order system fixture against the properties its generator asserts, and the flag."""
import pytest
import torch

from meta_interpolation_amd import config
from meta_interpolation_amd.config import default_args
from oracle import torch_ops as O
from tests import sepconv2_ref as R
from tests.helpers import golden

CASES = [(2, 3, 5, 7, 5), (1, 2, 1, 1, 1), (1, 3, 6, 9, 13)]


def _double_autograd(inp, v, h, gO, ggV, ggH):
    """d_gO, dV, dH by differentiating <gV, ggV> + <gH, ggH> of a create_graph=True backward, all in float64"""
    inp, v, h, gO = inp.double(), v.double().requires_grad_(), h.double().requires_grad_(), gO.double().requires_grad_()
    out = O.sepconv_torch(inp, v, h)
    gV, gH = torch.autograd.grad(out, (v, h), gO, create_graph=True)
    s = 0
    if ggV is not None:
        s = s + (gV * ggV.double()).sum()
    if ggH is not None:
        s = s + (gH * ggH.double()).sum()
    return torch.autograd.grad(s, (gO, v, h), allow_unused=True)


@pytest.mark.parametrize("B,C,Ho,Wo,K", CASES)
@pytest.mark.parametrize("drop", [None, "ggV", "ggH"])
def test_restatement_equals_double_autograd(B, C, Ho, Wo, K, drop):
    inp, v, h, gO, ggV, ggH = R.bwd2_inputs(B, C, Ho, Wo, K, seed=B * 1000 + Ho * 10 + K)
    if drop == "ggV":
        ggV = None
    if drop == "ggH":
        ggH = None
    want = _double_autograd(inp, v, h, gO, ggV, ggH)
    got = R.sepconv_bwd2_f64(inp, v, h, gO, ggV, ggH, rows=2)
    for name, g, w in zip(("d_gO", "dV", "dH"), got, want):
        if g is None:                      # dV without ggH / dH without ggV: identically zero
            assert w is None or w.abs().max().item() == 0.0, name
            continue
        assert g.dtype == torch.float64
        assert (g - w).abs().max().item() <= 1e-12 * w.abs().max().item(), (name, drop)


def test_restatement_in_float32_is_the_same_loops():
    inp, v, h, gO, ggV, ggH = R.bwd2_inputs(1, 3, 6, 9, 13, seed=5)
    ref = R.sepconv_bwd2_f64(inp, v, h, gO, ggV, ggH)
    got = R.sepconv_bwd2_f64(inp, v, h, gO, ggV, ggH, dtype=torch.float32)
    for g, w in zip(got, ref):
        assert g.dtype == torch.float32 and R.rel(g, w) < 1e-5


def test_fixture_holds_what_its_generator_asserted():
    R.check_fixture(golden(R.FIXTURE))


def test_flag_parses_and_defaults_to_zero():
    parser = config.build_parser()
    assert parser.parse_args([]).sepconv_second_order == 0
    assert parser.parse_args(['--sepconv_second_order', '1']).sepconv_second_order == 1
    with pytest.raises(SystemExit):
        parser.parse_args(['--sepconv_second_order', '2'])
    assert default_args().sepconv_second_order == 0
    assert default_args(sepconv_second_order=1).sepconv_second_order == 1
    assert 'sepconv_second_order' in config.__doc__
