"""GPU: the small-map 3 x 3 weight gradient (csrc/convk_wgrad.hip, convk_wgrad3_small) through its own entry points against float64.

Reference: torch.nn.grad.conv2d_weight in double on the CPU, per filter set n % T, and the sums of the cotangent for the bias gradient.
Gate: the local bound of tests/conv_ref.py with the constants tests/test_conv_layers_gpu.py holds the split-bf16 weight-gradient family
and the bias sums to (the arithmetic is that family's: 3-way bf16 splits, six products, fp32 accumulation).  Every case runs twice and
the two results must be equal bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
C_WGRAD = 4 * 4.89          # tests/test_conv_layers_gpu.py: C_FAMILY["convk_wgrad"]
C_BIAS = 4 * 0.64           # ... and C_FAMILY["bias"]

# (N, T, Ci, Co, H, W, pad)
CASES = [
    (2, 1, 64, 64, 12, 16, 1),          # two bands, two rows per K-step
    (4, 2, 64, 128, 24, 32, 1),         # six bands, T > 1
    (2, 2, 80, 72, 12, 16, 1),          # channel blocks padded by the loads
    (2, 1, 64, 64, 5, 7, 1),            # odd map, pixel padding to 32
    (2, 1, 64, 64, 12, 16, 0),          # pad 0
    (1, 1, 64, 64, 1, 1, 1),            # smallest map
    (8, 4, 512, 512, 12, 16, 1),        # 256 blocks: the direct-write path with no reduction
]


def _run(x, gz, N, T, Ci, Co, H, W, pad, bias):
    lib = _hip.lib()
    floats = lib.savfi_convk_wgrad3_small_workspace_floats(N, T, Ci, Co, H, W, pad)
    assert floats >= 0, floats
    ws = torch.full((max(int(floats), 4),), float("nan"), device=DEV)
    gw = torch.full((T, Co, Ci, 3, 3), float("nan"), device=DEV)
    if not bias:
        _hip.call("wgrad_small", "savfi_convk_wgrad3_small_tasks_f32", x, gz, gw, ws, N, T, Ci, Co, H, W, pad)
        torch.cuda.synchronize()
        return gw, None
    gb = torch.full((T, Co), float("nan"), device=DEV)
    _hip.call("wgrad_small", "savfi_convk_wgrad3_small_tasks_bias_f32", x, gz, gw, gb, ws, N, T, Ci, Co, H, W, pad)
    torch.cuda.synchronize()
    return gw, gb


@pytest.mark.parametrize("case", CASES, ids=["n%dt%d_%dto%d_%dx%d_p%d" % c for c in CASES])
def test_small_map_wgrad_matches_float64(case):
    N, T, Ci, Co, H, W, pad = case
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    g = torch.Generator(device=DEV).manual_seed(CASES.index(case))
    x = torch.randn((N, Ci, H, W), device=DEV, generator=g)
    gz = torch.randn((N, Co, Ho, Wo), device=DEV, generator=g)
    gw, gb = _run(x, gz, N, T, Ci, Co, H, W, pad, True)
    gw2, gb2 = _run(x, gz, N, T, Ci, Co, H, W, pad, True)
    gw3, _ = _run(x, gz, N, T, Ci, Co, H, W, pad, False)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2), "two runs differ"
    assert torch.equal(gw, gw3), "the entry without the bias sums gives another weight gradient"
    xd, gd = x.double().cpu(), gz.double().cpu()
    for t in range(T):
        xs, gs = xd[t::T], gd[t::T]
        ref = torch.nn.grad.conv2d_weight(xs, (Co, Ci, 3, 3), gs, padding=pad)
        mag = torch.nn.grad.conv2d_weight(xs.abs(), (Co, Ci, 3, 3), gs.abs(), padding=pad)
        r = R.local_ratio(gw[t].cpu(), ref, mag)
        rb = R.local_ratio(gb[t].cpu(), gs.sum((0, 2, 3)), gs.abs().sum((0, 2, 3)))
        print("case %s task %d: weight gradient %.3g x 2^-24 L (gate %g), bias gradient %.3g (gate %g)" % (case, t, r, C_WGRAD, rb, C_BIAS))
        assert r <= C_WGRAD, "weight gradient task %d: |got - ref| reaches %.3g x 2^-24 L (gate %g)" % (t, r, C_WGRAD)
        assert rb <= C_BIAS, "bias gradient task %d: |got - ref| reaches %.3g x 2^-24 L (gate %g)" % (t, rb, C_BIAS)
