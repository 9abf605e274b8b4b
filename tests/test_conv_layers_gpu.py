"""-m gpu: the benchmark's convolution layers, at their production shapes, through the routed entry points against float64.

The geometries are the distinct convolution launches of profiles/r06_layer_table_c2.txt (SepConv), _c3.txt (VoxelFlow) and _c5.txt
(CAIN): samples N, tasks T, channels, input map, kernel size, padding, and the kernel family each direction ran on.  Every layer runs
hip_ops.conv_bias_act_tasks (T > 1) or hip_ops.conv_bias_act (T = 1) forward and its autograd backward -- with the conv -> ReLU -> conv
chain fold (`in_slope`: the producer's ReLU derivative applied in this layer's data-gradient epilogue) where the model has one -- and
the launches are captured to assert that each direction ran the family the table names.

Forward and data gradient are compared with float64 on windows of 24 x 24 pixels, all channels: the four corners, the last (ragged) tile
block at the right and at the bottom, a window across a tile-block boundary of the F(4x4) plan, two random interior windows; each window
on one of the samples 0, T - 1, N - 1 and a random one.  The weight and bias gradients are compared on the full map and every sample of
each task, output channels {0, 31, 32, Co - 1} x input channels {0, 7, 8, Ci - 1} (the COB = 32 / KC = 8 block edges).  Gate: the local
bound of tests/conv_ref.py, with one constant per kernel family measured on an MI355X over these layers, tests/test_conv_variants_gpu.py
and seeds 0, 1, 2 (c_family = 4 x the measured maximum):  convk (forward / data gradient) 6.09, convk_wgrad 4.89, conv3x3_wgrad (the
Winograd weight gradient) 5.02, the bias gradient (wherever it is summed) 0.64; F(4x4) 63.3 and F(2x2) 1.78: tests/test_conv_variants_gpu.py."""
import random

import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops
from tests import conv_ref as R
from tests import test_conv_variants_gpu as V

pytestmark = pytest.mark.gpu

DEV = "cuda"

MEASURED_CONVK = 6.09
MEASURED_CONVK_WGRAD = 4.89
MEASURED_WINO_WGRAD = 5.02
MEASURED_BIAS = 0.64
C_FAMILY = {"convk": 4 * MEASURED_CONVK, "convk_wgrad": 4 * MEASURED_CONVK_WGRAD, "conv3x3_wgrad": 4 * MEASURED_WINO_WGRAD,
            "bias": 4 * MEASURED_BIAS}
POOLED = {"conv3x3f4": "f4", "conv3x3": "f2"}

# (table, N, T, Ci, Co, H, W, K, pad, forward, data gradient (None: the model asks for none), weight gradient, chain, mirrored border)
# H x W: the map the convolution reads; `mirrored`: it is the reflection-padded map of the layer before (CAIN's RCAB), read with pad 0
LAYERS = [
    ("c2", 16, 4, 51, 51, 258, 450, 3, 0, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 16, 4, 64, 51, 137, 236, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 16, 4, 64, 64, 137, 236, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 4, 1, 64, 256, 137, 236, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 6, 32, 384, 512, 3, 1, "convk", None, "convk_wgrad", False, False),
    ("c2", 8, 4, 32, 32, 384, 512, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 32, 64, 192, 256, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 64, 64, 192, 256, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 4, 1, 64, 64, 192, 256, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 64, 128, 96, 128, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 128, 128, 96, 128, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 4, 1, 128, 128, 96, 128, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 128, 64, 96, 128, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 64, 64, 96, 128, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 4, 4, 128, 128, 48, 64, 3, 1, "convk", "convk", "convk_wgrad", True, False),
    ("c2", 8, 4, 128, 128, 48, 64, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 128, 256, 48, 64, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 256, 128, 48, 64, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c2", 8, 4, 256, 256, 48, 64, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 4, 1, 256, 256, 48, 64, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 256, 256, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "conv3x3_wgrad", True, False),
    ("c2", 4, 4, 256, 256, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, False),
    ("c2", 8, 4, 256, 512, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "conv3x3_wgrad", False, False),
    ("c2", 8, 4, 512, 256, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "conv3x3_wgrad", False, False),
    ("c2", 8, 4, 512, 512, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "conv3x3_wgrad", True, False),
    ("c2", 4, 1, 512, 512, 24, 32, 3, 1, "conv3x3f4", "conv3x3f4", "conv3x3_wgrad", True, False),
    ("c2", 8, 4, 512, 512, 12, 16, 3, 1, "conv3x3", "conv3x3", "conv3x3_wgrad", True, False),
    ("c2", 4, 4, 512, 512, 12, 16, 3, 1, "conv3x3", "conv3x3", "convk_wgrad", True, False),
    ("c3", 16, 8, 6, 64, 256, 256, 5, 2, "convk", None, "convk_wgrad", False, False),
    ("c3", 16, 8, 192, 64, 256, 256, 5, 2, "convk", "convk", "convk_wgrad", False, False),
    ("c3", 16, 8, 64, 128, 128, 128, 5, 2, "convk", "convk", "convk_wgrad", False, False),
    ("c3", 16, 8, 384, 128, 128, 128, 5, 2, "convk", "convk", "convk_wgrad", False, False),
    ("c3", 16, 8, 64, 3, 256, 256, 5, 2, "convk", "convk", "convk_wgrad", False, False),
    ("c3", 16, 8, 128, 256, 64, 64, 3, 1, "convk", "convk", "convk_wgrad", False, False),
    ("c3", 16, 8, 256, 256, 32, 32, 3, 1, "convk", "convk", "convk_wgrad", True, False),
    ("c3", 16, 8, 512, 256, 64, 64, 3, 1, "convk", "convk", "convk_wgrad", False, False),
    ("c5", 2, 1, 192, 192, 98, 162, 3, 0, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, True),
    ("c5", 1, 1, 192, 192, 98, 162, 3, 0, "conv3x3f4", "conv3x3f4", "convk_wgrad", True, True),
    ("c5", 2, 1, 192, 192, 96, 160, 3, 1, "conv3x3f4", "conv3x3f4", "convk_wgrad", False, False),
    ("c5", 2, 1, 384, 192, 96, 160, 3, 1, "conv3x3f4", None, "convk_wgrad", False, False),
]
WIN = 24


def _id(layer):
    tb, N, T, Ci, Co, H, W, K, pad, *_ = layer
    return "%s-%dx%d-%d->%d-T%d-N%d-%dx%d-p%d" % (tb, K, K, Ci, Co, T, N, H, W, pad)


def _crop(t, n, y0, y1, x0, x1):
    """t[n:n+1, :, y0:y1, x0:x1] in float64 on the CPU, zeros outside the map"""
    H, W = t.shape[2:]
    ya, yb, xa, xb = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    c = t[n:n + 1, :, ya:yb, xa:xb].double().cpu()
    return F.pad(c, (xa - x0, x1 - xb, ya - y0, y1 - yb))


def _windows(Ho, Wo, block, rnd):
    """(y0, x0) of the WIN x WIN windows (clamped to the map): corners, the last tile block at the right / bottom, a block boundary,
    two random interior windows"""
    bh, bw = block
    wy, wx = min(WIN, Ho), min(WIN, Wo)
    last_y, last_x = (Ho - 1) // bh * bh, (Wo - 1) // bw * bw
    pts = [(0, 0), (0, Wo - wx), (Ho - wy, 0), (Ho - wy, Wo - wx), (last_y, Wo - wx), (Ho - wy, last_x),
           (bh - wy // 2, bw - wx // 2), (rnd.randrange(Ho), rnd.randrange(Wo)), (rnd.randrange(Ho), rnd.randrange(Wo))]
    return [(min(max(y, 0), Ho - wy), min(max(x, 0), Wo - wx), wy, wx) for y, x in pts]


def _check_windows(what, family, out, src, w, b, K, pad, T, samples, windows, mode, slope=1.0, gate_mask=None, in_slope=None):
    """out: the GPU result [N, I, Ho, Wo]; src: what it was computed from (forward: x, data gradient: gz), w [T, Co, Ci, K, K]"""
    pooled = family in POOLED
    fam = POOLED.get(family, family)
    Ho, Wo = out.shape[2:]
    for i, (y0, x0, wy, wx) in enumerate(windows):
        n = samples[i % len(samples)]
        t = n % T
        e = 3 if pooled else 0          # the pooled magnitude needs the 3 pixels around the window (inside the map)
        ey0, ey1, ex0, ex1 = max(y0 - e, 0), min(y0 + wy + e, Ho), max(x0 - e, 0), min(x0 + wx + e, Wo)
        if mode == 0:
            xc = _crop(src, n, ey0 - pad, ey1 - pad + K - 1, ex0 - pad, ex1 - pad + K - 1)
            wt, bt = w[t].double().cpu(), b[t].double().cpu()
            ref = R.act(F.conv2d(xc, wt, bt), slope)
            mag = F.conv2d(xc.abs(), wt.abs(), bt.abs())
        else:
            q = K - 1 - pad
            gc = _crop(src, n, ey0 - q, ey1 + pad, ex0 - q, ex1 + pad)
            wt = w[t].double().cpu().flip(-1, -2).transpose(0, 1)
            ref = F.conv2d(gc, wt)
            mag = F.conv2d(gc.abs(), wt.abs())
            if gate_mask is not None:
                ref = ref * R.mask_factor(_crop(gate_mask, n, ey0, ey1, ex0, ex1), in_slope)
        if pooled:
            mag = R.pool7(mag)
        sl = (slice(None), slice(None), slice(y0 - ey0, y0 - ey0 + wy), slice(x0 - ex0, x0 - ex0 + wx))
        got = out[n:n + 1, :, y0:y0 + wy, x0:x0 + wx].cpu()
        R.assert_local(got, ref[sl], mag[sl], C_FAMILY[fam] if fam in C_FAMILY else (V.C_F4 if fam == "f4" else V.C_F2), fam,
                       "%s n=%d window (%d, %d)" % (what, n, y0, x0))


@pytest.mark.parametrize("layer", LAYERS, ids=[_id(l) for l in LAYERS])
def test_production_layer_matches_float64(layer, monkeypatch):
    tb, N, T, Ci, Co, H, W, K, pad, fwd_family, dgrad_family, wgrad_family, chain, mirrored = layer
    direct = tb == "c3"             # VoxelFlow asks for the direct kernels (Winograd rounding amplified by its warp)
    seed = 1000 * R.SEED_OFFSET + LAYERS.index(layer)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = random.Random(seed)
    slope = 1.0 if Co in (3, 51) else 0.0          # the layers that end a block (SepConv's Subnets, VoxelFlow's output): no activation
    in_slope = 0.0 if chain and dgrad_family else None
    x = torch.randn(N, Ci, H - 2 * mirrored, W - 2 * mirrored, device=DEV, generator=g)
    if chain:
        x = torch.relu(x)           # the activated output of the producer: its ReLU derivative is the mask
    if mirrored:
        x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    wshape = (T, Co, Ci, K, K)
    w = torch.randn(wshape, device=DEV, generator=g) / (K * Ci ** 0.5)
    b = 0.1 * torch.randn(T, Co, device=DEV, generator=g)
    xr = x.clone().requires_grad_(dgrad_family is not None)
    wr, br = (w.clone().requires_grad_(), b.clone().requires_grad_()) if T > 1 else (w[0].clone().requires_grad_(), b[0].clone().requires_grad_())
    names = []
    orig = _hip.launch
    monkeypatch.setattr(_hip, "launch", lambda name, fn, **k: (names.append(name), orig(name, fn, **k))[1])
    if T > 1:
        y = hip_ops.conv_bias_act_tasks(xr, wr, br, 1, pad, 1, slope, direct=direct, in_slope=in_slope)
    else:
        y = hip_ops.conv_bias_act(xr, wr, br, 1, pad, 1, 1, slope, direct=direct, in_slope=in_slope)
    fwd_names = list(names)
    gy = torch.randn(y.shape, device=DEV, generator=g)
    inputs = ([xr] if dgrad_family else []) + [wr, br]
    grads = torch.autograd.grad(y, inputs, gy)
    torch.cuda.synchronize()
    bwd_names = names[len(fwd_names):]
    monkeypatch.setattr(_hip, "launch", orig)
    assert fwd_family + "_fwd" in fwd_names, (fwd_family, fwd_names)
    if dgrad_family:
        assert dgrad_family + "_bwd_data" in bwd_names and not any(n.endswith("_bwd_data") and not n.startswith(dgrad_family + "_b")
                                                                   for n in bwd_names), (dgrad_family, bwd_names)
    assert wgrad_family in bwd_names, (wgrad_family, bwd_names)
    gx = grads[0] if dgrad_family else None
    gw, gb = grads[-2].reshape(wshape), grads[-1].reshape(T, Co)
    y = y.detach()
    gz = gy if slope == 1.0 else gy * R.mask_factor(y, slope)

    Ho, Wo = y.shape[2:]
    plan = R.f4_plan(N, Ci, Co, H, W, pad, 0)
    block = (4 * (32 >> plan["tile_shift"]), 4 * (1 << plan["tile_shift"])) if plan else (32, 32)
    samples = sorted({0, T - 1, N - 1, rnd.randrange(N)})
    _check_windows("forward", fwd_family, y, x, w, b, K, pad, T, samples, _windows(Ho, Wo, block, rnd), 0, slope)
    if dgrad_family:
        plan = R.f4_plan(N, Ci, Co, Ho, Wo, pad, 1)
        block = (4 * (32 >> plan["tile_shift"]), 4 * (1 << plan["tile_shift"])) if plan else (32, 32)
        _check_windows("data gradient", dgrad_family, gx, gz, w, b, K, pad, T, samples, _windows(H, W, block, rnd), 1,
                       gate_mask=x if in_slope is not None else None, in_slope=in_slope)

    # weight and bias gradients: every sample of each task, the channel-block edges
    cos = sorted({c for c in (0, 31, 32, Co - 1) if c < Co})
    cis = sorted({c for c in (0, 7, 8, Ci - 1) if c < Ci})
    for t in range(T):
        S = list(range(t, N, T))
        xs = F.pad(x[S][:, cis].double().cpu(), (pad,) * 4).transpose(0, 1)
        gs = gz[S][:, cos].double().cpu().transpose(0, 1)
        ref = F.conv2d(xs, gs).transpose(0, 1)
        mag = F.conv2d(xs.abs(), gs.abs()).transpose(0, 1)
        got = gw[t][cos][:, cis].cpu()
        R.assert_local(got, ref, mag, C_FAMILY[wgrad_family], wgrad_family, "weight gradient task %d" % t)
        gs = gz[S][:, cos].double().cpu()
        R.assert_local(gb[t][cos].cpu(), gs.sum((0, 2, 3)), gs.abs().sum((0, 2, 3)), C_FAMILY["bias"], "bias", "bias gradient task %d" % t)
