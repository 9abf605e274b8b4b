"""-m gpu: every HIP kernel, called through the C ABI (ctypes -> libsavfi_hip.so), against the CPU
oracle on identical seeded inputs.  Tolerances are stated per test; fp32 everywhere."""
import math

import numpy as np

import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops
from meta_interpolation_amd.sepconv.sepconv_op.sepconv import FunctionSepconv
from oracle import torch_ops as O
from tests.helpers import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _sepconv_inputs(B, C, Ho, Wo, K, seed):
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, C, Ho + K - 1, Wo + K - 1, generator=g)
    v = torch.randn(B, K, Ho, Wo, generator=g) / math.sqrt(K)
    h = torch.randn(B, K, Ho, Wo, generator=g) / math.sqrt(K)
    gO = torch.randn(B, C, Ho, Wo, generator=g)
    return inp, v, h, gO


# shapes: the K=51 fast path with ragged tiles, batch>1, the generic path (K!=51, C!=3), tiny
SEPCONV_CASES = [
    (1, 3, 16, 32, 51), (2, 3, 37, 45, 51), (1, 3, 128, 128, 51), (1, 1, 9, 70, 51),
    (1, 3, 7, 5, 5), (2, 4, 10, 33, 3), (1, 2, 1, 1, 1), (1, 3, 20, 20, 13),
]


@pytest.mark.parametrize("B,C,Ho,Wo,K", SEPCONV_CASES)
def test_sepconv_forward_backward_vs_oracle(B, C, Ho, Wo, K):
    inp, v, h, gO = _sepconv_inputs(B, C, Ho, Wo, K, seed=B * 1000 + Ho * 10 + K)
    ref = O.sepconv_forward_c(inp, v, h)
    rI, rV, rH = O.sepconv_backward_c(inp, v, h, gO, need_input=True)

    di, dv, dh = (t.to(DEV).requires_grad_() for t in (inp, v, h))
    out = FunctionSepconv.apply(di, dv, dh)
    out.backward(gO.to(DEV))
    torch.cuda.synchronize()
    # fp32 sums of K*K (2601) products in a different association: 1e-5 relative to max|ref|
    assert _rel(out.detach().cpu(), ref) < 1e-5
    assert _rel(dv.grad.cpu(), rV) < 1e-5
    assert _rel(dh.grad.cpu(), rH) < 1e-5
    assert _rel(di.grad.cpu(), rI) < 1e-5


def test_sepconv_needs_input_grad_subsets():
    inp, v, h, gO = _sepconv_inputs(1, 3, 24, 40, 51, seed=7)
    _, rV, rH = O.sepconv_backward_c(inp, v, h, gO)
    for need_v, need_h in [(True, False), (False, True)]:
        di = inp.to(DEV)
        dv = v.to(DEV).requires_grad_(need_v)
        dh = h.to(DEV).requires_grad_(need_h)
        FunctionSepconv.apply(di, dv, dh).backward(gO.to(DEV))
        if need_v:
            assert _rel(dv.grad.cpu(), rV) < 1e-5 and dh.grad is None
        else:
            assert _rel(dh.grad.cpu(), rH) < 1e-5 and dv.grad is None


def test_sepconv_full_size_properties():
    """BASELINE config-2 shape (256x448 -> padded 384x512, K=51): oracle parity on the full tensor
    plus size-independent properties (linearity in the input; a delta kernel reproduces a shift)."""
    B, C, Ho, Wo, K = 1, 3, 384, 512, 51
    inp, v, h, gO = _sepconv_inputs(B, C, Ho, Wo, K, seed=99)
    di, dv, dh = inp.to(DEV), v.to(DEV), h.to(DEV)
    out = FunctionSepconv.apply(di, dv, dh)
    ref = O.sepconv_forward_c(inp, v, h)
    assert _rel(out.cpu(), ref) < 1e-5
    # linearity: f(a*x + y) = a*f(x) + f(y)
    inp2 = torch.rand_like(inp).to(DEV)
    lhs = FunctionSepconv.apply(2.5 * di + inp2, dv, dh)
    rhs = 2.5 * out + FunctionSepconv.apply(inp2, dv, dh)
    assert _rel(lhs, rhs) < 1e-5
    # delta taps at (fy0, fx0) -> pure crop/shift of the input, bit exact
    fy0, fx0 = 13, 42
    vd = torch.zeros_like(dv); vd[:, fy0] = 1
    hd = torch.zeros_like(dh); hd[:, fx0] = 1
    shifted = FunctionSepconv.apply(di, vd, hd)
    assert torch.equal(shifted, di[:, :, fy0:fy0 + Ho, fx0:fx0 + Wo])
    # filter gradients at full size
    dv.requires_grad_(); dh.requires_grad_()
    FunctionSepconv.apply(di, dv, dh).backward(gO.to(DEV))
    _, rV, rH = O.sepconv_backward_c(inp, v, h, gO)
    assert _rel(dv.grad.cpu(), rV) < 1e-5
    assert _rel(dh.grad.cpu(), rH) < 1e-5


def test_sepconv_does_not_write_out_of_bounds():
    """Canary-padded outputs around ragged tiles (odd sizes, K=51 halo edges)."""
    B, C, Ho, Wo, K = 1, 3, 19, 41, 51
    inp, v, h, gO = _sepconv_inputs(B, C, Ho, Wo, K, seed=5)
    lib = _hip.lib()
    n_out, n_f = B * C * Ho * Wo, B * K * Ho * Wo
    pad = 4096
    bufs = {k: torch.full((n + 2 * pad,), 7777.0, device=DEV) for k, n in
            dict(out=n_out, gV=n_f, gH=n_f).items()}
    di, dv, dh, dg = inp.to(DEV), v.to(DEV), h.to(DEV), gO.to(DEV)
    st = _hip.current_stream()
    _hip.check(lib.savfi_sepconv_fwd_f32(di.data_ptr(), dv.data_ptr(), dh.data_ptr(),
                                         bufs["out"][pad:].data_ptr(), B, C, Ho, Wo, K, st), "fwd")
    _hip.check(lib.savfi_sepconv_bwd_f32(di.data_ptr(), dv.data_ptr(), dh.data_ptr(), dg.data_ptr(), None,
                                         bufs["gV"][pad:].data_ptr(), bufs["gH"][pad:].data_ptr(),
                                         B, C, Ho, Wo, K, st), "bwd")
    torch.cuda.synchronize()
    for k, n in dict(out=n_out, gV=n_f, gH=n_f).items():
        assert torch.all(bufs[k][:pad] == 7777.0) and torch.all(bufs[k][pad + n:] == 7777.0), k
    assert _rel(bufs["out"][pad:pad + n_out].cpu().view(B, C, Ho, Wo), O.sepconv_forward_c(inp, v, h)) < 1e-5


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 256, 448), (3, 37, 52)])
def test_sepconv_taps_strided_entry_points_equal_the_contiguous_ones(shape):
    """savfi_sepconv_{fwd,bwd}_taps_strided_f32 through the C ABI: v / h (and gV / gH) as slices of one interleaved [B * 4, 51, Ho, Wo]
    buffer (tap_bstride = 4 * 51, the layout sepconv/model.py's batched Subnets leave) give bit for bit what the contiguous entry
    points give on copies of the slices, the planes of the buffer the call does not own stay untouched, and the protocol counter stays
    at zero; shapes the wave-specialised kernels do not take are refused, not mis-computed."""
    B, Ho, Wo = shape
    K, C = 51, 3
    lib, st = _hip.lib(), _hip.current_stream()
    g = torch.Generator().manual_seed(11)
    inp = torch.rand(B, C, Ho + K - 1, Wo + K - 1, generator=g).to(DEV)
    taps = (torch.randn(4 * B, K, Ho, Wo, generator=g) / 7).to(DEV)
    gO = torch.randn(B, C, Ho, Wo, generator=g).to(DEV)
    plane = K * Ho * Wo * 4
    for s in (0, 2):                                  # (v, h) = sub-networks (s, s + 1)
        v, h = taps.view(B, 4, K, Ho, Wo)[:, s].contiguous(), taps.view(B, 4, K, Ho, Wo)[:, s + 1].contiguous()
        out_c, out_s = torch.empty(B, C, Ho, Wo, device=DEV), torch.empty(B, C, Ho, Wo, device=DEV)
        _hip.check(lib.savfi_sepconv_fwd_f32(inp.data_ptr(), v.data_ptr(), h.data_ptr(), out_c.data_ptr(), B, C, Ho, Wo, K, st), "fwd")
        _hip.check(lib.savfi_sepconv_fwd_taps_strided_f32(inp.data_ptr(), taps.data_ptr() + s * plane, taps.data_ptr() + (s + 1) * plane,
                                                          out_s.data_ptr(), B, C, Ho, Wo, K, 4 * K, st), "fwd strided")
        assert torch.equal(out_s, out_c)
        gV, gH = torch.empty_like(v), torch.empty_like(h)
        _hip.check(lib.savfi_sepconv_bwd_f32(inp.data_ptr(), v.data_ptr(), h.data_ptr(), gO.data_ptr(), None, gV.data_ptr(), gH.data_ptr(),
                                             B, C, Ho, Wo, K, st), "bwd")
        gT = torch.full_like(taps, float('nan'))
        _hip.check(lib.savfi_sepconv_bwd_taps_strided_f32(inp.data_ptr(), taps.data_ptr() + s * plane, taps.data_ptr() + (s + 1) * plane,
                                                          gO.data_ptr(), gT.data_ptr() + s * plane, gT.data_ptr() + (s + 1) * plane,
                                                          B, C, Ho, Wo, K, 4 * K, st), "bwd strided")
        gT5 = gT.view(B, 4, K, Ho, Wo)
        assert torch.equal(gT5[:, s], gV) and torch.equal(gT5[:, s + 1], gH)
        other = [k for k in range(4) if k not in (s, s + 1)]
        assert torch.isnan(gT5[:, other]).all()       # the other sub-networks' planes were not written
    assert lib.savfi_sepconv_ws_errors() == 0
    # refused: a width the ws kernels do not take, a stride below K, other K
    args = lambda Wo_, K_, stride: (inp.data_ptr(), taps.data_ptr(), taps.data_ptr(), gO.data_ptr(), B, C, Ho, Wo_, K_, stride, st)
    assert lib.savfi_sepconv_fwd_taps_strided_f32(*args(Wo - 1, K, 4 * K)) == -3
    assert lib.savfi_sepconv_fwd_taps_strided_f32(*args(Wo, K, K - 1)) == -2
    assert lib.savfi_sepconv_fwd_taps_strided_f32(*args(Wo, 25, 100)) == -3


def test_sepconv_argument_errors():
    lib = _hip.lib()
    x = torch.zeros(16, device=DEV)
    st = _hip.current_stream()
    assert lib.savfi_sepconv_fwd_f32(None, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 1, 1, 1, 1, st) == -1
    assert lib.savfi_sepconv_fwd_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 1, 0, 1, 1, st) == -2
    with pytest.raises(NotImplementedError):
        FunctionSepconv.apply(torch.zeros(1, 1, 3, 3), torch.zeros(1, 3, 1, 1), torch.zeros(1, 3, 1, 1))
    with pytest.raises(AssertionError):
        FunctionSepconv.apply(torch.zeros(1, 1, 4, 3, device=DEV), torch.zeros(1, 3, 1, 1, device=DEV),
                              torch.zeros(1, 3, 1, 1, device=DEV))


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,amp", [(1, 64, 64, 0.3), (2, 33, 47, 1.0), (1, 256, 256, 1.0), (1, 5, 3, 2.0),
                                         (1, 1, 7, 1.0), (2, 6, 1, 1.0)])      # (a dimension of one: lin(n == 1), make_tap(size == 1))
def test_voxelwarp_vs_oracle(B, H, W, amp):
    g = torch.Generator().manual_seed(H * W)
    frames = torch.rand(B, 6, H, W, generator=g) * 2 - 1
    x3 = torch.tanh(torch.randn(B, 3, H, W, generator=g) * amp)  # amp>=1 pushes samples past the border
    gO = torch.randn(B, 3, H, W, generator=g)
    fr, xr = frames.clone().requires_grad_(), x3.clone().requires_grad_()
    ref = O.voxel_warp_blend(fr, xr)
    ref.backward(gO)

    fd, xd = frames.to(DEV).requires_grad_(), x3.to(DEV).requires_grad_()
    out = hip_ops.voxel_warp_blend(fd, xd)
    out.backward(gO.to(DEV))
    # bilinear weights are built from coordinates ~1e2 px: 1e-5 absolute on [-1,1] images
    assert (out.detach().cpu() - ref.detach()).abs().max() < 2e-5
    # d/dflow multiplies texel differences by (size-1)/2: compare relative to the largest gradient
    assert _rel(xd.grad.cpu(), xr.grad) < 1e-4
    assert _rel(fd.grad.cpu(), fr.grad) < 1e-4


# ---------------------------------------------------------------------------------------------
# 2x2 average pooling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(2, 32, 384, 512), (1, 5, 7, 9), (1, 3, 2, 2), (2, 4, 65, 130), (1, 2, 64, 67)])
def test_avgpool2x2_matches_aten(N, C, H, W):
    gen = torch.Generator().manual_seed(H * W)
    x = torch.randn(N, C, H, W, generator=gen)
    g = torch.randn(N, C, H // 2, W // 2, generator=gen)
    xr = x.clone().requires_grad_()
    ref = F.avg_pool2d(xr, 2)
    ref.backward(g)
    xd = x.to(DEV).requires_grad_()
    out = hip_ops.avg_pool2x2(xd)
    out.backward(g.to(DEV))
    assert torch.allclose(out.detach().cpu(), ref.detach(), atol=1e-6, rtol=1e-6)
    assert torch.equal(xd.grad.cpu(), xr.grad)                   # g / 4 and zeros: exact
    # the adjoint is a Function too: double backward (second-order MAML) goes through the forward kernel
    xd2 = x.to(DEV).requires_grad_()
    (gx,) = torch.autograd.grad(hip_ops.avg_pool2x2(xd2), xd2, g.to(DEV).requires_grad_(), create_graph=True)
    assert gx.requires_grad


# ---------------------------------------------------------------------------------------------
# pixel-flow backward warp (Super SloMo backWarp / RRIN warp)
# ---------------------------------------------------------------------------------------------
def test_flowwarp_matches_the_reference_fixture():
    """Values and flow gradient of the reference's own backWarp run on CPU (tests/golden/ops.npz: fw_*)."""
    g = golden("ops")
    img, gout = torch.from_numpy(g['fw_img']).to(DEV), torch.from_numpy(g['fw_gout']).to(DEV)
    flow = torch.from_numpy(g['fw_flow']).to(DEV).requires_grad_()
    out = hip_ops.flow_warp(img, flow)
    out.backward(gout)
    assert np.abs(out.detach().cpu().numpy() - g['fw_out']).max() < 2e-6
    assert np.abs(flow.grad.cpu().numpy() - g['fw_gflow']).max() < 1e-5 * np.abs(g['fw_gflow']).max()


@pytest.mark.parametrize("N,C,H,W,amp", [(1, 3, 128, 128, 1.0), (2, 3, 64, 192, 6.0), (1, 3, 37, 53, 30.0), (1, 1, 1, 1, 0.7),
                                         (2, 5, 3, 300, 2.0), (1, 3, 768, 1280, 8.0)])
def test_flowwarp_vs_oracle(N, C, H, W, amp):
    gen = torch.Generator().manual_seed(H * W + C)
    img = torch.rand(N, C, H, W, generator=gen)
    flow = torch.randn(N, 2, H, W, generator=gen) * amp              # large amp: most targets leave the frame
    gout = torch.randn(N, C, H, W, generator=gen)
    fr = flow.clone().requires_grad_()
    ref = O.flow_warp(img, fr)
    ref.backward(gout)
    fd = flow.to(DEV).requires_grad_()
    out = hip_ops.flow_warp(img.to(DEV), fd)
    out.backward(gout.to(DEV))
    # coordinates are rounded at ~6e-8 * W px; the image is white noise (texel differences ~1)
    assert (out.detach().cpu() - ref.detach()).abs().max() < 5e-6 * max(1.0, W / 64.0)
    assert _rel(fd.grad.cpu(), fr.grad) < 1e-5 * max(1.0, W / 64.0)
    # idempotence under a zero flow shifted by the reference's half pixel: sampling at (x - 0.5, y - 0.5)
    zero = hip_ops.flow_warp(img.to(DEV), torch.full((N, 2, H, W), 0.5, device=DEV))
    assert torch.allclose(zero.cpu(), img, atol=2e-4)      # the coordinate round trip is exact to ~1e-4 px at W = 1280


def test_flowwarp_refuses_an_image_gradient_and_survives_nan_flows():
    img = torch.rand(1, 3, 8, 8, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        hip_ops.flow_warp(img, torch.zeros(1, 2, 8, 8, device=DEV))
    bad = torch.zeros(1, 2, 8, 8, device=DEV)
    bad[0, 0, 0, 0], bad[0, 1, 1, 1], bad[0, 0, 2, 2] = float('nan'), float('inf'), -1e30
    out = hip_ops.flow_warp(img.detach(), bad)
    assert out[0, :, 0, 0].abs().sum() == 0 and out[0, :, 1, 1].abs().sum() == 0 and out[0, :, 2, 2].abs().sum() == 0


@pytest.mark.parametrize("B,C,H,W,r", [(1, 3, 128, 128, 8), (2, 3, 16, 24, 2), (1, 3, 768, 1280, 8), (1, 1, 8, 8, 8),
                                       (1, 2, 9, 15, 3)])
def test_pixel_shuffle_roundtrip_and_oracle(B, C, H, W, r):
    x = torch.randn(B, C, H, W)
    xd = x.to(DEV).requires_grad_()
    down = hip_ops.pixel_shuffle(xd, 1.0 / r)
    assert torch.equal(down.detach().cpu(), O.pixel_shuffle(x, 1.0 / r))   # pure permutation: bit exact
    up = hip_ops.pixel_shuffle(down, r)
    assert torch.equal(up.detach().cpu(), x)
    assert torch.equal(hip_ops.pixel_shuffle(down.detach(), r).cpu(), O.pixel_shuffle(down.detach().cpu(), r))
    g = torch.randn_like(down)
    down.backward(g)
    assert torch.equal(xd.grad.cpu(), O.pixel_shuffle(g.cpu(), r))            # adjoint = inverse permutation


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", [(1, 3, 256, 448), (1, 3, 7, 5), (2, 3, 64, 64)])
def test_l1_mse_vs_torch(kind, shape):
    a, b = torch.rand(shape), torch.rand(shape)
    ar = a.clone().requires_grad_()
    ref = (torch.nn.functional.l1_loss if kind == 0 else torch.nn.functional.mse_loss)(ar, b)
    ref.backward()
    ad = a.to(DEV).requires_grad_()
    out = (hip_ops.l1_loss if kind == 0 else hip_ops.mse_loss)(ad, b.to(DEV))
    (out * 1.0).backward()
    assert abs(out.item() - ref.item()) < 1e-6 * max(1.0, abs(ref.item())) + 1e-7
    assert _rel(ad.grad.cpu(), ar.grad) < 1e-6


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("shape,k,pad", [((2, 6, 37, 45), 3, 1), ((1, 64, 96, 128), 3, 1), ((1, 8, 16, 16), 5, 2), ((1, 3, 7, 9), 1, 0)])
def test_conv_bias_act_matches_unfused_torch(slope, shape, k, pad):
    """Fused conv epilogue (bias + LeakyReLU(slope) in place; act' * gy + bias gradient in one pass) against
    F.conv2d + F.leaky_relu and autograd on the same device.  Where both sides run the same MIOpen kernels: 1e-6; a
    3x3 layer large enough for the savfi Winograd / weight-gradient kernels differs by fp32 summation order: 1e-5."""
    g = torch.Generator().manual_seed(int(slope * 10) + shape[1])
    x = torch.randn(shape, generator=g).to(DEV).requires_grad_()
    w = (torch.randn(shape[1] + 1, shape[1], k, k, generator=g) / (k * shape[1] ** 0.5)).to(DEV).requires_grad_()
    b = torch.randn(shape[1] + 1, generator=g).to(DEV).requires_grad_()
    go = torch.randn(shape[0], shape[1] + 1, shape[2], shape[3], generator=g).to(DEV)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, w, b, 1, pad), slope)
    gx, gw, gb = torch.autograd.grad(ref, (x, w, b), go)
    out = hip_ops.conv_bias_act(x, w, b, 1, pad, 1, 1, slope)
    fx, fw, fb = torch.autograd.grad(out, (x, w, b), go)
    tol = 1e-5 if (hip_ops.conv3x3_wgrad_eligible(x, w, 1, pad, 1, 1) or hip_ops.conv3x3_eligible(x, w, 1, pad, 1, 1)) else 1e-6
    assert _rel(out.detach(), ref.detach()) < tol
    assert _rel(fx, gx) < tol and _rel(fw, gw) < tol and _rel(fb, gb) < 1e-5


def test_meta_sequential_fuses_conv_relu_pairs_and_matches_reference_modules():
    from meta_interpolation_amd import model_utils as mu
    torch.manual_seed(0)
    seq = mu.MetaSequential(mu.MetaConv2dLayer(6, 8, 3, 1, 1), torch.nn.ReLU(), mu.MetaConv2dLayer(8, 5, 3, 1, 1),
                            torch.nn.ReLU(), torch.nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True),
                            mu.MetaConv2dLayer(5, 5, 3, 1, 1)).to(DEV)
    x = torch.randn(2, 6, 20, 24, device=DEV)
    fast = {n: torch.randn_like(p).mul(0.1).requires_grad_() for n, p in seq.named_parameters()}
    calls = []
    orig = hip_ops.conv_bias_act
    hip_ops.conv_bias_act = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    mu.set_fuse_conv_act(True)
    try:
        y = seq(x, params=fast)
        gf = torch.autograd.grad(y.square().mean(), list(fast.values()))
    finally:
        hip_ops.conv_bias_act = orig
        mu.set_fuse_conv_act(False)
    # two conv+ReLU pairs fused; the last conv (bias, no activation) also takes the fused op: 2 x 20 x 24 tiles >= WINO_MIN_TILES_FWD_BATCHED
    assert len(calls) == 3
    y0 = seq(x, params=fast)                                  # unfused: MIOpen convolutions, separate activations
    g0 = torch.autograd.grad(y0.square().mean(), list(fast.values()))
    assert _rel(y, y0) < 5e-6                                 # Winograd rounding: <= 2e-7 of the output scale per layer
    for a, b in zip(gf, g0):
        assert _rel(a, b) < 2e-5


@pytest.mark.parametrize("case", ["wino_relu", "convk_relu", "wino_leaky", "tasks_wino", "tasks_convk", "small_maps_miopen"])
def test_conv_chain_folds_the_activation_derivative_into_the_consumer(case, monkeypatch):
    """conv -> act -> conv -> act -> conv in a MetaSequential: with the chain fusion the consumer's data-gradient kernel applies the
    producer's (leaky) ReLU derivative in its epilogue (savfi_conv3x3_dgrad_masked_f32 / savfi_convk_dgrad_masked_f32) and the producer
    only sums its bias gradient -- the same multiplications, so the gradients of the input and of every weight equal the unchained
    run (model_utils._FUSE_CONV_CHAIN = False) bit for bit, the bias gradients to summation order; and an element-wise bias_act_bwd launch disappears per chain link."""
    from meta_interpolation_amd import model_utils as mu
    torch.manual_seed(3)
    C, H, W, T, act = {"wino_relu": (32, 64, 96, 0, torch.nn.ReLU()), "convk_relu": (64, 48, 64, 0, torch.nn.ReLU()),
                       "wino_leaky": (32, 40, 56, 0, torch.nn.LeakyReLU(0.2)), "tasks_wino": (32, 48, 64, 4, torch.nn.ReLU()),
                       "tasks_convk": (64, 32, 48, 4, torch.nn.ReLU()), "small_maps_miopen": (16, 3, 5, 0, torch.nn.ReLU())}[case]
    seq = mu.MetaSequential(mu.MetaConv2dLayer(C, C, 3, 1, 1), act, mu.MetaConv2dLayer(C, C, 3, 1, 1), act,
                            mu.MetaConv2dLayer(C, C, 3, 1, 1), act).to(DEV)
    N = 2 * max(T, 1)
    x0 = torch.randn(N, C, H, W, device=DEV)
    if T:
        fast0 = {n: torch.randn((T,) + tuple(p.shape), device=DEV).mul(0.3 / C ** 0.5) for n, p in seq.named_parameters()}
    else:
        fast0 = {n: torch.randn_like(p).mul(0.3 / C ** 0.5) for n, p in seq.named_parameters()}
    results, launches = {}, {}
    for chained in (True, False):
        monkeypatch.setattr(mu, '_FUSE_CONV_CHAIN', chained)
        x = x0.clone().requires_grad_()
        fast = {n: v.clone().requires_grad_() for n, v in fast0.items()}
        count = []
        orig = _hip.launch
        monkeypatch.setattr(_hip, 'launch', lambda name, fn, **k: (count.append(name), orig(name, fn, **k))[1])
        mu.set_fuse_conv_act(True)
        try:
            y = seq(x, params=fast)
            grads = torch.autograd.grad(y.square().mean(), [x] + list(fast.values()))
        finally:
            mu.set_fuse_conv_act(False)
            monkeypatch.setattr(_hip, 'launch', orig)
        results[chained] = [y.detach()] + [g.detach() for g in grads]
        launches[chained] = count
    for name, a, b in zip(["y", "x"] + list(fast0), results[True], results[False]):
        if name.endswith("bias"):       # a link that defers has nothing to do with its cotangent: where its weight gradient runs on the
            assert _rel(a, b) < 2e-6, (case, name, _rel(a, b))      # all-taps kernel the bias sums ride on it (another summation order)
        else:
            assert torch.equal(a, b), (case, name, (a - b).abs().max().item())
    # the element-wise derivative pass of the two inner links is gone (the bias-gradient sums stay, or ride on the weight gradient)
    n_conv = lambda names: sum(1 for n in names if 'bwd_data' in n)
    assert n_conv(launches[True]) == n_conv(launches[False])
    if case != "small_maps_miopen":
        assert n_conv(launches[True]) == 3


@pytest.mark.parametrize("case", ["c5_shape", "small_f2", "tasks"])
def test_rcab_folds_the_relu_derivative_through_the_mirrored_border(case, monkeypatch):
    """CAIN's RCAB (reference model_utils.py:957-990): mirror -> conv -> ReLU -> mirror -> conv -> channel attention + skip.  The ReLU's
    derivative goes into the SECOND convolution's data gradient, masked by its padded input (a padded map's mask is the mirrored mask,
    so masking before the fold equals masking after it, bit for bit with slope 0), and both bias gradients ride on the all-taps
    weight-gradient kernel where that runs: no element-wise pass over a cotangent is left.  Against the run without the chain: output,
    input gradient and weight gradients bit-equal, bias gradients to summation order; and against the module in float64 on the CPU."""
    import copy
    from meta_interpolation_amd import model_utils as mu
    torch.manual_seed(5)
    C, N, H, W, T = {"c5_shape": (192, 1, 96, 160, 0), "small_f2": (64, 2, 20, 24, 0), "tasks": (64, 8, 16, 16, 4)}[case]
    rcab = mu.MetaRCAB(C, C, 3, 16).to(DEV)
    x0 = torch.randn(N, C, H, W, device=DEV)
    if T:
        fast0 = {n: torch.randn((T,) + tuple(p.shape), device=DEV).mul(0.5 / (p[0].numel() ** 0.5 if p.dim() > 1 else 4.0))
                 for n, p in rcab.named_parameters()}
    else:
        fast0 = {n: (torch.randn_like(p).mul(0.5 / p[0].numel() ** 0.5) if p.dim() > 1 else torch.randn_like(p).mul(0.1))
                 for n, p in rcab.named_parameters()}
    names = list(fast0)
    results, launches = {}, {}
    for chained in (True, False):
        monkeypatch.setattr(mu, '_FUSE_CONV_CHAIN', chained)
        x = x0.clone().requires_grad_()
        fast = {n: v.clone().requires_grad_() for n, v in fast0.items()}
        count = []
        orig = _hip.launch
        monkeypatch.setattr(_hip, 'launch', lambda name, fn, **k: (count.append(name), orig(name, fn, **k))[1])
        mu.set_fuse_conv_act(True)
        try:
            y = rcab(x, params=fast)
            grads = torch.autograd.grad(y.square().mean(), [x] + list(fast.values()))
        finally:
            mu.set_fuse_conv_act(False)
            monkeypatch.setattr(_hip, 'launch', orig)
        results[chained] = [y.detach()] + [g.detach() for g in grads]
        launches[chained] = count
    for name, a, b in zip(["out", "x"] + names, results[True], results[False]):
        if name.endswith("conv.bias"):
            assert _rel(a, b) < 2e-6, (case, name, _rel(a, b))
        else:
            assert torch.equal(a, b), (case, name, (a - b).abs().max().item())
    if case == "c5_shape":          # F(4x4) data gradients, all-taps weight gradients: nothing element-wise between the kernels
        assert sum(1 for n in launches[True] if 'bwd_data' in n) == 2
        assert 'bias_act_bwd' not in launches[True] and launches[False].count('bias_act_bwd') == 1
    if not T:
        ref = copy.deepcopy(rcab).cpu().double()
        xr = x0.cpu().double().requires_grad_()
        fr = {n: v.cpu().double().requires_grad_() for n, v in fast0.items()}
        yr = ref(xr, params=fr)
        gr = torch.autograd.grad(yr.square().mean(), [xr] + list(fr.values()))
        # (gradients in the 2-norm with room for a few flipped masks: a pre-activation within rounding of zero -- a handful of the
        # block's 3 million -- takes the other side of the ReLU in float32 and moves whole terms; a missing or misplaced mask is an
        # error of order one)
        for name, a, b in zip(["out", "x"] + names, results[True], [yr.detach()] + list(gr)):
            err = ((a.cpu().double() - b).norm() / b.norm()).item()
            assert err < (2e-5 if name == "out" else 1e-3), (case, name, err)


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape", [(1, 51, 192, 256), (2, 7, 5, 9), (1, 3, 1, 1), (1, 64, 12, 16), (2, 4, 33, 17)])
def test_upsample2x_matches_aten(align, shape):
    """Bilinear x2 forward and adjoint against F.interpolate + autograd on the device (same index rules)."""
    g = torch.Generator().manual_seed(shape[2] * 7 + shape[3])
    x = torch.randn(shape, generator=g).to(DEV).requires_grad_()
    ref = torch.nn.functional.interpolate(x, scale_factor=2, mode='bilinear', align_corners=align)
    go = torch.randn(ref.shape, generator=g).to(DEV)
    gref, = torch.autograd.grad(ref, x, go)
    out = hip_ops.upsample_bilinear2x(x, align)
    gx, = torch.autograd.grad(out, x, go)
    assert (out - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
    assert _rel(gx, gref) < 1e-5
    # and against the CPU result (pins the index arithmetic independently of the device ATen kernel)
    cpu = torch.nn.functional.interpolate(x.detach().cpu(), scale_factor=2, mode='bilinear', align_corners=align)
    assert (out.detach().cpu() - cpu).abs().max().item() <= 2e-6 * max(1.0, cpu.abs().max().item())


# ---------------------------------------------------------------------------------------------
# windowed x2 up-sampling and the windowed SepConv tail
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("geom", [
    # (H, W, crop y0, y1, x0, x1, window oy0, ox0, Hw, Ww)
    (24, 32, 0, 24, 0, 32, 0, 0, 48, 64),          # the full op
    (24, 32, 3, 20, 5, 30, 9, 13, 28, 40),
    (96, 128, 8, 80, 0, 128, 24, 0, 130, 256),     # clipped at the left / right border
    (17, 19, 0, 9, 10, 19, 0, 23, 15, 15),
])
def test_upsample_window_matches_full_op(align, geom):
    H, W, cy0, cy1, cx0, cx1, oy0, ox0, Hw, Ww = geom
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, H, W, generator=g).cuda()
    full = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=align)
    crop = x[:, :, cy0:cy1, cx0:cx1].contiguous().requires_grad_()
    out = hip_ops.upsample_bilinear2x_window(crop, (H, W), (cy0, cx0), (oy0, ox0, Hw, Ww), align)
    assert torch.equal(out, hip_ops.upsample_bilinear2x(x, align)[:, :, oy0:oy0 + Hw, ox0:ox0 + Ww])
    assert (out - full[:, :, oy0:oy0 + Hw, ox0:ox0 + Ww]).abs().max() < 1e-6
    # adjoint: gradient of the full op fed with a cotangent that is zero outside the window, cropped
    go = torch.randn(out.shape, generator=g).cuda()
    (gc,) = torch.autograd.grad(out, crop, go)
    xr = x.clone().requires_grad_()
    fr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=align)
    gfull = torch.zeros_like(fr)
    gfull[:, :, oy0:oy0 + Hw, ox0:ox0 + Ww] = go
    (gx,) = torch.autograd.grad(fr, xr, gfull)
    assert (gc - gx[:, :, cy0:cy1, cx0:cx1]).abs().max() < 2e-6
    # nothing of the cotangent may land outside the crop (the window reads only the crop)
    mask = torch.ones_like(gx, dtype=torch.bool)
    mask[:, :, cy0:cy1, cx0:cx1] = False
    assert gx[mask].abs().sum() == 0


def test_upsample_window_rejects_window_outside_crop():
    x = torch.zeros(1, 1, 8, 8).cuda()
    with pytest.raises(_hip.SavfiHipError):
        hip_ops.upsample_bilinear2x_window(x[:, :, 2:6, 2:6].contiguous(), (8, 8), (2, 2), (0, 0, 16, 16), True)


@pytest.mark.parametrize("hw", [(64, 96), (78, 60), (256, 448)])
def test_sepconv_windowed_tail_equals_full_canvas(hw):
    """sepconv/model.py: the sub-networks / 51-tap op evaluated on the frame window give the values (and the
    parameter / fast-weight gradients) of the reference's full-canvas evaluation (sepconv/model.py:309-349)."""
    from meta_interpolation_amd import synthetic
    from meta_interpolation_amd.sepconv.model import MetaNetwork
    H, W = hw
    nets = []
    for windowed in (False, True):
        net = MetaNetwork(windowed=windowed)
        synthetic.load_seeded_weights(net, 'sepconv')
        nets.append(net.cuda())
    frames = synthetic.septuplet_batch(2, H, W, model='sepconv')
    f0, f1, tgt = frames[2].cuda(), frames[4].cuda(), frames[3].cuda()
    res = []
    for net in nets:
        out = net(f0, f1)
        loss = (out - tgt).abs().mean()
        names = [n for n, _ in net.named_parameters()]
        grads = torch.autograd.grad(loss, list(net.parameters()))
        res.append((out.detach(), dict(zip(names, grads))))
    (o_full, g_full), (o_win, g_win) = res
    assert o_win.shape == o_full.shape == (2, 3, H, W)
    assert (o_win - o_full).abs().max() < 2e-6
    for n in g_full:
        ref = g_full[n]
        assert (g_win[n] - ref).abs().max() <= 2e-5 * ref.abs().max() + 1e-9, n


@pytest.mark.parametrize("const", [False, True])
@pytest.mark.parametrize("hw", [(64, 96), (72, 60), (256, 448)])
def test_sepconv_subnets_as_one_batched_launch_equal_one_by_one(hw, const):
    """sepconv/model.py: the four Subnets as ONE task-batched launch per layer (layer 1 a 64 -> 256 convolution, layers 2..4 with four
    filter sets on the interleaved [4 N, C, h, w] maps, the taps read in place by FunctionSepconvPair / savfi_sepconv_*_taps_strided_f32)
    against the Subnet-by-Subnet evaluation (reference sepconv/model.py:346-347): predictions, fast-weight gradients and -- when the
    plugin's own parameters are differentiated (`const` False: the outer pass) -- the Subnets' own gradients.  `const`: the support
    passes' mode (own parameters are constants; the stacked weights and their packed filters are cached across passes)."""
    from meta_interpolation_amd import model_utils as mu, synthetic
    from meta_interpolation_amd.sepconv.model import MetaNetwork
    H, W = hw
    net = MetaNetwork(windowed=True)
    synthetic.load_seeded_weights(net, 'sepconv')
    net = net.cuda()
    frames = synthetic.septuplet_batch(2, H, W, model='sepconv')
    f0, f1, tgt = frames[2].cuda(), frames[4].cuda(), frames[3].cuda()
    routed = {n: p for n, p in net.named_parameters() if n.startswith(('moduleConv', 'moduleDeconv'))}
    res = {}
    mu.set_fuse_conv_act(True)
    mu.set_own_params_const(const)
    try:
        for batched in (True, False, True):          # the second batched run hits the stacked-weight / filter cache
            net.batch_subnets = batched
            fast = {n: p.detach().clone().requires_grad_() for n, p in routed.items()}
            out = net(f0, f1, params=fast)
            loss = (out - tgt).abs().mean()
            wrt = list(fast.values()) + ([] if const else [p for n, p in net.named_parameters() if n not in routed])
            names = list(fast) + ([] if const else [n for n, _ in net.named_parameters() if n not in routed])
            grads = torch.autograd.grad(loss, wrt, allow_unused=True)
            cur = (out.detach(), dict(zip(names, grads)))
            if batched and True in res:
                assert torch.equal(cur[0], res[True][0])         # deterministic, cache or no cache
            res[batched] = cur
    finally:
        mu.set_fuse_conv_act(False)
        mu.set_own_params_const(False)
    from meta_interpolation_amd import _hip
    assert _hip.lib().savfi_sepconv_ws_errors() == 0
    (o_b, g_b), (o_s, g_s) = res[True], res[False]
    assert (o_b - o_s).abs().max() < 2e-6
    for n, ref in g_s.items():
        if ref is None:
            assert g_b[n] is None, n
            continue
        assert (g_b[n] - ref).abs().max() <= 2e-5 * ref.abs().max() + 1e-9, (n, (g_b[n] - ref).abs().max().item(), ref.abs().max().item())


# ---------------------------------------------------------------------------------------------
# Winograd convolution on the fp32 matrix cores: F(4x4,3x3) up to 512 -> 512 channels (csrc/winograd4.h), F(2x2,3x3) beyond
# ---------------------------------------------------------------------------------------------
def conv3x3_close(got, want, Ci, Co):
    """Rounding bound of the form the layer runs on, against float64.  F(2x2): 2e-6 of the result's scale (measured 2-4e-7).  F(4x4)
    (interpolation points 0, +-1, +-2, inf): its transforms multiply by up to 8 before they cancel -- measured 1.5-4e-7 rms, 3e-6..1e-5 max
    over tools/r6/wino4_check.py's shapes (a numpy transcription of the same arithmetic: 3.6e-7 / 4.6e-6; the direct fp32 sum 7e-8 / 6e-7).
    Gates: 2e-5 max AND 1e-6 rms of the scale -- the system-level contract (pixel L1 1e-4, loss 1e-5) is held by the fixture tests."""
    scale = want.abs().max()
    d = (got - want)
    if max(Ci, Co) <= 512:
        return bool(d.abs().max() <= 2e-5 * scale) and bool(d.pow(2).mean().sqrt() <= 1e-6 * scale)
    return bool(d.abs().max() <= 2e-6 * scale)



CONV_SHAPES = [
    # N, Ci, Co, H, W
    (1, 8, 64, 16, 64),       # exactly one tile block
    (2, 6, 32, 24, 40),       # padded Ci / Co, ragged tile block
    (1, 64, 51, 37, 45),      # odd sizes, Co = 51
    (2, 51, 51, 18, 30),
    (1, 128, 128, 48, 64),
    (1, 3, 5, 5, 7),
    (2, 256, 256, 13, 21),    # F(4x4) with its reduction split over workgroups
    (1, 512, 512, 12, 16),    # the deepest F(4x4) layer
    (1, 576, 528, 12, 20),    # beyond 512 channels: the F(2x2) kernel
]


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_forward_matches_conv2d(shape, pad):
    N, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(Co, generator=g)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    got = hip_ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), mode=0, slope=1.0, pad=pad).cpu().double()
    assert got.shape == want.shape
    assert conv3x3_close(got, want, Ci, Co)
    got = hip_ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), mode=0, slope=0.0, pad=pad).cpu().double()
    assert conv3x3_close(got, F.relu(want), Ci, Co)
    got = hip_ops.conv3x3(x.cuda(), w.cuda(), None, mode=0, slope=0.2, pad=pad).cpu().double()
    assert conv3x3_close(got, F.leaky_relu(F.conv2d(x.double(), w.double(), None, padding=pad), 0.2), Ci, Co)


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_data_gradient_matches_autograd(shape, pad):
    N, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(12)
    x = torch.randn(N, Ci, H, W, generator=g).double().requires_grad_()
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Co ** 0.5)
    y = F.conv2d(x, w.double(), None, padding=pad)
    gy = torch.randn(y.shape, generator=g)
    (want,) = torch.autograd.grad(y, x, gy.double())
    got = hip_ops.conv3x3(gy.cuda(), w.cuda(), None, mode=1, slope=1.0, pad=pad).cpu().double()
    assert got.shape == want.shape
    assert conv3x3_close(got, want, Ci, Co)


@pytest.mark.parametrize("T,N,Ci,Co,H,W,pad", [(1, 2, 6, 32, 24, 40, 1), (4, 8, 51, 51, 18, 30, 1), (2, 4, 64, 32, 16, 64, 0), (4, 8, 256, 256, 12, 16, 1),
                                               (4, 8, 640, 576, 12, 16, 1)])
def test_conv3x3_split_entry_points_equal_the_fused_one(T, N, Ci, Co, H, W, pad):
    """savfi_conv3x3_filters_f32 (both transforms in one launch) + savfi_conv3x3_tasks_pre_f32 == savfi_conv3x3_tasks_f32,
    bit for bit, forward and data gradient (the last shape splits its reduction channels: partial-output workspace)."""
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).cuda()
    b = torch.randn(T, Co, generator=g).cuda()
    x = torch.randn(N, Ci, H, W, generator=g).cuda()
    want = hip_ops.conv3x3_tasks(x, w, b, 0, 0.2, pad)
    gy = torch.randn(want.shape, generator=g).cuda()
    want_gx = hip_ops.conv3x3_tasks(gy, w, None, 1, 1.0, pad)
    for fwd, bwd in ((True, True), (True, False), (False, True)):
        u_f, u_b = hip_ops.conv3x3_filters(w, fwd, bwd)
        assert (u_f is None) == (not fwd) and (u_b is None) == (not bwd)
        if fwd:
            assert torch.equal(hip_ops.conv3x3_tasks_pre(x, u_f, T, Ci, Co, b, 0, 0.2, pad), want)
        if bwd:
            assert torch.equal(hip_ops.conv3x3_tasks_pre(gy, u_b, T, Ci, Co, None, 1, 1.0, pad), want_gx)


@pytest.mark.parametrize("T,N,Ci,Co,H,W,pad", [(1, 2, 51, 51, 18, 30, 1), (4, 8, 192, 192, 16, 16, 1), (2, 4, 64, 32, 16, 64, 0)])
def test_conv3x3_form2_keeps_small_launches_on_the_f2x2_kernel(T, N, Ci, Co, H, W, pad):
    """A launch too small for F(4x4) to pay runs the F(2x2) kernel although its channel counts would select F(4x4) (hip_ops.wino_form2 ->
    filters of kind 'wino2', bit 1 of the C ABI's `mode`): F(2x2)'s rounding bound (2e-6 of the scale) against float64, forward, data
    gradient and masked data gradient; and the form-0 call of the same layer is the F(4x4) kernel (different bits)."""
    g = torch.Generator().manual_seed(21)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(T, Co, generator=g)
    xc, wc, bc = x.to(DEV), w.to(DEV), b.to(DEV)
    assert hip_ops.wino_form2(xc, wc, pad)
    want = torch.cat([F.leaky_relu(F.conv2d(x[n:n + 1].double(), w[n % T].double(), b[n % T].double(), padding=pad), 0.2) for n in range(N)])
    u_f, u_b = hip_ops.conv3x3_filters(wc, True, True, f2=True)
    got = hip_ops.conv3x3_tasks_pre(xc, u_f, T, Ci, Co, bc, 0, 0.2, pad, f2=True)
    assert (got.cpu().double() - want).abs().max() <= 2e-6 * want.abs().max()
    assert torch.equal(got, hip_ops.conv3x3_tasks(xc, wc, bc, 0, 0.2, pad, f2=True))
    assert not torch.equal(got, hip_ops.conv3x3_tasks(xc, wc, bc, 0, 0.2, pad))          # form 0: the F(4x4) kernel
    gy = torch.randn(want.shape, generator=g)
    wantg = torch.cat([F.conv_transpose2d(gy[n:n + 1].double(), w[n % T].double(), padding=pad) for n in range(N)])
    gotg = hip_ops.conv3x3_tasks_pre(gy.to(DEV), u_b, T, Ci, Co, None, 1, 1.0, pad, f2=True)
    assert (gotg.cpu().double() - wantg).abs().max() <= 2e-6 * wantg.abs().max()
    mask = torch.randn(wantg.shape, generator=g).to(DEV)
    gotm = hip_ops.conv3x3_tasks_pre(gy.to(DEV), u_b, T, Ci, Co, None, 1, 1.0, pad, mask=mask, mask_slope=0.1, f2=True)
    assert torch.equal(gotm, gotg * torch.where(mask > 0, 1.0, 0.1))
    # the layer's module-level route: conv_bias_act_tasks picks the form by the launch
    y = hip_ops.conv_bias_act_tasks(xc, wc, bc, 1, pad, 1, 0.2)
    assert torch.equal(y, got)


@pytest.mark.parametrize("T,N,Ci,Co,H,W,pad", [(4, 32, 51, 51, 258, 450, 0), (4, 8, 64, 64, 192, 256, 1), (4, 8, 512, 512, 24, 32, 1), (4, 8, 32, 32, 384, 512, 1)])
def test_conv3x3_full_size_properties(T, N, Ci, Co, H, W, pad):
    """The benchmark's layer shapes, where float64 references take minutes: size-independent properties of the F(4x4) kernel instead.
    Adjointness -- <conv(x), y> == <x, dgrad(y)> (forward and data gradient are two launches on two filter transforms; unit-major in /
    out where the layer has them); linearity in the input; a one-hot centre-tap filter routes channel ci to channel co and reproduces it
    within the form's rounding."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Ci, H, W, generator=g).to(DEV)
    w = (torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).to(DEV)
    assert hip_ops.wino4_workgroups(N, Ci, Co, H, W, pad) >= hip_ops.WINO4_MIN_WORKGROUPS and not hip_ops.wino_form2(x, w, pad)
    u_f, u_b = hip_ops.conv3x3_filters(w, True, True)
    y = hip_ops.conv3x3_tasks_pre(x, u_f, T, Ci, Co, None, 0, 1.0, pad)
    gy = torch.randn(y.shape, generator=g).to(DEV)
    gx = hip_ops.conv3x3_tasks_pre(gy, u_b, T, Ci, Co, None, 1, 1.0, pad)
    assert gx.shape == x.shape
    lhs, rhs = (y.double() * gy.double()).sum().item(), (x.double() * gx.double()).sum().item()
    scale = (y.double().abs() * gy.double().abs()).sum().item()
    assert abs(lhs - rhs) <= 2e-6 * scale, (lhs, rhs, scale)
    x2 = torch.randn(x.shape, generator=g).to(DEV)
    y2 = hip_ops.conv3x3_tasks_pre(x2, u_f, T, Ci, Co, None, 0, 1.0, pad)
    y12 = hip_ops.conv3x3_tasks_pre(x + 0.5 * x2, u_f, T, Ci, Co, None, 0, 1.0, pad)
    assert (y12 - (y + 0.5 * y2)).abs().max().item() <= 2e-5 * y12.abs().max().item()
    if y.shape[3] % 16 == 0 and hip_ops.conv3x3_unit16_supported(x, w, pad):          # the unit-major twins move the same bits
        yu = hip_ops.conv3x3_tasks_pre(x, u_f, T, Ci, Co, None, 0, 1.0, pad, out_unit16=True)
        B, K, Ho, Wo = y.shape
        assert torch.equal(yu.reshape(B, Ho, Wo // 16, K, 16).permute(0, 3, 1, 2, 4).reshape(B, K, Ho, Wo), y)
        if hip_ops.conv3x3_in_unit16_supported(tuple(gy.shape), w, pad):
            gyu = gy.reshape(B, K, Ho, Wo // 16, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(B, K, Ho, Wo)
            assert torch.equal(hip_ops.conv3x3_dgrad_in_unit16(gyu, u_b, T, Ci, Co, pad), gx)
    onehot = torch.zeros_like(w)
    for t in range(T):
        for co in range(Co):
            onehot[t, co, (co * 7 + t) % Ci, 1, 1] = 1.0
    u1, _ = hip_ops.conv3x3_filters(onehot, True, False)
    z = hip_ops.conv3x3_tasks_pre(x, u1, T, Ci, Co, None, 0, 1.0, pad)
    crop = slice(1 - pad, H - (1 - pad)), slice(1 - pad, W - (1 - pad))
    for n in (0, N - 1):
        t = n % T
        src = torch.stack([x[n, (co * 7 + t) % Ci][crop] for co in range(Co)])
        assert (z[n] - src).abs().max().item() <= 2e-5 * x.abs().max().item()


@pytest.mark.parametrize("T,N,Ci,Co,H,W,pad", [(1, 1, 3, 5, 6, 8, 1), (1, 2, 32, 32, 16, 16, 1), (2, 4, 6, 32, 24, 40, 1), (1, 1, 64, 51, 37, 45, 1),
                                               (1, 2, 51, 51, 18, 30, 0), (4, 8, 32, 32, 20, 30, 1), (1, 1, 8, 8, 5, 7, 0), (2, 2, 40, 70, 9, 130, 1)])
def test_conv3x3_wgrad_winograd_form_matches_autograd(T, N, Ci, Co, H, W, pad):
    """savfi_conv3x3_wgrad_wino_tasks_f32 (F(3x3, 2x2): cotangent and input transformed per 2x2 tile, 16 GEMMs over the tiles, one
    output transform per workgroup) against autograd in float64, per task: odd sizes, both paddings, channel counts that do not
    fill a 32-block, a row of more than eight tile chunks, and bit-reproducibility (fixed-order reduction)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Ci, H, W, generator=g)
    gz = torch.randn(N, Co, H + 2 * pad - 2, W + 2 * pad - 2, generator=g)
    want = []
    for t in range(T):
        w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(F.conv2d(x[t::T].double(), w, None, padding=pad), w, gz[t::T].double())
        want.append(gw)
    want = torch.stack(want)
    lib = _hip.lib()
    xd, gd = x.to(DEV), gz.to(DEV)

    def run():
        ws = torch.empty(int(lib.savfi_conv3x3_wgrad_wino_tasks_workspace_floats(N, T, Ci, Co, H, W, pad)), device=DEV)
        gw = torch.full((T, Co, Ci, 3, 3), float('nan'), device=DEV)
        _hip.check(lib.savfi_conv3x3_wgrad_wino_tasks_f32(xd.data_ptr(), gd.data_ptr(), gw.data_ptr(), ws.data_ptr(), N, T, Ci, Co, H, W, pad,
                                                          _hip.current_stream()), "wino wgrad")
        return gw
    got = run()
    # transformed-domain sums over all tiles in fp32: a few ulp more than the direct form (2e-7)
    assert (got.cpu().double() - want).abs().max() <= 3e-6 * want.abs().max()
    assert torch.equal(got, run())


@pytest.mark.parametrize("route", ["winograd", "winograd+direct"])
def test_sepconv_with_winograd_convs_equals_miopen_convs(route):
    """BASELINE config-2 frame size: the backbone's large 3x3 convolutions on savfi_conv3x3_f32 (forward with fused
    bias + ReLU, data gradient) and savfi_conv3x3_wgrad_f32 give the network output and every parameter gradient of the MIOpen path.
    A smooth loss is used: with L1 a 1e-7 output difference flips sign(out - target) for a few pixels.
    route "winograd+direct" = the product routing: the >= 64-channel layers and the 6-channel input layer on the direct
    split-bf16 kernel (hip_ops.convk_eligible), the rest on the Winograd kernel."""
    from meta_interpolation_amd import model_utils as mu, synthetic
    from meta_interpolation_amd.sepconv.model import MetaNetwork
    net = MetaNetwork()
    synthetic.load_seeded_weights(net, 'sepconv')
    net = net.cuda()
    frames = synthetic.septuplet_batch(2, 256, 448, model='sepconv')
    f0, f1, tgt = frames[2].cuda(), frames[4].cuda(), frames[3].cuda()
    res = []
    mu.set_fuse_conv_act(True)
    calls, kcalls = [], []
    orig, korig = hip_ops.conv3x3_tasks_pre, hip_ops.convk_tasks_pre
    try:
        for wino in (False, True):
            hip_ops.WINOGRAD_CONV = wino
            hip_ops.CONVK = wino and route == "winograd+direct"
            hip_ops.conv3x3_tasks_pre = (lambda *a, **k: (calls.append(a[6] if len(a) > 6 else k.get('mode', 0)), orig(*a, **k))[1])
            hip_ops.convk_tasks_pre = (lambda *a, **k: (kcalls.append(a[7] if len(a) > 7 else k.get('mode', 0)), korig(*a, **k))[1])
            out = net(f0, f1)
            loss = ((out - tgt) ** 2).mean()
            res.append((out.detach(), torch.autograd.grad(loss, list(net.parameters()))))
    finally:
        mu.set_fuse_conv_act(False)
        hip_ops.WINOGRAD_CONV = True
        hip_ops.CONVK = True
        hip_ops.conv3x3_tasks_pre, hip_ops.convk_tasks_pre = orig, korig
    # forward and data-gradient launches happened
    if route == "winograd":
        assert calls.count(0) >= 20 and calls.count(1) >= 8 and not kcalls, (calls, kcalls)
    else:
        assert calls.count(0) + kcalls.count(0) >= 20 and kcalls.count(0) >= 8 and kcalls.count(1) >= 4, (calls, kcalls)
    (o_mi, g_mi), (o_wi, g_wi) = res
    assert (o_wi - o_mi).abs().max() < 5e-6
    for (n, _), a, b in zip(net.named_parameters(), g_wi, g_mi):
        # both are valid fp32 evaluations; ReLU masks of the deep layers flip on rounding-level differences
        assert (a - b).abs().max() <= 1e-3 * b.abs().max() + 1e-12, n


# ---------------------------------------------------------------------------------------------
# frame staging: uint8 HWC over PCIe -> fp32 NCHW on the GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["sepconv", "voxelflow", "superslomo"])
def test_frame_stager_is_bit_identical_to_the_cpu_reader(model, tmp_path):
    import random
    import types
    from meta_interpolation_amd import data, synthetic
    root = synthetic.write_fake_vimeo(str(tmp_path / "vimeo"))
    mk = lambda gpus: types.SimpleNamespace(data_root=root, batch_size=2, val_batch_size=1, test_batch_size=1, mode='train',
                                            model=model, num_gpu=gpus, num_workers=3, random_seed=5, dataset='vimeo90k',
                                            synthetic=False)
    got = []
    for gpus in (0, 1):
        prov = data.MetaLearningSystemDataLoader(mk(gpus))
        assert (prov.stager is not None) == bool(gpus)
        random.seed(11)
        got.append([b for b in prov.get_train_batches()] + [b for b in prov.get_val_batches()])
    assert len(got[0]) == len(got[1]) == 4
    for (ic, mc), (ig, mg) in zip(*got):
        assert mc == mg
        for a, b in zip(ic, ig):
            assert b.is_cuda and torch.equal(a, b.cpu())


# ---------------------------------------------------------------------------------------------
# 3x3 weight gradient on the fp32 matrix cores
# ---------------------------------------------------------------------------------------------
WGRAD_SHAPES = [
    # N, Ci, Co, H, W
    (1, 32, 32, 16, 64),
    (2, 6, 32, 24, 40),
    (1, 64, 51, 37, 45),
    (2, 51, 51, 18, 130),
    (1, 128, 96, 12, 16),
    (1, 3, 5, 5, 7),
    (3, 40, 33, 9, 70),
]


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic(shape, pad):
    N, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(13)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / 10).double().requires_grad_()
    y = F.conv2d(x.double(), w, None, padding=pad)
    gz = torch.randn(y.shape, generator=g)
    (want,) = torch.autograd.grad(y, w, gz.double())
    junk = torch.full((1 << 22,), float('nan'), device='cuda')
    del junk
    got = hip_ops.conv3x3_wgrad(x.cuda(), gz.cuda(), pad)
    assert got.shape == (Co, Ci, 3, 3)
    assert (got.cpu().double() - want).abs().max() <= 3e-6 * want.abs().max()
    again = hip_ops.conv3x3_wgrad(x.cuda(), gz.cuda(), pad)
    assert torch.equal(got, again)                       # fixed-order reductions: bit-reproducible


# ---------------------------------------------------------------------------------------------
# tasks in lockstep: per-task filter sets in one launch (savfi_conv3x3_tasks_f32, savfi_conv3x3_wgrad_tasks_f32,
# hip_ops.conv_bias_act_tasks) against the same op run once per task
# ---------------------------------------------------------------------------------------------
TASK_CONV_CASES = [  # T, n (samples per task), Ci, Co, H, W
    (4, 2, 6, 32, 40, 72), (4, 2, 64, 64, 24, 32), (3, 1, 51, 51, 33, 29), (2, 2, 512, 512, 4, 6), (4, 1, 128, 256, 12, 16),
    (4, 2, 32, 32, 96, 128)]


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("T,n,Ci,Co,H,W", TASK_CONV_CASES)
def test_conv3x3_tasks_equals_one_launch_per_task(T, n, Ci, Co, H, W, pad):
    if pad == 0 and min(H, W) < 3:
        pytest.skip("no output")
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n * T, Ci, H, W, generator=g).to(DEV)
    w = (torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)).to(DEV)
    b = torch.randn(T, Co, generator=g).to(DEV)
    y = hip_ops.conv3x3_tasks(x, w, b, 0, 0.2, pad)
    gy = torch.randn(y.shape, generator=g).to(DEV)
    gx = hip_ops.conv3x3_tasks(gy, w, None, 1, 1.0, pad)
    for t in range(T):
        sel = torch.arange(t, n * T, T, device=DEV)            # sample-major: task t owns samples t, t+T, ...
        yt = hip_ops.conv3x3(x[sel], w[t], b[t], 0, 0.2, pad)
        assert _rel(y[sel], yt) < 2e-6, (t, 'forward')           # same kernel and filters (deep layers may split the reduction differently)
        gxt = hip_ops.conv3x3(gy[sel], w[t], None, 1, 1.0, pad)
        assert _rel(gx[sel], gxt) < 2e-6, (t, 'data gradient')
    ref = torch.nn.functional.leaky_relu(hip_ops.conv2d_tasks(x, w, b, 1, pad, 1), 0.2)
    assert _rel(y, ref) < 2e-5


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("T,n,Ci,Co,H,W", [c for c in TASK_CONV_CASES if c[2] >= 16])
def test_conv3x3_wgrad_tasks_equals_per_task_gradients(T, n, Ci, Co, H, W, pad):
    if pad == 0 and min(H, W) < 3:
        pytest.skip("no output")
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n * T, Ci, H, W, generator=g).to(DEV)
    gz = torch.randn(n * T, Co, H + 2 * pad - 2, W + 2 * pad - 2, generator=g).to(DEV)
    gw = hip_ops.conv3x3_wgrad_tasks(x, gz, T, pad)
    again = hip_ops.conv3x3_wgrad_tasks(x, gz, T, pad)
    assert torch.equal(gw, again)                                  # deterministic
    for t in range(T):
        sel = torch.arange(t, n * T, T, device=DEV)
        want = torch.ops.aten.convolution_backward(gz[sel].double(), x[sel].double(), torch.zeros(Co, Ci, 3, 3, device=DEV).double(), None,
                                                   [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        assert _rel(gw[t], want.float()) < 2e-5, t


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("T,n,Ci,Co,H,W,k,pad", [(4, 2, 32, 32, 48, 64, 3, 1), (4, 2, 64, 64, 12, 16, 3, 1), (3, 1, 6, 16, 20, 24, 5, 2),
                                                   (2, 2, 192, 12, 1, 1, 1, 0), (4, 2, 51, 51, 34, 30, 3, 0)])
def test_conv_bias_act_tasks_matches_per_task_torch(T, n, Ci, Co, H, W, k, pad, slope):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n * T, Ci, H, W, generator=g).to(DEV).requires_grad_()
    w = (torch.randn(T, Co, Ci, k, k, generator=g) / (k * Ci ** 0.5)).to(DEV).requires_grad_()
    b = torch.randn(T, Co, generator=g).to(DEV).requires_grad_()
    y = hip_ops.conv_bias_act_tasks(x, w, b, 1, pad, 1, slope)
    co = torch.randn(y.shape, generator=g).to(DEV)
    gx, gw, gb = torch.autograd.grad((y * co).sum(), [x, w, b])
    xr, wr, br = (t.detach().double().requires_grad_() for t in (x, w, b))
    yr = hip_ops.conv2d_tasks(xr, wr, br, 1, pad, 1)
    yr = yr if slope == 1.0 else torch.nn.functional.leaky_relu(yr, slope)
    gxr, gwr, gbr = torch.autograd.grad((yr * co.double()).sum(), [xr, wr, br])
    assert _rel(y, yr.float()) < 2e-5
    assert _rel(gx, gxr.float()) < 2e-5 and _rel(gw, gwr.float()) < 5e-5 and _rel(gb, gbr.float()) < 2e-5
    assert gw.shape == w.shape and gb.shape == b.shape


@pytest.mark.parametrize("kind", [0, 1])
def test_per_sample_losses(kind):
    g = torch.Generator().manual_seed(3)
    a = torch.rand(8, 3, 64, 72, generator=g).to(DEV).requires_grad_()
    b = torch.rand(8, 3, 64, 72, generator=g).to(DEV)
    fn = hip_ops.l1_loss_per_sample if kind == 0 else hip_ops.mse_loss_per_sample
    got = fn(a, b)
    want = ((a - b).abs() if kind == 0 else (a - b).pow(2)).flatten(1).mean(1)
    assert got.shape == (8,) and _rel(got, want.detach()) < 1e-6
    co = torch.randn(8, generator=g).to(DEV)
    ga, = torch.autograd.grad((got * co).sum(), a)
    gr, = torch.autograd.grad((want * co).sum(), a)
    assert _rel(ga, gr) < 1e-6
    assert torch.equal(fn(a, b), got)                              # fixed-order reduction: bit-reproducible


# ---------------------------------------------------------------------------------------------
# direct K x K convolution on split-bf16 MFMAs (csrc/convk.hip, csrc/convk_wgrad.hip): fp32-equivalent arithmetic, so it is
# held to a float64 CPU convolution at fp32-rounding bounds (a CPU fp32 convolution differs from float64 by 2e-7 .. 1e-6 on
# these shapes); ragged tiles, channel tails, every padding, several tasks
# ---------------------------------------------------------------------------------------------
CONVK_CASES = [  # K, Ci, Co, H, W, pad, T, N
    (3, 6, 32, 20, 40, 1, 1, 1), (3, 64, 51, 17, 33, 1, 1, 2), (3, 51, 51, 18, 50, 0, 1, 1), (3, 128, 64, 12, 16, 1, 4, 8),
    (3, 24, 40, 9, 70, 2, 1, 1), (5, 6, 64, 32, 32, 2, 1, 2), (5, 64, 128, 16, 48, 2, 2, 2), (5, 64, 3, 24, 40, 2, 1, 2),
    (5, 20, 24, 11, 13, 0, 1, 1), (7, 6, 32, 24, 40, 3, 1, 1), (7, 32, 32, 16, 36, 3, 2, 2), (7, 20, 2, 10, 12, 6, 1, 1),
    (3, 1, 1, 1, 1, 1, 1, 1), (5, 3, 17, 33, 65, 4, 1, 1),
    # >= 192 output channels: the weight gradient's 4-tile variant (with SAVFI_WGRAD_NG=2: 8-wave workgroups on 64 x 32 channels where
    # Ci >= 32); ragged channel blocks, T > 1, a map smaller than a unit
    (3, 192, 192, 33, 47, 1, 1, 1), (3, 200, 208, 20, 40, 1, 2, 4), (3, 64, 256, 12, 16, 0, 1, 2), (3, 40, 192, 3, 5, 1, 1, 1), (3, 24, 192, 9, 33, 1, 1, 1),
]


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("K,Ci,Co,H,W,pad,T,N", CONVK_CASES)
def test_convk_forward_data_and_weight_gradient_match_float64(K, Ci, Co, H, W, pad, T, N, precise):
    g = torch.Generator().manual_seed(K * 1000 + Ci + Co)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(T, Co, Ci, K, K, generator=g) / (K * math.sqrt(Ci))
    b = torch.randn(T, Co, generator=g)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    gy = torch.randn(N, Co, Ho, Wo, generator=g)
    pf, pb = hip_ops.convk_filters(w.to(DEV), True, True)
    y = hip_ops.convk_tasks_pre(x.to(DEV), pf, T, Ci, Co, K, b.to(DEV), 0, 0.2, pad, precise).cpu().double()
    gx = hip_ops.convk_tasks_pre(gy.to(DEV), pb, T, Ci, Co, K, None, 1, 1.0, pad, precise).cpu().double()
    gw = hip_ops.convk_wgrad_tasks(x.to(DEV), gy.to(DEV), T, K, pad, precise).cpu().double()
    gw2 = hip_ops.convk_wgrad_tasks(x.to(DEV), gy.to(DEV), T, K, pad, precise).cpu().double()
    xd, wd, bd, gd = x.double(), w.double(), b.double(), gy.double()
    z = torch.cat([F.conv2d(xd[n:n + 1], wd[n % T], bd[n % T], padding=pad) for n in range(N)], 0)
    ref = torch.where(z > 0, z, 0.2 * z)
    gref = torch.cat([F.conv_transpose2d(gd[n:n + 1], wd[n % T], padding=pad) for n in range(N)], 0)
    wref = torch.stack([torch.nn.grad.conv2d_weight(xd[t::T], (Co, Ci, K, K), gd[t::T], padding=pad) for t in range(T)], 0)
    assert y.shape == ref.shape and gx.shape == (N, Ci, H, W) and gw.shape == wref.shape
    assert _rel(y, ref) < 3e-6 and _rel(gx, gref) < 3e-6 and _rel(gw, wref) < 3e-6
    assert torch.equal(gw, gw2)          # fixed-order reduction of the partial blocks: bit-reproducible


def test_convk_precise_mode_is_closer_to_float64_than_a_cpu_float32_convolution():
    """`precise` (cross terms in their own accumulators): on a long reduction (K = 25 * 192) the result is closer to float64
    than the single-accumulator form and not further than the CPU's blocked fp32 convolution."""
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 192, 24, 40, generator=g).relu()
    w = torch.randn(1, 64, 192, 5, 5, generator=g) * 0.05
    ref = F.conv2d(x.double(), w[0].double(), padding=2)
    cpu32 = F.conv2d(x, w[0], padding=2).double()
    pf, _ = hip_ops.convk_filters(w.to(DEV), True, False)
    err = {p: (hip_ops.convk_tasks_pre(x.to(DEV), pf, 1, 192, 64, 5, None, 0, 1.0, 2, p).cpu().double() - ref).abs().mean().item() for p in (False, True)}
    err_cpu = (cpu32 - ref).abs().mean().item()
    assert err[True] < 0.6 * err[False] and err[True] < 1.5 * err_cpu, (err, err_cpu)


def test_convk_one_hot_filter_reproduces_the_input_bit_for_bit():
    """The split is error-free: a filter that is 1 at one tap of one channel copies that (shifted) channel exactly."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(1, 16, 20, 33, generator=g) * torch.logspace(-6, 6, 16).view(1, 16, 1, 1)).to(DEV)
    w = torch.zeros(1, 16, 16, 5, 5)
    for c in range(16):
        w[0, c, (5 * c) % 16, c % 5, (c // 5) % 5] = 1.0
    pf, _ = hip_ops.convk_filters(w.to(DEV), True, False)
    y = hip_ops.convk_tasks_pre(x, pf, 1, 16, 16, 5, None, 0, 1.0, 2)
    ref = F.conv2d(x.cpu().double(), w[0].double(), padding=2).float()
    assert torch.equal(y.cpu(), ref)


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("shape,k,pad,co,bias", [((2, 6, 40, 48), 5, 2, 64, False), ((1, 64, 32, 32), 5, 2, 3, True), ((2, 6, 24, 40), 7, 3, 32, True),
                                                 ((1, 64, 32, 64), 3, 1, 64, True), ((1, 128, 16, 16), 3, 1, 256, False)])
def test_conv_bias_act_on_the_direct_kernel_matches_torch_autograd(slope, shape, k, pad, co, bias):
    """hip_ops.conv_bias_act routed to the split-bf16 kernels (5x5 / 7x7 always, 3x3 with direct=True): value, data gradient,
    weight gradient, bias gradient against plain torch ops in float64."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(co, shape[1], k, k, generator=g) / (k * math.sqrt(shape[1]))
    b = torch.randn(co, generator=g) if bias else None
    leaves = [t.to(DEV).requires_grad_() for t in (x, w)] + ([b.to(DEV).requires_grad_()] if bias else [])
    assert hip_ops.convk_eligible(leaves[0], leaves[1], 1, pad, 1, 1, True)
    y = hip_ops.conv_bias_act(leaves[0], leaves[1], leaves[2] if bias else None, 1, pad, 1, 1, slope, True, None)
    gy = torch.randn(y.shape, generator=g)
    grads = torch.autograd.grad(y, leaves, gy.to(DEV))
    ref_leaves = [t.double().requires_grad_() for t in (x, w)] + ([b.double().requires_grad_()] if bias else [])
    z = F.conv2d(ref_leaves[0], ref_leaves[1], ref_leaves[2] if bias else None, padding=pad)
    yr = torch.where(z > 0, z, slope * z)
    rgrads = torch.autograd.grad(yr, ref_leaves, gy.double())
    assert _rel(y.detach().cpu().double(), yr.detach()) < 3e-6
    for a, r in zip(grads, rgrads):
        assert _rel(a.cpu().double(), r) < 5e-6


@pytest.mark.parametrize("T,n,Ci,Co,H,W,k,pad", [(4, 2, 64, 64, 32, 32, 3, 1), (3, 1, 6, 16, 20, 24, 5, 2), (2, 2, 32, 32, 24, 40, 7, 3)])
def test_conv_bias_act_tasks_on_the_direct_kernel_matches_per_task_torch(T, n, Ci, Co, H, W, k, pad):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(n * T, Ci, H, W, generator=g)
    w = torch.randn(T, Co, Ci, k, k, generator=g) / (k * math.sqrt(Ci))
    b = torch.randn(T, Co, generator=g)
    xg, wg, bg = (t.to(DEV).requires_grad_() for t in (x, w, b))
    assert hip_ops.convk_eligible(xg, wg, 1, pad, 1, 1, True)
    y = hip_ops.conv_bias_act_tasks(xg, wg, bg, 1, pad, 1, 0.1, True)
    gy = torch.randn(y.shape, generator=g)
    grads = torch.autograd.grad(y, (xg, wg, bg), gy.to(DEV))
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    z = torch.cat([F.conv2d(xr[s:s + 1], wr[s % T], br[s % T], padding=pad) for s in range(n * T)], 0)
    yr = torch.where(z > 0, z, 0.1 * z)
    rgrads = torch.autograd.grad(yr, (xr, wr, br), gy.double())
    assert _rel(y.detach().cpu().double(), yr.detach()) < 3e-6
    for a, r in zip(grads, rgrads):
        assert _rel(a.cpu().double(), r) < 5e-6


def test_own_weight_filters_are_cached_per_weight_version():
    """A module's own parameter is packed once per version: the second pass reuses the buffers, an in-place update repacks."""
    cache = {}
    w = torch.nn.Parameter(torch.randn(64, 64, 5, 5, device=DEV) / 40)
    x = torch.randn(1, 64, 32, 32, device=DEV)
    y1 = hip_ops.conv_bias_act(x, w, None, 1, 2, 1, 1, 1.0, False, cache)
    n1 = len(cache)
    y2 = hip_ops.conv_bias_act(x, w, None, 1, 2, 1, 1, 1.0, False, cache)
    assert n1 == 1 and len(cache) == 1 and torch.equal(y1, y2)
    with torch.no_grad():
        w.mul_(2.0)
    y3 = hip_ops.conv_bias_act(x, w, None, 1, 2, 1, 1, 1.0, False, cache)
    assert len(cache) == 2 and _rel(y3.detach(), 2 * y1.detach()) < 1e-6


@pytest.mark.parametrize("N,T,C,Cr,H,W", [(2, 1, 192, 12, 16, 16), (4, 2, 192, 12, 12, 20), (1, 1, 64, 4, 33, 47), (3, 3, 16, 2, 5, 7), (2, 1, 320, 20, 8, 8),
                                          (2, 1, 192, 12, 96, 160), (1, 1, 192, 12, 90, 161)])
def test_channel_attention_residual_matches_the_composed_ops(N, T, C, Cr, H, W):
    """CAIN's RCAB tail (pool -> 1x1 -> ReLU -> 1x1 -> sigmoid -> scale -> + skip) as the fused savfi op against the reference's
    composition (model_utils.py:931-990) in float64: value, attention, and the gradients of both maps and all four parameters;
    per-task weight sets (sample n uses set n % T)."""
    g = torch.Generator().manual_seed(N * 100 + C)
    t, x = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    w1, b1 = torch.randn(T, Cr, C, 1, 1, generator=g) / math.sqrt(C), torch.randn(T, Cr, generator=g) * 0.1
    w2, b2 = torch.randn(T, C, Cr, 1, 1, generator=g) / math.sqrt(Cr), torch.randn(T, C, generator=g) * 0.1
    gout = torch.randn(N, C, H, W, generator=g)
    leaves = [v.to(DEV).requires_grad_() for v in (t, x, w1, b1, w2, b2)]
    args = leaves if T > 1 else leaves[:2] + [v[0] for v in leaves[2:]]
    out, y = hip_ops.channel_attention_residual(*args)
    grads = torch.autograd.grad(out, leaves, gout.to(DEV))
    ref = [v.double().requires_grad_() for v in (t, x, w1, b1, w2, b2)]
    rt, rx, rw1, rb1, rw2, rb2 = ref
    outs, ys = [], []
    for n in range(N):
        k = n % T
        s = rt[n:n + 1].mean((2, 3), keepdim=True)
        yy = torch.sigmoid(F.conv2d(F.relu(F.conv2d(s, rw1[k], rb1[k])), rw2[k], rb2[k]))
        ys.append(yy)
        outs.append(rt[n:n + 1] * yy + rx[n:n + 1])
    rout = torch.cat(outs, 0)
    rgrads = torch.autograd.grad(rout, ref, gout.double())
    assert _rel(out.detach().cpu().double(), rout.detach()) < 2e-6
    assert _rel(y.detach().cpu().double(), torch.cat(ys, 0).detach()) < 2e-6
    for a, r, name in zip(grads, rgrads, ("t", "x", "w1", "b1", "w2", "b2")):
        assert _rel(a.cpu().double(), r) < 2e-5, name


@pytest.mark.parametrize("N,Ci,Co,H,W,K", [(2, 64, 64, 40, 56, 3), (1, 192, 192, 33, 47, 3), (2, 8, 64, 30, 41, 5)])
def test_conv_with_mirrored_border_equals_reflection_pad_plus_conv(N, Ci, Co, H, W, K):
    """MetaConvNorm fused: conv_bias_act(reflect=True) == conv2d(ReflectionPad2d(K // 2)(x)) + bias + LeakyReLU, forward, data
    gradient (full data gradient folded by savfi_reflect_pad_bwd_f32) and weight gradient (mirrored staging), against float64."""
    g = torch.Generator().manual_seed(11 * H + K)
    p = K // 2
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, K, K, generator=g) / (K * Ci ** 0.5)
    b = torch.randn(Co, generator=g)
    gy = torch.randn(N, Co, H, W, generator=g)
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(torch.nn.functional.pad(xr, (p,) * 4, mode='reflect'), wr, br), 0.2)
    ref.backward(gy.double())
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    assert hip_ops.convk_reflect_eligible(xd, wd, p)
    out = hip_ops.conv_bias_act(xd, wd, bd, 1, p, 1, 1, 0.2, False, None, True)
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    for got, want in ((out, ref), (xd.grad, xr.grad), (wd.grad, wr.grad), (bd.grad, br.grad)):
        assert _rel(got.detach().cpu().double(), want.detach()) < 5e-6


def test_reflect_pad_backward_is_the_adjoint_for_every_pad():
    for (H, W, p) in ((9, 13, 1), (7, 6, 3), (4, 5, 2), (2, 3, 1)):
        gp = torch.randn(3, 2, H + 2 * p, W + 2 * p)
        x = torch.zeros(3, 2, H, W, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.pad(x, (p,) * 4, mode='reflect').backward(gp.double())
        got = hip_ops.reflect_pad_bwd(gp.to(DEV), p)
        assert _rel(got.cpu().double(), x.grad) < 1e-6


def test_filters_of_many_layers_in_one_launch_equal_the_single_layer_calls():
    """savfi_convk_filters_multi_f32 / savfi_conv3x3_filters_multi_f32 (hip_ops._filters_multi): bit-identical to one call per layer,
    for mixed shapes, task counts and forward-only / backward-only jobs."""
    g = torch.Generator().manual_seed(21)
    ws = [torch.randn(*shape, generator=g).to(DEV) for shape in
          ((64, 64, 3, 3), (4, 32, 6, 3, 3), (51, 64, 3, 3), (2, 128, 64, 3, 3), (192, 192, 3, 3))]
    wants = [(True, True), (True, False), (False, True), (True, True), (True, True)]
    for kind, single in (('convk', hip_ops.convk_filters), ('wino', hip_ops.conv3x3_filters)):
        multi = hip_ops._filters_multi(kind, [(w, f, b) for w, (f, b) in zip(ws, wants)])
        for w, (f, b), (mf, mb) in zip(ws, wants, multi):
            hip_ops._prepacked.clear()
            sf, sb = single(w, f, b)
            for one, many in ((sf, mf), (sb, mb)):
                assert (one is None) == (many is None)
                if one is not None:
                    assert torch.equal(one.view(-1), many.view(-1)[:one.numel()])
    w5 = torch.randn(64, 6, 5, 5, generator=g).to(DEV)
    (mf, mb), = hip_ops._filters_multi('convk', [(w5, True, True)])
    sf, sb = hip_ops.convk_filters(w5, True, True)
    assert torch.equal(sf.view(-1), mf.view(-1)[:sf.numel()]) and torch.equal(sb.view(-1), mb.view(-1)[:sb.numel()])


def test_filters_prepared_after_an_update_are_found_and_follow_the_weight_version():
    """hip_ops.filters_after_update: the second update of a list of the same shapes packs what the first one's layers used; a hit
    needs the same tensor AND version (an in-place change of the fast weight invalidates it)."""
    g = torch.Generator().manual_seed(22)
    hip_ops._pack_plans.clear()
    shapes = ((64, 64, 3, 3), (64,), (128, 64, 3, 3))
    x = torch.randn(2, 64, 40, 48, generator=g).to(DEV)

    def step():
        outs = [torch.randn(*s, generator=g).to(DEV) for s in shapes]
        hip_ops.filters_after_update(outs)
        return outs
    outs = step()                                   # first update: no plan yet
    assert not hip_ops._prepacked
    y1 = hip_ops.conv_bias_act(x, outs[0], outs[1], 1, 1, 1, 1, 0.0)          # learns: index 0 is packed for the direct kernel
    outs = step()                                   # second update: packed straight away
    assert ('convk', outs[0].data_ptr()) in hip_ops._prepacked
    ref = torch.nn.functional.relu(torch.nn.functional.conv2d(x.double().cpu(), outs[0].double().cpu(), outs[1].double().cpu(), padding=1))
    y2 = hip_ops.conv_bias_act(x, outs[0], outs[1], 1, 1, 1, 1, 0.0)
    assert _rel(y2.cpu().double(), ref) < 5e-6
    with torch.no_grad():
        outs[0].mul_(2.0)                           # version bump: the prepared filters no longer match
    assert hip_ops._prepacked_filters('convk', outs[0], True, False) is None
    y3 = hip_ops.conv_bias_act(x, outs[0], outs[1] * 2, 1, 1, 1, 1, 0.0)
    assert _rel(y3.cpu().double(), 2 * ref) < 5e-6
    hip_ops._prepacked.clear()
    del y1


# --------------------------------------------------------------------------------------------
# sub_mean (reference model_utils.py:11-15): per-plane mean removal
# --------------------------------------------------------------------------------------------
SUB_MEAN_SHAPES = [(1, 3, 64, 64), (2, 3, 37, 45), (1, 3, 720, 1280), (3, 2, 1, 5), (1, 1, 129, 127)]


@pytest.mark.parametrize("shape", SUB_MEAN_SHAPES)
def test_sub_mean_matches_the_two_stage_mean(shape):
    """float64 reference: mean over H, then over W.  Tolerance: 4 ulp of the mean's magnitude on the mean (fp32 sums of <= 1M
    terms in blocks of 16384) and on the difference."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(*shape, generator=g) + 0.25
    ref_mean = x.double().mean(2, keepdim=True).mean(3, keepdim=True)
    out, mean = hip_ops.sub_mean(x.to(DEV))
    assert tuple(mean.shape) == (shape[0], shape[1], 1, 1)
    assert (mean.cpu().double() - ref_mean).abs().max().item() < 5e-7
    assert (out.cpu().double() - (x.double() - ref_mean)).abs().max().item() < 5e-7


def test_sub_mean_gradients_and_double_backward():
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 9, 11, generator=g)
    wo, wm = torch.randn(2, 3, 9, 11, generator=g), torch.randn(2, 3, 1, 1, generator=g)

    def ref(t):
        m = t.mean(2, keepdim=True).mean(3, keepdim=True)
        return t - m, m

    xs = [x.clone().double().requires_grad_(True), x.clone().to(DEV).requires_grad_(True)]
    grads = []
    for t, f in zip(xs, (ref, hip_ops.sub_mean)):
        o, m = f(t)
        loss = (o * wo.to(t)).sum() + (m * wm.to(t)).sum() + (o * o).sum() * 0.5
        gx, = torch.autograd.grad(loss, t, create_graph=True)
        ggx, = torch.autograd.grad((gx * gx).sum(), t)      # through the backward: second-order MAML differentiates it
        grads.append((gx.detach().cpu().double(), ggx.detach().cpu().double()))
    assert _rel(grads[1][0], grads[0][0]) < 1e-5
    assert _rel(grads[1][1], grads[0][1]) < 1e-5
    # only the mean is used
    t = x.clone().to(DEV).requires_grad_(True)
    gx, = torch.autograd.grad((hip_ops.sub_mean(t)[1] * wm.to(DEV)).sum(), t)
    assert _rel(gx.cpu(), (wm / (9 * 11)).expand(2, 3, 9, 11)) < 1e-6


def test_sub_mean_in_a_replayed_graph_follows_its_inputs():
    """The reason this op exists: at 3 x 720 x 1280 ATen's x.mean(2) runs several workgroups per output behind a hipMemsetAsync'ed
    semaphore array, and a memset node of a captured hipGraph clears only in the graph's first launch on ROCm 7.2
    (tools/graph_memset_probe.py) -- from the second replay on the captured mean is stale.  The savfi op is replayed with new frame
    contents and must match its own eager result bit for bit every time."""
    x = torch.rand(1, 3, 720, 1280, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.sub_mean(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, mean = hip_ops.sub_mean(x)
    for it in range(4):
        x.uniform_(0.0, 1.0 + it)
        graph.replay()
        want_out, want_mean = hip_ops.sub_mean(x)
        assert torch.equal(mean, want_mean) and torch.equal(out, want_out), it
        assert abs(mean.mean().item() - (1.0 + it) / 2) < 1e-2


# --------------------------------------------------------------------------------------------
# bias + activation epilogue kernels on planes that are not a multiple of 4 floats (SepConv's windowed tail: 137 x 233)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(2, 5, 137, 233), (1, 3, 7, 9), (3, 2, 1, 1), (2, 4, 64, 66), (1, 2, 129, 65)])
@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_bias_act_kernels_on_odd_planes(N, C, H, W, slope, shift):
    """savfi_bias_act_fwd_f32 / savfi_bias_act_bwd_f32 straight through the C ABI, operands starting `shift` floats past an
    aligned address (all three the same shift -> vector body behind a peel; gz shifted differently -> scalar path).  The
    activation gradient is exact; the bias gradient is a sum of up to 64k terms: 1e-5 of its abs-sum scale."""
    lib = _hip.lib()
    g = torch.Generator().manual_seed(9)
    n = N * C * H * W

    def shifted(t, s):
        buf = torch.empty(n + 8, device=DEV)
        view = buf[s:s + n]
        view.copy_(t.reshape(-1).to(DEV))
        return buf, view

    z = torch.randn(N, C, H, W, generator=g)
    b = torch.randn(C, generator=g)
    want = z + b.view(1, C, 1, 1)
    want = torch.where(want > 0, want, slope * want)
    zb, zv = shifted(z, shift)
    _hip.check(lib.savfi_bias_act_fwd_f32(zv.data_ptr(), b.to(DEV).data_ptr(), N, C, H * W, slope, _hip.current_stream()), "fwd")
    assert torch.equal(zv.cpu().view(N, C, H, W), want)

    gy = torch.randn(N, C, H, W, generator=g)
    y = torch.randn(N, C, H, W, generator=g)
    want_gz = torch.where(y > 0, gy, slope * gy)
    for gz_shift in (shift, (shift + 1) % 4):
        _, gyv = shifted(gy, shift)
        _, yv = shifted(y, shift)
        gzb = torch.zeros(n + 8, device=DEV)
        gzv = gzb[gz_shift:gz_shift + n]
        gb = torch.empty(C, device=DEV)
        scratch = torch.empty(int(lib.savfi_bias_act_scratch_floats(N, C, H * W)), device=DEV)
        _hip.check(lib.savfi_bias_act_bwd_f32(gyv.data_ptr(), yv.data_ptr(), gzv.data_ptr(), gb.data_ptr(), scratch.data_ptr(),
                                              N, C, H * W, slope, _hip.current_stream()), "bwd")
        assert torch.equal(gzv.cpu().view(N, C, H, W), want_gz)
        assert float(gzb[:gz_shift].abs().sum()) == 0 and float(gzb[gz_shift + n:].abs().sum()) == 0      # nothing outside
        ref = want_gz.double().sum((0, 2, 3))
        assert (gb.cpu().double() - ref).abs().max().item() <= 1e-5 * want_gz.double().abs().sum((0, 2, 3)).max().item() + 1e-6


@pytest.mark.parametrize("shape,pad", [((2, 5, 16, 16), 1), ((1, 3, 7, 9), 2), ((3, 2, 2, 2), 1), ((1, 4, 33, 18), 3), ((2, 24, 96, 160), 1),
                                       ((1, 2, 31, 45), 1), ((1, 1, 5, 4), 3)])
def test_reflect_pad_op_has_atens_values_and_gradient(shape, pad):
    """hip_ops.reflect_pad = nn.ReflectionPad2d (savfi_reflect_pad_fwd_f32: the same values as ATen's kernel, bit for bit, on aligned,
    8-byte and odd row phases) with the gather adjoint: the gradient of a weighted sum against
    autograd through F.pad, on maps down to 2 x 2 (every border position folds twice).  Exact up to summation order: 1e-6."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=g).to(DEV)
    wgt = torch.randn(shape[0], shape[1], shape[2] + 2 * pad, shape[3] + 2 * pad, generator=g).to(DEV)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    ya = hip_ops.reflect_pad(a, pad)
    yb = F.pad(b, (pad,) * 4, mode='reflect')
    assert torch.equal(ya, yb)
    ga, = torch.autograd.grad((ya * wgt).sum(), a)
    gb, = torch.autograd.grad((yb * wgt).sum(), b)
    assert _rel(ga, gb) < 1e-6
    # the padded map and the map itself for a connection round the layer: both cotangents in the fold's pass, the same additions as
    # autograd's own (fold, then + skip): bit-equal; and each output alone
    w2 = torch.randn(*shape, generator=g).to(DEV)
    c = x.clone().requires_grad_(True)
    yc, xs = hip_ops.reflect_pad_with_skip(c, pad)
    assert torch.equal(yc, yb) and torch.equal(xs, x)
    gc, = torch.autograd.grad((yc * wgt).sum() + (xs * w2).sum(), c, retain_graph=True)
    assert torch.equal(gc, ga + w2)
    assert torch.equal(torch.autograd.grad((yc * wgt).sum(), c, retain_graph=True)[0], ga)
    assert torch.equal(torch.autograd.grad((xs * w2).sum(), c)[0], w2)


def test_mt_copy_is_a_bitwise_copy_over_many_tensors():
    """hip_ops.mt_copy / mt_clone (the multi-tensor scale kernel with gamma = 1): 130 tensors of ragged sizes -- three launch groups --
    including -0.0, infinities, NaN and denormals, compared as bit patterns; a shape-changing (same numel) destination; and the
    fallback for non-float32 lists."""
    g = torch.Generator().manual_seed(3)
    srcs = [torch.randn(int(n), generator=g) for n in torch.randint(1, 5000, (130,), generator=g)]
    srcs[0][:6] = torch.tensor([-0.0, float('inf'), float('-inf'), float('nan'), 1e-42, -1e-45])
    srcs = [s.to(DEV) for s in srcs]
    srcs[5] = torch.randn(6, 7, generator=g).to(DEV).t()                     # non-contiguous source
    dsts = [torch.full_like(s, 9.0, memory_format=torch.contiguous_format) for s in srcs]
    dsts[7] = torch.full((1, srcs[7].numel()), 9.0, device=DEV)               # [1, n] static buffer for an [n] parameter
    hip_ops.mt_copy(dsts, srcs)
    for d, s in zip(dsts, srcs):
        assert torch.equal(d.reshape(-1).view(torch.int32), s.contiguous().reshape(-1).view(torch.int32))
    for c, s in zip(hip_ops.mt_clone(srcs), srcs):
        assert c.shape == s.shape and c.data_ptr() != s.data_ptr()
        assert torch.equal(c.contiguous().view(-1).view(torch.int32), s.contiguous().view(-1).view(torch.int32))
    ints = [torch.arange(5, device=DEV), torch.arange(3, device=DEV)]
    outs = [torch.zeros(5, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)]
    hip_ops.mt_copy(outs, ints)
    assert all(torch.equal(o, i) for o, i in zip(outs, ints))


@pytest.mark.parametrize("N,T,Ci,Co,H,W,pad", [(8, 4, 32, 32, 96, 128, 1), (4, 1, 51, 51, 66, 130, 0), (8, 4, 64, 40, 48, 64, 1), (2, 2, 20, 70, 37, 53, 1)])
def test_winograd_weight_gradient_hands_out_the_bias_gradient(N, T, Ci, Co, H, W, pad):
    """savfi_conv3x3_wgrad_wino_tasks_bias_f32: the weight gradient is bit for bit the one of savfi_conv3x3_wgrad_wino_tasks_f32, and
    gb[t][co] is the sum of the cotangent over the samples n % T == t and the map (float64 reference, fp32 rounding of ~1e5 terms)"""
    lib, st = _hip.lib(), _hip.current_stream()
    g = torch.Generator().manual_seed(N * 1000 + Co)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x = torch.randn(N, Ci, H, W, generator=g).to(DEV)
    gz = torch.randn(N, Co, Ho, Wo, generator=g).to(DEV)
    ws0 = torch.empty(int(lib.savfi_conv3x3_wgrad_wino_tasks_workspace_floats(N, T, Ci, Co, H, W, pad)), device=DEV)
    ws1 = torch.empty(int(lib.savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats(N, T, Ci, Co, H, W, pad)), device=DEV)
    assert ws1.numel() > ws0.numel()
    gw0 = torch.full((T, Co, Ci, 3, 3), float('nan'), device=DEV)
    gw1, gb = torch.full_like(gw0, float('nan')), torch.full((T, Co), float('nan'), device=DEV)
    _hip.check(lib.savfi_conv3x3_wgrad_wino_tasks_f32(x.data_ptr(), gz.data_ptr(), gw0.data_ptr(), ws0.data_ptr(), N, T, Ci, Co, H, W, pad, st), "plain")
    _hip.check(lib.savfi_conv3x3_wgrad_wino_tasks_bias_f32(x.data_ptr(), gz.data_ptr(), gw1.data_ptr(), gb.data_ptr(), ws1.data_ptr(), N, T, Ci, Co, H, W, pad, st), "with bias")
    torch.cuda.synchronize()
    assert torch.equal(gw0, gw1)
    ref = gz.double().view(N // T, T, Co, -1).sum((0, 3))
    assert (gb.double() - ref).abs().max().item() <= 1e-5 * gz.double().abs().view(N // T, T, Co, -1).sum((0, 3)).max().item()
    assert lib.savfi_conv3x3_wgrad_wino_tasks_bias_f32(x.data_ptr(), gz.data_ptr(), gw1.data_ptr(), None, ws1.data_ptr(), N, T, Ci, Co, H, W, pad, st) == -1


@pytest.mark.parametrize("N,T,Ci,Co,H,W,pad,reflect", [
    (8, 4, 64, 64, 48, 64, 1, 0), (4, 1, 51, 51, 66, 130, 0, 0), (2, 2, 70, 100, 37, 53, 1, 0), (2, 1, 192, 192, 33, 47, 1, 1),
    (3, 3, 64, 128, 5, 200, 2, 0), (1, 1, 48, 48, 1, 1, 1, 0), (6, 2, 128, 64, 31, 33, 1, 0),
    (2, 1, 192, 192, 18, 18, 0, 0), (1, 1, 64, 64, 8, 14, 1, 0), (4, 2, 192, 192, 16, 16, 1, 1)])      # the small maps of CAIN at 64 x 64
def test_all_taps_weight_gradient_matches_float64_and_hands_out_the_bias_gradient(N, T, Ci, Co, H, W, pad, reflect):
    """convk_wgrad3_ring (3 x 3 layers of >= 48 -> 48 channels: all nine taps per wave, input rows on a ring): against a float64 weight gradient
    on maps with odd row counts, ragged channel blocks, several column segments, every padding, a mirrored border and T > 1; with the bias
    sums on (savfi_convk_wgrad_tasks_bias_f32) the weight gradient is bit for bit the same and gb[t][co] is the sum of the cotangent."""
    lib, st = _hip.lib(), _hip.current_stream()
    assert lib.savfi_convk_wgrad_sums_bias(N, T, Ci, Co, H, W, 3, pad) == 1 and lib.savfi_convk_wgrad_sums_bias(N, T, 32, Co, H, W, 3, pad) == 0
    g = torch.Generator().manual_seed(N * 1000 + Co + H)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x = torch.randn(N, Ci, H, W, generator=g)
    gz = torch.randn(N, Co, Ho, Wo, generator=g)
    xd, gd = x.to(DEV), gz.to(DEV)
    gw0 = hip_ops.convk_wgrad_tasks(xd, gd, T, 3, pad, False, bool(reflect))
    gw1, gb = hip_ops.convk_wgrad_tasks(xd, gd, T, 3, pad, False, bool(reflect), want_bias=True)
    assert torch.equal(gw0, gw1)
    xs = F.pad(x.double(), (pad,) * 4, mode='reflect') if reflect else x.double()
    wref = torch.stack([torch.nn.grad.conv2d_weight(xs[t::T], (Co, Ci, 3, 3), gz.double()[t::T], padding=0 if reflect else pad) for t in range(T)], 0)
    assert _rel(gw0.cpu().double(), wref) < 3e-6
    ref = gz.double().view(N // T, T, Co, -1).sum((0, 3))
    assert (gb.cpu().double() - ref).abs().max().item() <= 1e-5 * max(1.0, gz.double().abs().view(N // T, T, Co, -1).sum((0, 3)).max().item())
    ws = torch.empty(int(lib.savfi_convk_wgrad_workspace_floats(N, T, 32, Co, H, W, 3, pad)), device=DEV)
    x32 = torch.zeros(N, 32, H, W, device=DEV)
    assert lib.savfi_convk_wgrad_tasks_bias_f32(x32.data_ptr(), gd.data_ptr(), gw1.data_ptr(), gb.data_ptr(), ws.data_ptr(), N, T, 32, Co, H, W, 3, pad, 0, st) != 0


@pytest.mark.parametrize("shape,geom_kind,slope", [((3, 5, 12, 16), "full", 0.0), ((2, 64, 40, 70), "full", 0.2), ((2, 7, 31, 45), "window", 0.0),
                                                   ((1, 3, 100, 130), "window", 0.0), ((4, 33, 9, 8), "full", 0.0),
                                                   ((1, 2048, 41, 70), "full", 0.2), ((1, 1400, 41, 70), "window", 0.0),
                                                   ((1, 700, 41, 70), "window", 0.2)])
def test_upsample_adjoint_folds_the_producers_relu_derivative(shape, geom_kind, slope):
    """savfi_upsample2x_window_bwd_masked_f32 (all three kernel forms: small maps, the tiled and the streaming one): the adjoint of the
    bilinear x2 times (y > 0 ? 1 : slope) of its own input == the plain adjoint followed by savfi_bias_act_bwd_f32's derivative, bit for bit.
    The form each case runs is the library's own answer (savfi_upsample2x_bwd_form: 0 per pixel, 1 tiled, 8 / 16 / 32 streaming with strips
    of that many rows); the plain adjoint of every form is held to float64 in tests/test_upsample_forms_gpu.py."""
    want_form = {(3, 5, 12, 16): 0, (2, 64, 40, 70): 1, (2, 7, 31, 45): 1, (1, 3, 100, 130): 1, (4, 33, 9, 8): 0,
                 (1, 2048, 41, 70): 32, (1, 1400, 41, 70): 16, (1, 700, 41, 70): 8}[shape]
    assert _hip.lib().savfi_upsample2x_bwd_form(shape[0] * shape[1], shape[2], shape[3]) == want_form
    g = torch.Generator().manual_seed(shape[2] * 7 + shape[3])
    x = torch.randn(*shape, generator=g).to(DEV)
    if geom_kind == "full":
        up = lambda t, sl: hip_ops.upsample_bilinear2x(t, True, sl)
    else:
        N, C, H, W = shape
        full, origin = (H + 9, W + 6), (4, 3)
        oy0, ox0 = 2 * origin[0] + 6, 2 * origin[1] + 6
        win = (oy0, ox0, 2 * H - 14, 2 * W - 14)
        up = lambda t, sl: hip_ops.upsample_bilinear2x_window(t, full, origin, win, True, sl)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = up(xa, None), up(xb, slope)
    assert torch.equal(ya, yb)
    gy = torch.randn(ya.shape, generator=g).to(DEV)
    ga, = torch.autograd.grad(ya, xa, gy)
    gb, = torch.autograd.grad(yb, xb, gy)
    assert torch.equal(gb, hip_ops.mask_by_activation(ga, x, slope))


@pytest.mark.parametrize("shape,slope,use", [((2, 5, 12, 16), 0.0, "both"), ((3, 7, 13, 17), 0.2, "both"), ((2, 32, 64, 96), 0.0, "pool"),
                                             ((1, 3, 9, 8), None, "both"), ((2, 4, 10, 11), 0.0, "skip")])
def test_pool_and_skip_adjoint_is_one_pass_with_the_same_values(shape, slope, use):
    """hip_ops.avg_pool2x2_and_skip: (pool(x), x); its backward = (pool^T(g_pool) + g_skip) * (x > 0 ? 1 : slope) in one kernel
    (savfi_avgpool2x2_bwd_fused_f32) == the three passes it replaces, bit for bit (odd rows / columns, a consumer without gradient)."""
    g = torch.Generator().manual_seed(shape[2] * 31 + shape[3])
    x = torch.randn(*shape, generator=g).to(DEV)
    a = torch.randn(shape[0], shape[1], shape[2] // 2, shape[3] // 2, generator=g).to(DEV)
    b = torch.randn(*shape, generator=g).to(DEV)
    xa = x.clone().requires_grad_()
    pooled, skip = hip_ops.avg_pool2x2_and_skip(xa, slope)
    assert torch.equal(pooled, hip_ops.avg_pool2x2(x)) and torch.equal(skip, x)
    loss = (pooled * a).sum() * (use != "skip") + (skip * b).sum() * (use != "pool")
    got, = torch.autograd.grad(loss, xa)
    xb = x.clone().requires_grad_()
    gp, = torch.autograd.grad((hip_ops.avg_pool2x2(xb) * a).sum(), xb)
    want = gp * (use != "skip") + b * (use != "pool")
    if slope is not None:
        want = hip_ops.mask_by_activation(want, x, slope)
    assert torch.equal(got, want)
