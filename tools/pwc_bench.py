"""Timing of PWC-Net's kernels (csrc/correlation.hip) and of the whole PWCDCNet forward against the same computation composed from torch
ops on the GPU: the correlation forward (LeakyReLU fused) and backward (both gradients) and the warp at the five pyramid-level shapes of
256 x 448 and of 768 x 1280 frames, one sample, and PWCDCNet.forward at both sizes.

    python tools/pwc_bench.py [output file]        (needs the GPU)

How it is measured: every shape is warmed up first; a figure is the median over REPEATS windows of the time between two HIP events
around INNER back-to-back calls on one stream, divided by INNER -- so it includes the launch cost a caller in a loop pays, which is most
of what these small maps cost -- and the minimum window is printed next to it.  "torch" is the composition: 81 shifted multiply-and-mean
steps, stack and leaky_relu for the correlation (autograd of it for the backward); mesh grid, normalisation, two
grid_sample(align_corners=True), threshold and product for the warp; conv2d + leaky_relu, those two and conv_transpose2d for the network.
The fraction of the 8 TB/s HBM peak is the ALGORITHMIC bytes (each operand once: hip_ops.correlation_bytes / pwc_warp_bytes) over the
median time.  There is no speed gate: the figures say what was measured on these shapes, nothing more.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops
from meta_interpolation_amd.dain.PWCNet.PWCNet import PWCDCNet

PEAK = 8.0e12
SIZES = ((256, 448), (768, 1280))
LEVELS = ((2, 32, 5.0), (3, 64, 2.5), (4, 96, 1.25), (5, 128, 0.625), (6, 196, 0.625))       # level, channels, flow scale
REPEATS, WARM = 9, 3
MD, SLOPE = 4, 0.1


def timed(f, inner):
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    windows = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            f()
        b.record()
        torch.cuda.synchronize()
        windows.append(1e3 * a.elapsed_time(b) / inner)
    windows.sort()
    return windows[len(windows) // 2], windows[0]


def correlation_composed(f1, f2, slope=SLOPE):
    H, W = f1.shape[2:]
    p2 = F.pad(f2, (MD, MD, MD, MD))
    out = torch.stack([(f1 * p2[:, :, MD + tj:MD + tj + H, MD + ti:MD + ti + W]).mean(1)
                       for tj in range(-MD, MD + 1) for ti in range(-MD, MD + 1)], 1)
    return F.leaky_relu(out, slope)


def warp_composed(x, flo, scale):
    B, C, H, W = x.shape
    xx = torch.arange(0, W, device=x.device).view(1, -1).repeat(H, 1).view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = torch.arange(0, H, device=x.device).view(-1, 1).repeat(1, W).view(1, 1, H, W).repeat(B, 1, 1, 1)
    vgrid = torch.cat((xx, yy), 1).float() + flo * scale
    vgrid = torch.stack((2.0 * vgrid[:, 0] / max(W - 1, 1) - 1.0, 2.0 * vgrid[:, 1] / max(H - 1, 1) - 1.0), -1)
    output = F.grid_sample(x, vgrid, align_corners=True)
    mask = F.grid_sample(torch.ones_like(x), vgrid, align_corners=True)
    return output * (mask >= 0.9999).to(x.dtype)


def network_composed(net, x):
    """PWCDCNet.forward from torch ops on the module's own parameters (what tests/pwc_ref.py states on the host)."""
    def block(m, t):
        c = m[0]
        return F.leaky_relu(F.conv2d(t, c.weight, c.bias, c.stride, c.padding, c.dilation), SLOPE)

    def bare(c, t):
        return F.conv2d(t, c.weight, c.bias, c.stride, c.padding)

    def up(d, t):
        return F.conv_transpose2d(t, d.weight, d.bias, d.stride, d.padding)

    c1, c2 = [x[:, :3]], [x[:, 3:]]
    for lv in range(1, 7):
        a, aa = ('a', 'aa') if lv < 6 else ('aa', 'a')
        for pyr in (c1, c2):
            t = block(getattr(net, 'conv%d%s' % (lv, a)), pyr[-1])
            pyr.append(block(getattr(net, 'conv%db' % lv), block(getattr(net, 'conv%d%s' % (lv, aa)), t)))
    up_flow = up_feat = None
    for lv, scale in ((6, None), (5, 0.625), (4, 1.25), (3, 2.5), (2, 5.0)):
        f1, f2 = c1[lv], c2[lv]
        if lv == 6:
            t = correlation_composed(f1, f2)
        else:
            t = torch.cat((correlation_composed(f1, warp_composed(f2, up_flow, scale)), f1, up_flow, up_feat), 1)
        for i in range(5):
            t = torch.cat((block(getattr(net, 'conv%d_%d' % (lv, i)), t), t), 1)
        flow = bare(getattr(net, 'predict_flow%d' % lv), t)
        if lv > 2:
            up_flow, up_feat = up(getattr(net, 'deconv%d' % lv), flow), up(getattr(net, 'upfeat%d' % lv), t)
    for i in range(1, 7):
        t = block(getattr(net, 'dc_conv%d' % i), t)
    return flow + bare(net.dc_conv7, t)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("pwc_bench needs the GPU: nothing is measured without one")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def report(op, shape, hip, ref, nbytes=None, note=None):
        rec = dict(op=op, shape="x".join(str(v) for v in shape), hip_median_us=round(hip[0], 1), hip_min_us=round(hip[1], 1),
                   torch_median_us=round(ref[0], 1), torch_min_us=round(ref[1], 1), torch_over_hip=round(ref[0] / hip[0], 2))
        if nbytes is not None:
            rec.update(algorithmic_MB=round(nbytes / 1e6, 3), hbm_peak_fraction=round(nbytes / (hip[0] * 1e-6) / PEAK, 5))
        if note:
            rec["note"] = note
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for H, W in SIZES:
        for lv, C, scale in LEVELS:
            h, w = H >> lv, W >> lv
            shape = (1, C, h, w)
            f1, f2 = torch.randn(shape, device="cuda", generator=g), torch.randn(shape, device="cuda", generator=g)
            gout = torch.randn(1, 81, h, w, device="cuda", generator=g)
            flow = (torch.rand(1, 2, h, w, device="cuda", generator=g) * 4 - 2).contiguous()
            inner = 50 if h * w <= 4096 else 20
            with torch.no_grad():
                hip = timed(lambda: hip_ops.correlation(f1, f2, MD, SLOPE), inner)
                ref = timed(lambda: correlation_composed(f1, f2), max(2, inner // 10))
                report("correlation_fwd", shape, hip, ref, hip_ops.correlation_bytes(1, C, h, w))
                hip = timed(lambda: hip_ops.pwc_warp(f2, flow, scale), inner)
                ref = timed(lambda: warp_composed(f2, flow, scale), max(2, inner // 5))
                report("pwcwarp_fwd", shape, hip, ref, hip_ops.pwc_warp_bytes(1, C, h, w))
            a, b = f1.clone().requires_grad_(), f2.clone().requires_grad_()
            out = hip_ops.correlation(a, b, MD, SLOPE)
            hip = timed(lambda: torch.autograd.grad(out, (a, b), gout, retain_graph=True), inner)
            out_c = correlation_composed(a, b)
            ref = timed(lambda: torch.autograd.grad(out_c, (a, b), gout, retain_graph=True), max(2, inner // 10))
            report("correlation_bwd", shape, hip, ref, hip_ops.correlation_bytes(1, C, h, w, grads=1), note="both gradients")
            del out, out_c
        torch.manual_seed(0)
        net = PWCDCNet().cuda().eval()
        x = torch.rand(1, 6, H, W, device="cuda", generator=g)
        with torch.no_grad():
            hip = timed(lambda: net(x), 3)
            ref = timed(lambda: network_composed(net, x), 3)
        report("PWCDCNet.forward", (1, 6, H, W), hip, ref, note="eager; composed = conv2d + leaky_relu, composed correlation and warp")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("# tools/pwc_bench.py on an MI355X: median (and minimum) over %d windows of back-to-back calls between two HIP events, per call,\n"
                     "# after %d warm-up calls per shape; torch = the same computation composed from torch ops on the GPU.  Fraction of the 8 TB/s HBM\n"
                     "# peak = algorithmic bytes / median time / 8e12.  Measured on these shapes only; no speed gate.\n" % (REPEATS, WARM))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
