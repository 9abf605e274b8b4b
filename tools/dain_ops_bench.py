"""HIP-event timing of DAIN's two ops (csrc/dainwarp.hip) through the C ABI: the four entry points at 256 x 448 and at 720p padded to a
multiple of 64 (768 x 1280), one sample, the adaptive warping with C = 3 (frames) and C = 196 (context features).  For each it prints
the median and minimum time of isolated launches and the fraction of the 8 TB/s HBM peak that the ALGORITHMIC bytes (every operand
once; hip_ops.filterinterp_bytes / depthflowproj_bytes) over the median time amount to.  There is no speed gate on these kernels: the
figures say what was measured, on these shapes, nothing more.

    python tools/dain_ops_bench.py [output file]        (needs the GPU)

Inputs: flows uniform in +-8 pixels (almost every pixel valid, a few holes in the projection), filters N(0, 1/16), depth inverses
log-uniform in [1e-3, 1e2]; two more projection rows time the hole fill where nine of ten, and all, sources leave the image.  g_in of
the warping backward is timed on its own line: it is the fp32-atomic scatter, never asked for on the meta-learning path.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from meta_interpolation_amd import _hip, hip_ops

PEAK = 8.0e12
SIZES = ((256, 448), (768, 1280))
CHANNELS = (3, 196)
REPS, WARM = 40, 5


def timed(f):
    for _ in range(WARM):
        assert f() == 0
    torch.cuda.synchronize()
    evs = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    t = sorted(1e3 * a.elapsed_time(b) for a, b in evs)
    return t[len(t) // 2], t[0]


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dain_ops_bench needs the GPU: nothing is measured without one")
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    lib, st = _hip.lib(), _hip.current_stream()
    P = lambda t: None if t is None else t.data_ptr()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def report(op, shape, nbytes, med, mn):
        rec = dict(op=op, shape="x".join(str(v) for v in shape), median_us=round(med, 1), min_us=round(mn, 1), algorithmic_MB=round(nbytes / 1e6, 2),
                   hbm_peak_fraction=round(nbytes / (med * 1e-6) / PEAK, 4))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for H, W in SIZES:
        B = 1
        flow = (torch.rand(B, 2, H, W, device="cuda", generator=g) * 16 - 8).contiguous()
        wgt = torch.exp(torch.rand(B, 1, H, W, device="cuda", generator=g) * 11.5129 - 6.9078).contiguous()
        count, out = torch.empty(B, 1, H, W, device="cuda"), torch.empty(B, 2, H, W, device="cuda")
        gout2 = torch.randn(B, 2, H, W, device="cuda", generator=g)
        g_flow, g_w = torch.empty_like(flow), torch.empty_like(wgt)
        scratch = torch.empty(int(lib.savfi_depthflowproj_scratch_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
        for fill in (1, 0):
            med, mn = timed(lambda: lib.savfi_depthflowproj_fwd_f32(P(flow), P(wgt), P(count), P(out), P(scratch), B, H, W, fill, st))
            report("depthflowproj_fwd fillhole=%d" % fill, (B, H, W), hip_ops.depthflowproj_bytes(B, H, W), med, mn)
        med, mn = timed(lambda: lib.savfi_depthflowproj_bwd_f32(P(flow), P(wgt), P(count), P(out), P(gout2), P(g_flow), P(g_w), B, H, W, st))
        report("depthflowproj_bwd", (B, H, W), hip_ops.depthflowproj_bytes(B, H, W, grads=1), med, mn)
        holes = int((count <= 0).sum())
        lines.append("# %dx%d: %d of %d pixels are holes after the scatter" % (H, W, holes, B * H * W))
        print(lines[-1], flush=True)
        # the hole fill's worst cases: it walks O(W + H) per hole, so a frame most (or all) of whose sources leave the image costs
        # up to H W (W + H) dependent reads -- a case the +-8 pixel flows above never reach
        for name, keep in (("9 of 10 sources leave", 0.1), ("every source leaves", 0.0)):
            away = torch.rand(B, 1, H, W, device="cuda", generator=g) >= keep
            flow_h = torch.where(away, torch.full_like(flow, float(W + H)), flow).contiguous()
            med, mn = timed(lambda: lib.savfi_depthflowproj_fwd_f32(P(flow_h), P(wgt), P(count), P(out), P(scratch), B, H, W, 1, st))
            report("depthflowproj_fwd fillhole=1, %s" % name, (B, H, W), hip_ops.depthflowproj_bytes(B, H, W), med, mn)
            lines.append("# %dx%d, %s: %d of %d pixels are holes after the scatter" % (H, W, name, int((count <= 0).sum()), B * H * W))
            print(lines[-1], flush=True)
        for C in CHANNELS:
            inp = torch.randn(B, C, H, W, device="cuda", generator=g)
            filt = torch.randn(B, 16, H, W, device="cuda", generator=g) * 0.25
            gout = torch.randn(B, C, H, W, device="cuda", generator=g)
            o, gi, gf, gk = torch.empty_like(inp), torch.empty_like(inp), torch.empty_like(flow), torch.empty_like(filt)
            med, mn = timed(lambda: lib.savfi_filterinterp_fwd_f32(P(inp), P(flow), P(filt), P(o), B, C, H, W, 4, st))
            report("filterinterp_fwd", (B, C, H, W), hip_ops.filterinterp_bytes(B, C, H, W), med, mn)
            med, mn = timed(lambda: lib.savfi_filterinterp_bwd_f32(P(inp), P(flow), P(filt), P(gout), None, P(gf), P(gk), B, C, H, W, 4, st))
            report("filterinterp_bwd g_flow+g_filt", (B, C, H, W), 4 * B * H * W * (2 * C + 18 + 18), med, mn)
            med, mn = timed(lambda: lib.savfi_filterinterp_bwd_f32(P(inp), P(flow), P(filt), P(gout), P(gi), P(gf), P(gk), B, C, H, W, 4, st))
            report("filterinterp_bwd all (g_in by fp32 atomics)", (B, C, H, W), hip_ops.filterinterp_bytes(B, C, H, W, grads=1), med, mn)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("# tools/dain_ops_bench.py on an MI355X: isolated launches, HIP events, %d repetitions after %d warm-up calls; fraction of the\n"
                     "# 8 TB/s HBM peak = algorithmic bytes / median time / 8e12.  Measured on these shapes only; no speed gate.\n" % (REPS, WARM))
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
