"""Per-layer A/B of the deep 3x3 weight gradients: libraries given on the command line, alternating, HIP events."""
import ctypes
import sys

import torch

_P = ctypes.c_void_p
SHAPES = [  # (N, T, Ci, Co, H, W)
    (8, 4, 512, 512, 24, 32), (8, 4, 512, 512, 12, 16), (8, 4, 256, 256, 24, 32), (8, 4, 512, 256, 24, 32), (8, 4, 256, 512, 24, 32),
    (8, 4, 256, 256, 12, 16), (8, 4, 512, 256, 12, 16), (4, 4, 512, 256, 12, 16), (4, 1, 256, 256, 12, 16), (4, 1, 512, 256, 12, 16),
    (4, 1, 512, 512, 24, 32), (4, 1, 256, 256, 24, 32), (4, 1, 512, 256, 24, 32), (4, 1, 512, 512, 12, 16),
    (4, 4, 512, 512, 24, 32), (4, 4, 512, 512, 12, 16), (4, 4, 256, 256, 24, 32), (4, 4, 512, 256, 24, 32), (4, 4, 256, 256, 12, 16),
]
ROUNDS, REPS = 3, 40


def load(path):
    lib = ctypes.CDLL(path)
    lib.savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats.restype = ctypes.c_int64
    lib.savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats.argtypes = [ctypes.c_int] * 7
    lib.savfi_conv3x3_wgrad_wino_tasks_bias_f32.argtypes = [_P] * 5 + [ctypes.c_int] * 7 + [_P]
    return lib


def main():
    names = [a.split("=")[0] for a in sys.argv[1:]]
    libs = [load(a.split("=")[1]) for a in sys.argv[1:]]
    dev = "cuda"
    print("libraries:", ", ".join(sys.argv[1:]))
    print("%d rounds, alternating; each figure = mean of %d back-to-back calls between two HIP events, us per call (all launches of the call)" % (ROUNDS, REPS))
    for shp in SHAPES:
        N, T, Ci, Co, H, W = shp
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((N, Ci, H, W), device=dev, generator=g)
        gz = torch.randn((N, Co, H, W), device=dev, generator=g)
        st = torch.cuda.current_stream().cuda_stream
        outs, runs = [], []
        for lib in libs:
            fl = lib.savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats(N, T, Ci, Co, H, W, 1)
            assert fl > 0, fl
            ws = torch.empty(int(fl), device=dev)
            gw = torch.empty((T, Co, Ci, 3, 3), device=dev)
            gb = torch.empty((T, Co), device=dev)

            def run(lib=lib, ws=ws, gw=gw, gb=gb):
                rc = lib.savfi_conv3x3_wgrad_wino_tasks_bias_f32(x.data_ptr(), gz.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                                                 N, T, Ci, Co, H, W, 1, st)
                assert rc == 0, rc
            runs.append(run)
            outs.append((gw, gb))
        for run in runs:
            for _ in range(5):
                run()
        torch.cuda.synchronize()
        times = [[] for _ in libs]
        for _ in range(ROUNDS):
            for i, run in enumerate(runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(REPS):
                    run()
                b.record()
                torch.cuda.synchronize()
                times[i].append(1e3 * a.elapsed_time(b) / REPS)
        scale = outs[0][0].abs().max().item()
        line = "N=%d T=%d %3d->%3d @%dx%d:" % (N, T, Ci, Co, H, W)
        for i, nm in enumerate(names):
            line += "  %s %s" % (nm, "/".join("%.1f" % t for t in times[i]))
        for i in range(1, len(libs)):
            line += "  |gw_%s - gw_%s|max/max|gw| %.2e" % (names[i], names[0], (outs[i][0] - outs[0][0]).abs().max().item() / scale)
        tf = 18e-12 * Ci * Co * H * W * N
        line += "  direct-equivalent TF/s: " + ", ".join("%s %.0f" % (names[i], tf / (1e-6 * sorted(times[i])[len(times[i]) // 2])) for i in range(len(libs)))
        print(line, flush=True)


main()
