"""tools/gen_wino4_stage_bits.py -- the bits the F(4x4) Winograd kernel's output stage produces, on seeded inputs.

    python tools/gen_wino4_stage_bits.py [OUT.npz]        (default: tests/golden/wino4_stage_parent_bits.npz; needs the GPU)

Every case calls the convolution through the public hip_ops entry points on inputs drawn from numpy.random.default_rng(seed) and
stores what came back.  Run from a checkout of the commit whose bits are wanted -- the committed file comes from the parent of the lane
exchange (csrc/winograd4.h) -- and tests/test_wino4_lane_exchange_gpu.py, which imports CASES, inputs() and run() from here, holds a
later tree to those bits.  The file holds arrays and seeds only.

The cases sit where an output stage's lane -> (tile, channel) map, its shrunk channel descriptors and its mask fetch can go wrong:
produced channels I = 51 (the second block holds 19: lanes of several waves fall beyond I), 35, 32, 16; reduction channels K = 51, 12, 8;
maps 10x16 (row stores of 4, a partial tile row), 10x14 (stores of 2), 9x13 (stores of 1), 12x44 (33 tiles: the second group of 32 has
one live slot, and groups wrap rows); N = 1, 2 and T = 2 filter sets on N = 4; every activation form; masks of both slopes; the pooled
epilogue; unit-major output and input; one launch whose reduction is split; one SepConv forward and backward at 64x64.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "wino4_stage_parent_bits.npz")

# name: kind, T, N, Ci, Co, H, W (input map, pad 1: the output map has the same size), then per kind: slope (fwd / pool / unit16) or
# mask slope (mask; None: plain data gradient).  fwd / pool / unit16 produce I = Co channels from K = Ci; dgrad / mask / dgrad_unit16
# produce I = Ci from K = Co.
CASES = {
    "fwd_leaky_51_51_10x16": ("fwd", 1, 2, 51, 51, 10, 16, 0.1),
    "fwd_relu_12_35_10x14_T2": ("fwd", 2, 4, 12, 35, 10, 14, 0.0),
    "fwd_bias_8_35_9x13": ("fwd", 1, 2, 8, 35, 9, 13, 1.0),
    "fwd_leaky_51_16_12x44": ("fwd", 1, 2, 51, 16, 12, 44, 0.1),
    "dgrad_51_12_10x16": ("dgrad", 1, 2, 51, 12, 10, 16, None),
    "dgrad_35_8_9x13_T2": ("dgrad", 2, 4, 35, 8, 9, 13, None),
    "dgrad_16_51_12x44": ("dgrad", 1, 1, 16, 51, 12, 44, None),
    "dgrad_32_12_10x14": ("dgrad", 1, 2, 32, 12, 10, 14, None),
    "mask0_51_51_10x16": ("mask", 1, 2, 51, 51, 10, 16, 0.0),
    "mask01_35_12_10x14_T2": ("mask", 2, 4, 35, 12, 10, 14, 0.1),
    "mask01_51_8_9x13": ("mask", 1, 2, 51, 8, 9, 13, 0.1),
    "pool_12_51_12x16": ("pool", 1, 2, 12, 51, 12, 16, 0.0),
    "pool_8_35_10x14": ("pool", 1, 2, 8, 35, 10, 14, 0.1),
    "unit16_51_51_8x32": ("unit16", 1, 1, 51, 51, 8, 32, 0.1),
    "dgrad_unit16_51_51_8x32": ("dgrad_unit16", 1, 1, 51, 51, 8, 32, None),
    # the smallest reduction the F(4x4) plan splits (32 chunks of 8 channels: K > 248) on a launch far below the chip's workgroup slots
    "split_250_35_9x13": ("fwd", 1, 1, 250, 35, 9, 13, 0.1),
    "split_dgrad_35_250_9x13": ("dgrad", 1, 1, 35, 250, 9, 13, None),
}
PAD = 1
SEPCONV_SEED = 777


def sepconv_grad_names(net):
    """The parameters whose gradients the SepConv case keeps: the first layer's two (the end of the whole backward chain) and the last one."""
    names = [n for n, _ in net.named_parameters()]
    return [names[0], names[1], names[-1]]


def seed_of(name):
    return 1000 + sorted(CASES).index(name)


def inputs(name):
    """Seeded CPU tensors of a case: x (the kernel's input map), w [T,Co,Ci,3,3], b [T,Co], mask (mask cases; both signs in every tile)."""
    kind, T, N, Ci, Co, H, W = CASES[name][:7]
    rng = np.random.default_rng(seed_of(name))
    fwd = kind in ("fwd", "pool", "unit16")
    cin = Ci if fwd else Co
    t = {"x": torch.from_numpy(rng.standard_normal((N, cin, H, W), dtype=np.float32)),
         "w": torch.from_numpy(rng.standard_normal((T, Co, Ci, 3, 3), dtype=np.float32) / np.float32(3 * cin ** 0.5)),
         "b": torch.from_numpy(rng.standard_normal((T, Co), dtype=np.float32))}
    if kind == "mask":
        m = np.abs(rng.standard_normal((N, Ci, H, W), dtype=np.float32)) + np.float32(0.01)
        sign = np.where(rng.random((N, Ci, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
        sign[..., 0::4, 0::4] = 1.0
        sign[..., 1::4, 1::4] = -1.0
        sign[..., 0::4, 1::4] = -1.0
        t["mask"] = torch.from_numpy(m * sign)
    return t


def is_split(name):
    """Does the F(4x4) plan split this launch's reduction over workgroups?  savfi_conv3x3_f4_workgroups counts the splits in."""
    from meta_interpolation_amd import hip_ops
    kind, T, N, Ci, Co, H, W = CASES[name][:7]
    mode = 0 if kind in ("fwd", "pool", "unit16") else 1
    assert -(-H // 4) * -(-W // 4) <= 32                  # (one group of 32 tiles per sample, however the tiles are counted)
    blocks = 1
    unsplit = blocks * (-(-(Co if mode == 0 else Ci) // 32)) * N
    return hip_ops.wino4_workgroups(N, Ci, Co, H, W, PAD, mode) > unsplit


def run(name, dev="cuda"):
    """{key: CUDA tensor} of a case, through hip_ops on the F(4x4) filter transform (form 0)."""
    from meta_interpolation_amd import hip_ops
    kind, T, N, Ci, Co, H, W, arg = CASES[name]
    t = {k: v.to(dev) for k, v in inputs(name).items()}
    u_f, u_b = hip_ops.conv3x3_filters(t["w"], True, True)
    if kind == "fwd":
        return {"y": hip_ops.conv3x3_tasks_pre(t["x"], u_f, T, Ci, Co, t["b"], 0, arg, PAD)}
    if kind == "pool":
        y, p = hip_ops.conv3x3_tasks_pre_pool(t["x"], u_f, T, Ci, Co, t["b"], arg, PAD)
        return {"y": y, "pooled": p}
    if kind == "unit16":        # the tensor's MEMORY is [N][Ho][Wo/16][Co][16]: stored as it lies
        return {"y": hip_ops.conv3x3_tasks_pre(t["x"], u_f, T, Ci, Co, t["b"], 0, arg, PAD, out_unit16=True)}
    if kind == "dgrad":
        return {"y": hip_ops.conv3x3_tasks_pre(t["x"], u_b, T, Ci, Co, None, 1, 1.0, PAD)}
    if kind == "mask":
        return {"y": hip_ops.conv3x3_tasks_pre(t["x"], u_b, T, Ci, Co, None, 1, 1.0, PAD, mask=t["mask"], mask_slope=arg)}
    if kind == "dgrad_unit16":  # the cotangent's memory is unit-major
        gy = t["x"]
        gyu = gy.reshape(N, Co, H, W // 16, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(N, Co, H, W)
        return {"y": hip_ops.conv3x3_dgrad_in_unit16(gyu, u_b, T, Ci, Co, PAD)}
    raise ValueError(kind)


def sepconv_pass(dev="cuda"):
    """One SepConv forward and backward at 64x64 on seeded weights and frames: the interpolated frame and a few parameter gradients."""
    from tests.helpers import build_plugin
    net = build_plugin("sepconv", dev)
    rng = np.random.default_rng(SEPCONV_SEED)
    f0 = torch.from_numpy(rng.random((1, 3, 64, 64), dtype=np.float32)).to(dev)
    f1 = torch.from_numpy(rng.random((1, 3, 64, 64), dtype=np.float32)).to(dev)
    tgt = torch.from_numpy(rng.random((1, 3, 64, 64), dtype=np.float32)).to(dev)
    # (layers the library leaves to MIOpen: its default fp32 solvers are not reproducible run to run, tests/conftest.py)
    pinned, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        out = net(f0, f1)
        loss = (out - tgt).abs().mean()
        params = dict(net.named_parameters())
        names = sepconv_grad_names(net)
        grads = torch.autograd.grad(loss, [params[n] for n in names])
    finally:
        torch.backends.cudnn.deterministic = pinned
    res = {"out": out.detach()}
    for n, g in zip(names, grads):
        res["grad:" + n] = g
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    arrays = {}
    for name in CASES:
        if name.startswith("split"):
            assert is_split(name), name
        for key, val in run(name).items():
            arrays["%s/%s" % (name, key)] = val.cpu().numpy()
        arrays[name + "/seed"] = np.int64(seed_of(name))
    first, second = sepconv_pass(), sepconv_pass()
    for key, val in first.items():
        assert torch.equal(val, second[key]), "not reproducible run to run: %s" % key
        arrays["sepconv64/" + key] = val.cpu().numpy()
    arrays["sepconv64/seed"] = np.int64(SEPCONV_SEED)
    np.savez_compressed(out_path, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (out_path, len(arrays), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
