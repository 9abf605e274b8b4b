"""The F(4x4) Winograd kernel's output stage (csrc/winograd4.h: the lane-to-lane exchange) against the bits of its parent commit.

tests/golden/wino4_stage_parent_bits.npz was written by tools/gen_wino4_stage_bits.py on the parent of the lane exchange; the stage kept
every expression per output element, so every case must come back bit for bit (torch.equal).  Each case is also held to a float64
convolution at the bound tests/test_hip_ops_gpu.py uses for F(4x4) layers (2e-5 of the output's scale, 1e-6 rms), so that a stale
fixture cannot hide an error.  The pooled map is an average of four such values: it is held to 2e-5 of the UNPOOLED map's scale (its
own rounding, three additions, is 2e-7).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_wino4_stage_bits", os.path.join(REPO, "tools", "gen_wino4_stage_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def bits():
    return np.load(os.path.join(REPO, "tests", "golden", "wino4_stage_parent_bits.npz"), allow_pickle=False)


def _reference(name):
    """float64 results of a case, planar: {"y": ..., "pooled": ...}."""
    kind, T, N, Ci, Co, H, W, arg = gen.CASES[name]
    t = {k: v.double() for k, v in gen.inputs(name).items()}
    x, w, b = t["x"], t["w"], t["b"]
    if kind in ("fwd", "pool", "unit16"):
        y = torch.cat([F.conv2d(x[n:n + 1], w[n % T], b[n % T], padding=gen.PAD) for n in range(N)])
        if arg != 1.0:
            y = F.leaky_relu(y, arg)
        ref = {"y": y}
        if kind == "pool":
            ref["pooled"] = F.avg_pool2d(y, 2)
        return ref
    y = torch.cat([F.conv_transpose2d(x[n:n + 1], w[n % T], padding=gen.PAD) for n in range(N)])
    if kind == "mask":
        y = y * torch.where(t["mask"] > 0, 1.0, float(arg))
    return {"y": y}


def _planar(name, key, got):
    """A unit-major result ([N][Ho][Wo/16][C][16] in memory) as the planar tensor it stands for."""
    kind, T, N, Ci, Co, H, W, arg = gen.CASES[name]
    if kind == "unit16" and key == "y":
        return got.reshape(N, H, W // 16, Co, 16).permute(0, 3, 1, 2, 4).reshape(N, Co, H, W)
    return got


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_output_stage_keeps_the_parent_bits(name, bits):
    kind, T, N, Ci, Co, H, W, arg = gen.CASES[name]
    assert int(bits[name + "/seed"]) == gen.seed_of(name)
    if name.startswith("split"):
        assert gen.is_split(name)
    got = gen.run(name)
    ref = _reference(name)
    assert sorted(got) == sorted(ref)
    scale = ref["y"].abs().max()
    for key in sorted(got):
        g = got[key].cpu()
        want = torch.from_numpy(bits["%s/%s" % (name, key)])
        d = _planar(name, key, g).double() - ref[key]
        print("%s/%s: max %.3g rms %.3g of the scale, equal %s" % (name, key, d.abs().max() / scale, d.pow(2).mean().sqrt() / scale,
                                                                  torch.equal(g, want)))
        assert g.shape == want.shape and torch.equal(g, want), (name, key, (g - want).abs().max().item())
        assert d.abs().max() <= 2e-5 * scale and d.pow(2).mean().sqrt() <= 1e-6 * scale, (name, key)


def test_mask_cases_have_both_signs_in_every_tile():
    for name, case in gen.CASES.items():
        if case[0] != "mask":
            continue
        m = gen.inputs(name)["mask"]
        H, W = m.shape[2:]
        for y0 in range(0, H - 1, 4):
            for x0 in range(0, W - 1, 4):
                tile = m[:, :, y0:y0 + 4, x0:x0 + 4]
                assert bool((tile > 0).flatten(2).any(2).all()) and bool((tile < 0).flatten(2).any(2).all()), (name, y0, x0)


def test_sepconv_pass_keeps_the_parent_bits(bits):
    """One SepConv forward and backward at 64x64.  The interpolated frame and the last layer's gradient come back bit for bit.  The first
    layer's two gradients have passed the data gradients of the deep layers, which at this size are MIOpen's (conv_route: 'aten' from
    128 -> 256 @16x16 down): their bits follow the solver MIOpen's search picks on the machine at hand -- the parent library itself gave
    19 of 32 / 1332 of 1728 other values on a second machine (3e-8 absolute, one unit in the last place), the same ones as the new
    stage there.  Those two are held to the fixture at 1e-5 of their scale, the bound of the suite's gradient fingerprints."""
    got = gen.sepconv_pass()
    keys = sorted(k[len("sepconv64/"):] for k in bits.files if k.startswith("sepconv64/") and not k.endswith("/seed"))
    assert int(bits["sepconv64/seed"]) == gen.SEPCONV_SEED
    assert keys == sorted(got) and len(keys) == 4
    first_layer = sorted(keys)[:2]
    assert all(k.startswith("grad:moduleConv1.") for k in first_layer), first_layer
    for key in keys:
        want = torch.from_numpy(bits["sepconv64/" + key])
        g = got[key].cpu()
        err = (g - want).abs().max().item()
        print("sepconv64/%s: max difference %.3g of scale %.3g, equal %s" % (key, err, want.abs().max().item(), torch.equal(g, want)))
        assert g.shape == want.shape
        if key in first_layer:
            assert err <= 1e-5 * want.abs().max().item(), (key, err)
        else:
            assert torch.equal(g, want), (key, err)
