"""-m gpu: every launch variant of the Winograd 3x3 kernels against float64, on small shapes.

F(4x4) (csrc/winograd4.h): forward (bias; ReLU, leaky ReLU, identity) and data gradient, pad 0 / 1, row stores of 1 / 2 / 4 floats,
tile blocks 2^(5-s) x 2^s for every s, the reduction unsplit / split / split with a ragged last part, the masked epilogue (in the kernel
and behind wino_split_reduce), unit-major output and input, 1 and 3 tasks; F(2x2) (csrc/winograd.hip): even and odd widths, the masked
data gradient, the unit-major input and the split beyond 512 channels.  The plan of every case comes from the transcription in
tests/conv_ref.py (held to the library by tests/test_conv_plan_cpu.py), and test_variant_matrix_covers_every_f4_launch -- a CPU test --
holds this list to every launch that plan can produce.

Masks hold exact 0.0 and -0.0: torch's relu / leaky_relu backward take the slope side there.  Inputs are zero-mean normal and
non-negative with a DC offset (1 + 0.05 randn, relu(randn)), where F(4x4)'s transforms cancel most; the global scale gates apply to the
zero-mean inputs only, the local gate (tests/conv_ref.py) to all.

c_family = 4 x the largest |got - ref| / (2^-24 L) measured on an MI355X over every case of this file and of
tests/test_conv_layers_gpu.py and seeds 0, 1, 2:  F(4x4) 63.3, F(2x2) 1.78 (MEASURED_F4 / MEASURED_F2).
This file is the first to launch every wino4_conv3x3 instantiation in one process: each now sets its own 72 KB dynamic-LDS attribute
(csrc/winograd.hip, launch_wino4; one flag shared by all of them configured only the first one launched)."""
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import hip_ops
from tests import conv_ref as R

DEV = "cuda"

MEASURED_F4 = 63.3
MEASURED_F2 = 1.78
C_F4 = 4 * MEASURED_F4
C_F2 = 4 * MEASURED_F2

# name: (form, mode, T, N, Ci, Co, H, W, pad, slope (forward) or mask slope (data gradient; None = unmasked), layout)
#   form 4: F(4x4) (channels <= 512); 2: F(2x2) through the form bit (f2=True) or by channel counts (> 512)
#   layout: None, 'out16' (forward writes unit-major), 'in16' (data gradient reads a unit-major cotangent)
CASES = {
    "f4_fwd_ts0_v4_identity":      (4, 0, 1, 2, 8, 16, 128, 4, 1, 1.0, None),
    "f4_dgrad_ts1_v1_mask0":       (4, 1, 1, 2, 16, 24, 64, 7, 1, 0.0, None),
    "f4_fwd_ts2_v2_leaky":         (4, 0, 1, 2, 12, 40, 34, 16, 0, 0.2, None),
    "f4_dgrad_ts3_v2_mask01_T3":   (4, 1, 3, 6, 20, 33, 14, 28, 0, 0.1, None),
    "f4_fwd_ts4_v1_relu_T3":       (4, 0, 3, 6, 9, 31, 8, 61, 1, 0.0, None),
    "f4_dgrad_ts5_v1_mask0":       (4, 1, 1, 2, 24, 16, 3, 125, 1, 0.0, None),
    "f4_dgrad_ts3_v4_mask0":       (4, 1, 1, 2, 32, 51, 20, 24, 1, 0.0, None),
    "f4_dgrad_ts4_v4":             (4, 1, 3, 6, 51, 51, 8, 64, 1, None, None),
    "f4_fwd_split_v4_relu":        (4, 0, 1, 2, 256, 32, 8, 8, 1, 0.0, None),
    "f4_fwd_ragged_v4_leaky":      (4, 0, 1, 2, 264, 64, 12, 16, 1, 0.2, None),
    "f4_fwd_ragged_v1_T3":         (4, 0, 3, 6, 300, 40, 7, 9, 1, 1.0, None),
    "f4_dgrad_ragged_v1_mask0_T3": (4, 1, 3, 6, 40, 264, 10, 13, 0, 0.0, None),
    "f4_dgrad_split_v2_mask01":    (4, 1, 1, 2, 32, 256, 8, 10, 1, 0.1, None),
    "f4_dgrad_split_v2":           (4, 1, 1, 2, 32, 256, 8, 10, 1, None, None),
    "f4_fwd_out16_T3":             (4, 0, 3, 6, 24, 40, 12, 32, 1, 0.2, "out16"),
    "f4_dgrad_in16_pad1":          (4, 1, 1, 2, 24, 40, 12, 32, 1, None, "in16"),
    "f4_dgrad_in16_pad0_T3":       (4, 1, 3, 6, 24, 40, 10, 16, 0, None, "in16"),
    "f2_fwd_even_leaky":           (2, 0, 1, 2, 51, 51, 18, 30, 1, 0.2, None),
    "f2_fwd_odd_relu_T3":          (2, 0, 3, 6, 40, 24, 9, 13, 0, 0.0, None),
    "f2_dgrad_odd_mask0":          (2, 1, 1, 2, 24, 40, 11, 15, 1, 0.0, None),
    "f2_fwd_split_beyond_512":     (2, 0, 1, 2, 576, 528, 12, 20, 1, 0.0, None),
    "f2_dgrad_split_beyond_512":   (2, 1, 1, 2, 528, 576, 12, 20, 1, 0.1, None),
    "f2_dgrad_in16_beyond_512":    (2, 1, 1, 16, 32, 520, 62, 64, 0, None, "in16"),
}
KINDS = ["normal", "dc", "relu"]


def _draw(shape, kind, g):
    v = torch.randn(shape, generator=g)
    if kind == "dc":
        return 1.0 + 0.05 * v
    if kind == "relu":
        return torch.relu(v)
    return v


def _mask(shape, g):
    """a forward activation: normal values with ~1/4 exact 0.0 and ~1/8 exact -0.0"""
    m = torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g)
    m = torch.where(u < 0.25, torch.zeros_like(m), m)
    return torch.where((u >= 0.25) & (u < 0.375), torch.full_like(m, -0.0), m)


def f4_launch(case):
    """(plan, instance, masked, in16, out16) of an F(4x4) case"""
    form, mode, T, N, Ci, Co, H, W, pad, s, layout = case
    plan = R.f4_plan(N, Ci, Co, H, W, pad, mode) if form == 4 else None
    masked = mode == 1 and s is not None
    return plan, (R.f4_instance(plan, masked, layout == "in16") if plan else None), masked, layout == "in16", layout == "out16"


def _subset(n, cap):
    return None if n <= cap else sorted({0, 7, 8, 31, 32, n - 1})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_conv3x3_variant_matches_float64(name, kind):
    from tests.test_hip_ops_gpu import conv3x3_close
    case = CASES[name]
    form, mode, T, N, Ci, Co, H, W, pad, s, layout = case
    plan, inst, masked, in16, out16 = f4_launch(case)
    assert (plan is not None) == (form == 4), name
    f2 = form == 2 and max(Ci, Co) <= 512
    g = torch.Generator().manual_seed(1000 * R.SEED_OFFSET + 17 + sorted(CASES).index(name) * 3 + KINDS.index(kind))
    w = torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * (Ci if mode == 0 else Co) ** 0.5)
    wc = w.to(DEV)
    if not f2:
        assert hip_ops.wino4_workgroups(N, Ci, Co, H, W, pad, mode) == (plan["workgroups"] if plan else 0)
    u_f, u_b = hip_ops.conv3x3_filters(wc, mode == 0, mode == 1, f2=f2)
    c_family, family = (C_F4, "f4") if form == 4 else (C_F2, "f2")
    if mode == 0:
        x = _draw((N, Ci, H, W), kind, g)
        b = torch.randn(T, Co, generator=g)
        got = hip_ops.conv3x3_tasks_pre(x.to(DEV), u_f, T, Ci, Co, b.to(DEV), 0, s, pad, out_unit16=out16, f2=f2)
        if out16:
            B, K, Ho, Wo = got.shape
            got = got.reshape(B, Ho, Wo // 16, K, 16).permute(0, 3, 1, 2, 4).reshape(B, K, Ho, Wo)
        chans = _subset(Co, 64)
        z, mag = R.conv_tasks64(x, w, pad, T, chans=chans, bias=b)
        ref = R.act(z, s)
        got = got.cpu()[:, chans] if chans else got.cpu()
    else:
        Ho, Wo = H + 2 * (2 - pad) - 2, W + 2 * (2 - pad) - 2          # the data gradient's map
        gy = _draw((N, Co, H, W), kind, g)
        gyc = gy.to(DEV)
        mask = _mask((N, Ci, Ho, Wo), g) if masked else None
        if in16:
            gyu = gyc.reshape(N, Co, H, W // 16, 16).permute(0, 2, 3, 1, 4).contiguous().reshape(N, Co, H, W)
            got = hip_ops.conv3x3_dgrad_in_unit16(gyu, u_b, T, Ci, Co, pad)
            assert torch.equal(got, hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad))
        else:
            got = hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad, f2=f2)
        if masked:
            gotm = hip_ops.conv3x3_tasks_pre(gyc, u_b, T, Ci, Co, None, 1, 1.0, pad, mask=mask.to(DEV), mask_slope=s, f2=f2)
            assert torch.equal(gotm, got * R.mask_factor(mask.to(DEV), s))       # the existing contract, bit for bit
            got = gotm
        samples = [0, N - 1] if in16 and form == 2 else None
        chans = _subset(Ci, 64) or ([0, 7, 8, 31] if samples else None)
        ref, mag = R.dgrad_tasks64(gy, w, pad, T, samples=samples, chans=chans)
        if masked:
            m = mask[samples] if samples else mask
            ref = ref * R.mask_factor((m[:, chans] if chans else m).double(), s)
        got = got.cpu()
        got = got[samples] if samples else got
        got = got[:, chans] if chans else got
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if kind == "normal":
        assert conv3x3_close(got.double(), ref, Ci, Co), (name, R.global_err(got, ref))
    R.assert_local(got, ref, R.pool7(mag), c_family, family, "%s %s" % (name, kind))


def test_variant_matrix_covers_every_f4_launch():
    """CPU: the list above reaches every F(4x4) launch the plan (tests/conv_ref.py) can produce -- each mode, padding, store width,
    tile-block shape, split kind, mask (also behind a split), unit-major layout, task count, and every kernel instantiation that a shape
    can reach."""
    seen = {k: set() for k in ("mode", "pad", "vecw", "ts", "split", "masked", "masked_split", "masked_vecw", "layout", "T", "inst")}
    f2 = {"even": False, "odd": False, "in16": False, "split": False, "masked": False}
    for name, case in CASES.items():
        form, mode, T, N, Ci, Co, H, W, pad, s, layout = case
        assert N % T == 0 and (T == 1 or N == 2 * T), name
        plan, inst, masked, in16, out16 = f4_launch(case)
        if plan is None:
            Wo = W + 2 * (pad if mode == 0 else 2 - pad) - 2
            f2["even" if Wo % 2 == 0 else "odd"] = True
            f2["in16"] |= in16
            f2["masked"] |= masked
            f2["split"] |= max(Ci, Co) > 512 and not in16
            continue
        assert not (in16 or out16) or plan["nsplit"] == 1, name
        seen["mode"].add(mode)
        seen["pad"].add(pad)
        seen["vecw"].add(plan["vecw"])
        seen["ts"].add(plan["tile_shift"])
        seen["split"].add("ragged" if plan["ragged"] else "split" if plan["nsplit"] > 1 else "unsplit")
        seen["masked"].add(masked)
        if masked:
            seen["masked_split"].add(plan["nsplit"] > 1)
            seen["masked_vecw"].add(plan["vecw"])
        seen["layout"].add((layout, 1 + plan["off"]) if in16 else layout)
        seen["T"].add(T)
        seen["inst"].add(inst)
        if mode == 0:
            seen.setdefault("fwd_slope", set()).add(s)
    # every instantiation a shape can reach (scan of the plan: the unit-major input fixes the store width by its padding)
    reachable = set()
    for mode in (0, 1):
        for pad in (0, 1):
            for W in range(1, 70):
                p = R.f4_plan(1, 16, 16, 16, W, pad, mode)
                if p is None:
                    continue
                reachable.add(R.f4_instance(p))
                if mode == 1:
                    reachable.add(R.f4_instance(p, masked=True))
                    if W % 16 == 0 and p["Wo"] % 2 == 0:
                        reachable.add(R.f4_instance(p, in16=True))
    assert seen["mode"] == {0, 1} and seen["pad"] == {0, 1} and seen["vecw"] == {1, 2, 4}, seen
    assert seen["ts"] == set(range(6)), seen["ts"]
    assert seen["split"] == {"unsplit", "split", "ragged"}, seen["split"]
    assert seen["masked"] == {False, True} and seen["masked_split"] == {False, True} and seen["masked_vecw"] == {1, 2, 4}, seen
    assert seen["layout"] >= {None, "out16", ("in16", 2), ("in16", 3)}, seen["layout"]
    assert seen["T"] == {1, 3} and seen["fwd_slope"] >= {0.0, 0.2, 1.0}, seen
    assert seen["inst"] == reachable, (sorted(reachable - seen["inst"]), sorted(seen["inst"]))
    assert all(f2.values()), f2
