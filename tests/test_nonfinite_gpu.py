"""-m gpu: no kernel of the core that every model runs through may turn a NaN or an infinity into a number.

Every case plants NaN, +inf and -inf into sample 0 / task 0 of one input (tests/nonfinite_ref.py: plant) and holds the kernel's result
to the contract of that module (hold): (A) what float64 torch makes non-finite is non-finite, (B) what came out finite is right inside the
op's own float64 gate, computed from the clean inputs, (C) the other samples / tasks keep their clean bits and inside the planted sample a
stated footprint bounds what may be non-finite beyond the reference.  Shapes and entry points are those of the float64 suites; their
gates are imported from them.

The footprints, by kernel family ("Non-finite values"):
  * Winograd F(4x4) / F(2x2) forward and data gradient: the output tiles whose input tile holds the planted pixel, every produced channel;
  * direct kernels on split-bf16 products (convk, the weight gradients, the 51-tap op): none beyond the elements the reference makes
    non-finite -- an infinity may come out as NaN there (inf splits into inf + (inf - inf));
  * weight gradients: the planted channel's slice of the task's gradient (products with zero padding count);
  * `x > 0 ? x : slope * x` with slope 0 at -inf (0 * -inf): NaN where torch's relu gives 0 -- a footprint entry at that element;
  * bilinear x2: the products of weight exactly 0 (the forward's second tap, the adjoint's window of six candidate outputs per axis);
  * point-wise ops, permutations, pooling, losses, multi-tensor ops: none.
The activation derivative read from a stored activation takes the slope side where that activation is NaN, as torch's leaky_relu
backward does (its relu backward passes the cotangent): _act_bwd64 states it, and the masked cases hold the kernels to that."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops, synthetic
from tests import conv_ref as R
from tests import nonfinite_ref as NF
from tests import small_ops_ref as SR
from tests import test_conv_variants_gpu as V
from tests.nonfinite_ref import NAN, NINF, PINF

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP = 2.0 ** -24
VALUES = [NAN, PINF, NINF]


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _act_bwd64(g, y, slope):
    """torch's activation derivative from the stored activation y: relu's selects 0 behind an inactive unit (it never multiplies an
    infinite cotangent by 0), leaky_relu's multiplies by the slope.  Where y itself is NaN this takes the inactive side, as
    leaky_relu's backward and the kernels do (relu's backward would pass g: DESIGN.md, "Non-finite values")."""
    g = g.double()
    if slope is None or slope == 1.0:
        return g
    return torch.where(y.double() > 0, g, torch.zeros_like(g) if slope == 0.0 else slope * g)


def _tasks_first(t, T):
    """[N, ...] with sample n on task n % T -> [T, N / T, ...]: dimension 0 is the task, as hold() wants it for a planted weight"""
    return t.reshape((t.shape[0] // T, T) + tuple(t.shape[1:])).transpose(0, 1).contiguous()


# =====================================================================================================================================
# Winograd forward and masked data gradient
# =====================================================================================================================================
def _wino_candidates(C, H, W, Ho, Wo, m, off):
    """(what, (c, y, x)) of the planted input pixels, clipped to the map: a tile interior (a pixel only one tile reads), a pixel on a
    corner shared by four tiles, the outermost row, the last (ragged) tile, and the last channel (the padded channel remainder where the
    channel count is no multiple of the kernel's chunk)."""
    ty, tx = min(1, -(-Ho // m) - 1), min(1, -(-Wo // m) - 1)
    clip = lambda y, x: (min(max(y, 0), H - 1), min(max(x, 0), W - 1))
    return [("interior", (0,) + clip(m * ty - off + 2, m * tx - off + 2)),
            ("corner", (1 % C,) + clip(m * ty - off + m, m * tx - off + m)),
            ("border", (C // 2,) + clip(0, W // 2)),
            ("ragged", (max(C - 2, 0),) + clip(H - 1, W - 1)),
            ("channel", (C - 1,) + clip(H - 1, 0))]


def _wino_runs(cands, shape, m, off):
    """The candidates packed into as few runs as the share cap allows: [(names, where, values, footprint)].  A candidate whose own
    footprint is over the cap on this map (a corner of four tiles on a map of four) is left out; the interior one must fit.  The callers
    hold the names that ran to WINO_POSITIONS, so that an edit of a table cannot empty a class of positions without notice."""
    runs, k = [], 0
    for what, pos in cands:
        alone = NF.wino_footprint(shape, [pos[1:]], m, off)
        if float(alone.sum()) / alone.numel() > NF.MAX_SHARE:
            assert what != "interior", (what, pos, shape)
            continue
        value = VALUES[k % 3]
        k += 1
        for run in runs:
            both = run[3] | alone
            if float(both.sum()) / both.numel() <= NF.MAX_SHARE and pos not in run[1]:
                run[0].append(what), run[1].append(pos), run[2].append(value)
                run[3] = both
                break
        else:
            runs.append([[what], [pos], [value], alone])
    return runs


def _tiles(pos, shape, m, off):
    """how many output tiles read the input pixel pos = (c, y, x)"""
    fp = NF.wino_footprint((1,) + tuple(shape[1:]), [pos[1:]], m, off)[0]
    return int(fp[::m, ::m].sum())


def _ran(runs, shape, m, off):
    """{name: tiles that read it} of the positions the runs hold"""
    return {n: _tiles(pos, shape, m, off) for run in runs for n, pos in zip(run[0], run[1])}


def _t(interior, corner, border, ragged, channel):
    return dict(interior=interior, corner=corner, border=border, ragged=ragged, channel=channel)


# What each case exercises: the positions that ran (all five everywhere; one that did not fit under the share cap would be missing) and the
# number of tiles that read each.  F(2x2)'s 4 x 4 input tiles overlap by two, so every pixel off the border lies in four of them; a map of
# one or two tile rows or columns (8 x 61, 128 x 4, 64 x 7, 8 x 8) has no corner of four, the clipped position lies in two tiles or one.
WINO_POSITIONS = {
    "f4_fwd_ts4_v1_relu_T3": _t(1, 2, 1, 2, 1), "f4_fwd_ts2_v2_leaky": _t(1, 4, 2, 1, 1), "f4_fwd_ts0_v4_identity": _t(1, 2, 1, 1, 1),
    "f4_fwd_split_v4_relu": _t(1, 1, 2, 1, 1), "f4_fwd_ragged_v4_leaky": _t(1, 4, 2, 1, 1), "f4_fwd_out16_T3": _t(1, 4, 2, 1, 1),
    "f2_fwd_odd_relu_T3": _t(4, 4, 2, 1, 1), "f2_fwd_even_leaky": _t(4, 4, 2, 1, 1), "f2_fwd_split_beyond_512": _t(4, 4, 2, 1, 1),
    "f4_dgrad_ts1_v1_mask0": _t(1, 2, 2, 1, 1), "f4_dgrad_split_v2_mask01": _t(1, 2, 1, 1, 1), "f2_dgrad_odd_mask0": _t(4, 4, 2, 4, 2),
}


WINO_FWD = ["f4_fwd_ts4_v1_relu_T3", "f4_fwd_ts2_v2_leaky", "f4_fwd_ts0_v4_identity", "f4_fwd_split_v4_relu", "f4_fwd_ragged_v4_leaky",
            "f4_fwd_out16_T3", "f2_fwd_odd_relu_T3", "f2_fwd_even_leaky", "f2_fwd_split_beyond_512"]


@pytest.mark.parametrize("name", WINO_FWD)
def test_winograd_forward_keeps_non_finite_values(name):
    form, mode, T, N, Ci, Co, H, W, pad, s, layout = V.CASES[name]
    assert mode == 0
    f2 = form == 2 and max(Ci, Co) <= 512
    m = 4 if form == 4 else 2
    g = torch.Generator().manual_seed(4100 + sorted(V.CASES).index(name))
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    b = torch.randn(T, Co, generator=g)
    u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False, f2=f2)

    def run(inp):
        got = hip_ops.conv3x3_tasks_pre(inp.to(DEV), u_f, T, Ci, Co, b.to(DEV), 0, s, pad, out_unit16=layout == "out16", f2=f2)
        if layout == "out16":
            B, K, Ho, Wo = got.shape
            got = got.reshape(B, Ho, Wo // 16, K, 16).permute(0, 3, 1, 2, 4).reshape(B, K, Ho, Wo)
        return got.cpu()

    clean = run(x)
    z, mag = R.conv_tasks64(x, w, pad, T, bias=b)
    tol = R.local_bound(R.pool7(mag), V.C_F4 if form == 4 else V.C_F2)
    Ho, Wo = clean.shape[2:]
    runs = _wino_runs(_wino_candidates(Ci, H, W, Ho, Wo, m, pad), (Co, Ho, Wo), m, pad)
    assert _ran(runs, (Co, Ho, Wo), m, pad) == WINO_POSITIONS[name], (name, _ran(runs, (Co, Ho, Wo), m, pad))
    for names, where, values, fp in runs:
        xp = NF.plant(x, where, values)
        ref = R.act(z, s).clone()
        ref[0:1] = R.act(R.conv_tasks64(xp, w, pad, T, samples=[0], bias=b)[0], s)
        n = NF.hold(run(xp), ref, clean, footprint=fp, tol=tol, what="%s %s" % (name, names))
        print("%s: planted %s at %s -> %d non-finite outputs, footprint %d" % (name, values, where, n, int(fp.sum())))


def test_winograd_pooled_output_stage_keeps_non_finite_values():
    """savfi_conv3x3_tasks_pre_pool_f32 at the 13 x 18 map of tests/test_wino4_flat_pool_gpu.py: the full-size output and the pooled one
    (a pooled pixel is non-finite where one of its four is)."""
    from tests import test_wino4_flat_pool_gpu as P
    H, W = P.POOL_MAPS[1]
    N, T, Ci, Co, pad = P.N, P.T, 16, 40, 1
    for slope in (0.0, 0.2):
        g = torch.Generator().manual_seed(4200 + int(10 * slope))
        w = P._weights(Ci, Co, 0, g)
        x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T, Co, generator=g)
        u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False)
        run = lambda inp: [t.cpu() for t in hip_ops.conv3x3_tasks_pre_pool(inp.to(DEV), u_f, T, Ci, Co, b.to(DEV), slope, pad)]
        clean_y, clean_p = run(x)
        z, mag = R.conv_tasks64(x, w, pad, T, bias=b)
        tol = R.local_bound(R.pool7(mag), V.C_F4)
        where, values = [(0, 5, 6), (Ci - 1, H - 1, W - 1)], [NAN, NINF if slope else PINF]
        xp = NF.plant(x, where, values)
        fp = NF.wino_footprint((Co, H, W), [p[1:] for p in where], 4, pad)
        ref = R.act(R.conv_tasks64(xp, w, pad, T, bias=b)[0], slope)
        y, p = run(xp)
        NF.hold(y, ref, clean_y, footprint=fp, tol=tol, what="pool stage: full output")
        fp_p = F.max_pool2d(fp[None].float(), 2)[0] > 0
        NF.hold(p, F.avg_pool2d(ref, 2), clean_p, footprint=fp_p, tol=F.avg_pool2d(tol, 2), what="pool stage: pooled output")


WINO_DGRAD = ["f4_dgrad_ts1_v1_mask0", "f4_dgrad_split_v2_mask01", "f2_dgrad_odd_mask0"]


@pytest.mark.parametrize("planted", ["cotangent", "mask"])
@pytest.mark.parametrize("name", WINO_DGRAD)
def test_winograd_masked_data_gradient_keeps_non_finite_values(name, planted):
    form, mode, T, N, Ci, Co, H, W, pad, s, layout = V.CASES[name]
    assert mode == 1 and s is not None
    f2 = form == 2 and max(Ci, Co) <= 512
    m, off = (4 if form == 4 else 2), 2 - pad
    Ho, Wo = H + 2 * off - 2, W + 2 * off - 2
    g = torch.Generator().manual_seed(4300 + sorted(V.CASES).index(name))
    w = torch.randn(T, Co, Ci, 3, 3, generator=g) / (3 * Co ** 0.5)
    gy = torch.randn(N, Co, H, W, generator=g)
    mask = V._mask((N, Ci, Ho, Wo), g)
    _, u_b = hip_ops.conv3x3_filters(w.to(DEV), False, True, f2=f2)
    run = lambda c, mk: hip_ops.conv3x3_tasks_pre(c.to(DEV), u_b, T, Ci, Co, None, 1, 1.0, pad, mask=mk.to(DEV), mask_slope=s, f2=f2).cpu()
    clean = run(gy, mask)
    val, mag = R.dgrad_tasks64(gy, w, pad, T)
    tol = R.local_bound(R.pool7(mag), V.C_F4 if form == 4 else V.C_F2)
    if planted == "cotangent":
        runs = _wino_runs(_wino_candidates(Co, H, W, Ho, Wo, m, off), (Ci, Ho, Wo), m, off)
        assert _ran(runs, (Ci, Ho, Wo), m, off) == WINO_POSITIONS[name], (name, _ran(runs, (Ci, Ho, Wo), m, off))
        for names, where, values, fp in runs:
            gp = NF.plant(gy, where, values)
            ref = _act_bwd64(R.dgrad_tasks64(gp, w, pad, T)[0], mask, s)
            NF.hold(run(gp, mask), ref, clean, footprint=fp, tol=tol, what="%s %s" % (name, names))
    else:
        # the stored activation only selects the factor: NaN and -inf take the slope, +inf takes 1 (R.mask_factor); nothing is non-finite
        where = [(0, 1, 1), (Ci // 2, Ho - 1, Wo - 1), (Ci - 1, 0, Wo // 2)]
        mp = NF.plant(mask, where, VALUES)
        got = run(gy, mp)
        NF.hold(got, _act_bwd64(val, mp, s), clean, tol=tol, reaches=False, what="%s mask" % name)
        assert bool(torch.isfinite(got).all())


# =====================================================================================================================================
# direct kernels
# =====================================================================================================================================
def _convk_cases():
    from tests.test_hip_ops_gpu import CONVK_CASES
    picked = {}
    for case in CONVK_CASES:              # per K: the first case with several samples (a control) -- K, Ci, Co, H, W, pad, T, N
        if case[0] not in picked and case[7] >= 2:
            picked[case[0]] = case
    return [picked[K] for K in sorted(picked)]


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("case", _convk_cases(), ids=lambda c: "K%d-%dto%d" % c[:3])
def test_direct_convolution_keeps_non_finite_values(case, precise):
    """convk forward with leaky ReLU and with ReLU, and the data gradient, on split-bf16 products: an infinity may come out as NaN, and
    with slope 0 a -inf pre-activation comes out as NaN (0 * -inf) where torch's relu gives 0 -- both only where the reference's
    pre-activation is non-finite.  Gate: the 3e-6 of max|ref| of tests/test_hip_ops_gpu.py."""
    K, Ci, Co, H, W, pad, T, N = case
    g = torch.Generator().manual_seed(K * 1000 + Ci + Co + 1)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(T, Co, Ci, K, K, generator=g) / (K * math.sqrt(Ci))
    b = torch.randn(T, Co, generator=g)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    gy = torch.randn(N, Co, Ho, Wo, generator=g)
    pf, pb = hip_ops.convk_filters(w.to(DEV), True, True)
    conv64 = lambda t: torch.cat([F.conv2d(t[n:n + 1].double(), w[n % T].double(), b[n % T].double(), padding=pad) for n in range(N)], 0)
    dgrad64 = lambda t: torch.cat([F.conv_transpose2d(t[n:n + 1].double(), w[n % T].double(), padding=pad) for n in range(N)], 0)
    where = [(0, H // 2, W // 2), (Ci - 1, 0, W - 1), (Ci // 2, H - 1, 0)]
    xp = NF.plant(x, where, VALUES)
    zp = conv64(xp)
    spread = ~torch.isfinite(zp[0])
    for slope in (0.2, 0.0):
        run = lambda t: hip_ops.convk_tasks_pre(t.to(DEV), pf, T, Ci, Co, K, b.to(DEV), 0, slope, pad, precise).cpu()
        ref_clean = R.act(conv64(x), slope)
        NF.hold(run(xp), R.act(zp, slope), run(x), footprint=spread if float(spread.float().mean()) <= NF.MAX_SHARE else None,
                tol=3e-6 * float(ref_clean.abs().max()), what="convk forward K=%d slope %g precise %d" % (K, slope, precise))
    gwhere = [(0, Ho // 2, Wo // 2), (Co - 1, 0, Wo - 1), (Co // 2, Ho - 1, 0)]
    gp = NF.plant(gy, gwhere, VALUES)
    run = lambda t: hip_ops.convk_tasks_pre(t.to(DEV), pb, T, Ci, Co, K, None, 1, 1.0, pad, precise).cpu()
    NF.hold(run(gp), dgrad64(gp), run(gy), tol=3e-6 * float(dgrad64(gy).abs().max()), what="convk data gradient K=%d precise %d" % (K, precise))


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("N,Ci,Co,H,W,K", [(2, 64, 64, 40, 56, 3), (2, 8, 64, 30, 41, 5)])
def test_direct_convolution_with_mirrored_border_keeps_non_finite_values(N, Ci, Co, H, W, K, precise):
    """reflect=True (CAIN's RCAB: the layer reads the reflection of its input) at the two-sample shapes of
    test_conv_with_mirrored_border_equals_reflection_pad_plus_conv (tests/test_hip_ops_gpu.py), plain and precise: a planted pixel next
    to the border is read through the mirror too.  Gate: that test's 5e-6 of max|ref|."""
    pad = K // 2
    g = torch.Generator().manual_seed(11 * H + K + 1)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(1, Co, Ci, K, K, generator=g) / (K * math.sqrt(Ci))
    b = torch.randn(1, Co, generator=g)
    pf, _ = hip_ops.convk_filters(w.to(DEV), True, False)
    run = lambda t: hip_ops.convk_tasks_pre(t.to(DEV), pf, 1, Ci, Co, K, b.to(DEV), 0, 0.2, pad, precise, True).cpu()
    ref64 = lambda t: F.leaky_relu(F.conv2d(F.pad(t.double(), (pad,) * 4, mode="reflect"), w[0].double(), b[0].double()), 0.2)
    xp = NF.plant(x, [(0, 1, 1), (Ci - 1, H - 2, W - 1), (5, H // 2, W // 2)], VALUES)
    NF.hold(run(xp), ref64(xp), run(x), tol=5e-6 * float(ref64(x).abs().max()), what="convk mirrored border K=%d precise %d" % (K, precise))


# =====================================================================================================================================
# weight and bias gradients
# =====================================================================================================================================
def _wgrad64(x, gz, T, pad, reflect=False):
    Co, Ci = gz.shape[1], x.shape[1]
    xs = F.pad(x.double(), (pad,) * 4, mode="reflect") if reflect else x.double()
    gw = torch.stack([torch.nn.grad.conv2d_weight(xs[t::T], (Co, Ci, 3, 3), gz.double()[t::T], padding=0 if reflect else pad) for t in range(T)], 0)
    gb = gz.double().view(gz.shape[0] // T, T, Co, -1).sum((0, 3))
    return gw, gb


def _small_map_wgrad(x, gz, T, pad, reflect):
    from tests.test_wgrad_small_maps_gpu import _run
    N, Ci, H, W = x.shape
    return _run(x, gz, N, T, Ci, gz.shape[1], H, W, pad, True)


def _wino_wgrad(x, gz, T, pad, reflect):
    """savfi_conv3x3_wgrad_wino_tasks_bias_f32 through the C ABI, as tests/test_hip_ops_gpu.py runs it at this shape"""
    lib, st = _hip.lib(), _hip.current_stream()
    N, Ci, H, W = x.shape
    Co = gz.shape[1]
    ws = torch.empty(int(lib.savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats(N, T, Ci, Co, H, W, pad)), device=DEV)
    gw, gb = torch.full((T, Co, Ci, 3, 3), NAN, device=DEV), torch.full((T, Co), NAN, device=DEV)
    _hip.check(lib.savfi_conv3x3_wgrad_wino_tasks_bias_f32(x.data_ptr(), gz.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                                           N, T, Ci, Co, H, W, pad, st), "wino wgrad")
    torch.cuda.synchronize()
    return gw, gb


def _mfma_wgrad(x, gz, T, pad, reflect):
    assert T == 1 and not hip_ops._wgrad_wino(x.shape[0], x.shape[1], gz.shape[1], gz.shape[2], gz.shape[3])
    return hip_ops.conv3x3_wgrad(x, gz, pad)[None], None


def _ring_wgrad(x, gz, T, pad, reflect):
    N, Ci, H, W = x.shape
    assert _hip.lib().savfi_convk_wgrad_sums_bias(N, T, Ci, gz.shape[1], H, W, 3, pad) == 1
    return hip_ops.convk_wgrad_tasks(x, gz, T, 3, pad, False, bool(reflect), want_bias=True)


def _convk_wgrad(x, gz, T, pad, reflect):
    return hip_ops.convk_wgrad_tasks(x, gz, T, 3, pad, False, bool(reflect)), None


# kernel, (N, T, Ci, Co, H, W, pad, reflect) from the tables of tests/test_hip_ops_gpu.py and tests/test_wgrad_small_maps_gpu.py: ragged ones
WGRAD_CASES = {
    "wgrad3x3":       (_mfma_wgrad, (3, 1, 40, 33, 9, 70, 1, 0)),               # WGRAD_SHAPES
    "wino_wgrad3x3":  (_wino_wgrad, (2, 2, 20, 70, 37, 53, 1, 0)),              # test_winograd_weight_gradient_hands_out_the_bias_gradient
    "ring":           (_ring_wgrad, (2, 2, 70, 100, 37, 53, 1, 0)),             # test_all_taps_weight_gradient_...
    "ring_mirrored":  (_ring_wgrad, (4, 2, 192, 192, 16, 16, 1, 1)),
    "small_map":      (_small_map_wgrad, (2, 2, 80, 72, 12, 16, 1, 0)),         # tests/test_wgrad_small_maps_gpu.py
    "convk_wgrad":    (_convk_wgrad, (2, 1, 64, 51, 17, 33, 1, 0)),             # CONVK_CASES
}


@pytest.mark.parametrize("planted", ["x", "gz"])
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_weight_and_bias_gradients_keep_non_finite_values(name, planted):
    """A NaN / inf in x makes the planted input channel's slice of task 0's weight gradient non-finite, one in the cotangent the planted
    output channel's slice and its bias gradient.  The footprint is that slice (a kernel that multiplies the planted pixel with zero
    padding makes the taps non-finite that the reference leaves out at a border); the gradients of the other tasks keep their bits.
    Gate: 3e-6 of max|ref| (tests/test_hip_ops_gpu.py), 1e-5 of the abs-sum for the bias gradient; the small-map kernel's own local
    gate (tests/test_wgrad_small_maps_gpu.py) for that kernel."""
    fn, (N, T, Ci, Co, H, W, pad, reflect) = WGRAD_CASES[name]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    g = torch.Generator().manual_seed(4500 + list(WGRAD_CASES).index(name))
    x, gz = torch.randn(N, Ci, H, W, generator=g), torch.randn(N, Co, Ho, Wo, generator=g)
    run = lambda a, c: fn(a.to(DEV), c.to(DEV), T, pad, reflect)
    gw0, gb0 = run(x, gz)
    rw0, rb0 = _wgrad64(x, gz, T, pad, reflect)
    tol_w = 3e-6 * float(rw0.abs().max())
    tol_b = 1e-5 * max(1.0, float(gz.double().abs().view(N // T, T, Co, -1).sum((0, 3)).max()))
    if name == "small_map":             # this kernel has a local gate of its own: c x 2^-24 x the sum of magnitudes, per element
        from tests.test_wgrad_small_maps_gpu import C_BIAS, C_WGRAD
        mw, mb = _wgrad64(x.abs(), gz.abs(), T, pad, reflect)
        tol_w, tol_b = R.local_bound(mw, C_WGRAD), R.local_bound(mb, C_BIAS)
    fp_w, fp_b = torch.zeros(Co, Ci, 3, 3, dtype=torch.bool), torch.zeros(Co, dtype=torch.bool)
    if planted == "x":
        where = [(1, H // 2, W // 2), (Ci - 1, 0, W - 1), (Ci // 2, H - 1, 0)]
        xp, gp = NF.plant(x, where, VALUES), gz
        for c, _, _ in where:
            fp_w[:, c] = True
    else:
        where = [(1, Ho // 2, Wo // 2), (Co - 1, 0, Wo - 1), (Co // 2, Ho - 1, 0)]
        xp, gp = x, NF.plant(gz, where, VALUES)
        for c, _, _ in where:
            fp_w[c] = True
            fp_b[c] = True
    gw, gb = run(xp, gp)
    rw, rb = _wgrad64(xp, gp, T, pad, reflect)
    NF.hold(gw, rw, gw0, footprint=fp_w, tol=tol_w, what="%s: weight gradient, planted %s" % (name, planted))
    if gb is not None:
        NF.hold(gb, rb, gb0, footprint=fp_b, tol=tol_b, reaches=planted == "gz", what="%s: bias gradient, planted %s" % (name, planted))


# =====================================================================================================================================
# channel attention
# =====================================================================================================================================
def _ca_ref64(inp):
    """float64 torch with its own relu / sigmoid and autograd: out, y and the six gradients"""
    t, x, w1, b1, w2, b2, g = (inp[k].double() for k in ("t", "x", "w1", "b1", "w2", "b2", "g"))
    leaves = [v.clone().requires_grad_() for v in (t, x, w1, b1, w2, b2)]
    t, x, w1, b1, w2, b2 = leaves
    N, T = t.shape[0], w1.shape[0]
    k = torch.arange(N) % T
    a1 = F.relu(torch.einsum("njc,nc->nj", w1[k], t.mean((2, 3))) + b1[k])
    y = torch.sigmoid(torch.einsum("ncj,nj->nc", w2[k], a1) + b2[k])
    out = t * y[:, :, None, None] + x
    grads = torch.autograd.grad(out, leaves, g)
    return dict(zip(("out", "y", "gt", "gx", "gw1", "gb1", "gw2", "gb2"), (out.detach(), y.detach()) + tuple(grads)))


def _ca_run(inp, T):
    N, C = inp["t"].shape[:2]
    Cr = inp["w1"].shape[1]
    leaves = [inp[k].to(DEV).requires_grad_() for k in ("t", "x")]
    for k, shape in (("w1", (T, Cr, C, 1, 1)), ("b1", (T, Cr)), ("w2", (T, C, Cr, 1, 1)), ("b2", (T, C))):
        leaves.append(inp[k].view(*shape).to(DEV).requires_grad_())
    out, y = hip_ops.channel_attention_residual(*leaves)
    grads = torch.autograd.grad(out, leaves, inp["g"].to(DEV))
    res = dict(zip(("out", "y", "gt", "gx", "gw1", "gb1", "gw2", "gb2"), (out.detach(), y.detach().view(N, C)) + tuple(grads)))
    return {k: v.cpu().reshape(_CA_SHAPES[k](N, T, C, Cr, inp["t"].shape[2], inp["t"].shape[3])) for k, v in res.items()}


_CA_SHAPES = dict(out=lambda N, T, C, Cr, H, W: (N, C, H, W), y=lambda N, T, C, Cr, H, W: (N, C), gt=lambda N, T, C, Cr, H, W: (N, C, H, W),
                  gx=lambda N, T, C, Cr, H, W: (N, C, H, W), gw1=lambda N, T, C, Cr, H, W: (T, Cr, C), gb1=lambda N, T, C, Cr, H, W: (T, Cr),
                  gw2=lambda N, T, C, Cr, H, W: (T, C, Cr), gb2=lambda N, T, C, Cr, H, W: (T, C))
CA_FWD, CA_PER_SAMPLE = ("out", "y"), ("out", "y", "gt", "gx")


@pytest.mark.parametrize("planted", ["t_nan", "t_inf", "w1_nan"])
@pytest.mark.parametrize("case,fuse", [((4, 2, 192, 12, 12, 20), True), ((4, 2, 192, 12, 12, 20), False), ((4, 2, 320, 20, 4, 6), False)],
                         ids=["fused", "one_round", "generic"])
def test_channel_attention_keeps_non_finite_values(case, fuse, planted, monkeypatch):
    """Both routes of tests/test_small_ops_branches_gpu.py (the fused launches, and pool + MLP + apply with the one-round and the generic
    kernels), forward and backward.  A NaN in the attention's input reaches the pooled vector, both 1x1 layers and the sigmoid: torch
    turns the whole sample NaN, and every parameter gradient of its task.  Gates: 2e-6 (forward) / 2e-5 (gradients) of the clean scale."""
    N, T, C, Cr, H, W = case
    monkeypatch.setattr(hip_ops, "CA_FUSE_MLP", fuse)
    inp = dict(SR.ca_case(*case)[0])
    clean, clean64 = _ca_run(inp, T), _ca_ref64(inp)
    bad = dict(inp)
    if planted == "t_nan":
        bad["t"] = NF.plant(inp["t"], [(C // 3, H // 2, W // 2)], [NAN])
    elif planted == "t_inf":
        bad["t"] = NF.plant(inp["t"], [(0, 0, 0), (C - 1, H - 1, W - 1)], [PINF, NINF])
    else:
        bad["w1"] = NF.plant(inp["w1"], [(Cr - 1, C - 1)], [NAN])
    got, ref = _ca_run(bad, T), _ca_ref64(bad)
    for key in got:
        tol = (2e-6 if key in CA_FWD else 2e-5) * max(float(clean64[key].abs().max()), 1e-12)
        a, r, c = got[key], ref[key], clean[key]
        if planted == "w1_nan" and key in CA_PER_SAMPLE:          # the planted weight belongs to task 0: its samples are 0, T, 2T, ...
            a, r, c = (_tasks_first(v, T) for v in (a, r, c))
        reaches = bool((~torch.isfinite(r[0])).any())
        assert reaches or key == "gx", key                        # gx = g: the residual's cotangent passes through
        NF.hold(a, r, c, tol=tol, reaches=reaches, what="channel attention %s %s: %s" % (case, planted, key))


# =====================================================================================================================================
# glue: point-wise ops, pooling, padding, permutations
# =====================================================================================================================================
@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
def test_bias_act_kernels_keep_non_finite_values(slope):
    """savfi_bias_act_fwd_f32 / _bwd_f32 through the C ABI on the odd plane 137 x 233, operands a float past an aligned address.  The
    arithmetic is the reference's: classes are held.  Deviation (footprint): with slope 0 a -inf (forward) or an infinite cotangent
    behind an inactive unit (backward) meets 0 * inf = NaN where torch selects 0."""
    N, C, H, W = 2, 5, 137, 233
    lib, st = _hip.lib(), _hip.current_stream()
    g = torch.Generator().manual_seed(19)
    n = N * C * H * W

    def shifted(t, s=1):
        buf = torch.empty(n + 8, device=DEV)
        view = buf[s:s + n]
        view.copy_(t.reshape(-1).to(DEV))
        return view

    act64 = lambda v: R.act(v.double(), slope)
    z, b = torch.randn(N, C, H, W, generator=g), torch.randn(C, generator=g)
    where = [(0, 0, 0), (2, 68, 117), (C - 1, H - 1, W - 1)]

    def fwd(t):
        v = shifted(t)
        _hip.check(lib.savfi_bias_act_fwd_f32(v.data_ptr(), b.to(DEV).data_ptr(), N, C, H * W, slope, st), "fwd")
        return v.cpu().view(N, C, H, W)

    zp = NF.plant(z, where, VALUES)
    fp = torch.zeros(C, H, W, dtype=torch.bool)
    if slope == 0.0:
        fp[where[2]] = True                                     # 0 * -inf
    tol = 2 * ULP * (z.double().abs() + b.double().abs().view(1, C, 1, 1))
    NF.hold(fwd(zp), act64(zp.double() + b.double().view(1, C, 1, 1)), fwd(z), footprint=fp, same_class=True, tol=tol, what="bias_act forward")

    gy, y = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    y[0][where[1]], y[0][where[2]] = 1.0, -1.0                   # the infinite cotangents: one behind an active unit, one behind an inactive

    def bwd(c, a):
        gz, gb = torch.zeros(n + 8, device=DEV)[1:1 + n], torch.empty(C, device=DEV)
        scratch = torch.empty(int(lib.savfi_bias_act_scratch_floats(N, C, H * W)), device=DEV)
        cv, av = shifted(c), shifted(a)
        _hip.check(lib.savfi_bias_act_bwd_f32(cv.data_ptr(), av.data_ptr(), gz.data_ptr(), gb.data_ptr(), scratch.data_ptr(),
                                              N, C, H * W, slope, st), "bwd")
        torch.cuda.synchronize()
        return gz.cpu().view(N, C, H, W), gb.cpu()

    def bwd64(c, a):
        v = a.double().clone().requires_grad_()                  # torch's own relu / leaky_relu backward at a pre-activation of y's sign
        gz, = torch.autograd.grad(act64(v), v, c.double())
        return gz, gz.sum((0, 2, 3))

    gz0, gb0 = bwd(gy, y)
    gp = NF.plant(gy, where, VALUES)
    gz, gb = bwd(gp, y)
    rz, rb = bwd64(gp, y)
    NF.hold(gz, rz, gz0, footprint=fp, same_class=True, tol=ULP * gy.double().abs(), what="bias_act backward: planted cotangent")
    tol_b = 1e-5 * float(gy.double().abs().sum((0, 2, 3)).max()) + 1e-6
    fpb = torch.zeros(C, dtype=torch.bool)
    fpb[where[2][0]] = slope == 0.0
    NF.hold(gb[None], rb[None], gb0[None], footprint=fpb, control=False, tol=tol_b, what="bias_act backward: bias gradient")
    # the stored activation only selects the factor (NaN and -inf: the slope, +inf: 1)
    yp = NF.plant(y, where, VALUES)
    gz, gb = bwd(gy, yp)
    NF.hold(gz, _act_bwd64(gy, yp, slope), gz0, tol=ULP * gy.double().abs(), reaches=False, what="bias_act backward: planted y")
    assert bool(torch.isfinite(gz).all()) and bool(torch.isfinite(gb).all())


@pytest.mark.parametrize("shape", [(3, 7, 13, 17), (2, 5, 12, 16)], ids=["odd_13x17", "even_12x16"])
def test_avg_pool_and_its_adjoints_keep_non_finite_values(shape):
    """avg_pool2x2 forward and adjoint on the odd map 13 x 17 (the last row and column are dropped: a value planted there reaches
    nothing) and the even map 12 x 16 (the kernels' two-float paths), both of test_pool_and_skip_adjoint_... in tests/test_hip_ops_gpu.py,
    and the pool-and-skip adjoint without and with the producer's activation derivative."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(23)
    x = torch.randn(N, C, H, W, generator=g)
    where = [(0, 0, 0), (3, 5, 8), (C - 1, H - 2, W - 2)]
    xp = NF.plant(x, where, VALUES)
    run = lambda t: hip_ops.avg_pool2x2(t.to(DEV)).cpu()
    NF.hold(run(xp), F.avg_pool2d(xp.double(), 2), run(x), tol=2 * ULP * F.avg_pool2d(x.double().abs(), 2), what="avg_pool2x2")
    if H % 2 and W % 2:
        dropped = NF.plant(x, [(0, H - 1, 3), (1, 2, W - 1)], [NAN, PINF])
        assert NF.bits_equal(run(dropped), run(x))

    a = torch.randn(N, C, H // 2, W // 2, generator=g)
    awhere = [(0, 0, 0), (3, 2, 4), (C - 1, H // 2 - 1, W // 2 - 1)]
    ap = NF.plant(a, awhere, VALUES)

    def adj(c):
        t = x.to(DEV).requires_grad_()
        return torch.autograd.grad(hip_ops.avg_pool2x2(t), t, c.to(DEV))[0].cpu()

    def adj64(c):
        t = x.double().requires_grad_()
        return torch.autograd.grad(F.avg_pool2d(t, 2), t, c.double())[0]

    NF.hold(adj(ap), adj64(ap), adj(a), same_class=True, tol=ULP * adj64(a).abs(), what="avg_pool2x2 adjoint")

    for slope in (None, 0.0, 0.2):
        skip = torch.randn(N, C, H, W, generator=g)
        act = x.clone()
        act[0, 3, 4:6, 8:10] = torch.tensor([[1.0, -1.0], [2.0, -2.0]])        # the +inf cotangent's four pixels: two active, two not

        def fused(c, s_, y_):
            t = y_.to(DEV).requires_grad_()
            p, k = hip_ops.avg_pool2x2_and_skip(t, slope)
            return torch.autograd.grad([p, k], t, [c.to(DEV), s_.to(DEV)])[0].cpu()

        def fused64(c, s_, y_):
            return _act_bwd64(adj64(c) + s_.double(), y_, slope)

        fp = torch.zeros(C, H, W, dtype=torch.bool)
        if slope == 0.0:                                                        # 0 * inf behind an inactive unit
            bad = ~torch.isfinite(adj64(ap)[0]) & ~(act[0] > 0)
            fp |= bad
        tol = 2 * ULP * (adj64(a).abs() + skip.double().abs())
        NF.hold(fused(ap, skip, act), fused64(ap, skip, act), fused(a, skip, act), footprint=fp, tol=tol, what="pool-and-skip adjoint: pooled cotangent")
        sp = NF.plant(skip, where, VALUES)
        fp = torch.zeros(C, H, W, dtype=torch.bool)
        if slope == 0.0:
            for idx in where:
                fp[idx] = not bool(act[0][idx] > 0)
        NF.hold(fused(a, sp, act), fused64(a, sp, act), fused(a, skip, act), footprint=fp, tol=tol, what="pool-and-skip adjoint: skip cotangent")
        yp = NF.plant(act, where, VALUES)
        if slope is not None:
            NF.hold(fused(a, skip, yp), fused64(a, skip, yp), fused(a, skip, act), tol=tol, reaches=False, what="pool-and-skip adjoint: planted activation")


@pytest.mark.parametrize("pad", [1, 3])
def test_reflect_pad_and_its_fold_keep_non_finite_values(pad):
    shape = (2, 4, 33, 18)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(*shape, generator=g)
    N, C, H, W = shape
    where = [(0, 0, 0), (1, 1, W - 2), (C - 1, H - 1, W // 2)]                    # a corner (not mirrored), mirrored pixels, the last row
    xp = NF.plant(x, where, VALUES)
    run = lambda t: hip_ops.reflect_pad(t.to(DEV), pad).cpu()
    ref = lambda t: F.pad(t.double(), (pad,) * 4, mode="reflect")
    NF.hold(run(xp), ref(xp), run(x), same_class=True, what="reflect pad")
    gp_clean = torch.randn(N, C, H + 2 * pad, W + 2 * pad, generator=g)
    add = torch.randn(*shape, generator=g)
    gwhere = [(0, 0, 0), (1, pad + 1, pad + 1), (C - 1, H + 2 * pad - 1, W + pad)]
    gp = NF.plant(gp_clean, gwhere, VALUES)

    def fold64(c, extra):
        t = x.double().requires_grad_()
        return torch.autograd.grad(ref(t), t, c.double())[0] + (0 if extra is None else extra.double())

    for extra in (None, add):
        fold = lambda c: hip_ops.reflect_pad_bwd(c.to(DEV), pad, None if extra is None else extra.to(DEV)).cpu()
        mag = fold64(gp_clean.abs(), None if extra is None else extra.abs())
        NF.hold(fold(gp), fold64(gp, extra), fold(gp_clean), tol=4 * ULP * mag, what="reflect pad fold (add: %s)" % (extra is not None))


@pytest.mark.parametrize("r", [2, 4])
def test_pixel_shuffle_and_unshuffle_keep_non_finite_values(r):
    """A permutation: every bit arrives, a NaN's payload included.  The permutation itself is read off the kernel's result on the
    element indices (exact in float32) -- its values are held by tests/test_hip_ops_gpu.py."""
    N, C, H, W = 2, 3, 8, 12
    g = torch.Generator().manual_seed(31)
    for down, shape in ((True, (N, C, H, W)), (False, (N, C * r * r, H // r, W // r))):
        op = lambda t: hip_ops.pixel_shuffle(t.to(DEV), 1.0 / r if down else r).cpu()
        x = torch.randn(*shape, generator=g)
        index = op(torch.arange(x.numel(), dtype=torch.float32).reshape(shape))
        perm = index.long().reshape(-1)
        assert sorted(perm.tolist()) == list(range(x.numel()))
        xp = NF.plant(x, [(0, 0, 0), (1, 3 % shape[2], 7 % shape[3]), (shape[1] - 1, shape[2] - 1, shape[3] - 1)], VALUES)
        xp.view(torch.int32)[0, 2, 1, 1] = 0x7FC12345                              # a quiet NaN with a payload
        want = xp.reshape(-1)[perm].reshape(index.shape)
        got = op(xp)
        NF.hold(got, want.double(), op(x), same_class=True, what="pixel %s" % ("unshuffle" if down else "shuffle"))
        assert NF.bits_equal(got, want)


def test_sub_mean_keeps_non_finite_values():
    """(x - mean, mean) per plane: a planted plane is non-finite as a whole (inf - inf = NaN: classes are not held), the others keep
    their bits.  Gate: 1e-6 of max|x| on the mean of tests/test_hip_ops_gpu.py's two-stage sum."""
    shape = (2, 3, 37, 45)
    g = torch.Generator().manual_seed(37)
    x = torch.randn(*shape, generator=g) + 0.5
    for where, values in (([(0, 5, 6)], [NAN]), ([(1, 0, 0), (2, 36, 44)], [PINF, NINF])):
        xp = NF.plant(x, where, values)
        run = lambda t: [v.cpu() for v in hip_ops.sub_mean(t.to(DEV))]
        ref = lambda t: (t.double() - t.double().mean((2, 3), keepdim=True), t.double().mean((2, 3), keepdim=True))
        tol = 4e-6 * float(x.abs().max())
        for got, want, clean, what in zip(run(xp), ref(xp), run(x), ("difference", "mean")):
            NF.hold(got, want, clean, tol=tol, what="sub_mean %s %s" % (what, values))
            bad = {c for c, _, _ in where}
            for c in range(shape[1]):
                if c not in bad:
                    assert NF.bits_equal(got[0, c], clean[0, c]), "sub_mean: plane %d of the planted sample changed" % c


# ---- bilinear x2 ---------------------------------------------------------------------------------------------------------------------
def _bilinear_sets(bad, geom, align, adjoint):
    """(must, may) for the planted elements `bad` [planes, rows, cols] (bool) of the forward's source or the adjoint's cotangent:
    `must` = the results that a tap of non-zero weight joins to a planted element, `may` = those that any product of the kernels
    does.  Forward: an output's two taps per axis are i0 and i1 (tests/upsample_ref.py axis_sources) even where the weight of i1 is
    exactly 0.  Adjoint: source i gathers the candidate outputs 2i - 2 .. 2i + 3 of each axis (csrc/upsample.hip: the outputs with
    src(o) in (i - 1, i + 1) "and one more on each side ... extra candidates simply weigh zero") and multiplies every one."""
    from tests import upsample_ref as U
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    Ay, Ax = U.window_matrices(geom, align)                                        # [Hw, Hs], [Ww, Ws]
    Ty, Tx = torch.zeros_like(Ay), torch.zeros_like(Ax)
    iy0, iy1, _, _ = U.axis_sources(H, align)
    ix0, ix1, _, _ = U.axis_sources(W, align)
    for T_, n_out, o0, s0, n_src, i0, i1 in ((Ty, Hw, oy0, sy0, Hs, iy0, iy1), (Tx, Ww, ox0, sx0, Ws, ix0, ix1)):
        for o in range(n_out):
            taps = [i for i in range(s0, s0 + n_src) if 2 * i - 2 <= o0 + o <= 2 * i + 3] if adjoint else (int(i0[o0 + o]), int(i1[o0 + o]))
            for i in taps:
                if 0 <= i - s0 < n_src:
                    T_[o, i - s0] = 1
    hit = bad.flatten(1).any(1).nonzero().flatten()                                # the few planes that hold a planted element
    b = bad[hit].double()
    out_shape = (bad.shape[0], Hs, Ws) if adjoint else (bad.shape[0], Hw, Ww)

    def join(L, Rm):
        full = torch.zeros(out_shape, dtype=torch.bool)
        full[hit] = torch.einsum("oh,pow,wx->phx" if adjoint else "oh,phx,wx->pow", L, b, Rm) > 0
        return full
    return join((Ay != 0).double(), (Ax != 0).double()), join(Ty, Tx)


def _bilinear_ref(fn, t, geom, align, adjoint):
    """(reference, footprint of sample 0) of the linear map fn = U.fwd / U.bwd on the planted tensor t [N, C, rows, cols]"""
    N, C = t.shape[:2]
    planes = t.reshape(N * C, t.shape[2], t.shape[3])
    must, may = _bilinear_sets(~torch.isfinite(planes), geom, align, adjoint)
    ref = fn(torch.where(torch.isfinite(planes), planes, torch.zeros_like(planes)), geom, align)
    ref[must] = NAN
    out_shape = (N, C) + tuple(ref.shape[1:])
    return ref.reshape(out_shape), (may & ~must).reshape(out_shape)[0]


def _bilinear_adjoint_holds(y, gout, geom, align, slope, form, what, planted_activation):
    """The adjoint of the window `geom` (through hip_ops' autograd, (masked by y > 0 ? 1 : slope) on a planted cotangent and, where asked, on
    a planted stored activation; the library must report the adjoint form the case is about."""
    from tests import upsample_ref as U
    N, C, H, W = y.shape
    full, origin, win = geom[0:2], geom[2:4], geom[6:10]
    assert _hip.lib().savfi_upsample2x_bwd_form(N * C, H, W) == form == U.bwd_form(N * C, H, W), (what, N * C, H, W, form)
    planes = lambda t: t.reshape(N * C, t.shape[2], t.shape[3])

    def adj(c, act):
        t = act.to(DEV).requires_grad_()
        return torch.autograd.grad(hip_ops.upsample_bilinear2x_window(t, full, origin, win, align, slope), t, c.to(DEV))[0].cpu()

    gwhere = [(0, win[2] // 2, win[3] // 2), (C // 2, win[2] - 1, win[3] - 1), (C - 1, 0, 1)]
    gp = NF.plant(gout, gwhere, VALUES)
    tol = U.BWD_UNITS * ULP * U.bwd_abs(planes(gout), geom, align).reshape(N, C, H, W)
    clean = adj(gout, y)
    ref, fp = _bilinear_ref(U.bwd, gp, geom, align, True)
    if slope is not None:
        if slope == 0.0:                                                            # 0 * inf behind an inactive unit: torch's relu selects 0
            fp = fp | (~torch.isfinite(ref[0]) & ~(y[0] > 0))
        ref = _act_bwd64(ref, y, slope)
    NF.hold(adj(gp, y), ref, clean, footprint=fp, tol=tol, what="bilinear x2 adjoint %s slope %s" % (what, slope))
    if planted_activation:
        yp = NF.plant(y, [(0, H // 2, W // 2), (C // 2, H - 2, W - 3), (C - 1, 4, 5)], VALUES)
        ref = _act_bwd64(U.bwd(planes(gout), geom, align).reshape(N, C, H, W), yp, slope)
        NF.hold(adj(gout, yp), ref, clean, tol=tol, reaches=False, what="bilinear x2 adjoint %s: planted activation" % what)


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape,geom_kind,slope,form", [((3, 5, 12, 16), "full", None, 0), ((2, 7, 31, 45), "window", None, 1),
                                                        ((3, 5, 12, 16), "full", 0.0, 0), ((2, 64, 40, 70), "full", 0.2, 1)])
def test_bilinear_x2_forward_and_adjoints_keep_non_finite_values(shape, geom_kind, slope, form, align):
    """upsample_bilinear2x and its window form (shapes of tests/test_hip_ops_gpu.py: the per-pixel and the tiled adjoint), both
    align_corners, with and without the producer's activation derivative in the adjoint.  Reference: the float64 restatement of
    tests/upsample_ref.py (the op's float32 source coordinates; float64 F.interpolate takes other coordinates and is 1e-5 away) on the
    input with the planted elements zeroed, made NaN wherever a tap of non-zero weight reads a planted element.  Footprint: wherever a
    product of weight exactly 0 does: the forward's second tap (align_corners: output 0 reads source 1 with weight 0; torch multiplies it
    too) and the adjoint's candidate window of six outputs per axis.  Gates: 8 / 16 x 2^-24 x abs-sum of that module."""
    from tests import upsample_ref as U
    N, C, H, W = shape
    g = torch.Generator().manual_seed(41 + H)
    x = torch.randn(*shape, generator=g)
    if geom_kind == "full":
        full, origin, win = (H, W), (0, 0), (0, 0, 2 * H, 2 * W)
    else:
        full, origin = (H + 9, W + 6), (4, 3)
        win = (2 * origin[0] + 6, 2 * origin[1] + 6, 2 * H - 14, 2 * W - 14)
    geom = (full[0], full[1], origin[0], origin[1], H, W) + win
    up = lambda t, sl=None: hip_ops.upsample_bilinear2x_window(t, full, origin, win, align, sl)
    planes = lambda t: t.reshape(N * C, t.shape[2], t.shape[3])
    where = [(0, H // 2, W // 2), (C // 2, H - 2, W - 3), (C - 1, 4, 5)]
    xp = NF.plant(x, where, VALUES)
    mag = U.fwd_abs(planes(x), geom, align).reshape(N, C, win[2], win[3])
    run = lambda t: up(t.to(DEV)).cpu()
    ref, fp = _bilinear_ref(U.fwd, xp, geom, align, False)
    torch_bad = ~torch.isfinite(_up64_plain(xp, C, full, origin, H, W, win, align))
    assert bool((torch_bad | fp[None].expand_as(torch_bad) == ~torch.isfinite(ref) | fp[None].expand_as(torch_bad)).all())   # float64 torch agrees on the set
    NF.hold(run(xp), ref, run(x), footprint=fp, tol=U.FWD_UNITS * ULP * mag, what="bilinear x2 forward %s" % geom_kind)
    gout = torch.randn(N, C, win[2], win[3], generator=g)
    _bilinear_adjoint_holds(x, gout, geom, align, slope, form, geom_kind, planted_activation=slope is not None)


# the plane counts of tests/test_upsample_forms_gpu.py at 41 x 70 and the streaming strip height each takes (FORMS_41x70), as two samples
STREAMING = [(2048, 32, None, True), (1400, 16, None, True), (1400, 16, None, False), (700, 8, None, True), (700, 8, 0.0, True), (2048, 32, 0.2, False)]


@pytest.mark.parametrize("planes,form,slope,align", STREAMING, ids=lambda v: str(v))
def test_bilinear_x2_streaming_adjoint_keeps_non_finite_values(planes, form, slope, align):
    """The streaming form of the adjoint (the one training batches run) at strip heights 32, 16 and 8, plain and with the producer's
    activation derivative (a planted cotangent, and a planted stored activation), on the 41 x 70 map of tests/test_upsample_forms_gpu.py."""
    from tests.test_upsample_forms_gpu import FORMS_41x70
    assert (planes, form) in FORMS_41x70
    N, C, H, W = 2, planes // 2, 41, 70
    g = torch.Generator().manual_seed(planes + form)
    y = torch.randn(N, C, H, W, generator=g)
    gout = torch.randn(N, C, 2 * H, 2 * W, generator=g)
    _bilinear_adjoint_holds(y, gout, (H, W, 0, 0, H, W, 0, 0, 2 * H, 2 * W), align, slope, form, "streaming %d rows" % form,
                            planted_activation=slope is not None)


def _up64_plain(t, C, full, origin, H, W, win, align):
    """float64 torch: the crop inside a zero map, F.interpolate, the window"""
    big = F.pad(t.double(), (origin[1], full[1] - origin[1] - W, origin[0], full[0] - origin[0] - H))
    out = F.interpolate(big, scale_factor=2, mode="bilinear", align_corners=align)
    return out[:, :, win[0]:win[0] + win[2], win[1]:win[1] + win[3]]


# =====================================================================================================================================
# losses
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_losses_keep_non_finite_values(kind):
    """L1 / MSE, whole and per sample, value and gradient (shape of tests/test_hip_ops_gpu.py: 3 x 4099 elements per row would be the
    ABI's; here the op's [N, C, H, W]).  Only the planted sample's row may be NaN; the gradient of L1 at a NaN difference is
    sign(NaN) = 0 in torch and in the kernel.  Gate: 1e-6 relative on the value, one rounding on the gradient."""
    N, C, H, W = 3, 3, 37, 45
    g = torch.Generator().manual_seed(43)
    a, b = torch.rand(N, C, H, W, generator=g), torch.rand(N, C, H, W, generator=g)
    gl = torch.randn(N, generator=g) + 2.0
    per, whole = (hip_ops.l1_loss_per_sample, hip_ops.l1_loss) if kind == "l1" else (hip_ops.mse_loss_per_sample, hip_ops.mse_loss)
    f64 = (lambda d: d.abs()) if kind == "l1" else (lambda d: d * d)

    def run(t):
        leaf = t.to(DEV).requires_grad_()
        rows = per(leaf, b.to(DEV))
        grad, = torch.autograd.grad(rows, leaf, gl.to(DEV))
        leaf2 = t.to(DEV).requires_grad_()
        one = whole(leaf2, b.to(DEV))
        grad1, = torch.autograd.grad(one, leaf2)
        return rows.detach().cpu(), grad.cpu(), one.detach().cpu().reshape(1), grad1.cpu()

    def ref(t):
        leaf = t.double().requires_grad_()
        rows = f64(leaf - b.double()).flatten(1).mean(1)
        grad, = torch.autograd.grad(rows, leaf, gl.double())
        leaf2 = t.double().requires_grad_()
        one = f64(leaf2 - b.double()).mean()
        grad1, = torch.autograd.grad(one, leaf2)
        return rows.detach(), grad, one.detach().reshape(1), grad1

    clean = run(a)
    for where, values in (([(1, 5, 6)], [NAN]), ([(0, 0, 0), (2, 36, 44)], [PINF, NINF])):
        ap = NF.plant(a, where, values)
        got, want = run(ap), ref(ap)
        NF.hold(got[0], want[0], clean[0], tol=1e-6, what="%s per sample" % kind)
        NF.hold(got[1], want[1], clean[1], same_class=True, tol=4 * ULP * want[1].abs().nan_to_num(0, 0, 0) + 1e-12, reaches=kind == "mse",
                what="%s per sample: gradient" % kind)
        NF.hold(got[2][None], want[2][None], clean[2][None], control=False, tol=1e-6, what="%s" % kind)
        NF.hold(got[3][None], want[3][None], clean[3][None], control=False, same_class=True, tol=4 * ULP * want[3].abs().nan_to_num(0, 0, 0) + 1e-12,
                reaches=kind == "mse", what="%s: gradient" % kind)


# =====================================================================================================================================
# multi-tensor ops
# =====================================================================================================================================
MT_PICK = [0, 3, 4, 5, 6, 7, 8, 9, 12]             # sizes 1, 5, 4095, 4096, 4097, 8191, 12288 and two random ones of tests/small_ops_ref.py


def _mt_lists():
    c = SR.mt_case()
    pick = lambda key: [c[key][i].clone() for i in MT_PICK]
    return dict(w=pick("w"), lr=pick("lr"), m=pick("m0"), s=pick("s0"), go=pick("go"), g=[c["g"][0][i].clone() for i in MT_PICK],
                steps=[c["steps"][i] for i in MT_PICK])


def _mt_plant(ts):
    """NaN, +inf and -inf into tensor 0 (one element), 2 and 5 of the list: the others are the control"""
    out = [t.clone() for t in ts]
    out[0][0] = NAN
    out[2][4094] = PINF
    out[5][17] = NINF
    return out, (0, 2, 5)


def _mt_hold(got, ref, clean, planted, tol, what, same_class=False, reaches=True):
    """per tensor: the planted ones through hold (their own element only: point-wise), the others equal their clean bits"""
    for i, (a, r, c) in enumerate(zip(got, ref, clean)):
        a, c = a.detach().cpu().reshape(-1), c.detach().cpu().reshape(-1)
        r = torch.as_tensor(np.asarray(r, np.float64)).reshape(-1)
        if i in planted:
            lim = tol * torch.clamp(r.abs().nan_to_num(0, 0, 0), min=1.0)
            NF.hold(a[None], r[None], c[None], control=False, same_class=same_class, tol=lim, reaches=reaches, what="%s tensor %d" % (what, i))
        else:
            assert NF.bits_equal(a, c), "%s: tensor %d has no planted value and changed" % (what, i)


@pytest.mark.parametrize("lr_mode", [SR.LR_SCALAR, SR.LR_ELEMENT])
@pytest.mark.parametrize("rule", [SR.RULE_SGD, SR.RULE_ADAM, SR.RULE_ADAMAX_LSLR, SR.RULE_ADAMAX_MSGD])
def test_mt_update_keeps_non_finite_gradients(rule, lr_mode):
    """A NaN or infinite gradient gives a non-finite weight, direction (coef) and, where the rule stores them, moments.  Tolerances:
    SR.RULE_TOL of tests/test_small_ops_branches_gpu.py."""
    L = _mt_lists()
    n = len(L["w"])
    bc1 = [1 - SR.BETA1 ** k for k in L["steps"]]
    sbc2 = [math.sqrt(1 - SR.BETA2 ** k) for k in L["steps"]]
    lrs = [torch.tensor(SR.MT_LR_TABLE[i % 4]) for i in range(n)] if lr_mode == SR.LR_SCALAR else L["lr"]

    def run(gs):
        m, s = _dev(*L["m"]), _dev(*L["s"])
        outs, coefs = hip_ops.mt_update_nograd(rule, lr_mode, _dev(*L["w"]), _dev(*gs), _dev(*lrs), m, s, bc1, sbc2, SR.BETA1, SR.BETA2, SR.EPS, True)
        torch.cuda.synchronize()
        return dict(out=outs, m=m, s=s, coef=coefs)

    def ref(gs):
        res = dict(out=[], m=[], s=[], coef=[])
        for i in range(n):
            lr = np.float64(np.float32(SR.MT_LR_TABLE[i % 4])) if lr_mode == SR.LR_SCALAR else lrs[i].double().numpy()
            with np.errstate(all="ignore"):
                o = SR.mt_update(rule, L["w"][i].numpy(), gs[i].numpy(), lr, L["m"][i].double().numpy(), L["s"][i].double().numpy(), bc1[i], sbc2[i])
            for key, v in zip(("out", "m", "s", "coef"), o):
                res[key].append(v)
        return res

    gp, planted = _mt_plant(L["g"])
    clean, got, want = run(L["g"]), run(gp), ref(gp)
    stores = {SR.RULE_SGD: (), SR.RULE_ADAM: ("m", "s"), SR.RULE_ADAMAX_LSLR: ("m",), SR.RULE_ADAMAX_MSGD: ()}[rule]
    for key in ("out", "coef", "m", "s"):
        tol = max(SR.RULE_TOL[rule][key], 2 * ULP)
        reaches = key in ("out", "coef") + stores
        _mt_hold(got[key], want[key], clean[key], planted, tol, "mt_update rule %d lr_mode %d %s" % (rule, lr_mode, key), reaches=reaches)


def test_mt_scale_mean_and_copy_keep_non_finite_values():
    L = _mt_lists()
    n = len(L["w"])
    wp, planted = _mt_plant(L["w"])
    gamma = torch.randn(n, generator=torch.Generator().manual_seed(4)) + 2.0
    # scale: gamma * w is one product -- classes held (gamma > 0 here)
    run = lambda ws: [o.detach() for o in hip_ops.mt_scale(gamma.to(DEV), _dev(*ws))]
    _mt_hold(run(wp), [SR.mt_scale(gamma[i].item(), wp[i].numpy()) for i in range(n)], run(L["w"]), planted, ULP, "mt_scale", same_class=True)
    # scale backward: g_w = gamma * g_out, g_gamma = <g_out, w>
    gop, _ = _mt_plant(L["go"])
    for what, gos, ws in (("planted cotangent", gop, L["w"]), ("planted weight", L["go"], wp)):
        gg, gws = hip_ops.mt_scale_grads(gamma.to(DEV), _dev(*ws), _dev(*gos))
        gg0, gws0 = hip_ops.mt_scale_grads(gamma.to(DEV), _dev(*L["w"]), _dev(*L["go"]))
        with np.errstate(all="ignore"):
            ref = [SR.mt_scale_bwd(gamma[i].item(), gos[i].numpy(), ws[i].numpy()) for i in range(n)]
        _mt_hold(gws, [r[0] for r in ref], gws0, planted, ULP, "mt_scale backward g_w, " + what, same_class=True, reaches=gos is gop)
        for i in range(n):
            a, c = gg[i].cpu().reshape(1), gg0[i].cpu().reshape(1)
            if i in planted:
                assert not bool(torch.isfinite(a).any()), "mt_scale backward g_gamma, %s: tensor %d came out finite" % (what, i)
            else:       # a sum of atomics over chunks: the op's tolerance, relative to the sum of magnitudes
                assert abs(float(a) - float(c)) <= 1e-5 * float((L["go"][i].double() * L["w"][i].double()).abs().sum()) + 1e-6, (what, i)
    # mean
    got, clean = hip_ops.mt_mean(_dev(*wp)).cpu(), hip_ops.mt_mean(_dev(*L["w"])).cpu()
    for i in range(n):
        if i in planted:
            assert not math.isfinite(float(got[i])), "mt_mean: tensor %d came out finite" % i
        else:
            assert abs(float(got[i]) - float(clean[i])) * L["w"][i].numel() <= 1e-5 * float(L["w"][i].abs().sum()) + 1e-6, i
    # copy: every bit, a NaN's payload included
    src = [t.clone() for t in wp]
    src[1].view(torch.int32)[2] = 0x7FC12345                        # a quiet NaN with a payload
    src[3].view(torch.int32)[7] = -0x3EDCBB                         # 0xFFC12345: negative, payload
    dsts = [torch.full_like(t, 9.0).to(DEV) for t in src]
    hip_ops.mt_copy(dsts, _dev(*src))
    for d, s_ in zip(dsts, src):
        assert NF.bits_equal(d.cpu(), s_), "mt_copy changed a bit"


# =====================================================================================================================================
# the 51-tap op
# =====================================================================================================================================
@pytest.mark.parametrize("frames8", [False, True], ids=["fp32_frames", "byte_frames"])
def test_sepconv_op_keeps_non_finite_taps_and_cotangents(frames8):
    """The 51-tap op at (B, Ho, Wo) = (2, 37, 36) of tests/test_sepconv_frames8_gpu.py, with fp32 frames (six bf16 products per fp32
    product) and with k / 255 frames (the byte-frame kernels, three): a NaN / inf in the vertical taps, in the horizontal taps and in the
    cotangent.  out[y, x] reads v[:, y, x] and h[:, y, x] only, gV reads h and gO, gH reads v and gO: the reference's non-finite set is
    the planted pixels' and no footprint beyond it is allowed (split products: an infinity may come out as NaN).  Gate: the 1e-5 of
    max|ref| of that file."""
    from oracle import torch_ops as O
    from tests import test_sepconv_frames8_gpu as S8
    B, Ho, Wo = 2, 37, 36
    inp, v, h, gO = S8._inputs(B, Ho, Wo, seed=100 * B + Ho, frames8=frames8)
    di = inp.to(DEV)
    words = S8._words(di)
    assert (int(words.abs().sum()) == 0) == frames8

    def run(v_, h_, g_):
        dv, dh, dg = _dev(v_, h_, g_)
        out = S8._abi_fwd(di, dv, dh, words)
        gV, gH = S8._abi_bwd(di, dv, dh, dg, words)
        torch.cuda.synchronize()
        return out.cpu(), gV.cpu(), gH.cpu()

    def ref(v_, h_, g_):
        v64, h64 = v_.double().requires_grad_(), h_.double().requires_grad_()
        out = O.sepconv_torch(inp.double(), v64, h64)
        gV, gH = torch.autograd.grad(out, [v64, h64], g_.double())
        return out.detach(), gV, gH

    clean, clean64 = run(v, h, gO), ref(v, h, gO)
    tols = [1e-5 * float(t.abs().max()) for t in clean64]
    twhere = [(0, 0, 0), (25, 18, 17), (50, Ho - 1, Wo - 1)]
    gwhere = [(0, 0, 0), (1, 18, 17), (2, Ho - 1, Wo - 1)]
    for what, args, reach in (("v", (NF.plant(v, twhere, VALUES), h, gO), (True, False, True)),
                              ("h", (v, NF.plant(h, twhere, VALUES), gO), (True, True, False)),
                              ("cotangent", (v, h, NF.plant(gO, gwhere, VALUES)), (False, True, True))):
        got, want = run(*args), ref(*args)
        for a, r, c, tol, rch, key in zip(got, want, clean, tols, reach, ("out", "gV", "gH")):
            NF.hold(a, r, c, tol=tol, reaches=rch, what="sepconv (%s frames) planted %s: %s" % ("byte" if frames8 else "fp32", what, key))
    assert _hip.lib().savfi_sepconv_ws_errors() == 0


# =====================================================================================================================================
# end to end: a NaN frame gives a NaN loss, and nothing keeps it
# =====================================================================================================================================
@pytest.mark.parametrize("model", ["sepconv", "voxelflow", "superslomo", "cain", "rrin"])
def test_a_nan_support_frame_gives_a_non_finite_loss_and_leaves_no_trace(model):
    """One task, one inner step at 64 x 64 (the builders of tests/test_system_gpu.py), as an evaluation iteration (the inner loop adapts,
    the outer weights stay): with one NaN pixel in the first support frame the loss is non-finite; the same task with the clean frame
    afterwards gives the clean loss bit for bit -- no state, filter store or moment keeps the NaN."""
    from tests.helpers import build_system
    over = dict(number_of_training_steps_per_iter=1, number_of_evaluation_steps_per_iter=1)
    if model == "voxelflow":
        over["weight_recipe"] = "smooth"
    system = build_system(model, over)
    frames = synthetic.septuplet_batch(1, 64, 64, model=model)
    loss = lambda fr: system.run_validation_iter(data_batch=fr)[0]["loss"].detach().cpu().reshape(1).clone()
    clean = loss(frames)
    assert bool(torch.isfinite(clean).all()), (model, clean)
    bad = [f.clone() for f in frames]
    bad[0][0, 1, 30, 33] = NAN
    planted = loss(bad)
    torch.cuda.synchronize()
    print("%s: clean loss %.8f, with a NaN support pixel %r" % (model, float(clean), float(planted)))
    assert not bool(torch.isfinite(planted).any()), "%s: a NaN support frame gave the finite loss %r" % (model, float(planted))
    again = loss(frames)
    assert NF.bits_equal(again, clean), "%s: the clean loss after a NaN iteration is %r, before it %r" % (model, float(again), float(clean))
