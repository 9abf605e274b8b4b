"""-m gpu: every op-layer launch between canaries, on allocations that start out as NaN (tests/helpers.py: guarded_calls,
poisoned_empties; tests/test_launch_guards_cpu.py holds the two instruments themselves).

(a) Every case of tests/test_launch_manifest_gpu.py runs twice from an empty filter store, plain and inside both instruments.  No canary
    may be touched, no returned tensor may hold a NaN or the integer poison, the two runs agree (bit for bit; the atomic-path cases of
    ATOMIC inside the tolerance of the op's own float64 test), and every symbol tests/golden/launch_manifest.json records for the case
    went through the guard or is listed in BYPASS with the reason it cannot.
(b) The manifest shapes are the smallest that REACH a path; many are aligned, where rounding up costs nothing.  OVERRUN runs the ragged
    members of the float64 suites inside both instruments, their value assertions unchanged: a write past a buffer shows as a touched
    canary, an element never written or a workspace read first as a NaN that fails the suite's own comparison.
(c) Whole training iterations run under the poison alone (about 1400 launches each: too many to guard one by one).

What the guard cannot see: a write through one view into the neighbouring slice of the SAME storage (guarded_calls' docstring)."""
import contextlib
import json

import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops
from tests import conv_ref as R
from tests import dain_ops_ref, warp_ref
from tests import test_adacof_gpu as A
from tests import test_census_gpu as CE
from tests import test_conv_variants_gpu as V
from tests import test_dain_net_ops_gpu as DN
from tests import test_dain_ops_gpu as D
from tests import test_dain_warp_slice_gpu as DS
from tests import test_hip_ops_gpu as T
from tests import test_laploss_gpu as LA
from tests import test_launch_manifest_gpu as M
from tests import test_metrics_gpu as ME
from tests import test_msssim_gpu as MS
from tests import test_pwc_ops_gpu as P
from tests import test_sepconv2_gpu as S2
from tests import test_sepconv_frames8_gpu as F8
from tests import test_small_ops_branches_gpu as SB
from tests import test_ssim_gpu as SS
from tests import test_system_gpu as SY
from tests import test_warp2_gpu as W2
from tests import test_warp_gpu as W1
from tests import test_wgrad_small_maps_gpu as WS
from tests.helpers import guarded_calls, integer_poison, poisoned_empties, record_launches

pytestmark = pytest.mark.gpu

DEV = "cuda"


@contextlib.contextmanager
def both():
    """both instruments, and the size queries hip_ops asked meanwhile (rec.queries)"""
    asked, query = set(), hip_ops._workspace_floats

    def spy(name, *shape):
        asked.add(name)
        return query(name, *shape)

    hip_ops._workspace_floats = spy
    try:
        with guarded_calls() as rec, poisoned_empties() as poison:
            rec.queries, rec.poison = asked, poison
            yield rec
        torch.cuda.synchronize()
    finally:
        hip_ops._workspace_floats = query


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the manifest cases
# ---------------------------------------------------------------------------------------------------------------------------------
# Entries launched without _hip.call: the guard cannot wrap them.  symbol -> reason (every case), (case, symbol) -> reason (one case).
BYPASS = {}         # (data.py's frame stager also calls lib() directly, but no manifest case launches it: nothing to list)
BYPASS_IN = {(case, "savfi_sepconv_fwd_frames8_f32"): "sepconv.py's _sepconv_fwd calls lib() directly: SAVFI_E_UNSUPPORTED falls through there"
             for case in ("sepconv-fp32", "sepconv-fp32-twice", "sepconv-frames8", "sepconv-frames8+gI", "sepconv-frames8-twice")}


def _bits(i, got, plain):
    return torch.equal(got, plain)


def _mt_close(count, summed):
    """The returned tensors `summed` (of `count`) are per-tensor sums that mt_update.hip adds up with one atomicAdd per block:
    SB._sum_close per element, with |value| in place of the sum of magnitudes (never larger: the tighter side).  Every other
    tensor is element-wise work and comes back bit for bit."""
    def close(i, got, plain):
        assert i < count, (i, count)
        if i not in summed:
            return torch.equal(got, plain)
        assert got.numel() <= 6, (i, tuple(got.shape))                                   # a scalar, one value per tensor, or [steps, tensors]
        a, b = got.double().reshape(-1).tolist(), plain.double().reshape(-1).tolist()
        return all(SB._sum_close(x, y, abs(y)) for x, y in zip(a, b))
    return close


def _voxel_close(i, got, plain):
    """g_frames (tensor 1 of the case): tests/test_warp_gpu.py's bound, the magnitudes and units from the float64 reference of the
    case's own inputs (redrawn as M._warp_once draws them)"""
    if i != 1:
        return torch.equal(got, plain)
    g = M._gen(1)
    frames, x3 = M._randn(g, *M.VOX[0]), M._randn(g, *M.VOX[1])
    gout = M._randn(g, M.VOX[0][0], 3, *M.VOX[0][2:])
    ref = warp_ref.voxel(frames.cpu(), x3.cpu(), gout.cpu())
    return warp_ref.bound_ratio(got, plain.double().cpu(), ref['g_frames_mag'] * ref['g_frames_units'], 1) <= 1.0


def _dain_warp_close(i, got, plain):
    """g_in (tensor 1 of the case): tests/test_dain_ops_gpu.py's gate max(K E, FLOOR scale) from the float32 and float64 references of
    the case's own inputs (redrawn as M._dain_warp draws them)"""
    if i != 1:
        return torch.equal(got, plain)
    g = M._gen(15)
    x, flow, filt = M._randn(g, 2, 3, 7, 9), 4 * M._randn(g, 2, 2, 7, 9), M._randn(g, 2, 16, 7, 9) / 4
    gout = M._randn(g, 2, 3, 7, 9)
    args = [t.cpu().numpy() for t in (x, flow, filt, gout)]
    E, scale = D.errs(dain_ops_ref.filterinterp_backward(*args, D.np.float32)[0], dain_ops_ref.filterinterp_backward(*args)[0])
    return float((got.double() - plain.double()).abs().max()) <= max(D.K * E, D.FLOOR * scale)


# The cases whose results pass through floating-point atomics (arrival order): case -> (the kernel it rests on, the comparison)
ATOMIC = {
    "voxelwarp+g_frames": ("voxelwarp.hip voxelwarp_bwd<true>: g_frames is scattered with atomicAdd", _voxel_close),
    "dain-warp": ("dainwarp.hip filterinterp_bwd: g_in is scattered with atomicAdd", _dain_warp_close),
    # 3 updated weights, 3 weight gradients, then the 3 scalar learning rates' gradients
    "mt_update-sgd": ("mt_update.hip mt_update_bwd: a scalar learning rate's gradient, one atomicAdd per block", _mt_close(9, {6, 7, 8})),
    # the accumulator's [steps, tensors] rows of the same sums
    "graph-loop-lr-grads": ("mt_update.hip mt_update_bwd: the same sums, from the graph loop's accumulator", _mt_close(1, {0})),
    # 3 scaled tensors; g_gamma + 3 g_w; g_gamma + g_w of the one live output; mt_scale_grads' g_gamma + 3 g_w; mt_mean's means
    "mt_scale": ("mt_update.hip mt_mean / mt_scale_bwd: per-tensor means and g_gamma, one atomicAdd per block",
                 _mt_close(14, {3, 7, 9, 13})),
}
# csrc/sepconv_ws.hip has atomics too, but no floating-point ones (LDS flags and work counters, an unsigned error count): every
# sepconv-* case is held to torch.equal.


def _run_manifest_case(name):
    hip_ops.filters_after_update([])
    hip_ops._pack_plans.clear()
    torch.cuda.synchronize()
    out = M.CASES[name]()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def manifest():
    with open(M.FIXTURE) as fh:
        return json.load(fh)


def test_the_atomic_and_bypass_lists_name_manifest_cases():
    assert set(ATOMIC) <= set(M.CASES) and {case for case, _ in BYPASS_IN} <= set(M.CASES)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_manifest_case_between_canaries_on_poisoned_allocations(name, manifest):
    plain = _run_manifest_case(name)
    with both() as rec:
        got = _run_manifest_case(name)
    assert plain and len(got) == len(plain), (name, len(got), len(plain))
    close = ATOMIC[name][1] if name in ATOMIC else _bits
    for i, (a, b) in enumerate(zip(got, plain)):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, i)
        if a.dtype.is_floating_point:
            assert not bool(torch.isnan(a).any()), "%s: returned tensor %d %s holds a NaN" % (name, i, tuple(a.shape))
        elif a.dtype != torch.bool:
            left = (a == integer_poison(a.dtype)) & (b != integer_poison(a.dtype))
            assert not bool(left.any()), "%s: returned tensor %d %s holds the integer poison" % (name, i, tuple(a.shape))
        assert close(i, a, b), "%s: returned tensor %d %s differs from the plain run" % (name, i, tuple(a.shape))
    recorded = {symbol for launch in manifest[name] for symbol in launch[1]}
    for symbol in sorted(recorded):
        bypassed = symbol in BYPASS or (name, symbol) in BYPASS_IN
        assert (symbol in rec.guarded) != bypassed, "%s: %s %s" % (
            name, symbol, "is listed as a bypass and went through the guard" if bypassed else "was launched outside the guard")


def test_the_manifest_names_no_symbol_outside_the_guard_and_the_bypass_lists(manifest):
    """Every symbol of the fixture belongs to a case (each held above to guard-or-bypass), and the bypass lists name real symbols."""
    assert sorted(manifest) == sorted(M.CASES)
    assert set(BYPASS) | {s for _, s in BYPASS_IN} <= set(_hip._PROTOTYPES)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the shapes where an overrun is possible
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _second_order_pass():
    """what tests/test_warp2_gpu.py's fixture of that name sets"""
    hip_ops.set_double_backward(True)
    hip_ops.set_warp_second_order(True)
    try:
        yield
    finally:
        hip_ops.set_double_backward(False)
        hip_ops.set_warp_second_order(False)


def _twice(fn, *args):
    with _second_order_pass():
        fn(*args, None)


def _pool_close(got, want, scale, Ci, Co, extra=0.0):
    d = got.cpu().double() - want
    if max(Ci, Co) <= 512:                             # T.conv3x3_close's gates, on the scale of the unpooled result
        return bool(d.abs().max() <= (2e-5 + extra) * scale) and bool(d.pow(2).mean().sqrt() <= (1e-6 + extra) * scale)
    return bool(d.abs().max() <= (2e-6 + extra) * scale)


def _pooled_epilogue(N, T_, Ci, Co, H, W, pad, in_kernel):
    """conv3x3_tasks_pre_pool against float64: y inside T.conv3x3_close, the pooled map against avg_pool2d of the float64 result inside
    the same gates on y's scale plus the pooling's own three roundings (3 * 2^-24 of four values no larger than that scale; * 0.25 is
    exact); and pooled == avg_pool2x2(y) bit for bit, the op's contract.  in_kernel: the convolution's output stage wrote it."""
    g = torch.Generator().manual_seed(41)
    x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T_, Co, generator=g)
    w = torch.randn(T_, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    u_f, _ = hip_ops.conv3x3_filters(w.to(DEV), True, False)
    with record_launches() as launches:
        y, pooled = hip_ops.conv3x3_tasks_pre_pool(x.to(DEV), u_f, T_, Ci, Co, b.to(DEV), 0.2, pad)
    assert ("avgpool2x2_fwd" not in launches.names) == in_kernel, launches.names
    z, _ = R.conv_tasks64(x, w, pad, T_, bias=b)
    ref = R.act(z, 0.2)
    assert y.shape == ref.shape and pooled.shape == ref.shape[:2] + (ref.shape[2] // 2, ref.shape[3] // 2)
    assert T.conv3x3_close(y.cpu().double(), ref, Ci, Co)
    assert _pool_close(pooled, F.avg_pool2d(ref, 2), ref.abs().max(), Ci, Co, extra=3 * R.ULP)
    assert torch.equal(pooled, hip_ops.avg_pool2x2(y))


def _plain_conv3x3(N, Ci, Co, H, W, pad):
    """hip_ops.conv3x3 forward and data gradient at an odd shape, against tests/conv_ref.py in float64"""
    g = torch.Generator().manual_seed(42)
    x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(1, Co, generator=g)
    w = torch.randn(1, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    z, _ = R.conv_tasks64(x, w, pad, 1, bias=b)
    y = hip_ops.conv3x3(x.to(DEV), w[0].to(DEV), b[0].to(DEV), 0, 0.2, pad)
    assert T.conv3x3_close(y.cpu().double(), R.act(z, 0.2), Ci, Co)
    gy = torch.randn(z.shape, generator=g)
    gx = hip_ops.conv3x3(gy.to(DEV), w[0].to(DEV), None, 1, 1.0, pad)
    assert T.conv3x3_close(gx.cpu().double(), R.dgrad_tasks64(gy, w, pad, 1)[0], Ci, Co)


def _plain_conv3x3_tasks(T_, n, Ci, Co, H, W, pad):
    g = torch.Generator().manual_seed(43)
    x, b = torch.randn(n * T_, Ci, H, W, generator=g), torch.randn(T_, Co, generator=g)
    w = torch.randn(T_, Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    z, _ = R.conv_tasks64(x, w, pad, T_, bias=b)
    y = hip_ops.conv3x3_tasks(x.to(DEV), w.to(DEV), b.to(DEV), 0, 0.0, pad)
    assert T.conv3x3_close(y.cpu().double(), R.act(z, 0.0), Ci, Co)
    gy = torch.randn(z.shape, generator=g)
    gx = hip_ops.conv3x3_tasks(gy.to(DEV), w.to(DEV), None, 1, 1.0, pad)
    assert T.conv3x3_close(gx.cpu().double(), R.dgrad_tasks64(gy, w, pad, T_)[0], Ci, Co)


def _plain_conv3x3_wgrad_tasks(T_, n, Ci, Co, H, W, pad):
    """hip_ops.conv3x3_wgrad_tasks at an odd shape against float64 autograd of tests/conv_ref.py's convolution, inside the bound of
    test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic (3e-6 of max |want|)"""
    g = torch.Generator().manual_seed(44)
    x = torch.randn(n * T_, Ci, H, W, generator=g)
    w = (torch.randn(T_, Co, Ci, 3, 3, generator=g) / 10).double().requires_grad_()
    z, _ = R.conv_tasks64(x, w, pad, T_)
    gz = torch.randn(z.shape, generator=g)
    want, = torch.autograd.grad(z, w, gz.double())
    got = hip_ops.conv3x3_wgrad_tasks(x.to(DEV), gz.to(DEV), T_, pad)
    assert got.shape == want.shape and (got.cpu().double() - want).abs().max() <= 3e-6 * want.abs().max()


def _convk_plain_entries(K, Ci, Co, H, W, pad, T_, N):
    """savfi_convk_tasks_pre_f32 (forward, data gradient) and savfi_convk_wgrad_tasks_f32 -- the entries without the mirrored border,
    which no op calls any more -- against float64, with the references and the bound of
    test_convk_forward_data_and_weight_gradient_match_float64; the workspace has exactly the floats its query names."""
    g = torch.Generator().manual_seed(K * 1000 + Ci + Co)
    x, b = torch.randn(N, Ci, H, W, generator=g), torch.randn(T_, Co, generator=g)
    w = torch.randn(T_, Co, Ci, K, K, generator=g) / (K * Ci ** 0.5)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    gy = torch.randn(N, Co, Ho, Wo, generator=g)
    pf, pb = hip_ops.convk_filters(w.to(DEV), True, True)
    xd, gd, bd = x.to(DEV), gy.to(DEV), b.to(DEV)
    y, gx, gw = torch.empty(N, Co, Ho, Wo, device=DEV), torch.empty(N, Ci, H, W, device=DEV), torch.empty(T_, Co, Ci, K, K, device=DEV)
    ws = torch.empty(hip_ops._workspace_floats("savfi_convk_wgrad_workspace_floats", N, T_, Ci, Co, H, W, K, pad), device=DEV)
    _hip.call("convk_fwd", "savfi_convk_tasks_pre_f32", xd, pf, bd, y, N, T_, Ci, Co, H, W, K, pad, 0, 0.2, 0)
    _hip.call("convk_bwd_data", "savfi_convk_tasks_pre_f32", gd, pb, None, gx, N, T_, Ci, Co, Ho, Wo, K, pad, 1, 1.0, 0)
    _hip.call("convk_wgrad", "savfi_convk_wgrad_tasks_f32", xd, gd, gw, ws, N, T_, Ci, Co, H, W, K, pad, 0)
    x64, w64, b64, g64 = x.double(), w.double(), b.double(), gy.double()
    z = torch.cat([F.conv2d(x64[n:n + 1], w64[n % T_], b64[n % T_], padding=pad) for n in range(N)], 0)
    gref = torch.cat([F.conv_transpose2d(g64[n:n + 1], w64[n % T_], padding=pad) for n in range(N)], 0)
    wref = torch.stack([torch.nn.grad.conv2d_weight(x64[t::T_], (Co, Ci, K, K), g64[t::T_], padding=pad) for t in range(T_)], 0)
    assert T._rel(y.cpu().double(), torch.where(z > 0, z, 0.2 * z)) < 3e-6
    assert T._rel(gx.cpu().double(), gref) < 3e-6 and T._rel(gw.cpu().double(), wref) < 3e-6


def _wino_bias_through_op(N, T_, Ci, Co, H, W, pad):
    """hip_ops.conv3x3_wgrad_tasks(want_bias=True) in its Winograd form (test_winograd_weight_gradient_hands_out_the_bias_gradient
    calls the library directly, so no canary surrounds it there): gw against float64 autograd per task inside the bound of
    test_conv3x3_wgrad_winograd_form_matches_autograd (3e-6 of max |want|), gb inside the bound of the hand-out test (1e-5 of the
    largest sum of magnitudes)."""
    g = torch.Generator().manual_seed(N * 1000 + Co)
    x = torch.randn(N, Ci, H, W, generator=g)
    gz = torch.randn(N, Co, H + 2 * pad - 2, W + 2 * pad - 2, generator=g)
    with M._knob(hip_ops, "WGRAD_WINO_MIN_GFLOP", 0.0):
        assert hip_ops.conv3x3_wgrad_tasks_sums_bias(tuple(x.shape), Co, T_, pad)
        gw, gb = hip_ops.conv3x3_wgrad_tasks(x.to(DEV), gz.to(DEV), T_, pad, want_bias=True)
    want = []
    for t in range(T_):
        w = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
        want.append(torch.autograd.grad(F.conv2d(x[t::T_].double(), w, None, padding=pad), w, gz[t::T_].double())[0])
    want = torch.stack(want)
    assert (gw.cpu().double() - want).abs().max() <= 3e-6 * want.abs().max()
    sums = gz.double().view(N // T_, T_, Co, -1)
    assert (gb.cpu().double() - sums.sum((0, 3))).abs().max().item() <= 1e-5 * sums.abs().sum((0, 3)).max().item()


CV = V.test_conv3x3_variant_matches_float64
RAGGED_VARIANTS = ["f4_fwd_ts4_v1_relu_T3", "f4_dgrad_ts5_v1_mask0", "f4_fwd_ragged_v1_T3", "f4_dgrad_ragged_v1_mask0_T3",
                   "f4_dgrad_split_v2_mask01", "f4_fwd_out16_T3", "f4_dgrad_in16_pad0_T3", "f2_fwd_odd_relu_T3", "f2_dgrad_odd_mask0",
                   "f2_fwd_split_beyond_512"]
SMALL_MAPS = [c for c in WS.CASES if c[2] % 64 or c[3] % 64 or (c[4] * c[5]) % 32]      # channels off the 64-band, pixels off the 32-unit
TILE_EDGES = [s for s in A.TILE if s[2] != A.R.TILE_H and s[3] != A.R.TILE_W]           # TILE_H +- 1 x TILE_W +- 1
Q = "savfi_%s_workspace_floats"

# id -> (call, the size queries and symbols the case must reach)
OVERRUN = {"variant-" + name: ((lambda name=name: CV(name, "normal")), ()) for name in RAGGED_VARIANTS}
OVERRUN.update({
    "pool-odd-9x13": (lambda: _pooled_epilogue(2, 1, 9, 31, 9, 13, 1, False), ("savfi_conv3x3_tasks_pre_pool_f32",)),
    "pool-in-kernel-12x16": (lambda: _pooled_epilogue(2, 1, 16, 40, 12, 16, 1, True), ("savfi_conv3x3_tasks_pre_pool_f32",)),
    "wgrad-1x3to5-5x7-p1": (lambda: T.test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic((1, 3, 5, 5, 7), 1),
                            (Q % "conv3x3_wgrad",)),
    "wgrad-3x40to33-9x70-p0": (lambda: T.test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic((3, 40, 33, 9, 70), 0),
                               (Q % "conv3x3_wgrad",)),
    # more than 16 splits: the two-level reduction, the only path that writes the second stage of the workspace (its last floats)
    "wgrad-2x51to51-18x130-p1-two-levels": (lambda: T.test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic(
        (2, 51, 51, 18, 130), 1), (Q % "conv3x3_wgrad",)),
    "wgrad-17x3to5-5x7-p1-two-levels": (lambda: T.test_conv3x3_weight_gradient_matches_autograd_and_is_deterministic(
        (17, 3, 5, 5, 7), 1), (Q % "conv3x3_wgrad",)),
    "wgrad-wino-bias": (lambda: T.test_winograd_weight_gradient_hands_out_the_bias_gradient(2, 2, 20, 70, 37, 53, 1), ()),
    "wgrad-wino-bias-through-the-op": (lambda: _wino_bias_through_op(2, 2, 20, 70, 37, 53, 1),
                                       ("savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats", "savfi_conv3x3_wgrad_wino_tasks_bias_f32")),
    "wgrad-all-taps-reflect": (lambda: T.test_all_taps_weight_gradient_matches_float64_and_hands_out_the_bias_gradient(
        2, 1, 192, 192, 33, 47, 1, 1), ()),
    "wgrad-all-taps": (lambda: T.test_all_taps_weight_gradient_matches_float64_and_hands_out_the_bias_gradient(
        2, 2, 70, 100, 37, 53, 1, 0), ()),
    "plain-conv3x3": (lambda: _plain_conv3x3(1, 5, 7, 9, 13, 1), (Q % "conv3x3", "savfi_conv3x3_f32")),
    "plain-conv3x3-tasks": (lambda: _plain_conv3x3_tasks(3, 1, 7, 5, 7, 11, 0), (Q % "conv3x3_tasks", "savfi_conv3x3_tasks_f32")),
    "plain-conv3x3-wgrad-tasks": (lambda: _plain_conv3x3_wgrad_tasks(3, 1, 7, 5, 7, 11, 1),
                                  (Q % "conv3x3_wgrad_tasks", "savfi_conv3x3_wgrad_tasks_f32")),
    "convk-5x5-co3": (lambda: T.test_convk_forward_data_and_weight_gradient_match_float64(5, 64, 3, 24, 40, 2, 1, 2, False), ()),
    "convk-plain-entries-5x5-11x13": (lambda: _convk_plain_entries(5, 20, 24, 11, 13, 0, 1, 1),
                                      ("savfi_convk_tasks_pre_f32", "savfi_convk_wgrad_tasks_f32")),
    "convk-plain-entries-7x7-co2": (lambda: _convk_plain_entries(7, 20, 2, 10, 12, 6, 1, 1),
                                    ("savfi_convk_tasks_pre_f32", "savfi_convk_wgrad_tasks_f32")),
    "convk-5x5-11x13": (lambda: T.test_convk_forward_data_and_weight_gradient_match_float64(5, 20, 24, 11, 13, 0, 1, 1, False), ()),
    "convk-7x7-co2": (lambda: T.test_convk_forward_data_and_weight_gradient_match_float64(7, 20, 2, 10, 12, 6, 1, 1, True), ()),
    "convk-5x5-reflect": (lambda: T.test_conv_with_mirrored_border_equals_reflection_pad_plus_conv(2, 8, 64, 30, 41, 5), ()),
    "sepconv2-7x5": (lambda: S2.test_double_backward_matches_the_restatement((1, 3, 7, 5, 5)), ()),
    "frames8-3x5x4": (lambda: F8.test_frames8_kernels_vs_oracle(3, 5, 4), ()),
    "frames8-2x37x36": (lambda: F8.test_frames8_kernels_vs_oracle(2, 37, 36), ()),
    "frames8-pair-2x37x36": (lambda: F8.test_pair_launch_gives_the_bits_of_the_two_launches(2, 37, 36, True, 0), ()),
    "ssim": (SS.test_hip_ops_surface, ()),
    "msssim": (MS.test_hip_ops_autograd_and_the_composed_form, ()),
    "lap-17x17": (lambda: LA.test_single_sample_matches_float64((17, 17)), ()),
    "lap-7x9-two-levels": (lambda: LA.test_fewer_levels_on_small_planes(2, (7, 9)), ()),
    "census-3x3": (lambda: CE.test_single_sample_matches_float64((3, 3)), ()),
    "census-7x9": (lambda: CE.test_single_sample_matches_float64((7, 9)), ()),
    "l1-rows": (lambda: T.test_l1_mse_vs_torch(0, (1, 3, 7, 5)), ()),
    "mse-rows": (lambda: T.test_l1_mse_vs_torch(1, (1, 3, 7, 5)), ()),
    "l1-per-sample": (lambda: T.test_per_sample_losses(0), ()),
    "mse-per-sample": (lambda: T.test_per_sample_losses(1), ()),
    "charbonnier-105": (lambda: DN.test_charbonnier_loss_and_gradients(2, 105), ()),
    "psnr-ssim": (ME.test_hip_ops_surface_and_the_path_selection, ()),
    "frames-to-u8-11x11": (lambda: ME.test_writer_bytes_equal_torch_quantize_exactly("noise", (11, 11)), ()),
    "upsample-full-5x9": (lambda: T.test_upsample2x_matches_aten(False, (2, 7, 5, 9)), ()),
    "upsample-full-1x1": (lambda: T.test_upsample2x_matches_aten(True, (1, 3, 1, 1)), ()),
    "upsample-window-odd": (lambda: T.test_upsample_window_matches_full_op(True, (17, 19, 0, 9, 10, 19, 0, 23, 15, 15)), ()),
    "avgpool-7x9": (lambda: T.test_avgpool2x2_matches_aten(1, 5, 7, 9), ()),
    "avgpool-2x2": (lambda: T.test_avgpool2x2_matches_aten(1, 3, 2, 2), ()),
    "pixel-shuffle-9x15": (lambda: T.test_pixel_shuffle_roundtrip_and_oracle(1, 2, 9, 15, 3), ()),
    "reflect-pad-7x9": (lambda: T.test_reflect_pad_op_has_atens_values_and_gradient((1, 3, 7, 9), 2), ()),
    "sub-mean-1x1": (lambda: T.test_sub_mean_matches_the_two_stage_mean((3, 2, 1, 1)), (Q % "sub_mean",)),
    "sub-mean-37x45": (lambda: T.test_sub_mean_matches_the_two_stage_mean((2, 3, 37, 45)), (Q % "sub_mean",)),
    "bias-act-7x9-shift1": (lambda: T.test_bias_act_kernels_on_odd_planes(1, 3, 7, 9, 0.2, 1), ()),
    "bias-act-1x1-shift3": (lambda: T.test_bias_act_kernels_on_odd_planes(3, 2, 1, 1, 0.0, 3), ()),
    "channel-attention-33x47": (lambda: T.test_channel_attention_residual_matches_the_composed_ops(1, 1, 64, 4, 33, 47), ()),
    "channel-attention-5x7": (lambda: T.test_channel_attention_residual_matches_the_composed_ops(3, 3, 16, 2, 5, 7), ()),
    "batchnorm-slice-3x5": (lambda: DN.test_batchnorm_train_mode_into_a_channel_slice("odd_two_groups", True), ()),
    "maxpool-5x7": (lambda: DN.test_maxpool_equals_torch_bit_for_bit((5, 7)), ()),
    "upnearest-add-3x5": (lambda: DN.test_upnearest2x_add_equals_the_host_composition((3, 5)), ()),
    "voxelwarp-5x3": (lambda: T.test_voxelwarp_vs_oracle(1, 5, 3, 2.0), ()),
    "voxelwarp-1x7": (lambda: T.test_voxelwarp_vs_oracle(1, 1, 7, 1.0), ()),
    "voxelwarp-lattice-2x3": (lambda: W1.test_voxelwarp_fused_op_against_float64((1, 2, 3), None), ()),
    "flowwarp-1x1": (lambda: T.test_flowwarp_vs_oracle(1, 1, 1, 1, 0.7), ()),
    "flowwarp-3x300": (lambda: T.test_flowwarp_vs_oracle(2, 5, 3, 300, 2.0), ()),
    "voxelwarp-twice-2x3": (lambda: _twice(W2.test_voxelwarp_bwd2_against_float64, (1, 2, 3), None), ()),
    "voxelwarp-twice-5x1": (lambda: _twice(W2.test_voxelwarp_bwd2_against_float64, (1, 5, 1), None), ()),
    "flowwarp-twice-1x1": (lambda: _twice(W2.test_flowwarp_bwd2_against_float64, (1, 1, 1, 1), None), ()),
    "flowwarp-twice-6x70": (lambda: _twice(W2.test_flowwarp_bwd2_against_float64, (1, 3, 6, 70), 1.0), ()),
    "correlation-3x5": (lambda: P.test_correlation_autograd_matches_the_abi((1, 3, 3, 5), "normal"), ()),
    "pwc-warp-1x1": (lambda: P.test_warp_abi_matches_float64((1, 1, 1, 1), "uniform", 1.0), ("savfi_pwcwarp_fwd_f32",)),
    "pwc-warp-7x9": (lambda: P.test_warp_abi_matches_float64((2, 3, 7, 9), "uniform", 0.625), ("savfi_pwcwarp_fwd_f32",)),
    "filterinterp-7x9": (lambda: D.test_warp_autograd_matches_the_abi((2, 3, 7, 9), "uniform"), ()),
    "filterinterp-slice-7x9": (lambda: DS.test_slice_holds_the_warp_and_nothing_else_moves((2, 3, 7, 9), 3, 0), ()),
    "depthflowproj-7x9": (lambda: D.test_proj_autograd_matches_the_abi((2, 3, 7, 9), "uniform"), ()),
    "adacof-6x6-f11-d2": (lambda: A.test_autograd_equals_the_abi_and_gradient_outputs_may_be_null((1, 3, 6, 6, 11, 2)), ()),
})
OVERRUN.update({"sepconv-%dx%dx%dx%dx%d" % c: ((lambda c=c: T.test_sepconv_forward_backward_vs_oracle(*c)), ())
                for c in [(2, 3, 37, 45, 51), (1, 1, 9, 70, 51), (2, 4, 10, 33, 3), (1, 2, 1, 1, 1)]})
OVERRUN.update({"wgrad-small-n%dt%d_%dto%d_%dx%d_p%d" % c: ((lambda c=c: WS.test_small_map_wgrad_matches_float64(c)), ()) for c in SMALL_MAPS})
OVERRUN.update({"adacof-tile-%dx%d" % s[2:4]: ((lambda s=s: A.test_autograd_equals_the_abi_and_gradient_outputs_may_be_null(s)), ())
                for s in TILE_EDGES})


# These suites call the library directly (their own arenas and canaries): nothing passes through _hip.call, the poison alone acts -- on
# the scratch and output blocks they take from torch.empty.  (The Winograd bias hand-out runs between canaries in
# wgrad-wino-bias-through-the-op, the bias + activation kernels in the manifest's conv cases.)
ABI_DIRECT = {"bias-act-7x9-shift1", "bias-act-1x1-shift3", "wgrad-wino-bias"}


def test_the_ragged_lists_are_what_they_claim():
    assert ABI_DIRECT <= set(OVERRUN)
    assert all(name in V.CASES for name in RAGGED_VARIANTS)
    assert len(SMALL_MAPS) >= 3 and len(TILE_EDGES) == 4
    assert (3, 40, 33, 9, 70) in T.WGRAD_SHAPES and (1, 3, 5, 5, 7) in T.WGRAD_SHAPES
    assert {(5, 64, 3, 24, 40, 2, 1, 2), (5, 20, 24, 11, 13, 0, 1, 1), (7, 20, 2, 10, 12, 6, 1, 1)} <= set(T.CONVK_CASES)
    assert {(2, 3, 37, 45, 51), (1, 1, 9, 70, 51), (2, 4, 10, 33, 3), (1, 2, 1, 1, 1)} <= set(T.SEPCONV_CASES)


@pytest.mark.parametrize("name", sorted(OVERRUN))
def test_ragged_shape_between_canaries_on_poisoned_allocations(name):
    run, reaches = OVERRUN[name]
    hip_ops.filters_after_update([])
    torch.cuda.synchronize()
    with both() as rec:
        run()
    assert (sum(rec.guarded.values()) > 0) != (name in ABI_DIRECT), "%s: %d launches through _hip.call" % (name, sum(rec.guarded.values()))
    missing = [r for r in reaches if r not in rec.queries and r not in rec.guarded]
    assert not missing, (name, missing, sorted(rec.guarded), sorted(rec.queries))


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) whole iterations on poisoned allocations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SY.SYSTEM)
def test_training_iteration_matches_its_fixture_on_poisoned_allocations(name):
    with poisoned_empties() as poison:
        SY.test_iteration_matches_reference_fixture(name, "train")
    assert poison.filled > 0
