"""The float64 restatements of DAIN's two CUDA extensions (tests/dain_ops_ref.py) pinned on their own, without a GPU: identities,
adjoints, central differences and hand-evaluated cases.  The GPU tests (tests/test_dain_ops_gpu.py) then hold the kernels to them.

Flows of the difference tests are multiples of 2^-10 and the step is 2^-12, so that x2 +- step is exact in the float32 the decisions
are taken in; both ops are (bi)linear in the flow inside a cell, so the central difference is exact up to float64 rounding.
"""
import numpy as np

from tests import dain_ops_ref as R


def _dyadic(rng, shape, lo, hi):
    """multiples of 2^-10 in [lo, hi] whose fractional part stays 1e-3 away from 0 and 1"""
    whole = rng.integers(lo, hi, size=shape).astype(np.float64)
    frac = rng.integers(8, 1016, size=shape).astype(np.float64) / 1024.0
    return (whole + frac).astype(np.float32)


def _warp_case(seed, B=2, C=3, H=9, W=11):
    rng = np.random.default_rng(seed)
    inp = rng.standard_normal((B, C, H, W)).astype(np.float32)
    filt = rng.standard_normal((B, 16, H, W)).astype(np.float32)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32)
    flow = _dyadic(rng, (B, 2, H, W), -3, 3)
    return inp, flow, filt, gout


def _valid_mask(flow, H, W):
    B = flow.shape[0]
    m = np.zeros((B, H, W), bool)
    for b in range(B):
        for h in range(H):
            for w in range(W):
                m[b, h, w] = R.warp_geom(flow[b, 0, h, w], flow[b, 1, h, w], w, h, W, H) is not None
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# adaptive warping
# ---------------------------------------------------------------------------------------------------------------------------------
def test_warp_zero_flow_one_hot_tap5_reproduces_the_input():
    rng = np.random.default_rng(0)
    inp = rng.standard_normal((2, 3, 6, 7)).astype(np.float32)
    flow = np.zeros((2, 2, 6, 7), np.float32)
    filt = np.zeros((2, 16, 6, 7), np.float32)
    filt[:, 5] = 1.0                      # tap (1, 1): window origin (x-1, y-1), so the pixel itself; alpha = beta = 0 keeps TL only
    assert np.array_equal(R.filterinterp_forward(inp, flow, filt), inp.astype(np.float64))


def test_warp_g_in_and_g_filt_are_the_adjoints():
    inp, flow, filt, gout = _warp_case(1)
    B, C, H, W = inp.shape
    valid = _valid_mask(flow, H, W)
    assert valid.any() and not valid.all()
    g_in, _, g_filt = R.filterinterp_backward(inp, flow, filt, gout)
    rng = np.random.default_rng(2)
    d_in = rng.standard_normal(inp.shape).astype(np.float32)
    d_filt = rng.standard_normal(filt.shape).astype(np.float32)
    # the forward is bilinear in (in, filt) on the valid pixels: <gout, F(d_in, filt)> = <g_in, d_in>, <gout, F(in, d_filt)> = <g_filt, d_filt>
    vm = valid[:, None].astype(np.float64)
    lhs = float((gout * vm * R.filterinterp_forward(d_in, flow, filt)).sum())
    rhs = float((g_in * d_in).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    lhs = float((gout * vm * R.filterinterp_forward(inp, flow, d_filt)).sum())
    rhs = float((g_filt * d_filt).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)


def test_warp_g_flow_equals_a_central_difference():
    inp, flow, filt, gout = _warp_case(3, B=1, C=2, H=7, W=9)
    B, C, H, W = inp.shape
    _, g_flow, _ = R.filterinterp_backward(inp, flow, filt, gout)
    step = np.float32(2.0 ** -12)
    valid = _valid_mask(flow, H, W)
    checked = 0
    for ch in range(2):
        for h in range(H):
            for w in range(W):
                if not valid[0, h, w]:
                    continue
                # away from the validity bounds as well: x2, y2 at least 1e-3 inside [0, W-1] x [0, H-1] and |f| below the half size
                x2, y2 = w + float(flow[0, 0, h, w]), h + float(flow[0, 1, h, w])
                if not (1e-3 <= x2 <= W - 1 - 1e-3 and 1e-3 <= y2 <= H - 1 - 1e-3 and abs(flow[0, 0, h, w]) < W / 2 - 1e-3
                        and abs(flow[0, 1, h, w]) < H / 2 - 1e-3):
                    continue
                fp, fm = flow.copy(), flow.copy()
                fp[0, ch, h, w] += step
                fm[0, ch, h, w] -= step
                op = R.filterinterp_forward(inp, fp, filt)[0, :, h, w]
                om = R.filterinterp_forward(inp, fm, filt)[0, :, h, w]
                num = float((gout[0, :, h, w] * (op - om)).sum() / (2.0 * float(step)))
                assert abs(num - g_flow[0, ch, h, w]) <= 1e-9 * max(1.0, abs(num)), (ch, h, w, num, g_flow[0, ch, h, w])
                checked += 1
    assert checked >= 40


def test_warp_invalid_pixels_pass_the_input_and_give_no_gradient():
    inp, flow, filt, gout = _warp_case(4)
    B, C, H, W = inp.shape
    flow[0, 0, 2, 3] = np.nan
    flow[1, 1, 4, 5] = np.inf
    flow[0, 0, 0, 0] = -0.5               # x2 < 0
    flow[0, 0, 5, W - 1] = 0.25           # x2 > W - 1
    flow[1, 0, 3, 8] = -(W / 2.0)         # inside the frame, |fx| = W/2 fails the strict test
    valid = _valid_mask(flow, H, W)
    for b, h, w in ((0, 2, 3), (1, 4, 5), (0, 0, 0), (0, 5, W - 1), (1, 3, 8)):
        assert not valid[b, h, w]
    out = R.filterinterp_forward(inp, flow, filt)
    inv = ~valid
    assert np.array_equal(out.transpose(0, 2, 3, 1)[inv], inp.astype(np.float64).transpose(0, 2, 3, 1)[inv])
    assert not np.isnan(out).any()
    # every gradient of a cotangent that lives on invalid pixels only is zero -- g_in too, although the forward copies `in` there
    g_only = gout * inv[:, None]
    g_in, g_flow, g_filt = R.filterinterp_backward(inp, flow, filt, g_only)
    assert not g_in.any() and not g_flow.any() and not g_filt.any()
    g_in, g_flow, g_filt = R.filterinterp_backward(inp, flow, filt, gout)
    assert not g_flow.transpose(0, 2, 3, 1)[inv].any() and not g_filt.transpose(0, 2, 3, 1)[inv].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# depth-aware flow projection
# ---------------------------------------------------------------------------------------------------------------------------------
def _single_source(H, W, h, w, fx, fy, wv):
    flow = np.full((1, 2, H, W), 1000.0, np.float32)          # every other source leaves the frame
    flow[0, :, h, w] = (fx, fy)
    wgt = np.full((1, 1, H, W), 0.5, np.float32)
    wgt[0, 0, h, w] = wv
    return flow, wgt


def test_proj_single_interior_source():
    flow, wgt = _single_source(6, 8, 2, 3, 1.25, 0.5, 0.75)
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    targets = {(2, 4), (2, 5), (3, 4), (3, 5)}                # x2 = 4.25, y2 = 2.5
    for h in range(6):
        for w in range(8):
            if (h, w) in targets:
                assert count[0, 0, h, w] == 0.75 and out[0, 0, h, w] == -1.25 and out[0, 1, h, w] == -0.5
            else:
                assert count[0, 0, h, w] == 0 and not out[0, :, h, w].any()


def test_proj_source_on_the_last_column_hits_two_targets_twice():
    flow, wgt = _single_source(6, 8, 2, 5, 2.0, 0.5, 0.75)   # x2 = 7 = W - 1: L = R = 7
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    assert count[0, 0, 2, 7] == 1.5 and count[0, 0, 3, 7] == 1.5 and np.count_nonzero(count) == 2
    assert out[0, 0, 2, 7] == -2.0 and out[0, 1, 3, 7] == -0.5
    flow, wgt = _single_source(6, 8, 2, 5, 2.0, 3.0, 0.75)   # and the last row: one target, four hits
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    assert count[0, 0, 5, 7] == 3.0 and np.count_nonzero(count) == 1 and out[0, 0, 5, 7] == -2.0 and out[0, 1, 5, 7] == -3.0


def test_proj_hole_fill_on_a_hand_built_field():
    # 5 x 7, two samples.  Sample 0 has two scattered sources with integer flows: A = (-2, -1) at (1, 2) lands on (0, 0) and covers the
    # 2 x 2 block below (one hit each, out = (2, 1)); B = (3, 2) at (2, 3) lands on the corner (4, 6), where L = R and T = Bt make
    # one target of four hits (count 4, out = (-3, -2)).  Sample 1 has no valid source at all.
    #        0 1 2 3 4 5 6
    #   0    A A . . . . .
    #   1    A A . . . . .
    #   2    . . . . . . .
    #   3    . . . . . . .
    #   4    . . . . . . B
    H, W = 5, 7
    flow = np.full((2, 2, H, W), 1000.0, np.float32)
    wgt = np.ones((2, 1, H, W), np.float32)
    flow[0, :, 1, 2] = (-2.0, -1.0)
    flow[0, :, 2, 3] = (3.0, 2.0)
    A, Bv = (2.0, 1.0), (-3.0, -2.0)
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    block = {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(h, w) for h in range(H) for w in range(W) if count[0, 0, h, w] > 0} == block | {(4, 6)}
    assert count[0, 0, 4, 6] == 4.0 and all(count[0, 0, h, w] == 1.0 for h, w in block)
    filled, count2 = R.depthflowproj_forward(flow, wgt, 1)
    assert np.array_equal(count, count2)
    for k in block:
        assert tuple(filled[0, :, k[0], k[1]]) == A                                  # sources are never written
    assert tuple(filled[0, :, 4, 6]) == Bv
    half = tuple((a + b) / 2.0 for a, b in zip(A, Bv))
    assert tuple(filled[0, :, 0, 3]) == A                                            # left only: nothing right, above or below
    assert tuple(filled[0, :, 1, 2]) == A
    assert tuple(filled[0, :, 4, 0]) == half                                         # right B, above A; nothing left or below
    assert tuple(filled[0, :, 1, 6]) == half                                         # left A, below B
    assert tuple(filled[0, :, 2, 6]) == Bv                                           # below only
    assert tuple(filled[0, :, 2, 3]) == (0.0, 0.0)                                   # no valid pixel in its row or column: stays 0
    assert tuple(filled[0, :, 3, 4]) == (0.0, 0.0)
    assert not filled[1].any() and not count2[1].any()                               # the sample without a valid source


def test_proj_integer_flow_targets():
    # an integer landing position inside the frame hits (T,L), (T,R), (Bt,L), (Bt,R) with R = L + 1, Bt = T + 1: four pixels
    flow, wgt = _single_source(5, 7, 1, 1, 1.0, 1.0, 2.0)
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    assert {(h, w) for h in range(5) for w in range(7) if count[0, 0, h, w] > 0} == {(2, 2), (2, 3), (3, 2), (3, 3)}


def _proj_case(seed, B=1, H=7, W=9):
    rng = np.random.default_rng(seed)
    flow = _dyadic(rng, (B, 2, H, W), -3, 3)
    wgt = rng.uniform(0.1, 2.0, (B, 1, H, W)).astype(np.float32)
    gout = rng.standard_normal((B, 2, H, W)).astype(np.float32)
    return flow, wgt, gout


def test_proj_g_flow_equals_a_central_difference():
    flow, wgt, gout = _proj_case(5)
    B, _, H, W = flow.shape
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    g_flow, _ = R.depthflowproj_backward(flow, wgt, count, out, gout)
    step = np.float32(2.0 ** -12)
    checked = 0
    for ch in range(2):
        for h in range(H):
            for w in range(W):
                if R.proj_src(flow[0, 0, h, w], flow[0, 1, h, w], w, h, W, H) is None:
                    assert g_flow[0, ch, h, w] == 0
                    continue
                fp, fm = flow.copy(), flow.copy()
                fp[0, ch, h, w] += step
                fm[0, ch, h, w] -= step
                if R.proj_src(fp[0, 0, h, w], fp[0, 1, h, w], w, h, W, H) is None or R.proj_src(fm[0, 0, h, w], fm[0, 1, h, w], w, h, W, H) is None:
                    continue
                op, _ = R.depthflowproj_forward(fp, wgt, 0)
                om, _ = R.depthflowproj_forward(fm, wgt, 0)
                num = float((gout * (op - om)).sum() / (2.0 * float(step)))
                assert abs(num - g_flow[0, ch, h, w]) <= 1e-9 * max(1.0, abs(num)), (ch, h, w, num, g_flow[0, ch, h, w])
                checked += 1
    assert checked >= 30


def test_proj_g_w_is_the_formula_as_written():
    # single source: out = -f on its targets and count = w, so the .cu's sum is -sum_t sum_xy g_t / w (f - (-f))
    #              = -2 (fx sum_t g_x,t + fy sum_t g_y,t) / w  -- NOT the derivative of -sum(w f) / sum(w), which is 0 here
    fx, fy, wv = 1.25, 0.5, 0.75
    flow, wgt = _single_source(6, 8, 2, 3, fx, fy, wv)
    gout = np.random.default_rng(6).standard_normal((1, 2, 6, 8)).astype(np.float32)
    out, count = R.depthflowproj_forward(flow, wgt, 0)
    g_flow, g_w = R.depthflowproj_backward(flow, wgt, count, out, gout)
    t = [(2, 4), (2, 5), (3, 4), (3, 5)]
    sx = sum(float(gout[0, 0, a, b]) for a, b in t)
    sy = sum(float(gout[0, 1, a, b]) for a, b in t)
    want = -2.0 * (fx * sx + fy * sy) / wv
    assert abs(g_w[0, 0, 2, 3] - want) <= 1e-12 * abs(want)
    assert np.count_nonzero(g_w) == 1
    assert abs(g_flow[0, 0, 2, 3] - (-sx)) <= 1e-12 * abs(sx) and abs(g_flow[0, 1, 2, 3] - (-sy)) <= 1e-12 * abs(sy)      # -sum g w / w


def test_fp32_mode_is_close_and_decides_identically():
    inp, flow, filt, gout = _warp_case(7)
    o64, o32 = R.filterinterp_forward(inp, flow, filt), R.filterinterp_forward(inp, flow, filt, np.float32)
    assert o32.dtype == np.float32 and np.abs(o32 - o64).max() <= 1e-5 * np.abs(o64).max()
    for a, b in zip(R.filterinterp_backward(inp, flow, filt, gout), R.filterinterp_backward(inp, flow, filt, gout, np.float32)):
        assert b.dtype == np.float32 and np.abs(b - a).max() <= 1e-5 * np.abs(a).max() and np.array_equal(a == 0, b == 0)
    fl, wgt, g = _proj_case(8, B=2)
    (p64, c64), (p32, c32) = R.depthflowproj_forward(fl, wgt, 1), R.depthflowproj_forward(fl, wgt, 1, np.float32)
    assert np.array_equal(c64 > 0, c32 > 0) and np.abs(p32 - p64).max() <= 1e-5 * np.abs(p64).max()
