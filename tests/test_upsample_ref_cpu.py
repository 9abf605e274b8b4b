"""CPU: the float64 restatement of the bilinear x2 op (tests/upsample_ref.py) and its transcription of the adjoint's form gate.

The GPU suite (tests/test_upsample_forms_gpu.py) holds every kernel of csrc/upsample.hip to this reference inside bounds that are derived,
not measured: 16 roundings of the sum of magnitudes for the adjoint, 8 for the forward.  Here the reference is held to ATen's float32 CPU
kernels inside the same bounds, to its own transpose and slices, to hip_ops.upsample_window_sources and -- the gate -- to the library's
savfi_upsample2x_bwd_form on a grid across every threshold; and three wrong adjoints are shown to MISS the bound, so that the bound is
known to be able to fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from meta_interpolation_amd import _hip, hip_ops
from tests import upsample_ref as R

SHAPES = [(7, 5, 9), (3, 1, 1), (4, 33, 17), (5, 41, 70)]                 # planes, H, W
# H, W, crop rows, crop columns, window (oy0, ox0, Hw, Ww): the full op, an inner window, one clipped at the right / bottom border
WINDOWS = [(12, 16, (0, 12), (0, 16), (0, 0, 24, 32)),
           (24, 32, (3, 20), (5, 30), (9, 13, 28, 40)),
           (45, 83, (2, 43), (6, 76), (7, 15, 75, 136)),
           (17, 19, (0, 9), (10, 19), (0, 23, 15, 15)),
           (45, 83, (4, 45), (13, 83), (11, 29, 79, 137))]


def _case(planes, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    return torch.randn(planes, H, W, generator=g), torch.randn(planes, 2 * H, 2 * W, generator=g)


def _geom(win):
    H, W, (y0, y1), (x0, x1), (oy0, ox0, Hw, Ww) = win
    return (H, W, y0, x0, y1 - y0, x1 - x0, oy0, ox0, Hw, Ww)


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_matches_aten_float32_within_the_bounds(shape, align):
    """F.interpolate and its autograd adjoint on the CPU in float32 against the reference, inside the bounds the kernels are held to.
    Measured on these inputs: ATen reaches at most 3.1 (forward, bound 8) and 3.2 (adjoint, bound 16) units of 2^-24 * abs-sum."""
    planes, H, W = shape
    x, go = _case(*shape)
    geom = R.full_geom(H, W)
    xr = x.unsqueeze(0).clone().requires_grad_()
    out = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=align)
    gin, = torch.autograd.grad(out, xr, go.unsqueeze(0))
    rf = R.bound_ratio(out.detach()[0], R.fwd(x, geom, align), R.fwd_abs(x, geom, align), R.FWD_UNITS)
    rb = R.bound_ratio(gin[0], R.bwd(go, geom, align), R.bwd_abs(go, geom, align), R.BWD_UNITS)
    print("ATen fp32 %s align %d: forward %.2f of %d units, adjoint %.2f of %d units" % (shape, align, rf * R.FWD_UNITS, R.FWD_UNITS,
                                                                                     rb * R.BWD_UNITS, R.BWD_UNITS))
    assert rf <= 1.0 and rb <= 1.0, (rf, rb)


def test_axis_matrix_rows_sum_to_one_and_follow_the_index_rules():
    for n in (1, 2, 5, 41, 70, 256):
        for align in (True, False):
            A = R.axis_matrix(n, align)
            assert A.shape == (2 * n, n) and (A >= 0).all()
            assert np.abs(A.sum(1) - 1).max() <= 2.0 ** -23                 # l0 = 1 - l1 in float32: the pair sums to 1 within a rounding
            assert (np.count_nonzero(A, 1) <= 2).all()
            i0, i1, l0, l1 = R.axis_sources(n, align)
            assert l0.dtype == np.float32 and (i1 - i0 <= 1).all() and (np.diff(i0) >= 0).all() and i1.max() == n - 1
    # align_corners maps the ends onto the ends; half-pixel centres clamp at the first sample
    assert R.axis_matrix(5, True)[0, 0] == 1 and R.axis_matrix(5, True)[9, 4] == 1
    assert R.axis_matrix(5, False)[0, 0] == 1 and R.axis_matrix(5, False)[1, 0] == 0.75 and R.axis_matrix(5, False)[1, 1] == 0.25
    assert (R.axis_matrix(1, True) == 1).all() and (R.axis_matrix(1, False) == 1).all()


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("win", WINDOWS)
def test_adjoint_is_the_transpose_and_a_window_is_a_slice(win, align):
    """<fwd(x), g> == <x, bwd(g)> to 1e-12 of the sum of magnitudes; the windowed forward is the window of the full forward, and the
    windowed adjoint the crop of the full adjoint of a cotangent that is zero outside the window (nothing of it lands outside the
    crop).  Slices agree to 1e-14 of the element's sum of magnitudes: the same <= 2 x 2 (<= 6 x 6) non-zero float64 products, summed by
    matrix products of other sizes."""
    H, W, (y0, y1), (x0, x1), (oy0, ox0, Hw, Ww) = win
    geom = _geom(win)
    x, gfull = _case(3, H, W, seed=1)
    crop = x[:, y0:y1, x0:x1].contiguous()
    g = gfull[:, oy0:oy0 + Hw, ox0:ox0 + Ww].contiguous()
    out, gin = R.fwd(crop, geom, align), R.bwd(g, geom, align)
    lhs, rhs = (out * g.double()).sum().item(), (crop.double() * gin).sum().item()
    scale = (R.fwd_abs(crop, geom, align) * g.double().abs()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
    full = R.full_geom(H, W)
    want = R.fwd(x, full, align)[:, oy0:oy0 + Hw, ox0:ox0 + Ww]
    assert ((out - want).abs() <= 1e-14 * R.fwd_abs(crop, geom, align)).all()
    gz = torch.zeros_like(gfull)
    gz[:, oy0:oy0 + Hw, ox0:ox0 + Ww] = g
    gx = R.bwd(gz, full, align)
    assert ((gin - gx[:, y0:y1, x0:x1]).abs() <= 1e-14 * R.bwd_abs(g, geom, align)).all()
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[y0:y1, x0:x1] = False
    assert float(gx[:, outside].abs().sum()) == 0


def test_touched_range_equals_the_ops_window_sources():
    """The source range a run of outputs reads, from the reference's index arrays, is what hip_ops.upsample_window_sources hands the
    product (which sizes SepConv's crops with it): every run of every length at the small sizes, a seeded sample at the large ones."""
    rnd = np.random.RandomState(3)
    for n in (1, 2, 3, 5, 9, 17, 41, 45, 70, 83, 256, 448):
        for align in (True, False):
            if n <= 17:
                runs = [(a, b) for a in range(2 * n) for b in range(a + 1, 2 * n + 1)]
            else:
                runs = [tuple(sorted(rnd.choice(2 * n + 1, 2, replace=False))) for _ in range(300)] + [(0, 2 * n), (0, 1), (2 * n - 1, 2 * n)]
            for a, b in runs:
                assert R.touched(int(a), int(b), n, align) == hip_ops.upsample_window_sources(int(a), int(b), n, align), (n, align, a, b)


def _planes_around(Hs, Ws, usr):
    """the plane counts on either side of the gate at strip height `usr` (the last below, the first at or above it)"""
    per_plane = R.cdiv(Ws, R.USW) * R.cdiv(Hs, usr)
    first = R.cdiv(R.STRIP_GATE, per_plane)
    return [first - 1, first]


def test_form_gate_transcription_matches_the_library():
    """R.bwd_form against savfi_upsample2x_bwd_form (host only: no device is touched) across every threshold of the gate: Ws 31 / 32
    (per pixel / tiled), 64 / 65 and 128 / 129 (one more column strip), products 8191 / 8192 exactly and the plane counts either side of
    the gate for each strip height, planes 1 and 65535, and the refusals."""
    lib = _hip.lib()
    cases = set()
    widths = (1, 31, 32, 33, 63, 64, 65, 70, 127, 128, 129, 130, 256, 448)
    heights = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 41, 64, 65, 256)
    for Ws in widths:
        for Hs in heights:
            for planes in (1, 2, 51, 680, 700, 1400, 2048, 4096, 8191, 8192, 8193, 65535):
                cases.add((planes, Hs, Ws))
            if Ws >= 32:
                for usr in (32, 16, 8):
                    cases.update((p, Hs, Ws) for p in _planes_around(Hs, Ws, usr) if p > 0)
    # products of exactly 8191 and 8192 strips at each height: one column strip, 1 x planes strips
    for usr in (32, 16, 8):
        for Hs in (1, usr):
            cases.update({(8191, Hs, 64), (8192, Hs, 64), (8191, Hs, 32), (8192, Hs, 32)})
        cases.update({(4096, usr + 1, 64), (4095, usr + 1, 64), (4096, 2 * usr, 65 if usr == 32 else 64), (2048, 2 * usr, 65), (2047, 2 * usr, 65),
                      (2048, 2 * usr + 1, 65), (1, 8192 * usr, 64), (1, 8191 * usr, 64), (1, 8191 * usr + 1, 64)})
    seen = {}
    for planes, Hs, Ws in sorted(cases):
        got = lib.savfi_upsample2x_bwd_form(planes, Hs, Ws)
        assert got == R.bwd_form(planes, Hs, Ws), (planes, Hs, Ws, got)
        assert got in (0, 1, 8, 16, 32) and (got == 0) == (Ws < 32)
        seen[got] = seen.get(got, 0) + 1
    assert all(seen.get(f, 0) >= 20 for f in (0, 1, 8, 16, 32)), seen
    # the thresholds, spelled out
    form = lib.savfi_upsample2x_bwd_form
    assert form(65535, 64, 31) == 0 and form(65535, 64, 32) == 32 and form(1, 1, 32) == 1
    assert (form(8191, 1, 64), form(8192, 1, 64)) == (1, 32)                      # 8191 / 8192 strips, one row: every height gives the same count
    assert (form(8191, 32, 64), form(8192, 32, 64)) == (16, 32)                   # 8191 strips at USR 32, twice as many at 16
    # 8191 is prime: a product of 8191 strips is 8191 planes of one strip (above) or one plane of 8191 strips
    assert (form(1, 8191 * 32, 64), form(1, 8191 * 32 + 1, 64)) == (16, 32)       # 8191 / 8192 strips of 32 rows
    assert (form(1, 8191 * 16, 64), form(1, 8191 * 16 + 1, 64)) == (8, 16)        # ... of 16 rows (4096 of 32)
    assert (form(1, 8191 * 8, 64), form(1, 8191 * 8 + 1, 64)) == (1, 8)           # ... of 8 rows
    assert (form(4096, 32, 64), form(4096, 32, 65)) == (16, 32)                   # 64 / 65: a second column strip, 4096 -> 8192 strips of 32 rows
    assert (form(2731, 32, 128), form(2731, 32, 129)) == (16, 32)                 # 128 / 129: a third, 5462 -> 8193
    assert (form(680, 41, 70), form(700, 41, 70), form(1400, 41, 70), form(2048, 41, 70)) == (1, 8, 16, 32)     # the GPU suite's family A
    for bad in ((0, 8, 64), (-1, 8, 64), (4, 0, 64), (4, 8, 0), (4, -3, 64), (4, 8, -64), (0, 0, 0)):
        assert form(*bad) == R.E_SHAPE == R.bwd_form(*bad), bad


def test_the_adjoint_bound_can_fail():
    """Three wrong adjoints at (41, 70), align_corners, all of which must MISS 16 * 2^-24 * abs-sum:
      a) the reference with float64 source coordinates (the weights move by up to 5e-6: the bound tells ATen's float32 definition from it);
      b) source row 32 -- the first row of the second strip at USR 32 -- loses output row 63, the one of its candidates that the
         first strip's walk also reads, with the smallest weight of the four (0.11);
      c) at the last column, i1's weight lands on i0.
    And the true adjoint evaluated in float32 (ATen) passes: test_reference_matches_aten_float32_within_the_bounds."""
    H, W, align = 41, 70, True
    geom = R.full_geom(H, W)
    _, g = _case(4, H, W, seed=2)
    ref, mag = R.bwd(g, geom, align), R.bwd_abs(g, geom, align)
    assert R.bound_ratio(ref.float(), ref, mag, R.BWD_UNITS) <= 1.0 / R.BWD_UNITS          # its own float32 rounding: half a unit

    a = R.bwd(g, geom, align, coord=np.float64)
    ra = R.bound_ratio(a, ref, mag, R.BWD_UNITS)

    Ay, Ax = R.window_matrices(geom, align)
    onto32 = torch.nonzero(Ay[:, 32]).view(-1).tolist()
    assert onto32 == [63, 64, 65, 66] and Ay[63, 32] == Ay[onto32, 32].min() and 0.1 < Ay[63, 32] < 0.12
    Ayb = Ay.clone()
    Ayb[63, 32] = 0
    b = R.apply(g, Ayb.t().contiguous(), Ax.t().contiguous())
    rb = R.bound_ratio(b, ref, mag, R.BWD_UNITS)
    assert torch.equal(b[:, :32], ref[:, :32]) and torch.equal(b[:, 33:], ref[:, 33:])       # only that row is wrong

    i0, i1, _, l1 = R.axis_sources(W, align)
    Axc = Ax.clone()
    moved = 0
    for o in range(2 * W):
        if i1[o] == W - 1 and i0[o] == W - 2:
            Axc[o, W - 2] += Axc[o, W - 1]
            Axc[o, W - 1] = 0
            moved += 1
    assert moved >= 1
    c = R.apply(g, Ay.t().contiguous(), Axc.t().contiguous())
    rc = R.bound_ratio(c, ref, mag, R.BWD_UNITS)
    assert torch.equal(c[:, :, :W - 2], ref[:, :, :W - 2])
    print("error / bound of the wrong adjoints: float64 coordinates %.1f, dropped row %.3g, misplaced weight %.3g" % (ra, rb, rc))
    assert ra > 1.0 and rb > 1.0 and rc > 1.0, (ra, rb, rc)
