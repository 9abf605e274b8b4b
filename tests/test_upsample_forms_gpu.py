"""GPU: every kernel of csrc/upsample.hip -- the forward and the three forms of its adjoint (one thread per source pixel, the LDS-tiled
form, the streaming form at strip heights 32, 16 and 8) -- through the C ABI against the float64 restatement of tests/upsample_ref.py.

The host picks the adjoint's form by work size (savfi_upsample2x_bwd_form); training and evaluation batch sizes land on different forms.
Every adjoint case here names the form it is about and asserts that the library reports it, so a moved gate cannot quietly take a
case to another kernel.  The results lie between canaries and start as NaN: every element must be written, also the crop pixels no
window output reads (they get 0), and nothing beyond.

Bounds (derived in tests/upsample_ref.py, shown to be able to fail in tests/test_upsample_ref_cpu.py), element-wise:
    adjoint  |gin - ref| <= 16 * 2^-24 * (|Ay|^T |g| |Ax|)        forward  |out - ref| <= 8 * 2^-24 * (|Ay| |x| |Ax|^T)
The comments in upsample.hip promise that the three adjoint forms give identical bits: families A and B assert it on the planes that all
four launches share.

Largest error / bound measured on the MI355X (every test prints its own), align_corners 1 / 0; a form with more planes has more elements
to take the maximum over, the planes the forms share came out bit-equal in every case:
    adjoint, streaming 32 rows   A 0.192 / 0.165   B 0.201 / 0.201   edges 0.166 (4096 x 9 x 65), 0.150 (8192 x 1 x 32)
    adjoint, streaming 16 rows   A 0.192 / 0.164   B 0.201 / 0.201   edges 0.177 / 0.171 (1400 x 17 x 130)
    adjoint, streaming 8 rows    A 0.192 / 0.161   B 0.191 / 0.181
    adjoint, tiled               A 0.192 / 0.161   B 0.191 / 0.181   edges 0.125
    adjoint, per pixel                                               edges 0.105
    forward                      0.350 / 0.353 over all windows
Tried once: a library whose streaming kernel finishes every source row before its last two candidate rows (wrong sums, same memory
accesses) fails families A and B and the two streaming edge cases with more than one source row, and passes the rest."""
import numpy as np
import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import upsample_ref as R
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
# planes -> form at Hs, Ws = 41, 70 (two column strips): 2 * 2 * 2048 = 8192 strips of 32 rows; 2 * 3 * 1400 = 8400 of 16 (5600 of 32);
# 2 * 6 * 700 = 8400 of 8 (4200 of 16); 2 * 6 * 680 = 8160: the tiled form
FORMS_41x70 = [(2048, 32), (1400, 16), (700, 8), (680, 1)]
SHARED = 680                                            # planes every launch of a family computes


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _adjoint(gout_dev, planes, geom, align, form, y=None, slope=None):
    """One launch of the (masked) adjoint on the first `planes` planes of gout_dev -> gin on the host.  Asserts the form, the return code,
    the canaries and that no NaN of the prefill is left."""
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    assert gout_dev.is_contiguous() and gout_dev.shape[0] >= planes and tuple(gout_dev.shape[1:]) == (Hw, Ww)
    lib, st = _hip.lib(), _hip.current_stream()
    assert lib.savfi_upsample2x_bwd_form(planes, Hs, Ws) == form == R.bwd_form(planes, Hs, Ws), (planes, Hs, Ws, form)
    G = Guarded()
    gin = G.new("gin", planes, Hs, Ws, fill=NAN)
    if y is None:
        rc = lib.savfi_upsample2x_window_bwd_f32(gout_dev.data_ptr(), gin.data_ptr(), planes, *geom, int(align), st)
    else:
        assert y.is_contiguous() and y.shape[0] >= planes and tuple(y.shape[1:]) == (Hs, Ws)
        rc = lib.savfi_upsample2x_window_bwd_masked_f32(gout_dev.data_ptr(), y.data_ptr(), slope, gin.data_ptr(), planes, *geom, int(align), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    G.check("adjoint form %d %s" % (form, (geom, align)))
    got = gin.cpu()
    assert not torch.isnan(got).any(), "form %d left elements of gin unwritten" % form
    return got


def _forward(x_dev, planes, geom, align):
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    assert x_dev.is_contiguous() and tuple(x_dev.shape) == (planes, Hs, Ws)
    lib, st = _hip.lib(), _hip.current_stream()
    G = Guarded()
    out = G.new("out", planes, Hw, Ww, fill=NAN)
    rc = lib.savfi_upsample2x_window_fwd_f32(x_dev.data_ptr(), out.data_ptr(), planes, *geom, int(align), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    G.check("forward %s" % ((geom, align),))
    got = out.cpu()
    assert not torch.isnan(got).any(), "the forward left elements of the window unwritten"
    return got


def _every_form_of_41x70(gout, geom, align, what):
    """The four launches of a family on the 41 x 70 crop: each against float64 (computed once on all 2048 planes), and the planes they
    share against each other, bit for bit."""
    ref, mag = R.bwd(gout, geom, align), R.bwd_abs(gout, geom, align)
    gd = gout.to(DEV)
    got = {}
    for planes, form in FORMS_41x70:
        got[form] = _adjoint(gd, planes, geom, align, form)
        ratio = R.bound_ratio(got[form], ref[:planes], mag[:planes], R.BWD_UNITS)
        print("upsample adjoint %s align %d form %2d: error / bound %.3f" % (what, align, form, ratio))
        assert ratio <= 1.0, (what, align, form, ratio)
    for form in (16, 8, 1):
        same = _bits_equal(got[form][:SHARED], got[32][:SHARED])
        print("upsample adjoint %s align %d form %2d against form 32 on %d planes: %s" % (what, align, form, SHARED,
                                                                                        "bit-equal" if same else "DIFFERENT"))
        assert same, "%s align %d: forms %d and 32 differ on the planes both compute" % (what, align, form)


_A = {}


def _family_a_gout():
    if "gout" not in _A:
        _A["gout"] = _randn(41 * 70, 2048, 82, 140)
    return _A["gout"]


@pytest.mark.parametrize("align", [True, False])
def test_family_a_full_op_in_every_form(align):
    """H, W = 41, 70 -> 82 x 140: two column strips of 64 + 6 columns; row strips of 32 + 9, 16 + 16 + 9 and 5 x 8 + 1 rows; 2048,
    1400, 700 and 680 planes of one seeded cotangent run the streaming form at 32, 16 and 8 rows and the tiled form."""
    _every_form_of_41x70(_family_a_gout(), R.full_geom(41, 70), align, "A (full 41x70)")


def _outputs_reading(lo, hi, n, align, odd_start=False):
    """The longest run of outputs [o0, o1) of an axis of n samples that reads only the sources [lo, hi], by hip_ops.upsample_window_sources
    (what the product sizes its crops with); odd_start: the first such output with an odd index."""
    o0 = 0
    while hip_ops.upsample_window_sources(o0, o0 + 1, n, align)[0] < lo or (odd_start and o0 % 2 == 0):
        o0 += 1
    o1 = 2 * n
    while hip_ops.upsample_window_sources(o1 - 1, o1, n, align)[1] > hi:
        o1 -= 1
    assert o0 < o1
    return o0, o1


def _window_b(which, align):
    """geom of the two windows of family B on the virtual 45 x 83 map, both with a 41 x 70 crop."""
    H, W = 45, 83
    if which == "inner":          # crop rows [2, 43), columns [6, 76): a row and a column more than the window reads at the top and left
        sy0, sx0 = 2, 6
        oy0, oy1 = _outputs_reading(sy0 + 1, sy0 + 40, H, align)
        ox0, ox1 = _outputs_reading(sx0 + 1, sx0 + 69, W, align, odd_start=True)
    else:                         # crop rows [4, 45), columns [13, 83): the window ends at the map's bottom and right border
        sy0, sx0 = 4, 13
        oy0, oy1 = _outputs_reading(sy0, H - 1, H, align)
        ox0, ox1 = _outputs_reading(sx0, W - 1, W, align)
        assert (oy1, ox1) == (2 * H, 2 * W)
    return (H, W, sy0, sx0, 41, 70, oy0, ox0, oy1 - oy0, ox1 - ox0)


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("which", ["inner", "border"])
def test_family_b_windows_in_every_form(which, align):
    """The same 41 x 70 crop as a window of a virtual 45 x 83 map, the same four plane counts.  `inner`: the crop is strictly larger than
    what the window reads at the top and left (row 2 and column 6 receive nothing and must come back 0) and exactly what it reads at the
    bottom and right; the window starts at an odd column.  `border`: the window is clipped by the map's right and bottom border."""
    geom = _window_b(which, align)
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    ylo, yhi = hip_ops.upsample_window_sources(oy0, oy0 + Hw, H, align)
    xlo, xhi = hip_ops.upsample_window_sources(ox0, ox0 + Ww, W, align)
    if which == "inner":
        assert ylo > sy0 and xlo > sx0 and yhi == sy0 + Hs - 1 and xhi == sx0 + Ws - 1 and ox0 % 2 == 1, (geom, ylo, yhi, xlo, xhi)
    else:
        assert (ylo, yhi, xlo, xhi) == (sy0, H - 1, sx0, W - 1) and oy0 + Hw == 2 * H and ox0 + Ww == 2 * W
    gout = _randn(100 * Hw + Ww, 2048, Hw, Ww)
    _every_form_of_41x70(gout, geom, align, "B (%s window %s)" % (which, geom[6:]))
    if which == "inner":          # spelled out: the crop's first row and column get exact zeros in the form the product runs
        got = _adjoint(gout[:700].to(DEV), 700, geom, align, 8)
        assert float(got[:, 0, :].abs().sum()) == 0 and float(got[:, :, 0].abs().sum()) == 0


EDGES = [  # form, planes, Hs, Ws, align values
    (32, 8192, 1, 32, (True,)),          # H = 1 (scale 0, every output reads row 0); lanes 32 .. 63 of every wave idle
    (32, 4096, 9, 65, (True,)),          # a strip shorter than USR; a second column strip of one column
    (16, 1400, 17, 130, (True, False)),  # three column strips; row strips of 16 + 1 rows
    (1, 5, 9, 32, (True,)),
    (1, 4, 17, 130, (True,)),
    (0, 3, 40, 31, (True,)),
    (0, 2, 5, 1, (True,)),
    (0, 1, 1, 1, (True,)),
]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "form%d-%dx%dx%d" % c[:4])
def test_family_c_edges(case):
    form, planes, Hs, Ws, aligns = case
    geom = R.full_geom(Hs, Ws)
    gout = _randn(1000 * Hs + Ws, planes, 2 * Hs, 2 * Ws)
    gd = gout.to(DEV)
    for align in aligns:
        got = _adjoint(gd, planes, geom, align, form)
        ratio = R.bound_ratio(got, R.bwd(gout, geom, align), R.bwd_abs(gout, geom, align), R.BWD_UNITS)
        print("upsample adjoint C (%d x %d x %d) align %d form %2d: error / bound %.3f" % (planes, Hs, Ws, align, form, ratio))
        assert ratio <= 1.0, (case, align, ratio)


@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("align", [True, False])
def test_masked_adjoint_is_the_plain_one_times_the_derivative_in_every_form(align, slope):
    """savfi_upsample2x_window_bwd_masked_f32 on family A: where(y > 0, plain, slope * plain) of the same form's plain result -- which
    test_family_a_full_op_in_every_form holds to float64 -- bit for bit.  y holds 0.0 and -0.0 (both take the slope) and negatives."""
    geom = R.full_geom(41, 70)
    gd = _family_a_gout().to(DEV)
    y = _randn(5, 2048, 41, 70)
    y.view(-1)[::5] = 0.0
    y.view(-1)[1::5] = -0.0
    assert bool((y < 0).any()) and bool(torch.signbit(y[y == 0]).any()) and not bool(torch.signbit(y[y == 0]).all())
    yd = y.to(DEV)
    s32 = float(np.float32(slope))                       # what the C entry receives
    for planes, form in FORMS_41x70:
        plain = _adjoint(gd, planes, geom, align, form)
        masked = _adjoint(gd, planes, geom, align, form, y=yd, slope=s32)
        want = torch.where(y[:planes] > 0, plain, torch.tensor(s32, dtype=torch.float32) * plain)
        assert _bits_equal(masked, want), "form %d slope %g" % (form, slope)
        assert not _bits_equal(masked, plain)


FWD_MAP = (45, 83)


def _fwd_window(oy0, Hw, ox0, Ww, align):
    """a window of the virtual 45 x 83 map with exactly the crop it reads"""
    H, W = FWD_MAP
    ylo, yhi = hip_ops.upsample_window_sources(oy0, oy0 + Hw, H, align)
    xlo, xhi = hip_ops.upsample_window_sources(ox0, ox0 + Ww, W, align)
    return (H, W, ylo, xlo, yhi - ylo + 1, xhi - xlo + 1, oy0, ox0, Hw, Ww)


def _fwd_cases():
    cases = [("A", lambda align: R.full_geom(41, 70)), ("B-inner", lambda align: _window_b("inner", align)),
             ("B-border", lambda align: _window_b("border", align))]
    # rows of 4k, 4k + 1 and 4k + 3 floats from an even and an odd column: with the buffer 256-byte aligned a row of 4k floats keeps every
    # group of four on 16 bytes; 4k + 1 and 4k + 3 walk the rows through 16-byte, 8-byte and 4-byte alignment, and the last group is partial
    for Ww in (64, 65, 67, 132):
        for ox0 in (12, 13):
            cases.append(("Ww%d-ox%d" % (Ww, ox0), lambda align, Ww=Ww, ox0=ox0: _fwd_window(5, 70, ox0, Ww, align)))
    return cases


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("name,make", _fwd_cases(), ids=[c[0] for c in _fwd_cases()])
def test_forward_windows_match_float64(name, make, align):
    """savfi_upsample2x_window_fwd_f32 on 5 planes: families A and B (two tile rows, two tile columns) and windows whose row length
    takes the store through its 16-byte, 8-byte and scalar paths, against float64 inside 8 * 2^-24 * abs-sum."""
    geom = make(align)
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    x = _randn(10 * Hw + Ww, 5, Hs, Ws)
    got = _forward(x.to(DEV), 5, geom, align)
    ratio = R.bound_ratio(got, R.fwd(x, geom, align), R.fwd_abs(x, geom, align), R.FWD_UNITS)
    print("upsample forward %s align %d %s: error / bound %.3f" % (name, align, geom, ratio))
    assert ratio <= 1.0, (name, align, ratio)


@pytest.mark.parametrize("windowed", [False, True])
def test_second_order_of_the_adjoint_is_the_forward(windowed):
    """The op is linear: the gradient of hip_ops' adjoint with respect to its cotangent, contracted with v, is the forward of v -- the
    same launch, so the same bits."""
    if windowed:
        full, origin, win = (20, 27), (3, 4), (9, 11, 24, 31)
        up = lambda t: hip_ops.upsample_bilinear2x_window(t, full, origin, win, True)
        shape = (2, 3, 14, 18)
    else:
        up = lambda t: hip_ops.upsample_bilinear2x(t, True)
        shape = (2, 3, 12, 16)
    x = _randn(1, *shape).to(DEV).requires_grad_()
    v = _randn(2, *shape).to(DEV)
    out = up(x)
    g = _randn(3, *out.shape).to(DEV).requires_grad_()
    gin, = torch.autograd.grad(out, x, g, create_graph=True)
    assert gin.requires_grad
    gg, = torch.autograd.grad(gin, g, v)
    assert _bits_equal(gg, up(v).detach())
    assert float(gg.abs().sum()) > 0
