"""The instrument of tests/nonfinite_ref.py on the CPU: torch float32 stands in for a kernel and passes hold() against float64; stand-ins
that drop a NaN, that spread it across samples, that answer wrongly where they are finite or that change an infinity's sign are caught;
the share cap fires."""
import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_ref as NF
from tests.nonfinite_ref import NAN, NINF, PINF

ULP = 2.0 ** -24
WHERE = [(1, 5, 6), (0, 0, 0), (2, 8, 10)]          # interior, a corner, the last row and column
VALUES = [NAN, PINF, NINF]


def _inputs(seed=0, N=3, C=3, H=9, W=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    return x, NF.plant(x, WHERE, VALUES)


def _conv_case(seed=0):
    x, xp = _inputs(seed)
    g = torch.Generator().manual_seed(seed + 100)
    w, b = torch.randn(5, 3, 3, 3, generator=g) / 5, torch.randn(5, generator=g)
    z64 = lambda t: F.conv2d(t.double(), w.double(), b.double(), padding=1)
    tol = 8 * ULP * F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)     # the clean magnitude
    return x, xp, w, b, z64, tol


def test_plant_writes_sample_zero_only_and_copies():
    x, xp = _inputs()
    assert torch.isfinite(x).all() and NF.bits_equal(xp[1:], x[1:])
    assert NF.klass(xp[0])[1, 5, 6] == 1 and NF.klass(xp[0])[0, 0, 0] == 2 and NF.klass(xp[0])[2, 8, 10] == 3
    assert int((~torch.isfinite(xp)).sum()) == 3
    with pytest.raises(AssertionError):
        NF.plant(x, [(0, 0, 0)], [1.0])


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_conv_act_float32_holds(slope):
    x, xp, w, b, z64, tol = _conv_case()
    act = (lambda z: F.leaky_relu(z, slope)) if slope else F.relu
    f32 = lambda t: act(F.conv2d(t, w, b, padding=1))
    n = NF.hold(f32(xp), act(z64(xp)), f32(x), tol=tol, what="conv")
    assert n >= 9 * 5                  # at least the NaN's 3 x 3 neighbourhood in five channels (relu turns a -inf into 0)


def test_pointwise_and_pool_and_bilinear_hold():
    x, xp = _inputs(1, H=10, W=12)
    for name, f in (("leaky", lambda t: F.leaky_relu(t, 0.2)), ("relu", F.relu)):
        NF.hold(f(xp), f(xp.double()), f(x), same_class=True, tol=ULP * x.abs().double(), what=name)      # 0.2 is rounded in float32
    NF.hold(F.avg_pool2d(xp, 2), F.avg_pool2d(xp.double(), 2), F.avg_pool2d(x, 2), tol=2 * ULP * F.avg_pool2d(x.double().abs(), 2), what="pool")
    for align in (False, True):
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=align)
        NF.hold(up(xp), up(xp.double()), up(x), tol=32 * ULP * float(x.abs().max()), what="bilinear %s" % align)       # fp32 source coordinates: index x 2^-24


def test_losses_and_plane_mean_hold():
    x, xp = _inputs(2)
    y = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    for kind, f in (("l1", lambda a, b: (a - b).abs().mean((1, 2, 3))), ("mse", lambda a, b: (a - b).pow(2).mean((1, 2, 3)))):
        NF.hold(f(xp, y), f(xp.double(), y.double()), f(x, y), tol=1e-5, what=kind)
    mean = lambda t: t.mean((2, 3))
    NF.hold(mean(xp), mean(xp.double()), mean(x), tol=1e-6, what="plane mean")


def test_a_stand_in_that_drops_nan_fails_A():
    x, xp, w, b, z64, tol = _conv_case()
    drop = lambda t: torch.fmax(F.conv2d(t, w, b, padding=1), torch.zeros(()))             # fmaxf(NaN, 0) = 0
    with pytest.raises(AssertionError, match=r"\(A\)"):
        NF.hold(drop(xp), F.relu(z64(xp)), drop(x), tol=tol, what="fmax")


def test_a_stand_in_that_spreads_across_samples_fails_C():
    x, xp, w, b, z64, tol = _conv_case()
    f32 = lambda t: F.relu(F.conv2d(t, w, b, padding=1))
    spread = lambda t: f32(t) + 0 * f32(t).sum()                                           # a batch-wide reduction leaks the NaN
    with pytest.raises(AssertionError, match=r"\(C\)"):
        NF.hold(spread(xp), F.relu(z64(xp)), spread(x), tol=tol, what="spread")
    leak = f32(xp)
    leak[1, 0, 0, 0] = torch.nextafter(leak[1, 0, 0, 0], torch.tensor(9.0))                # one ulp in a control sample
    with pytest.raises(AssertionError, match=r"\(C\).*clean bits"):
        NF.hold(leak, F.relu(z64(xp)), f32(x), tol=tol, what="leak")


def test_spread_inside_the_sample_needs_a_footprint():
    x, xp, w, b, z64, tol = _conv_case()
    f32 = lambda t: F.relu(F.conv2d(t, w, b, padding=1))
    got = f32(xp)
    got[0, :, 4:8, 4:8] = NAN                                                              # the whole tile of the planted pixel (5, 6) turns NaN
    with pytest.raises(AssertionError, match=r"\(C\)"):
        NF.hold(got, F.relu(z64(xp)), f32(x), tol=tol, what="no footprint")
    fp = NF.wino_footprint((5, 9, 11), [(5, 6), (0, 0), (8, 10)], 4, 1)
    assert fp[:, 4:8, 4:8].all() and not fp[:, 0:4, 4:8].any()
    NF.hold(got, F.relu(z64(xp)), f32(x), footprint=fp, tol=tol, what="footprint")
    with pytest.raises(AssertionError, match=r"\(C\)"):                                     # ... but not in a control sample
        got[1, 0, 0, 0] = NAN
        NF.hold(got, F.relu(z64(xp)), f32(x), footprint=fp, tol=tol, what="control")


def test_finite_and_wrong_fails_B_and_class_is_held():
    x, xp, w, b, z64, tol = _conv_case()
    f32 = lambda t: F.relu(F.conv2d(t, w, b, padding=1))
    got = f32(xp)
    got[0, 4, 2, 9] += 1e-3
    with pytest.raises(AssertionError, match=r"\(B\)"):
        NF.hold(got, F.relu(z64(xp)), f32(x), tol=tol, what="wrong")
    neg = lambda t: -(-t)
    NF.hold(neg(xp), xp.double(), x, same_class=True, what="copy")
    with pytest.raises(AssertionError, match="changed class"):
        NF.hold(xp.abs(), xp.double(), x.abs(), same_class=True, tol=1e30, what="abs")     # -inf came out +inf
    with pytest.raises(AssertionError, match="checks nothing"):
        NF.hold(x, x.double(), x, what="nothing planted")


def test_the_share_cap_fires():
    x, xp, w, b, z64, tol = _conv_case()
    f32 = lambda t: F.relu(F.conv2d(t, w, b, padding=1))
    fp = torch.zeros(5, 9, 11, dtype=torch.bool)
    fp[:, :5] = True                                                                        # 5 of 9 rows: 56%
    with pytest.raises(AssertionError, match="footprint covers"):
        NF.hold(f32(xp), F.relu(z64(xp)), f32(x), footprint=fp, tol=tol, what="share")
    fp[:, 4] = False                                                                        # 4 of 9 rows
    NF.hold(f32(xp), F.relu(z64(xp)), f32(x), footprint=fp, tol=tol, what="share")


def test_wino_footprint_geometry():
    # F(4x4), pad 1: tile t reads input rows 4t - 1 .. 4t + 4; pixel 3 lies in tiles 0 and 1, pixel 5 in tile 1 only
    fp = NF.wino_footprint((1, 12, 12), [(3, 5)], 4, 1)
    assert fp[0, :8, 4:8].all() and int(fp.sum()) == 32
    # the corner shared by four tiles
    assert int(NF.wino_footprint((1, 12, 12), [(3, 4)], 4, 1).sum()) == 64
    # F(2x2), pad 0 (data-gradient offset 2): tile t reads 2t - 2 .. 2t + 1; the ragged last tile is clipped to the map
    fp = NF.wino_footprint((2, 5, 5), [(4, 4)], 2, 2)
    assert fp[:, 4:, 4:].all() and not fp[:, :2].any()
