"""-m gpu: every persistent SepConv kernel in every state of its work partition, against float64.

The K = 51, C = 3 kernels launch one workgroup per CU, and each workgroup walks a piece of the strip-major phase list that the host cuts
for it (csrc/sepconv_x6_shared.h ws_work_range / x6_work_range, csrc/sepconv.hip persistent_work_range).  A piece that crosses into the
next strip -- or the next sample, or in a pair launch the other frame tensor -- starts a new run: a window prologue, reset LDS flags, a
pipeline ramp; inside a run the 64-row window slides and the in-LDS sequence counters keep counting.  Which of these states a launch
reaches depends on the shape AND on the CU count, and on a 256-CU device small shapes reach none of them.  So the cases here are
(shape, cus) pairs: savfi_sepconv_debug_cus makes the launches plan for `cus` CUs (fewer workgroups that take more phases each: an ordinary
launch), and every case first ASSERTS, with the transcription of tests/sepconv_ref.py (held to the library by
tests/test_sepconv_partition_cpu.py), that it reaches the state it is there for -- a change of the partition that moves a case fails
loudly instead of silently testing less.

Per case and kernel, through the C-ABI entry points, into NaN-filled buffers between canaries:
  * forward, gV and gH within 1e-5 of max|ref| of a float64 evaluation of the op and its filter gradients on the fp32 inputs
    (sepconv_ref.sepconv_f64) -- the project's SepConv bound, unchanged;
  * the results at `cus` are torch.equal to the results at the device's own count: nothing in a 16-pixel unit's arithmetic reads the
    partition;
  * savfi_sepconv_ws_errors() == 0, the canaries intact, the planes of an interleaved buffer that a strided call does not own still NaN.

Measured on an MI355X (256 CUs): max error / max|ref| against float64 over all cases of a kernel and both CU counts of each.  Every result
was bit-identical at the two counts.  The gate of 1e-5 is 15 to 40 times what the kernels achieve:
    kernel                      forward    gV         gH
    ws six products             2.30e-07   2.15e-07   2.38e-07
    ws three products           2.52e-07   1.66e-07   1.82e-07
    ws strided six              2.30e-07   2.15e-07   2.38e-07
    ws strided three            2.52e-07   1.66e-07   1.82e-07
    ws unit-major six           1.26e-07   2.15e-07   2.24e-07
    ws unit-major three         1.25e-07   1.53e-07   1.80e-07
    pair six products           2.27e-07   2.61e-07   2.61e-07
    pair three products         2.03e-07   1.80e-07   2.21e-07
    pair unit-major six         1.48e-07   2.01e-07   2.11e-07
    pair unit-major three       1.67e-07   1.69e-07   1.84e-07
    x6                          1.81e-07   2.77e-07   2.64e-07
    fp32 persistent gV only     -          6.43e-07   -
    fp32 persistent gH only     -          -          6.37e-07

The chunk loop of the contiguous entry points (a batch beyond the span of one buffer descriptor runs in chunks of consecutive samples;
test_batch_chunks_equal_the_samples_one_by_one, B = 3, chunks of 2 + 1 and 1 + 1 + 1: bit-identical to the samples one by one), and the
direct kernels the same calls run when not even one sample fits the span:
    ws 10x36, chunked           8.15e-08   1.89e-07   1.51e-07        direct    2.12e-07   2.06e-07   2.25e-07
    x6 10x35, chunked           1.34e-07   1.69e-07   1.80e-07        direct    1.68e-07   2.15e-07   2.33e-07
    fp32 5x70, chunked          -          4.13e-07   3.76e-07        direct    -          1.95e-07   2.29e-07
"""
import ctypes
import functools
import math

import pytest
import torch

from meta_interpolation_amd import _hip
from meta_interpolation_amd.sepconv.sepconv_op import sepconv as S
from tests import sepconv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = R.K
TOL = 1e-5                                        # of max|ref|: the bound of tests/test_hip_ops_gpu.py and tests/test_sepconv_frames8_gpu.py
PAD, CANARY = 4096, 7777.0
ERRORS = {}                                       # kernel -> [forward, gV, gH] maxima over the cases run so far


# ---- the cases: (B, Ho, Wo, cus) and what the partition makes of them (asserted on sepconv_ref.describe) --------------------------------
WS_CASES = [
    # one workgroup, 9 runs of 33 phases across both sample boundaries; ragged last phase (130 % 4) and ragged last strip (68 % 32)
    ((3, 130, 68, 1), dict(grid=1, runs_per_wg=[9], run_lengths=[33], sample_crossings=2, ragged_rows=2, ragged_strip=4)),
    # up to 3 runs per workgroup, pieces that start and end inside a strip
    ((3, 130, 68, 5), dict(grid=5, runs_per_wg=[2, 3, 3, 3, 2], starts_mid_strip=4, ends_mid_strip=4, sample_crossings=2)),
    # 4 runs in a workgroup, Ho % 4 = 3
    ((2, 67, 100, 3), dict(grid=3, runs_per_wg=[3, 4, 3], ragged_rows=3, starts_mid_strip=2, sample_crossings=1)),
    # runs of 65 phases: longer than any product run, every window slot rewritten four times
    ((1, 258, 36, 1), dict(grid=1, runs_per_wg=[2], run_lengths=[65], ragged_rows=2, ragged_strip=4)),
    # per workgroup exactly what (32, 256, 448) reaches on 256 CUs (config c4b32): 113 phases, 3 runs, 64-phase runs; unit-major capable
    ((2, 256, 448, 16), dict(grid=16, max_phases=113, max_runs=3, longest_run=64, starts_mid_strip=12)),
    # 3 runs of at most 2 phases, one 4-pixel column
    ((5, 6, 4, 2), dict(grid=2, runs_per_wg=[3, 3], run_lengths=[1, 2], sample_crossings=4, ragged_strip=4)),
    # fewer rows than a phase
    ((1, 3, 4, 1), dict(grid=1, total=1, ragged_rows=3)),
    # unit-major capable (Wo % 16 == 0): 2 runs per workgroup over both sample boundaries, pieces inside strips
    ((3, 130, 64, 5), dict(grid=5, runs_per_wg=[2, 2, 2, 2, 2], starts_mid_strip=4, sample_crossings=2, ragged_strip=0)),
    ((2, 67, 48, 1), dict(grid=1, runs_per_wg=[4], run_lengths=[17], sample_crossings=1, ragged_rows=3, ragged_strip=16)),
]
# the pair launches: B' = 2 B virtual samples 2 b + f, frame f of sample b; a stretch that crosses from virtual sample a to a + 1 switches
# between `in0` and `in1` (frame_switches: the parities it goes from and to)
PAIR_CASES = [
    ((2, 67, 100, 3), dict(grid=3, runs_per_wg=[3, 4, 3], frame_switches=[(0, 1)])),
    ((4, 67, 100, 3), dict(grid=3, runs_per_wg=[6, 6, 6], frame_switches=[(0, 1), (1, 0)], sample_crossings=3)),
    ((2, 130, 68, 1), dict(grid=1, runs_per_wg=[6], run_lengths=[33], frame_switches=[(0, 1)])),
    ((6, 6, 4, 2), dict(grid=2, runs_per_wg=[3, 3], frame_switches=[(0, 1), (1, 0)], sample_crossings=4)),
    ((4, 130, 64, 5), dict(grid=5, max_runs=3, frame_switches=[(0, 1), (1, 0)], sample_crossings=3, starts_mid_strip=4)),   # unit-major too
    ((2, 256, 448, 16), dict(grid=16, max_phases=113, max_runs=3, longest_run=64)),                                       # unit-major too
]
# one program per wave: the widths that are no multiple of 4
X6_CASES = [
    ((3, 130, 70, 1), dict(grid=1, runs_per_wg=[9], run_lengths=[33], sample_crossings=2, ragged_rows=2, ragged_strip=6)),
    ((3, 130, 70, 5), dict(grid=5, runs_per_wg=[2, 3, 3, 3, 2], starts_mid_strip=4, ends_mid_strip=4, sample_crossings=2)),
    ((2, 67, 101, 3), dict(grid=3, runs_per_wg=[3, 4, 3], ragged_rows=3, ragged_strip=5, sample_crossings=1)),
    ((1, 258, 41, 1), dict(grid=1, runs_per_wg=[2], run_lengths=[65], ragged_strip=9)),
    ((5, 6, 5, 2), dict(grid=2, runs_per_wg=[3, 3], run_lengths=[1, 2], sample_crossings=4)),
    ((1, 3, 5, 1), dict(grid=1, total=1, ragged_rows=3)),
    ((2, 37, 45, 3), dict(grid=3, runs_per_wg=[2, 2, 2], starts_mid_strip=2, ends_mid_strip=2, sample_crossings=1, ragged_rows=1)),
]
# the fp32 kernel of savfi_sepconv_bwd_f32 with only one of gV / gH wanted: phases of 2 rows on strips of 64 columns, any width
FP32_CASES = [
    ((3, 66, 70, 1), dict(grid=1, runs_per_wg=[6], run_lengths=[33], sample_crossings=2, ragged_strip=6)),
    ((3, 130, 68, 5), dict(grid=5, runs_per_wg=[2, 2, 2, 2, 2], longest_run=65, starts_mid_strip=4, ends_mid_strip=4, sample_crossings=2)),
    ((2, 67, 100, 3), dict(grid=3, runs_per_wg=[2, 2, 2], ragged_rows=1, ragged_strip=36, starts_mid_strip=2, sample_crossings=1)),
    ((1, 258, 41, 1), dict(grid=1, runs_per_wg=[1], run_lengths=[129], ragged_strip=41)),
    ((5, 3, 4, 2), dict(grid=2, runs_per_wg=[3, 3], run_lengths=[1, 2], sample_crossings=4, ragged_rows=1)),
    ((1, 1, 4, 1), dict(grid=1, total=1, ragged_rows=1)),
    ((2, 131, 45, 7), dict(grid=7, runs_per_wg=[1, 1, 1, 2, 1, 1, 1], starts_mid_strip=6, sample_crossings=1, ragged_rows=1)),
]


def _ids(cases):
    return ["%dx%dx%d-cus%d" % c[0] for c in cases]


def _assert_reaches(kind, case, claims):
    d = R.describe(kind, *case)
    for key, want in claims.items():
        assert d[key] == want, "case %s no longer reaches what it is there for: %s = %s, expected %s" % (case, key, d[key], want)
    return d


@pytest.fixture(scope="module", autouse=True)
def _summary_of_the_float64_errors():
    """after the module's last test: the maxima over the cases that ran (what the module docstring records)"""
    yield
    for kernel in sorted(ERRORS):
        print("\n[summary] %-26s %s" % (kernel, "  ".join("%s %.3g" % (n, e) for n, e in zip(("forward", "gV", "gH"), ERRORS[kernel]) if e is not None)),
              end="")
    print()


# ---- the CU count the launches plan for ------------------------------------------------------------------------------------------------
def _device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture
def plan_for():
    """plan_for(cus): the persistent launches plan for `cus` CUs from now on (0: the device's own count); restored when the test ends"""
    lib = _hip.lib()
    try:
        yield lambda cus: _hip.check(lib.savfi_sepconv_debug_cus(int(cus), None), "savfi_sepconv_debug_cus")
    finally:
        lib.savfi_sepconv_debug_cus(0, None)


def _planned_grid(kind, B, Ho, Wo):
    g0, g1 = ctypes.c_int(), ctypes.c_int()
    return _hip.lib().savfi_sepconv_partition(kind, B, Ho, Wo, 0, 0, ctypes.byref(g0), ctypes.byref(g1))


# ---- inputs and their float64 reference -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _problem(B, Ho, Wo):
    """Two frame tensors of 8-bit images (k / 255: they qualify for the three-product kernels, and the six-product kernels take them like
    any other floats), an interleaved tap tensor [4 B][K][Ho][Wo] (sample 4 b + s = sub-network s: v0, h0, v1, h1) and a cotangent.
    The single-frame cases use frame 0 with sub-networks 0 / 1."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * Ho + Wo)
    f0 = torch.randint(0, 256, (B, 3, Ho + K - 1, Wo + K - 1), generator=g).float().div(255)
    f1 = torch.randint(0, 256, (B, 3, Ho + K - 1, Wo + K - 1), generator=g).float().div(255)
    taps = torch.randn(4 * B, K, Ho, Wo, generator=g) / math.sqrt(K)
    gO = torch.randn(B, 3, Ho, Wo, generator=g)
    return f0, f1, taps, gO


@functools.lru_cache(maxsize=4)
def _reference(B, Ho, Wo, f):
    """(out, gV, gH) in float64 of frame f with sub-networks 2 f / 2 f + 1"""
    f0, f1, taps, gO = _problem(B, Ho, Wo)
    t5 = taps.view(B, 4, K, Ho, Wo)
    return R.sepconv_f64((f0, f1)[f], t5[:, 2 * f], t5[:, 2 * f + 1], gO)


def _err(x, ref):
    return (x.detach().cpu().double() - ref).abs().max().item() / ref.abs().max().item()


def _record(kernel, case, cus, triple, refs):
    """print the float64 errors of one launch (forward, gV, gH; None = not computed by this kernel) and hold them to the bound"""
    errs = [None if x is None else _err(x, r) for x, r in zip(triple, refs)]
    print("%-22s B=%d Ho=%d Wo=%d planned cus=%-3d  max error / max|ref| against float64: %s"
          % ((kernel,) + tuple(case[:3]) + (cus, "  ".join("%s %.3g" % (n, e) for n, e in zip(("forward", "gV", "gH"), errs) if e is not None))))
    acc = ERRORS.setdefault(kernel.split(",")[0], [None, None, None])
    for i, e in enumerate(errs):
        if e is not None:
            acc[i] = max(acc[i] or 0.0, e) if e == e else float("nan")
            assert e < TOL, (kernel, case, cus, ("forward", "gV", "gH")[i], e)


class _Buffers:
    """NaN-filled output tensors between canaries"""

    def __init__(self):
        self.held = []

    def new(self, *shape):
        n = math.prod(shape)
        flat = torch.full((n + 2 * PAD,), CANARY, device=DEV)
        flat[PAD:PAD + n] = float("nan")
        self.held.append((flat, n))
        return flat[PAD:PAD + n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for flat, n in self.held:
            intact = bool(torch.all(flat[:PAD] == CANARY)) and bool(torch.all(flat[PAD + n:] == CANARY))
            assert intact, "a kernel wrote outside its output"
        self.held = []


def _to_unit16(t):
    """[B,K,H,W] values -> a tensor of the same shape whose MEMORY is [B][H][W/16][K][16] (what savfi_conv3x3_tasks_pre_unit16_f32 writes)"""
    B, Kk, H, W = t.shape
    return t.view(B, Kk, H, W // 16, 16).permute(0, 2, 3, 1, 4).contiguous().view(B, Kk, H, W)


def _words(x, forged=False):
    """the classifier words of a frame tensor; forged: non-zero words, with which the device takes the six-product kernel for any frames"""
    w = S.frames8_classify(x)
    torch.cuda.synchronize()
    assert int(w.abs().sum()) == 0, "the frames are k / 255"
    if forged:
        w = w.clone()
        w[S.FRAMES8_WORDS - 1] = 1
    return w


P = lambda t: None if t is None else t.data_ptr()


# ---- the launches -----------------------------------------------------------------------------------------------------------------------
def _single_frame_launches(B, Ho, Wo, ws):
    """every kernel that takes frame 0 with sub-networks 0 / 1: name -> (out, gV, gH) on the device.  ws: the width is a multiple of 4
    (the wave-specialised kernels and their strided / frames8 / unit-major entry points); otherwise one program per wave."""
    lib, st = _hip.lib(), _hip.current_stream()
    f0, _, taps, gO = (t.to(DEV) for t in _problem(B, Ho, Wo))
    t5 = taps.view(B, 4, K, Ho, Wo)
    v, h = t5[:, 0].contiguous(), t5[:, 1].contiguous()
    plane = K * Ho * Wo * 4
    bufs, res = _Buffers(), {}
    dims = (B, 3, Ho, Wo, K)

    # the contiguous entry points: six products on the wave-specialised kernels (Wo % 4 == 0) or on one program per wave
    out, gV, gH = bufs.new(B, 3, Ho, Wo), bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
    _hip.check(lib.savfi_sepconv_fwd_f32(P(f0), P(v), P(h), P(out), *dims, st), "fwd")
    _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, P(gV), P(gH), *dims, st), "bwd")
    res["ws six products" if ws else "x6"] = (out, gV, gH)
    if not ws:
        bufs.check()
        return res
    assert lib.savfi_sepconv_taps_strided_supported(*dims, 4 * K) == 1

    # three products: the frames with their real classifier words
    w8 = _words(f0)
    out, gV, gH = bufs.new(B, 3, Ho, Wo), bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
    _hip.check(lib.savfi_sepconv_fwd_frames8_f32(P(f0), P(v), P(h), P(out), P(w8), *dims, K, 0, st), "fwd8")
    _hip.check(lib.savfi_sepconv_bwd_frames8_f32(P(f0), P(v), P(h), P(gO), P(gV), P(gH), P(w8), *dims, K, 0, st), "bwd8")
    res["ws three products"] = (out, gV, gH)

    # strided taps: v / h read, gV / gH written in place in the interleaved buffer (tap_bstride = 4 K); sub-networks 2, 3 are not ours
    def strided(name, words):
        out, gt = bufs.new(B, 3, Ho, Wo), bufs.new(4 * B, K, Ho, Wo)
        if words is None:
            _hip.check(lib.savfi_sepconv_fwd_taps_strided_f32(P(f0), P(taps), P(taps) + plane, P(out), *dims, 4 * K, st), name)
            _hip.check(lib.savfi_sepconv_bwd_taps_strided_f32(P(f0), P(taps), P(taps) + plane, P(gO), P(gt), P(gt) + plane, *dims, 4 * K, st), name)
        else:
            _hip.check(lib.savfi_sepconv_fwd_frames8_f32(P(f0), P(taps), P(taps) + plane, P(out), P(words), *dims, 4 * K, 0, st), name)
            _hip.check(lib.savfi_sepconv_bwd_frames8_f32(P(f0), P(taps), P(taps) + plane, P(gO), P(gt), P(gt) + plane, P(words), *dims, 4 * K, 0,
                                                         st), name)
        g5 = gt.view(B, 4, K, Ho, Wo)
        torch.cuda.synchronize()
        untouched = bool(torch.isnan(g5[:, 2:]).all())
        assert untouched, name + ": wrote planes of the interleaved buffer that it does not own"
        res[name] = (out, g5[:, 0], g5[:, 1])
    strided("ws strided six", None)
    strided("ws strided three", w8)

    # unit-major taps (a sample is [Ho][Wo / 16][K][16]); the gradients planar (taps_unit16 = 1) and unit-major as well (3)
    if Wo % 16 == 0:
        vu, hu = _to_unit16(v), _to_unit16(h)
        for name, words in (("ws unit-major three", w8), ("ws unit-major six", _words(f0, forged=True))):
            out, gV, gH = bufs.new(B, 3, Ho, Wo), bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
            gVu, gHu = bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
            _hip.check(lib.savfi_sepconv_fwd_frames8_f32(P(f0), P(vu), P(hu), P(out), P(words), *dims, K, 1, st), name)
            _hip.check(lib.savfi_sepconv_bwd_frames8_f32(P(f0), P(vu), P(hu), P(gO), P(gV), P(gH), P(words), *dims, K, 1, st), name)
            _hip.check(lib.savfi_sepconv_bwd_frames8_f32(P(f0), P(vu), P(hu), P(gO), P(gVu), P(gHu), P(words), *dims, K, 3, st), name)
            torch.cuda.synchronize()
            same = torch.equal(gVu, _to_unit16(gV)) and torch.equal(gHu, _to_unit16(gH))
            assert same, name + ": unit-major gradients differ from planar"
            res[name] = (out, gV, gH)
    bufs.check()
    return res


def _pair_launches(B, Ho, Wo):
    """the pair forward and backward (B samples = 2 B virtual ones): name -> [(out, gV, gH) of frame 0, of frame 1]"""
    lib, st = _hip.lib(), _hip.current_stream()
    f0, f1, taps, gO = (t.to(DEV) for t in _problem(B, Ho, Wo))
    bufs, res = _Buffers(), {}
    variants = [("pair three products", False, 0), ("pair six products", True, 0)]
    if Wo % 16 == 0:
        variants += [("pair unit-major three", False, 1), ("pair unit-major six", True, 1)]
    for name, forged, u16 in variants:
        w0, w1 = _words(f0, forged), _words(f1)           # one forged set is enough: the three-product kernel needs both frames to qualify
        tp = _to_unit16(taps) if u16 else taps
        out, gt = bufs.new(B, 2, 3, Ho, Wo), bufs.new(4 * B, K, Ho, Wo)
        _hip.check(lib.savfi_sepconv_fwd_pair_frames8_f32(P(f0), P(f1), P(tp), P(out), P(w0), P(w1), B, 3, Ho, Wo, K, u16, st), name)
        _hip.check(lib.savfi_sepconv_bwd_pair_frames8_f32(P(f0), P(f1), P(tp), P(gO), P(gt), P(w0), P(w1), B, 3, Ho, Wo, K, u16, st), name)
        if u16:                                           # ... and the gradients unit-major as well
            gu = bufs.new(4 * B, K, Ho, Wo)
            _hip.check(lib.savfi_sepconv_bwd_pair_frames8_f32(P(f0), P(f1), P(tp), P(gO), P(gu), P(w0), P(w1), B, 3, Ho, Wo, K, 3, st), name)
            torch.cuda.synchronize()
            same = torch.equal(gu, _to_unit16(gt))
            assert same, name + ": unit-major gradients differ from planar"
        g5 = gt.view(B, 4, K, Ho, Wo)
        res[name] = [(out[:, f], g5[:, 2 * f], g5[:, 2 * f + 1]) for f in (0, 1)]
    bufs.check()
    return res


def _fp32_launches(B, Ho, Wo):
    """savfi_sepconv_bwd_f32 with only gV, with only gH wanted: name -> (None, gV, gH)"""
    lib, st = _hip.lib(), _hip.current_stream()
    f0, _, taps, gO = (t.to(DEV) for t in _problem(B, Ho, Wo))
    t5 = taps.view(B, 4, K, Ho, Wo)
    v, h = t5[:, 0].contiguous(), t5[:, 1].contiguous()
    bufs = _Buffers()
    gV, gH = bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
    _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, P(gV), None, B, 3, Ho, Wo, K, st), "gV only")
    _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, None, P(gH), B, 3, Ho, Wo, K, st), "gH only")
    bufs.check()
    return {"fp32 persistent gV only": (None, gV, None), "fp32 persistent gH only": (None, None, gH)}


def _both_counts(kind, shape, cus, plan_for, launch):
    """launch() with the launches planning for `cus` CUs and for the device's own count: {planned: results}"""
    assert cus <= _device_cus(), "the device has fewer CUs than the case plans for"
    got = {}
    for planned in (cus, 0):
        plan_for(planned)
        assert _planned_grid(kind, *shape) == R.grid_size(kind, *shape, planned or _device_cus()), "the hook did not take"
        got[planned] = launch()
        if kind == R.WS:
            assert _hip.lib().savfi_sepconv_ws_errors() == 0
    return got


def _assert_same_bits(a, b, what):
    for x, y, n in zip(a, b, ("forward", "gV", "gH")):
        if x is not None:
            same = torch.equal(x, y)
            assert same, "%s: %s depends on the CU count the launch was planned for" % (what, n)


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,claims", WS_CASES, ids=_ids(WS_CASES))
def test_wave_specialised_kernels_across_the_partition(case, claims, plan_for):
    B, Ho, Wo, cus = case
    _assert_reaches(R.WS, case, claims)
    got = _both_counts(R.WS, case[:3], cus, plan_for, lambda: _single_frame_launches(B, Ho, Wo, ws=True))
    ref = _reference(B, Ho, Wo, 0)
    assert set(got[cus]) == set(got[0]) and len(got[cus]) == (6 if Wo % 16 == 0 else 4)
    for name in got[cus]:
        for planned in (cus, 0):
            _record(name, case, planned or _device_cus(), got[planned][name], ref)
        _assert_same_bits(got[cus][name], got[0][name], "%s %s" % (name, case))


@pytest.mark.parametrize("case,claims", PAIR_CASES, ids=_ids(PAIR_CASES))
def test_pair_launches_across_the_partition(case, claims, plan_for):
    B2, Ho, Wo, cus = case                             # the partition sees 2 B virtual samples
    _assert_reaches(R.WS, case, claims)
    B = B2 // 2
    got = _both_counts(R.WS, case[:3], cus, plan_for, lambda: _pair_launches(B, Ho, Wo))
    refs = [_reference(B, Ho, Wo, f) for f in (0, 1)]
    assert set(got[cus]) == set(got[0]) and len(got[cus]) == (4 if Wo % 16 == 0 else 2)
    for name in got[cus]:
        for f in (0, 1):
            for planned in (cus, 0):
                _record("%s, frame %d" % (name, f), case, planned or _device_cus(), got[planned][name][f], refs[f])
            _assert_same_bits(got[cus][name][f], got[0][name][f], "%s %s frame %d" % (name, case, f))


@pytest.mark.parametrize("case,claims", X6_CASES, ids=_ids(X6_CASES))
def test_one_program_per_wave_kernels_across_the_partition(case, claims, plan_for):
    B, Ho, Wo, cus = case
    assert Wo % 4 != 0
    _assert_reaches(R.X6, case, claims)
    got = _both_counts(R.X6, case[:3], cus, plan_for, lambda: _single_frame_launches(B, Ho, Wo, ws=False))
    ref = _reference(B, Ho, Wo, 0)
    for planned in (cus, 0):
        _record("x6", case, planned or _device_cus(), got[planned]["x6"], ref)
    _assert_same_bits(got[cus]["x6"], got[0]["x6"], "x6 %s" % (case,))


@pytest.mark.parametrize("case,claims", FP32_CASES, ids=_ids(FP32_CASES))
def test_fp32_persistent_kernel_across_the_partition(case, claims, plan_for):
    B, Ho, Wo, cus = case
    _assert_reaches(R.FP32, case, claims)
    got = _both_counts(R.FP32, case[:3], cus, plan_for, lambda: _fp32_launches(B, Ho, Wo))
    ref = _reference(B, Ho, Wo, 0)
    for name in got[cus]:
        for planned in (cus, 0):
            _record(name, case, planned or _device_cus(), got[planned][name], ref)
        _assert_same_bits(got[cus][name], got[0][name], "%s %s" % (name, case))


# ---- the chunk loop of the contiguous entry points ---------------------------------------------------------------------------------------
# A batch whose tensors do not fit the span of one buffer descriptor (2^31 bytes) is launched in runs of `chunk` consecutive samples
# (savfi_sepconv_route).  savfi_sepconv_debug_span_bytes shrinks the span -- host state only -- so that B = 3 samples of the smallest
# shapes that are ragged in both directions for each kernel are cut 2 + 1 and 1 + 1 + 1; with the span at one sample's size nothing
# fits and the direct kernels run.  (kernel, B, Ho, Wo, the wants the case calls: 0 forward, 3 gV and gH, 1 gV only, 2 gH only)
CHUNK_CASES = [
    ("ws", R.WS, (3, 10, 36), (0, 3)),                    # phases of 4 rows, strips of 32 columns; the taps are the larger tensor
    ("x6", R.X6, (3, 10, 35), (0, 3)),
    ("fp32", R.FP32, (3, 5, 70), (1, 2)),                 # phases of 2 rows, strips of 64 columns; the input window is the larger tensor
]


@pytest.fixture
def span():
    """span(L): the persistent kernels' tensors must stay below L bytes from now on (0: 2^31); restored when the test ends"""
    lib = _hip.lib()
    try:
        yield lambda L: _hip.check(lib.savfi_sepconv_debug_span_bytes(int(L), None), "savfi_sepconv_debug_span_bytes")
    finally:
        lib.savfi_sepconv_debug_span_bytes(0, None)


def _routes(wants, B, Ho, Wo):
    """{(kernel, chunk)} of the library's route over `wants`"""
    chunk, got = ctypes.c_int(-1), set()
    for want in wants:
        kernel = _hip.lib().savfi_sepconv_route(want, B, 3, Ho, Wo, K, ctypes.byref(chunk))
        got.add((kernel, chunk.value))
    return got


def _contiguous_launches(f0, v, h, gO, wants):
    """savfi_sepconv_fwd_f32 / savfi_sepconv_bwd_f32 for every want of the case: (out, gV, gH), None = not asked for"""
    lib, st = _hip.lib(), _hip.current_stream()
    B, _, Ho, Wo = gO.shape
    dims = (B, 3, Ho, Wo, K)
    bufs = _Buffers()
    out = gV = gH = None
    if 0 in wants:
        out = bufs.new(B, 3, Ho, Wo)
        _hip.check(lib.savfi_sepconv_fwd_f32(P(f0), P(v), P(h), P(out), *dims, st), "fwd")
    if 3 in wants:
        gV, gH = bufs.new(B, K, Ho, Wo), bufs.new(B, K, Ho, Wo)
        _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, P(gV), P(gH), *dims, st), "bwd")
    if 1 in wants:
        gV = bufs.new(B, K, Ho, Wo)
        _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, P(gV), None, *dims, st), "gV only")
    if 2 in wants:
        gH = bufs.new(B, K, Ho, Wo)
        _hip.check(lib.savfi_sepconv_bwd_f32(P(f0), P(v), P(h), P(gO), None, None, P(gH), *dims, st), "gH only")
    bufs.check()
    if lib.savfi_sepconv_ws_errors() != 0:
        raise AssertionError("a bounded wait of the wave-specialised kernels gave up")
    return out, gV, gH


@pytest.mark.parametrize("name,kind,shape,wants", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_batch_chunks_equal_the_samples_one_by_one(name, kind, shape, wants, span):
    B, Ho, Wo = shape
    m = max(K * Ho * Wo * 4, 3 * (Ho + K - 1) * (Wo + K - 1) * 4)          # one sample of the larger of the tap and the window tensor
    f0, _, taps, gO = (t.to(DEV) for t in _problem(B, Ho, Wo))
    t5 = taps.view(B, 4, K, Ho, Wo)
    v, h = t5[:, 0].contiguous(), t5[:, 1].contiguous()
    ref = _reference(B, Ho, Wo, 0)

    span(0)                                               # the samples one by one, nothing cut
    assert _routes(wants, 1, Ho, Wo) == {(kind, 1)} and _routes(wants, B, Ho, Wo) == {(kind, B)}
    singles = [_contiguous_launches(f0[b:b + 1], v[b:b + 1], h[b:b + 1], gO[b:b + 1], wants) for b in range(B)]
    one_by_one = [None if xs[0] is None else torch.cat(xs) for xs in zip(*singles)]

    for L, chunk in ((3 * m, 2), (m + 1, 1)):             # launches of 2 + 1 samples, of 1 + 1 + 1
        span(L)
        assert _routes(wants, B, Ho, Wo) == {(kind, chunk)}, "the span hook did not take"
        got = _contiguous_launches(f0, v, h, gO, wants)
        _record("%s chunks of %d" % (name, chunk), shape, _device_cus(), got, ref)
        _assert_same_bits(one_by_one, got, "%s %s in chunks of %d against its samples one by one" % (name, shape, chunk))

    span(m)                                               # not even one sample fits: the direct kernels
    assert _routes(wants, B, Ho, Wo) == {(_hip.SEPCONV_ROUTE_DIRECT, B)}
    got = _contiguous_launches(f0, v, h, gO, wants)
    _record("%s span of one sample: direct" % name, shape, _device_cus(), got, ref)
