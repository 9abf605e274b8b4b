"""Shared by the bilinear x2 suites: the op of csrc/upsample.hip restated as two interpolation matrices, its windowed forward and adjoint
in float64 with the sums of magnitudes that scale the error bounds, and a transcription of the gate that picks the adjoint's kernel.

The op's DEFINITION is ATen's (UpSample.h, area_pixel_compute_source_index): the source coordinate of an output index is computed in
float32, and index and weights are taken from that float32 number.  axis_matrix does the same in numpy float32 and only then widens the
weights, so what the float64 products below are away from a kernel's result is the kernel's own rounding: a coordinate computed in float64
moves the align_corners weights by up to 5e-6 at W = 70, many times the bounds (tests/test_upsample_ref_cpu.py shows that such a
reference misses them).

geom = (H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww) as in hip_ops._Upsample2x: the source buffer holds rows [sy0, sy0 + Hs) x columns
[sx0, sx0 + Ws) of a virtual [H, W] map, the output buffer rows [oy0, oy0 + Hw) x columns [ox0, ox0 + Ww) of its [2H, 2W] result.

tests/test_upsample_ref_cpu.py holds all of this to ATen on the CPU, to hip_ops.upsample_window_sources and to the library's own answer
(savfi_upsample2x_bwd_form); tests/test_upsample_forms_gpu.py holds the kernels to it."""
import numpy as np
import torch

torch.set_num_threads(min(16, torch.get_num_threads()))        # the CPU references: at most 16 threads

E_SHAPE = -2                                       # SAVFI_E_SHAPE (include/savfi_hip.h)
USW, STRIP_GATE = 64, 8192                         # csrc/upsample.hip: columns of a strip, strips the streaming form wants
ULP = 2.0 ** -24                                   # half a unit in the last place of a float32 in [1, 2): one rounding, relative
# An element of the adjoint is two nested fma sums of at most 6 terms each over weights that carry one rounding each: 16 roundings of
# the sum of magnitudes cover it.  An element of the forward is three blends (two horizontal, one vertical) of two products each: 8.
BWD_UNITS, FWD_UNITS = 16, 8


def cdiv(a, b):
    return -(-a // b)


def full_geom(H, W):
    return (H, W, 0, 0, H, W, 0, 0, 2 * H, 2 * W)


def axis_sources(n, align, coord=np.float32):
    """i0, i1 (int64) and l0, l1 (dtype `coord`) of the 2n outputs of one axis of n samples.  coord = float32 is the op; float64 exists
    so that the CPU suite can show that the bounds tell the two apart."""
    f = coord
    dst = np.arange(2 * n).astype(f)
    if align:
        scale = f(n - 1) / f(2 * n - 1) if n > 1 else f(0)
        src = scale * dst
    else:
        src = np.maximum((dst + f(0.5)) * f(0.5) - f(0.5), f(0))
    assert src.dtype == f
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    l1 = src - i0.astype(f)
    l0 = f(1) - l1
    assert l0.dtype == f and l1.dtype == f
    return i0, i1, l0, l1


def axis_matrix(n, align, coord=np.float32):
    """The [2n, n] interpolation matrix of one axis, float64: row o holds l0 at i0 and l1 at i1 (their sum where i1 == i0)."""
    i0, i1, l0, l1 = axis_sources(n, align, coord)
    A = np.zeros((2 * n, n), np.float64)
    rows = np.arange(2 * n)
    np.add.at(A, (rows, i0), l0.astype(np.float64))
    np.add.at(A, (rows, i1), l1.astype(np.float64))
    return A


def touched(o0, o1, n, align):
    """First / last source index the outputs [o0, o1) read: i0 of the first, i1 of the last (an index counts even where its weight is 0)."""
    i0, i1, _, _ = axis_sources(n, align)
    return int(i0[o0]), int(i1[o1 - 1])


def window_matrices(geom, align, coord=np.float32):
    """(Ay [Hw, Hs], Ax [Ww, Ws]) float64 tensors: the window's rows and the crop's columns of the two axis matrices.  The window must
    read nothing outside the crop (the C entry refuses such a geometry)."""
    H, W, sy0, sx0, Hs, Ws, oy0, ox0, Hw, Ww = geom
    out = []
    for n, s0, ns, o0, no in ((H, sy0, Hs, oy0, Hw), (W, sx0, Ws, ox0, Ww)):
        assert 0 <= s0 and s0 + ns <= n and 0 <= o0 and o0 + no <= 2 * n and ns > 0 and no > 0, geom
        lo, hi = touched(o0, o0 + no, n, align)
        assert s0 <= lo and hi < s0 + ns, ("the window reads outside the crop", geom)
        A = axis_matrix(n, align, coord)[o0:o0 + no]
        assert not A[:, :s0].any() and not A[:, s0 + ns:].any()
        out.append(torch.from_numpy(np.ascontiguousarray(A[:, s0:s0 + ns])))
    return out


def apply(t, L, Rt, magnitudes=False, chunk=256):
    """L t Rt^T for every plane of t [planes, rows, cols] in float64, `chunk` planes at a time (the float64 copies of a chunk stay
    small); magnitudes: |L| |t| |Rt|^T, the scale of the rounding error of any evaluation of the same sums."""
    t = t.detach().cpu()
    assert t.dim() == 3 and t.shape[1] == L.shape[1] and t.shape[2] == Rt.shape[1], (t.shape, L.shape, Rt.shape)
    if magnitudes:
        L, Rt = L.abs(), Rt.abs()
    R = Rt.t().contiguous()
    out = torch.empty(t.shape[0], L.shape[0], Rt.shape[0], dtype=torch.float64)
    for p in range(0, t.shape[0], chunk):
        c = t[p:p + chunk].double()
        out[p:p + chunk] = torch.matmul(torch.matmul(L, c.abs() if magnitudes else c), R)
    return out


def fwd(x, geom, align, coord=np.float32):
    """x [planes, Hs, Ws] -> the window [planes, Hw, Ww] = Ay x Ax^T"""
    Ay, Ax = window_matrices(geom, align, coord)
    return apply(x, Ay, Ax)


def fwd_abs(x, geom, align):
    Ay, Ax = window_matrices(geom, align)
    return apply(x, Ay, Ax, magnitudes=True)


def bwd(gout, geom, align, coord=np.float32):
    """gout [planes, Hw, Ww] -> gin [planes, Hs, Ws] = Ay^T g Ax: the adjoint; crop pixels no window output reads get 0"""
    Ay, Ax = window_matrices(geom, align, coord)
    return apply(gout, Ay.t().contiguous(), Ax.t().contiguous())


def bwd_abs(gout, geom, align):
    Ay, Ax = window_matrices(geom, align)
    return apply(gout, Ay.t().contiguous(), Ax.t().contiguous(), magnitudes=True)


def bound_ratio(got, ref, mag, units):
    """max over the elements of |got - ref| / (units * 2^-24 * mag): <= 1 is inside the bound.  Where mag == 0 every term of the element
    is zero and the element must be exactly 0 (inf otherwise).  NaN in `got` gives inf."""
    err = (got.detach().cpu().double() - ref).abs()
    allowed = units * ULP * mag
    ratio = torch.where(allowed > 0, err / allowed.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, np.inf)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, np.inf), ratio)
    return float(ratio.max())


def bwd_form(planes, Hs, Ws):
    """Transcription of bwd_form() of csrc/upsample.hip (default build): 0 = one thread per source pixel, 1 = the tiled kernel, 8 / 16 / 32
    = the streaming kernel with strips of that many source rows -- the first of 32, 16, 8 that yields STRIP_GATE strips of USW columns."""
    if planes <= 0 or Hs <= 0 or Ws <= 0:
        return E_SHAPE
    if Ws < 32:
        return 0
    for usr in (32, 16, 8):
        if cdiv(Ws, USW) * cdiv(Hs, usr) * planes >= STRIP_GATE:
            return usr
    return 1
