"""The non-finite contract of the kernels and the instrument that holds an op to it: no GPU and no library.

A kernel fed a NaN or an infinity must not hand back a plausible number.  hold() compares the kernel's result on a planted input (`got`)
with float64 torch on the same planted fp32 input (`ref64`) and with the same kernel on the unplanted input (`clean_got`):

  (A) nothing is swallowed: every element that is non-finite in ref64 is non-finite in got (same_class=True: the same of NaN / +inf /
      -inf -- for copies, permutations and point-wise ops whose arithmetic is the reference's);
  (B) finite means right: where got is finite, |got - ref64| <= tol.  `tol` is a number or a tensor of per-element bounds that the case
      computes with the gate of the op's own float64 test from the CLEAN inputs (an infinity must not inflate a scale);
  (C) containment: the control samples / tasks (everything but index 0 of dimension 0: plant() writes to index 0 only) equal clean_got
      bit for bit (`control_tol`: the op's tolerance instead, for the atomic paths only), and inside the planted sample got may be
      non-finite where ref64 is finite only within `footprint`, a boolean mask the case states from the op's geometry.

The direction is fixed: too much NaN is a stated, bounded spread; too little NaN is a failure.  The bound on the spread is the share of
the planted sample a footprint may cover, MAX_SHARE: beyond it (B) would check nothing there, so hold() asserts it."""
import torch

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
MAX_SHARE = 0.5


def plant(t, where, values):
    """a copy of t with values[i] written at t[0][where[i]]: sample 0 / task 0 only, the rest is the control.  `where`: index tuples
    into t[0]; `values`: as many of NAN / PINF / NINF."""
    assert len(where) == len(values) and len(where) > 0
    out = t.clone()
    for idx, v in zip(where, values):
        assert v != v or v in (PINF, NINF), "plant() is for non-finite values: %r" % (v,)
        out[0][tuple(idx)] = v
    return out


def klass(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return torch.isnan(t).to(torch.int8) + 2 * torch.isposinf(t).to(torch.int8) + 3 * torch.isneginf(t).to(torch.int8)


def bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    if a.dtype == torch.float64:
        return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
    return bool(torch.equal(a, b))


def hold(got, ref64, clean_got, footprint=None, same_class=False, tol=0.0, control=True, control_tol=None, reaches=True, what=""):
    """Assert (A), (B) and (C) of the module docstring.  got / ref64 / clean_got: same shape, dimension 0 = samples or tasks, index 0
    the planted one.  `footprint`: None (no spread allowed) or a boolean mask that broadcasts to got[0].  control=False: the op reduces
    over dimension 0 (weight gradients of one task), there is no control.  reaches=False: the planted value is one the op only
    compares with (a stored activation that selects a slope): the reference may be finite everywhere, (B) and (C) still hold.
    Returns the count of non-finite elements of got."""
    got, ref64, clean_got = got.detach().cpu(), ref64.detach().cpu(), clean_got.detach().cpu()
    assert got.shape == ref64.shape == clean_got.shape, (what, got.shape, ref64.shape, clean_got.shape)
    assert ref64.dtype == torch.float64, (what, ref64.dtype)
    assert bool(torch.isfinite(clean_got).all()), "%s: the clean run is not finite" % what
    bad_ref, bad_got = ~torch.isfinite(ref64), ~torch.isfinite(got)
    assert not reaches or bool(bad_ref[0].any()), "%s: the reference is finite: the plant reaches nothing, the case checks nothing" % what

    # (A)
    swallowed = bad_ref & ~bad_got
    assert not bool(swallowed.any()), "%s: (A) %d of %d non-finite elements came out finite, first at %s: %r" % (
        what, int(swallowed.sum()), int(bad_ref.sum()), tuple(swallowed.nonzero()[0].tolist()), got[swallowed][:4].tolist())
    if same_class:
        other = bad_ref & (klass(got) != klass(ref64))
        assert not bool(other.any()), "%s: (A) %d non-finite elements changed class, first at %s" % (
            what, int(other.sum()), tuple(other.nonzero()[0].tolist()))

    # (C) the footprint and its cap
    fp = torch.zeros(got.shape[1:], dtype=torch.bool)
    if footprint is not None:
        fp = fp | footprint.cpu()
        share = float(fp.sum()) / max(fp.numel(), 1)
        assert share <= MAX_SHARE, "%s: the footprint covers %.0f%% of the planted sample (cap %.0f%%)" % (what, 100 * share, 100 * MAX_SHARE)
    spread = bad_got & ~bad_ref
    outside = spread.clone()
    outside[0] &= ~fp
    if not control:
        outside[1:] &= ~fp
    assert not bool(outside.any()), "%s: (C) %d elements are non-finite outside the reference's and the footprint, first at %s" % (
        what, int(outside.sum()), tuple(outside.nonzero()[0].tolist()))
    if control and got.shape[0] > 1:
        if control_tol is None:
            assert bits_equal(got[1:], clean_got[1:]), "%s: (C) a sample without a planted value differs from its clean bits" % what
        else:
            d = (got[1:].double() - clean_got[1:].double()).abs()
            lim = control_tol[1:] if torch.is_tensor(control_tol) and control_tol.dim() == got.dim() else control_tol
            assert bool((d <= lim).all()), "%s: (C) a sample without a planted value left its tolerance: %g" % (what, float(d.max()))

    # (B)
    fin = ~bad_got
    d = torch.where(fin, (got.double() - ref64).abs(), torch.zeros_like(ref64))
    lim = tol.detach().cpu().double().expand_as(d) if torch.is_tensor(tol) else torch.full_like(d, float(tol))
    wrong = fin & ~(d <= lim)
    assert not bool(wrong.any()), "%s: (B) %d finite elements are wrong, worst |got - ref| = %g (bound there %g) at %s" % (
        what, int(wrong.sum()), float(d[wrong].max()), float(lim[wrong][d[wrong].argmax()]), tuple(wrong.nonzero()[0].tolist()))
    return int(bad_got.sum())


def wino_footprint(shape, planted, m, off):
    """Winograd F(m x m, 3x3), forward (off = pad) or data gradient (off = 2 - pad): output tile (ty, tx) covers the output pixels
    m ty .. m ty + m - 1 and reads the input pixels m ty - off .. m ty - off + m + 1; its input transform spreads a non-finite pixel over
    the whole tile in every output channel.  shape: (channels, Ho, Wo) of one output sample; planted: (y, x) input pixels."""
    C, Ho, Wo = shape
    fp = torch.zeros(shape, dtype=torch.bool)
    for (py, px) in planted:
        tys = [t for t in range(-(-Ho // m)) if m * t - off <= py <= m * t - off + m + 1]
        txs = [t for t in range(-(-Wo // m)) if m * t - off <= px <= m * t - off + m + 1]
        for ty in tys:
            for tx in txs:
                fp[:, m * ty:m * ty + m, m * tx:m * tx + m] = True
    return fp
