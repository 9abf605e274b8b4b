"""Shared by the convolution suites: a transcription of the F(4x4) launch plan (csrc/winograd.hip, make_plan) and the float64 references
with the per-element rounding gate.

The local gate: |got - ref| <= c_family * 2^-24 * L per element, where L is the float64 magnitude of the same operation -- the sum of
|x| |w| over the products that make the element (direct forms), max-pooled 7 x 7 for the Winograd forms: an F(4x4) output tile is made
from a 6 x 6 input patch, and its transforms spread the rounding of every product over the whole tile."""
import torch
import torch.nn.functional as F

ULP = 2.0 ** -24
torch.set_num_threads(min(16, torch.get_num_threads()))        # the CPU references: at most 16 threads

# csrc/winograd4.h and csrc/winograd.hip
TT, COB, KC = 32, 32, 8
SPLIT_SLOTS = 512
MAXC = 512


def cdiv(a, b):
    return -(-a // b)


def f4_plan(N, Ci, Co, H, W, pad, mode):
    """make_plan for a layer on the F(4x4) kernel; None where the layer's channel counts put it on F(2x2) (or the output is empty).
    mode 0: forward, 1: data gradient."""
    K, I = (Ci, Co) if mode == 0 else (Co, Ci)
    if K > MAXC or I > MAXC:
        return None
    KP, IP = cdiv(K, KC) * KC, cdiv(I, COB) * COB
    off = pad if mode == 0 else 2 - pad
    Ho, Wo = H + 2 * off - 2, W + 2 * off - 2
    if Ho <= 0 or Wo <= 0:
        return None
    ty4, tx4 = cdiv(Ho, 4), cdiv(Wo, 4)
    best, ts = -1, None
    for s in (5, 4, 3, 2, 1, 0):                 # fewest blocks, ties to the widest
        blocks = cdiv(ty4, TT >> s) * cdiv(tx4, 1 << s)
        if best < 0 or blocks < best:
            best, ts = blocks, s
    th, tw = cdiv(ty4, TT >> ts), cdiv(tx4, 1 << ts)
    nchunk = KP // KC
    wgs = th * tw * (IP // COB) * N
    want = SPLIT_SLOTS // (wgs if wgs > 0 else 1)
    want = 1 if (want < 2 or nchunk < 32) else min(want, 8)
    cps = cdiv(nchunk, want)
    if cps < 8:
        cps = nchunk if nchunk < 8 else 8
    nsplit = cdiv(nchunk, cps)
    return dict(tile_shift=ts, th=th, tw=tw, nsplit=nsplit, chunks_per_split=cps, vecw=4 if Wo % 4 == 0 else (2 if Wo % 2 == 0 else 1),
                split_reduce=nsplit > 1, ragged=nsplit > 1 and nchunk % cps != 0, off=off, Ho=Ho, Wo=Wo, IP=IP,
                workgroups=th * tw * (IP // COB) * nsplit * N)


def f4_instance(plan, masked=False, in16=False):
    """(VECW, IN16, MASK) of the wino4_conv3x3 instantiation launch_conv picks for this plan."""
    if in16:
        return (plan["vecw"], 1 + plan["off"], False)
    return (plan["vecw"], 0, bool(masked) and plan["nsplit"] == 1)


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def act(z, slope):
    return z if slope == 1.0 else F.leaky_relu(z, slope) if slope else F.relu(z)


def mask_factor(mask, mask_slope):
    """torch's semantics: relu / leaky_relu backward take the slope side at exactly 0 (and -0)."""
    return torch.where(mask > 0, torch.ones_like(mask), torch.full_like(mask, mask_slope))


def conv_tasks64(x, w, pad, T, samples=None, chans=None, bias=None):
    """conv2d of x [N,Ci,H,W] with w [T,Co,Ci,K,K] (sample n: task n % T) in float64, for the given samples and output channels (all:
    None); returns (value, magnitude = sum |x||w| (+ |bias|))."""
    samples = range(x.shape[0]) if samples is None else samples
    chans = slice(None) if chans is None else list(chans)
    val, mag = [], []
    for n in samples:
        xn, wn = x[n:n + 1].double(), w[n % T][chans].double()
        bn = None if bias is None else bias[n % T][chans].double()
        val.append(F.conv2d(xn, wn, bn, padding=pad))
        mag.append(F.conv2d(xn.abs(), wn.abs(), None if bn is None else bn.abs(), padding=pad))
    return torch.cat(val), torch.cat(mag)


def dgrad_tasks64(gy, w, pad, T, samples=None, chans=None):
    """data gradient of the pad-`pad` convolution with w [T,Co,Ci,K,K]: gy [N,Co,Ho,Wo] -> [N,Ci,H,W] in float64, for the given samples
    and input channels, with its magnitude."""
    samples = range(gy.shape[0]) if samples is None else samples
    chans = slice(None) if chans is None else list(chans)
    val, mag = [], []
    for n in samples:
        gn, wn = gy[n:n + 1].double(), w[n % T][:, chans].double()
        val.append(F.conv_transpose2d(gn, wn, padding=pad))
        mag.append(F.conv_transpose2d(gn.abs(), wn.abs(), padding=pad))
    return torch.cat(val), torch.cat(mag)


def pool7(mag):
    """the magnitude of a Winograd output: the largest direct magnitude within 3 pixels (covers the 6 x 6 patch of its 4 x 4 tile)."""
    return F.max_pool2d(mag, 7, stride=1, padding=3)


def local_bound(mag, c_family):
    """the local gate as a per-element bound: c_family * 2^-24 * L"""
    return c_family * ULP * mag


def local_ratio(got, ref, mag):
    """max over elements of |got - ref| / (2^-24 L): the measured constant of the local gate (0 where L = 0 and got == ref)."""
    d = (got.double() - ref).abs()
    lim = ULP * mag
    bad = (lim == 0) & (d > 0)
    if bool(bad.any()):
        return float("inf")
    return float((d / lim.clamp_min(1e-300)).max().item()) if d.numel() else 0.0


def global_err(got, ref):
    """(max, rms) of |got - ref| in units of the reference's largest magnitude: for messages"""
    d, scale = (got.double() - ref), max(ref.abs().max().item(), 1e-300)
    return d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale


# measured maxima of local_ratio per kernel family, filled by every assert_local (tools that measure c_family switch GATE off)
MEASURED = {}
CASES_MEASURED = []
GATE = True
SEED_OFFSET = 0         # added to every seed of the suites that use this module (measurements over several seeds)


def assert_local(got, ref, mag, c_family, family, what=""):
    r = local_ratio(got, ref, mag)
    MEASURED[family] = max(MEASURED.get(family, 0.0), r)
    if not GATE:
        CASES_MEASURED.append((r, family, what))
    if GATE:
        assert r <= c_family, "%s %s: |got - ref| reaches %.3g x 2^-24 L (gate %g)" % (family, what, r, c_family)
    return r
