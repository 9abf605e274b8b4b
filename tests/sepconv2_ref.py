"""Shared by the SepConv second-order suites: a float64 evaluation of the backward of the op's filter gradients
(savfi_sepconv_bwd2_f32, csrc/sepconv_bwd2.hip) and the gate of the second-order system fixture.

With gV, gH the filter gradients of out = sep(in, v, h) for an upstream gO, cotangents ggV of gV and ggH of gH, and frames without
gradient (the op is trilinear, so these are exact):

    d_gO = sep(in, ggV, h) + sep(in, v, ggH)        dV = the gV formula with h <- ggH        dH = the gH formula with v <- ggV
"""
import numpy as np
import torch

from tests.helpers import FP_ATOL

torch.set_num_threads(min(16, torch.get_num_threads()))        # the CPU references: at most 16 threads


def sepconv_bwd2_f64(inp, v, h, gO, ggV, ggH, dtype=torch.float64, rows=4):
    """d_gO, dV, dH in `dtype` on the given (fp32) tensors, by tap loops in another association than the kernel's (written like
    tests/sepconv_ref.sepconv_f64: chunks of `rows` output rows, addcmul_ over unfolded windows):
        T [b,c,y,x,i] = sum_j in[b,c,y+i,x+j] h  [b,j,y,x]        d_gO = sum_i (T ggV + T' v)
        T'[b,c,y,x,i] = sum_j in[b,c,y+i,x+j] ggH[b,j,y,x]        dV[b,i] = sum_c gO T'
        D [b,c,y,x,j] = sum_i in[b,c,y+i,x+j] ggV[b,i,y,x]        dH[b,j] = sum_c gO D
    ggV or ggH may be None (= zero); then dH / dV is None.  tests/test_sepconv2_ref_cpu.py holds it to double autograd through
    oracle.torch_ops.sepconv_torch."""
    cast = lambda t: None if t is None else t.detach().cpu().to(dtype)
    inp, v, h, gO, ggV, ggH = (cast(t) for t in (inp, v, h, gO, ggV, ggH))
    B, C, Hi, Wi = inp.shape
    Kk, Ho, Wo = v.shape[1], v.shape[2], v.shape[3]
    assert Hi == Ho + Kk - 1 and Wi == Wo + Kk - 1 and h.shape == v.shape and gO.shape == (B, C, Ho, Wo)
    assert ggV is not None or ggH is not None
    d_gO = torch.zeros(B, C, Ho, Wo, dtype=dtype)
    dV = torch.empty_like(v) if ggH is not None else None
    dH = torch.empty_like(h) if ggV is not None else None
    taps_last = lambda t, y0, y1: t[:, :, y0:y1].permute(0, 2, 3, 1).unsqueeze(1)        # [B,1,n,Wo,K]
    for y0 in range(0, Ho, rows):
        y1 = min(Ho, y0 + rows)
        n = y1 - y0
        g = gO[:, :, y0:y1].unsqueeze(-1)
        if ggV is not None:
            T = torch.zeros(B, C, n, Wo, Kk, dtype=dtype)
            D = torch.zeros(B, C, n, Wo, Kk, dtype=dtype)
            for f in range(Kk):
                T.addcmul_(inp[:, :, y0:y1 + Kk - 1, f:f + Wo].unfold(2, Kk, 1), h[:, f, y0:y1].view(B, 1, n, Wo, 1))
                D.addcmul_(inp[:, :, y0 + f:y1 + f, :].unfold(3, Kk, 1), ggV[:, f, y0:y1].view(B, 1, n, Wo, 1))
            d_gO[:, :, y0:y1] += (T * taps_last(ggV, y0, y1)).sum(-1)
            dH[:, :, y0:y1] = (D * g).sum(1).permute(0, 3, 1, 2)
        if ggH is not None:
            Tp = torch.zeros(B, C, n, Wo, Kk, dtype=dtype)
            for f in range(Kk):
                Tp.addcmul_(inp[:, :, y0:y1 + Kk - 1, f:f + Wo].unfold(2, Kk, 1), ggH[:, f, y0:y1].view(B, 1, n, Wo, 1))
            d_gO[:, :, y0:y1] += (Tp * taps_last(v, y0, y1)).sum(-1)
            dV[:, :, y0:y1] = (Tp * g).sum(1).permute(0, 3, 1, 2)
    return d_gO, dV, dH


def bwd2_inputs(B, C, Ho, Wo, K, seed):
    """inp, v, h, gO as _sepconv_inputs of tests/test_hip_ops_gpu.py, plus ggV, ggH ~ randn / sqrt(K)"""
    g = torch.Generator().manual_seed(seed)
    inp = torch.rand(B, C, Ho + K - 1, Wo + K - 1, generator=g)
    v = torch.randn(B, K, Ho, Wo, generator=g) / K ** 0.5
    h = torch.randn(B, K, Ho, Wo, generator=g) / K ** 0.5
    gO = torch.randn(B, C, Ho, Wo, generator=g)
    ggV = torch.randn(B, K, Ho, Wo, generator=g) / K ** 0.5
    ggH = torch.randn(B, K, Ho, Wo, generator=g) / K ** 0.5
    return inp, v, h, gO, ggV, ggH


def rel(a, b):
    """max error over max|ref|"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


# ---- the fixture tests/golden/system_sepconv_second_order_2step.npz (tools/gen_sepconv2_golden.py) ----------------------------------
FIXTURE = "system_sepconv_second_order_2step"
FP_RTOL, LOSS_RTOL = 2e-3, 5e-5          # the gates of the sibling second-order system tests (tests/test_system_gpu.py)
N_TENSORS = 94


def fp_dist(got, want):
    """how far two fingerprints [sum, abs-sum, ...] are apart: the larger of the two differences assert_fp_close bounds"""
    return max(abs(got[0] - want[0]), abs(got[1] - want[1]))


def fp_contract(want):
    """the contract part of the gate: FP_RTOL of the abs-sum scale, with assert_fp_close's absolute floor"""
    return FP_RTOL * max(abs(want[1]), 1e-12) + FP_ATOL


def fp_gate(full64, full32):
    """contract or 3 x the oracle's own fp32-vs-fp64 spread, whichever is larger"""
    return max(fp_contract(full64), 3 * fp_dist(full32, full64))


def check_fixture(fx):
    """The three properties the generator asserts before it writes, from the stored arrays: all tensors there; the fp32 oracle run is
    within the contract of the fp64 one; dropping the second-order terms moves EVERY tensor by more than 10 x the gate."""
    names = [str(n) for n in fx['names']]
    assert len(names) == N_TENSORS == len(set(names))
    for k in ('full64', 'full32', 'drop64'):
        assert fx[k + '_fp'].shape == (N_TENSORS, 6) and np.isfinite(fx[k + '_fp']).all() and np.isfinite(fx[k + '_loss'])
    assert abs(float(fx['full32_loss']) - float(fx['full64_loss'])) <= LOSS_RTOL * abs(float(fx['full64_loss']))
    for i, n in enumerate(names):
        f64, f32, d64 = fx['full64_fp'][i], fx['full32_fp'][i], fx['drop64_fp'][i]
        assert fp_dist(f32, f64) <= fp_contract(f64), (n, f32[:2], f64[:2])
        assert fp_dist(d64, f64) > 10 * fp_gate(f64, f32), (n, d64[:2], f64[:2])
