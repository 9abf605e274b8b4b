"""Shared by the SepConv partition suites: a transcription of the work partition of the three persistent kernels (csrc/sepconv_ws.hip,
csrc/sepconv_x6.hip, sepconv_bwd_mfma_p of csrc/sepconv.hip), what a launch reaches under it, and a float64 evaluation of the op and its
filter gradients.

The persistent kernels launch at most one workgroup per CU.  The phases of all strips in strip-major order -- position g is phase
g % nph of strip g / nph, strip s is strip s % ncol of sample s / ncol -- are cut into one piece [g0, g1) per workgroup.  A piece that
crosses into the next strip (or, with it, the next sample) starts a new RUN there: a new LDS window, reset flags, a pipeline ramp.
tests/test_sepconv_partition_cpu.py holds the transcription to the library's own answer (savfi_sepconv_partition);
tests/test_sepconv_partition_gpu.py computes with it which of those states each of its launches reaches."""
import torch

torch.set_num_threads(min(16, torch.get_num_threads()))        # the CPU references: at most 16 threads

K = 51
WS, X6, FP32 = 0, 1, 2                            # SAVFI_SEPCONV_PARTITION_* (include/savfi_hip.h)
# csrc/sepconv_x6_shared.h: rows per phase and strip width of the split-bf16 kernels, half phases that a strip start costs
XPR, XMC = 4, 32
WS_RUN_COST = 2
# csrc/sepconv.hip: the fp32 persistent kernel works in phases of two rows on strips of MC columns
PPR, MC = 2, 64


def cdiv(a, b):
    return -(-a // b)


def geometry(kind, B, Ho, Wo):
    """(phase rows, strip columns, nph = phases per strip, ncol = strips per sample, total phases)"""
    rows, cols = (PPR, MC) if kind == FP32 else (XPR, XMC)
    nph, ncol = cdiv(Ho, rows), cdiv(Wo, cols)
    return rows, cols, nph, ncol, B * ncol * nph


def ws_cost_to_phase(t, nph):
    C = 2 * nph + WS_RUN_COST
    strip = t // C
    r = t - strip * C
    return strip * nph + min(max((r - WS_RUN_COST + 1) >> 1, 0), nph)


def grid_size(kind, B, Ho, Wo, cus):
    total = geometry(kind, B, Ho, Wo)[4]
    return cdiv(total, cdiv(total, cus))           # ws_grid; per_wg and grid of the other two launchers


def pieces(kind, B, Ho, Wo, cus):
    """[(g0, g1)] for every workgroup of a launch planned for `cus` CUs"""
    _, _, nph, ncol, total = geometry(kind, B, Ho, Wo)
    grid = grid_size(kind, B, Ho, Wo, cus)
    if kind == WS:
        T = B * ncol * (2 * nph + WS_RUN_COST)
        return [(ws_cost_to_phase(bx * T // grid, nph), ws_cost_to_phase((bx + 1) * T // grid, nph)) for bx in range(grid)]
    per_wg = cdiv(total, cus)
    return [(bx * per_wg, min(bx * per_wg + per_wg, total)) for bx in range(grid)]


def ws_piece_bound(B, Ho, Wo, grid):
    """The most phases a piece of the wave-specialised partition can hold.  The cost axis has T = S (2 nph + WS_RUN_COST) slots
    (S = B ncol strips); workgroup bx takes the slots [floor(bx T / G), floor((bx + 1) T / G)): at most ceil(T / G) of them.  A phase
    is counted where the position passes an odd offset r = WS_RUN_COST + 1 + 2 p of its strip (ws_cost_to_phase), so phases begin at
    least two slots apart and L consecutive slots hold at most ceil(L / 2) of them.

    In terms of the even share: with C = 2 nph + WS_RUN_COST slots per strip write S C / G = q C + rho, 0 <= rho < C.  A piece has at
    most q C + ceil(rho) slots: q whole periods with nph phases each and ceil(rho) more slots with at most ceil(ceil(rho) / 2)
    < rho / 2 + 3 / 2 phases, while the even share total / G = (q + rho / C) nph is at least q nph + rho / 2 - WS_RUN_COST / 2.  So a piece
    holds fewer than total / G + 3 / 2 + WS_RUN_COST / 2 phases: at most cdiv(total, G) + WS_RUN_COST for WS_RUN_COST = 2 (the test
    asserts both forms)."""
    _, _, nph, ncol, _ = geometry(WS, B, Ho, Wo)
    return cdiv(cdiv(B * ncol * (2 * nph + WS_RUN_COST), grid), 2)


def runs(piece, nph, ncol):
    """the runs of a piece: [(sample, strip of the sample, first phase, phases)]"""
    g, g1 = piece
    out = []
    while g < g1:
        s, ph0 = divmod(g, nph)
        n = min(g1 - g, nph - ph0)
        out.append((s // ncol, s % ncol, ph0, n))
        g += n
    return out


def describe(kind, B, Ho, Wo, cus):
    """What a launch reaches under the partition: the coverage claims of the GPU cases are assertions on this."""
    rows, cols, nph, ncol, total = geometry(kind, B, Ho, Wo)
    ps = pieces(kind, B, Ho, Wo, cus)
    rs = [runs(p, nph, ncol) for p in ps]
    allruns = [r for wg in rs for r in wg]
    samples = [sorted({r[0] for r in wg}) for wg in rs]
    return dict(
        grid=len(ps), nph=nph, ncol=ncol, total=total,
        phases=[g1 - g0 for g0, g1 in ps],
        max_phases=max(g1 - g0 for g0, g1 in ps),
        runs_per_wg=[len(wg) for wg in rs],
        max_runs=max(len(wg) for wg in rs),
        run_lengths=sorted({r[3] for r in allruns}),
        longest_run=max(r[3] for r in allruns),
        starts_mid_strip=sum(1 for wg in rs if wg and wg[0][2] != 0),             # pieces whose first run begins inside a strip
        ends_mid_strip=sum(1 for wg in rs if wg and wg[-1][2] + wg[-1][3] != nph),  # ... whose last run stops inside one
        sample_crossings=sum(len(s) - 1 for s in samples),                        # sample boundaries inside a stretch
        max_samples_per_wg=max(len(s) for s in samples),
        # a pair launch alternates frames: virtual sample 2 b + f reads `in` for f = 0 and `in2` for f = 1
        frame_switches=sorted({(a % 2, b % 2) for s in samples for a, b in zip(s, s[1:])}),
        empty=sum(1 for g0, g1 in ps if g0 >= g1),
        ragged_rows=Ho % rows, ragged_strip=Wo % cols,
    )


def check_tiling(ps, total):
    """pieces are ordered, disjoint and tile [0, total) exactly"""
    pos = 0
    for g0, g1 in ps:
        assert g0 == pos and g1 >= g0, (ps, total)
        pos = g1
    assert pos == total, (ps, total)


def sepconv_f64(inp, v, h, gO, rows=4):
    """out, gV, gH of the op in float64 on the given (fp32) tensors, by tap loops in another association than any kernel's:
        M1[b,c,y,x,fy] = sum_fx in[b,c,y+fy,x+fx] h[b,fx,y,x]        out = sum_fy M1 v        gV[b,fy] = sum_c gO M1
        M2[b,c,y,x,fx] = sum_fy in[b,c,y+fy,x+fx] v[b,fy,y,x]                                 gH[b,fx] = sum_c gO M2
    in chunks of `rows` output rows (the partial sums of a chunk stay in the caches).  tests/test_sepconv_partition_cpu.py holds it to
    autograd through oracle.torch_ops.sepconv_torch in double."""
    inp, v, h, gO = (t.detach().cpu().double() for t in (inp, v, h, gO))
    B, C, Hi, Wi = inp.shape
    Kk, Ho, Wo = v.shape[1], v.shape[2], v.shape[3]
    assert Hi == Ho + Kk - 1 and Wi == Wo + Kk - 1 and h.shape == v.shape and gO.shape == (B, C, Ho, Wo)
    out = torch.empty(B, C, Ho, Wo, dtype=torch.float64)
    gV, gH = torch.empty_like(v), torch.empty_like(h)
    for y0 in range(0, Ho, rows):
        y1 = min(Ho, y0 + rows)
        n = y1 - y0
        M1 = torch.zeros(B, C, n, Wo, Kk, dtype=torch.float64)
        M2 = torch.zeros(B, C, n, Wo, Kk, dtype=torch.float64)
        for f in range(Kk):
            # [B,C,n,Wo,K]: in[y + fy, x + f] over fy; in[y + f, x + fx] over fx
            M1.addcmul_(inp[:, :, y0:y1 + Kk - 1, f:f + Wo].unfold(2, Kk, 1), h[:, f, y0:y1].view(B, 1, n, Wo, 1))
            M2.addcmul_(inp[:, :, y0 + f:y1 + f, :].unfold(3, Kk, 1), v[:, f, y0:y1].view(B, 1, n, Wo, 1))
        g = gO[:, :, y0:y1].unsqueeze(-1)
        out[:, :, y0:y1] = (M1 * v[:, :, y0:y1].permute(0, 2, 3, 1).unsqueeze(1)).sum(-1)
        gV[:, :, y0:y1] = (M1 * g).sum(1).permute(0, 3, 1, 2)
        gH[:, :, y0:y1] = (M2 * g).sum(1).permute(0, 3, 1, 2)
    return out, gV, gH
