"""tests/dain_ops_ref.py -- TEST INFRASTRUCTURE (never imported by the product path).

DAIN's two own CUDA extensions restated in numpy, loop for loop, forward and backward:

  dain/my_package/FilterInterpolation/filterinterpolation_cuda_kernel.cu     forward :29-160, backward :164-460
  dain/my_package/DepthFlowProjection/depthflowprojection_cuda_kernel.cu     scatter :29-96, averaging :99-143, hole fill :146-241,
                                                                             backward :244-341

Index and validity decisions -- x2, y2, the W/2.f test, int(), alpha, beta -- are taken in FLOAT32 exactly as the kernels take them
(csrc/dainwarp.hip warp_geom / proj_src), so the restatement and the kernel decide identically on every input.  Everything after the
decision is computed in `dtype`:

  dtype=np.float64 (default)   the yardstick
  dtype=np.float32             every product and sum rounded to fp32, accumulated sequentially in raster order (pixel by pixel, the
                               reference's statement order inside a pixel): one admissible ordering of the reference's own fp32
                               atomics, whose arrival order cannot be run here.  |fp32 mode - float64| stands for the reference's
                               own fp32 error.

Loops run over pixels (and over channels where a sum over channels has an order); the channel axis is vectorised where the channels
are independent, which changes no rounding.
"""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# adaptive warping
# ---------------------------------------------------------------------------------------------------------------------------------
def warp_geom(fx, fy, w_i, h_i, W, H):
    """.cu:65-80 in float32.  None for an invalid pixel, else (rows[4], cols[4], alpha, beta) with alpha, beta float32."""
    fx, fy = F32(fx), F32(fy)
    x2 = F32(w_i) + fx
    y2 = F32(h_i) + fy
    if not (x2 >= F32(0) and y2 >= F32(0) and x2 <= F32(W - 1) and y2 <= F32(H - 1)
            and abs(fx) < F32(W) / F32(2) and abs(fy) < F32(H) / F32(2)):          # :72-73 (a NaN fails every comparison)
        return None
    ix, iy = int(x2), int(y2)                                                       # truncation of a non-negative value
    L, T = ix + 1 - 2, iy + 1 - 2                                                   # :74-75, filter_size = 4
    rows = [min(max(0, T + j), H - 1) for j in range(4)]                            # :88 (the clamp serves input1 only)
    cols = [min(max(0, L + i), W - 1) for i in range(4)]                            # :90
    return rows, cols, x2 - F32(ix), y2 - F32(iy)                                   # :79-80


# taps of the four quadrants in the reference's loop order (:87-124): rows 0-1 top, columns 0-1 left; tap (j, i) = channel 4 j + i
_QUAD_TAPS = ((0, 1, 4, 5), (2, 3, 6, 7), (8, 9, 12, 13), (10, 11, 14, 15))      # TL, TR, BL, BR


def _quadrants(V, Fk):
    """V [C,16] gathered inputs, Fk [16] filter taps -> TL, TR, BL, BR [C] summed in the reference's order."""
    P = V * Fk
    out = []
    for taps in _QUAD_TAPS:
        s = P[:, taps[0]].copy()
        for k in taps[1:]:
            s = s + P[:, k]
        out.append(s)
    return out


def filterinterp_forward(inp, flow, filt, dtype=np.float64):
    B, C, H, W = inp.shape
    assert flow.shape == (B, 2, H, W) and filt.shape == (B, 16, H, W)
    x, f = inp.astype(dtype), filt.astype(dtype)
    out = np.empty((B, C, H, W), dtype)
    one = dtype(1)
    with np.errstate(invalid='ignore'):
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    g = warp_geom(flow[b, 0, h, w], flow[b, 1, h, w], w, h, W, H)
                    if g is None:
                        out[b, :, h, w] = x[b, :, h, w]                             # :151-156
                        continue
                    rows, cols, al, be = g
                    al, be = dtype(al), dtype(be)
                    V = x[b][:, rows][:, :, cols].reshape(C, 16)
                    TL, TR, BL, BR = _quadrants(V, f[b, :, h, w])
                    out[b, :, h, w] = (one - al) * (one - be) * TL + al * (one - be) * TR + (one - al) * be * BL + al * be * BR   # :126-130
    return out


def filterinterp_backward(inp, flow, filt, gout, dtype=np.float64):
    """-> g_in, g_flow, g_filt (all zero where the pixel is invalid: the reference's gradients start zeroed and an invalid pixel
    adds nothing, :200-201 -- not even to input1, which the forward passes through)."""
    B, C, H, W = inp.shape
    x, f, go = inp.astype(dtype), filt.astype(dtype), gout.astype(dtype)
    g_in = np.zeros((B, C, H, W), dtype)
    g_flow = np.zeros((B, 2, H, W), dtype)
    g_filt = np.zeros((B, 16, H, W), dtype)
    one = dtype(1)
    with np.errstate(invalid='ignore'):
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    g = warp_geom(flow[b, 0, h, w], flow[b, 1, h, w], w, h, W, H)
                    if g is None:
                        continue
                    rows, cols, al, be = g
                    al, be = dtype(al), dtype(be)
                    V = x[b][:, rows][:, :, cols].reshape(C, 16)
                    Fk = f[b, :, h, w]
                    G = go[b, :, h, w]
                    QG = (G * (one - al) * (one - be), G * al * (one - be), G * (one - al) * be, G * al * be)    # :222,237,253,269
                    gf = np.zeros(16, dtype)
                    for q, taps in enumerate(_QUAD_TAPS):
                        for k in taps:
                            g_in[b, :, rows[k >> 2], cols[k & 3]] += QG[q] * Fk[k]  # :227-229 (atomicAdd; clamped taps coincide)
                    quad = np.empty(16, np.intp)
                    for q, taps in enumerate(_QUAD_TAPS):
                        quad[list(taps)] = q
                    QGm = np.stack(QG, axis=1)                                      # [C,4]
                    for c in range(C):                                              # :230-232, one add per channel in channel order
                        gf = gf + QGm[c, quad] * V[c]
                    g_filt[b, :, h, w] = gf
                    TL, TR, BL, BR = _quadrants(V, Fk)
                    gamma = one - be                                                # :302
                    tx = gamma * (TR - TL) + (one - gamma) * (BR - BL)              # :347-349
                    gamma = one - al                                                # :373
                    ty = gamma * (BL - TL) + (one - gamma) * (BR - TR)              # :418-420
                    bx, by = dtype(0), dtype(0)
                    for c in range(C):
                        bx = bx + G[c] * tx[c]                                      # :350
                        by = by + G[c] * ty[c]                                      # :421
                    g_flow[b, 0, h, w] = bx
                    g_flow[b, 1, h, w] = by
    return g_in, g_flow, g_filt


# ---------------------------------------------------------------------------------------------------------------------------------
# depth-aware flow projection
# ---------------------------------------------------------------------------------------------------------------------------------
def proj_src(fx, fy, w_i, h_i, W, H):
    """.cu:65-74 in float32.  None when the source is not scattered, else (L, T, R, Bt)."""
    x2 = F32(w_i) + F32(fx)
    y2 = F32(h_i) + F32(fy)
    if not (x2 >= F32(0) and y2 >= F32(0) and x2 <= F32(W - 1) and y2 <= F32(H - 1)):
        return None
    L, T = int(x2), int(y2)
    return L, T, min(L + 1, W - 1), min(T + 1, H - 1)


def _targets(s):
    L, T, R, Bt = s
    return ((T, L), (T, R), (Bt, L), (Bt, R))                                       # the reference's order; doubled targets stay doubled


def depthflowproj_forward(flow, wgt, fillhole, dtype=np.float64):
    """-> out [B,2,H,W], count [B,1,H,W]"""
    B, two, H, W = flow.shape
    assert two == 2 and wgt.shape == (B, 1, H, W)
    fl, wt = flow.astype(dtype), wgt.astype(dtype)
    out = np.zeros((B, 2, H, W), dtype)
    count = np.zeros((B, 1, H, W), dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    s = proj_src(flow[b, 0, h, w], flow[b, 1, h, w], w, h, W, H)
                    if s is None:
                        continue
                    t = wt[b, 0, h, w]
                    vx, vy = -t * fl[b, 0, h, w], -t * fl[b, 1, h, w]
                    for (ty, tx) in _targets(s):                                    # :78-91
                        out[b, 0, ty, tx] += vx
                        out[b, 1, ty, tx] += vy
                        count[b, 0, ty, tx] += t
            pos = count[b, 0] > 0                                                   # :136-139
            out[b, 0][pos] = out[b, 0][pos] / count[b, 0][pos]
            out[b, 1][pos] = out[b, 1][pos] / count[b, 0][pos]
            if fillhole:
                cn = count[b, 0]
                src = out[b].copy()           # sources have count > 0 and are never written by the fill: reading the copy changes nothing
                for h in range(H):
                    for w in range(W):
                        if cn[h, w] > 0:
                            continue                                                # :183
                        lo, lt = w, dtype(0)
                        while lt == 0 and lo - 1 >= 0:                              # :185-189
                            lo -= 1
                            lt = cn[h, lo]
                        ro, rt = w, dtype(0)
                        while rt == 0 and ro + 1 <= W - 1:                          # :191-195
                            ro += 1
                            rt = cn[h, ro]
                        uo, ut = h, dtype(0)
                        while ut == 0 and uo - 1 >= 0:                              # :197-201
                            uo -= 1
                            ut = cn[uo, w]
                        dn, dt = h, dtype(0)
                        while dt == 0 and dn + 1 <= H - 1:                          # :203-207
                            dn += 1
                            dt = cn[dn, w]
                        if lt + rt + ut + dt <= 0:                                  # :209-212
                            continue
                        lt, rt, ut, dt = (dtype(1 if v > 0 else 0) for v in (lt, rt, ut, dt))     # :214-217
                        for ch in range(2):                                         # :219-236
                            out[b, ch, h, w] = (lt * src[ch, h, lo] + rt * src[ch, h, ro] + ut * src[ch, uo, w] + dt * src[ch, dn, w]) \
                                / (lt + rt + ut + dt)
    return out, count


def depthflowproj_backward(flow, wgt, count, out, gout, dtype=np.float64):
    """.cu:276-337 as written -> g_flow [B,2,H,W], g_w [B,1,H,W].  `count` and `out` are the forward's (out after the fill)."""
    B, _, H, W = flow.shape
    fl, wt, cn, ot, go = (a.astype(dtype) for a in (flow, wgt, count, out, gout))
    g_flow = np.zeros((B, 2, H, W), dtype)
    g_w = np.zeros((B, 1, H, W), dtype)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    s = proj_src(flow[b, 0, h, w], flow[b, 1, h, w], w, h, W, H)
                    if s is None:
                        continue
                    t = wt[b, 0, h, w]
                    for ch in range(2):
                        a = dtype(0)
                        for (ty, tx) in _targets(s):
                            a = a + (-go[b, ch, ty, tx] * t / cn[b, 0, ty, tx])     # :291-308
                        g_flow[b, ch, h, w] = a
                    a = dtype(0)
                    for ch in range(2):
                        f = fl[b, ch, h, w]
                        for (ty, tx) in _targets(s):
                            a = a + (-go[b, ch, ty, tx] / cn[b, 0, ty, tx] * (f - ot[b, ch, ty, tx]))   # :312-336
                    g_w[b, 0, h, w] = a
    return g_flow, g_w
