// Second-order terms of the separable local convolution (SepConv) for gfx950: the backward of its filter gradients.
//
//   out[b,c,y,x] = sum_i sum_j in[b,c,y+i,x+j] * v[b,i,y,x] * h[b,j,y,x]                   (csrc/sepconv.hip)
//   gV, gH       = the filter gradients of that for an upstream gO                         (csrc/sepconv.hip)
//
// The op is trilinear in (in, v, h) and the frames carry no gradient here, so with cotangents ggV of gV and ggH of gH
//
//   d_gO[c]  = sum_i ( ggV_i * T_i[c] + v_i * T'_i[c] )        T[c]  = W[c] . h      (window rows times a tap vector)
//   dV_i     = sum_c gO_c * T'_i[c]                            T'[c] = W[c] . ggH
//   dH_j     = sum_c gO_c * D_j[c]                             D[c]  = W[c]^T . ggV  (window columns)
//
// per output pixel, W[c] = in[c, y + ., x + .] its K x K window.  One launch, every requested element written once from a sequential
// sum: no atomics, no cleared memory, nothing read back by the host.
//
// K = 51, C = 3: sepconv_bwd2_mfma -- the banded-GEMM statement of csrc/sepconv.hip on the exact-fp32 matrix cores, every wave the
// same program (no wave roles, no waits on LDS flags).  Every other (K, C): sepconv_bwd2_direct, one thread per output pixel.
#include "common.h"

namespace {

constexpr int KFAST = 51;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// geometry shared with the first-order fp32 MFMA kernels (csrc/sepconv.hip; that file's helpers are private to it, the few needed here
// are restated): 8 waves = 2 row lanes x 4 column groups of 16 pixels, a window of MROWS + 50 rows x 116 columns per channel at pitch 132
constexpr int MC = 64, MLW = 132, MSPAN = 116, MNT = 512;
constexpr int TAPROWS = 52;                     // rows of a wave's [tap][16] LDS buffer (51 taps + one spare)
constexpr unsigned OOR = 0x80000000u;           // a byte offset no buffer resource here reaches: such a lane stores nothing

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void bstore(float val, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), r, (int)voff, (int)soff, 0);
}

// LH x SPAN window of a [Hi, Wi] plane (top-left (y0, x0)) -> LDS rows of pitch LW; thread -> (column tid % 128, row group tid / 128).
// Coordinates past the plane are clamped: such entries only feed output pixels outside the image, which are never stored.
template <int LH, int SPAN, int LW, int NTHREADS>
__device__ __forceinline__ void stage_window(float* __restrict__ tile, const float* __restrict__ src, int y0, int x0, int Hi, int Wi,
                                             int tid) {
  static_assert(SPAN <= 128 && NTHREADS % 128 == 0, "one column per thread");
  constexpr int RG = NTHREADS / 128, NIT = (LH + RG - 1) / RG;
  const int q = tid & 127, rg = tid >> 7;
  const __amdgpu_buffer_rsrc_t rs = rsrc(src, (unsigned)(Hi * Wi) * 4u);
  const int colb = min(x0 + q, Wi - 1) * 4, rowb = Wi * 4;
  float buf[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) buf[it] = bload(rs, (unsigned)(min(y0 + rg + it * RG, Hi - 1) * rowb + colb), 0u);
  float* dst = tile + rg * LW + q;
  if (q < SPAN) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (it * RG + RG <= LH || rg + it * RG < LH) dst[it * RG * LW] = buf[it];
  }
}

// Two register layouts of a pixel strip's taps (lane = (column j = lane & 15, group ks = lane >> 4)), both 64-byte runs per tap plane:
//   "band" layout   regs[it] = tap 4 it + ks            -> the wave's [tap][16] LDS rows, from which the banded B operand is gathered
//   "tile" layout   regs[mm][e] = tap 16 mm + 4 ks + e  -> the taps that meet the accumulator rows of M-tile mm of a channel, and the
//                                                          k-slots of the column contraction
// A lane whose tap is >= K loads through the offset OOR, which lies past every resource: the hardware returns 0 for it, and no address
// outside the K planes is ever formed.
template <int NREG>
__device__ __forceinline__ void load_band(float (&regs)[NREG], __amdgpu_buffer_rsrc_t src, unsigned plane_b, unsigned pix_b, int ks) {
  const unsigned voff = (unsigned)ks * plane_b + pix_b;
#pragma unroll
  for (int it = 0; it < NREG; ++it)
    regs[it] = bload(src, (4 * it + 3 >= KFAST && 4 * it + ks >= KFAST) ? OOR : voff, (unsigned)(4 * it) * plane_b);
}
__device__ __forceinline__ void load_tile(f32x4 (&regs)[4], __amdgpu_buffer_rsrc_t src, unsigned plane_b, unsigned pix_b, int ks) {
#pragma unroll
  for (int mm = 0; mm < 4; ++mm)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      regs[mm][e] = bload(src, (16 * mm + 12 + e >= KFAST && 16 * mm + 4 * ks + e >= KFAST) ? OOR : (unsigned)(4 * ks) * plane_b + pix_b,
                          (unsigned)(min(16 * mm + e, KFAST)) * plane_b);
}
template <int K, int NREG>
__device__ __forceinline__ void store_band(float* __restrict__ dst /* [TAPROWS][16] */, const float (&regs)[NREG], int lane) {
  static_assert(4 * NREG <= TAPROWS, "tap rows");
#pragma unroll
  for (int it = 0; it < NREG; ++it) dst[(4 * it + (lane >> 4)) * 16 + (lane & 15)] = regs[it];     // tap 51 arrives as 0 (see above)
}

// ------------------------------------------------------------------------------------------------------------------------------------
// K = 51, C = 3.  Workgroup = MROWS output rows x 64 columns, processed two rows at a time by 2 x 4 waves; wave (wr, wc) owns the 16 pixels
// x0 + 16 wc .. + 15 of row y0 + 2 ph + wr.  The window of `in` is staged ONCE per workgroup; a strip's four tap vectors are fetched ONCE
// per row, one row ahead (h and ggH into the wave's private LDS rows, v and ggV into registers), and feed three contractions:
//
//   T [(c,i), p] = sum_q W[c][i][q] * Hb [q][p],   Hb [q][p] = h  [q - p][y][x0 + p]      (the banded operand of csrc/sepconv.hip:66)
//   T'[(c,i), p] = sum_q W[c][i][q] * Hb'[q][p],   Hb'[q][p] = ggH[q - p][y][x0 + p]      same A fragments, a second accumulator
//   D'[q, p]     = sum_{c,i} W[c][i][q] * (gO[c,p] * ggV[i,p]),   dH[j, p] = D'[p + j, p]  (csrc/sepconv.hip:292-293 with v <- ggV)
//
// M layout of T / T': 64 rows per channel (51 taps, 13 of padding) = four M-tiles, so that accumulator (mm, e) of a lane is tap
// 16 mm + 4 ks + e of ONE channel for every c: dV accumulates over c in registers, and the taps that meet the accumulators are the
// "tile" registers.  12 x 17 x 2 MFMAs for T and T', 3 x 15 x 4 for D' (its k-slots are taps in the tile layout too; slot (3, 3) holds
// only taps >= 51 and is skipped) -- 588 per 16 pixels, against 2 x (170 + 399) for two forwards and two backwards of the fp32 kernels.
// GV / GH: ggV / ggH is present (an absent one is zero: its contraction is skipped, not multiplied out); DH: dH is wanted.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int K, int MROWS, bool GV, bool GH, bool DH>
__global__ __launch_bounds__(MNT) void sepconv_bwd2_mfma(const float* __restrict__ in, const float* __restrict__ v,
                                                         const float* __restrict__ h, const float* __restrict__ gO,
                                                         const float* __restrict__ ggV, const float* __restrict__ ggH,
                                                         float* __restrict__ d_gO, float* __restrict__ dV, float* __restrict__ dH,
                                                         int Ho, int Wo) {
  constexpr int C = 3, LH = MROWS + K - 1, LP = LH * MLW;
  constexpr int KT = (16 + K - 1 + 3) / 4;                 // 17 column steps of the banded operands
  constexpr int NREG = (K + 3) / 4;                        // 13 dwords per lane per band-layout tap array
  static_assert(K == 51 && KT == 17 && 16 * 3 + 4 * KT <= MSPAN && MSPAN <= MLW && MLW % 4 == 0 && MROWS % 2 == 0, "operand geometry");
  static_assert(GV || GH, "one cotangent at least");
  static_assert(!DH || GV, "dH needs ggV");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* inT = lds;                                                        // [C][LH][MLW]
  float* hB = lds + C * LP + (threadIdx.x >> 6) * 2 * TAPROWS * 16;        // this wave's [TAPROWS][16] h taps ...
  float* gB = hB + TAPROWS * 16;                                           // ... and ggH taps

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wc = w & 3, wr = w >> 2;
  const int j = lane & 15, ks = lane >> 4;
  const int x0 = blockIdx.x * MC, y0 = blockIdx.y * MROWS, b = blockIdx.z;
  const int Hi = Ho + K - 1, Wi = Wo + K - 1;
  const size_t plane = (size_t)Ho * Wo;
  const unsigned plane_b = (unsigned)plane * 4u;
  const __amdgpu_buffer_rsrc_t hsrc = rsrc(h + (size_t)b * K * plane, (unsigned)K * plane_b);
  const __amdgpu_buffer_rsrc_t vsrc = rsrc(v + (size_t)b * K * plane, (unsigned)K * plane_b);
  const __amdgpu_buffer_rsrc_t ghsrc = rsrc(GH ? ggH + (size_t)b * K * plane : nullptr, GH ? (unsigned)K * plane_b : 0u);
  const __amdgpu_buffer_rsrc_t gvsrc = rsrc(GV ? ggV + (size_t)b * K * plane : nullptr, GV ? (unsigned)K * plane_b : 0u);
  const __amdgpu_buffer_rsrc_t gsrc = rsrc(gO + (size_t)b * C * plane, (unsigned)C * plane_b);
  // an output that is not wanted (a NULL pointer: uniform over the launch) is never stored to
  const __amdgpu_buffer_rsrc_t odst = rsrc(d_gO ? d_gO + (size_t)b * C * plane : nullptr, d_gO ? (unsigned)C * plane_b : 0u);
  const __amdgpu_buffer_rsrc_t vdst = rsrc(dV ? dV + (size_t)b * K * plane : nullptr, dV ? (unsigned)K * plane_b : 0u);
  const __amdgpu_buffer_rsrc_t hdst = rsrc(dH ? dH + (size_t)b * K * plane : nullptr, dH ? (unsigned)K * plane_b : 0u);
  // byte offset of this lane's pixel in row y of a plane (clamped: pixels outside the image are computed and never stored)
  auto pix_off = [&](int y) { return (unsigned)(min(y, Ho - 1) * Wo + min(x0 + 16 * wc + j, Wo - 1)) * 4u; };

  float hreg[NREG], greg[NREG], g[C];
  f32x4 v16[4], w16[4];                                    // v and ggV in the tile layout
  {
    const unsigned po = pix_off(y0 + wr);
    load_band<NREG>(hreg, hsrc, plane_b, po, ks);
    if (GH) load_band<NREG>(greg, ghsrc, plane_b, po, ks);
    load_tile(v16, vsrc, plane_b, po, ks);
    if (GV) load_tile(w16, gvsrc, plane_b, po, ks);
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = bload(gsrc, po, (unsigned)c * plane_b);
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    stage_window<LH, MSPAN, MLW, MNT>(inT + c * LP, in + ((size_t)b * C + c) * Hi * Wi, y0, x0, Hi, Wi, tid);
  store_band<K, NREG>(hB, hreg, lane);
  if (GH) store_band<K, NREG>(gB, greg, lane);
  __syncthreads();
  // the two waves of a SIMD run the same instruction stream: a one-off head start for one of them lets each wave's VALU / LDS / store
  // phases hide under the other's MFMAs (csrc/sepconv.hip)
  if (wr == 1) __builtin_amdgcn_s_sleep(40);

#pragma unroll 1
  for (int ph = 0; ph < MROWS / 2; ++ph) {
    const int y = y0 + 2 * ph + wr;
    const int x = x0 + 16 * wc + j;
    const bool pvalid = (x < Wo) && (y < Ho);
    const unsigned opix_b = pix_off(y);
    const int rowoff = (2 * ph + wr) * MLW + 16 * wc;
    const bool more = ph + 1 < MROWS / 2;

    // banded B operands.  Slot (step t, lane group ks) takes window column q = 16 (t / 4) + 4 ks + t % 4 for t < 16 and 64 + ks for
    // t = 16, so that a lane's 16 A values of an M-tile are four aligned 16-byte LDS reads and one dword (csrc/sepconv.hip)
    float bh[KT], bg[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int q = (t < 16) ? (16 * (t >> 2) + 4 * ks + (t & 3)) : (64 + ks);
      const int tap = q - j;
      const bool live = tap >= 0 && tap < K;
      const int row = min(max(tap, 0), K - 1) * 16 + j;
      if (GV) { const float val = hB[row]; bh[t] = live ? val : 0.f; }
      if (GH) { const float val = gB[row]; bg[t] = live ? val : 0.f; }
    }
    // the tap rows are dead from here to the end of the row: the next row's h / ggH leave HBM now
    if (more) {
      const unsigned po = pix_off(y + 2);
      load_band<NREG>(hreg, hsrc, plane_b, po, ks);
      if (GH) load_band<NREG>(greg, ghsrc, plane_b, po, ks);
    }

    // ---- T and T': 12 M-tiles (c, mm), A row = tap 16 mm + j of channel c (rows >= 51 are padding: they repeat row 50 and meet zero taps)
    float o[C] = {0.f, 0.f, 0.f};
    f32x4 dv[4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) dv[mm] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto load_a = [&](f32x4 (&d)[4], float& tail, int m) {
      const int c = m >> 2, mm = m & 3;
      const float* ap = inT + c * LP + min(16 * mm + j, K - 1) * MLW + rowoff + 4 * ks;
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = *reinterpret_cast<const f32x4*>(ap + 16 * u);
      tail = ap[64 - 3 * ks];                                                  // column 64 + ks (the base holds + 4 ks)
    };
    f32x4 a[4], an[4];
    float at, ant;
    load_a(a, at, 0);
#pragma unroll
    for (int m = 0; m < 4 * C; ++m) {
      const int c = m >> 2, mm = m & 3;
      if (m + 1 < 4 * C) load_a(an, ant, m + 1);
      f32x4 accT = {0.f, 0.f, 0.f, 0.f}, accP = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        if (GV) accT = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t >> 2][t & 3], bh[t], accT, 0, 0, 0);
        if (GH) accP = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t >> 2][t & 3], bg[t], accP, 0, 0, 0);
      }
      if (GV) accT = __builtin_amdgcn_mfma_f32_16x16x4f32(at, bh[16], accT, 0, 0, 0);
      if (GH) accP = __builtin_amdgcn_mfma_f32_16x16x4f32(at, bg[16], accP, 0, 0, 0);
      // the lane holds rows 16 mm + 4 ks + e of pixel j, channel c
      if (GV) {
        float s = w16[mm][0] * accT[0];
        s = fmaf(w16[mm][1], accT[1], s);
        s = fmaf(w16[mm][2], accT[2], s);
        s = fmaf(w16[mm][3], accT[3], s);
        o[c] += s;
      }
      if (GH) {
        float s = v16[mm][0] * accP[0];
        s = fmaf(v16[mm][1], accP[1], s);
        s = fmaf(v16[mm][2], accP[2], s);
        s = fmaf(v16[mm][3], accP[3], s);
        o[c] += s;
#pragma unroll
        for (int e = 0; e < 4; ++e) dv[mm][e] = fmaf(g[c], accP[e], dv[mm][e]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = an[u];
      at = ant;
      // one tile of A fragments in flight, not more: left alone the scheduler hoists several tiles' LDS reads and the kernel spills
      __builtin_amdgcn_sched_barrier(0);
    }
    // the 4 k-lanes of a pixel hold disjoint row subsets: fold them
#pragma unroll
    for (int c = 0; c < C; ++c) {
      o[c] += __shfl_xor(o[c], 16, 64);
      o[c] += __shfl_xor(o[c], 32, 64);
      if (d_gO) bstore(o[c], odst, (pvalid && ks == 0) ? opix_b : OOR, (unsigned)c * plane_b);
    }
    if (GH && dV) {
#pragma unroll
      for (int mm = 0; mm < 4; ++mm)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (16 * mm + e < K) bstore(dv[mm][e], vdst, (pvalid && 16 * mm + 4 * ks + e < K) ? opix_b + (unsigned)(4 * ks) * plane_b : OOR,
                 (unsigned)(16 * mm + e) * plane_b);
    }

    // ---- D': M = window column q = 4 i + m (one 16-byte read gives a lane its four M-tiles), k-slot (step (mm, e), group ks) = tap
    //      16 mm + 4 ks + e with B = gO[c] * ggV[tap] from the tile registers; taps >= 51 have B = 0 and read window row 50 again
    if (GV && DH && dH) {
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* abase = inT + rowoff + 4 * j;
      // (the channel loops of this block stay rolled and fenced: unrolled, the scheduler hoists their 45 + 96 LDS reads over the T / T'
      // pass and the kernel spills)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const float gc = c == 0 ? g[0] : (c == 1 ? g[1] : g[2]);
#pragma unroll
        for (int s = 0; s < 15; ++s) {
          const int mm = s >> 2, e = s & 3;
          const f32x4 av = *reinterpret_cast<const f32x4*>(abase + c * LP + min(16 * mm + 4 * ks + e, K - 1) * MLW);
          const float bb = gc * w16[mm][e];
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bb, acc[m], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // Window columns 64 and 65 hold three entries of the band (q, p) = (64, 14), (64, 15), (65, 15): dot products on the VALU, each
      // lane over its own 16 taps and 3 channels, folded over the four lane groups of a pixel
      float p64 = 0.f, p65 = 0.f;
      {
        const float* col = inT + rowoff + 64;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
          const float gc = c == 0 ? g[0] : (c == 1 ? g[1] : g[2]);
          float s64 = 0.f, s65 = 0.f;
#pragma unroll
          for (int s = 0; s < 15; ++s) {
            const int mm = s >> 2, e = s & 3;
            const float* cp = col + c * LP + min(16 * mm + 4 * ks + e, K - 1) * MLW;
            s64 = fmaf(w16[mm][e], cp[0], s64);
            s65 = fmaf(w16[mm][e], cp[1], s65);
          }
          p64 = fmaf(gc, s64, p64);
          p65 = fmaf(gc, s65, p65);
        }
        __builtin_amdgcn_sched_barrier(0);
        p64 += __shfl_xor(p64, 16, 64); p64 += __shfl_xor(p64, 32, 64);
        p65 += __shfl_xor(p65, 16, 64); p65 += __shfl_xor(p65, 32, 64);
      }
      // accumulator (m, e) of lane (j, ks) is D'[q][j], q = 4 (4 ks + e) + m.  dH[fx][p] = D'[p + fx][p]: through the wave's dead tap
      // rows, so that a store instruction writes four 64-byte runs instead of 64 scattered dwords (csrc/sepconv.hip)
      __builtin_amdgcn_wave_barrier();
      float* tile = hB;                                      // [64 q][16 p] floats of the wave's 2 x 52 x 16
      static_assert(64 * 16 <= 2 * TAPROWS * 16, "transpose tile fits the tap rows");
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(16 * ks + 4 * e + m) * 16 + j] = acc[m][e];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < NREG; ++t) {
        const int fx = 4 * t + ks;
        const float val = tile[min(j + fx, 63) * 16 + j];
        bstore(val, hdst, (pvalid && fx < K && j + fx < 64) ? opix_b + (unsigned)ks * plane_b : OOR, (unsigned)(4 * t) * plane_b);
      }
      bstore(p64, hdst, (pvalid && lane == 14) ? opix_b : OOR, 50u * plane_b);
      bstore(p64, hdst, (pvalid && lane == 15) ? opix_b : OOR, 49u * plane_b);
      bstore(p65, hdst, (pvalid && lane == 15) ? opix_b : OOR, 50u * plane_b);
    }

    if (more) {
      // next row: v, ggV and gO into the registers this row is done with; h and ggH, fetched above, into the wave's LDS rows (the LDS
      // queue of a wave is in order: no workgroup barrier)
      const unsigned po = pix_off(y + 2);
      load_tile(v16, vsrc, plane_b, po, ks);
      if (GV) load_tile(w16, gvsrc, plane_b, po, ks);
#pragma unroll
      for (int c = 0; c < C; ++c) g[c] = bload(gsrc, po, (unsigned)c * plane_b);
      __builtin_amdgcn_wave_barrier();
      store_band<K, NREG>(hB, hreg, lane);
      if (GH) store_band<K, NREG>(gB, greg, lane);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Any K, any C: one thread per output pixel, one sequential sum per output element (cold path, kept for the op's full surface).
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ void sepconv_bwd2_direct(const float* __restrict__ in, const float* __restrict__ v, const float* __restrict__ h,
                                    const float* __restrict__ gO, const float* __restrict__ ggV, const float* __restrict__ ggH,
                                    float* __restrict__ d_gO, float* __restrict__ dV, float* __restrict__ dH, int C, int Ho, int Wo,
                                    int K) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= Wo) return;
  const size_t plane = (size_t)Ho * Wo, pix = (size_t)y * Wo + x;
  const size_t Wi = (size_t)Wo + K - 1, iplane = ((size_t)Ho + K - 1) * Wi;
  const size_t tb = (size_t)b * K * plane + pix, ob = (size_t)b * C * plane + pix;
  const float* win = in + (size_t)b * C * iplane + (size_t)y * Wi + x;       // W[c][i][j] = win[c * iplane + i * Wi + j]
  if (d_gO) {
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
      for (int i = 0; i < K; ++i) {
        const float* row = win + c * iplane + i * Wi;
        float t = 0.f, tp = 0.f;
        for (int j = 0; j < K; ++j) {
          const float a = row[j];
          if (ggV) t = fmaf(a, h[tb + j * plane], t);
          if (ggH) tp = fmaf(a, ggH[tb + j * plane], tp);
        }
        if (ggV) acc = fmaf(ggV[tb + i * plane], t, acc);
        if (ggH) acc = fmaf(v[tb + i * plane], tp, acc);
      }
      d_gO[ob + c * plane] = acc;
    }
  }
  if (dV) {
    for (int i = 0; i < K; ++i) {
      float acc = 0.f;
      for (int c = 0; c < C; ++c) {
        const float* row = win + c * iplane + i * Wi;
        float tp = 0.f;
        for (int j = 0; j < K; ++j) tp = fmaf(row[j], ggH[tb + j * plane], tp);
        acc = fmaf(gO[ob + c * plane], tp, acc);
      }
      dV[tb + i * plane] = acc;
    }
  }
  if (dH) {
    for (int j = 0; j < K; ++j) {
      float acc = 0.f;
      for (int c = 0; c < C; ++c) {
        const float* col = win + c * iplane + j;
        float d = 0.f;
        for (int i = 0; i < K; ++i) d = fmaf(col[i * Wi], ggV[tb + i * plane], d);
        acc = fmaf(gO[ob + c * plane], d, acc);
      }
      dH[tb + j * plane] = acc;
    }
  }
}

constexpr size_t mfma_lds_bytes(int rows) {
  return ((size_t)3 * (rows + KFAST - 1) * MLW + (size_t)(MNT / 64) * 2 * TAPROWS * 16) * sizeof(float);
}

// rows per workgroup (one workgroup per CU: the window fills most of its LDS): as few rounds of the 256 CUs as possible, each costing
// its rows plus the staging of the 50-row halo (the rule of the tiled first-order kernels that HISTORY.md records; the row here is ~3x as long, the halo counts for less)
int bwd2_rows(int B, int Ho, int Wo) {
  int best = 8;
  long best_cost = -1;
  for (int r : {8, 16}) {
    const long wgs = (long)B * savfi_cdiv(Wo, MC) * savfi_cdiv(Ho, r);
    const long cost = ((wgs + 255) / 256) * (r + 1);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = r; }
  }
  return best;
}

template <int R, bool GV, bool GH, bool DH>
int launch_one(const float* in, const float* v, const float* h, const float* gO, const float* ggV, const float* ggH, float* d_gO,
               float* dV, float* dH, int B, int Ho, int Wo, hipStream_t st) {
  constexpr size_t lds = mfma_lds_bytes(R);
  static_assert(lds <= 160 * 1024, "LDS per CU");
  static uint32_t done = 0;
  if (int e = savfi_ensure_dynamic_lds((const void*)sepconv_bwd2_mfma<KFAST, R, GV, GH, DH>, lds, done)) return e;
  dim3 grid(savfi_cdiv(Wo, MC), savfi_cdiv(Ho, R), B);
  hipLaunchKernelGGL((sepconv_bwd2_mfma<KFAST, R, GV, GH, DH>), grid, dim3(MNT), lds, st, in, v, h, gO, ggV, ggH, d_gO, dV, dH, Ho, Wo);
  return savfi_launch_status();
}

template <int R>
int launch_rows(const float* in, const float* v, const float* h, const float* gO, const float* ggV, const float* ggH, float* d_gO,
                float* dV, float* dH, int B, int Ho, int Wo, hipStream_t st) {
  if (ggV && ggH) {
    if (dH) return launch_one<R, true, true, true>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
    return launch_one<R, true, true, false>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
  }
  if (ggV) {
    if (dH) return launch_one<R, true, false, true>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
    return launch_one<R, true, false, false>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
  }
  return launch_one<R, false, true, false>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
}

}  // namespace

extern "C" int savfi_sepconv_bwd2_f32(const float* in, const float* v, const float* h, const float* gO, const float* ggV,
                                      const float* ggH, float* d_gO, float* dV, float* dH, int B, int C, int Ho, int Wo, int K,
                                      void* stream) {
  // NULL: the four operands; a cotangent and an output at least; an output whose only term needs an absent cotangent
  if (!in || !v || !h || !gO) return SAVFI_E_NULL;
  if (!ggV && !ggH) return SAVFI_E_NULL;
  if (!d_gO && !dV && !dH) return SAVFI_E_NULL;
  if ((dH && !ggV) || (dV && !ggH)) return SAVFI_E_NULL;
  // SHAPE
  if (B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || K <= 0) return SAVFI_E_SHAPE;
  // UNSUPPORTED: an output that is one of the operands or another output (every output element is written while its neighbours'
  // operands are still being read), or a pointer that is not a float's
  {
    const void* ins[6] = {in, v, h, gO, ggV, ggH};
    const void* outs[3] = {d_gO, dV, dH};
    for (int a = 0; a < 3; ++a) {
      if (!outs[a]) continue;
      for (int i = 0; i < 6; ++i)
        if (outs[a] == ins[i]) return SAVFI_E_UNSUPPORTED;
      for (int o = a + 1; o < 3; ++o)
        if (outs[a] == outs[o]) return SAVFI_E_UNSUPPORTED;
    }
    for (const void* p : ins)
      if ((uintptr_t)p & 3) return SAVFI_E_UNSUPPORTED;
    for (const void* p : outs)
      if ((uintptr_t)p & 3) return SAVFI_E_UNSUPPORTED;
  }
  // TOOBIG: the limits of savfi_sepconv_bwd_f32
  // (the small limits first: behind them the element counts fit 64 bits for any int arguments)
  const int64_t Hi = (int64_t)Ho + K - 1, Wi = (int64_t)Wo + K - 1;
  if ((int64_t)B * K > 65535 || (int64_t)B * C > 65535 || Hi > 65535 || Wi >= (int64_t)1 << 31) return SAVFI_E_TOOBIG;
  if ((int64_t)B * K * Ho * Wo >= (int64_t)1 << 40 || (int64_t)B * C * Hi * Wi >= (int64_t)1 << 40) return SAVFI_E_TOOBIG;

  hipStream_t st = (hipStream_t)stream;
  // the MFMA kernel addresses one sample's tap planes, and one plane of the frames, through 32-bit buffer offsets
  const bool fits = (int64_t)KFAST * Ho * Wo * 4 < ((int64_t)1 << 31) && Hi * Wi * 4 < ((int64_t)1 << 31);
  if (K == KFAST && C == 3 && fits) {
    if (bwd2_rows(B, Ho, Wo) == 16) return launch_rows<16>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
    return launch_rows<8>(in, v, h, gO, ggV, ggH, d_gO, dV, dH, B, Ho, Wo, st);
  }
  dim3 grid(savfi_cdiv(Wo, 64), Ho, B);
  hipLaunchKernelGGL(sepconv_bwd2_direct, grid, dim3(64), 0, st, in, v, h, gO, ggV, ggH, d_gO, dV, dH, C, Ho, Wo, K);
  return savfi_launch_status();
}
