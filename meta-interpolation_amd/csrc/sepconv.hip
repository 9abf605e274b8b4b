// Separable local convolution (SepConv) for gfx950 -- forward, filter gradients, input gradient.
//
// Replaces the four cupy/NVRTC kernels of the reference
// (sepconv/sepconv_op/sepconv.py:5-30, :32-63, :138-163, :165-190).
//
//   out[b,c,y,x] = sum_fy sum_fx in[b,c,y+fy,x+fx] * v[b,fy,y,x] * h[b,fx,y,x]
//
// Layout: fp32 NCHW, contiguous.  in [B,C,Ho+K-1,Wo+K-1], v/h [B,K,Ho,Wo], out/gO [B,C,Ho,Wo].
//
// K = 51, C = 3 (the only shape the model uses) runs on persistent matrix-core kernels, one workgroup per CU: the forward and the
// pair (gV, gH) on the split-bf16 kernels of csrc/sepconv_ws.hip (widths that are a multiple of 4) and csrc/sepconv_x6.hip (other
// widths), a single filter gradient on sepconv_bwd_mfma_p below (exact-fp32 MFMA).  sepconv_route() at the end of this file is the
// one place that decides; a batch whose tensors do not fit one buffer descriptor is launched in chunks of consecutive samples.
// Every other (K, C), and a single sample that does not fit, takes the generic direct kernels (one thread per output element;
// cold path, kept for the op's full surface).  The input gradient is always the direct kernel.
// Earlier generations (VALU kernels; the tiled fp32-MFMA kernels sepconv_fwd_mfma / sepconv_bwd_mfma) were removed; HISTORY.md
// keeps their structure and numbers.
#include "common.h"
#include <stdlib.h>

// Compile-time experiment switch (on in the shipped library; profiles/r02_sepconv_variants.txt has the A/B numbers):
//   SC_PIN     pin the LDS-read / MFMA interleave with sched_group_barrier (software-pipelined A fragments)
#ifndef SC_PIN
#define SC_PIN 1
#endif

namespace {

constexpr int KFAST = 51;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// geometry of the fp32-MFMA kernel: 8 waves = 2 row lanes x 4 column groups of 16 pixels work on a phase of 2 output rows x MC
// columns; the input window is MSPAN = 64 + 50 (+ 2) columns wide in LDS rows of pitch MLW (16-byte aligned A fragments)
constexpr int MC = 64, MLW = 132, MSPAN = 116, MNT = 512;
constexpr int MKP = 52;   // rows per channel in the M dimension (51 taps + 1 zero row): lanes never straddle channels

// Tap rows are PRIVATE to a wave: wave (wr, wc) needs h / v of its own 16 pixels only ([K][16] floats = 64-byte
// runs per tap plane).  Keeping them private removes every workgroup barrier from the row loop, so the two waves
// that share a SIMD drift out of phase and one's VALU / LDS / store phases hide under the other's MFMAs.
// lane = (tap group tg = lane >> 4, column j = lane & 15); NREG = ceil(K / 4) dwords per lane.
// Raw buffer loads: one resource per tensor, a per-lane byte offset (sample + tap group + pixel) computed once per row and a
// wave-uniform byte offset per tap quadruple -- no 64-bit per-load addresses on the VALU.  Tap 51 of the last quadruple is the
// next sample's tap 0 (or past num_records: 0); mfma_store_taps replaces it by the zero tap row.
__device__ __forceinline__ float sc_bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
// store with the same addressing; a lane whose offset is >= num_records (SC_OOR) writes nothing: predication without a branch,
// so a row's stores are a FIXED number of memory instructions and the compiler can count vmcnt for the loads around them
constexpr unsigned SC_OOR = 0x80000000u;
__device__ __forceinline__ void sc_bstore(float val, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sc_rsrc(const float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
template <int K, int NREG>
__device__ __forceinline__ void mfma_store_taps(float* __restrict__ dst /* [>=K][16] */, const float (&regs)[NREG],
                                                int lane) {
  // Branch-free: row K (one past the last tap) is written with zeros.  For the h rows that is row 0 of the v rows right behind
  // them, which the v copy that always follows overwrites; for the v rows it is the zero tap row itself.  (A lane-predicated
  // write made the compiler wait for vmcnt(0) -- every outstanding gradient store -- in front of the last quadruple.)
#pragma unroll
  for (int it = 0; it < NREG; ++it) {
    const int tap = 4 * it + (lane >> 4);
    if (4 * it + 3 < K) dst[tap * 16 + (lane & 15)] = regs[it];
    else dst[min(tap, K) * 16 + (lane & 15)] = tap < K ? regs[it] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// Filter gradients on the exact-fp32 matrix cores, persistent (sepconv_bwd_mfma_p): what runs when only one of gV / gH is wanted.
//
// For the 16 pixels p of one output row (y, x0 .. x0 + 15) the horizontal pass is a banded GEMM over the 66 window columns q:
//     Hb[q][p] = h[q - p][y][x0 + p]  (0 <= q - p < 51, else 0)       -- a "Toeplitz with per-pixel taps" B operand
// and the two gradients are banded GEMMs that share the staged input window In, with the upstream gradient folded into B so
// that the accumulators ARE the results (no cross-lane reduction):
//     gV[fy,p] = sum_{c,q}  In[c][y+fy][x0+q] * (gO[c,p] * Hb[q][p])            M = fy (51 -> 64), K = 3 * 68:  204 MFMA
//     D'[q,p]  = sum_{c,fy} In[c][y+fy][x0+q] * (gO[c,p] * v[fy,p])             M = q (64 of 66),  K = 3 * 52:  156 MFMA
//     gH[fx,p] = D'[p+fx, p]                                                    (the band of D')
// v_mfma_f32_16x16x4_f32 is bit for bit an fp32 fmaf chain at the fp32 VALU rate, but needs one LDS dword per 1024 FMA.
//   * gV: the order in which window columns go to the MFMA k-slots is free as long as A and B agree.  Slot (step t, lane group ks)
//     takes q = 16 (t / 4) + 4 ks + t % 4 for t < 16 and q = 64 + ks for t = 16, so a lane's 16 A values of an M-tile are four
//     aligned 16-byte LDS reads (+ one dword); the next group's A fragments are in flight while this group's MFMAs issue.  Left
//     alone the compiler sinks every LDS read to just before its first use: the schedule is pinned (SC_PIN).
//   * gH: M index q = 4 i + m puts the four M-tiles' A values of a lane (i = j) into ONE 16-byte LDS read per step, fetched two
//     steps ahead.  Of the fifth M-tile (q = 64 .. 79) only (q, j) = (64, 14), (64, 15), (65, 15) lie inside the band: three
//     153-term dot products on the VALU instead of 39 more MFMAs per row.  Straight from the accumulators every lane of a store
//     would hit a different tap plane; the wave's tap rows are dead by then, so the 64 x 16 tile goes through them (an LDS
//     transpose) and leaves as 13 instructions of four 64-byte runs.
//   * The two waves of a SIMD (row lanes wr = 0 / 1) run identical instruction streams and would stay in lockstep, both in their
//     VALU / LDS / store phases and then both competing for the matrix pipe: a one-off s_sleep head start for one of them lets
//     each wave's non-MFMA work hide under the other's MFMAs.
//
// The launch has ONE workgroup per CU and the output is cut into "phases" (two output rows of one 64-column strip of one sample,
// the unit the 2 x 4 waves process), numbered strip-major; workgroup w takes the phases [w Q, (w + 1) Q): equal shares, no partly
// filled last round and no per-tile staging prologue.  Consecutive phases of a strip slide down by two rows, so the input window
// lives in a CIRCULAR buffer of 64 rows per channel (slot = input row & 63): a phase reads rows 2 ph .. 2 ph + 51, twelve further
// rows are staged every sixth phase (two barriers), the full 64 only when a workgroup enters a strip.
// ------------------------------------------------------------------------------------------
constexpr int PWIN = 64;                       // window rows per channel (power of two >= K + 1)
// the piece [g0, g1) of the strip-major phase list (phases of 2 rows, strips of MC columns) that workgroup `block` of the persistent
// kernel takes: per_wg consecutive phases.  The kernel and savfi_sepconv_partition() evaluate the same function.
__host__ __device__ __forceinline__ void persistent_work_range(int total, int per_wg, int block, int& g0, int& g1) {
  g0 = block * per_wg;
  g1 = g0 + per_wg < total ? g0 + per_wg : total;
}
constexpr int PAHEAD = PWIN - (KFAST + 1);     // rows staged per refill (12)

// rows [r_lo, r_lo + nrows) of the strip (b, x0) -> their circular slots, all three channels; thread -> (column, row group).
// Two halves so that the slide (twelve rows every sixth phase) can be in flight for a whole phase: loads -> registers, then,
// behind a barrier, registers -> LDS.
template <int NROWS>
struct StagedRows {
  static constexpr int C = 3, RG = MNT / 128, NIT = (NROWS + RG - 1) / RG;
  float buf[C][NIT];
};
template <int NROWS>
__device__ __forceinline__ void stage_rows_load(StagedRows<NROWS>& sr, __amdgpu_buffer_rsrc_t in_rs, int b, int x0, int r_lo,
                                                int Hi, int Wi, int tid) {
  constexpr int C = 3, RG = MNT / 128, NIT = StagedRows<NROWS>::NIT;
  const int q = tid & 127, rg = tid >> 7;
  const int colb = min(x0 + q, Wi - 1) * 4;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int r = min(r_lo + rg + it * RG, Hi - 1);
      sr.buf[c][it] = sc_bload(in_rs, (unsigned)(((b * C + c) * Hi + r) * Wi * 4 + colb), 0u);
    }
}
template <int NROWS>
__device__ __forceinline__ void stage_rows_write(const StagedRows<NROWS>& sr, float* __restrict__ inT, int r_lo, int tid) {
  constexpr int C = 3, RG = MNT / 128, NIT = StagedRows<NROWS>::NIT, LP = PWIN * MLW;
  const int q = tid & 127, rg = tid >> 7;
  // branch-free: all 128 columns are written.  Columns MSPAN .. 127 of a window row are only read by gH rows that are
  // discarded (they must merely stay finite, and image data is), and no lane skips the reads of its staging registers -- a
  // skipped lane leaves its loads "possibly in flight" for the compiler, which then waits for vmcnt(0) wherever those
  // registers are reused.
  static_assert(128 <= MLW, "staged columns fit a window row");
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int rr = rg + it * RG;
      if (rr < NROWS) inT[c * LP + ((r_lo + rr) & (PWIN - 1)) * MLW + q] = sr.buf[c][it];
    }
}
template <int NROWS>
__device__ __forceinline__ void stage_rows_circular(float* __restrict__ inT, __amdgpu_buffer_rsrc_t in_rs, int b, int x0, int r_lo,
                                                    int Hi, int Wi, int tid) {
  StagedRows<NROWS> sr;
  stage_rows_load<NROWS>(sr, in_rs, b, x0, r_lo, Hi, Wi, tid);
  stage_rows_write<NROWS>(sr, inT, r_lo, tid);
}

template <int K, bool WANT_V, bool WANT_H>
__global__ __launch_bounds__(MNT) void sepconv_bwd_mfma_p(const float* __restrict__ in, const float* __restrict__ v,
                                                         const float* __restrict__ h, const float* __restrict__ gO,
                                                         float* __restrict__ gV, float* __restrict__ gH,
                                                         int B, int Ho, int Wo, int nph, int ncol, int per_wg) {
  constexpr int C = 3, LP = PWIN * MLW;
  constexpr int KT = (16 + K - 1 + 3) / 4, MTV = (K + 15) / 16, KTV = (K + 3) / 4, MTH = (16 + K - 1 + 15) / 16, NREG = (K + 3) / 4;
  static_assert(KT == 17 && MTV == 4 && MLW % 4 == 0 && 4 * KTV == MKP && 16 * 3 + 16 * MTH <= MLW && K + 1 <= PWIN, "operand geometry");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* inT = lds;
  float* hB = lds + C * LP + (threadIdx.x >> 6) * (K + MKP) * 16;
  float* vB = hB + K * 16;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wc = w & 3, wr = w >> 2;
  const int j = lane & 15, ks = lane >> 4;
  const int total = B * ncol * nph;
  int g0, g1;
  persistent_work_range(total, per_wg, (int)blockIdx.x, g0, g1);
  if (g0 >= g1) return;
  const int Hi = Ho + K - 1, Wi = Wo + K - 1;
  const size_t plane = (size_t)Ho * Wo;
  const unsigned plane_b = (unsigned)plane * 4u;
  // whole-tensor resources (the launcher checks that they fit 2^31 bytes); the sample goes into the per-lane offset
  const __amdgpu_buffer_rsrc_t hsrc = sc_rsrc(h, (unsigned)(B * K) * plane_b);
  const __amdgpu_buffer_rsrc_t vsrc = sc_rsrc(v, (unsigned)(B * K) * plane_b);
  const __amdgpu_buffer_rsrc_t gsrc = sc_rsrc(gO, (unsigned)(B * C) * plane_b);
  const __amdgpu_buffer_rsrc_t isrc = sc_rsrc(in, (unsigned)(B * C) * (unsigned)(Hi * Wi) * 4u);
  const __amdgpu_buffer_rsrc_t gvdst = sc_rsrc(gV, WANT_V ? (unsigned)(B * K) * plane_b : 0u);
  const __amdgpu_buffer_rsrc_t ghdst = sc_rsrc(gH, WANT_H ? (unsigned)(B * K) * plane_b : 0u);

  auto pos_of = [&](int g, int& b, int& x0, int& ph) {
    const int s = g / nph;
    ph = g - s * nph;
    b = s / ncol;
    x0 = (s - b * ncol) * MC;
  };
  // byte offset of this lane's pixel (row y of sample b, clamped) inside a [B][*][Ho][Wo] tensor with `ch` planes per sample
  auto pix_off = [&](int b, int x0, int y, int ch) {
    return (unsigned)b * (unsigned)ch * plane_b + (unsigned)(min(y, Ho - 1) * Wo + min(x0 + 16 * wc + j, Wo - 1)) * 4u;
  };
  auto load_taps = [&](float (&regs)[NREG], __amdgpu_buffer_rsrc_t src, int b, int x0, int y) {
    const unsigned voff = pix_off(b, x0, y, K) + (unsigned)(lane >> 4) * plane_b;
#pragma unroll
    for (int it = 0; it < NREG; ++it) regs[it] = sc_bload(src, voff, (unsigned)(4 * it) * plane_b);
  };

  int b, x0, ph;
  pos_of(g0, b, x0, ph);
  float hreg[NREG], vreg[NREG], gnext[C];
  load_taps(hreg, hsrc, b, x0, 2 * ph + wr);
  load_taps(vreg, vsrc, b, x0, 2 * ph + wr);
  {
    const unsigned go = pix_off(b, x0, 2 * ph + wr, C);
#pragma unroll
    for (int c = 0; c < C; ++c) gnext[c] = sc_bload(gsrc, go, (unsigned)c * plane_b);
  }
  stage_rows_circular<PWIN>(inT, isrc, b, x0, 2 * ph, Hi, Wi, tid);
  int loaded_hi = 2 * ph + PWIN;
  // columns MSPAN..MLW-1 are only read by gH rows q >= 66, which are discarded, but keep them finite (never restaged)
  static_assert(MLW - MSPAN == 16, "zero-fill indexing");
  for (int i = tid; i < C * PWIN * 16; i += MNT) inT[(i >> 4) * MLW + MSPAN + (i & 15)] = 0.f;
  if (lane < 16) vB[K * 16 + lane] = 0.f;
  mfma_store_taps<K, NREG>(hB, hreg, lane);
  mfma_store_taps<K, NREG>(vB, vreg, lane);
  __syncthreads();
  if (wr == 1) __builtin_amdgcn_s_sleep(40);      // de-phase the two waves of a SIMD (see the comment above)

#pragma unroll 1
  for (int g = g0; g < g1; ++g) {
    // ---- window upkeep (workgroup-uniform decisions) ------------------------------------------------------------
    if (g != g0 && ph == 0) {                      // entered the next strip: the whole window is new
      __syncthreads();
#pragma unroll 1
      for (int r = 0; r < PWIN; r += 16)           // in four pieces: 12 staging registers instead of 48 (rare path)
        stage_rows_circular<16>(inT, isrc, b, x0, r, Hi, Wi, tid);
      loaded_hi = PWIN;
      __syncthreads();
    }
    // next phase (position and whether it needs the window slid by twelve rows first)
    int nb, nx0, nph_;
    pos_of(min(g + 1, g1 - 1), nb, nx0, nph_);
    const bool slide = (g + 1 < g1) && nph_ != 0 && (2 * nph_ + K + 1 > loaded_hi);
    // The slide's rows travel HBM -> registers during this phase and registers -> LDS behind the barrier at its end: issued
    // first, they are older than the tap prefetch, so the exact vmcnt wait of the tap copy covers them and nobody waits for
    // memory with the matrix pipe idle (before: two barriers around a load + wait, every sixth phase, with all eight waves idle).
    StagedRows<PAHEAD> slid;
    if (slide) stage_rows_load<PAHEAD>(slid, isrc, b, x0, loaded_hi, Hi, Wi, tid);
    const int y = 2 * ph + wr;
    const int x = x0 + 16 * wc + j;
    const bool pvalid = (x < Wo) && (y < Ho);
    // byte offset of this lane's pixel in tap plane 0 of sample b (gV / gH are [B][K][Ho][Wo]); out of range = no store
    const unsigned opix_b = (unsigned)b * (unsigned)K * plane_b + (unsigned)(min(y, Ho - 1) * Wo + min(x, Wo - 1)) * 4u;
    float g_[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g_[c] = gnext[c];
    // next phase's taps and upstream gradient: HBM -> registers.  Unconditional (the last phase re-reads itself), and the
    // stores below are a fixed number of instructions, so the wait in front of the LDS copy at the end of the phase is an
    // exact vmcnt(#stores) -- not a wait for every store's write acknowledge.
    load_taps(hreg, hsrc, nb, nx0, 2 * nph_ + wr);
    load_taps(vreg, vsrc, nb, nx0, 2 * nph_ + wr);
    {
      const unsigned go = pix_off(nb, nx0, 2 * nph_ + wr, C);
#pragma unroll
      for (int c = 0; c < C; ++c) gnext[c] = sc_bload(gsrc, go, (unsigned)c * plane_b);
    }
    const float* hb = hB + j;
    const float* vb = vB + j;

    if (WANT_V) {
      float bf[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const int q = (t < 16) ? (16 * (t >> 2) + 4 * ks + (t & 3)) : (64 + ks);
        const int tap = q - j;
        const float val = hb[min(max(tap, 0), K - 1) * 16];
        bf[t] = (tap >= 0 && tap < K) ? val : 0.f;
      }
      // A rows: tap fy = 16 m + j (clamped) of this wave's output row -> input row y + fy -> its circular slot
      int abV[MTV];
#pragma unroll
      for (int m = 0; m < MTV; ++m) abV[m] = ((y + min(16 * m + j, K - 1)) & (PWIN - 1)) * MLW + 16 * wc + 4 * ks;
      f32x4 acc[MTV];
#pragma unroll
      for (int m = 0; m < MTV; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      constexpr int NG = C * 5;
      auto load_group = [&](f32x4 (&dst)[MTV], int gi) {
        const int c = gi / 5, u = gi - 5 * c;
#pragma unroll
        for (int m = 0; m < MTV; ++m) {
          const float* ap = inT + abV[m] + c * LP;
          if (u < 4) dst[m] = *reinterpret_cast<const f32x4*>(ap + 16 * u);
          else dst[m][0] = ap[64 - 3 * ks];
        }
      };
      f32x4 acur[MTV], anxt[MTV];
#if SC_PIN
      __builtin_amdgcn_sched_barrier(0);
#endif
      load_group(acur, 0);
#if SC_PIN
      __builtin_amdgcn_sched_group_barrier(0x100, MTV, 0);
#endif
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        if (gi + 1 < NG) load_group(anxt, gi + 1);
        const int c = gi / 5, u = gi - 5 * c;
#pragma unroll
        for (int e = 0; e < (u < 4 ? 4 : 1); ++e) {
          const float bb = g_[c] * bf[u < 4 ? 4 * u + e : 16];
#pragma unroll
          for (int m = 0; m < MTV; ++m)
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(acur[m][e], bb, acc[m], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < MTV; ++m) acur[m] = anxt[m];
#if SC_PIN
        if (gi + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, MTV, 0);
        if (u < 4) {
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4 * MTV, 0);
        } else {
          __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, MTV, 0);
        }
#endif
      }
#if SC_PIN
      __builtin_amdgcn_sched_barrier(0);
#endif
      {   // fy = 16 m + 4 ks + e: all real for m < 3; for m = 3 only ks = 0, e < 3 (fy = 48, 49, 50)
        static_assert(K == 51 && MTV == 4, "gV store predication");
        const unsigned vo = opix_b + (unsigned)(4 * ks) * plane_b;
        const unsigned voA = pvalid ? vo : SC_OOR, voB = (pvalid && ks == 0) ? vo : SC_OOR;
#pragma unroll
        for (int m = 0; m < MTV; ++m)
#pragma unroll
          for (int e = 0; e < (m < 3 ? 4 : 3); ++e) sc_bstore(acc[m][e], gvdst, m < 3 ? voA : voB, (unsigned)(16 * m + e) * plane_b);
      }
    }

    if (WANT_H) {
      constexpr int MTHM = MTH - 1;
      static_assert(K == 51 && 16 * MTHM == 64, "band geometry of the VALU tail");
      float bv[KTV];
#pragma unroll
      for (int t = 0; t < KTV; ++t) bv[t] = vb[(4 * t + ks) * 16];
      f32x4 acc[MTHM];
#pragma unroll
      for (int m = 0; m < MTHM; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // step (c, t) reads input row y + 4 t + ks (tap 4t + ks; the zero tap 51 steps back one row): slot (s0 + 4 t) & 63.
      // The 13 rows span 48 < 64 slots, so they wrap at most once: two bases, picked per step by a compare.
      const int s0 = (y + ks) & (PWIN - 1);
      const float* pA = inT + s0 * MLW + 16 * wc + 4 * j;
      const float* pB = pA - PWIN * MLW;
      const int s0l = (y + 4 * (KTV - 1) + ks - (ks == 3 ? 1 : 0)) & (PWIN - 1);      // last step's row
      const float* pL = inT + s0l * MLW + 16 * wc + 4 * j;
      auto a_of = [&](int idx) {
        const int c = idx / KTV, t = idx - KTV * c;
        const float* p = (t == KTV - 1) ? pL : ((s0 + 4 * t >= PWIN) ? pB : pA) + 4 * t * MLW;
        return *reinterpret_cast<const f32x4*>(p + c * LP);
      };
      constexpr int NS = C * KTV;
#if SC_PIN
      __builtin_amdgcn_sched_barrier(0);
#endif
      f32x4 a0 = a_of(0), a1 = a_of(1);
#if SC_PIN
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#endif
#pragma unroll
      for (int idx = 0; idx < NS; ++idx) {
        f32x4 a2 = a0;
        if (idx + 2 < NS) a2 = a_of(idx + 2);
        const int c = idx / KTV, t = idx - KTV * c;
        const float bb = g_[c] * bv[t];
#pragma unroll
        for (int m = 0; m < MTHM; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m], bb, acc[m], 0, 0, 0);
        a0 = a1;
        a1 = a2;
#if SC_PIN
        if (idx + 2 < NS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, MTHM, 0);
#endif
      }
#if SC_PIN
      __builtin_amdgcn_sched_barrier(0);
#endif
      // VALU tail (q = 64, 65): lane = tap row fy, then a 64-lane sum of the three partial products
      float s6414 = 0.f, s6415 = 0.f, s6515 = 0.f;
      {
        const int fy = min(lane, K - 1);
        const float live = lane < K ? 1.f : 0.f;
        const float v14 = vB[fy * 16 + 14] * live, v15 = vB[fy * 16 + 15] * live;
        const float* col = inT + ((y + fy) & (PWIN - 1)) * MLW + 16 * wc + 64;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float a64 = col[c * LP], a65 = col[c * LP + 1];
          const float g14 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g_[c]), 14));
          const float g15 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g_[c]), 15));
          s6414 = fmaf(g14 * v14, a64, s6414);
          s6415 = fmaf(g15 * v15, a64, s6415);
          s6515 = fmaf(g15 * v15, a65, s6515);
        }
        s6414 = wave_sum(s6414);
        s6415 = wave_sum(s6415);
        s6515 = wave_sum(s6515);
      }
      {   // gH through an LDS transpose of the wave's (dead) tap rows: 13 x four 64-byte runs
        __builtin_amdgcn_wave_barrier();
        float* tile = hB;
#pragma unroll
        for (int m = 0; m < MTHM; ++m)
#pragma unroll
          for (int e = 0; e < 4; ++e) tile[(16 * ks + 4 * e + m) * 16 + j] = acc[m][e];
        __builtin_amdgcn_wave_barrier();
        const unsigned ho = opix_b + (unsigned)ks * plane_b;
#pragma unroll
        for (int t = 0; t < KTV; ++t) {
          const int fx = 4 * t + ks;
          const float val = tile[min(j + fx, 63) * 16 + j];
          sc_bstore(val, ghdst, (pvalid && fx < K && j + fx < 64) ? ho : SC_OOR, (unsigned)(4 * t) * plane_b);
        }
        __builtin_amdgcn_wave_barrier();
      }
      sc_bstore(s6414, ghdst, (pvalid && lane == 14) ? opix_b : SC_OOR, 50u * plane_b);
      sc_bstore(s6415, ghdst, (pvalid && lane == 15) ? opix_b : SC_OOR, 49u * plane_b);
      sc_bstore(s6515, ghdst, (pvalid && lane == 15) ? opix_b : SC_OOR, 50u * plane_b);
    }

    __builtin_amdgcn_wave_barrier();
    mfma_store_taps<K, NREG>(hB, hreg, lane);
    mfma_store_taps<K, NREG>(vB, vreg, lane);
    __builtin_amdgcn_wave_barrier();
    if (slide) {                                   // the twelve oldest rows are behind every wave's next phase
      __syncthreads();
      stage_rows_write<PAHEAD>(slid, inT, loaded_hi, tid);
      loaded_hi += PAHEAD;
      __syncthreads();
    }
    b = nb; x0 = nx0; ph = nph_;
  }
}

// ------------------------------------------------------------------------------------------
// generic direct kernels (any K, any C): one thread per output element, x fastest.
// ------------------------------------------------------------------------------------------
__global__ void sepconv_fwd_direct(const float* __restrict__ in, const float* __restrict__ v,
                                   const float* __restrict__ h, float* __restrict__ out, int C, int Ho,
                                   int Wo, int K) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int bc = blockIdx.z, b = bc / C;
  if (x >= Wo) return;
  const int Hi = Ho + K - 1, Wi = Wo + K - 1;
  const size_t plane = (size_t)Ho * Wo;
  const size_t pix = (size_t)b * K * plane + (size_t)y * Wo + x;
  const float* src = in + (size_t)bc * Hi * Wi + (size_t)y * Wi + x;
  float acc = 0.f;
  for (int fy = 0; fy < K; ++fy) {
    float t = 0.f;
    for (int fx = 0; fx < K; ++fx) t = fmaf(src[(size_t)fy * Wi + fx], h[pix + fx * plane], t);
    acc = fmaf(v[pix + fy * plane], t, acc);
  }
  out[(size_t)bc * plane + (size_t)y * Wo + x] = acc;
}

// which = 0: gV[b,f,y,x] = sum_c gO * sum_fx in[y+f][x+fx]*h[fx]
// which = 1: gH[b,f,y,x] = sum_c gO * sum_fy in[y+fy][x+f]*v[fy]
__global__ void sepconv_bwd_filter_direct(const float* __restrict__ in, const float* __restrict__ other,
                                          const float* __restrict__ gO, float* __restrict__ gF, int C,
                                          int Ho, int Wo, int K, int which) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int bf = blockIdx.z, b = bf / K, f = bf - b * K;
  if (x >= Wo) return;
  const int Hi = Ho + K - 1, Wi = Wo + K - 1;
  const size_t plane = (size_t)Ho * Wo;
  const size_t opix = (size_t)y * Wo + x;
  const size_t pix = (size_t)b * K * plane + opix;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* src = in + ((size_t)b * C + c) * Hi * Wi;
    float t = 0.f;
    if (which == 0) {
      for (int fx = 0; fx < K; ++fx) t = fmaf(src[(size_t)(y + f) * Wi + x + fx], other[pix + fx * plane], t);
    } else {
      for (int fy = 0; fy < K; ++fy) t = fmaf(src[(size_t)(y + fy) * Wi + x + f], other[pix + fy * plane], t);
    }
    acc = fmaf(gO[((size_t)b * C + c) * plane + opix], t, acc);
  }
  gF[pix + f * plane] = acc;
}

// gI[b,c,Y,X] = sum over (fy,fx) with 0 <= Y-fy < Ho, 0 <= X-fx < Wo of
//               gO[b,c,Y-fy,X-fx] * v[b,fy,Y-fy,X-fx] * h[b,fx,Y-fy,X-fx]
// (exact adjoint of the forward; the reference kernel tests `> max` instead of `>= max`,
//  sepconv.py:51,54, and reads one row/column past the end).
__global__ void sepconv_bwd_input_direct(const float* __restrict__ v, const float* __restrict__ h,
                                         const float* __restrict__ gO, float* __restrict__ gI, int C,
                                         int Ho, int Wo, int K) {
  const int Hi = Ho + K - 1, Wi = Wo + K - 1;
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  const int Y = blockIdx.y;
  const int bc = blockIdx.z, b = bc / C;
  if (X >= Wi) return;
  const size_t plane = (size_t)Ho * Wo;
  const float* g = gO + (size_t)bc * plane;
  const float* vb = v + (size_t)b * K * plane;
  const float* hb = h + (size_t)b * K * plane;
  const int fy_lo = max(0, Y - (Ho - 1)), fy_hi = min(K - 1, Y);
  const int fx_lo = max(0, X - (Wo - 1)), fx_hi = min(K - 1, X);
  float acc = 0.f;
  for (int fy = fy_lo; fy <= fy_hi; ++fy) {
    const int y = Y - fy;
    for (int fx = fx_lo; fx <= fx_hi; ++fx) {
      const int x = X - fx;
      const size_t o = (size_t)y * Wo + x;
      acc = fmaf(g[o] * vb[fy * plane + o], hb[fx * plane + o], acc);
    }
  }
  gI[(size_t)bc * Hi * Wi + (size_t)Y * Wi + X] = acc;
}

constexpr size_t persistent_lds_bytes() {
  return ((size_t)3 * PWIN * MLW + (size_t)(MNT / 64) * (KFAST + MKP) * 16) * sizeof(float);
}

int debug_cus = 0;                             // savfi_sepconv_debug_cus: > 0 = the CU count the persistent launches plan for

int device_cu_count_real() {
  static int cus[32] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  int& n = cus[dev & 31];
  if (n == 0) {
    int v = 0;
    n = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return n;
}
// what the wave-specialised, the one-program-per-wave and the fp32 persistent launchers size their grids by
int device_cu_count() {
  const int n = device_cu_count_real();
  return debug_cus > 0 ? (debug_cus < n ? debug_cus : n) : n;
}

// The persistent kernels address every tensor of a launch through ONE raw buffer descriptor: byte offsets, and the out-of-range
// marker SC_OOR, need each tensor to stay below the span of 2^31 bytes (savfi_sepconv_debug_span_bytes: a smaller one, for tests).
constexpr int64_t SPAN_MAX = (int64_t)1 << 31;
int64_t span_bytes = SPAN_MAX;

// the largest Bc <= B whose tap tensors [Bc][51][Ho][Wo] and input windows [Bc][3][Ho + 50][Wo + 50] both stay below the span
// (0: not even one sample does).  Callers have bounded Ho * Wo (check_dims, savfi_sepconv_partition).
int persistent_chunk(int B, int Ho, int Wo) {
  const int64_t taps = (int64_t)KFAST * Ho * Wo * 4, win = 3 * ((int64_t)Ho + KFAST - 1) * ((int64_t)Wo + KFAST - 1) * 4;
  const int64_t fit = (span_bytes - 1) / (taps > win ? taps : win);
  return (int)(fit < B ? fit : B);
}
bool persistent_ok(int B, int Ho, int Wo) { return persistent_chunk(B, Ho, Wo) == B; }

// the launch geometry of the fp32 persistent kernel: phases per strip, strips per sample, phases per workgroup and the grid
int persistent_plan(int B, int Ho, int Wo, int cus, int& nph, int& ncol, int& per_wg) {
  nph = savfi_cdiv(Ho, 2);
  ncol = savfi_cdiv(Wo, MC);
  const int64_t total = (int64_t)B * ncol * nph;
  per_wg = savfi_cdiv(total, cus);
  return savfi_cdiv(total, per_wg);
}

template <bool WV, bool WH>
int launch_bwd_persistent_one(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH, int B,
                              int Ho, int Wo, hipStream_t st) {
  constexpr size_t lds = persistent_lds_bytes();
  static_assert(lds <= 160 * 1024, "LDS per CU");
  static uint32_t done = 0;
  if (int e = savfi_ensure_dynamic_lds((const void*)sepconv_bwd_mfma_p<KFAST, WV, WH>, lds, done)) return e;
  int nph, ncol, per_wg;
  const int grid = persistent_plan(B, Ho, Wo, device_cu_count(), nph, ncol, per_wg);
  hipLaunchKernelGGL((sepconv_bwd_mfma_p<KFAST, WV, WH>), dim3(grid), dim3(MNT), lds, st, in, v, h, gO, gV, gH, B, Ho, Wo, nph, ncol,
                     per_wg);
  return savfi_launch_status();
}

int launch_bwd_persistent(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH, int B, int Ho,
                          int Wo, hipStream_t st) {
  if (gV && gH) return launch_bwd_persistent_one<true, true>(in, v, h, gO, gV, gH, B, Ho, Wo, st);
  if (gV) return launch_bwd_persistent_one<true, false>(in, v, h, gO, gV, gH, B, Ho, Wo, st);
  return launch_bwd_persistent_one<false, true>(in, v, h, gO, gV, gH, B, Ho, Wo, st);
}

int check_dims(int B, int C, int Ho, int Wo, int K) {
  if (B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || K <= 0) return SAVFI_E_SHAPE;
  const int64_t Hi = (int64_t)Ho + K - 1, Wi = (int64_t)Wo + K - 1;
  if ((int64_t)B * K * Ho * Wo >= (int64_t)1 << 40 || (int64_t)B * C * Hi * Wi >= (int64_t)1 << 40)
    return SAVFI_E_TOOBIG;
  if ((int64_t)B * K > 65535 || (int64_t)B * C > 65535 || Ho + K - 1 > 65535) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

// Kernel switches of VARIANT BUILDS (compile-time: tools/build_variant.sh NAME sepconv.hip -DSAVFI_SEPCONV_...; the shipped library has
// none set): _NO_MFMA forces the direct kernels, _NO_WS the one-program-per-wave split-bf16 kernels (csrc/sepconv_x6.hip) instead of the
// wave-specialised ones (csrc/sepconv_ws.hip; _NO_WS_FWD: forward only), _F32_MFMA keeps every filter gradient on sepconv_bwd_mfma_p.
#ifdef SAVFI_SEPCONV_NO_MFMA
constexpr bool NO_MFMA = true;
#else
constexpr bool NO_MFMA = false;
#endif
#ifdef SAVFI_SEPCONV_NO_WS
constexpr bool NO_WS = true;
#else
constexpr bool NO_WS = false;
#endif
#ifdef SAVFI_SEPCONV_NO_WS_FWD
constexpr bool NO_WS_FWD = true;
#else
constexpr bool NO_WS_FWD = false;
#endif
#ifdef SAVFI_SEPCONV_F32_MFMA
constexpr bool F32_MFMA = true;
#else
constexpr bool F32_MFMA = false;
#endif

// THE route (include/savfi_hip.h, savfi_sepconv_route): which kernel a call of the contiguous entry points runs, and on how many
// consecutive samples per launch.  want: 0 = forward, 1 = gV only, 2 = gH only, 3 = both.  Pure host arithmetic.
constexpr int WS = SAVFI_SEPCONV_PARTITION_WS, X6 = SAVFI_SEPCONV_PARTITION_X6, FP32 = SAVFI_SEPCONV_PARTITION_FP32,
              DIRECT = SAVFI_SEPCONV_ROUTE_DIRECT;
struct Route {
  int kernel, chunk;
};
Route sepconv_route(int B, int C, int Ho, int Wo, int K, int want) {
  const int chunk = persistent_chunk(B, Ho, Wo);
  if (NO_MFMA || K != KFAST || C != 3 || chunk == 0) return {DIRECT, B};
  if (want == 1 || want == 2 || (want == 3 && F32_MFMA)) return {FP32, chunk};
  const bool ws = (Wo & 3) == 0 && !NO_WS && !(want == 0 && NO_WS_FWD);
  return {ws ? WS : X6, chunk};
}

}  // namespace

// Test hook: the span the persistent kernels' tensors must stay below (host state only: a smaller span means more, smaller launches;
// nothing in a kernel reads it).  0 restores 2^31, anything else is clamped to [1, 2^31].  The previous span goes to *previous (may be NULL).
extern "C" int savfi_sepconv_debug_span_bytes(int64_t bytes, int64_t* previous) {
  if (previous) *previous = span_bytes;
  span_bytes = bytes == 0 || bytes > SPAN_MAX ? SPAN_MAX : (bytes < 1 ? 1 : bytes);
  return SAVFI_OK;
}

extern "C" int savfi_sepconv_route(int want, int B, int C, int Ho, int Wo, int K, int* chunk) {
  if (want < 0 || want > 3) return SAVFI_E_SHAPE;
  if (int e = check_dims(B, C, Ho, Wo, K)) return e;
  const Route r = sepconv_route(B, C, Ho, Wo, K, want);
  if (chunk) *chunk = r.chunk;
  return r.kernel;
}

// Test hook: the CU count the persistent launches plan for (host side only: fewer workgroups that take more phases each is an ordinary
// launch, there is no dependency between workgroups).  0 restores the device's count, anything else is clamped to [1, device count].
// The previous setting (0 = the device's count) goes to *previous (may be NULL).
extern "C" int savfi_sepconv_debug_cus(int cus, int* previous) {
  if (previous) *previous = debug_cus;
  debug_cus = cus == 0 ? 0 : (cus < 1 ? 1 : cus);
  return SAVFI_OK;
}

// The piece [*g0, *g1) of the strip-major phase list that workgroup `block` of a persistent launch takes, from the host code the launches
// size their grids with and the functions the kernels cut their pieces with.  Returns the grid, or a negative error.
extern "C" int savfi_sepconv_partition(int kind, int B, int Ho, int Wo, int cus, int block, int* g0, int* g1) {
  if (!g0 || !g1) return SAVFI_E_NULL;
  if (B <= 0 || Ho <= 0 || Wo <= 0 || block < 0) return SAVFI_E_SHAPE;
  if ((int64_t)Ho * Wo >= (int64_t)1 << 40 || !persistent_ok(B, Ho, Wo)) return SAVFI_E_TOOBIG;   // what the route would cut into chunks
  if (cus <= 0) cus = device_cu_count();
  int grid;
  switch (kind) {
    case SAVFI_SEPCONV_PARTITION_WS: grid = savfi_sepconv_ws_partition(B, Ho, Wo, cus, block, g0, g1); break;
    case SAVFI_SEPCONV_PARTITION_X6: grid = savfi_sepconv_x6_partition(B, Ho, Wo, cus, block, g0, g1); break;
    case SAVFI_SEPCONV_PARTITION_FP32: {
      int nph, ncol, per_wg;
      grid = persistent_plan(B, Ho, Wo, cus, nph, ncol, per_wg);
      persistent_work_range(B * ncol * nph, per_wg, block, *g0, *g1);
      break;
    }
    default: return SAVFI_E_UNSUPPORTED;
  }
  if (block >= grid) return SAVFI_E_SHAPE;
  return grid;
}

extern "C" int savfi_sepconv_fwd_f32(const float* in, const float* v, const float* h, float* out, int B,
                                     int C, int Ho, int Wo, int K, void* stream) {
  if (!in || !v || !h || !out) return SAVFI_E_NULL;
  if (int e = check_dims(B, C, Ho, Wo, K)) return e;
  hipStream_t st = (hipStream_t)stream;
  const Route r = sepconv_route(B, C, Ho, Wo, K, 0);
  // one launch per run of r.chunk consecutive samples (the whole batch, unless its tensors exceed the span)
  const size_t in_s = (size_t)C * (Ho + K - 1) * ((size_t)Wo + K - 1), tap_s = (size_t)K * Ho * Wo, out_s = (size_t)C * Ho * Wo;
  for (int b = 0; b < B; b += r.chunk) {
    const int n = B - b < r.chunk ? B - b : r.chunk;
    const float *ib = in + b * in_s, *vb = v + b * tap_s, *hb = h + b * tap_s;
    float* ob = out + b * out_s;
    int e;
    switch (r.kernel) {
      case WS: e = savfi_sepconv_fwd_ws_launch(ib, vb, hb, ob, n, Ho, Wo, device_cu_count(), KFAST, nullptr, 0, st); break;
      case X6: e = savfi_sepconv_fwd_x6_launch(ib, vb, hb, ob, n, Ho, Wo, device_cu_count(), st); break;
      default: {   // DIRECT: any K, C; the whole batch (chunk = B)
        dim3 grid(savfi_cdiv(Wo, 64), Ho, n * C);
        hipLaunchKernelGGL(sepconv_fwd_direct, grid, dim3(64), 0, st, ib, vb, hb, ob, C, Ho, Wo, K);
        e = savfi_launch_status();
      }
    }
    if (e) return e;
  }
  return SAVFI_OK;
}

// The same op on tap tensors that are SLICES of one interleaved buffer: sample b of v / h (gV / gH) starts tap_bstride planes (of Ho * Wo
// floats) after sample b - 1 (51 = contiguous).  sepconv/model.py runs its four sub-networks as ONE task-batched launch per layer; their
// outputs form a [B * 4, 51, Ho, Wo] tensor whose sample 4 b + s belongs to sub-network s, and the two local convolutions read (and their
// gradients write) that buffer in place with tap_bstride = 4 * 51.  K = 51, C = 3, Wo % 4 == 0 (the wave-specialised kernels);
// anything else: SAVFI_E_UNSUPPORTED (the caller copies the slices and uses the contiguous entry points).
static int taps_strided_ok(int B, int C, int Ho, int Wo, int K, int tap_bstride) {
  if (int e = check_dims(B, C, Ho, Wo, K)) return e;
  if (tap_bstride < K) return SAVFI_E_SHAPE;
  // what the contiguous call runs on the wave-specialised kernels in one launch, with the strided tap buffer inside the span as well
  const Route r = sepconv_route(B, C, Ho, Wo, K, 3);
  const int64_t taps = ((int64_t)(B - 1) * tap_bstride + K) * Ho * Wo * 4;
  if (r.kernel != WS || r.chunk != B || taps >= span_bytes) return SAVFI_E_UNSUPPORTED;
  return SAVFI_OK;
}

// 1: the strided / frames8 / pair entry points take this problem NOW (shapes, sizes and the switches of a variant build:
// SAVFI_SEPCONV_NO_WS, _NO_WS_FWD, _NO_MFMA, _F32_MFMA make them refuse), 0: the caller uses the contiguous entry points
extern "C" int savfi_sepconv_taps_strided_supported(int B, int C, int Ho, int Wo, int K, int tap_bstride) {
  return taps_strided_ok(B, C, Ho, Wo, K, tap_bstride) == SAVFI_OK && !NO_WS_FWD ? 1 : 0;
}

extern "C" int savfi_sepconv_fwd_taps_strided_f32(const float* in, const float* v, const float* h, float* out, int B, int C, int Ho, int Wo,
                                                  int K, int tap_bstride, void* stream) {
  if (!in || !v || !h || !out) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, tap_bstride)) return e;
  return savfi_sepconv_fwd_ws_launch(in, v, h, out, B, Ho, Wo, device_cu_count(), tap_bstride, nullptr, 0, (hipStream_t)stream);
}

extern "C" int savfi_sepconv_bwd_taps_strided_f32(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH,
                                                  int B, int C, int Ho, int Wo, int K, int tap_bstride, void* stream) {
  if (!in || !v || !h || !gO || !gV || !gH) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, tap_bstride)) return e;
  return savfi_sepconv_bwd_ws_launch(in, v, h, gO, gV, gH, B, Ho, Wo, device_cu_count(), tap_bstride, nullptr, 0, (hipStream_t)stream);
}

// the strided entry points with the words of savfi_frames8_classify_f32(in) (csrc/sepconv_ws.hip): the device picks the three-product
// kernel for frames of 8-bit images and the six-product kernel for anything else
extern "C" int savfi_sepconv_fwd_frames8_f32(const float* in, const float* v, const float* h, float* out, const unsigned* cls, int B, int C,
                                             int Ho, int Wo, int K, int tap_bstride, int taps_unit16, void* stream) {
  if (!in || !v || !h || !out || !cls) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, tap_bstride)) return e;
  if (NO_WS_FWD) return SAVFI_E_UNSUPPORTED;
  return savfi_sepconv_fwd_ws_launch(in, v, h, out, B, Ho, Wo, device_cu_count(), tap_bstride, cls, taps_unit16 & 1, (hipStream_t)stream);
}

extern "C" int savfi_sepconv_bwd_frames8_f32(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH,
                                             const unsigned* cls, int B, int C, int Ho, int Wo, int K, int tap_bstride, int taps_unit16,
                                             void* stream) {
  if (!in || !v || !h || !gO || !gV || !gH || !cls) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, tap_bstride)) return e;
  return savfi_sepconv_bwd_ws_launch(in, v, h, gO, gV, gH, B, Ho, Wo, device_cu_count(), tap_bstride, cls, taps_unit16 & 3,
                                     (hipStream_t)stream);
}

// The forward of both local convolutions in ONE launch: out [B][2][C][Ho][Wo], out[b][f] = the local convolution of frame f of sample b with
// sub-networks 2 f / 2 f + 1 of taps [4 B][K][Ho][Wo]; the caller adds out[:, 0] and out[:, 1] (sepconv/model.py:346-347).  Bit for bit the
// results of the two calls of savfi_sepconv_fwd_frames8_f32 it replaces.
extern "C" int savfi_sepconv_fwd_pair_frames8_f32(const float* in0, const float* in1, const float* taps, float* out, const unsigned* cls0,
                                                  const unsigned* cls1, int B, int C, int Ho, int Wo, int K, int taps_unit16, void* stream) {
  if (!in0 || !in1 || !taps || !out || !cls0 || !cls1) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, 4 * K)) return e;
  if (NO_WS_FWD || B > 0x3fffffff / 2 || !persistent_ok(2 * B, Ho, Wo)) return SAVFI_E_UNSUPPORTED;
  const size_t plane = (size_t)K * Ho * Wo;
  return savfi_sepconv_fwd_ws_launch(in0, taps, taps + plane, out, 2 * B, Ho, Wo, device_cu_count(), 2 * K, cls0, taps_unit16 & 1,
                                     (hipStream_t)stream, in1, cls1);
}

// Both local convolutions of an interleaved tap tensor in ONE launch: taps / gtaps [4 B][K][Ho][Wo] with sample 4 b + s = sub-network s
// (0: v of frame 0, 1: h of frame 0, 2: v of frame 1, 3: h of frame 1), in0 / in1 the two frames, gO the cotangent of their sum.  The kernel
// sees 2 B virtual samples at a tap stride of 2 K planes (csrc/sepconv_ws.hip `pair`).  Same results, bit for bit, as the two calls of
// savfi_sepconv_bwd_frames8_f32 it replaces.
extern "C" int savfi_sepconv_bwd_pair_frames8_f32(const float* in0, const float* in1, const float* taps, const float* gO, float* gtaps,
                                                  const unsigned* cls0, const unsigned* cls1, int B, int C, int Ho, int Wo, int K,
                                                  int taps_unit16, void* stream) {
  if (!in0 || !in1 || !taps || !gO || !gtaps || !cls0 || !cls1) return SAVFI_E_NULL;
  if (int e = taps_strided_ok(B, C, Ho, Wo, K, 4 * K)) return e;
  if (B > 0x3fffffff / 2 || !persistent_ok(2 * B, Ho, Wo)) return SAVFI_E_UNSUPPORTED;
  const size_t plane = (size_t)K * Ho * Wo;
  return savfi_sepconv_bwd_ws_launch(in0, taps, taps + plane, gO, gtaps, gtaps + plane, 2 * B, Ho, Wo, device_cu_count(), 2 * K, cls0,
                                     taps_unit16 & 3, (hipStream_t)stream, in1, cls1);
}

extern "C" int savfi_sepconv_bwd_f32(const float* in, const float* v, const float* h, const float* gO,
                                     float* gI, float* gV, float* gH, int B, int C, int Ho, int Wo, int K,
                                     void* stream) {
  if (!in || !v || !h || !gO) return SAVFI_E_NULL;
  if (int e = check_dims(B, C, Ho, Wo, K)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (gV || gH) {
    const Route r = sepconv_route(B, C, Ho, Wo, K, (gV ? 1 : 0) | (gH ? 2 : 0));
    // one launch per run of r.chunk consecutive samples (the whole batch, unless its tensors exceed the span)
    const size_t in_s = (size_t)C * (Ho + K - 1) * ((size_t)Wo + K - 1), tap_s = (size_t)K * Ho * Wo, out_s = (size_t)C * Ho * Wo;
    for (int b = 0; b < B; b += r.chunk) {
      const int n = B - b < r.chunk ? B - b : r.chunk;
      const float *ib = in + b * in_s, *vb = v + b * tap_s, *hb = h + b * tap_s, *gb = gO + b * out_s;
      float *gVb = gV ? gV + b * tap_s : nullptr, *gHb = gH ? gH + b * tap_s : nullptr;
      int e;
      switch (r.kernel) {
        case WS: e = savfi_sepconv_bwd_ws_launch(ib, vb, hb, gb, gVb, gHb, n, Ho, Wo, device_cu_count(), KFAST, nullptr, 0, st); break;
        case X6: e = savfi_sepconv_bwd_x6_launch(ib, vb, hb, gb, gVb, gHb, n, Ho, Wo, device_cu_count(), st); break;
        case FP32: e = launch_bwd_persistent(ib, vb, hb, gb, gVb, gHb, n, Ho, Wo, st); break;
        default: {   // DIRECT: any K, C; the whole batch (chunk = B)
          dim3 grid(savfi_cdiv(Wo, 64), Ho, n * K);
          if (gV) hipLaunchKernelGGL(sepconv_bwd_filter_direct, grid, dim3(64), 0, st, ib, hb, gb, gVb, C, Ho, Wo, K, 0);
          if (gH) hipLaunchKernelGGL(sepconv_bwd_filter_direct, grid, dim3(64), 0, st, ib, vb, gb, gHb, C, Ho, Wo, K, 1);
          e = savfi_launch_status();
        }
      }
      if (e) return e;
    }
  }
  if (gI) {
    dim3 grid(savfi_cdiv(Wo + K - 1, 64), Ho + K - 1, B * C);
    hipLaunchKernelGGL(sepconv_bwd_input_direct, grid, dim3(64), 0, st, v, h, gO, gI, C, Ho, Wo, K);
    if (int e = savfi_launch_status()) return e;
  }
  return SAVFI_OK;
}
