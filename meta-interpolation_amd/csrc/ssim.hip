// Fused SSIM loss term (and its gradient) for gfx950: what the reference's Loss wrapper computes for 'SSIM'
// (loss.py:294 -> pytorch_msssim/__init__.py:7-131): an 11 x 11 Gaussian window (sigma 1.5), valid correlation, over the five
// moment maps of prediction and target, a rational expression per pixel, mean, (1 - mean) / 2 -- with the dynamic range L
// decided from the prediction's data on every call (:21-31).  Composed from library ops that is 5 depthwise convolutions,
// ~15 element-wise launches, a max / min with a host decision, and twice that again in autograd's backward.
//
// Here: `rows` independent losses per launch (one per sample: tasks in lockstep, the two support triplets of a step).
//   ssim_range   max / min of every row of the prediction -> per-block partial extrema (skipped for a fixed L)
//   ssim_fwd     fwd_tile: a workgroup owns a 16 x 64 tile of SSIM values of one channel plane: 26 x 76 patches of both images into
//                LDS (float4 where the operands allow), 11-tap row pass over the five products into LDS, column pass out of LDS
//                (separable: 22 instead of 121 multiply-adds per moment), map, one partial sum per workgroup.  It reduces
//                the row's partial extrema itself (no host read: the op is capturable) and publishes the row's range word.
//   ssim_finish  adds a row's partial sums in a fixed order (no float atomics: bit-reproducible) -> (1 - sum / n) / 2
//   ssim_bwd     bwd_tile, one launch: a workgroup owns 16 x 32 pixels of d loss / d sr, recomputes the moments on the tile grown by
//                the 10-pixel halo (26 x 42 SSIM positions from 36 x 56 patches), forms the three coefficient planes a, b, c in
//                LDS and applies the adjoint window (row pass, column pass) to them:
//                  d loss / d sr = -(g / (2 n)) (G^T[a] + 2 sr G^T[b] + hr G^T[c])
//                  b = d map / d s1, c = d map / d s12, a = (d map / d mu1 at fixed s1, s12) - 2 mu1 b - mu2 c
//                Nothing is kept from the forward but the two images and the range word.
// There is ONE forward tile and ONE backward tile; the other two users are the same tiles with options switched on, under kernel names
// of their own:
//   metric_tile    the PSNR / SSIM evaluation metric (utils.py:171-204: quantize + calc_psnr + ssim(val_range=255)): fwd_tile with
//                  both unit-range images quantised to 0 .. 255 as they are loaded into LDS, L = 255 fixed (no range pass, no range
//                  word), and next to the SSIM partial sum the integer sum of squared differences of the pixels the workgroup owns
//   metric_finish  per row: SSIM partial sums in ssim_finish's order -> mean; integer partials as 64 bits -> S, mse = S / (65025 n)
//   msssim_level, msssim_finish, msssim_bwd_level   multi-scale SSIM (pytorch_msssim/__init__.py:78-104), per level: fwd_tile with the
//                  cs partial sum, the 2 x 2 pooling of the next level's pair and the partial extrema of its prediction; the means,
//                  product and factors; bwd_tile on the cs or the SSIM map, coarse to fine.  See the section further down.
// One window table (GN: the windows of 1 .. 11 taps, zero beyond the last tap) and one row-tap function serve every kernel; the
// single-scale entry points run with taps = 11.  Every window sum is accumulated tap 0 .. 10 in the same association for every pixel,
// whatever its place in a tile and whichever kernel runs the tile: tests/test_ssim_family_bits_gpu.py holds the users to each other's bits.
// LDS: lanes run along image columns in every pass, so each ds_read_b32 / ds_write_b32 of a wave touches consecutive
// words (conflict-free for any row stride); 49 KB (forward) and 59 KB (backward) of static LDS: three resp. two workgroups per CU.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / SAVFI_WAVE;
constexpr int WIN = 11;
constexpr int HALO = WIN - 1;

// forward tile
constexpr int TH = 16, TW = 64;
constexpr int PH = TH + HALO;          // 26 patch rows
constexpr int PW = 76;                 // 74 patch columns, rounded up to float4s
// backward tile (pixels of the gradient)
constexpr int BH = 16, BW = 32;
constexpr int CH = BH + HALO;          // 26 rows of SSIM positions whose window touches the tile
constexpr int CW = BW + HALO;          // 42 columns
constexpr int QH = CH + HALO;          // 36 patch rows
constexpr int QX = 12;                 // patch column 0 is pixel x0 - QX (float4 aligned; the halo needs x0 - 10)
constexpr int QW = 56;                 // 2 + 52 + 2 patch columns

constexpr int RANGE_PER_BLOCK = 8192;
constexpr int RANGE_MAX_BLOCKS = NT;   // partial extrema per row: one per thread of a forward workgroup

// The windows of pytorch_msssim.create_window, gaussian(n, 1.5) for n = 1 .. 11 taps: exp(-(i - n / 2)^2 / 4.5) evaluated in double,
// rounded to fp32, divided by their fp32 sum.  (The reference multiplies the outer product out in fp32; the separable passes here
// round differently by < 1 ulp per weight.)  Row n - 1 is the window of n taps, zero beyond tap n - 1: every pass runs 11 taps in one
// association, the trailing products are 0 * (a pixel or the zero fill), and the valid positions are H - n + 1, W - n + 1.  The SSIM
// loss and the metric use the last row; multi-scale SSIM min(11, H_s, W_s) taps on level s.
__device__ __constant__ float GN[WIN][WIN] = {
    {0x1p+0f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.c75814p-2f, 0x1.1c53f6p-1f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.3b3046p-2f, 0x1.899f76p-2f, 0x1.3b3046p-2f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.177ae4p-3f, 0x1.102d28p-2f, 0x1.53e83ep-2f, 0x1.102d28p-2f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.ebd74ep-4f, 0x1.defcdep-3f, 0x1.2b1778p-2f, 0x1.defcdep-3f, 0x1.ebd74ep-4f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.3781f8p-5f, 0x1.d9236ep-4f, 0x1.ccc61cp-3f, 0x1.1fb7eep-2f, 0x1.ccc61cp-3f, 0x1.d9236ep-4f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {0x1.2c18a6p-5f, 0x1.c7ce56p-4f, 0x1.bbe4fap-3f, 0x1.152db4p-2f, 0x1.bbe4fap-3f, 0x1.c7ce56p-4f, 0x1.2c18a6p-5f, 0.f, 0.f, 0.f, 0.f},
    {0x1.f6d8f2p-8f, 0x1.29cb2ep-5f, 0x1.c44f04p-4f, 0x1.b87d0cp-3f, 0x1.130d42p-2f, 0x1.b87d0cp-3f, 0x1.c44f04p-4f, 0x1.29cb2ep-5f, 0.f, 0.f,
     0.f},
    {0x1.f304c2p-8f, 0x1.2786b2p-5f, 0x1.c0dd56p-4f, 0x1.b5226ap-3f, 0x1.10f51ap-2f, 0x1.b5226ap-3f, 0x1.c0dd56p-4f, 0x1.2786b2p-5f,
     0x1.f304c2p-8f, 0.f, 0.f},
    {0x1.0ddc78p-10f, 0x1.f2813ep-8f, 0x1.2738dp-5f, 0x1.c0670ap-4f, 0x1.b4af36p-3f, 0x1.10ad2ap-2f, 0x1.b4af36p-3f, 0x1.c0670ap-4f,
     0x1.2738dp-5f, 0x1.f2813ep-8f, 0.f},
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, 0x1.b43c3ep-3f, 0x1.bff0fep-4f,
     0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}};

// the window of `taps` taps, into registers
__device__ __forceinline__ void load_window(int taps, float (&g)[WIN]) {
#pragma unroll
  for (int k = 0; k < WIN; ++k) g[k] = GN[taps - 1][k];
}

// range word: bit 0 = min(sr) < -0.5, bit 1 = max(sr) > 128  ->  L = (255 or 1) - (-1 or 0); C1 = (0.01 L)^2, C2 = (0.03 L)^2
// evaluated in double like the reference's Python scalars
__device__ __forceinline__ void ssim_constants(unsigned cls, float& C1, float& C2) {
  constexpr float c1[4] = {(float)((0.01 * 1.0) * (0.01 * 1.0)), (float)((0.01 * 2.0) * (0.01 * 2.0)),
                           (float)((0.01 * 255.0) * (0.01 * 255.0)), (float)((0.01 * 256.0) * (0.01 * 256.0))};
  constexpr float c2[4] = {(float)((0.03 * 1.0) * (0.03 * 1.0)), (float)((0.03 * 2.0) * (0.03 * 2.0)),
                           (float)((0.03 * 255.0) * (0.03 * 255.0)), (float)((0.03 * 256.0) * (0.03 * 256.0))};
  cls &= 3u;
  C1 = cls == 0 ? c1[0] : cls == 1 ? c1[1] : cls == 2 ? c1[2] : c1[3];
  C2 = cls == 0 ? c2[0] : cls == 1 ? c2[1] : cls == 2 ? c2[2] : c2[3];
}

// block-wide max of `hi` and min of `lo`; every thread gets both
__device__ __forceinline__ void block_extrema(float& hi, float& lo, float* lds /* 2 * NW floats */) {
  hi = wave_max(hi);
  lo = -wave_max(-lo);
  const int lane = threadIdx.x & (SAVFI_WAVE - 1), wid = threadIdx.x / SAVFI_WAVE;
  if (lane == 0) {
    lds[wid] = hi;
    lds[NW + wid] = lo;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    hi = fmaxf(hi, lds[w]);
    lo = fminf(lo, lds[NW + w]);
  }
  __syncthreads();
}

// ext[(row * blocks + blk) * 2 + {0, 1}] = max, min of the block's chunk of row `row`
__global__ __launch_bounds__(NT) void ssim_range(const float* __restrict__ sr, float* __restrict__ ext, long long n, long long per_block,
                                                 int vec_ok) {
  __shared__ float red[2 * NW];
  const float* p = sr + (long long)blockIdx.y * n;
  const long long base = (long long)blockIdx.x * per_block;
  const long long end = min(base + per_block, n);
  float hi = -INFINITY, lo = INFINITY;
  if (vec_ok && base < end) {      // per_block % 4 == 0 and 16-byte aligned rows
    const long long vend = base + ((end - base) & ~3LL);
    for (long long e = base + 4 * threadIdx.x; e < vend; e += 4 * NT) {
      const float4 v = *reinterpret_cast<const float4*>(p + e);
      hi = fmaxf(fmaxf(hi, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
      lo = fminf(fminf(lo, fminf(v.x, v.y)), fminf(v.z, v.w));
    }
    for (long long e = vend + threadIdx.x; e < end; e += NT) {
      hi = fmaxf(hi, p[e]);
      lo = fminf(lo, p[e]);
    }
  } else {
    for (long long e = base + threadIdx.x; e < end; e += NT) {
      hi = fmaxf(hi, p[e]);
      lo = fminf(lo, p[e]);
    }
  }
  block_extrema(hi, lo, red);
  if (threadIdx.x == 0) {
    float* o = ext + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = hi;
    o[1] = lo;
  }
}

// (ROWS x COLS) patch of a plane with origin (y0, x0) -> LDS [ROWS][COLS], zero outside the plane.  x0 % 4 == 0;
// vec_ok: plane base 16-byte aligned and W % 4 == 0.  QUANT: the values are quantised to 0 .. 255 on the way (the metric: LDS holds
// the integers, nothing quantised goes to HBM); outside the plane stays 0.
template <int ROWS, int COLS, bool QUANT = false>
__device__ __forceinline__ void load_patch(const float* __restrict__ plane, float* __restrict__ dst, int y0, int x0, int H, int W,
                                           int vec_ok) {
  constexpr int QUADS = COLS / 4;
  for (int i = threadIdx.x; i < ROWS * QUADS; i += NT) {
    const int r = i / QUADS, q = i - r * QUADS;
    const int gy = y0 + r, gx = x0 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H) {
      const float* src = plane + (size_t)gy * W;
      if (vec_ok && gx >= 0 && gx + 3 < W) {
        v = *reinterpret_cast<const float4*>(src + gx);
      } else {
        if (gx >= 0 && gx < W) v.x = src[gx];
        if (gx + 1 >= 0 && gx + 1 < W) v.y = src[gx + 1];
        if (gx + 2 >= 0 && gx + 2 < W) v.z = src[gx + 2];
        if (gx + 3 >= 0 && gx + 3 < W) v.w = src[gx + 3];
      }
      if constexpr (QUANT) v = make_float4(savfi_quantize255(v.x), savfi_quantize255(v.y), savfi_quantize255(v.z), savfi_quantize255(v.w));
    }
    *reinterpret_cast<float4*>(dst + r * COLS + 4 * q) = v;
  }
}

// The five window sums of one position of the 11-tap row pass under window g: x, y, x^2, y^2, xy.
__device__ __forceinline__ void row_taps_n(const float (&g)[WIN], const float* __restrict__ x, const float* __restrict__ y, float (&s)[5]) {
  s[0] = s[1] = s[2] = s[3] = s[4] = 0.f;
#pragma unroll
  for (int k = 0; k < WIN; ++k) {
    const float a = x[k], b = y[k];
    s[0] = fmaf(g[k], a, s[0]);
    s[1] = fmaf(g[k], b, s[1]);
    s[2] = fmaf(g[k], a * a, s[2]);
    s[3] = fmaf(g[k], b * b, s[3]);
    s[4] = fmaf(g[k], a * b, s[4]);
  }
}

// SSIM value of one position from its five window sums (mu1, mu2, E[x^2], E[y^2], E[xy]).  Written so that an identical pair
// gives exactly 1: no contraction, so that mu1 mu1 + mu2 mu2 == 2 (mu1 mu2) and s1 + s2 == 2 s12 bit for bit when the
// operands are equal, and A / B == 1.
__device__ __forceinline__ float ssim_value(const float (&m)[5], float C1, float C2, float& r1, float& r2, float& B1, float& B2) {
#pragma clang fp contract(off)
  const float m11 = m[0] * m[0], m22 = m[1] * m[1], m12 = m[0] * m[1];
  const float s1 = m[2] - m11, s2 = m[3] - m22, s12 = m[4] - m12;
  const float A1 = 2.f * m12 + C1;
  const float A2 = 2.f * s12 + C2;
  B1 = (m11 + m22) + C1;
  B2 = (s1 + s2) + C2;
  r1 = A1 / B1;
  r2 = A2 / B2;
  return r1 * r2;
}

// NaN word of a workgroup's squared-error partial (a workgroup's sum stays below 2^27, see metric_tile)
constexpr unsigned SQ_NAN = 0xffffffffu;

// THE forward tile, of every kernel below that computes an SSIM map.  grid (tiles_x, tiles_y, rows * C) over the (H - taps + 1) x
// (W - taps + 1) positions; the workgroup's index w = (z * tiles_y + by) * tiles_x + bx; partial[w] = its SSIM sum.
// The range class: fixed_cls, or (fixed_cls < 0) from `ext`, the ext_blocks (max, min) pairs of this row's prediction; the first
// workgroup of a row publishes it in *cls_word (the word of ITS row; NULL: nobody asks).
// Every pixel of the plane has one owner: the tiles step over the SSIM positions, so the last tile row / column also own the trailing
// pixel rows / columns, which lie inside their patch.  The options work on the owned pixels, out of the LDS patches:
//   QUANT  the patches are quantised on load
//   SQERR  the workgroup also adds (x - y)^2 of the (quantised) pair as an integer -> sq_partial[w] (<= 26 x 74 pixels * 65025 < 2^27:
//          the 32-bit sum is exact); a NaN among the owned pixels -> SQ_NAN
//   MULTI  the cs map v1 / v2 is summed too -> partial[total + w], and unless pool1 is NULL (the last level) the pair is pooled for the
//          next level: pool1 / pool2 [rows * C, H / 2, W / 2] averages, ((a + b) + c) + d over (0,0) (0,1) (1,0) (1,1), times 0.25 --
//          avg_pool2d's order; ext_out[2 w] = max, min of the pooled prediction values this workgroup wrote (the next level's `ext`: the
//          pooled pair is not read again for it).  TH and TW are even, so no 2 x 2 block straddles two owners.
template <bool QUANT, bool SQERR, bool MULTI>
__device__ __forceinline__ void fwd_tile(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ ext,
                                         int ext_blocks, int fixed_cls, unsigned* __restrict__ cls_word, float* __restrict__ partial,
                                         unsigned* __restrict__ sq_partial, float* __restrict__ pool1, float* __restrict__ pool2,
                                         float* __restrict__ ext_out, int row, int H, int W, int taps, int vec_ok) {
  __shared__ __attribute__((aligned(16))) float px[PH * PW];
  __shared__ __attribute__((aligned(16))) float py[PH * PW];
  __shared__ float rf[5][PH][TW];
  __shared__ float red[2 * NW];
  const int z = blockIdx.z;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int Ho = H - taps + 1, Wo = W - taps + 1;
  const size_t plane = (size_t)z * H * W;
  const size_t wg = ((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int own_h = blockIdx.y + 1 == gridDim.y ? H - y0 : TH, own_w = blockIdx.x + 1 == gridDim.x ? W - x0 : TW;
  load_patch<PH, PW, QUANT>(sr + plane, px, y0, x0, H, W, vec_ok);
  load_patch<PH, PW, QUANT>(hr + plane, py, y0, x0, H, W, vec_ok);
  unsigned cls = (unsigned)fixed_cls;
  if (fixed_cls < 0) {
    float hi = -INFINITY, lo = INFINITY;
    const float* e = ext + (size_t)row * ext_blocks * 2;
    for (int i = threadIdx.x; i < ext_blocks; i += NT) {
      hi = fmaxf(hi, e[2 * i]);
      lo = fminf(lo, e[2 * i + 1]);
    }
    block_extrema(hi, lo, red);
    cls = (lo < -0.5f ? 1u : 0u) | (hi > 128.f ? 2u : 0u);
  }
  if (cls_word && threadIdx.x == 0) *cls_word = cls;
  float C1, C2;
  ssim_constants(cls, C1, C2);
  float g[WIN];
  load_window(taps, g);
  __syncthreads();

  if constexpr (SQERR) {
    __shared__ unsigned sq_red[NW];
    unsigned acc = 0;
    int bad = 0;
    for (int i = threadIdx.x; i < own_h * own_w; i += NT) {
      const int r = i / own_w, c = i - r * own_w;
      const float d = px[r * PW + c] - py[r * PW + c];
      if (d != d) {
        bad = 1;
      } else {
        acc += (unsigned)(int)(d * d);      // integers up to 255^2: exact in fp32
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += (unsigned)__shfl_xor((int)acc, off, SAVFI_WAVE);
    if ((threadIdx.x & (SAVFI_WAVE - 1)) == 0) sq_red[threadIdx.x / SAVFI_WAVE] = acc;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
      unsigned tot = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) tot += sq_red[w];
      sq_partial[wg] = bad ? SQ_NAN : tot;
    }
  }

  if (MULTI && pool1) {
    const int ph = own_h / 2, pw = own_w / 2, H2 = H / 2, W2 = W / 2;
    const size_t pplane = (size_t)z * H2 * W2;
    float hi = -INFINITY, lo = INFINITY;
    for (int i = threadIdx.x; i < ph * pw; i += NT) {
      const int r = i / pw, c = i - r * pw;
      const float* a = px + (2 * r) * PW + 2 * c;
      const float* b = py + (2 * r) * PW + 2 * c;
      const float va = (((a[0] + a[1]) + a[PW]) + a[PW + 1]) * 0.25f;
      const float vb = (((b[0] + b[1]) + b[PW]) + b[PW + 1]) * 0.25f;
      const size_t o = pplane + (size_t)(y0 / 2 + r) * W2 + (x0 / 2 + c);
      pool1[o] = va;
      pool2[o] = vb;
      hi = fmaxf(hi, va);
      lo = fminf(lo, va);
    }
    block_extrema(hi, lo, red);
    if (threadIdx.x == 0) {
      ext_out[2 * wg] = hi;
      ext_out[2 * wg + 1] = lo;
    }
  }

  for (int i = threadIdx.x; i < PH * TW; i += NT) {
    const int r = i / TW, c = i - r * TW;
    float s[5];
    row_taps_n(g, px + r * PW + c, py + r * PW + c, s);
#pragma unroll
    for (int p = 0; p < 5; ++p) rf[p][r][c] = s[p];
  }
  __syncthreads();

  // column pass: thread = one column, four consecutive rows (14 values of every plane slide through registers)
  const int c = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * 4;
  float mom[4][5];
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    float v[4 + HALO];
#pragma unroll
    for (int k = 0; k < 4 + HALO; ++k) v[k] = rf[p][r0 + k][c];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmaf(g[k], v[o + k], acc);
      mom[o][p] = acc;
    }
  }
  float sum = 0.f, cs = 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    float r1, r2, B1, B2;
    const float v = ssim_value(mom[o], C1, C2, r1, r2, B1, B2);
    if (y0 + r0 + o < Ho && x0 + c < Wo) {
      sum += v;
      if constexpr (MULTI) cs += r2;
    }
  }
  const float tot = block_sum<NW>(sum, red);
  if (threadIdx.x == 0) partial[wg] = tot;
  if constexpr (MULTI) {
    const float tcs = block_sum<NW>(cs, red);
    if (threadIdx.x == 0) partial[(size_t)gridDim.z * gridDim.y * gridDim.x + wg] = tcs;
  }
}

// the word of row `row` for its first workgroup, NULL for every other one
__device__ __forceinline__ unsigned* first_of_row(unsigned* word, int row, int C) {
  return blockIdx.x == 0 && blockIdx.y == 0 && (int)blockIdx.z == row * C ? word : nullptr;
}

__global__ __launch_bounds__(NT) void ssim_fwd(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ ext,
                                               int ext_blocks, int fixed_cls, unsigned* __restrict__ range_word,
                                               float* __restrict__ partial, int C, int H, int W, int vec_ok) {
  const int row = blockIdx.z / C;
  fwd_tile<false, false, false>(sr, hr, ext, ext_blocks, fixed_cls, first_of_row(range_word + row, row, C), partial, nullptr, nullptr,
                                nullptr, nullptr, row, H, W, WIN, vec_ok);
}

// the metric's tile kernel: unit-range pred / target in, SSIM partial sum and integer squared-error partial out; L = 255
__global__ __launch_bounds__(NT) void metric_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                  float* __restrict__ partial, unsigned* __restrict__ sq_partial, int C, int H, int W,
                                                  int vec_ok) {
  fwd_tile<true, true, false>(pred, target, nullptr, 0, 2, nullptr, partial, sq_partial, nullptr, nullptr, nullptr, 0, H, W, WIN, vec_ok);
}

// the sum of `blocks` partial sums by one wave: lane-strided, then a butterfly -- always the same order; every lane gets it.
// also(i) runs in the same pass for whatever else the caller gathers per workgroup (one walk over the row: the loop is latency-bound).
template <typename F>
__device__ __forceinline__ float row_sum(const float* __restrict__ p, int blocks, F also) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < blocks; i += 64) {
    acc += p[i];
    also(i);
  }
  return wave_sum(acc);
}

// result[row] = (1 - (the row's partial sums) / n) / 2
__global__ __launch_bounds__(64) void ssim_finish(const float* __restrict__ partial, float* __restrict__ result, int blocks, float n) {
  const float acc = row_sum(partial + (size_t)blockIdx.x * blocks, blocks, [](int) {});
  if (threadIdx.x == 0) result[blockIdx.x] = (1.f - acc / n) / 2.f;
}

// result[row] = {mse, ssim}: the SSIM partial sums in ssim_finish's order / n_out; the squared-error partials as 64-bit integers
// (exact, whatever the order) -> S / (65025 n_pix) in double.  A NaN word makes the mse NaN (the SSIM sum then is NaN by itself:
// every pixel lies in some window) and sq_sum[row] all ones.
__global__ __launch_bounds__(64) void metric_finish(const float* __restrict__ partial, const unsigned* __restrict__ sq_partial,
                                                    float* __restrict__ result, unsigned long long* __restrict__ sq_sum, int blocks,
                                                    float n_out, double n_pix) {
  const unsigned* q = sq_partial + (size_t)blockIdx.x * blocks;
  unsigned long long S = 0;
  int bad = 0;
  const float acc = row_sum(partial + (size_t)blockIdx.x * blocks, blocks, [&](int i) {
    const unsigned w = q[i];
    bad |= w == SQ_NAN;
    S += w;
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)S, off, SAVFI_WAVE), hi = (unsigned)__shfl_xor((int)(unsigned)(S >> 32), off, SAVFI_WAVE);
    S += ((unsigned long long)hi << 32) | lo;
    bad |= __shfl_xor(bad, off, SAVFI_WAVE);
  }
  if (threadIdx.x == 0) {
    result[2 * blockIdx.x] = bad ? __builtin_nanf("") : (float)((double)S / (65025.0 * n_pix));
    result[2 * blockIdx.x + 1] = acc / n_out;
    if (sq_sum) sq_sum[blockIdx.x] = bad ? ~0ULL : S;
  }
}

// THE backward tile.  grid (cdiv(W, BW), cdiv(H, BH), rows * C): g_sr = scale * (the gradient of the sum of a map under the window of
// `taps` taps and range class `cls`) + a quarter of g_coarse, replicated.  SSIM_MAP: the SSIM map, else the cs map v1 / v2.
// g_coarse (NULL: none): the gradient of the next-coarser level [rows * C, H / 2, W / 2]; a pixel whose 2 x 2 block was dropped by the
// floor gets nothing from it.
template <bool SSIM_MAP>
__device__ __forceinline__ void bwd_tile(const float* __restrict__ sr, const float* __restrict__ hr, unsigned cls, float scale,
                                         const float* __restrict__ g_coarse, float* __restrict__ g_sr, int H, int W, int taps,
                                         int vec_ok) {
  __shared__ __attribute__((aligned(16))) float px[QH * QW];
  __shared__ __attribute__((aligned(16))) float py[QH * QW];
  __shared__ float rf[5][QH][CW];                  // row-filtered moments; later the row-filtered coefficients [3][CH][BW]
  __shared__ float coef[3][CH][CW];
  float(*ar)[CH][BW] = reinterpret_cast<float(*)[CH][BW]>(&rf[0][0][0]);
  static_assert(3 * CH * BW <= 5 * QH * CW, "the row-filtered coefficients reuse the moments' planes");
  const int z = blockIdx.z;
  const int y0 = blockIdx.y * BH, x0 = blockIdx.x * BW;
  const int Ho = H - taps + 1, Wo = W - taps + 1;
  const size_t plane = (size_t)z * H * W;
  load_patch<QH, QW>(sr + plane, px, y0 - HALO, x0 - QX, H, W, vec_ok);
  load_patch<QH, QW>(hr + plane, py, y0 - HALO, x0 - QX, H, W, vec_ok);
  float C1, C2;
  ssim_constants(cls, C1, C2);
  float g[WIN];
  load_window(taps, g);
  __syncthreads();

  // moments, row pass: SSIM column cc is position x0 - 10 + cc, its window starts at patch column cc + 2
  for (int i = threadIdx.x; i < QH * CW; i += NT) {
    const int r = i / CW, cc = i - r * CW;
    float s[5];
    row_taps_n(g, px + r * QW + cc + (QX - HALO), py + r * QW + cc + (QX - HALO), s);
#pragma unroll
    for (int p = 0; p < 5; ++p) rf[p][r][cc] = s[p];
  }
  __syncthreads();

  // moments, column pass, and the coefficient planes (zero outside the valid SSIM positions)
  for (int i = threadIdx.x; i < CH * CW; i += NT) {
    const int cr = i / CW, cc = i - cr * CW;
    const int oy = y0 - HALO + cr, ox = x0 - HALO + cc;
    float a = 0.f, b = 0.f, c = 0.f;
    if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
      float m[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) acc = fmaf(g[k], rf[p][cr + k][cc], acc);
        m[p] = acc;
      }
      float r1, r2, B1, B2;
      const float v = ssim_value(m, C1, C2, r1, r2, B1, B2);
      {
#pragma clang fp contract(off)
        if constexpr (SSIM_MAP) {
          // an identical pair gives v = r1 = r2 = 1: then c == -2 b, dm == 0 and a == 0 exactly, and so is the gradient
          b = -v / B2;
          c = (2.f * r1) / B2;
          const float dm = ((2.f * m[1]) * r2) / B1 - ((2.f * m[0]) * v) / B1;
          a = (dm - (2.f * m[0]) * b) - m[1] * c;
        } else {
          // cs = A2 / B2 does not see mu1 but through s1 and s12; an identical pair gives r2 = 1, c == -2 b and a == 0 exactly
          b = -r2 / B2;
          c = 2.f / B2;
          a = (0.f - (2.f * m[0]) * b) - m[1] * c;
        }
      }
    }
    coef[0][cr][cc] = a;
    coef[1][cr][cc] = b;
    coef[2][cr][cc] = c;
  }
  __syncthreads();      // every read of rf is done: `ar` reuses it

  // adjoint, row pass: pixel column ix gathers G[k] * coef[position ix - k] = coef column ix + 10 - k
  for (int i = threadIdx.x; i < CH * BW; i += NT) {
    const int cr = i / BW, ix = i - cr * BW;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmaf(g[k], coef[p][cr][ix + HALO - k], acc);
      ar[p][cr][ix] = acc;
    }
  }
  __syncthreads();

  // adjoint, column pass, and the gradient
  const int H2 = H / 2, W2 = W / 2;
  for (int i = threadIdx.x; i < BH * BW; i += NT) {
    const int iy = i / BW, ix = i - iy * BW;
    const int gy = y0 + iy, gx = x0 + ix;
    float t[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmaf(g[k], ar[p][iy + HALO - k][ix], acc);
      t[p] = acc;
    }
    if (gy < H && gx < W) {
#pragma clang fp contract(off)
      const float x = px[(iy + HALO) * QW + ix + QX], y = py[(iy + HALO) * QW + ix + QX];
      float v = scale * ((t[0] + (2.f * x) * t[1]) + y * t[2]);
      if (g_coarse && (gy >> 1) < H2 && (gx >> 1) < W2) v += 0.25f * g_coarse[(size_t)z * H2 * W2 + (size_t)(gy >> 1) * W2 + (gx >> 1)];
      g_sr[plane + (size_t)gy * W + gx] = v;
    }
  }
}

// d loss / d sr of the SSIM loss: the SSIM map's gradient times -g / (2 n)
__global__ __launch_bounds__(NT) void ssim_bwd(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ g_loss,
                                               const unsigned* __restrict__ range_word, float* __restrict__ g_sr, int C, int H, int W,
                                               float inv_2n, int vec_ok) {
  const int row = blockIdx.z / C;
  bwd_tile<true>(sr, hr, range_word[row], -g_loss[row] * inv_2n, nullptr, g_sr, H, W, WIN, vec_ok);
}

// ------------------------------------------------------------------------------------------------------------------------
// Multi-scale SSIM (pytorch_msssim/__init__.py:78-104, "as implemented"): five levels, each the SSIM map and the cs map v1 / v2 of
// one image pair under the window of min(11, H_s, W_s) taps, then both images 2 x 2 averaged (floor).  Result
// ssim_4 ^ (4 w_4) * prod_{s < 4} cs_s ^ w_s (the reference's prod(pow1[:-1] * pow2[-1])).
//   msssim_level   fwd_tile with MULTI: SSIM and cs partial sums of one level, and out of the same LDS patches the 2 x 2 averages of
//                  the pixels the workgroup owns (both images, the next level's operands) and the partial extrema of the pooled
//                  prediction (the next level's range class)
//   msssim_finish  per row: the ten means (partial sums in a fixed order), the result, and the ten factors d out / d mean
//   msssim_bwd_level  coarse to fine, bwd_tile: the level's own map gradient (cs map on levels 0 .. 3, SSIM map on level 4: the
//                  other factors are identically zero) plus a quarter of the next-coarser level's gradient, replicated
// The kernels here add nothing to the tiles but where a level's class word, factor and window length are found.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int MS_LEVELS = 5;
constexpr int MS_HEAD = 16;      // 32-bit words per row at the start of the scratch: 10 factors, 5 class words, 1 spare

// One level of the forward.  ext: ssim_range's partial extrema on level 0, the previous level's workgroups' after that; QUANT only on
// level 0 (the metric: the pooled pair then is the quantised one's).
template <bool QUANT>
__global__ __launch_bounds__(NT) void msssim_level(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ ext,
                                                   int ext_blocks, int fixed_cls, unsigned* __restrict__ head, int level,
                                                   float* __restrict__ partial, float* __restrict__ pool1, float* __restrict__ pool2,
                                                   float* __restrict__ ext_out, int C, int H, int W, int taps, int vec_ok) {
  const int row = blockIdx.z / C;
  fwd_tile<QUANT, false, true>(sr, hr, ext, ext_blocks, fixed_cls, first_of_row(head + (size_t)row * MS_HEAD + 2 * MS_LEVELS + level, row, C),
                               partial, nullptr, pool1, pool2, ext_out, row, H, W, taps, vec_ok);
}

struct MsFinish {
  long long partial[MS_LEVELS];      // offset of the level's partial sums in the scratch, floats
  int blocks[MS_LEVELS];             // workgroups per row
  int wgs[MS_LEVELS];                // workgroups of the level (the cs sums follow the SSIM sums)
  float n[MS_LEVELS];                // map values per row
};

// One workgroup per row.  The ten means as ssim_finish adds them (fp32, / n), the normalisation (m + 1) / 2 in fp32 as the reference
// does it; powers and factors in double by one thread.  head[row]: d out / d ssim_0..4 (only ssim_4's is non-zero), d out / d cs_0..4
// (cs_4's is zero), with respect to the plain means.  A negative base: pow gives NaN, and so are the result and every factor.
__global__ __launch_bounds__(64) void msssim_finish(const float* __restrict__ scratch, float* __restrict__ head, float* __restrict__ result,
                                                    MsFinish f, int normalize) {
  const float w[MS_LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
  const int row = blockIdx.x;
  float ms[MS_LEVELS], mc[MS_LEVELS];
#pragma unroll
  for (int s = 0; s < MS_LEVELS; ++s) {
    const float* p = scratch + f.partial[s] + (size_t)row * f.blocks[s];
    float b = 0.f;
    ms[s] = row_sum(p, f.blocks[s], [&](int i) { b += p[f.wgs[s] + i]; }) / f.n[s];
    mc[s] = wave_sum(b) / f.n[s];
    if (normalize) {
      ms[s] = (ms[s] + 1.f) / 2.f;
      mc[s] = (mc[s] + 1.f) / 2.f;
    }
  }
  if (threadIdx.x != 0) return;
  const double w4 = 4.0 * (double)w[MS_LEVELS - 1];
  double out = pow((double)ms[MS_LEVELS - 1], w4);
#pragma unroll
  for (int s = 0; s < MS_LEVELS - 1; ++s) out *= pow((double)mc[s], (double)w[s]);
  const double chain = normalize ? 0.5 : 1.0;
  float* h = head + (size_t)row * MS_HEAD;
#pragma unroll
  for (int s = 0; s < MS_LEVELS - 1; ++s) {
    h[s] = 0.f;
    h[MS_LEVELS + s] = (float)(chain * out * (double)w[s] / (double)mc[s]);
  }
  h[MS_LEVELS - 1] = (float)(chain * out * w4 / (double)ms[MS_LEVELS - 1]);
  h[2 * MS_LEVELS - 1] = 0.f;
  result[row] = (float)out;
}

// One level of the backward.  SSIM_TERM: the SSIM map's gradient times d out / d ssim_level (the last level), else the cs map's times
// d out / d cs_level; g_coarse is NULL on the last level.
template <bool SSIM_TERM>
__global__ __launch_bounds__(NT) void msssim_bwd_level(const float* __restrict__ sr, const float* __restrict__ hr,
                                                       const float* __restrict__ g_out, const float* __restrict__ head, int level,
                                                       const float* __restrict__ g_coarse, float* __restrict__ g_sr, int C, int H, int W,
                                                       int taps, float inv_n, int vec_ok) {
  const int row = blockIdx.z / C;
  const float* h = head + (size_t)row * MS_HEAD;
  bwd_tile<SSIM_TERM>(sr, hr, reinterpret_cast<const unsigned*>(h)[2 * MS_LEVELS + level],
                      (g_out[row] * h[SSIM_TERM ? level : MS_LEVELS + level]) * inv_n, g_coarse, g_sr, H, W, taps, vec_ok);
}

// the limits of every entry point: rows * C is grid z; in-plane indices are int
bool too_big(int rows, int C, int H, int W) { return (int64_t)rows * C > 65535 || (int64_t)H * W > 0x7fffffffLL; }

int ssim_check(int rows, int C, int H, int W) {
  if (rows <= 0 || C <= 0 || H < WIN || W < WIN) return SAVFI_E_SHAPE;
  return too_big(rows, C, H, W) ? SAVFI_E_TOOBIG : SAVFI_OK;
}

// NULL, then SHAPE, UNSUPPORTED, TOOBIG.  The reference pools once more after the fifth level: 32 is the smallest legal size.
int msssim_check(int rows, int C, int H, int W, int range_mode) {
  if (rows <= 0 || C <= 0 || H < 32 || W < 32) return SAVFI_E_SHAPE;
  if (range_mode < 0 || range_mode > SAVFI_SSIM_RANGE_FIXED + 3) return SAVFI_E_UNSUPPORTED;
  return too_big(rows, C, H, W) ? SAVFI_E_TOOBIG : SAVFI_OK;
}

// float4 loads of both operands' rows: 16-byte aligned planes of a width that is a multiple of four
int vec4_ok(const float* a, const float* b, int W) { return ((((uintptr_t)a | (uintptr_t)b) & 15u) == 0) && (W % 4 == 0); }

// The range pass over `rows` rows of n elements each -> ext, *eb (max, min) pairs per row
int launch_range(const float* sr, float* ext, int rows, int64_t n, hipStream_t st, int* eb) {
  *eb = (int)((n + RANGE_PER_BLOCK - 1) / RANGE_PER_BLOCK);
  if (*eb > RANGE_MAX_BLOCKS) *eb = RANGE_MAX_BLOCKS;
  const long long per_block = (((n + *eb - 1) / *eb) + 3) & ~3LL;
  const int rvec = (((uintptr_t)sr & 15u) == 0) && (rows == 1 || n % 4 == 0);
  hipLaunchKernelGGL(ssim_range, dim3(*eb, rows), dim3(NT), 0, st, sr, ext, (long long)n, per_block, rvec);
  return savfi_launch_status();
}

// Where everything lies in the scratch, in 32-bit words (every region starts on a multiple of four words).  The same for every range mode.
struct MsPlan {
  int h[MS_LEVELS], w[MS_LEVELS], taps[MS_LEVELS], tx[MS_LEVELS], ty[MS_LEVELS];
  int64_t img1[MS_LEVELS], img2[MS_LEVELS], grad[MS_LEVELS];      // levels 1 .. 4
  int64_t partial[MS_LEVELS], ext[MS_LEVELS];
  int64_t words;
};

MsPlan msssim_plan(int rows, int C, int H, int W) {
  MsPlan p;
  const int64_t planes = (int64_t)rows * C;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  int64_t at = up4((int64_t)rows * MS_HEAD);
  for (int s = 0; s < MS_LEVELS; ++s) {
    p.h[s] = H >> s;
    p.w[s] = W >> s;
    p.taps[s] = p.h[s] < WIN || p.w[s] < WIN ? (p.h[s] < p.w[s] ? p.h[s] : p.w[s]) : WIN;
    p.tx[s] = savfi_cdiv(p.w[s] - p.taps[s] + 1, TW);
    p.ty[s] = savfi_cdiv(p.h[s] - p.taps[s] + 1, TH);
  }
  for (int s = 1; s < MS_LEVELS; ++s) {
    const int64_t n = up4(planes * p.h[s] * p.w[s]);
    p.img1[s] = at;
    p.img2[s] = at + n;
    p.grad[s] = at + 2 * n;
    at += 3 * n;
  }
  for (int s = 0; s < MS_LEVELS; ++s) {
    p.partial[s] = at;
    at += up4(2 * planes * p.tx[s] * p.ty[s]);
  }
  for (int s = 0; s < MS_LEVELS; ++s) {
    p.ext[s] = at;
    at += up4(s == 0 ? 2 * (int64_t)rows * RANGE_MAX_BLOCKS : 2 * planes * p.tx[s - 1] * p.ty[s - 1]);
  }
  p.words = at;
  return p;
}

}  // namespace

extern "C" int64_t savfi_ssim_scratch_floats(int rows, int C, int H, int W) {
  if (int e = ssim_check(rows, C, H, W)) return e;
  // per-workgroup partial sums + per-block partial extrema (max, min) of the range pass; the same for every range mode
  return (int64_t)rows * C * savfi_cdiv(W - HALO, TW) * savfi_cdiv(H - HALO, TH) + 2 * (int64_t)rows * RANGE_MAX_BLOCKS;
}

extern "C" int savfi_ssim_loss_f32(const float* sr, const float* hr, float* result, uint32_t* range_word, float* scratch, int rows, int C,
                                   int H, int W, int range_mode, void* stream) {
  if (!sr || !hr || !result || !range_word || !scratch) return SAVFI_E_NULL;
  if (int e = ssim_check(rows, C, H, W)) return e;
  if (range_mode < 0 || range_mode > SAVFI_SSIM_RANGE_FIXED + 3) return SAVFI_E_UNSUPPORTED;
  if (range_mode == SAVFI_SSIM_RANGE_BATCH) {      // one loss over everything: the samples are further channel planes
    C *= rows;
    rows = 1;
  }
  const int fixed_cls = range_mode >= SAVFI_SSIM_RANGE_FIXED ? range_mode - SAVFI_SSIM_RANGE_FIXED : -1;
  const int tx = savfi_cdiv(W - HALO, TW), ty = savfi_cdiv(H - HALO, TH);
  float* partial = scratch;
  float* ext = scratch + (int64_t)rows * C * tx * ty;
  hipStream_t st = (hipStream_t)stream;
  int eb = 0;
  if (fixed_cls < 0) {
    if (int e = launch_range(sr, ext, rows, (int64_t)C * H * W, st, &eb)) return e;
  }
  hipLaunchKernelGGL(ssim_fwd, dim3(tx, ty, rows * C), dim3(NT), 0, st, sr, hr, ext, eb, fixed_cls, range_word, partial, C, H, W,
                     vec4_ok(sr, hr, W));
  if (int e = savfi_launch_status()) return e;
  const int64_t n_out = (int64_t)C * (H - HALO) * (W - HALO);
  hipLaunchKernelGGL(ssim_finish, dim3(rows), dim3(64), 0, st, partial, result, C * tx * ty, (float)n_out);
  return savfi_launch_status();
}

extern "C" int savfi_ssim_loss_bwd_f32(const float* sr, const float* hr, const float* g_loss, const uint32_t* range_word, float* g_sr,
                                       int rows, int C, int H, int W, void* stream) {
  if (!sr || !hr || !g_loss || !range_word || !g_sr) return SAVFI_E_NULL;
  if (int e = ssim_check(rows, C, H, W)) return e;
  const int64_t n_out = (int64_t)C * (H - HALO) * (W - HALO);
  const float inv_2n = (float)(1.0 / (2.0 * (double)n_out));
  hipLaunchKernelGGL(ssim_bwd, dim3(savfi_cdiv(W, BW), savfi_cdiv(H, BH), rows * C), dim3(NT), 0, (hipStream_t)stream, sr, hr, g_loss,
                     range_word, g_sr, C, H, W, inv_2n, vec4_ok(sr, hr, W));
  return savfi_launch_status();
}

extern "C" int64_t savfi_psnr_ssim_scratch_bytes(int rows, int C, int H, int W) {
  if (int e = ssim_check(rows, C, H, W)) return e;
  // per workgroup: one float (SSIM partial sum) and one 32-bit integer (squared-error partial)
  return (int64_t)rows * C * savfi_cdiv(W - HALO, TW) * savfi_cdiv(H - HALO, TH) * (int64_t)(sizeof(float) + sizeof(unsigned));
}

extern "C" int savfi_psnr_ssim_f32(const float* pred, const float* target, float* result, unsigned long long* sq_sum, void* scratch,
                                   int rows, int C, int H, int W, void* stream) {
  if (!pred || !target || !result || !scratch) return SAVFI_E_NULL;
  if (int e = ssim_check(rows, C, H, W)) return e;
  const int tx = savfi_cdiv(W - HALO, TW), ty = savfi_cdiv(H - HALO, TH);
  float* partial = (float*)scratch;
  unsigned* sq_partial = (unsigned*)(partial + (int64_t)rows * C * tx * ty);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(metric_tile, dim3(tx, ty, rows * C), dim3(NT), 0, st, pred, target, partial, sq_partial, C, H, W,
                     vec4_ok(pred, target, W));
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(metric_finish, dim3(rows), dim3(64), 0, st, partial, sq_partial, result, sq_sum, C * tx * ty,
                     (float)((int64_t)C * (H - HALO) * (W - HALO)), (double)C * H * W);
  return savfi_launch_status();
}

extern "C" int64_t savfi_msssim_scratch_bytes(int rows, int C, int H, int W) {
  if (int e = msssim_check(rows, C, H, W, SAVFI_SSIM_RANGE_PER_ROW)) return e;
  return msssim_plan(rows, C, H, W).words * (int64_t)sizeof(float);
}

extern "C" int savfi_msssim_f32(const float* img1, const float* img2, float* result, void* scratch, int rows, int C, int H, int W,
                                int range_mode, int normalize, int quantize, void* stream) {
  if (!img1 || !img2 || !result || !scratch) return SAVFI_E_NULL;
  if (int e = msssim_check(rows, C, H, W, range_mode)) return e;
  const MsPlan p = msssim_plan(rows, C, H, W);
  float* base = (float*)scratch;
  if (range_mode == SAVFI_SSIM_RANGE_BATCH) {      // one value over everything: the samples are further channel planes
    C *= rows;
    rows = 1;
  }
  const int fixed_cls = range_mode >= SAVFI_SSIM_RANGE_FIXED ? range_mode - SAVFI_SSIM_RANGE_FIXED : -1;
  hipStream_t st = (hipStream_t)stream;
  int eb = 0;
  if (fixed_cls < 0) {
    if (int e = launch_range(img1, base + p.ext[0], rows, (int64_t)C * H * W, st, &eb)) return e;
  }
  MsFinish f;
  const float* x = img1;
  const float* y = img2;
  for (int s = 0; s < MS_LEVELS; ++s) {
    const bool last = s + 1 == MS_LEVELS;
    const int vec_ok = vec4_ok(x, y, p.w[s]);
    float* o1 = last ? nullptr : base + p.img1[s + 1];
    float* o2 = last ? nullptr : base + p.img2[s + 1];
    float* eo = last ? nullptr : base + p.ext[s + 1];
    const dim3 grid(p.tx[s], p.ty[s], rows * C);
    if (s == 0 && quantize) {
      hipLaunchKernelGGL(msssim_level<true>, grid, dim3(NT), 0, st, x, y, base + p.ext[s], eb, fixed_cls, (unsigned*)base, s,
                         base + p.partial[s], o1, o2, eo, C, p.h[s], p.w[s], p.taps[s], vec_ok);
    } else {
      hipLaunchKernelGGL(msssim_level<false>, grid, dim3(NT), 0, st, x, y, base + p.ext[s], eb, fixed_cls, (unsigned*)base, s,
                         base + p.partial[s], o1, o2, eo, C, p.h[s], p.w[s], p.taps[s], vec_ok);
    }
    if (int e = savfi_launch_status()) return e;
    f.partial[s] = p.partial[s];
    f.blocks[s] = C * p.tx[s] * p.ty[s];
    f.wgs[s] = rows * C * p.tx[s] * p.ty[s];
    f.n[s] = (float)((int64_t)C * (p.h[s] - p.taps[s] + 1) * (p.w[s] - p.taps[s] + 1));
    eb = f.blocks[s];      // the next level's extrema: one pair per workgroup of this one
    x = o1;
    y = o2;
  }
  hipLaunchKernelGGL(msssim_finish, dim3(rows), dim3(64), 0, st, base, base, result, f, normalize ? 1 : 0);
  return savfi_launch_status();
}

extern "C" int savfi_msssim_bwd_f32(const float* img1, const float* img2, const float* g_out, void* scratch, float* g_img1, int rows,
                                    int C, int H, int W, int range_mode, void* stream) {
  if (!img1 || !img2 || !g_out || !scratch || !g_img1) return SAVFI_E_NULL;
  if (int e = msssim_check(rows, C, H, W, range_mode)) return e;
  const MsPlan p = msssim_plan(rows, C, H, W);
  float* base = (float*)scratch;
  if (range_mode == SAVFI_SSIM_RANGE_BATCH) {
    C *= rows;
    rows = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int s = MS_LEVELS - 1; s >= 0; --s) {
    const bool last = s + 1 == MS_LEVELS;
    const float* x = s ? base + p.img1[s] : img1;
    const float* y = s ? base + p.img2[s] : img2;
    float* gx = s ? base + p.grad[s] : g_img1;
    const float* gc = last ? nullptr : base + p.grad[s + 1];
    const int vec_ok = vec4_ok(x, y, p.w[s]);
    const float inv_n = (float)(1.0 / (double)((int64_t)C * (p.h[s] - p.taps[s] + 1) * (p.w[s] - p.taps[s] + 1)));
    const dim3 grid(savfi_cdiv(p.w[s], BW), savfi_cdiv(p.h[s], BH), rows * C);
    if (last) {
      hipLaunchKernelGGL(msssim_bwd_level<true>, grid, dim3(NT), 0, st, x, y, g_out, base, s, gc, gx, C, p.h[s], p.w[s], p.taps[s], inv_n,
                         vec_ok);
    } else {
      hipLaunchKernelGGL(msssim_bwd_level<false>, grid, dim3(NT), 0, st, x, y, g_out, base, s, gc, gx, C, p.h[s], p.w[s], p.taps[s], inv_n,
                         vec_ok);
    }
    if (int e = savfi_launch_status()) return e;
  }
  return SAVFI_OK;
}
