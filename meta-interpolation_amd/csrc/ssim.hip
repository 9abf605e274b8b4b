// Fused SSIM loss term (and its gradient) for gfx950: what the reference's Loss wrapper computes for 'SSIM'
// (loss.py:294 -> pytorch_msssim/__init__.py:7-131): an 11 x 11 Gaussian window (sigma 1.5), valid correlation, over the five
// moment maps of prediction and target, a rational expression per pixel, mean, (1 - mean) / 2 -- with the dynamic range L
// decided from the prediction's data on every call (:21-31).  Composed from library ops that is 5 depthwise convolutions,
// ~15 element-wise launches, a max / min with a host decision, and twice that again in autograd's backward.
//
// Here: `rows` independent losses per launch (one per sample: tasks in lockstep, the two support triplets of a step).
//   ssim_range   max / min of every row of the prediction -> per-block partial extrema (skipped for a fixed L)
//   ssim_fwd     a workgroup owns a 16 x 64 tile of SSIM values of one channel plane: 26 x 76 patches of both images into LDS
//                (float4 where the operands allow), 11-tap row pass over the five products into LDS, column pass out of LDS
//                (separable: 22 instead of 121 multiply-adds per moment), map, one partial sum per workgroup.  It reduces
//                the row's partial extrema itself (no host read: the op is capturable) and publishes the row's range word.
//   ssim_finish  adds a row's partial sums in a fixed order (no float atomics: bit-reproducible) -> (1 - sum / n) / 2
//   ssim_bwd     one launch: a workgroup owns 16 x 32 pixels of d loss / d sr, recomputes the moments on the tile grown by
//                the 10-pixel halo (26 x 42 SSIM positions from 36 x 56 patches), forms the three coefficient planes a, b, c in
//                LDS and applies the adjoint window (row pass, column pass) to them:
//                  d loss / d sr = -(g / (2 n)) (G^T[a] + 2 sr G^T[b] + hr G^T[c])
//                  b = d map / d s1, c = d map / d s12, a = (d map / d mu1 at fixed s1, s12) - 2 mu1 b - mu2 c
//                Nothing is kept from the forward but the two images and the range word.
// The PSNR / SSIM evaluation metric (utils.py:171-204: quantize + calc_psnr + ssim(val_range=255)) is the forward tile once more:
//   metric_tile    fwd_tile<METRIC>: both unit-range images quantised to 0 .. 255 as they are loaded into LDS, L = 255 fixed (no range
//                  pass, no range word), and next to the SSIM partial sum the integer sum of squared differences of the pixels the
//                  workgroup owns
//   metric_finish  per row: SSIM partial sums in ssim_finish's order -> mean; integer partials as 64 bits -> S, mse = S / (65025 n)
// Every window sum is accumulated tap 0 .. 10 in the same association for every pixel, whatever its place in a tile.
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

// The window of pytorch_msssim.create_window: taps exp(-(i - 5)^2 / 4.5) evaluated in double, rounded to fp32, divided by
// their fp32 sum.  (The reference multiplies the outer product out in fp32; the separable passes here round differently by
// < 1 ulp per weight.)
__device__ __constant__ float G[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                        0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

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

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, SAVFI_WAVE));
  return x;
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

// The five window sums of one position of the 11-tap row pass: x, y, x^2, y^2, xy.
__device__ __forceinline__ void row_taps(const float* __restrict__ x, const float* __restrict__ y, float (&s)[5]) {
  s[0] = s[1] = s[2] = s[3] = s[4] = 0.f;
#pragma unroll
  for (int k = 0; k < WIN; ++k) {
    const float g = G[k], a = x[k], b = y[k];
    s[0] = fmaf(g, a, s[0]);
    s[1] = fmaf(g, b, s[1]);
    s[2] = fmaf(g, a * a, s[2]);
    s[3] = fmaf(g, b * b, s[3]);
    s[4] = fmaf(g, a * b, s[4]);
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

// One forward tile, for both kernels below.  grid (tiles_x, tiles_y, rows * C); partial[(z * tiles_y + by) * tiles_x + bx].
// METRIC: the patches are quantised on load, the range class is 2 (L = 255: no extrema, no range word), and the workgroup also adds
// (q_p - q_t)^2 as an integer over the pixels it owns -> sq_partial (same index).  Every pixel of the plane has one owner: the
// tiles step over the SSIM positions, so the last tile row / column also own the 10 trailing pixel rows / columns, which lie
// inside their patch (<= 26 x 74 pixels * 65025 < 2^27: the 32-bit sum is exact).  A NaN among the owned pixels -> SQ_NAN.
template <bool METRIC>
__device__ __forceinline__ void fwd_tile(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ ext,
                                         int ext_blocks, int fixed_cls, unsigned* __restrict__ range_word, float* __restrict__ partial,
                                         unsigned* __restrict__ sq_partial, int C, int H, int W, int vec_ok) {
  __shared__ __attribute__((aligned(16))) float px[PH * PW];
  __shared__ __attribute__((aligned(16))) float py[PH * PW];
  __shared__ float rf[5][PH][TW];
  __shared__ float red[2 * NW];
  const int z = blockIdx.z, row = z / C;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int Ho = H - HALO, Wo = W - HALO;
  const size_t plane = (size_t)z * H * W;
  load_patch<PH, PW, METRIC>(sr + plane, px, y0, x0, H, W, vec_ok);
  load_patch<PH, PW, METRIC>(hr + plane, py, y0, x0, H, W, vec_ok);
  // the row's range class: from its partial extrema (<= NT of them), or the fixed one
  unsigned cls = (unsigned)fixed_cls;
  if (!METRIC && fixed_cls < 0) {
    float hi = -INFINITY, lo = INFINITY;
    if ((int)threadIdx.x < ext_blocks) {
      hi = ext[((size_t)row * ext_blocks + threadIdx.x) * 2];
      lo = ext[((size_t)row * ext_blocks + threadIdx.x) * 2 + 1];
    }
    block_extrema(hi, lo, red);
    cls = (lo < -0.5f ? 1u : 0u) | (hi > 128.f ? 2u : 0u);
  }
  if (!METRIC && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && z == row * C) range_word[row] = cls;
  float C1, C2;
  ssim_constants(cls, C1, C2);
  __syncthreads();

  if constexpr (METRIC) {
    __shared__ unsigned sq_red[NW];
    const int own_h = blockIdx.y + 1 == gridDim.y ? H - y0 : TH, own_w = blockIdx.x + 1 == gridDim.x ? W - x0 : TW;
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
      sq_partial[((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = bad ? SQ_NAN : tot;
    }
  }

  for (int i = threadIdx.x; i < PH * TW; i += NT) {
    const int r = i / TW, c = i - r * TW;
    float s[5];
    row_taps(px + r * PW + c, py + r * PW + c, s);
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
      for (int k = 0; k < WIN; ++k) acc = fmaf(G[k], v[o + k], acc);
      mom[o][p] = acc;
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    float r1, r2, B1, B2;
    const float v = ssim_value(mom[o], C1, C2, r1, r2, B1, B2);
    if (y0 + r0 + o < Ho && x0 + c < Wo) sum += v;
  }
  const float tot = block_sum<NW>(sum, red);
  if (threadIdx.x == 0) partial[((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(NT) void ssim_fwd(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ ext,
                                               int ext_blocks, int fixed_cls, unsigned* __restrict__ range_word,
                                               float* __restrict__ partial, int C, int H, int W, int vec_ok) {
  fwd_tile<false>(sr, hr, ext, ext_blocks, fixed_cls, range_word, partial, nullptr, C, H, W, vec_ok);
}

// the metric's tile kernel: unit-range pred / target in, SSIM partial sum and integer squared-error partial out
__global__ __launch_bounds__(NT) void metric_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                  float* __restrict__ partial, unsigned* __restrict__ sq_partial, int C, int H, int W,
                                                  int vec_ok) {
  fwd_tile<true>(pred, target, nullptr, 0, 2, nullptr, partial, sq_partial, C, H, W, vec_ok);
}

// result[row] = (1 - (the row's partial sums, lane-strided then a butterfly: always the same order) / n) / 2
__global__ __launch_bounds__(64) void ssim_finish(const float* __restrict__ partial, float* __restrict__ result, int blocks, float n) {
  const float* p = partial + (size_t)blockIdx.x * blocks;
  float acc = 0.f;
  for (int i = threadIdx.x; i < blocks; i += 64) acc += p[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) result[blockIdx.x] = (1.f - acc / n) / 2.f;
}

// result[row] = {mse, ssim}: the SSIM partial sums in ssim_finish's order / n_out; the squared-error partials as 64-bit integers
// (exact, whatever the order) -> S / (65025 n_pix) in double.  A NaN word makes the mse NaN (the SSIM sum then is NaN by itself:
// every pixel lies in some window) and sq_sum[row] all ones.
__global__ __launch_bounds__(64) void metric_finish(const float* __restrict__ partial, const unsigned* __restrict__ sq_partial,
                                                    float* __restrict__ result, unsigned long long* __restrict__ sq_sum, int blocks,
                                                    float n_out, double n_pix) {
  const float* p = partial + (size_t)blockIdx.x * blocks;
  const unsigned* q = sq_partial + (size_t)blockIdx.x * blocks;
  float acc = 0.f;
  unsigned long long S = 0;
  int bad = 0;
  for (int i = threadIdx.x; i < blocks; i += 64) {
    acc += p[i];
    const unsigned w = q[i];
    bad |= w == SQ_NAN;
    S += w;
  }
  acc = wave_sum(acc);
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

// grid (cdiv(W, BW), cdiv(H, BH), rows * C)
__global__ __launch_bounds__(NT) void ssim_bwd(const float* __restrict__ sr, const float* __restrict__ hr, const float* __restrict__ g_loss,
                                               const unsigned* __restrict__ range_word, float* __restrict__ g_sr, int C, int H, int W,
                                               float inv_2n, int vec_ok) {
  __shared__ __attribute__((aligned(16))) float px[QH * QW];
  __shared__ __attribute__((aligned(16))) float py[QH * QW];
  __shared__ float rf[5][QH][CW];                  // row-filtered moments; later the row-filtered coefficients [3][CH][BW]
  __shared__ float coef[3][CH][CW];
  float(*ar)[CH][BW] = reinterpret_cast<float(*)[CH][BW]>(&rf[0][0][0]);
  static_assert(3 * CH * BW <= 5 * QH * CW, "the row-filtered coefficients reuse the moments' planes");
  const int z = blockIdx.z, row = z / C;
  const int y0 = blockIdx.y * BH, x0 = blockIdx.x * BW;
  const int Ho = H - HALO, Wo = W - HALO;
  const size_t plane = (size_t)z * H * W;
  load_patch<QH, QW>(sr + plane, px, y0 - HALO, x0 - QX, H, W, vec_ok);
  load_patch<QH, QW>(hr + plane, py, y0 - HALO, x0 - QX, H, W, vec_ok);
  float C1, C2;
  ssim_constants(range_word[row], C1, C2);
  __syncthreads();

  // moments, row pass: SSIM column cc is position x0 - 10 + cc, its window starts at patch column cc + 2
  for (int i = threadIdx.x; i < QH * CW; i += NT) {
    const int r = i / CW, cc = i - r * CW;
    float s[5];
    row_taps(px + r * QW + cc + (QX - HALO), py + r * QW + cc + (QX - HALO), s);
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
        for (int k = 0; k < WIN; ++k) acc = fmaf(G[k], rf[p][cr + k][cc], acc);
        m[p] = acc;
      }
      float r1, r2, B1, B2;
      const float v = ssim_value(m, C1, C2, r1, r2, B1, B2);
      {
#pragma clang fp contract(off)
        // an identical pair gives v = r1 = r2 = 1: then c == -2 b, dm == 0 and a == 0 exactly, and so is the gradient
        b = -v / B2;
        c = (2.f * r1) / B2;
        const float dm = ((2.f * m[1]) * r2) / B1 - ((2.f * m[0]) * v) / B1;
        a = (dm - (2.f * m[0]) * b) - m[1] * c;
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
      for (int k = 0; k < WIN; ++k) acc = fmaf(G[k], coef[p][cr][ix + HALO - k], acc);
      ar[p][cr][ix] = acc;
    }
  }
  __syncthreads();

  // adjoint, column pass, and the gradient
  const float scale = -g_loss[row] * inv_2n;
  for (int i = threadIdx.x; i < BH * BW; i += NT) {
    const int iy = i / BW, ix = i - iy * BW;
    const int gy = y0 + iy, gx = x0 + ix;
    float t[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmaf(G[k], ar[p][iy + HALO - k][ix], acc);
      t[p] = acc;
    }
    if (gy < H && gx < W) {
#pragma clang fp contract(off)
      const float x = px[(iy + HALO) * QW + ix + QX], y = py[(iy + HALO) * QW + ix + QX];
      g_sr[plane + (size_t)gy * W + gx] = scale * ((t[0] + (2.f * x) * t[1]) + y * t[2]);
    }
  }
}

int ssim_check(int rows, int C, int H, int W) {
  if (rows <= 0 || C <= 0 || H < WIN || W < WIN) return SAVFI_E_SHAPE;
  if ((int64_t)rows * C > 65535 || (int64_t)H * W > 0x7fffffffLL) return SAVFI_E_TOOBIG;      // grid z; in-plane indices are int
  return SAVFI_OK;
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
  const int64_t n = (int64_t)C * H * W;
  const int vec_ok = ((((uintptr_t)sr | (uintptr_t)hr) & 15u) == 0) && (W % 4 == 0);
  float* partial = scratch;
  float* ext = scratch + (int64_t)rows * C * tx * ty;
  hipStream_t st = (hipStream_t)stream;
  int eb = 0;
  if (fixed_cls < 0) {
    eb = (int)((n + RANGE_PER_BLOCK - 1) / RANGE_PER_BLOCK);
    if (eb > RANGE_MAX_BLOCKS) eb = RANGE_MAX_BLOCKS;
    const long long per_block = (((n + eb - 1) / eb) + 3) & ~3LL;
    const int rvec = (((uintptr_t)sr & 15u) == 0) && (rows == 1 || n % 4 == 0);
    hipLaunchKernelGGL(ssim_range, dim3(eb, rows), dim3(NT), 0, st, sr, ext, (long long)n, per_block, rvec);
    if (int e = savfi_launch_status()) return e;
  }
  hipLaunchKernelGGL(ssim_fwd, dim3(tx, ty, rows * C), dim3(NT), 0, st, sr, hr, ext, eb, fixed_cls, range_word, partial, C, H, W, vec_ok);
  if (int e = savfi_launch_status()) return e;
  const int64_t n_out = (int64_t)C * (H - HALO) * (W - HALO);
  hipLaunchKernelGGL(ssim_finish, dim3(rows), dim3(64), 0, st, partial, result, C * tx * ty, (float)n_out);
  return savfi_launch_status();
}

extern "C" int savfi_ssim_loss_bwd_f32(const float* sr, const float* hr, const float* g_loss, const uint32_t* range_word, float* g_sr,
                                       int rows, int C, int H, int W, void* stream) {
  if (!sr || !hr || !g_loss || !range_word || !g_sr) return SAVFI_E_NULL;
  if (int e = ssim_check(rows, C, H, W)) return e;
  const int vec_ok = ((((uintptr_t)sr | (uintptr_t)hr) & 15u) == 0) && (W % 4 == 0);
  const int64_t n_out = (int64_t)C * (H - HALO) * (W - HALO);
  const float inv_2n = (float)(1.0 / (2.0 * (double)n_out));
  hipLaunchKernelGGL(ssim_bwd, dim3(savfi_cdiv(W, BW), savfi_cdiv(H, BH), rows * C), dim3(NT), 0, (hipStream_t)stream, sr, hr, g_loss,
                     range_word, g_sr, C, H, W, inv_2n, vec_ok);
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
  const int vec_ok = ((((uintptr_t)pred | (uintptr_t)target) & 15u) == 0) && (W % 4 == 0);
  float* partial = (float*)scratch;
  unsigned* sq_partial = (unsigned*)(partial + (int64_t)rows * C * tx * ty);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(metric_tile, dim3(tx, ty, rows * C), dim3(NT), 0, st, pred, target, partial, sq_partial, C, H, W, vec_ok);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(metric_finish, dim3(rows), dim3(64), 0, st, partial, sq_partial, result, sq_sum, C * tx * ty,
                     (float)((int64_t)C * (H - HALO) * (W - HALO)), (double)C * H * W);
  return savfi_launch_status();
}
