// AdaCoF's deformable-tap op and its parameter gradients for gfx950 (definition: include/savfi_hip.h, tests/adacof_ref.py).
//   x [N, C, Hp, Wp] (the frame, padded by the caller), w, a, b [N, F^2, H, W], Hp = H + (F - 1) d, Wp = W + (F - 1) d.
//   For pixel (y, x) and tap t = k F + l:  sy = float(y + k d) + a_t, sx = float(x + l d) + b_t (ONE fp32 addition each), clamped in
//   float to [-1, Hp] / [-1, Wp], cell iy = floor(sy), ty = sy - iy (likewise ix, tx), the four texel indices clamped to the frame
//   (border replicate), S_c(t) the bilinear sample, out_c = sum_t w_t S_c(t) with the taps added in the order t = 0 .. F^2 - 1.
//
// Forward: adacof_fwd, grid (N * cdiv(H, 4) * cdiv(W, 64)), 256 threads, one output pixel per thread of a tile of 4 rows x 64
// columns: consecutive lanes own consecutive x, so a wave reads one 256-byte row piece of every one of the 3 F^2 parameter planes;
// they are read once and fetched non-temporally.  The frame gathers are plain loads: a padded 256 x 448 frame is 1.4 MB and stays in cache.
// Backward: adacof_bwd, the same grid and walk, ONE launch for whichever of g_w, g_a, g_b are wanted; g_out[C] is loaded once per
// pixel, three values leave per tap.  No gradient of the frame is built.
//
// The float clamp comes BEFORE every conversion to an integer, and the conversion itself reads fmaxf(floor, -1), which is -1 for a
// NaN: +-inf, +-1e30 and NaN offsets index inside the frame.  A NaN coordinate leaves ty / tx NaN, so the pixel's `out`, the tap's
// g_w and (through the term 0 * (ty + tx), which is +0 for every finite coordinate) both offset gradients of the tap are NaN.
// Where both texel indices of an axis clamp to one texel the differences below are x - x = 0: the offset gradient is exactly 0.
//
// fp32 throughout, every operation rounded on its own (contraction is switched off for this file: the tap sum is the running sum
// the definition writes, product first); no atomics, no cleared memory, no host read: capturable, bit-reproducible, every element
// written exactly once.  All global accesses are scalar 4-byte ones: operands 4 bytes off a 16-byte boundary give the same bits.
#include "common.h"

#pragma clang fp contract(off)

namespace {

#ifndef SAVFI_ADACOF_TW            // A/B (tools/build_variant.sh): the tile's width, 32 or 64
#define SAVFI_ADACOF_TW 64
#endif
constexpr int NT = 256;
constexpr int TW = SAVFI_ADACOF_TW;  // tile: 64 columns (a wave owns one row: 256 contiguous bytes of every parameter plane) ...
constexpr int TH = NT / TW;          // ... by 4 rows; 256 x 448 gives 448 workgroups.  Measured against 8 rows x 32 columns (two 128-byte
                                     // pieces per wave): equal at 256 x 448, 3 % / 5 % faster forward / forward + backward at 720p

__device__ __forceinline__ float stream_load(const float* p) { return __builtin_nontemporal_load(p); }

// One axis of a tap: coordinate s = base + offset -> texel indices i0, i1 inside [0, size - 1] and the weight t of i1 (NaN for a NaN s).
__device__ __forceinline__ void axis(int base, float offset, int size, int& i0, int& i1, float& t) {
  float s = (float)base + offset;
  s = s < -1.f ? -1.f : (s > (float)size ? (float)size : s);      // NaN passes; everything else is now in [-1, size]
  const float fl = floorf(s);
  t = s - fl;
  const int i = (int)fmaxf(fl, -1.f);                             // in [-1, size]; a NaN floor reads -1
  i0 = min(max(i, 0), size - 1);
  i1 = i < 0 ? 0 : min(i0 + 1, size - 1);                         // clamp(i + 1, 0, size - 1) without forming i + 1
}

struct Pixel {
  int n, y, x;
  bool inside;
};

__device__ __forceinline__ Pixel pixel_of_thread(int H, int W, int tx, int tiles) {
  Pixel p;
  p.n = blockIdx.x / tiles;
  const int tile = blockIdx.x - p.n * tiles;
  p.y = (tile / tx) * TH + threadIdx.x / TW;
  p.x = (tile % tx) * TW + (threadIdx.x & (TW - 1));
  p.inside = p.y < H && p.x < W;
  return p;
}

template <int C>
__global__ __launch_bounds__(NT) void adacof_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ a,
                                                 const float* __restrict__ b, float* __restrict__ out, int H, int W, int F, int d,
                                                 int tx, int tiles) {
  const Pixel p = pixel_of_thread(H, W, tx, tiles);
  if (!p.inside) return;
  const int Hp = H + (F - 1) * d, Wp = W + (F - 1) * d;
  const size_t hw = (size_t)H * W, at = (size_t)p.y * W + p.x;
  const int plane = Hp * Wp;
  const float* xs = x + (size_t)p.n * C * plane;
  const size_t taps = (size_t)p.n * F * F * hw + at;
  const float* wp = w + taps;
  const float* ap = a + taps;
  const float* bp = b + taps;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll 1
  for (int k = 0; k < F; ++k) {
#pragma unroll 1
    for (int l = 0; l < F; ++l) {
      const float wt = stream_load(wp), av = stream_load(ap), bv = stream_load(bp);
      wp += hw, ap += hw, bp += hw;
      int i0, i1, j0, j1;
      float ty, tx_;
      axis(p.y + k * d, av, Hp, i0, i1, ty);
      axis(p.x + l * d, bv, Wp, j0, j1, tx_);
      const float uy = 1.f - ty, ux = 1.f - tx_;
      const int r0 = i0 * Wp, r1 = i1 * Wp;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* xc = xs + c * plane;
        const float top = ux * xc[r0 + j0] + tx_ * xc[r0 + j1];
        const float bot = ux * xc[r1 + j0] + tx_ * xc[r1 + j1];
        const float s = uy * top + ty * bot;
        acc[c] = acc[c] + wt * s;
      }
    }
  }
  float* o = out + (size_t)p.n * C * hw + at;
#pragma unroll
  for (int c = 0; c < C; ++c) o[c * hw] = acc[c];
}

template <int C>
__global__ __launch_bounds__(NT) void adacof_bwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ a,
                                                 const float* __restrict__ b, const float* __restrict__ g_out, float* __restrict__ g_w,
                                                 float* __restrict__ g_a, float* __restrict__ g_b, int H, int W, int F, int d, int tx,
                                                 int tiles) {
  const Pixel p = pixel_of_thread(H, W, tx, tiles);
  if (!p.inside) return;
  const int Hp = H + (F - 1) * d, Wp = W + (F - 1) * d;
  const size_t hw = (size_t)H * W, at = (size_t)p.y * W + p.x;
  const int plane = Hp * Wp;
  const float* xs = x + (size_t)p.n * C * plane;
  size_t tap = (size_t)p.n * F * F * hw + at;
  const bool offsets = g_a != nullptr || g_b != nullptr;
  float g[C];
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = stream_load(g_out + (size_t)p.n * C * hw + c * hw + at);
#pragma unroll 1
  for (int k = 0; k < F; ++k) {
#pragma unroll 1
    for (int l = 0; l < F; ++l, tap += hw) {
      const float av = stream_load(a + tap), bv = stream_load(b + tap);
      int i0, i1, j0, j1;
      float ty, tx_;
      axis(p.y + k * d, av, Hp, i0, i1, ty);
      axis(p.x + l * d, bv, Wp, j0, j1, tx_);
      const float uy = 1.f - ty, ux = 1.f - tx_;
      const int r0 = i0 * Wp, r1 = i1 * Wp;
      float sw = 0.f, sa = 0.f, sb = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* xc = xs + c * plane;
        const float x00 = xc[r0 + j0], x01 = xc[r0 + j1], x10 = xc[r1 + j0], x11 = xc[r1 + j1];
        const float s = uy * (ux * x00 + tx_ * x01) + ty * (ux * x10 + tx_ * x11);
        const float da = ux * (x10 - x00) + tx_ * (x11 - x01);
        const float db = uy * (x01 - x00) + ty * (x11 - x10);
        sw = c == 0 ? g[c] * s : sw + g[c] * s;
        sa = c == 0 ? g[c] * da : sa + g[c] * da;
        sb = c == 0 ? g[c] * db : sb + g[c] * db;
      }
      if (g_w) g_w[tap] = sw;
      if (offsets) {
        const float wt = stream_load(w + tap);
        const float poison = 0.f * (ty + tx_);        // +0 for finite coordinates, NaN for a NaN one
        if (g_a) g_a[tap] = wt * (sa + poison);
        if (g_b) g_b[tap] = wt * (sb + poison);
      }
    }
  }
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// SHAPE, then the part of UNSUPPORTED that the dimensions decide
int adacof_check_dims(int N, int C, int H, int W, int F, int dilation) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || F <= 0 || dilation <= 0) return SAVFI_E_SHAPE;
  if ((C != 1 && C != 3) || F > 11 || (F & 1) == 0 || dilation > 8) return SAVFI_E_UNSUPPORTED;
  return SAVFI_OK;
}

int adacof_check_size(int N, int C, int H, int W, int F, int dilation) {
  const int64_t Hp = (int64_t)H + (int64_t)(F - 1) * dilation, Wp = (int64_t)W + (int64_t)(F - 1) * dilation;
  const int64_t limit = (int64_t)1 << 31;
  // (every factor is below 2^31 and each partial product is tested before the next factor: no overflow of the int64)
  if ((int64_t)H * W >= limit || (int64_t)H * W * F * F >= limit || (int64_t)H * W * F * F * N >= limit) return SAVFI_E_TOOBIG;
  if (Hp * Wp >= limit || Hp * Wp * C >= limit || Hp * Wp * C * N >= limit) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

}  // namespace

extern "C" int savfi_adacof_fwd_f32(const float* x, const float* w, const float* a, const float* b, float* out, int N, int C, int H,
                                    int W, int F, int dilation, void* stream) {
  if (!x || !w || !a || !b || !out) return SAVFI_E_NULL;
  if (int e = adacof_check_dims(N, C, H, W, F, dilation)) return e;
  if (out == x || out == w || out == a || out == b) return SAVFI_E_UNSUPPORTED;
  if (misaligned(x) || misaligned(w) || misaligned(a) || misaligned(b) || misaligned(out)) return SAVFI_E_UNSUPPORTED;
  if (int e = adacof_check_size(N, C, H, W, F, dilation)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int tx = savfi_cdiv(W, TW), tiles = tx * savfi_cdiv(H, TH);      // N * tiles <= N * H * W < 2^31: fits the grid's x
  const dim3 grid((unsigned)((int64_t)N * tiles));
  if (C == 3) {
    hipLaunchKernelGGL(adacof_fwd<3>, grid, dim3(NT), 0, st, x, w, a, b, out, H, W, F, dilation, tx, tiles);
  } else {
    hipLaunchKernelGGL(adacof_fwd<1>, grid, dim3(NT), 0, st, x, w, a, b, out, H, W, F, dilation, tx, tiles);
  }
  return savfi_launch_status();
}

extern "C" int savfi_adacof_bwd_f32(const float* x, const float* w, const float* a, const float* b, const float* g_out, float* g_w,
                                    float* g_a, float* g_b, int N, int C, int H, int W, int F, int dilation, void* stream) {
  if (!x || !w || !a || !b || !g_out || (!g_w && !g_a && !g_b)) return SAVFI_E_NULL;
  if (int e = adacof_check_dims(N, C, H, W, F, dilation)) return e;
  float* const outs[3] = {g_w, g_a, g_b};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    if (outs[i] == x || outs[i] == w || outs[i] == a || outs[i] == b || outs[i] == g_out) return SAVFI_E_UNSUPPORTED;
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) return SAVFI_E_UNSUPPORTED;
  }
  if (misaligned(x) || misaligned(w) || misaligned(a) || misaligned(b) || misaligned(g_out) || misaligned(g_w) || misaligned(g_a) ||
      misaligned(g_b))
    return SAVFI_E_UNSUPPORTED;
  if (int e = adacof_check_size(N, C, H, W, F, dilation)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int tx = savfi_cdiv(W, TW), tiles = tx * savfi_cdiv(H, TH);
  const dim3 grid((unsigned)((int64_t)N * tiles));
  if (C == 3) {
    hipLaunchKernelGGL(adacof_bwd<3>, grid, dim3(NT), 0, st, x, w, a, b, g_out, g_w, g_a, g_b, H, W, F, dilation, tx, tiles);
  } else {
    hipLaunchKernelGGL(adacof_bwd<1>, grid, dim3(NT), 0, st, x, w, a, b, g_out, g_w, g_a, g_b, H, W, F, dilation, tx, tiles);
  }
  return savfi_launch_status();
}
