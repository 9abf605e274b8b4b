// Census (soft ternary) term `Census` of --loss and its gradient for gfx950 (definition: include/savfi_hip.h, tests/census_ref.py).
//   g = gray(x), zero outside the frame.  For the 49 offsets o in {-3..3}^2: d_o(p) = g(p + o) - g(p), t_o = d_o / sqrt(0.81 + d_o^2),
//   delta_o = (t_o(sr) - t_o(hr))^2, h_o = delta_o / (0.1 + delta_o).  census = sum_p m(p) sum_o h_o(p) / (49 H W), m = 0 on the
//   outermost ring of pixels.
//
// Forward: census_tiles, grid (cdiv(W, 32) * cdiv(H, 8), 1, rows * n), 256 threads.  A workgroup stages the 14 x 38 gray patches of
// both images around its tile of 8 rows x 32 columns (zeros outside the frame), every thread walks the 49 offsets of its pixel, and
// the workgroup leaves ONE double.  census_finish adds a row's partials (samples ascending, tiles in raster order: thread-strided,
// then one butterfly) and divides once.
//
// Backward: census_bwd, the same grid, ONE launch, nothing kept from the forward.  With
//   A_o(p) = 2 (t_o(sr) - t_o(hr)) * 0.1 / (0.1 + delta_o)^2 * 0.81 / (0.81 + d_o(sr)^2)^(3/2)
// the gradient of the gray image is the gather  sum_o m(q - o) A_o(q - o) - m(q) sum_o A_o(q).  Both sums run over the neighbours
// r = q + u of q: the first with o = -u (p = r, d = g(q) - g(r)), the second with o = u (d = g(r) - g(q)).  fp32 subtraction, tern()
// and census_a() are exactly odd, so A_u(q) = -A_{-u}(r) bit for bit and the two sums fold into ONE walk:
//   d / d g(q) = sum_u (m(q) + m(q + u)) A(g(q) - g(q + u)).
// t and delta come from the forward's device functions (tern, explicit fmaf: no contraction can differ between the two sites).
//
// Elements are fp32 with correctly rounded sqrtf and division (hipcc's default for HIP; no approximate reciprocal forms are asked
// for); sums are carried in double.  An identical pair has t(sr) == t(hr) bit for bit: delta = 0, h = 0, A = 0 exactly.
// No atomics, no cleared memory, no host read: capturable, bit-reproducible.  All global accesses are scalar 4-byte ones: operands
// 4 or 8 bytes off a 16-byte boundary take the same path and give the same bits.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / SAVFI_WAVE;
constexpr int TW = 32;             // tile: 32 columns (a 32-lane half of a wave reads one LDS row: no bank conflict) ...
constexpr int TH = NT / TW;        // ... by 8 rows, one pixel per thread.  Small tiles: the op is VALU-bound (49 x two square roots and
                                   // three divisions per pixel), staging is a percent of it, and 256 x 448 gives 448 workgroups, not 112
constexpr int R = 3;               // halo: offsets -3 .. 3
constexpr int PW = TW + 2 * R;     // patch: columns x0 - 3 .. x0 + TW + 2,
constexpr int PH = TH + 2 * R;     //        rows y0 - 3 .. y0 + TH + 2
constexpr int PST = PW + 1;        // its row stride

__device__ __forceinline__ float gray3(float r, float g, float b) { return fmaf(0.1140f, b, fmaf(0.5870f, g, 0.2989f * r)); }

// s = 0.81 + d^2
__device__ __forceinline__ float tern_s(float d) { return fmaf(d, d, 0.81f); }
// t = d / sqrt(0.81 + d^2): odd in d, bit for bit
__device__ __forceinline__ float tern(float d) { return d / sqrtf(tern_s(d)); }
// h = delta / (0.1 + delta) of delta = diff^2
__device__ __forceinline__ float census_h(float diff) { return (diff * diff) / fmaf(diff, diff, 0.1f); }
// A = 2 diff * 0.1 / (0.1 + delta)^2 * 0.81 / s^(3/2), diff = t(ds) - t(dh), s = 0.81 + ds^2: one division
__device__ __forceinline__ float census_a(float ds, float dh) {
  const float s = tern_s(ds);
  const float diff = tern(ds) - tern(dh);
  const float e = fmaf(diff, diff, 0.1f);
  return (0.162f * diff) / ((e * e) * (s * sqrtf(s)));
}

// The gray patches of sample z around tile (y0, x0) -> LDS, entry (r, c) = pixel (y0 - 3 + r, x0 - 3 + c), zero outside the frame.
template <int C>
__device__ __forceinline__ void stage(const float* __restrict__ sr, const float* __restrict__ hr, float* __restrict__ ps,
                                      float* __restrict__ ph, size_t z, int y0, int x0, int H, int W) {
  const size_t hw = (size_t)H * W;
  const float* a = sr + z * C * hw;
  const float* b = hr + z * C * hw;
  for (int i = threadIdx.x; i < PH * PW; i += NT) {
    const int r = i / PW, c = i - r * PW;
    const int gy = y0 - R + r, gx = x0 - R + c;
    float vs = 0.f, vh = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t at = (size_t)gy * W + gx;
      if (C == 3) {
        vs = gray3(a[at], a[at + hw], a[at + 2 * hw]);
        vh = gray3(b[at], b[at + hw], b[at + 2 * hw]);
      } else {
        vs = a[at];
        vh = b[at];
      }
    }
    ps[r * PST + c] = vs;
    ph[r * PST + c] = vh;
  }
}

__device__ __forceinline__ bool unmasked(int y, int x, int H, int W) { return y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2; }

// partial[z * gridDim.x + ty * tx + bx] = sum over tile (ty, bx) of m(p) sum_o h_o(p); blockIdx.x = ty * tx + bx (raster order)
template <int C>
__global__ __launch_bounds__(NT) void census_tiles(const float* __restrict__ sr, const float* __restrict__ hr,
                                                   double* __restrict__ partial, int H, int W, int tx) {
  __shared__ float ps[PH * PST];
  __shared__ float ph[PH * PST];
  __shared__ double red[NW];
  const int y0 = (blockIdx.x / tx) * TH, x0 = (blockIdx.x % tx) * TW;
  stage<C>(sr, hr, ps, ph, blockIdx.z, y0, x0, H, W);
  __syncthreads();

  const int c = threadIdx.x & (TW - 1), r = threadIdx.x / TW;
  double sum = 0.0;
  if (unmasked(y0 + r, x0 + c, H, W)) {
    const float* qs = ps + (r + R) * PST + c + R;
    const float* qh = ph + (r + R) * PST + c + R;
    const float cs = qs[0], ch = qh[0];
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        const float diff = tern(qs[dy * PST + dx] - cs) - tern(qh[dy * PST + dx] - ch);
        sum += (double)census_h(diff);
      }
    }
  }
  const double tot = block_sum_d<NW>(sum, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = tot;
}

// result[row] = (sum of the row's `count` partials) * inv: thread-strided, then a butterfly -- one order
__global__ __launch_bounds__(NT) void census_finish(const double* __restrict__ partial, float* __restrict__ result, int64_t count,
                                                    double inv) {
  __shared__ double red[NW];
  const double* p = partial + (size_t)blockIdx.x * count;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += NT) a += p[i];
  const double tot = block_sum_d<NW>(a, red);
  if (threadIdx.x == 0) result[blockIdx.x] = (float)(tot * inv);
}

// g_sr[z][ch](q) = coef_ch * (d / d g(q)) * g_loss[z / n] * inv, inv = 1 / (49 n H W)
template <int C>
__global__ __launch_bounds__(NT) void census_bwd(const float* __restrict__ sr, const float* __restrict__ hr,
                                                 const float* __restrict__ g_loss, float* __restrict__ g_sr, int n, int H, int W,
                                                 int tx, double inv) {
  __shared__ float ps[PH * PST];
  __shared__ float ph[PH * PST];
  const int y0 = (blockIdx.x / tx) * TH, x0 = (blockIdx.x % tx) * TW;
  const size_t z = blockIdx.z;
  stage<C>(sr, hr, ps, ph, z, y0, x0, H, W);
  __syncthreads();

  const double scale = (double)g_loss[z / n] * inv;
  const size_t hw = (size_t)H * W;
  float* out = g_sr + z * C * hw;
  const int c = threadIdx.x & (TW - 1), r = threadIdx.x / TW;
  const int x = x0 + c, y = y0 + r;
  if (y < H && x < W) {
    const float* qs = ps + (r + R) * PST + c + R;
    const float* qh = ph + (r + R) * PST + c + R;
    const float cs = qs[0], ch = qh[0];
    const float mq = unmasked(y, x, H, W) ? 1.f : 0.f;
    double acc = 0.0;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        const float w = mq + (unmasked(y + dy, x + dx, H, W) ? 1.f : 0.f);
        acc += (double)(w * census_a(cs - qs[dy * PST + dx], ch - qh[dy * PST + dx]));
      }
    }
    const float v = (float)(acc * scale);
    const size_t at = (size_t)y * W + x;
    if (C == 3) {
      out[at] = 0.2989f * v;
      out[at + hw] = 0.5870f * v;
      out[at + 2 * hw] = 0.1140f * v;
    } else {
      out[at] = v;
    }
  }
}

// NULL is checked by the callers; then SHAPE, UNSUPPORTED (C; the pointers by the callers), TOOBIG (the limits of the SSIM entries).
int census_check_shape(int rows, int n, int C, int H, int W) {
  if (rows <= 0 || n <= 0 || C <= 0 || H <= 0 || W <= 0 || H < 3 || W < 3) return SAVFI_E_SHAPE;
  return SAVFI_OK;
}

int census_check_channels(int C) { return (C != 1 && C != 3) ? SAVFI_E_UNSUPPORTED : SAVFI_OK; }

int census_check_size(int rows, int n, int H, int W) {
  if ((int64_t)rows * n > 65535 || (int64_t)H * W > 0x7fffffffLL) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

bool misaligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" int64_t savfi_census_scratch_bytes(int rows, int n, int C, int H, int W) {
  if (int e = census_check_shape(rows, n, C, H, W)) return e;
  if (int e = census_check_channels(C)) return e;
  if (int e = census_check_size(rows, n, H, W)) return e;
  const int64_t groups = (int64_t)rows * n * savfi_cdiv(H, TH) * savfi_cdiv(W, TW);
  return (groups * (int64_t)sizeof(double) + 15) & ~(int64_t)15;
}

extern "C" int savfi_census_f32(const float* sr, const float* hr, float* result, void* scratch, int rows, int n, int C, int H, int W,
                                void* stream) {
  if (!sr || !hr || !result || !scratch) return SAVFI_E_NULL;
  if (int e = census_check_shape(rows, n, C, H, W)) return e;
  if (int e = census_check_channels(C)) return e;
  // an output that is an operand or the other output; a pointer that is not a float's (a double's for the scratch)
  if (result == sr || result == hr || scratch == (const void*)sr || scratch == (const void*)hr || scratch == (void*)result)
    return SAVFI_E_UNSUPPORTED;
  if (misaligned(sr, 3) || misaligned(hr, 3) || misaligned(result, 3) || misaligned(scratch, 7)) return SAVFI_E_UNSUPPORTED;
  if (int e = census_check_size(rows, n, H, W)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int tx = savfi_cdiv(W, TW), ty = savfi_cdiv(H, TH);      // tx * ty <= H * W / 8 + H + W: fits the grid's x
  const dim3 grid(tx * ty, 1, rows * n);
  double* partial = (double*)scratch;
  if (C == 3) {
    hipLaunchKernelGGL(census_tiles<3>, grid, dim3(NT), 0, st, sr, hr, partial, H, W, tx);
  } else {
    hipLaunchKernelGGL(census_tiles<1>, grid, dim3(NT), 0, st, sr, hr, partial, H, W, tx);
  }
  if (int e = savfi_launch_status()) return e;
  const double inv = 1.0 / (49.0 * (double)n * (double)H * (double)W);
  hipLaunchKernelGGL(census_finish, dim3(rows), dim3(NT), 0, st, partial, result, (int64_t)n * tx * ty, inv);
  return savfi_launch_status();
}

extern "C" int savfi_census_bwd_f32(const float* sr, const float* hr, const float* g_loss, float* g_sr, int rows, int n, int C, int H,
                                    int W, void* stream) {
  if (!sr || !hr || !g_loss || !g_sr) return SAVFI_E_NULL;
  if (int e = census_check_shape(rows, n, C, H, W)) return e;
  if (int e = census_check_channels(C)) return e;
  if (g_sr == sr || g_sr == hr || g_sr == g_loss) return SAVFI_E_UNSUPPORTED;
  if (misaligned(sr, 3) || misaligned(hr, 3) || misaligned(g_loss, 3) || misaligned(g_sr, 3)) return SAVFI_E_UNSUPPORTED;
  if (int e = census_check_size(rows, n, H, W)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int tx = savfi_cdiv(W, TW), ty = savfi_cdiv(H, TH);
  const dim3 grid(tx * ty, 1, rows * n);
  const double inv = 1.0 / (49.0 * (double)n * (double)H * (double)W);
  if (C == 3) {
    hipLaunchKernelGGL(census_bwd<3>, grid, dim3(NT), 0, st, sr, hr, g_loss, g_sr, n, H, W, tx, inv);
  } else {
    hipLaunchKernelGGL(census_bwd<1>, grid, dim3(NT), 0, st, sr, hr, g_loss, g_sr, n, H, W, tx, inv);
  }
  return savfi_launch_status();
}
