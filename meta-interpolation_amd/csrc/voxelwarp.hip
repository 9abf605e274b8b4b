// VoxelFlow warp + blend for gfx950: one kernel forward, one kernel backward.
//
// Replaces the ~20-launch unfused sequence of the reference
// (voxelflow/core/models/voxel_flow.py:471-509; meshgrid :9-17): channel split of the tanh map,
// CPU meshgrid + H2D copy, coordinate arithmetic, two F.grid_sample(bilinear, border,
// align_corners=True), mask affine, repeat, blend.
//
//   flow = 0.5 * x3[:,0:2]   (normalised [-1,1] units)     mask = 0.5 * (1 + x3[:,2])
//   out[c] = mask * S(I0[c], g - flow) + (1 - mask) * S(I1[c], g + flow)
//
// HBM-bound: per pixel 3 floats of x3 in, 3 out, and 2x4 bilinear corners x 3 channels that hit
// L2/L1 (neighbouring lanes sample neighbouring texels).  One thread per pixel, x fastest, so the
// x3 / out / gO accesses are fully coalesced 256-byte wave segments.
#include "common.h"

namespace {

struct Tap {
  int i0, i1;     // clamped corner indices
  float w0, w1;   // weights of i0 / i1 (w1 == 0 when i1 falls outside)
  float dmul;     // d(clipped source index)/d(normalised coord): (size-1)/2 or 0 when clipped
};

// PyTorch grid_sampler semantics: unnormalise (align_corners=True), clip to the border,
// floor, and drop the out-of-range upper corner.
__device__ __forceinline__ Tap make_tap(float coord, int size) {
  Tap t;
  // grid_sampler_unnormalize(align_corners=True): ((coord + 1) / 2) * (size - 1)
  float s = ((coord + 1.f) / 2.f) * (float)(size - 1);
  t.dmul = 0.5f * (float)(size - 1);
  const float mx = (float)(size - 1);
  if (!(s > 0.f)) { s = 0.f; t.dmul = 0.f; }
  else if (s >= mx) { s = mx; t.dmul = 0.f; }
  const float f = floorf(s);
  const int i = (int)f;
  t.i0 = i;
  t.w1 = s - f;
  t.w0 = 1.f - t.w1;
  if (i + 1 <= size - 1) t.i1 = i + 1;
  else { t.i1 = i; t.w1 = 0.f; }
  return t;
}

__device__ __forceinline__ float lin(int i, int n) {
  // torch.linspace(-1, 1, n)[i]: symmetric evaluation from both ends.
  if (n == 1) return -1.f;
  const float step = 2.f / (float)(n - 1);
  return (i < n / 2) ? (-1.f + step * (float)i) : (1.f - step * (float)(n - 1 - i));
}

__global__ __launch_bounds__(256) void voxelwarp_fwd(const float* __restrict__ frames,
                                                     const float* __restrict__ x3,
                                                     float* __restrict__ out, int H, int W) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  const float* t = x3 + (size_t)b * 3 * plane + p;
  const float fx = 0.5f * t[0], fy = 0.5f * t[plane];
  const float m = 0.5f * (1.f + t[2 * plane]);
  const float gx = lin(x, W), gy = lin(y, H);
  const Tap ax = make_tap(gx - fx, W), ay = make_tap(gy - fy, H);
  const Tap bx = make_tap(gx + fx, W), by = make_tap(gy + fy, H);
  const float* I0 = frames + (size_t)b * 6 * plane;
  const float* I1 = I0 + 3 * plane;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* a = I0 + c * plane;
    const float* q = I1 + c * plane;
    const float o1 = ay.w0 * (ax.w0 * a[(size_t)ay.i0 * W + ax.i0] + ax.w1 * a[(size_t)ay.i0 * W + ax.i1]) +
                     ay.w1 * (ax.w0 * a[(size_t)ay.i1 * W + ax.i0] + ax.w1 * a[(size_t)ay.i1 * W + ax.i1]);
    const float o2 = by.w0 * (bx.w0 * q[(size_t)by.i0 * W + bx.i0] + bx.w1 * q[(size_t)by.i0 * W + bx.i1]) +
                     by.w1 * (bx.w0 * q[(size_t)by.i1 * W + bx.i0] + bx.w1 * q[(size_t)by.i1 * W + bx.i1]);
    out[((size_t)b * 3 + c) * plane + p] = m * o1 + (1.f - m) * o2;
  }
}

template <bool WANT_FRAMES>
__global__ __launch_bounds__(256) void voxelwarp_bwd(const float* __restrict__ frames,
                                                     const float* __restrict__ x3,
                                                     const float* __restrict__ gO,
                                                     float* __restrict__ g_x3,
                                                     float* __restrict__ g_frames, int H, int W) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  const float* t = x3 + (size_t)b * 3 * plane + p;
  const float fx = 0.5f * t[0], fy = 0.5f * t[plane];
  const float m = 0.5f * (1.f + t[2 * plane]);
  const float gx = lin(x, W), gy = lin(y, H);
  const Tap ax = make_tap(gx - fx, W), ay = make_tap(gy - fy, H);
  const Tap bx = make_tap(gx + fx, W), by = make_tap(gy + fy, H);
  const float* I0 = frames + (size_t)b * 6 * plane;
  const float* I1 = I0 + 3 * plane;
  float d_ax = 0.f, d_ay = 0.f, d_bx = 0.f, d_by = 0.f, d_m = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float go = gO[((size_t)b * 3 + c) * plane + p];
    const float* a = I0 + c * plane;
    const float* q = I1 + c * plane;
    const float a00 = a[(size_t)ay.i0 * W + ax.i0], a01 = a[(size_t)ay.i0 * W + ax.i1];
    const float a10 = a[(size_t)ay.i1 * W + ax.i0], a11 = a[(size_t)ay.i1 * W + ax.i1];
    const float q00 = q[(size_t)by.i0 * W + bx.i0], q01 = q[(size_t)by.i0 * W + bx.i1];
    const float q10 = q[(size_t)by.i1 * W + bx.i0], q11 = q[(size_t)by.i1 * W + bx.i1];
    const float o1 = ay.w0 * (ax.w0 * a00 + ax.w1 * a01) + ay.w1 * (ax.w0 * a10 + ax.w1 * a11);
    const float o2 = by.w0 * (bx.w0 * q00 + bx.w1 * q01) + by.w1 * (bx.w0 * q10 + bx.w1 * q11);
    d_m += go * (o1 - o2);
    const float g1 = go * m, g2 = go * (1.f - m);
    // d o / d (source x) = sum_rows wy * (I[.,i1] - I[.,i0]) when the upper corner exists
    const float sx1 = (ax.i1 != ax.i0) ? 1.f : 0.f, sy1 = (ay.i1 != ay.i0) ? 1.f : 0.f;
    const float sx2 = (bx.i1 != bx.i0) ? 1.f : 0.f, sy2 = (by.i1 != by.i0) ? 1.f : 0.f;
    d_ax += g1 * sx1 * (ay.w0 * (a01 - a00) + ay.w1 * (a11 - a10));
    d_ay += g1 * sy1 * (ax.w0 * (a10 - a00) + ax.w1 * (a11 - a01));
    d_bx += g2 * sx2 * (by.w0 * (q01 - q00) + by.w1 * (q11 - q10));
    d_by += g2 * sy2 * (bx.w0 * (q10 - q00) + bx.w1 * (q11 - q01));
    if (WANT_FRAMES) {
      float* ga = g_frames + ((size_t)b * 6 + c) * plane;
      float* gq = ga + 3 * plane;
      atomicAdd(&ga[(size_t)ay.i0 * W + ax.i0], g1 * ay.w0 * ax.w0);
      atomicAdd(&ga[(size_t)ay.i0 * W + ax.i1], g1 * ay.w0 * ax.w1);
      atomicAdd(&ga[(size_t)ay.i1 * W + ax.i0], g1 * ay.w1 * ax.w0);
      atomicAdd(&ga[(size_t)ay.i1 * W + ax.i1], g1 * ay.w1 * ax.w1);
      atomicAdd(&gq[(size_t)by.i0 * W + bx.i0], g2 * by.w0 * bx.w0);
      atomicAdd(&gq[(size_t)by.i0 * W + bx.i1], g2 * by.w0 * bx.w1);
      atomicAdd(&gq[(size_t)by.i1 * W + bx.i0], g2 * by.w1 * bx.w0);
      atomicAdd(&gq[(size_t)by.i1 * W + bx.i1], g2 * by.w1 * bx.w1);
    }
  }
  // coord1 = g - 0.5*t ; coord2 = g + 0.5*t ; source = (coord+1)*(size-1)/2 (zero slope when clipped)
  float* g = g_x3 + (size_t)b * 3 * plane + p;
  g[0] = 0.5f * (d_bx * bx.dmul - d_ax * ax.dmul);
  g[plane] = 0.5f * (d_by * by.dmul - d_ay * ay.dmul);
  g[2 * plane] = 0.5f * d_m;
}

// The backward of voxelwarp_bwd<false> (second order, frames constant).  out[:, y, x] depends on x3[:, y, x] alone, so the Hessian of
// <gO, out> in x3 is one 3 x 3 block per pixel: one thread per pixel, the gathers of the first-order backward, every output element
// written once.  With v = (v0, v1, v2) the cotangent of g_x3, A. / B. the dmul of the four taps, DX / DY the per-channel brackets of
// voxelwarp_bwd (slopes included) and X = sx * sy * ((c11 - c10) - (c01 - c00)), the only second derivative of a bilinear cell:
//   d_gO[c] = 0.5 * (v0 * ((1 - m) Bx DXb - m Ax DXa) + v1 * ((1 - m) By DYb - m Ay DYa) + v2 * (o1 - o2))
//   H01 = 0.25 sum_c go (m Ax Ay Xa + (1 - m) Bx By Xb)   H02 = -0.25 sum_c go (Ax DXa + Bx DXb)   H12 = -0.25 sum_c go (Ay DYa + By DYb)
//   d_x3 = (v1 H01 + v2 H02, v0 H01 + v2 H12, v0 H02 + v1 H12)          (H00 = H11 = H22 = 0: a cell is linear in each axis)
// Per pixel 9 floats in (x3, gO, v) and 3 per requested output, coalesced; 2 x 4 corners x 3 channels from L2 / L1.
template <bool WANT_GO, bool WANT_X>
__global__ __launch_bounds__(256) void voxelwarp_bwd2(const float* __restrict__ frames, const float* __restrict__ x3,
                                                      const float* __restrict__ gO, const float* __restrict__ v,
                                                      float* __restrict__ d_gO, float* __restrict__ d_x3, int H, int W) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  const float* t = x3 + (size_t)b * 3 * plane + p;
  const float fx = 0.5f * t[0], fy = 0.5f * t[plane];
  const float m = 0.5f * (1.f + t[2 * plane]);
  const float gx = lin(x, W), gy = lin(y, H);
  const Tap ax = make_tap(gx - fx, W), ay = make_tap(gy - fy, H);
  const Tap bx = make_tap(gx + fx, W), by = make_tap(gy + fy, H);
  const float* I0 = frames + (size_t)b * 6 * plane;
  const float* I1 = I0 + 3 * plane;
  const float* vp = v + (size_t)b * 3 * plane + p;
  const float v0 = vp[0], v1 = vp[plane], v2 = vp[2 * plane];
  const float m2 = 1.f - m;
  const float sx1 = (ax.i1 != ax.i0) ? 1.f : 0.f, sy1 = (ay.i1 != ay.i0) ? 1.f : 0.f;
  const float sx2 = (bx.i1 != bx.i0) ? 1.f : 0.f, sy2 = (by.i1 != by.i0) ? 1.f : 0.f;
  const float maxy = m * (ax.dmul * ay.dmul), mbxy = m2 * (bx.dmul * by.dmul);
  float h01 = 0.f, h02 = 0.f, h12 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* a = I0 + c * plane;
    const float* q = I1 + c * plane;
    const float a00 = a[(size_t)ay.i0 * W + ax.i0], a01 = a[(size_t)ay.i0 * W + ax.i1];
    const float a10 = a[(size_t)ay.i1 * W + ax.i0], a11 = a[(size_t)ay.i1 * W + ax.i1];
    const float q00 = q[(size_t)by.i0 * W + bx.i0], q01 = q[(size_t)by.i0 * W + bx.i1];
    const float q10 = q[(size_t)by.i1 * W + bx.i0], q11 = q[(size_t)by.i1 * W + bx.i1];
    const float dxa = sx1 * (ay.w0 * (a01 - a00) + ay.w1 * (a11 - a10));
    const float dya = sy1 * (ax.w0 * (a10 - a00) + ax.w1 * (a11 - a01));
    const float dxb = sx2 * (by.w0 * (q01 - q00) + by.w1 * (q11 - q10));
    const float dyb = sy2 * (bx.w0 * (q10 - q00) + bx.w1 * (q11 - q01));
    if (WANT_GO) {
      const float o1 = ay.w0 * (ax.w0 * a00 + ax.w1 * a01) + ay.w1 * (ax.w0 * a10 + ax.w1 * a11);
      const float o2 = by.w0 * (bx.w0 * q00 + bx.w1 * q01) + by.w1 * (bx.w0 * q10 + bx.w1 * q11);
      d_gO[((size_t)b * 3 + c) * plane + p] = 0.5f * (v0 * ((m2 * bx.dmul) * dxb - (m * ax.dmul) * dxa) +
                                                      v1 * ((m2 * by.dmul) * dyb - (m * ay.dmul) * dya) + v2 * (o1 - o2));
    }
    if (WANT_X) {
      const float go = gO[((size_t)b * 3 + c) * plane + p];
      const float xa = (sx1 * sy1) * ((a11 - a10) - (a01 - a00));
      const float xb = (sx2 * sy2) * ((q11 - q10) - (q01 - q00));
      h01 += go * (maxy * xa + mbxy * xb);
      h02 += go * (ax.dmul * dxa + bx.dmul * dxb);
      h12 += go * (ay.dmul * dya + by.dmul * dyb);
    }
  }
  if (WANT_X) {
    h01 *= 0.25f;
    h02 *= -0.25f;
    h12 *= -0.25f;
    float* d = d_x3 + (size_t)b * 3 * plane + p;
    d[0] = v1 * h01 + v2 * h02;
    d[plane] = v0 * h01 + v2 * h12;
    d[2 * plane] = v0 * h02 + v1 * h12;
  }
}

}  // namespace

extern "C" int savfi_voxelwarp_bwd2_f32(const float* frames, const float* x3, const float* gO, const float* v, float* d_gO,
                                        float* d_x3, int B, int H, int W, void* stream) {
  if (!frames || !x3 || !gO || !v || (!d_gO && !d_x3)) return SAVFI_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || B > 65535) return SAVFI_E_SHAPE;
  dim3 grid(savfi_cdiv(W, 256), H, B);
  hipStream_t st = (hipStream_t)stream;
  if (d_gO && d_x3)
    hipLaunchKernelGGL((voxelwarp_bwd2<true, true>), grid, dim3(256), 0, st, frames, x3, gO, v, d_gO, d_x3, H, W);
  else if (d_gO)
    hipLaunchKernelGGL((voxelwarp_bwd2<true, false>), grid, dim3(256), 0, st, frames, x3, gO, v, d_gO, d_x3, H, W);
  else
    hipLaunchKernelGGL((voxelwarp_bwd2<false, true>), grid, dim3(256), 0, st, frames, x3, gO, v, d_gO, d_x3, H, W);
  return savfi_launch_status();
}

extern "C" int savfi_voxelwarp_fwd_f32(const float* frames, const float* x3, float* out, int B, int H,
                                       int W, void* stream) {
  if (!frames || !x3 || !out) return SAVFI_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || B > 65535) return SAVFI_E_SHAPE;
  dim3 grid(savfi_cdiv(W, 256), H, B);
  hipLaunchKernelGGL(voxelwarp_fwd, grid, dim3(256), 0, (hipStream_t)stream, frames, x3, out, H, W);
  return savfi_launch_status();
}

extern "C" int savfi_voxelwarp_bwd_f32(const float* frames, const float* x3, const float* gO, float* g_x3,
                                       float* g_frames, int B, int H, int W, void* stream) {
  if (!frames || !x3 || !gO || !g_x3) return SAVFI_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || B > 65535) return SAVFI_E_SHAPE;
  dim3 grid(savfi_cdiv(W, 256), H, B);
  if (g_frames)
    hipLaunchKernelGGL(voxelwarp_bwd<true>, grid, dim3(256), 0, (hipStream_t)stream, frames, x3, gO, g_x3,
                       g_frames, H, W);
  else
    hipLaunchKernelGGL(voxelwarp_bwd<false>, grid, dim3(256), 0, (hipStream_t)stream, frames, x3, gO, g_x3,
                       g_frames, H, W);
  return savfi_launch_status();
}
