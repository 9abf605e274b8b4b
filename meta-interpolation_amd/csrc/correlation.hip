// PWC-Net's two own operations for gfx950 (dain/PWCNet/PWCNet.py, which DAIN calls once per flow direction).
//
// 1. The cost-volume correlation (correlation_package_pytorch1_0/correlation_cuda_kernel.cu) in PWC-Net's only configuration,
//    pad_size = max_displacement = md = 4, kernel_size = 1, stride1 = stride2 = 1:
//      out[n, tc, y, x] = (1/C) sum_c p1[n,c,y,x] p2[n,c,y+tj,x+ti],  tc = (tj+md)(2md+1) + (ti+md),  p = the input with md zeros around.
//    The reference first copies both inputs into padded channels-last buffers; here NCHW is read in place and the zero border exists
//    only in LDS.  A displacement that leaves the frame is MULTIPLIED by that zero, not skipped (a NaN / inf of f1 gives 81 NaNs).
//    Both gradients are gathers: g1 = (1/C) sum_tc ge p2 (never skipped), g2 = (1/C) sum_tc ge f1 at the source pixel (y-tj, x-ti),
//    over the sources inside the frame (the reference `continue`s past the others).  No atomics, no memset, every element written by
//    exactly one thread with a sequential sum: bit-reproducible and capturable.
//    Forward: a thread owns ONE displacement row tj, 4 horizontally adjacent pixels and all 9 ti -- 36 accumulators fed per channel
//    from a 12-float window of f2 (three 16-byte LDS reads) and 4 floats of f1: 4 LDS reads for 36 FMAs where one thread per pixel
//    would do 81 for 81.  Channels are summed in order, one fp32 accumulator per output, like one lane of the reference.
//    Backward: a thread owns one pixel, keeps its 81 cotangents (masked by the fused LeakyReLU) in registers and walks the channels.
//
// 2. PWCDCNet.warp: out = bilinear_zero_padded(img, x + s u, y + s v) * (mask >= 0.9999), mask = the same sample of an all-ones image,
//    with grid_sample as the reference's pinned torch (1.2) ran it: align_corners=True, for which its normalisation
//    2 v / max(W-1, 1) - 1 is written.  (csrc/flowwarp.hip follows align_corners=False for RRIN / Super SloMo.)  Every step of the
//    coordinate chain is one separately rounded fp32 operation, as one torch op each in the reference.  Forward only.
#include "common.h"

namespace {

constexpr int MD = 4, ND = 2 * MD + 1, NT = ND * ND;     // the one supported displacement: 9 x 9 = 81 output channels

// ------------------------------------------------------------------------------------------------------------------------------
// correlation, forward
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int STRIP = 4, SX = 8, TW = STRIP * SX, TH = 4;      // a workgroup: 32 x 4 pixels, 8 strips of 4 pixels a row
constexpr int CC = 8;                                          // channels staged per round
constexpr int PW = TW + 2 * MD, PH = TH + 2 * MD;              // the f2 tile with its border
constexpr int FWD_THREADS = SX * TH * ND;                      // (strip, row, tj) = 288

__global__ __launch_bounds__(FWD_THREADS) void correlation_fwd(const float* __restrict__ f1, const float* __restrict__ f2,
                                                               float* __restrict__ out, int C, int H, int W, float slope) {
  __shared__ __attribute__((aligned(16))) float s2[CC][PH][PW];
  __shared__ __attribute__((aligned(16))) float s1[CC][TH][TW];
  const int tid = threadIdx.x;
  const int sx = tid % SX, ty = (tid / SX) % TH, tj = tid / (SX * TH);
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, n = blockIdx.z;
  const size_t plane = (size_t)H * W;
  const float* a = f1 + (size_t)n * C * plane;
  const float* b = f2 + (size_t)n * C * plane;
  float acc[ND][STRIP];
#pragma unroll
  for (int ti = 0; ti < ND; ++ti)
#pragma unroll
    for (int q = 0; q < STRIP; ++q) acc[ti][q] = 0.f;

  for (int c0 = 0; c0 < C; c0 += CC) {
    const int nc = min(CC, C - c0);
    __syncthreads();
    for (int i = tid; i < nc * PH * PW; i += FWD_THREADS) {
      const int cc = i / (PH * PW), r = (i / PW) % PH, col = i % PW;
      const int gy = y0 - MD + r, gx = x0 - MD + col;
      s2[cc][r][col] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? b[(size_t)(c0 + cc) * plane + (size_t)gy * W + gx] : 0.f;
    }
    for (int i = tid; i < nc * TH * TW; i += FWD_THREADS) {
      const int cc = i / (TH * TW), r = (i / TW) % TH, col = i % TW;
      const int gy = y0 + r, gx = x0 + col;
      s1[cc][r][col] = (gy < H && gx < W) ? a[(size_t)(c0 + cc) * plane + (size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int cc = 0; cc < nc; ++cc) {
      float p[STRIP], w[STRIP + 2 * MD];
#pragma unroll
      for (int q = 0; q < STRIP; ++q) p[q] = s1[cc][ty][sx * STRIP + q];
#pragma unroll
      for (int q = 0; q < STRIP + 2 * MD; ++q) w[q] = s2[cc][ty + tj][sx * STRIP + q];
#pragma unroll
      for (int ti = 0; ti < ND; ++ti)
#pragma unroll
        for (int q = 0; q < STRIP; ++q) acc[ti][q] += p[q] * w[q + ti];
    }
  }

  const int y = y0 + ty;
  if (y >= H) return;
  const float nelems = (float)C;
#pragma unroll
  for (int ti = 0; ti < ND; ++ti) {
    float* o = out + ((size_t)n * NT + tj * ND + ti) * plane + (size_t)y * W;
#pragma unroll
    for (int q = 0; q < STRIP; ++q) {
      const int x = x0 + sx * STRIP + q;
      if (x < W) {
        const float v = acc[ti][q] / nelems;
        o[x] = v > 0.f ? v : slope * v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// correlation, backward: SGN = +1 -> g1 (tile of f2, taps at +displacement), SGN = -1 -> g2 (tile of f1, sources at -displacement)
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int BW = 32, BH = 8;                  // one thread per pixel
constexpr int BC = 4;                           // channels staged per round
constexpr int BCH = 16;                         // channels per workgroup (grid.z = N * ceil(C / BCH))

template <int SGN>
__global__ __launch_bounds__(BW * BH) void correlation_bwd(const float* __restrict__ other, const float* __restrict__ gout,
                                                           const float* __restrict__ out, float slope, float* __restrict__ g, int C,
                                                           int H, int W, int chunks) {
  __shared__ float s[BC][BH + 2 * MD][BW + 2 * MD];
  const int tx = threadIdx.x % BW, ty = threadIdx.x / BW;
  const int n = blockIdx.z / chunks, ck = blockIdx.z % chunks;
  const int x0 = blockIdx.x * BW, y0 = blockIdx.y * BH;
  const int x = x0 + tx, y = y0 + ty;
  const bool live = x < W && y < H;
  const size_t plane = (size_t)H * W;

  // the 81 cotangents this pixel's gradient is made of, with the fused activation's derivative
  float k[NT];
#pragma unroll
  for (int tj = 0; tj < ND; ++tj)
#pragma unroll
    for (int ti = 0; ti < ND; ++ti) {
      const int tc = tj * ND + ti;
      const int ys = SGN > 0 ? y : y - (tj - MD), xs = SGN > 0 ? x : x - (ti - MD);
      const bool ok = live && ys >= 0 && ys < H && xs >= 0 && xs < W;
      float v = 0.f;
      if (ok) {
        const size_t idx = ((size_t)n * NT + tc) * plane + (size_t)ys * W + xs;
        v = gout[idx];
        if (out != nullptr && !(out[idx] > 0.f)) v *= slope;
      }
      k[tc] = v;
    }

  const int c_end = min(C, (ck + 1) * BCH);
  const float* src = other + (size_t)n * C * plane;
  const float nelems = (float)C;
  for (int c0 = ck * BCH; c0 < c_end; c0 += BC) {
    const int nc = min(BC, c_end - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * (BH + 2 * MD) * (BW + 2 * MD); i += BW * BH) {
      const int cc = i / ((BH + 2 * MD) * (BW + 2 * MD)), r = (i / (BW + 2 * MD)) % (BH + 2 * MD), col = i % (BW + 2 * MD);
      const int gy = y0 - MD + r, gx = x0 - MD + col;
      s[cc][r][col] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(size_t)(c0 + cc) * plane + (size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int cc = 0; cc < nc; ++cc) {
      float acc = 0.f;
#pragma unroll
      for (int tj = 0; tj < ND; ++tj)
#pragma unroll
        for (int ti = 0; ti < ND; ++ti) acc += k[tj * ND + ti] * s[cc][ty + MD + SGN * (tj - MD)][tx + MD + SGN * (ti - MD)];
      if (live) g[((size_t)n * C + c0 + cc) * plane + (size_t)y * W + x] = acc / nelems;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// PWC warp
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int WT = 256;         // pixels per workgroup (a flat pixel index: the maps are as small as 4 x 7)
constexpr int WCH = 8;          // channels per workgroup (grid.y = N * ceil(C / WCH))

__global__ __launch_bounds__(WT) void pwcwarp_fwd(const float* __restrict__ img, const float* __restrict__ flow, float scale,
                                                  float* __restrict__ out, int C, int H, int W, int chunks) {
  // every step is a separately rounded fp32 operation in the reference (one torch / ATen op each): no FMA contraction here
#pragma clang fp contract(off)
  const size_t plane = (size_t)H * W;
  const size_t p = (size_t)blockIdx.x * WT + threadIdx.x;
  if (p >= plane) return;
  const int n = blockIdx.y / chunks, ck = blockIdx.y % chunks;
  const int y = (int)(p / W), x = (int)(p % W);
  const float* f = flow + (size_t)n * 2 * plane + p;
  // PWCNet.py:235 `up_flow * s`, :178 `grid + flo`, :181 `2.0 * v / max(W-1, 1) - 1.0`; ATen (align_corners): ((g + 1) / 2) * (W - 1)
  const float vx = (float)x + f[0] * scale, vy = (float)y + f[plane] * scale;
  const float nx = 2.f * vx / (float)max(W - 1, 1) - 1.f, ny = 2.f * vy / (float)max(H - 1, 1) - 1.f;
  const float ix = ((nx + 1.f) / 2.f) * (float)(W - 1), iy = ((ny + 1.f) / 2.f) * (float)(H - 1);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  // positions far outside (also NaN / inf flows) sample nothing: park the cell outside the image
  const int cx = (fx0 >= -2.f && fx0 <= (float)W) ? (int)fx0 : -2;
  const int cy = (fy0 >= -2.f && fy0 <= (float)H) ? (int)fy0 : -2;
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  const float wnw = (fx1 - ix) * (fy1 - iy), wne = (ix - fx0) * (fy1 - iy), wsw = (fx1 - ix) * (iy - fy0), wse = (ix - fx0) * (iy - fy0);
  const bool xl = cx >= 0 && cx < W, xr = cx + 1 >= 0 && cx + 1 < W, yt = cy >= 0 && cy < H, yb = cy + 1 >= 0 && cy + 1 < H;
  const bool inw = xl && yt, ine = xr && yt, isw = xl && yb, ise = xr && yb;
  // a corner outside the image is skipped, as ATen does; the mask is the same sample of an all-ones image, in the same order
  float mask = 0.f;
  if (inw) mask += wnw;
  if (ine) mask += wne;
  if (isw) mask += wsw;
  if (ise) mask += wse;
  const float keep = mask >= 0.9999f ? 1.f : 0.f;
  const int64_t onw = (int64_t)cy * W + cx;      // only dereferenced where the corner is inside
  const int c_end = min(C, (ck + 1) * WCH);
  for (int ch = ck * WCH; ch < c_end; ++ch) {
    const float* a = img + ((size_t)n * C + ch) * plane;
    float acc = 0.f;
    if (inw) acc += a[onw] * wnw;
    if (ine) acc += a[onw + 1] * wne;
    if (isw) acc += a[onw + W] * wsw;
    if (ise) acc += a[onw + W + 1] * wse;
    out[((size_t)n * C + ch) * plane + p] = acc * keep;
  }
}

// H W <= 2^31 - 257 (a flat in-plane index plus a workgroup of threads stays below 2^31), grids within 65535 in y and z,
// N * widest * H W (the largest tensor of the call) below 2^40
int too_big(int N, int C, int H, int W, int chans_per_group, int rows_per_group, int widest) {
  const int64_t plane = (int64_t)H * W;
  if (plane > ((int64_t)1 << 31) - 257 || N > 65535 || C > 65535) return SAVFI_E_TOOBIG;
  if ((int64_t)N * savfi_cdiv(C, chans_per_group) > 65535 || savfi_cdiv(H, rows_per_group) > 65535) return SAVFI_E_TOOBIG;
  if ((int64_t)N * widest * plane >= ((int64_t)1 << 40)) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

}  // namespace

extern "C" int savfi_correlation_fwd_f32(const float* f1, const float* f2, float* out, int N, int C, int H, int W, int md, float slope,
                                         void* stream) {
  if (!f1 || !f2 || !out) return SAVFI_E_NULL;
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (md != MD) return SAVFI_E_UNSUPPORTED;
  if (int e = too_big(N, C, H, W, BCH, TH, C > NT ? C : NT)) return e;
  hipLaunchKernelGGL(correlation_fwd, dim3(savfi_cdiv(W, TW), savfi_cdiv(H, TH), N), dim3(FWD_THREADS), 0, (hipStream_t)stream, f1, f2,
                     out, C, H, W, slope);
  return savfi_launch_status();
}

extern "C" int savfi_correlation_bwd_f32(const float* f1, const float* f2, const float* gout, const float* out, float slope, float* g1,
                                         float* g2, int N, int C, int H, int W, int md, void* stream) {
  if (!f1 || !f2 || !gout) return SAVFI_E_NULL;
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (md != MD) return SAVFI_E_UNSUPPORTED;
  if (int e = too_big(N, C, H, W, BCH, TH, C > NT ? C : NT)) return e;       // the forward's limits: what it took, this takes
  if (!g1 && !g2) return SAVFI_OK;                 // nothing asked for: nothing to launch
  const int chunks = savfi_cdiv(C, BCH);
  const dim3 grid(savfi_cdiv(W, BW), savfi_cdiv(H, BH), N * chunks);
  if (g1) hipLaunchKernelGGL(correlation_bwd<1>, grid, dim3(BW * BH), 0, (hipStream_t)stream, f2, gout, out, slope, g1, C, H, W, chunks);
  if (g2) hipLaunchKernelGGL(correlation_bwd<-1>, grid, dim3(BW * BH), 0, (hipStream_t)stream, f1, gout, out, slope, g2, C, H, W, chunks);
  return savfi_launch_status();
}

extern "C" int savfi_pwcwarp_fwd_f32(const float* img, const float* flow, float scale, float* out, int N, int C, int H, int W,
                                     void* stream) {
  if (!img || !flow || !out) return SAVFI_E_NULL;
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (int e = too_big(N, C, H, W, WCH, 1 << 30, C)) return e;
  const int chunks = savfi_cdiv(C, WCH);
  hipLaunchKernelGGL(pwcwarp_fwd, dim3(savfi_cdiv((int64_t)H * W, WT), N * chunks), dim3(WT), 0, (hipStream_t)stream, img, flow, scale, out,
                     C, H, W, chunks);
  return savfi_launch_status();
}
