// Frame staging for gfx950: decoded frames travel over PCIe as uint8 HWC (a quarter of the fp32 bytes) and become the
// fp32 NCHW tensors of the meta-batch on the GPU, on a side stream, while the previous meta-iteration computes.
//
// Replaces the host-side tail of the dataset readers: `[2,1,0]` channel swap, `np.transpose(im, (2,0,1))`,
// `.float() / 255` and torchvision's Normalize (data/vimeo_septuplet.py:68-80, data/video.py:44-51).
//   dst[n][c][y][x] = (src[n][y][x][swap ? 2-c : c] / div - mean[c]) / std    (fp32, the reference's operation order)
// One thread per pixel: 3 adjacent bytes in, one float to each of the 3 planes (coalesced along x).
//
// And the way back for a frame that leaves the device (utils.py:276-285 save_image): fp32 NCHW in [0, 1] -> uint8 NHWC, so that
// only bytes cross PCIe.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void frames_u8_to_f32(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                        size_t pixels_per_image, size_t total_pixels, int swap_rb, float div,
                                                        float mean0, float mean1, float mean2, float std) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total_pixels) return;
  const size_t n = p / pixels_per_image, q = p - n * pixels_per_image;
  const unsigned char* s = src + p * 3;
  float* d = dst + n * 3 * pixels_per_image + q;
  const float mean[3] = {mean0, mean1, mean2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (float)s[swap_rb ? 2 - c : c];
    d[(size_t)c * pixels_per_image] = (v / div - mean[c]) / std;
  }
}

// The way back: a unit-range fp32 NCHW frame -> uint8 NHWC, quantised as utils.save_image does (savfi_quantize255).  One thread
// per 4 consecutive pixels of an image: C float4 loads, 4 C bytes packed into C dwords (vec: H W % 4 == 0, src 16-byte and dst
// 4-byte aligned); otherwise scalar loads and byte stores of the same values.  A NaN is written as 0.
__device__ __forceinline__ unsigned quant_byte(float x) {
  const float q = savfi_quantize255(x);
  return q == q ? (unsigned)(int)q : 0u;
}

template <int C>
__global__ __launch_bounds__(256) void frames_f32_to_u8(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                        size_t pixels_per_image, size_t quads_per_image, size_t total_quads, int vec) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total_quads) return;
  const size_t n = t / quads_per_image, q = (t - n * quads_per_image) * 4;
  const float* s = src + n * C * pixels_per_image + q;
  unsigned char* d = dst + (n * pixels_per_image + q) * C;
  if (vec) {
    unsigned char b[4 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(s + (size_t)c * pixels_per_image);
      b[c] = (unsigned char)quant_byte(v.x);
      b[C + c] = (unsigned char)quant_byte(v.y);
      b[2 * C + c] = (unsigned char)quant_byte(v.z);
      b[3 * C + c] = (unsigned char)quant_byte(v.w);
    }
    unsigned* out = reinterpret_cast<unsigned*>(d);
#pragma unroll
    for (int w = 0; w < C; ++w) out[w] = b[4 * w] | ((unsigned)b[4 * w + 1] << 8) | ((unsigned)b[4 * w + 2] << 16) | ((unsigned)b[4 * w + 3] << 24);
  } else {
    const int left = (int)min((size_t)4, pixels_per_image - q);
    for (int k = 0; k < left; ++k)
#pragma unroll
      for (int c = 0; c < C; ++c) d[k * C + c] = (unsigned char)quant_byte(s[(size_t)c * pixels_per_image + k]);
  }
}

}  // namespace

extern "C" int savfi_frames_f32_to_u8(const float* src, unsigned char* dst, int64_t N, int C, int H, int W, void* stream) {
  if (!src || !dst) return SAVFI_E_NULL;
  if (N <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (C != 1 && C != 3) return SAVFI_E_UNSUPPORTED;
  const size_t ppi = (size_t)H * W, qpi = (ppi + 3) / 4, total = (size_t)N * qpi;
  if ((total + 255) / 256 > 0x7fffffffULL) return SAVFI_E_TOOBIG;
  const int vec = ppi % 4 == 0 && ((uintptr_t)src & 15u) == 0 && ((uintptr_t)dst & 3u) == 0;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (C == 3)
    hipLaunchKernelGGL(frames_f32_to_u8<3>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, ppi, qpi, total, vec);
  else
    hipLaunchKernelGGL(frames_f32_to_u8<1>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, ppi, qpi, total, vec);
  return savfi_launch_status();
}

extern "C" int savfi_frames_u8_to_f32(const unsigned char* src, float* dst, int64_t N, int H, int W, int swap_rb, float div,
                                      float mean_c0, float mean_c1, float mean_c2, float std, void* stream) {
  if (!src || !dst) return SAVFI_E_NULL;
  if (N <= 0 || H <= 0 || W <= 0 || div == 0.f || std == 0.f) return SAVFI_E_SHAPE;
  const size_t ppi = (size_t)H * W, total = (size_t)N * ppi;
  if ((total + 255) / 256 > 0x7fffffffULL) return SAVFI_E_TOOBIG;
  hipLaunchKernelGGL(frames_u8_to_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, ppi,
                     total, swap_rb ? 1 : 0, div, mean_c0, mean_c1, mean_c2, std);
  return savfi_launch_status();
}
