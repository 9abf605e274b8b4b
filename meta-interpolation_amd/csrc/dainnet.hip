// The small kernels of DAIN's frozen front for gfx950 (dain/MegaDepth, dain/networks/DAIN.py, dain/Resblock): what the depth hourglass,
// the filter net and the rectify net leave to ATen between their convolutions.  float32 NCHW read in place, forward only, no atomics,
// no memset, every launch bit-reproducible and capturable.
//
//   savfi_bn_stats_f32          per (group, channel) mean and biased variance of train-mode BatchNorm2d: a group is n_per_group consecutive
//                               samples (the two frames of one task), its statistics are those of a call of its own, bit for bit
//   savfi_bn_apply_relu_f32     relu((x - mean) / sqrt(var + eps) * gamma + beta) written into channels [c_off, c_off + C) of a C_total
//                               channel output: the four branches of an inception block land in their concatenation
//   savfi_maxpool2x2_f32        nn.MaxPool2d(2, 2): odd sides floor, NaN propagates as in ATen
//   savfi_upnearest2x_add_f32   skip + UpsamplingNearest2d(2)(low): the hourglass's upsample followed by its CAddTable
//   savfi_add_relu_f32          relu(a + r): the tail of a residual block
//   savfi_bn_running_update_f32 running <- (1 - m) running + m (stat * unbias) for a table of buffers: the running-statistics update of
//                               every BatchNorm of the hourglass in ceil(n / SAVFI_MT_MAX_TENSORS) launches
//
// All of them are HBM-bound streams.  Traffic per element: stats 2 reads (mean pass, centred pass: the second comes from L2 for the
// hourglass's planes), apply 1 read + 1 write, max-pool 1 read + 1/4 write, nearest-add 1/4 + 1 read + 1 write, add_relu 2 reads +
// 1 write.  float4 per lane where the plane size and the pointers admit it (float2 for the 2x2 windows).
//
// Statistics: two passes (mean, then centred squares).  The sum of a (group, channel) is cut the same way whatever else is in the batch:
// up to SINGLE_MAX values one workgroup adds everything; above, every plane is cut into PART-element pieces, one workgroup each, whose
// partial sums a later kernel adds lane-strided and then by butterfly -- one fixed order.  Inside a piece every lane adds groups of four
// consecutive values as (a + b) + (c + d) whether it loaded them as a float4 or one by one, so the bits do not depend on the alignment of
// the tensor either.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int SINGLE_MAX = 16384;   // values per (group, channel) one workgroup reduces alone
constexpr int PART = 8192;          // values of one plane per workgroup above that

// CENTRED: sum of (x - mean)^2 over [lo, hi) of a plane, else the plain sum; lanes take groups of 4 consecutive values, group stride
// 4 * NT.  `vec`: the plane starts on a 16-byte boundary (a group that lies inside [lo, hi) entirely is one float4 load).
template <bool CENTRED>
__device__ __forceinline__ float piece_sum(const float* __restrict__ p, int lo, int hi, float mean, bool vec) {
  float acc = 0.f;
  for (int e = lo + 4 * (int)threadIdx.x; e < hi; e += 4 * NT) {
    float v[4];
    if (vec && e + 4 <= hi) {
      const float4 t = *reinterpret_cast<const float4*>(p + e);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      if (CENTRED) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float d = v[k] - mean; v[k] = d * d; }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float x = 0.f;
        if (e + k < hi) {
          x = p[e + k];
          if (CENTRED) { const float d = x - mean; x = d * d; }
        }
        v[k] = x;
      }
    }
    acc += (v[0] + v[1]) + (v[2] + v[3]);
  }
  return acc;
}

// sum of `n` partial sums in one fixed order by wave 0 (lane-strided, then the butterfly); valid in every lane of wave 0
__device__ __forceinline__ float partials_sum(const float* __restrict__ p, int n) {
  float acc = 0.f;
  for (int i = threadIdx.x & (SAVFI_WAVE - 1); i < n; i += SAVFI_WAVE) acc += p[i];
  return wave_sum(acc);
}

// one workgroup per (channel, group): both passes
__global__ __launch_bounds__(NT) void bn_stats_single(const float* __restrict__ x, float* __restrict__ mean_out, float* __restrict__ var_out,
                                                      long long stat_stride, int C, int HW, int npg, int vec) {
  __shared__ float red[NT / SAVFI_WAVE];
  __shared__ float bc;
  const int c = blockIdx.x, g = blockIdx.y;
  const float count = (float)npg * (float)HW;
  const float* base = x + ((size_t)g * npg * C + c) * HW;
  float acc = 0.f;
  for (int s = 0; s < npg; ++s) acc += piece_sum<false>(base + (size_t)s * C * HW, 0, HW, 0.f, vec);
  float tot = block_sum<NT / SAVFI_WAVE>(acc, red);
  if (threadIdx.x == 0) bc = tot / count;
  __syncthreads();
  const float mean = bc;
  acc = 0.f;
  for (int s = 0; s < npg; ++s) acc += piece_sum<true>(base + (size_t)s * C * HW, 0, HW, mean, vec);
  tot = block_sum<NT / SAVFI_WAVE>(acc, red);
  if (threadIdx.x == 0) {
    mean_out[(size_t)g * stat_stride + c] = mean;
    var_out[(size_t)g * stat_stride + c] = tot / count;
  }
}

// grid (parts, C, G): part = s * ppp + k is piece k of sample s of the group.  CENTRED: the mean first, from the partial sums of pass 1
// (every workgroup of a (group, channel) adds them in the same order, so all of them use the same bits).
template <bool CENTRED>
__global__ __launch_bounds__(NT) void bn_stats_part(const float* __restrict__ x, const float* __restrict__ sums, float* __restrict__ partial,
                                                    int C, int HW, int npg, int ppp, int vec) {
  __shared__ float red[NT / SAVFI_WAVE];
  __shared__ float bc;
  const int part = blockIdx.x, c = blockIdx.y, g = blockIdx.z, parts = gridDim.x;
  const size_t gc = (size_t)g * C + c;
  float mean = 0.f;
  if (CENTRED) {
    if (threadIdx.x < SAVFI_WAVE) {
      const float tot = partials_sum(sums + gc * parts, parts);
      if (threadIdx.x == 0) bc = tot / ((float)npg * (float)HW);
    }
    __syncthreads();
    mean = bc;
  }
  const int s = part / ppp, k = part - s * ppp;
  const float* plane = x + (((size_t)g * npg + s) * C + c) * HW;
  const int lo = k * PART, hi = min(lo + PART, HW);
  const float tot = block_sum<NT / SAVFI_WAVE>(piece_sum<CENTRED>(plane, lo, hi, mean, vec), red);
  if (threadIdx.x == 0) partial[gc * parts + part] = tot;
}

// grid (C, G), one wave: mean and variance from the two rows of partial sums
__global__ __launch_bounds__(SAVFI_WAVE) void bn_stats_finish(const float* __restrict__ sums, const float* __restrict__ squares,
                                                              float* __restrict__ mean_out, float* __restrict__ var_out,
                                                              long long stat_stride, int C, int parts, float count) {
  const int c = blockIdx.x, g = blockIdx.y;
  const size_t gc = (size_t)g * C + c;
  const float s = partials_sum(sums + gc * parts, parts);
  const float q = partials_sum(squares + gc * parts, parts);
  if (threadIdx.x == 0) {
    mean_out[(size_t)g * stat_stride + c] = s / count;
    var_out[(size_t)g * stat_stride + c] = q / count;
  }
}

// grid (ceil(HW / (4 NT)), C, N)
__global__ __launch_bounds__(NT) void bn_apply_relu(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ var,
                                                    long long stat_stride, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, float* __restrict__ out, int C, int HW, int npg, int c_off, int C_total,
                                                    int vec) {
  const int c = blockIdx.y, n = blockIdx.z;
  const size_t st = (size_t)(n / npg) * stat_stride + c;
  const float mu = mean[st];
  const float inv = 1.0f / sqrtf(var[st] + eps);
  const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
  const float* src = x + ((size_t)n * C + c) * HW;
  float* dst = out + ((size_t)n * C_total + c_off + c) * HW;
  const bool affine = gamma != nullptr || beta != nullptr;
  auto f = [&](float v) {
    float t = (v - mu) * inv;
    if (affine) t = t * ga + be;
    return t < 0.f ? 0.f : t;                       // relu that keeps NaN, as torch's does
  };
  const int e = (blockIdx.x * NT + threadIdx.x) * 4;
  if (e >= HW) return;
  if (vec && e + 4 <= HW) {
    const float4 t = *reinterpret_cast<const float4*>(src + e);
    *reinterpret_cast<float4*>(dst + e) = make_float4(f(t.x), f(t.y), f(t.z), f(t.w));
  } else {
    for (int k = 0; k < 4 && e + k < HW; ++k) dst[e + k] = f(src[e + k]);
  }
}

// one thread per pooled pixel; ATen's scan: rows then columns, `v > m || isnan(v)` from -inf
__global__ __launch_bounds__(NT) void maxpool2x2(const float* __restrict__ in, float* __restrict__ out, int H, int W, int Ho, int Wo, int vec) {
  const int item = blockIdx.x * NT + threadIdx.x;
  if (item >= Ho * Wo) return;
  const int y = item / Wo, x = item - y * Wo;
  const size_t pl = blockIdx.y;
  const float* r0 = in + (pl * H + 2 * y) * W + 2 * x;
  const float* r1 = r0 + W;
  float v[4];
  if (vec) {
    const float2 t = *reinterpret_cast<const float2*>(r0), u = *reinterpret_cast<const float2*>(r1);
    v[0] = t.x; v[1] = t.y; v[2] = u.x; v[3] = u.y;
  } else {
    v[0] = r0[0]; v[1] = r0[1]; v[2] = r1[0]; v[3] = r1[1];
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (v[k] > m || v[k] != v[k]) m = v[k];
  out[(pl * Ho + y) * Wo + x] = m;
}

// one thread per pixel of `low`: its 2x2 block of skip / out
__global__ __launch_bounds__(NT) void upnearest2x_add(const float* __restrict__ low, const float* __restrict__ skip, float* __restrict__ out,
                                                      int h, int w, int vec) {
  const int item = blockIdx.x * NT + threadIdx.x;
  if (item >= h * w) return;
  const int y = item / w, x = item - y * w;
  const size_t pl = blockIdx.y;
  const float v = low[(pl * h + y) * w + x];
  const size_t o0 = (pl * 2 * h + 2 * y) * (size_t)(2 * w) + 2 * x, o1 = o0 + 2 * w;
  if (vec) {
    const float2 a = *reinterpret_cast<const float2*>(skip + o0), b = *reinterpret_cast<const float2*>(skip + o1);
    *reinterpret_cast<float2*>(out + o0) = make_float2(a.x + v, a.y + v);
    *reinterpret_cast<float2*>(out + o1) = make_float2(b.x + v, b.y + v);
  } else {
    out[o0] = skip[o0] + v; out[o0 + 1] = skip[o0 + 1] + v;
    out[o1] = skip[o1] + v; out[o1 + 1] = skip[o1 + 1] + v;
  }
}

__global__ __launch_bounds__(NT) void add_relu(const float* __restrict__ a, const float* __restrict__ r, float* __restrict__ y, long long n,
                                               int vec) {
  auto f = [](float p, float q) { const float t = p + q; return t < 0.f ? 0.f : t; };
  const long long stride = (long long)gridDim.x * NT * 4;
  for (long long e = ((long long)blockIdx.x * NT + threadIdx.x) * 4; e < n; e += stride) {
    if (vec && e + 4 <= n) {
      const float4 p = *reinterpret_cast<const float4*>(a + e), q = *reinterpret_cast<const float4*>(r + e);
      *reinterpret_cast<float4*>(y + e) = make_float4(f(p.x, q.x), f(p.y, q.y), f(p.z, q.z), f(p.w, q.w));
    } else {
      for (int k = 0; k < 4 && e + k < n; ++k) y[e + k] = f(a[e + k], r[e + k]);
    }
  }
}

// a table of small buffers by value in the kernel arguments (the scheme of csrc/mt_update.hip): one workgroup per buffer
struct RunTable {
  float* run[SAVFI_MT_MAX_TENSORS];
  const float* stat[SAVFI_MT_MAX_TENSORS];
  int numel[SAVFI_MT_MAX_TENSORS];
  float unbias[SAVFI_MT_MAX_TENSORS];
};

__global__ __launch_bounds__(NT) void bn_running_update(RunTable tb, float momentum) {
  const int t = blockIdx.x;
  float* run = tb.run[t];
  const float* stat = tb.stat[t];
  const float ub = tb.unbias[t], keep = 1.f - momentum;
  for (int e = threadIdx.x; e < tb.numel[t]; e += NT) run[e] = keep * run[e] + momentum * (stat[e] * ub);
}

inline bool aligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) == 0; }

// 0, or the error of a [N, C, H, W] tensor cut into groups of n_per_group samples
inline int check_nchw(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  return SAVFI_OK;
}

inline int too_big(int64_t N, int64_t C, int64_t H, int64_t W, int64_t C_total) {
  if (H * W > 0x7fffffffLL - 4 * NT || N > 65535 || C > 65535 || N * C_total * H * W >= (1LL << 40)) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

}  // namespace

extern "C" int64_t savfi_bn_stats_scratch_floats(int N, int C, int H, int W, int n_per_group) {
  if (check_nchw(N, C, H, W) || n_per_group <= 0 || N % n_per_group) return SAVFI_E_SHAPE;
  const int64_t HW = (int64_t)H * W, count = HW * n_per_group;
  if (count <= SINGLE_MAX) return 0;
  return 2 * (int64_t)(N / n_per_group) * C * n_per_group * ((HW + PART - 1) / PART);
}

extern "C" int savfi_bn_stats_f32(const float* x, float* mean, float* var, int64_t stat_stride, float* scratch, int N, int C, int H, int W,
                                  int n_per_group, void* stream) {
  if (!x || !mean || !var) return SAVFI_E_NULL;
  if (int e = check_nchw(N, C, H, W)) return e;
  if (n_per_group <= 0 || N % n_per_group || stat_stride < 0) return SAVFI_E_SHAPE;
  const int64_t HW = (int64_t)H * W, count = HW * n_per_group;
  if (count < 2) return SAVFI_E_SHAPE;                     // one value per channel has no variance (torch raises too)
  if (int e = too_big(N, C, H, W, C)) return e;
  if (count >= (1LL << 31)) return SAVFI_E_TOOBIG;
  const int G = N / n_per_group;
  const int vec = aligned(x, 15u) && HW % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (count <= SINGLE_MAX) {
    hipLaunchKernelGGL(bn_stats_single, dim3(C, G), dim3(NT), 0, st, x, mean, var, (long long)stat_stride, C, (int)HW, n_per_group, vec);
    return savfi_launch_status();
  }
  if (!scratch) return SAVFI_E_NULL;
  const int ppp = (int)((HW + PART - 1) / PART), parts = ppp * n_per_group;
  float* sums = scratch;
  float* squares = scratch + (size_t)G * C * parts;
  hipLaunchKernelGGL(bn_stats_part<false>, dim3(parts, C, G), dim3(NT), 0, st, x, (const float*)nullptr, sums, C, (int)HW, n_per_group, ppp, vec);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(bn_stats_part<true>, dim3(parts, C, G), dim3(NT), 0, st, x, (const float*)sums, squares, C, (int)HW, n_per_group, ppp, vec);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(bn_stats_finish, dim3(C, G), dim3(SAVFI_WAVE), 0, st, (const float*)sums, (const float*)squares, mean, var,
                     (long long)stat_stride, C, parts, (float)n_per_group * (float)HW);
  return savfi_launch_status();
}

extern "C" int savfi_bn_apply_relu_f32(const float* x, const float* mean, const float* var, int64_t stat_stride, const float* gamma,
                                       const float* beta, float eps, float* out, int N, int C, int H, int W, int n_per_group, int c_off,
                                       int C_total, void* stream) {
  if (!x || !mean || !var || !out) return SAVFI_E_NULL;
  if (int e = check_nchw(N, C, H, W)) return e;
  if (n_per_group <= 0 || N % n_per_group || stat_stride < 0) return SAVFI_E_SHAPE;
  if (c_off < 0 || C_total < 0 || (int64_t)c_off + C > C_total) return SAVFI_E_SHAPE;
  if (!(eps >= 0.f)) return SAVFI_E_UNSUPPORTED;
  if (int e = too_big(N, C, H, W, C_total)) return e;
  const int64_t HW = (int64_t)H * W;
  const int vec = aligned(x, 15u) && aligned(out, 15u) && HW % 4 == 0;
  hipLaunchKernelGGL(bn_apply_relu, dim3(savfi_cdiv(HW, 4 * NT), C, N), dim3(NT), 0, (hipStream_t)stream, x, mean, var,
                     (long long)stat_stride, gamma, beta, eps, out, C, (int)HW, n_per_group, c_off, C_total, vec);
  return savfi_launch_status();
}

extern "C" int savfi_maxpool2x2_f32(const float* in, float* out, int64_t planes, int H, int W, void* stream) {
  if (!in || !out) return SAVFI_E_NULL;
  if (planes <= 0 || H < 2 || W < 2) return SAVFI_E_SHAPE;
  if (planes > 65535 || (int64_t)H * W > 0x7fffffffLL - 4 * NT) return SAVFI_E_TOOBIG;
  const int Ho = H / 2, Wo = W / 2;
  const int vec = aligned(in, 7u) && W % 2 == 0;
  hipLaunchKernelGGL(maxpool2x2, dim3(savfi_cdiv((int64_t)Ho * Wo, NT), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream, in, out, H, W,
                     Ho, Wo, vec);
  return savfi_launch_status();
}

extern "C" int savfi_upnearest2x_add_f32(const float* low, const float* skip, float* out, int64_t planes, int h, int w, int H, int W,
                                         void* stream) {
  if (!low || !skip || !out) return SAVFI_E_NULL;
  if (planes <= 0 || h <= 0 || w <= 0 || H != 2 * (int64_t)h || W != 2 * (int64_t)w) return SAVFI_E_SHAPE;
  if (planes > 65535 || (int64_t)H * W > 0x7fffffffLL - 4 * NT) return SAVFI_E_TOOBIG;
  const int vec = aligned(skip, 7u) && aligned(out, 7u);
  hipLaunchKernelGGL(upnearest2x_add, dim3(savfi_cdiv((int64_t)h * w, NT), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream, low, skip,
                     out, h, w, vec);
  return savfi_launch_status();
}

extern "C" int savfi_add_relu_f32(const float* a, const float* r, float* y, int64_t n, void* stream) {
  if (!a || !r || !y) return SAVFI_E_NULL;
  if (n <= 0) return SAVFI_E_SHAPE;
  if (n >= (1LL << 40)) return SAVFI_E_TOOBIG;
  const int vec = aligned(a, 15u) && aligned(r, 15u) && aligned(y, 15u);
  const int64_t want = (n + 4 * NT - 1) / (4 * NT);
  hipLaunchKernelGGL(add_relu, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(NT), 0, (hipStream_t)stream, a, r, y, (long long)n, vec);
  return savfi_launch_status();
}

extern "C" int savfi_bn_running_update_f32(int n, float* const* running, const float* const* stat, const int64_t* numel,
                                           const float* unbias, float momentum, void* stream) {
  if (n < 0) return SAVFI_E_SHAPE;
  if (n == 0) return SAVFI_OK;
  if (!running || !stat || !numel) return SAVFI_E_NULL;
  for (int i = 0; i < n; ++i) {
    if (!running[i] || !stat[i]) return SAVFI_E_NULL;
    if (numel[i] <= 0) return SAVFI_E_SHAPE;
    if (numel[i] > 0x7fffffffLL) return SAVFI_E_TOOBIG;
  }
  if (!(momentum >= 0.f && momentum <= 1.f)) return SAVFI_E_UNSUPPORTED;
  for (int first = 0; first < n; first += SAVFI_MT_MAX_TENSORS) {
    RunTable tb;
    const int cnt = n - first < SAVFI_MT_MAX_TENSORS ? n - first : SAVFI_MT_MAX_TENSORS;
    for (int i = 0; i < cnt; ++i) {
      tb.run[i] = running[first + i];
      tb.stat[i] = stat[first + i];
      tb.numel[i] = (int)numel[first + i];
      tb.unbias[i] = unbias ? unbias[first + i] : 1.f;
    }
    hipLaunchKernelGGL(bn_running_update, dim3(cnt), dim3(NT), 0, (hipStream_t)stream, tb, momentum);
    if (int e = savfi_launch_status()) return e;
  }
  return SAVFI_OK;
}
