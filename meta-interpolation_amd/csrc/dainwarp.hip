// DAIN's two own operations for gfx950, fp32: the adaptive warping layer and the depth-aware flow projection.
//
// Reference (semantics kept AS IMPLEMENTED, line numbers of the reference checkout):
//   dain/my_package/FilterInterpolation/filterinterpolation_cuda_kernel.cu   forward :29-160, backward :164-460
//   dain/my_package/DepthFlowProjection/depthflowprojection_cuda_kernel.cu   scatter :29-96, averaging :99-143, hole fill :146-241,
//                                                                            backward :244-341
//
// Adaptive warping: per pixel a learned 4 x 4 filter applied to `in` at the flow-displaced position, the four 2 x 2 quadrants of the
// window blended bilinearly.  A gather; one thread per pixel, the channels split over grid.y so that a 196-channel call on a small
// map still fills the chip.  The 16 products (quadrant weight x filter tap) depend on the pixel only and are formed once per thread.
//
// Depth-aware flow projection: a data-dependent scatter of (-w fx, -w fy, w) to the four neighbours of p + flow(p).  The reference
// adds floats with atomicAdd in arrival order, which is not reproducible; its result feeds int(x2) decisions in the warping layer.
// Here every contribution is converted to a 64-bit fixed-point integer with a per-sample power-of-two scale and added with a vector
// 64-bit integer atomic: integer addition commutes, so the sums -- and everything computed from them -- are bit-reproducible.  The
// scale comes from a device-side maximum (an integer atomicMax on float bits, order-independent as well), see proj_max / proj_scale.
//
// The one result of this file that is NOT bit-reproducible is g_in of the warping backward (fp32 atomicAdd to data-dependent targets,
// as the reference does); it is produced only when asked for.
#include "common.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------------------------------------------------------
// Adaptive warping
// ------------------------------------------------------------------------------------------------------------------------------
struct WarpGeom {
  bool valid;
  int rows[4], cols[4];   // window rows / columns clamped into the image (.cu:88,90: the clamp is used for input1 only)
  float qw[4];            // quadrant weights TL, TR, BL, BR (.cu:127-130)
  float alpha, beta;
};

// .cu:65-80.  x2, y2, the validity test, int() and alpha / beta are all fp32, as the reference takes them.
__device__ __forceinline__ WarpGeom warp_geom(float fx, float fy, int w_i, int h_i, int W, int H) {
  WarpGeom g;
  const float x2 = (float)w_i + fx, y2 = (float)h_i + fy;
  // a NaN flow fails every comparison: invalid
  g.valid = x2 >= 0.0f && y2 >= 0.0f && x2 <= (float)(W - 1) && y2 <= (float)(H - 1) && fabsf(fx) < (float)W / 2.0f &&
            fabsf(fy) < (float)H / 2.0f;
  if (!g.valid) return g;
  const int ix = (int)x2, iy = (int)y2;
  const int L = ix + 1 - 2, T = iy + 1 - 2;   // .cu:74-75 with filter_size = 4
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.rows[k] = min(max(0, T + k), H - 1);
    g.cols[k] = min(max(0, L + k), W - 1);
  }
  g.alpha = x2 - (float)ix;
  g.beta = y2 - (float)iy;
  g.qw[0] = (1.f - g.alpha) * (1.f - g.beta);
  g.qw[1] = g.alpha * (1.f - g.beta);
  g.qw[2] = (1.f - g.alpha) * g.beta;
  g.qw[3] = g.alpha * g.beta;
  return g;
}

// tap (j, i) of the window belongs to quadrant 2 * (j >= 2) + (i >= 2): rows 0-1 "top" (filter_j <= int(y2)), columns 0-1 "left"
__device__ __forceinline__ constexpr int quad_of(int k) { return 2 * ((k >> 2) >> 1) + ((k & 3) >> 1); }

// One pixel of one channel chunk, shared by both forwards: `dst` is the output element of channel c0 at pixel p, its channels one
// plane apart (whatever tensor they lie in).
__device__ __forceinline__ void filterinterp_pixel(const float* __restrict__ in, const float* __restrict__ flow,
                                                   const float* __restrict__ filt, float* __restrict__ dst, int b, int c0, int c1, int p,
                                                   int C, int H, int W) {
  const int plane = H * W;                                  // < 2^31 (entry check)
  const int h_i = p / W, w_i = p - h_i * W;
  const float* fl = flow + (size_t)b * 2 * plane + p;
  const WarpGeom g = warp_geom(fl[0], fl[plane], w_i, h_i, W, H);
  const float* src = in + ((size_t)b * C + c0) * plane;
  if (!g.valid) {                                           // .cu:151-156: the input passes through
    for (int c = c0; c < c1; ++c, src += plane, dst += plane) *dst = src[p];
    return;
  }
  float wt[16];
  int idx[16];
  const float* ft = filt + (size_t)b * 16 * plane + p;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    wt[k] = g.qw[quad_of(k)] * ft[(size_t)k * plane];     // tap (j, i) reads filter channel 4 j + i (.cu:92)
    idx[k] = g.rows[k >> 2] * W + g.cols[k & 3];
  }
  for (int c = c0; c < c1; ++c, src += plane, dst += plane) {
    float q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) q[quad_of(k)] = fmaf(wt[k], src[idx[k]], q[quad_of(k)]);
    *dst = (q[0] + q[1]) + (q[2] + q[3]);
  }
}

// grid: (pixel blocks, channel chunks, B)
__global__ __launch_bounds__(NT) void filterinterp_fwd(const float* __restrict__ in, const float* __restrict__ flow,
                                                       const float* __restrict__ filt, float* __restrict__ out, int C, int H, int W,
                                                       int cpc) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * cpc, c1 = min(C, c0 + cpc);
  filterinterp_pixel(in, flow, filt, out + ((size_t)b * C + c0) * plane + p, b, c0, c1, p, C, H, W);
}

// The same into channels [c_off, c_off + C) of out [B, C_total, H, W]: scalar stores one plane apart, as above -- a slice base
// c_off * H * W has no alignment beyond a float's -- and no other channel of `out` is touched.  Same grid.
__global__ __launch_bounds__(NT) void filterinterp_fwd_slice(const float* __restrict__ in, const float* __restrict__ flow,
                                                             const float* __restrict__ filt, float* __restrict__ out, int C, int H,
                                                             int W, int cpc, int C_total, int c_off) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * cpc, c1 = min(C, c0 + cpc);
  filterinterp_pixel(in, flow, filt, out + ((size_t)b * C_total + c_off + c0) * plane + p, b, c0, c1, p, C, H, W);
}

__global__ __launch_bounds__(NT) void zero_f32(float* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) p[i] = 0.f;
}

// One thread per pixel over ALL channels: g_filt and g_flow are sums over c at the thread's own pixel, accumulated in registers in
// channel order (no atomics, one fixed order).  g_in (nullable) is the scatter.  grid: (pixel blocks, 1, B)
__global__ __launch_bounds__(NT) void filterinterp_bwd(const float* __restrict__ in, const float* __restrict__ flow,
                                                       const float* __restrict__ filt, const float* __restrict__ gout,
                                                       float* __restrict__ g_in, float* __restrict__ g_flow, float* __restrict__ g_filt,
                                                       int C, int H, int W) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const int h_i = p / W, w_i = p - h_i * W;
  const float* fl = flow + (size_t)b * 2 * plane + p;
  const WarpGeom g = warp_geom(fl[0], fl[plane], w_i, h_i, W, H);
  float* gfl = g_flow ? g_flow + (size_t)b * 2 * plane + p : nullptr;
  float* gft = g_filt ? g_filt + (size_t)b * 16 * plane + p : nullptr;
  if (!g.valid) {     // .cu:200-201: an invalid pixel gives no gradient to anything, `in` included (the forward passes it through)
    if (gfl) { gfl[0] = 0.f; gfl[plane] = 0.f; }
    if (gft) {
#pragma unroll
      for (int k = 0; k < 16; ++k) gft[(size_t)k * plane] = 0.f;
    }
    return;
  }
  float f[16], gf[16];
  int idx[16];
  const float* ft = filt + (size_t)b * 16 * plane + p;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    f[k] = ft[(size_t)k * plane];
    gf[k] = 0.f;
    idx[k] = g.rows[k >> 2] * W + g.cols[k & 3];
  }
  float gx = 0.f, gy = 0.f;
  const float* src = in + (size_t)b * C * plane;
  const float* go = gout + (size_t)b * C * plane + p;
  float* gi = g_in ? g_in + (size_t)b * C * plane : nullptr;
  for (int c = 0; c < C; ++c, src += plane, go += plane) {
    const float gv = *go;
    float qg[4], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) qg[k] = gv * g.qw[k];       // TL_grad ... BR_grad (.cu:222,237,253,269)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float v = src[idx[k]];
      gf[k] = fmaf(qg[quad_of(k)], v, gf[k]);               // .cu:230-232
      q[quad_of(k)] = fmaf(v, f[k], q[quad_of(k)]);         // TL, TR, BL, BR (.cu:307-345)
      if (gi) atomicAdd(gi + idx[k], qg[quad_of(k)] * f[k]);   // .cu:227-229
    }
    gx = fmaf(gv, (1.f - g.beta) * (q[1] - q[0]) + g.beta * (q[3] - q[2]), gx);    // .cu:348-350
    gy = fmaf(gv, (1.f - g.alpha) * (q[2] - q[0]) + g.alpha * (q[3] - q[1]), gy);  // .cu:419-421
    if (gi) gi += plane;
  }
  if (gfl) { gfl[0] = gx; gfl[plane] = gy; }
  if (gft) {
#pragma unroll
    for (int k = 0; k < 16; ++k) gft[(size_t)k * plane] = gf[k];
  }
}

int warp_check(int B, int C, int H, int W, int filter_size) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (filter_size != 4) return SAVFI_E_UNSUPPORTED;
  // in-plane indices are int (block * NT + thread included); grid z and y are 16-bit; the whole tensor within 2^40 elements
  if ((int64_t)H * W > 0x7fffffffLL - NT || B > 65535 || C > 65535 || (int64_t)B * C * H * W >= ((int64_t)1 << 40)) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Depth-aware flow projection
// ------------------------------------------------------------------------------------------------------------------------------
// scratch: long long acc[B][3][H*W] (sum of -w fx, sum of -w fy, sum of w, fixed point) | unsigned maxbits[B]
struct ProjSrc {
  bool valid;
  int L, T, R, Bt;
};

// .cu:65-74: a source is scattered iff x2, y2 lie inside [0, W-1] x [0, H-1] (NaN: never)
__device__ __forceinline__ ProjSrc proj_src(float fx, float fy, int w_i, int h_i, int W, int H) {
  ProjSrc s;
  const float x2 = (float)w_i + fx, y2 = (float)h_i + fy;
  s.valid = x2 >= 0.0f && y2 >= 0.0f && x2 <= (float)(W - 1) && y2 <= (float)(H - 1);
  if (!s.valid) return s;
  s.L = (int)x2;
  s.T = (int)y2;
  s.R = min(s.L + 1, W - 1);
  s.Bt = min(s.T + 1, H - 1);
  return s;
}

// |w| max(|fx|, |fy|, 1) in fp32: what sets the per-sample scale; a source is scattered iff this is finite
__device__ __forceinline__ float proj_magnitude(float wv, float fx, float fy) {
  return fabsf(wv) * fmaxf(fmaxf(fabsf(fx), fabsf(fy)), 1.f);
}

__global__ __launch_bounds__(64) void proj_zero_max(unsigned* __restrict__ maxbits, int B) {
  for (int i = threadIdx.x; i < B; i += 64) maxbits[i] = 0u;
}

// clears the accumulators (with a kernel: a captured memset node clears only in the first replay) and takes the per-sample maximum
// of |w| max(|fx|, |fy|, 1) over the sources that will be scattered.  Non-negative floats order like their bit patterns, so an
// unsigned atomicMax on the bits is exact and order-independent.  grid: (pixel blocks, 1, B)
__global__ __launch_bounds__(NT) void proj_max(const float* __restrict__ flow, const float* __restrict__ wgt, long long* __restrict__ acc,
                                               unsigned* __restrict__ maxbits, int H, int W) {
  __shared__ float lds[NT / SAVFI_WAVE];
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  const int b = blockIdx.z;
  float m = 0.f;
  if (p < plane) {
    long long* a = acc + (size_t)b * 3 * plane + p;
    a[0] = 0;
    a[plane] = 0;
    a[2 * (size_t)plane] = 0;
    const int h_i = p / W, w_i = p - h_i * W;
    const float fx = flow[(size_t)b * 2 * plane + p], fy = flow[((size_t)b * 2 + 1) * plane + p];
    if (proj_src(fx, fy, w_i, h_i, W, H).valid) {
      const float v = proj_magnitude(wgt[(size_t)b * plane + p], fx, fy);
      if (v < INFINITY) m = v;                              // a source without a finite magnitude is not scattered (proj_scatter)
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, SAVFI_WAVE));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NT / SAVFI_WAVE; ++i) m = fmaxf(m, lds[i]);
    if (m > 0.f) atomicMax(maxbits + b, __float_as_uint(m));
  }
}

// k with: every |contribution| * 2^k <= 2^(62 - lg), lg = ceil(log2(4 H W)) -- at most 4 H W contributions reach one target (each of
// the H W sources hits a target at most 4 times), so a sum stays below 2^62 + 4 H W (the round-away unit) < 2^63.
__device__ __forceinline__ int proj_scale(unsigned mbits, int lg) {
  int e = 0;
  if (mbits) (void)frexpf(__uint_as_float(mbits), &e);      // max = m 2^e, m in [0.5, 1): 2^e > max
  return 62 - lg - e;                                       // in [-99, 209]: 2^k is a normal double
}
__device__ __forceinline__ double pow2d(int k) { return __longlong_as_double((long long)(k + 1023) << 52); }

// a contribution in fixed point, rounded AWAY from zero: a non-zero contribution stays non-zero, so count > 0 still says that
// something landed.  v * s is exact (a power-of-two scale of a double that holds the fp32 product exactly).
__device__ __forceinline__ long long to_fixed(double v, double s) {
  const double t = v * s;
  return (long long)(t > 0.0 ? ceil(t) : floor(t));
}

__global__ __launch_bounds__(NT) void proj_scatter(const float* __restrict__ flow, const float* __restrict__ wgt,
                                                   long long* __restrict__ acc, const unsigned* __restrict__ maxbits, int H, int W,
                                                   int lg) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const int h_i = p / W, w_i = p - h_i * W;
  const float fx = flow[(size_t)b * 2 * plane + p], fy = flow[((size_t)b * 2 + 1) * plane + p];
  const ProjSrc s = proj_src(fx, fy, w_i, h_i, W, H);
  if (!s.valid) return;
  const float wv = wgt[(size_t)b * plane + p];
  // the predicate of proj_max: a NaN / Inf depth inverse, or one so large that |w| max(|f|, 1) overflows fp32, has no fixed-point
  // value under the sample's scale and is skipped (documented in savfi_hip.h)
  if (!(proj_magnitude(wv, fx, fy) < INFINITY)) return;
  const double sc = pow2d(proj_scale(maxbits[b], lg));
  const unsigned long long qx = (unsigned long long)to_fixed(-(double)wv * (double)fx, sc);   // .cu:78-81
  const unsigned long long qy = (unsigned long long)to_fixed(-(double)wv * (double)fy, sc);   // .cu:83-86
  const unsigned long long qc = (unsigned long long)to_fixed((double)wv, sc);                 // .cu:88-91
  unsigned long long* a = (unsigned long long*)acc + (size_t)b * 3 * plane;
  // the four targets in the reference's order; L == R or T == Bt hits one target twice (kept)
  const int t[4] = {s.T * W + s.L, s.T * W + s.R, s.Bt * W + s.L, s.Bt * W + s.R};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    atomicAdd(a + t[k], qx);
    atomicAdd(a + (size_t)plane + t[k], qy);
    atomicAdd(a + 2 * (size_t)plane + t[k], qc);
  }
}

// .cu:134-140: count leaves fixed point; out = sum / count where count > 0, the raw sum elsewhere (0 where nothing landed)
__global__ __launch_bounds__(NT) void proj_average(const long long* __restrict__ acc, const unsigned* __restrict__ maxbits,
                                                   float* __restrict__ count, float* __restrict__ out, int H, int W, int lg) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const long long* a = acc + (size_t)b * 3 * plane + p;
  const long long sx = a[0], sy = a[plane], sc = a[2 * (size_t)plane];
  const double inv = pow2d(-proj_scale(maxbits[b], lg));
  const float cnt = (float)((double)sc * inv);
  count[(size_t)b * plane + p] = cnt;
  float ox, oy;
  if (cnt > 0.0f) {
    ox = (float)((double)sx / (double)sc);
    oy = (float)((double)sy / (double)sc);
  } else {
    ox = (float)((double)sx * inv);
    oy = (float)((double)sy * inv);
  }
  out[(size_t)b * 2 * plane + p] = ox;
  out[((size_t)b * 2 + 1) * plane + p] = oy;
}

// .cu:181-237.  Only pixels with count <= 0 are written and only pixels with count > 0 are read: no race.
__global__ __launch_bounds__(NT) void proj_fill(const float* __restrict__ count, float* __restrict__ out, int H, int W) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const float* cn = count + (size_t)b * plane;
  if (cn[p] > 0.0f) return;
  const int h_i = p / W, w_i = p - h_i * W;
  int lo = w_i, ro = w_i, uo = h_i, dn = h_i;
  float lt = 0.f, rt = 0.f, ut = 0.f, dt = 0.f;
  while (lt == 0.0f && lo - 1 >= 0) lt = cn[h_i * W + --lo];
  while (rt == 0.0f && ro + 1 <= W - 1) rt = cn[h_i * W + ++ro];
  while (ut == 0.0f && uo - 1 >= 0) ut = cn[--uo * W + w_i];
  while (dt == 0.0f && dn + 1 <= H - 1) dt = cn[++dn * W + w_i];
  if (lt + rt + ut + dt <= 0.0f) return;                    // .cu:209-212, the fp32 sum in the reference's order
  lt = lt > 0.0f ? 1.f : 0.f;
  rt = rt > 0.0f ? 1.f : 0.f;
  ut = ut > 0.0f ? 1.f : 0.f;
  dt = dt > 0.0f ? 1.f : 0.f;
  const float den = lt + rt + ut + dt;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    float* o = out + ((size_t)b * 2 + ch) * plane;
    float s = 0.f;                                          // a direction that found nothing valid is not read (weight 0)
    if (lt > 0.f) s += o[h_i * W + lo];
    if (rt > 0.f) s += o[h_i * W + ro];
    if (ut > 0.f) s += o[uo * W + w_i];
    if (dt > 0.f) s += o[dn * W + w_i];
    o[p] = s / den;
  }
}

// .cu:276-337, a gather over the same four targets (a doubled target is read twice, as written).  Note the (f - out) factor of g_w:
// kept as implemented although the derivative of -sum(w f) / sum(w) has -(f + out) / count.
__global__ __launch_bounds__(NT) void proj_bwd(const float* __restrict__ flow, const float* __restrict__ wgt,
                                               const float* __restrict__ count, const float* __restrict__ out,
                                               const float* __restrict__ gout, float* __restrict__ g_flow, float* __restrict__ g_w, int H,
                                               int W) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int b = blockIdx.z;
  const int h_i = p / W, w_i = p - h_i * W;
  const float fx = flow[(size_t)b * 2 * plane + p], fy = flow[((size_t)b * 2 + 1) * plane + p];
  const ProjSrc s = proj_src(fx, fy, w_i, h_i, W, H);
  float gfx = 0.f, gfy = 0.f, gw = 0.f;
  if (s.valid) {
    const float wv = wgt[(size_t)b * plane + p];
    const float* cn = count + (size_t)b * plane;
    const float* ox = out + (size_t)b * 2 * plane;
    const float* gx = gout + (size_t)b * 2 * plane;
    const int t[4] = {s.T * W + s.L, s.T * W + s.R, s.Bt * W + s.L, s.Bt * W + s.R};
    float gwx = 0.f, gwy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float c = cn[t[k]], g0 = gx[t[k]], g1 = gx[(size_t)plane + t[k]];
      gfx += -g0 * wv / c;                                  // .cu:291-298
      gfy += -g1 * wv / c;                                  // .cu:301-308
      gwx += -g0 / c * (fx - ox[t[k]]);                     // .cu:312-323
      gwy += -g1 / c * (fy - ox[(size_t)plane + t[k]]);     // .cu:325-336
    }
    gw = gwx + gwy;
  }
  if (g_flow) {
    g_flow[(size_t)b * 2 * plane + p] = gfx;
    g_flow[((size_t)b * 2 + 1) * plane + p] = gfy;
  }
  if (g_w) g_w[(size_t)b * plane + p] = gw;
}

int proj_check(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  // in-plane indices are int (block * NT + thread included); grid z is 16-bit; B * 3 * H * W accumulators within 2^40
  if ((int64_t)H * W > 0x7fffffffLL - NT || B > 65535 || (int64_t)B * 3 * H * W >= ((int64_t)1 << 40)) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

int ceil_log2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

}  // namespace

// channel chunks: enough workgroups for 256 CUs x 8 on a small map, at least 4 channels a thread to amortise the 16 tap products
static void warp_chunks(int B, int C, int pb, int* chunks_out, int* cpc_out) {
  int chunks = savfi_cdiv(2048, (int64_t)pb * B);
  chunks = chunks < 1 ? 1 : chunks;
  int cpc = savfi_cdiv(C, chunks);
  if (cpc < 4) cpc = C < 4 ? C : 4;
  *chunks_out = savfi_cdiv(C, cpc);
  *cpc_out = cpc;
}

extern "C" int savfi_filterinterp_fwd_f32(const float* in, const float* flow, const float* filt, float* out, int B, int C, int H, int W,
                                          int filter_size, void* stream) {
  if (!in || !flow || !filt || !out) return SAVFI_E_NULL;
  if (int e = warp_check(B, C, H, W, filter_size)) return e;
  const int pb = savfi_cdiv((int64_t)H * W, NT);
  int chunks, cpc;
  warp_chunks(B, C, pb, &chunks, &cpc);
  hipLaunchKernelGGL(filterinterp_fwd, dim3(pb, chunks, B), dim3(NT), 0, (hipStream_t)stream, in, flow, filt, out, C, H, W, cpc);
  return savfi_launch_status();
}

extern "C" int savfi_filterinterp_fwd_slice_f32(const float* in, const float* flow, const float* filt, float* out, int B, int C, int H,
                                                int W, int filter_size, int C_total, int c_off, void* stream) {
  if (!in || !flow || !filt || !out) return SAVFI_E_NULL;
  if (C_total <= 0 || c_off < 0 || (int64_t)c_off + C > C_total) return SAVFI_E_SHAPE;
  if (int e = warp_check(B, C, H, W, filter_size)) return e;
  if (int e = warp_check(B, C_total, H, W, filter_size)) return e;      // the OUTPUT's element count
  const int pb = savfi_cdiv((int64_t)H * W, NT);
  int chunks, cpc;
  warp_chunks(B, C, pb, &chunks, &cpc);
  hipLaunchKernelGGL(filterinterp_fwd_slice, dim3(pb, chunks, B), dim3(NT), 0, (hipStream_t)stream, in, flow, filt, out, C, H, W, cpc,
                     C_total, c_off);
  return savfi_launch_status();
}

extern "C" int savfi_filterinterp_bwd_f32(const float* in, const float* flow, const float* filt, const float* gout, float* g_in,
                                          float* g_flow, float* g_filt, int B, int C, int H, int W, int filter_size, void* stream) {
  if (!in || !flow || !filt || !gout) return SAVFI_E_NULL;
  if (int e = warp_check(B, C, H, W, filter_size)) return e;
  if (!g_in && !g_flow && !g_filt) return SAVFI_OK;
  hipStream_t st = (hipStream_t)stream;
  if (g_in) {
    const size_t n = (size_t)B * C * H * W;
    const int zb = (int)((n + NT - 1) / NT < 8192 ? (n + NT - 1) / NT : 8192);
    hipLaunchKernelGGL(zero_f32, dim3(zb), dim3(NT), 0, st, g_in, n);
    if (int e = savfi_launch_status()) return e;
  }
  hipLaunchKernelGGL(filterinterp_bwd, dim3(savfi_cdiv((int64_t)H * W, NT), 1, B), dim3(NT), 0, st, in, flow, filt, gout, g_in, g_flow,
                     g_filt, C, H, W);
  return savfi_launch_status();
}

extern "C" int64_t savfi_depthflowproj_scratch_bytes(int B, int H, int W) {
  if (int e = proj_check(B, H, W)) return e;
  return (int64_t)B * 3 * H * W * (int64_t)sizeof(long long) + (((int64_t)B * (int64_t)sizeof(unsigned) + 7) & ~(int64_t)7);
}

extern "C" int savfi_depthflowproj_fwd_f32(const float* flow, const float* w, float* count, float* out, void* scratch, int B, int H, int W,
                                           int fillhole, void* stream) {
  if (!flow || !w || !count || !out || !scratch) return SAVFI_E_NULL;
  if (int e = proj_check(B, H, W)) return e;
  if ((uintptr_t)scratch & 7u) return SAVFI_E_UNSUPPORTED;  // 64-bit accumulators
  long long* acc = (long long*)scratch;
  unsigned* maxbits = (unsigned*)(acc + (size_t)B * 3 * H * W);
  const int lg = ceil_log2(4 * (int64_t)H * W);
  const dim3 grid(savfi_cdiv((int64_t)H * W, NT), 1, B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(proj_zero_max, dim3(1), dim3(64), 0, st, maxbits, B);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(proj_max, grid, dim3(NT), 0, st, flow, w, acc, maxbits, H, W);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(proj_scatter, grid, dim3(NT), 0, st, flow, w, acc, maxbits, H, W, lg);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(proj_average, grid, dim3(NT), 0, st, acc, maxbits, count, out, H, W, lg);
  if (int e = savfi_launch_status()) return e;
  if (fillhole) {
    hipLaunchKernelGGL(proj_fill, grid, dim3(NT), 0, st, count, out, H, W);
    if (int e = savfi_launch_status()) return e;
  }
  return SAVFI_OK;
}

extern "C" int savfi_depthflowproj_bwd_f32(const float* flow, const float* w, const float* count, const float* out, const float* gout,
                                           float* g_flow, float* g_w, int B, int H, int W, void* stream) {
  if (!flow || !w || !count || !out || !gout) return SAVFI_E_NULL;
  if (int e = proj_check(B, H, W)) return e;
  if (!g_flow && !g_w) return SAVFI_OK;
  hipLaunchKernelGGL(proj_bwd, dim3(savfi_cdiv((int64_t)H * W, NT), 1, B), dim3(NT), 0, (hipStream_t)stream, flow, w, count, out, gout,
                     g_flow, g_w, H, W);
  return savfi_launch_status();
}
