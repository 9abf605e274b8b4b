// Softmax splatting (forward warping with a learned importance; Niklaus & Liu, CVPR 2020) for gfx950, fp32 in and out.
// Definition: include/savfi_hip.h; restatement: tests/softsplat_ref.py.
//
//   x [N, C, H, W], flow [N, 2, H, W] (x then y), metric Z [N, 1, H, W] -> out [N, C, H, W], hit, D, M [N, 1, H, W].
//   Source p = (i, j) lands at X = float(j) + flow_x, Y = float(i) + flow_y (ONE fp32 addition each), cell floor(X), floor(Y), and gives
//   the bilinear share b_k of itself to each of the four corners q_k that TAKE PART: inside the frame, both 1-D factors > 0.
//   sum: out = sum b x.   avg: out = sum b x / sum b.   soft: out = sum e b x / sum e b, e = expf(Z_p - M(q)), M(q) the largest Z that
//   takes part at q -- a per-target softmax, finite for every finite Z.
//
// A scatter: the sums are data-dependent.  Float atomics would add in arrival order; here, as in csrc/dainwarp.hip, every contribution is
// formed in double, converted to a 64-bit fixed-point integer (rounded AWAY from zero: a share that takes part never vanishes) and added
// with a vector 64-bit integer atomic.  Integer addition commutes, and so does the integer maximum that builds M and the per-sample
// scale: everything is bit-reproducible, and every sample depends on itself alone.
//
// Forward, four launches:  splat_init (clears the accumulators, the M keys and the per-sample words -- a kernel, never a memset: a
// captured memset node clears only once);  splat_scan (per-sample maximum of |x| and non-finite flag, and in soft mode the scatter-max
// of Z);  splat_scatter;  splat_finish (out, hit, D, M as fp32 planes, every element written).
// Backward, one launch: a gather per source pixel over the same four corners, no atomics.
// No host read, no memset node, no fast intrinsic (expf, IEEE division), no contraction.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
enum { MODE_SUM = 0, MODE_AVG = 1, MODE_SOFT = 2 };

// scratch: long long acc[N][C + 1][H W] (numerators, then the denominator) | unsigned keys[N][H W] | unsigned words[N][2]
//   words[n][0]: bits of the largest finite |x| of sample n, words[n][1]: != 0 iff the sample holds a non-finite element
struct Scratch {
  unsigned long long* acc;
  unsigned* keys;
  unsigned* words;
};

Scratch carve(void* scratch, int N, int C, int H, int W) {
  Scratch s;
  const size_t plane = (size_t)H * W;
  s.acc = (unsigned long long*)scratch;
  s.keys = (unsigned*)(s.acc + (size_t)N * (C + 1) * plane);
  s.words = s.keys + (size_t)N * plane;
  return s;
}

// The four corners of a source in the order (x0, y0), (x1, y0), (x0, y1), (x1, y1); bit k of `mask`: corner k takes part.
struct Corners {
  int mask;
  int t[4];        // in-plane index of the target (0 where the corner takes no part)
  double wx[2], wy[2];
};

// The coordinate, the range test, the cell and the fractions are fp32.  Every comparison that keeps a coordinate in range is made in
// float BEFORE the conversion to an integer: NaN, +-inf and 1e30 fail it.  X in (-1, W) is what any corner taking part needs.
__device__ __forceinline__ Corners corners_of(float fx, float fy, int i, int j, int H, int W) {
  Corners c;
  c.mask = 0;
  c.t[0] = c.t[1] = c.t[2] = c.t[3] = 0;
  c.wx[0] = c.wx[1] = c.wy[0] = c.wy[1] = 0.0;
  const float X = (float)j + fx, Y = (float)i + fy;
  if (!(X > -1.f && X < (float)W && Y > -1.f && Y < (float)H)) return c;
  const float xf = floorf(X), yf = floorf(Y);
  const float tx = X - xf, ty = Y - yf;
  const int x0 = (int)xf, y0 = (int)yf;                     // in [-1, W - 1], [-1, H - 1]
  c.wx[0] = 1.0 - (double)tx, c.wx[1] = (double)tx;         // exact in double
  c.wy[0] = 1.0 - (double)ty, c.wy[1] = (double)ty;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int dx = k & 1, dy = k >> 1;
    const int xx = x0 + dx, yy = y0 + dy;
    const bool ok = xx >= 0 && xx < W && yy >= 0 && yy < H && c.wx[dx] > 0.0 && c.wy[dy] > 0.0;   // on the factors, not the product
    c.t[k] = ok ? yy * W + xx : 0;
    if (ok) c.mask |= 1 << k;
  }
  return c;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }   // false for NaN

// Order-preserving key of a finite float (-0 counted as +0): key(a) < key(b) iff a < b, and no finite float has key 0 ("nothing").
__device__ __forceinline__ unsigned key_of(float z) {
  const unsigned u = __float_as_uint(z + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The fixed-point scheme of csrc/dainwarp.hip.  At most H W contributions reach one target (a source hits a target at most once), each
// at most 2^e in magnitude: with lg = ceil(log2(H W)) a scale 2^(62 - lg - e) keeps a sum below 2^62 + H W (the round-away units) < 2^63.
// The denominator's contributions are at most 1: its scale 2^(62 - lg) is a constant of the shape.
__device__ __forceinline__ int num_scale(unsigned mbits, int lg) {
  int e = 0;
  if (mbits) (void)frexpf(__uint_as_float(mbits), &e);      // max = m 2^e, m in [0.5, 1): 2^e > max
  return 62 - lg - e;                                       // in [-97, 211]: 2^k is a normal double
}
__device__ __forceinline__ double pow2d(int k) { return __longlong_as_double((long long)(k + 1023) << 52); }
__device__ __forceinline__ unsigned long long to_fixed(double v, double s) {
  const double t = v * s;
  return (unsigned long long)(long long)(t > 0.0 ? ceil(t) : floor(t));
}

__global__ __launch_bounds__(NT) void splat_init(unsigned long long* __restrict__ acc, size_t n_acc, unsigned* __restrict__ keys,
                                                 size_t n_keys) {      // keys and words are contiguous: n_keys counts both
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n_acc; i += stride) acc[i] = 0ull;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n_keys; i += stride) keys[i] = 0u;
}

// grid: (pixel blocks, channel chunks, N).  Chunk 0 also scatters the maximum of Z in soft mode.
__global__ __launch_bounds__(NT) void splat_scan(const float* __restrict__ x, const float* __restrict__ flow, const float* __restrict__ metric,
                                                 unsigned* __restrict__ keys, unsigned* __restrict__ words, int C, int H, int W, int mode,
                                                 int cpc) {
  __shared__ unsigned lds[2 * (NT / SAVFI_WAVE)];
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * cpc, c1 = min(C, c0 + cpc);
  unsigned mb = 0u, bad = 0u;
  if (p < plane) {
    const float* xs = x + ((size_t)n * C + c0) * plane + p;
    for (int c = c0; c < c1; ++c, xs += plane) {
      const float v = fabsf(*xs);
      if (v < INFINITY) mb = max(mb, __float_as_uint(v));   // non-negative floats order like their bits
      else bad = 1u;                                        // Inf or NaN
    }
    if (mode == MODE_SOFT && blockIdx.y == 0) {
      const float Z = metric[(size_t)n * plane + p];
      if (finite_f(Z)) {
        const int i = p / W, j = p - i * W;
        const Corners cn = corners_of(flow[(size_t)n * 2 * plane + p], flow[((size_t)n * 2 + 1) * plane + p], i, j, H, W);
        const unsigned key = key_of(Z);
        unsigned* kp = keys + (size_t)n * plane;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cn.mask >> k & 1) atomicMax(kp + cn.t[k], key);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mb = max(mb, (unsigned)__shfl_xor((int)mb, off, SAVFI_WAVE));
    bad |= (unsigned)__shfl_xor((int)bad, off, SAVFI_WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
    lds[2 * (threadIdx.x >> 6)] = mb;
    lds[2 * (threadIdx.x >> 6) + 1] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NT / SAVFI_WAVE; ++w) {
      mb = max(mb, lds[2 * w]);
      bad |= lds[2 * w + 1];
    }
    if (mb) atomicMax(words + 2 * n, mb);
    if (bad) atomicMax(words + 2 * n + 1, 1u);
  }
}

// grid: (pixel blocks, channel chunks, N), one thread per source pixel.  Chunk 0 also adds the denominator.
__global__ __launch_bounds__(NT) void splat_scatter(const float* __restrict__ x, const float* __restrict__ flow,
                                                    const float* __restrict__ metric, unsigned long long* __restrict__ acc,
                                                    const unsigned* __restrict__ keys, const unsigned* __restrict__ words, int C, int H,
                                                    int W, int mode, int lg, int cpc) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int n = blockIdx.z;
  float Z = 0.f;
  if (mode == MODE_SOFT) {
    Z = metric[(size_t)n * plane + p];
    if (!finite_f(Z)) return;
  }
  const int i = p / W, j = p - i * W;
  const Corners cn = corners_of(flow[(size_t)n * 2 * plane + p], flow[((size_t)n * 2 + 1) * plane + p], i, j, H, W);
  if (!cn.mask) return;
  double w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[k] = 0.0;
    if (cn.mask >> k & 1) {
      w[k] = cn.wx[k & 1] * cn.wy[k >> 1];
      if (mode == MODE_SOFT) w[k] *= (double)expf((Z + 0.0f) - key_to_float(keys[(size_t)n * plane + cn.t[k]]));   // e <= 1
    }
  }
  unsigned long long* a = acc + (size_t)n * (C + 1) * plane;
  if (blockIdx.y == 0) {
    const double sd = pow2d(62 - lg);
    unsigned long long* d = a + (size_t)C * plane;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cn.mask >> k & 1) {
        const unsigned long long q = to_fixed(w[k], sd);    // 0 only where expf underflowed to 0
        if (q) atomicAdd(d + cn.t[k], q);
      }
  }
  if (words[2 * n + 1]) return;                             // a non-finite sample: the finish writes NaN, no numerator is needed
  const double sn = pow2d(num_scale(words[2 * n], lg));
  const int c0 = blockIdx.y * cpc, c1 = min(C, c0 + cpc);
  const float* xs = x + ((size_t)n * C + c0) * plane + p;
  a += (size_t)c0 * plane;
  for (int c = c0; c < c1; ++c, xs += plane, a += plane) {
    const double xv = (double)*xs;
    if (xv == 0.0) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cn.mask >> k & 1) {
        const unsigned long long q = to_fixed(w[k] * xv, sn);
        if (q) atomicAdd(a + cn.t[k], q);
      }
  }
}

// grid: (pixel blocks, channel chunks, N), one thread per target pixel.  Chunk 0 also writes hit, D and M.
__global__ __launch_bounds__(NT) void splat_finish(const unsigned long long* __restrict__ acc, const unsigned* __restrict__ keys,
                                                   const unsigned* __restrict__ words, float* __restrict__ out, float* __restrict__ hit,
                                                   float* __restrict__ den, float* __restrict__ mx, int C, int H, int W, int mode, int lg,
                                                   int cpc) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int n = blockIdx.z;
  const long long* a = (const long long*)acc + (size_t)n * (C + 1) * plane + p;
  const long long d = a[(size_t)C * plane];
  const bool landed = d > 0;                                // rounded away from zero: positive iff something took part
  const double D = (double)d * pow2d(-(62 - lg));
  if (blockIdx.y == 0) {
    const size_t q = (size_t)n * plane + p;
    hit[q] = landed ? 1.f : 0.f;
    den[q] = (float)D;
    mx[q] = (mode == MODE_SOFT && landed) ? key_to_float(keys[q]) : 0.f;
  }
  const bool bad = words[2 * n + 1] != 0u;
  const double inv = pow2d(-num_scale(words[2 * n], lg));
  const int c0 = blockIdx.y * cpc, c1 = min(C, c0 + cpc);
  float* o = out + ((size_t)n * C + c0) * plane + p;
  a += (size_t)c0 * plane;
  for (int c = c0; c < c1; ++c, o += plane, a += plane) {
    float v = 0.f;
    if (bad) v = __uint_as_float(0x7fc00000u);
    else if (landed) {
      const double num = (double)*a * inv;
      v = (float)(mode == MODE_SUM ? num : num / D);
    }
    *o = v;
  }
}

// grid: (pixel blocks, 1, N), one thread per source pixel over all channels; sums in double, in the order of the channels and corners.
__global__ __launch_bounds__(NT) void splat_bwd(const float* __restrict__ x, const float* __restrict__ flow, const float* __restrict__ metric,
                                                const float* __restrict__ out, const float* __restrict__ den, const float* __restrict__ mx,
                                                const float* __restrict__ g_out, float* __restrict__ g_x, float* __restrict__ g_flow,
                                                float* __restrict__ g_metric, int C, int H, int W, int mode) {
  const int plane = H * W;
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= plane) return;
  const int n = blockIdx.z;
  float Z = 0.f;
  bool part = true;
  if (mode == MODE_SOFT) {
    Z = metric[(size_t)n * plane + p];
    part = finite_f(Z);
  }
  const int i = p / W, j = p - i * W;
  // a source whose metric is not finite takes no part: a NaN coordinate fails the range test
  const Corners cn = corners_of(part ? flow[(size_t)n * 2 * plane + p] : __uint_as_float(0x7fc00000u), flow[((size_t)n * 2 + 1) * plane + p],
                                i, j, H, W);
  double e[4], w[4], invD[4], s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = w[k] = invD[k] = s[k] = 0.0;
    if (cn.mask >> k & 1) {
      const size_t q = (size_t)n * plane + cn.t[k];
      e[k] = mode == MODE_SOFT ? (double)expf((Z + 0.0f) - mx[q]) : 1.0;
      w[k] = e[k] * (cn.wx[k & 1] * cn.wy[k >> 1]);
      invD[k] = mode == MODE_SUM ? 1.0 : 1.0 / (double)den[q];
    }
  }
  const size_t base = (size_t)n * C * plane;
  for (int c = 0; c < C; ++c) {
    const size_t ch = base + (size_t)c * plane;
    const double xv = (double)x[ch + p];
    double gx = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cn.mask >> k & 1) {
        const double gd = (double)g_out[ch + cn.t[k]] * invD[k];
        const double o = mode == MODE_SUM ? 0.0 : (double)out[ch + cn.t[k]];
        gx += w[k] * gd;
        s[k] += gd * (xv - o);
      }
    if (g_x) g_x[ch + p] = (float)gx;
  }
  if (g_metric) {
    double gz = 0.0;
    if (mode == MODE_SOFT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) gz += s[k] * w[k];
    }
    g_metric[(size_t)n * plane + p] = (float)gz;
  }
  if (g_flow) {
    // d b_k / dX = -wy0, +wy0, -wy1, +wy1;  d b_k / dY = -wx0, -wx1, +wx0, +wx1  (a corner that took no part has s e = 0)
    const double se[4] = {s[0] * e[0], s[1] * e[1], s[2] * e[2], s[3] * e[3]};
    const double gfx = (se[1] - se[0]) * cn.wy[0] + (se[3] - se[2]) * cn.wy[1];
    const double gfy = (se[2] - se[0]) * cn.wx[0] + (se[3] - se[1]) * cn.wx[1];
    g_flow[(size_t)n * 2 * plane + p] = (float)gfx;
    g_flow[((size_t)n * 2 + 1) * plane + p] = (float)gfy;
  }
}

bool misaligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }

int ceil_log2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

// SHAPE, then the part of UNSUPPORTED that the numbers decide
int splat_check_dims(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  if (C > 256) return SAVFI_E_UNSUPPORTED;
  return SAVFI_OK;
}

// in-plane indices are int (block * NT + thread included); grid z is 16-bit; N (C + 1) H W accumulators within 2^40
int splat_check_size(int N, int C, int H, int W) {
  if ((int64_t)H * W > 0x7fffffffLL - NT || N > 65535 || (int64_t)N * (C + 1) * H * W >= ((int64_t)1 << 40)) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

bool known_mode(int mode) { return mode == MODE_SUM || mode == MODE_AVG || mode == MODE_SOFT; }

// channel chunks: enough workgroups for 256 CUs x 8 on a small map, at least 4 channels a thread
void splat_chunks(int N, int C, int pb, int* chunks_out, int* cpc_out) {
  int chunks = savfi_cdiv(2048, (int64_t)pb * N);
  chunks = chunks < 1 ? 1 : chunks;
  int cpc = savfi_cdiv(C, chunks);
  if (cpc < 4) cpc = C < 4 ? C : 4;
  *chunks_out = savfi_cdiv(C, cpc);
  *cpc_out = cpc;
}

}  // namespace

extern "C" int64_t savfi_softsplat_scratch_bytes(int N, int C, int H, int W) {
  if (int e = splat_check_dims(N, C, H, W)) return e;
  if (int e = splat_check_size(N, C, H, W)) return e;
  const int64_t plane = (int64_t)H * W;
  const int64_t bytes = (int64_t)N * (C + 1) * plane * 8 + (int64_t)N * plane * 4 + (int64_t)N * 8;
  return (bytes + 15) & ~(int64_t)15;
}

extern "C" int savfi_softsplat_fwd_f32(const float* x, const float* flow, const float* metric, float* out, float* hit, float* den,
                                       float* mx, void* scratch, int N, int C, int H, int W, int mode, void* stream) {
  if (!x || !flow || !out || !hit || !den || !mx || !scratch) return SAVFI_E_NULL;
  if (int e = splat_check_dims(N, C, H, W)) return e;
  if (!known_mode(mode) || (mode == MODE_SOFT && !metric)) return SAVFI_E_UNSUPPORTED;
  const void* const ins[4] = {x, flow, metric, scratch};
  const void* const outs[4] = {out, hit, den, mx};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j)
      if (outs[i] == ins[j]) return SAVFI_E_UNSUPPORTED;
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) return SAVFI_E_UNSUPPORTED;
  }
  if (misaligned(x, 4) || misaligned(flow, 4) || misaligned(metric, 4) || misaligned(out, 4) || misaligned(hit, 4) || misaligned(den, 4) ||
      misaligned(mx, 4) || misaligned(scratch, 8))
    return SAVFI_E_UNSUPPORTED;
  if (int e = splat_check_size(N, C, H, W)) return e;
  hipStream_t st = (hipStream_t)stream;
  const Scratch s = carve(scratch, N, C, H, W);
  const size_t plane = (size_t)H * W;
  const size_t n_acc = (size_t)N * (C + 1) * plane, n_keys = (size_t)N * plane + 2 * (size_t)N;
  const int lg = ceil_log2((int64_t)plane);
  const int pb = savfi_cdiv((int64_t)plane, NT);
  int chunks, cpc;
  splat_chunks(N, C, pb, &chunks, &cpc);
  const dim3 grid(pb, chunks, N);
  const size_t ib = (n_acc + NT - 1) / NT;
  hipLaunchKernelGGL(splat_init, dim3((unsigned)(ib < 8192 ? ib : 8192)), dim3(NT), 0, st, s.acc, n_acc, s.keys, n_keys);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(splat_scan, grid, dim3(NT), 0, st, x, flow, metric, s.keys, s.words, C, H, W, mode, cpc);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(splat_scatter, grid, dim3(NT), 0, st, x, flow, metric, s.acc, s.keys, s.words, C, H, W, mode, lg, cpc);
  if (int e = savfi_launch_status()) return e;
  hipLaunchKernelGGL(splat_finish, grid, dim3(NT), 0, st, s.acc, s.keys, s.words, out, hit, den, mx, C, H, W, mode, lg, cpc);
  return savfi_launch_status();
}

extern "C" int savfi_softsplat_bwd_f32(const float* x, const float* flow, const float* metric, const float* out, const float* den,
                                       const float* mx, const float* g_out, float* g_x, float* g_flow, float* g_metric, int N, int C,
                                       int H, int W, int mode, void* stream) {
  if (!x || !flow || !out || !den || !mx || !g_out || (!g_x && !g_flow && !g_metric)) return SAVFI_E_NULL;
  if (int e = splat_check_dims(N, C, H, W)) return e;
  if (!known_mode(mode) || (mode == MODE_SOFT && !metric)) return SAVFI_E_UNSUPPORTED;
  const void* const ins[7] = {x, flow, metric, out, den, mx, g_out};
  float* const outs[3] = {g_x, g_flow, g_metric};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    for (int j = 0; j < 7; ++j)
      if (outs[i] == ins[j]) return SAVFI_E_UNSUPPORTED;
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) return SAVFI_E_UNSUPPORTED;
  }
  for (int j = 0; j < 7; ++j)
    if (misaligned(ins[j], 4)) return SAVFI_E_UNSUPPORTED;
  if (misaligned(g_x, 4) || misaligned(g_flow, 4) || misaligned(g_metric, 4)) return SAVFI_E_UNSUPPORTED;
  if (int e = splat_check_size(N, C, H, W)) return e;
  hipLaunchKernelGGL(splat_bwd, dim3(savfi_cdiv((int64_t)H * W, NT), 1, N), dim3(NT), 0, (hipStream_t)stream, x, flow, metric, out, den,
                     mx, g_out, g_x, g_flow, g_metric, C, H, W, mode);
  return savfi_launch_status();
}
