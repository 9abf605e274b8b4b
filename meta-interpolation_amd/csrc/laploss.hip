// Laplacian-pyramid L1 term `Lap` of --loss and its gradient for gfx950 (definition: include/savfi_hip.h, tests/laploss_ref.py).
//   g = [1, 4, 6, 4, 1] / 16, window g g^T, reflected borders (pad 2).  c_0 = sr - hr (the pyramid is linear: one pyramid of the
//   difference).  c_{s+1} = (G c_s)[::2, ::2]; b_s = c_s - 4 G z_s, z_s = c_{s+1} at the even positions of an H_s x W_s map of zeros;
//   b_{L-1} = c_{L-1}.  lap = sum_s 2^s sum |b_s| / n_0.
//
// Forward: lap_level, one launch per filtered level s = 0 .. L - 2, grid (cdiv(W_s, 32), cdiv(H_s, 32), rows * C).  A workgroup stages
// the 39 x 39 patch of c_s around its 32 x 32 tile (reflection applied while loading; level 0 forms sr - hr there), filters it
// separably into the 18 x 18 values of c_{s+1} that its bands need (the 16 x 16 it owns go to scratch; the ring is recomputed, from
// the same values in the same order, hence with the bits its owner writes), inserts the zeros, filters again and adds |b_s| over its
// tile: one partial sum per workgroup.  lap_finish adds the residual level and all partial sums of a row in a fixed order.
//
// Backward: lap_bwd_level, coarse to fine, ONE launch per level (the adjoint of the up-sampling is folded in):
//   g_{c_s} = q_s + G^T D^T (g_{c_{s+1}} - U^T q_s),   q_s = g_row 2^s / n_0 sign(b_s),   U^T q = 4 (G^T q)[::2, ::2]
// G^T, the adjoint of filtering a reflected map, is written as a gather with folded border weights (adj_w), as reflect_pad_bwd does.
// sign(b_s) is recomputed from c_s and c_{s+1} (scratch; sr - hr on level 0) through the SAME device functions as the forward (tap5,
// band; explicit fmaf chains, so no contraction can differ between the two sites): the backward uses the signs the forward summed.
// The residual level's gradient g 2^{L-1} / n_0 sign(c_{L-1}) is formed inside the launch of level L - 2.
//
// Every band element is fp32.  The SUMS of |b| are carried in double from a thread's four values on (partials are doubles): the
// value's gate is 4 ulp of a result near 0.5, which an fp32 tree over 10^4 .. 10^6 terms does not hold with margin.
// No atomics, no cleared memory, no host read: capturable, bit-reproducible.  All global accesses are scalar 4-byte ones: operands
// 4 or 8 bytes off a 16-byte boundary take the same path and give the same bits.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / SAVFI_WAVE;
constexpr int T = 32;              // tile side (even: a tile starts on an even row / column of every level)
constexpr int FP = T + 7;          // patch of c_s: rows y0 - 4 .. y0 + T + 2
constexpr int FPS = FP + 1;        // its row stride
constexpr int CP = T / 2 + 2;      // patch of c_{s+1}: rows y0 / 2 - 1 .. y0 / 2 + T / 2
constexpr int ZP = T + 4;          // zero-inserted map around the tile: rows y0 - 2 .. y0 + T + 1
constexpr int ZB = T + 11;         // the same around the backward's 39 x 39 band patch: rows y0 - 6 .. y0 + T + 4
constexpr int ZBS = ZB + 1;
constexpr int MAX_LEVELS = 5;

__device__ __forceinline__ float gk(int k) { return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f); }

// one 5-tap pass, the same association wherever it is used
__device__ __forceinline__ float tap5(float v0, float v1, float v2, float v3, float v4) {
  float a = 0.0625f * v0;
  a = fmaf(0.25f, v1, a);
  a = fmaf(0.375f, v2, a);
  a = fmaf(0.25f, v3, a);
  a = fmaf(0.0625f, v4, a);
  return a;
}

// b = c - 4 (G z)
__device__ __forceinline__ float band(float c, float gz) { return fmaf(-4.f, gz, c); }

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// reflection about the border samples, for p in [-2, n + 1] (n >= 3); anything farther out is clamped (such values are never used)
__device__ __forceinline__ int reflect_clamped(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return p < 0 ? 0 : (p >= n ? n - 1 : p);
}

// Weight of input sample o in (G^T v)[y] along one axis of length n: sum of g[a] over the taps a with reflect(o + a - 2) == y.
// The direct tap, plus the tap that reaches y through the left / top pad, plus the one through the right / bottom pad.
__device__ __forceinline__ float adj_w(int o, int y, int n) {
  if (o < 0 || o >= n) return 0.f;
  float w = 0.f;
  const int d = y - o + 2;
  if (d >= 0 && d <= 4) w += gk(d);
  if (y >= 1 && y + o <= 2) w += gk(2 - y - o);
  if (y <= n - 2 && y + o >= 2 * n - 4) w += gk(2 * n - y - o);
  return w;
}

// Zero-inserted map around a tile -> LDS [ROWS][STRIDE], entry (r, c) = position (oy + r, ox + c) of the H x W level, reflected.
// `coarse(i, j)` returns c_{s+1}[i][j] for 0 <= i < ceil(H / 2), 0 <= j < ceil(W / 2).
template <int ROWS, int STRIDE, typename F>
__device__ __forceinline__ void fill_zero_inserted(float* __restrict__ dst, int oy, int ox, int H, int W, F coarse) {
  for (int i = threadIdx.x; i < ROWS * ROWS; i += NT) {
    const int r = i / ROWS, c = i - r * ROWS;
    const int zy = oy + r, zx = ox + c;
    float v = 0.f;
    if (zy >= -2 && zy <= H + 1 && zx >= -2 && zx <= W + 1) {
      const int ry = reflect_clamped(zy, H), rx = reflect_clamped(zx, W);
      if (((ry | rx) & 1) == 0) v = coarse(ry >> 1, rx >> 1);
    }
    dst[r * STRIDE + c] = v;
  }
}

// One filtered level.  a: c_s (level 0: sr, and b = hr), planes of H x W; cnext: c_{s+1}, planes of h2 x w2;
// partial[(z * gridDim.y + by) * gridDim.x + bx] = sum |b_s| over the tile.
template <bool FIRST>
__global__ __launch_bounds__(NT) void lap_level(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ cnext,
                                                double* __restrict__ partial, int H, int W, int h2, int w2) {
  __shared__ float fp[FP * FPS];
  __shared__ float tmp[FP * CP];
  __shared__ float cn[CP * CP];
  __shared__ float zp[ZP * ZP];
  __shared__ float uh[ZP * T];
  __shared__ double red[NW];
  const int z = blockIdx.z;
  const int y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t plane = (size_t)z * H * W;
  const float* pa = a + plane;
  const float* pb = FIRST ? b + plane : nullptr;

  for (int i = threadIdx.x; i < FP * FP; i += NT) {
    const int r = i / FP, c = i - r * FP;
    const int gy = reflect_clamped(y0 - 4 + r, H), gx = reflect_clamped(x0 - 4 + c, W);
    const int at = gy * W + gx;
    float v = pa[at];
    if (FIRST) v -= pb[at];
    fp[r * FPS + c] = v;
  }
  __syncthreads();

  // c_{s+1}: rows first (coarse column j <-> patch columns 2 j .. 2 j + 4), then columns
  for (int i = threadIdx.x; i < FP * CP; i += NT) {
    const int r = i / CP, j = i - r * CP;
    const float* p = fp + r * FPS + 2 * j;
    tmp[r * CP + j] = tap5(p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();
  const int cy0 = y0 / 2 - 1, cx0 = x0 / 2 - 1;
  float* pn = cnext + (size_t)z * h2 * w2;
  for (int i = threadIdx.x; i < CP * CP; i += NT) {
    const int r = i / CP, j = i - r * CP;
    const float* p = tmp + 2 * r * CP + j;
    const int ci = cy0 + r, cj = cx0 + j;
    float v = 0.f;
    if (ci >= 0 && ci < h2 && cj >= 0 && cj < w2) {
      v = tap5(p[0], p[CP], p[2 * CP], p[3 * CP], p[4 * CP]);
      if (r >= 1 && r <= T / 2 && j >= 1 && j <= T / 2) pn[ci * w2 + cj] = v;      // the 16 x 16 this workgroup owns
    }
    cn[r * CP + j] = v;
  }
  __syncthreads();

  fill_zero_inserted<ZP, ZP>(zp, y0 - 2, x0 - 2, H, W, [&](int ci, int cj) {
    const int r = ci - cy0, j = cj - cx0;
    return (r >= 0 && r < CP && j >= 0 && j < CP) ? cn[r * CP + j] : 0.f;
  });
  __syncthreads();
  for (int i = threadIdx.x; i < ZP * T; i += NT) {
    const int r = i / T, c = i - r * T;
    const float* p = zp + r * ZP + c;
    uh[r * T + c] = tap5(p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();

  // thread = one column of the tile, four consecutive rows
  const int c = threadIdx.x & (T - 1), r0 = (threadIdx.x / T) * 4;
  double sum = 0.0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int r = r0 + o;
    const float* p = uh + r * T + c;
    const float bv = band(fp[(r + 4) * FPS + c + 4], tap5(p[0], p[T], p[2 * T], p[3 * T], p[4 * T]));
    if (y0 + r < H && x0 + c < W) sum += (double)fabsf(bv);
  }
  const double tot = block_sum_d<NW>(sum, red);
  if (threadIdx.x == 0) partial[((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

struct LapFinish {
  int64_t partial[MAX_LEVELS];      // offset of the level's partial sums in the scratch, in doubles
  int blocks[MAX_LEVELS];           // partial sums per row
  int levels;
  int64_t last;                     // offset of c_{L-1}, in floats
  int last_n;                       // its elements per row
  double inv_n0;
};

// result[row] = (sum_s 2^s (partial sums of level s) + 2^{L-1} sum |c_{L-1}|) / n_0: thread-strided, then a butterfly -- one order
__global__ __launch_bounds__(NT) void lap_finish(const void* __restrict__ scratch, float* __restrict__ result, LapFinish f) {
  __shared__ double red[NW];
  const int row = blockIdx.x;
  double acc = 0.0;
  double scale = 1.0;
  for (int s = 0; s + 1 < f.levels; ++s) {
    const double* p = (const double*)scratch + f.partial[s] + (size_t)row * f.blocks[s];
    double a = 0.0;
    for (int i = threadIdx.x; i < f.blocks[s]; i += NT) a += p[i];
    acc += scale * a;
    scale *= 2.0;
  }
  const float* c = (const float*)scratch + f.last + (size_t)row * f.last_n;
  double a = 0.0;
  for (int i = threadIdx.x; i < f.last_n; i += NT) a += (double)fabsf(c[i]);
  acc += scale * a;
  const double tot = block_sum_d<NW>(acc, red);
  if (threadIdx.x == 0) result[row] = (float)(tot * f.inv_n0);
}

// The gradient of one level.  a (b): c_s as in lap_level; cnext: c_{s+1}; gcn: g_{c_{s+1}} (LASTPAIR: unused, level s + 1 is the
// residual and its gradient g scale_n sign(c_{s+1}) is formed here); out: g_{c_s} (level 0: g_sr), every element written once.
template <bool FIRST, bool LASTPAIR>
__global__ __launch_bounds__(NT) void lap_bwd_level(const float* __restrict__ a, const float* __restrict__ b,
                                                    const float* __restrict__ cnext, const float* __restrict__ gcn,
                                                    const float* __restrict__ g_loss, float* __restrict__ out, int C, int H, int W, int h2,
                                                    int w2, float scale_s, float scale_n) {
  __shared__ float q[FP * FPS];      // c_s, then q_s in place
  __shared__ float zb[ZB * ZBS];
  __shared__ float uh[ZB * FP];
  __shared__ float t1[FP * CP];
  __shared__ float rr[CP * CP];
  __shared__ float t2[CP * T];
  const int z = blockIdx.z;
  const int y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t plane = (size_t)z * H * W;
  const float* pa = a + plane;
  const float* pb = FIRST ? b + plane : nullptr;
  const float* pn = cnext + (size_t)z * h2 * w2;
  const float g = g_loss[z / C];
  const float qs = g * scale_s;

  for (int i = threadIdx.x; i < FP * FP; i += NT) {
    const int r = i / FP, c = i - r * FP;
    const int gy = y0 - 4 + r, gx = x0 - 4 + c;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int at = gy * W + gx;
      v = pa[at];
      if (FIRST) v -= pb[at];
    }
    q[r * FPS + c] = v;
  }
  fill_zero_inserted<ZB, ZBS>(zb, y0 - 6, x0 - 6, H, W, [&](int ci, int cj) { return pn[ci * w2 + cj]; });
  __syncthreads();
  // G z_s: rows (uh column c <-> position x0 - 4 + c), then columns, then the band and its sign -- the forward's functions
  for (int i = threadIdx.x; i < ZB * FP; i += NT) {
    const int r = i / FP, c = i - r * FP;
    const float* p = zb + r * ZBS + c;
    uh[r * FP + c] = tap5(p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FP * FP; i += NT) {
    const int r = i / FP, c = i - r * FP;
    const int gy = y0 - 4 + r, gx = x0 - 4 + c;
    const float* p = uh + r * FP + c;
    const float bv = band(q[r * FPS + c], tap5(p[0], p[FP], p[2 * FP], p[3 * FP], p[4 * FP]));
    q[r * FPS + c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? qs * sgn(bv) : 0.f;
  }
  __syncthreads();

  // r = g_{c_{s+1}} - 4 (G^T q)[::2, ::2] on the 18 x 18 coarse patch: rows, then columns
  const int cy0 = y0 / 2 - 1, cx0 = x0 / 2 - 1;
  for (int i = threadIdx.x; i < FP * CP; i += NT) {
    const int r = i / CP, j = i - r * CP;
    const int cj = cx0 + j;
    float acc = 0.f;
    if (cj >= 0 && cj < w2) {
      const float* p = q + r * FPS + 2 * j;
#pragma unroll
      for (int k = 0; k < 5; ++k) acc = fmaf(adj_w(2 * cj - 2 + k, 2 * cj, W), p[k], acc);
    }
    t1[r * CP + j] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CP * CP; i += NT) {
    const int r = i / CP, j = i - r * CP;
    const int ci = cy0 + r, cj = cx0 + j;
    float v = 0.f;
    if (ci >= 0 && ci < h2 && cj >= 0 && cj < w2) {
      const float* p = t1 + 2 * r * CP + j;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) acc = fmaf(adj_w(2 * ci - 2 + k, 2 * ci, H), p[k * CP], acc);
      const float gc = LASTPAIR ? (g * scale_n) * sgn(pn[ci * w2 + cj]) : gcn[(size_t)z * h2 * w2 + ci * w2 + cj];
      v = fmaf(-4.f, acc, gc);
    }
    rr[r * CP + j] = v;
  }
  __syncthreads();

  // g_{c_s} = q + G^T (r at the even positions): rows, then columns
  for (int i = threadIdx.x; i < CP * T; i += NT) {
    const int r = i / T, c = i - r * T;
    const int x = x0 + c;
    float acc = 0.f;
#pragma unroll
    for (int k = -2; k <= 2; ++k) {
      const int ox = x + k;
      if ((ox & 1) == 0 && ox >= 0 && ox < W) acc = fmaf(adj_w(ox, x, W), rr[r * CP + (ox >> 1) - cx0], acc);
    }
    t2[r * T + c] = acc;
  }
  __syncthreads();
  const int c = threadIdx.x & (T - 1), r0 = (threadIdx.x / T) * 4;
  const int x = x0 + c;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = y0 + r0 + o;
    if (y < H && x < W) {
      float acc = 0.f;
#pragma unroll
      for (int k = -2; k <= 2; ++k) {
        const int oy = y + k;
        if ((oy & 1) == 0 && oy >= 0 && oy < H) acc = fmaf(adj_w(oy, y, H), t2[((oy >> 1) - cy0) * T + c], acc);
      }
      out[plane + (size_t)y * W + x] = q[(r0 + o + 4) * FPS + c + 4] + acc;
    }
  }
}

// NULL is checked by the callers; then SHAPE (with `levels` clamped into 2..5, so that the order holds for any `levels`),
// UNSUPPORTED, TOOBIG (the limits of the SSIM entries).
int lap_check(int rows, int C, int H, int W, int levels) {
  if (rows <= 0 || C <= 0 || H <= 0 || W <= 0) return SAVFI_E_SHAPE;
  const int L = levels < 2 ? 2 : (levels > MAX_LEVELS ? MAX_LEVELS : levels);
  int h = H, w = W;
  for (int s = 0; s + 1 < L; ++s) {      // every filtered level reflects by 2
    if (h < 3 || w < 3) return SAVFI_E_SHAPE;
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  if (levels < 2 || levels > MAX_LEVELS) return SAVFI_E_UNSUPPORTED;
  if ((int64_t)rows * C > 65535 || (int64_t)H * W > 0x7fffffffLL) return SAVFI_E_TOOBIG;
  return SAVFI_OK;
}

// Where everything lies in the scratch, in 32-bit words; every region starts on a multiple of four words (see savfi_hip.h).
struct LapPlan {
  int h[MAX_LEVELS], w[MAX_LEVELS], tx[MAX_LEVELS], ty[MAX_LEVELS];
  int64_t c[MAX_LEVELS];            // c_s, s = 1 .. L - 1
  int64_t g[MAX_LEVELS];            // g_{c_s}, s = 1 .. L - 2
  int64_t partial[MAX_LEVELS];      // doubles, s = 0 .. L - 2
  int64_t words;
};

LapPlan lap_plan(int rows, int C, int H, int W, int levels) {
  LapPlan p;
  const int64_t planes = (int64_t)rows * C;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  p.h[0] = H;
  p.w[0] = W;
  for (int s = 1; s < levels; ++s) {
    p.h[s] = (p.h[s - 1] + 1) / 2;
    p.w[s] = (p.w[s - 1] + 1) / 2;
  }
  int64_t at = 0;
  for (int s = 1; s < levels; ++s) {
    p.c[s] = at;
    at += up4(planes * p.h[s] * p.w[s]);
  }
  for (int s = 1; s + 1 < levels; ++s) {
    p.g[s] = at;
    at += up4(planes * p.h[s] * p.w[s]);
  }
  for (int s = 0; s + 1 < levels; ++s) {
    p.tx[s] = savfi_cdiv(p.w[s], T);
    p.ty[s] = savfi_cdiv(p.h[s], T);
    p.partial[s] = at;
    at += up4(2 * planes * p.tx[s] * p.ty[s]);
  }
  p.words = at;
  return p;
}

}  // namespace

extern "C" int64_t savfi_laploss_scratch_bytes(int rows, int C, int H, int W, int levels) {
  if (int e = lap_check(rows, C, H, W, levels)) return e;
  return lap_plan(rows, C, H, W, levels).words * (int64_t)sizeof(float);
}

extern "C" int savfi_laploss_f32(const float* sr, const float* hr, float* result, void* scratch, int rows, int C, int H, int W,
                                 int levels, void* stream) {
  if (!sr || !hr || !result || !scratch) return SAVFI_E_NULL;
  if (int e = lap_check(rows, C, H, W, levels)) return e;
  const LapPlan p = lap_plan(rows, C, H, W, levels);
  float* base = (float*)scratch;
  hipStream_t st = (hipStream_t)stream;
  LapFinish f;
  f.levels = levels;
  for (int s = 0; s + 1 < levels; ++s) {
    const dim3 grid(p.tx[s], p.ty[s], rows * C);
    double* partial = (double*)(base + p.partial[s]);
    if (s == 0) {
      hipLaunchKernelGGL(lap_level<true>, grid, dim3(NT), 0, st, sr, hr, base + p.c[1], partial, p.h[0], p.w[0], p.h[1], p.w[1]);
    } else {
      hipLaunchKernelGGL(lap_level<false>, grid, dim3(NT), 0, st, base + p.c[s], nullptr, base + p.c[s + 1], partial, p.h[s], p.w[s],
                         p.h[s + 1], p.w[s + 1]);
    }
    if (int e = savfi_launch_status()) return e;
    f.partial[s] = p.partial[s] / 2;
    f.blocks[s] = C * p.tx[s] * p.ty[s];
  }
  f.last = p.c[levels - 1];
  f.last_n = C * p.h[levels - 1] * p.w[levels - 1];
  f.inv_n0 = 1.0 / ((double)C * H * W);
  hipLaunchKernelGGL(lap_finish, dim3(rows), dim3(NT), 0, st, scratch, result, f);
  return savfi_launch_status();
}

extern "C" int savfi_laploss_bwd_f32(const float* sr, const float* hr, const float* g_loss, void* scratch, float* g_sr, int rows, int C,
                                     int H, int W, int levels, void* stream) {
  if (!sr || !hr || !g_loss || !scratch || !g_sr) return SAVFI_E_NULL;
  if (int e = lap_check(rows, C, H, W, levels)) return e;
  const LapPlan p = lap_plan(rows, C, H, W, levels);
  float* base = (float*)scratch;
  hipStream_t st = (hipStream_t)stream;
  const double n0 = (double)C * H * W;
  for (int s = levels - 2; s >= 0; --s) {
    const bool lastpair = s == levels - 2;
    const float scale_s = (float)((double)(1 << s) / n0), scale_n = (float)((double)(1 << (s + 1)) / n0);
    const float* cn = base + p.c[s + 1];
    const float* gcn = lastpair ? nullptr : base + p.g[s + 1];
    const dim3 grid(p.tx[s], p.ty[s], rows * C);
    const int h = p.h[s], w = p.w[s], h2 = p.h[s + 1], w2 = p.w[s + 1];
    if (s == 0) {
      if (lastpair) {
        hipLaunchKernelGGL((lap_bwd_level<true, true>), grid, dim3(NT), 0, st, sr, hr, cn, gcn, g_loss, g_sr, C, h, w, h2, w2, scale_s, scale_n);
      } else {
        hipLaunchKernelGGL((lap_bwd_level<true, false>), grid, dim3(NT), 0, st, sr, hr, cn, gcn, g_loss, g_sr, C, h, w, h2, w2, scale_s, scale_n);
      }
    } else {
      const float* cs = base + p.c[s];
      float* gs = base + p.g[s];
      if (lastpair) {
        hipLaunchKernelGGL((lap_bwd_level<false, true>), grid, dim3(NT), 0, st, cs, nullptr, cn, gcn, g_loss, gs, C, h, w, h2, w2, scale_s, scale_n);
      } else {
        hipLaunchKernelGGL((lap_bwd_level<false, false>), grid, dim3(NT), 0, st, cs, nullptr, cn, gcn, g_loss, gs, C, h, w, h2, w2, scale_s, scale_n);
      }
    }
    if (int e = savfi_launch_status()) return e;
  }
  return SAVFI_OK;
}
