// tOF, the device end: dense Farneback optical flow of P pairs of planes and the mean end-point distance of two flow fields.  The
// contract is fcvsr_amd/harness/tof.py (farneback_host, epe_host): a restatement, by reading, of
// cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0); every kernel here evaluates the f32 expression tree of
// that module, in an order fixed by the image size alone, so the flow of a pair does not depend on the batch it is scored in.
// No atomics.  Per pyramid level, coarsest first:
//   (a) level_image_kernel   blur (separable Gaussian, REFLECT_101) + bilinear resize of the source planes into the level image
//   (b) poly_exp_kernel      polynomial expansion, vertical pass from an LDS tile, then the horizontal pass -> R (pixel-interleaved)
//   (c) first_matrices_kernel  flow = 2 x bilinear resize of the coarser flow (zeros at the coarsest level); M from (R0, R1, flow)
//   (d) box_solve_kernel x 3 M tile + 7-pixel halo in LDS, separable 15x15 box sums, the 2x2 solve, the flow; where another
//                            iteration follows, the gather of R1 at the new flow and the new M into the other M buffer (the box sums
//                            read the old M at neighbours: hence two buffers)
// Layouts: R is (images,h,w,8) f32 with 5 live channels - the gather reads 4 neighbours of which two are adjacent, 2 x 16 bytes
// each, and poly_exp stores 2 x 16 bytes per pixel; M is planar (P,5,h,w), what the box sums read row by row (DESIGN.md section 9
// has the byte counts).
#include <math.h>
#include "common.h"

namespace fcvsr {
namespace {

constexpr int kRC = FCVSR_FLOW_R_CHANNELS;
constexpr int kTileW = 64, kTileH = 16, kThreads = 256;   // output tile of poly_exp and box_solve: thread (tx, ty) owns rows ty + 4 j
constexpr int kRowsPerThread = kTileH / (kThreads / kTileW);
constexpr int kPolyN = 5, kPolyTaps = 2 * kPolyN + 1;
constexpr int kBoxR = 7, kBoxTaps = 2 * kBoxR + 1;
constexpr int kMaxBlurTaps = 19;                          // level 3: sigma 3.5
constexpr int kMaxLevels = 4;
constexpr int kMinSize = 32;
constexpr int kMaxSide = 16384;
constexpr int kEpePix = 4096;                             // pixels per stage-1 workgroup of the end-point distance

struct BlurTaps { float t[kMaxBlurTaps]; int r; };
struct PolyTaps { float g[kPolyTaps], xg[kPolyTaps], xxg[kPolyTaps]; float ig11, ig03, ig33, ig55; };

__constant__ float kBorder[6] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f, 1.0f};

struct Level { int h, w, ks; double sigma; };

// round-half-even of a non-negative double (the default rounding mode)
inline int round_even(double v) { return (int)nearbyint(v); }

inline int level_count(int h, int w) {
  int k = 0;
  double s = 1.0;
  while (k < 3) {
    s *= 0.5;
    if (w * s < kMinSize || h * s < kMinSize) break;
    ++k;
  }
  return k + 1;
}

inline Level level_of(int h, int w, int k) {
  const double s = 1.0 / (double)(1 << k);
  Level l;
  l.sigma = (1.0 / s - 1.0) * 0.5;
  const int ks = round_even(l.sigma * 5) | 1;
  l.ks = ks > 3 ? ks : 3;
  l.h = round_even(h * s);
  l.w = round_even(w * s);
  return l;
}

inline BlurTaps blur_taps(const Level& l) {
  BlurTaps b = {};
  b.r = (l.ks - 1) / 2;
  if (l.sigma <= 0) {
    b.t[0] = 0.25f; b.t[1] = 0.5f; b.t[2] = 0.25f;
    return b;
  }
  double g[kMaxBlurTaps], sum = 0;
  for (int i = 0; i < l.ks; ++i) {
    const double x = i - b.r;
    g[i] = exp(-(x * x) / (2.0 * l.sigma * l.sigma));
    sum += g[i];
  }
  for (int i = 0; i < l.ks; ++i) b.t[i] = (float)(g[i] / sum);
  return b;
}

// g, x g, x^2 g for sigma 1.2 and the four entries of inv(G) the expansion needs.  G, the moment matrix of [1, x, y, x^2, y^2, xy]
// under g(y) g(x), separates into [x], [y], [xy] (diagonal: m2, m2, m2^2) and the 3x3 block of [1, x^2, y^2], inverted here by
// cofactors in f64.
inline PolyTaps poly_taps() {
  PolyTaps p;
  double g[kPolyTaps], sum = 0;
  for (int i = 0; i < kPolyTaps; ++i) {
    const double x = i - kPolyN;
    g[i] = exp(-(x * x) / (2.0 * 1.2 * 1.2));
    sum += g[i];
  }
  double m0 = 0, m2 = 0, m4 = 0;
  for (int i = 0; i < kPolyTaps; ++i) {
    const double x = i - kPolyN;
    g[i] /= sum;
    p.g[i] = (float)g[i];
    p.xg[i] = (float)(x * g[i]);
    p.xxg[i] = (float)(x * x * g[i]);
    m0 += g[i];
    m2 += x * x * g[i];
    m4 += x * x * x * x * g[i];
  }
  // block A = [[a, b, b], [b, c, d], [b, d, c]] with a = m0^2, b = m0 m2, c = m0 m4, d = m2^2
  const double a = m0 * m0, b = m0 * m2, c = m0 * m4, d = m2 * m2;
  const double det = a * (c * c - d * d) - 2.0 * b * (b * c - b * d);
  p.ig11 = (float)(1.0 / (m0 * m2));
  p.ig03 = (float)(-(b * c - b * d) / det);         // cofactor (0,1) of A over det: inv(A)[0][1]
  p.ig33 = (float)((a * c - b * b) / det);          // inv(A)[1][1]
  p.ig55 = (float)(1.0 / d);
  return p;
}

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// One source sample as float.  plane: the first sample of the plane (of its R plane for RGB8); hw: samples of one plane.
template <int ELEM>
__device__ __forceinline__ float sample(const void* plane, long long i, long long hw) {
  if (ELEM == FCVSR_FLOW_U8) return (float)((const unsigned char*)plane)[i];
  if (ELEM == FCVSR_FLOW_U16) {
    const unsigned v = ((const unsigned short*)plane)[i];
    return (float)(v > 1023u ? 1023u : v);
  }
  if (ELEM == FCVSR_FLOW_F32) return ((const float*)plane)[i];
  const unsigned char* q = (const unsigned char*)plane;
  const float r = (float)q[i], g = (float)q[i + hw], b = (float)q[i + 2 * hw];
  return ((65.481f * r + 128.553f * g) + 24.966f * b) / 255.0f + 16.0f;
}

// The blurred source at (by, bx): rows first, taps ascending - tof.blur_host.
template <int ELEM>
__device__ __forceinline__ float blurred(const void* plane, int by, int bx, int h, int w, const BlurTaps& t) {
  const long long hw = (long long)h * w;
  float acc = 0.f;
  for (int ky = -t.r; ky <= t.r; ++ky) {
    const long long row = (long long)reflect101(by + ky, h) * w;
    float s = 0.f;
    for (int kx = -t.r; kx <= t.r; ++kx) s = s + t.t[kx + t.r] * sample<ELEM>(plane, row + reflect101(bx + kx, w), hw);
    acc = acc + t.t[ky + t.r] * s;
  }
  return acc;
}

// Source index pair and fraction of one axis of the bilinear resize (tof._resize_axis)
__device__ __forceinline__ void resize_axis(int i, int n_src, int n_dst, int& i0, int& i1, float& fr) {
  const float scale = (float)n_src / (float)n_dst;
  const float f = ((float)i + 0.5f) * scale - 0.5f;
  const float fl = floorf(f);
  fr = f - fl;
  const int k = (int)fl;
  i0 = clampi(k, 0, n_src - 1);
  i1 = clampi(k + 1, 0, n_src - 1);
}

// (a) grid (cdiv(wl, 64), cdiv(hl, 4), P), block 256.  out (P,hl,wl).
template <int ELEM>
__global__ __launch_bounds__(kThreads) void level_image_kernel(const void* __restrict__ src, long long stride_bytes, int h, int w, int hl,
                                                               int wl, BlurTaps t, float* __restrict__ out) {
  const int x = blockIdx.x * kTileW + threadIdx.x % kTileW, y = blockIdx.y * (kThreads / kTileW) + threadIdx.x / kTileW;
  if (x >= wl || y >= hl) return;
  const long long p = blockIdx.z;
  const void* plane = (const unsigned char*)src + p * stride_bytes;
  float v;
  if (hl == h && wl == w) {
    v = blurred<ELEM>(plane, y, x, h, w, t);            // scale 1: the fractions are 0 and the other three samples have weight 0
  } else {
    int y0, y1, x0, x1;
    float fy, fx;
    resize_axis(y, h, hl, y0, y1, fy);
    resize_axis(x, w, wl, x0, x1, fx);
    const float p00 = blurred<ELEM>(plane, y0, x0, h, w, t), p01 = blurred<ELEM>(plane, y0, x1, h, w, t);
    const float p10 = blurred<ELEM>(plane, y1, x0, h, w, t), p11 = blurred<ELEM>(plane, y1, x1, h, w, t);
    const float top = p00 * (1.0f - fx) + p01 * fx, bot = p10 * (1.0f - fx) + p11 * fx;
    v = top * (1.0f - fy) + bot * fy;
  }
  out[(p * hl + y) * wl + x] = v;
}

// (b) grid (cdiv(w, 64), cdiv(h, 16), images), block 256.  img (n,h,w) -> R (n,h,w,8).
__global__ __launch_bounds__(kThreads) void poly_exp_kernel(const float* __restrict__ img, int h, int w, PolyTaps t, float* __restrict__ R) {
  constexpr int SW = kTileW + 2 * kPolyN, SH = kTileH + 2 * kPolyN;
  __shared__ float src[SH][SW];
  __shared__ float mid[3][kTileH][SW];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const float* im = img + (long long)blockIdx.z * h * w;
  for (int i = threadIdx.x; i < SH * SW; i += kThreads) {
    const int ry = i / SW, rx = i % SW;
    src[ry][rx] = im[(long long)clampi(y0 + ry - kPolyN, 0, h - 1) * w + clampi(x0 + rx - kPolyN, 0, w - 1)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileH * SW; i += kThreads) {   // vertical: 1, y, y^2 moments of every column of the tile + halo
    const int ry = i / SW, rx = i % SW;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < kPolyTaps; ++k) {
      const float s = src[ry + k][rx];
      v0 = v0 + t.g[k] * s;
      v1 = v1 + t.xg[k] * s;
      v2 = v2 + t.xxg[k] * s;
    }
    mid[0][ry][rx] = v0;
    mid[1][ry][rx] = v1;
    mid[2][ry][rx] = v2;
  }
  __syncthreads();
  const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
  const int x = x0 + tx;
  if (x >= w) return;
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int ry = ty + j * (kThreads / kTileW), y = y0 + ry;
    if (y >= h) break;
    float b1 = 0.f, bx = 0.f, bxx = 0.f, by = 0.f, bxy = 0.f, byy = 0.f;
#pragma unroll
    for (int k = 0; k < kPolyTaps; ++k) {
      const float a0 = mid[0][ry][tx + k], a1 = mid[1][ry][tx + k], a2 = mid[2][ry][tx + k];
      b1 = b1 + t.g[k] * a0;
      bx = bx + t.xg[k] * a0;
      bxx = bxx + t.xxg[k] * a0;
      by = by + t.g[k] * a1;
      bxy = bxy + t.xg[k] * a1;
      byy = byy + t.g[k] * a2;
    }
    float4* o = (float4*)(R + (((long long)blockIdx.z * h + y) * w + x) * kRC);
    o[0] = make_float4(by * t.ig11, bx * t.ig11, b1 * t.ig03 + byy * t.ig33, b1 * t.ig03 + bxx * t.ig33);
    o[1] = make_float4(bxy * t.ig55, 0.f, 0.f, 0.f);
  }
}

// tof.matrices_host at one pixel.  R0, R1: the two expansions of this pair (h,w,8); M: the pair's (5,h,w) planes.
__device__ __forceinline__ void matrices_at(const float* __restrict__ R0, const float* __restrict__ R1, int x, int y, int h, int w,
                                            float dx, float dy, float* __restrict__ M) {
  const long long pix = (long long)y * w + x;
  const float4 a = ((const float4*)(R0 + pix * kRC))[0];
  const float c4 = R0[pix * kRC + 4];
  float fx = (float)x + dx, fy = (float)y + dy;
  const float x1f = floorf(fx), y1f = floorf(fy);
  float r2, r3, r4, r5, r6;
  if (x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1)) {
    const int x1 = (int)x1f, y1 = (int)y1f;
    fx = fx - x1f;
    fy = fy - y1f;
    const float a00 = (1.0f - fx) * (1.0f - fy), a01 = fx * (1.0f - fy), a10 = (1.0f - fx) * fy, a11 = fx * fy;
    const float* q = R1 + ((long long)y1 * w + x1) * kRC;
    const float4 p00 = ((const float4*)q)[0], p01 = ((const float4*)(q + kRC))[0];
    const float4 p10 = ((const float4*)(q + (long long)w * kRC))[0], p11 = ((const float4*)(q + (long long)(w + 1) * kRC))[0];
    const float e00 = q[4], e01 = q[kRC + 4], e10 = q[(long long)w * kRC + 4], e11 = q[(long long)(w + 1) * kRC + 4];
    r2 = a00 * p00.x + a01 * p01.x + a10 * p10.x + a11 * p11.x;
    r3 = a00 * p00.y + a01 * p01.y + a10 * p10.y + a11 * p11.y;
    r4 = a00 * p00.z + a01 * p01.z + a10 * p10.z + a11 * p11.z;
    r5 = a00 * p00.w + a01 * p01.w + a10 * p10.w + a11 * p11.w;
    r6 = a00 * e00 + a01 * e01 + a10 * e10 + a11 * e11;
    r4 = (a.z + r4) * 0.5f;
    r5 = (a.w + r5) * 0.5f;
    r6 = (c4 + r6) * 0.25f;
  } else {
    r2 = 0.f;
    r3 = 0.f;
    r4 = a.z;
    r5 = a.w;
    r6 = c4 * 0.5f;
  }
  r2 = (a.x - r2) * 0.5f;
  r3 = (a.y - r3) * 0.5f;
  r2 = r2 + r4 * dy + r6 * dx;
  r3 = r3 + r6 * dy + r5 * dx;
  const int ex = x < 5 ? x : 5, fxe = w - 1 - x < 5 ? w - 1 - x : 5, ey = y < 5 ? y : 5, fye = h - 1 - y < 5 ? h - 1 - y : 5;
  const float sc = (kBorder[ex] * kBorder[fxe]) * (kBorder[ey] * kBorder[fye]);
  r2 = r2 * sc; r3 = r3 * sc; r4 = r4 * sc; r5 = r5 * sc; r6 = r6 * sc;
  const long long hw = (long long)h * w;
  M[pix] = r4 * r4 + r6 * r6;
  M[hw + pix] = (r4 + r5) * r6;
  M[2 * hw + pix] = r5 * r5 + r6 * r6;
  M[3 * hw + pix] = r4 * r2 + r6 * r3;
  M[4 * hw + pix] = r6 * r2 + r5 * r3;
}

// (c) grid (cdiv(w, 64), cdiv(h, 4), P), block 256.  coarse: the (P,hc,wc,2) flow of the level above, or null at the coarsest level
// (zeros); flow_in: a given flow instead (the stage entry); flow_out: where the level's starting flow goes (null: not stored).
__global__ __launch_bounds__(kThreads) void first_matrices_kernel(const float* __restrict__ R0, const float* __restrict__ R1,
                                                                  const float* __restrict__ coarse, int hc, int wc,
                                                                  const float* __restrict__ flow_in, int h, int w,
                                                                  float* __restrict__ flow_out, float* __restrict__ M) {
  const int x = blockIdx.x * kTileW + threadIdx.x % kTileW, y = blockIdx.y * (kThreads / kTileW) + threadIdx.x / kTileW;
  if (x >= w || y >= h) return;
  const long long p = blockIdx.z, hw = (long long)h * w, pix = (long long)y * w + x;
  float dx = 0.f, dy = 0.f;
  if (flow_in) {
    const float2 f = ((const float2*)flow_in)[p * hw + pix];
    dx = f.x;
    dy = f.y;
  } else if (coarse) {
    int y0, y1, x0, x1;
    float fy, fx;
    resize_axis(y, hc, h, y0, y1, fy);
    resize_axis(x, wc, w, x0, x1, fx);
    const float2* c = (const float2*)coarse + p * hc * wc;
    const float2 p00 = c[(long long)y0 * wc + x0], p01 = c[(long long)y0 * wc + x1];
    const float2 p10 = c[(long long)y1 * wc + x0], p11 = c[(long long)y1 * wc + x1];
    const float tx = p00.x * (1.0f - fx) + p01.x * fx, bx = p10.x * (1.0f - fx) + p11.x * fx;
    const float ty = p00.y * (1.0f - fx) + p01.y * fx, by = p10.y * (1.0f - fx) + p11.y * fx;
    dx = (tx * (1.0f - fy) + bx * fy) * 2.0f;
    dy = (ty * (1.0f - fy) + by * fy) * 2.0f;
  }
  if (flow_out) ((float2*)flow_out)[p * hw + pix] = make_float2(dx, dy);
  matrices_at(R0 + p * hw * kRC, R1 + p * hw * kRC, x, y, h, w, dx, dy, M + p * 5 * hw);
}

// (d) grid (cdiv(w, 64), cdiv(h, 16), P), block 256.  M (P,5,h,w) -> flow (P,h,w,2); with M_next, the matrices of the new flow.
__global__ __launch_bounds__(kThreads) void box_solve_kernel(const float* __restrict__ M, const float* __restrict__ R0,
                                                             const float* __restrict__ R1, int h, int w, float* __restrict__ flow,
                                                             float* __restrict__ M_next) {
  constexpr int SW = kTileW + 2 * kBoxR, SH = kTileH + 2 * kBoxR;
  __shared__ float tile[SH][SW];
  __shared__ float vs[kTileH][SW];
  __shared__ float sums[5][kTileH][kTileW];         // a thread's own box averages, parked so the solve loop below stays rolled
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const long long p = blockIdx.z, hw = (long long)h * w;
  const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
  for (int c = 0; c < 5; ++c) {
    const float* m = M + (p * 5 + c) * hw;
#pragma unroll 2
    for (int i = threadIdx.x; i < SH * SW; i += kThreads) {
      const int ry = i / SW, rx = i % SW;
      tile[ry][rx] = m[(long long)clampi(y0 + ry - kBoxR, 0, h - 1) * w + clampi(x0 + rx - kBoxR, 0, w - 1)];
    }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < kTileH * SW; i += kThreads) {
      const int ry = i / SW, rx = i % SW;
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < kBoxTaps; ++k) v = v + tile[ry + k][rx];
      vs[ry][rx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
      const int ry = ty + j * (kThreads / kTileW);
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < kBoxTaps; ++k) v = v + vs[ry][tx + k];
      sums[c][ry][tx] = v * (float)(1.0 / (kBoxTaps * kBoxTaps));
    }
    // the next channel's tile loads touch `tile` only, and its first barrier orders them against these reads of `vs`
  }
  const int x = x0 + tx;
  if (x >= w) return;
#pragma unroll 1
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int ry = ty + j * (kThreads / kTileW), y = y0 + ry;
    if (y >= h) break;
    const float g11 = sums[0][ry][tx], g12 = sums[1][ry][tx], g22 = sums[2][ry][tx], h1 = sums[3][ry][tx], h2 = sums[4][ry][tx];
    const float idet = 1.0f / (g11 * g22 - g12 * g12 + 1e-3f);
    const float dx = (g11 * h2 - g12 * h1) * idet, dy = (g22 * h1 - g12 * h2) * idet;
    ((float2*)flow)[p * hw + (long long)y * w + x] = make_float2(dx, dy);
    if (M_next) matrices_at(R0 + p * hw * kRC, R1 + p * hw * kRC, x, y, h, w, dx, dy, M_next + p * 5 * hw);
  }
}

// End-point distance, stage 1: grid (blocks, P); partial[p][blk] = the f64 sum of this block's kEpePix pixels.  A thread adds its
// pixels (tid, tid + 256, ..) in ascending order, the block adds its threads by a fixed tree.
__global__ __launch_bounds__(kThreads) void epe_partial_kernel(const float2* __restrict__ a, const float2* __restrict__ b, long long hw,
                                                               double* __restrict__ partial) {
  __shared__ double sm[kThreads];
  const long long p = blockIdx.y, first = (long long)blockIdx.x * kEpePix;
  const long long last = first + kEpePix < hw ? first + kEpePix : hw;
  double acc = 0.0;
  for (long long i = first + threadIdx.x; i < last; i += kThreads) {
    const float2 u = a[p * hw + i], v = b[p * hw + i];
    const float ddx = u.x - v.x, ddy = u.y - v.y;
    acc += (double)sqrtf(ddx * ddx + ddy * ddy);        // the correctly rounded one (hipcc's default), as numpy's
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[p * gridDim.x + blockIdx.x] = sm[0];
}

// stage 2: grid (P); out[p] = (the sum of the plane's nparts partials, fixed order) / hw
__global__ __launch_bounds__(kThreads) void epe_finish_kernel(const double* __restrict__ partial, int nparts, long long hw,
                                                              double* __restrict__ out) {
  __shared__ double sm[kThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) acc += partial[(long long)blockIdx.x * nparts + i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sm[0] / (double)hw;
}

inline long long round4(long long v) { return (v + 3) / 4 * 4; }
inline bool size_ok(int P, int h, int w) { return P >= 0 && P <= 65535 && h >= 2 && w >= 2 && h <= kMaxSide && w <= kMaxSide; }
inline int elem_bytes(int elem) { return elem == FCVSR_FLOW_U16 ? 2 : elem == FCVSR_FLOW_F32 ? 4 : 1; }

// The scratch of a whole flow, in floats: level images of both frames, their expansions, two M buffers, and two flow buffers of the
// level-1 size (levels above 0 alternate between them; level 0 works in flow_out).  Every level reuses the level-0 sized buffers.
struct Carve { long long img, R, M, flow, total; };
inline Carve carve(int P, int h, int w) {
  const long long hw = (long long)h * w;
  Carve c;
  c.img = round4(2 * P * hw);
  c.R = 2 * P * hw * kRC;
  c.M = round4(5 * P * hw);
  const Level l1 = level_of(h, w, 1);
  c.flow = level_count(h, w) > 1 ? round4(2ll * P * l1.h * l1.w) : 0;
  c.total = c.img + c.R + 2 * c.M + 2 * c.flow;
  return c;
}

void launch_level_image(const void* src, int elem, int P, int h, int w, long long stride, const Level& l, float* out, hipStream_t st) {
  const BlurTaps t = blur_taps(l);
  const dim3 grid((unsigned)cdiv(l.w, kTileW), (unsigned)cdiv(l.h, kThreads / kTileW), (unsigned)P);
  const long long sb = stride * elem_bytes(elem);
  switch (elem) {
    case FCVSR_FLOW_U8: hipLaunchKernelGGL((level_image_kernel<FCVSR_FLOW_U8>), grid, dim3(kThreads), 0, st, src, sb, h, w, l.h, l.w, t, out); break;
    case FCVSR_FLOW_U16: hipLaunchKernelGGL((level_image_kernel<FCVSR_FLOW_U16>), grid, dim3(kThreads), 0, st, src, sb, h, w, l.h, l.w, t, out); break;
    case FCVSR_FLOW_F32: hipLaunchKernelGGL((level_image_kernel<FCVSR_FLOW_F32>), grid, dim3(kThreads), 0, st, src, sb, h, w, l.h, l.w, t, out); break;
    default: hipLaunchKernelGGL((level_image_kernel<FCVSR_FLOW_RGB8>), grid, dim3(kThreads), 0, st, src, sb, h, w, l.h, l.w, t, out); break;
  }
}

inline dim3 tile_grid(int h, int w, int n) { return dim3((unsigned)cdiv(w, kTileW), (unsigned)cdiv(h, kTileH), (unsigned)n); }
inline dim3 pixel_grid(int h, int w, int n) { return dim3((unsigned)cdiv(w, kTileW), (unsigned)cdiv(h, kThreads / kTileW), (unsigned)n); }

}  // namespace
}  // namespace fcvsr

#define FCVSR_FLOW_CHECK_SRC(src, elem, stride)                                                                                    \
  FCVSR_CHECK_ARG(elem >= FCVSR_FLOW_U8 && elem <= FCVSR_FLOW_RGB8, "elem: FCVSR_FLOW_U8, _U16, _F32 or _RGB8");                   \
  FCVSR_CHECK_ARG(stride >= 0 && stride <= (1ll << 40), "stride: 0 .. 2^40 samples");                                              \
  FCVSR_CHECK_ARG(((uintptr_t)src % elem_bytes(elem)) == 0, "planes: aligned to their sample size")

extern "C" long long fcvsr_farneback_scratch_bytes(int P, int h, int w) {
  using namespace fcvsr;
  if (!size_ok(P, h, w)) return -1;
  return carve(P, h, w).total * 4;
}

extern "C" int fcvsr_flow_level_image(const void* src, int elem, int P, int h, int w, long long stride, int level, float* out,
                                      void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(size_ok(P, h, w), "P: 0 .. 65535, h and w: 2 .. 16384");
  FCVSR_CHECK_ARG(level >= 0 && level < kMaxLevels, "level: 0 .. 3");
  if (P == 0) return 0;
  FCVSR_CHECK_ARG(src && out, "null device pointer");
  FCVSR_FLOW_CHECK_SRC(src, elem, stride);
  const Level l = level_of(h, w, level);
  FCVSR_CHECK_ARG(l.h >= 1 && l.w >= 1, "the level is empty");
  launch_level_image(src, elem, P, h, w, stride, l, out, (hipStream_t)stream);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_flow_poly_exp(const float* img, int n, int h, int w, float* R, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "n: 0 .. 65535, h and w: 1 .. 16384");
  if (n == 0) return 0;
  FCVSR_CHECK_ARG(img && R, "null device pointer");
  FCVSR_CHECK_ARG(((uintptr_t)img % 4) == 0 && ((uintptr_t)R % 16) == 0, "img: 4-byte aligned, R: 16-byte aligned");
  hipLaunchKernelGGL(poly_exp_kernel, tile_grid(h, w, n), dim3(kThreads), 0, (hipStream_t)stream, img, h, w, poly_taps(), R);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_flow_matrices(const float* R0, const float* R1, const float* flow, int P, int h, int w, float* M, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(P >= 0 && P <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "P: 0 .. 65535, h and w: 1 .. 16384");
  if (P == 0) return 0;
  FCVSR_CHECK_ARG(R0 && R1 && flow && M, "null device pointer");
  FCVSR_CHECK_ARG(((uintptr_t)R0 % 16) == 0 && ((uintptr_t)R1 % 16) == 0 && ((uintptr_t)flow % 8) == 0 && ((uintptr_t)M % 4) == 0,
                  "R0, R1: 16-byte aligned, flow: 8-byte aligned");
  hipLaunchKernelGGL(first_matrices_kernel, pixel_grid(h, w, P), dim3(kThreads), 0, (hipStream_t)stream, R0, R1, (const float*)nullptr, 0,
                     0, flow, h, w, (float*)nullptr, M);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_flow_box_solve(const float* M, int P, int h, int w, float* flow, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(P >= 0 && P <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "P: 0 .. 65535, h and w: 1 .. 16384");
  if (P == 0) return 0;
  FCVSR_CHECK_ARG(M && flow, "null device pointer");
  FCVSR_CHECK_ARG(((uintptr_t)M % 4) == 0 && ((uintptr_t)flow % 8) == 0, "M: 4-byte aligned, flow: 8-byte aligned");
  hipLaunchKernelGGL(box_solve_kernel, tile_grid(h, w, P), dim3(kThreads), 0, (hipStream_t)stream, M, (const float*)nullptr,
                     (const float*)nullptr, h, w, flow, (float*)nullptr);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_farneback_flow(const void* prev, const void* next, int elem, int P, int h, int w, long long stride_prev,
                                    long long stride_next, void* scratch, long long scratch_bytes, float* flow_out, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(size_ok(P, h, w), "P: 0 .. 65535, h and w: 2 .. 16384");
  if (P == 0) return 0;
  FCVSR_CHECK_ARG(prev && next && scratch && flow_out, "null device pointer");
  FCVSR_FLOW_CHECK_SRC(prev, elem, stride_prev);
  FCVSR_FLOW_CHECK_SRC(next, elem, stride_next);
  FCVSR_CHECK_ARG(((uintptr_t)scratch % 16) == 0 && ((uintptr_t)flow_out % 8) == 0, "scratch: 16-byte aligned, flow_out: 8-byte aligned");
  const Carve c = carve(P, h, w);
  FCVSR_CHECK_ARG(scratch_bytes >= c.total * 4, "scratch: fcvsr_farneback_scratch_bytes(P, h, w) bytes");
  hipStream_t st = (hipStream_t)stream;
  float* img = (float*)scratch;
  float* R = img + c.img;
  float* Mbuf[2] = {R + c.R, R + c.R + c.M};
  float* fbuf[2] = {Mbuf[1] + c.M, Mbuf[1] + c.M + c.flow};
  const PolyTaps pt = poly_taps();
  const int levels = level_count(h, w);
  const float* coarse = nullptr;
  int hc = 0, wc = 0;
  for (int k = levels - 1; k >= 0; --k) {
    const Level l = level_of(h, w, k);
    const long long lhw = (long long)l.h * l.w;
    launch_level_image(prev, elem, P, h, w, stride_prev, l, img, st);
    FCVSR_LAUNCH_CHECK();
    launch_level_image(next, elem, P, h, w, stride_next, l, img + P * lhw, st);
    FCVSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_exp_kernel, tile_grid(l.h, l.w, 2 * P), dim3(kThreads), 0, st, (const float*)img, l.h, l.w, pt, R);
    FCVSR_LAUNCH_CHECK();
    const float* R0 = R;
    const float* R1 = R + P * lhw * kRC;
    float* flow = k == 0 ? flow_out : fbuf[k & 1];
    hipLaunchKernelGGL(first_matrices_kernel, pixel_grid(l.h, l.w, P), dim3(kThreads), 0, st, R0, R1, coarse, hc, wc,
                       (const float*)nullptr, l.h, l.w, flow, Mbuf[0]);
    FCVSR_LAUNCH_CHECK();
    for (int i = 0; i < 3; ++i) {
      hipLaunchKernelGGL(box_solve_kernel, tile_grid(l.h, l.w, P), dim3(kThreads), 0, st, (const float*)Mbuf[i & 1], R0, R1, l.h, l.w,
                         flow, i < 2 ? Mbuf[(i + 1) & 1] : (float*)nullptr);
      FCVSR_LAUNCH_CHECK();
    }
    coarse = flow;
    hc = l.h;
    wc = l.w;
  }
  return 0;
}

extern "C" long long fcvsr_flow_epe_scratch_bytes(int P, int h, int w) {
  using namespace fcvsr;
  if (P < 0 || P > 65535 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return -1;
  return (long long)P * cdiv((long long)h * w, kEpePix) * 8;
}

extern "C" int fcvsr_flow_epe(const float* flow_a, const float* flow_b, int P, int h, int w, void* scratch, long long scratch_bytes,
                              double* out, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(P >= 0 && P <= 65535 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "P: 0 .. 65535, h and w: 1 .. 16384");
  if (P == 0) return 0;
  FCVSR_CHECK_ARG(flow_a && flow_b && scratch && out, "null device pointer");
  FCVSR_CHECK_ARG(((uintptr_t)flow_a % 8) == 0 && ((uintptr_t)flow_b % 8) == 0 && ((uintptr_t)scratch % 8) == 0 && ((uintptr_t)out % 8) == 0,
                  "flows, scratch and out: 8-byte aligned");
  const long long hw = (long long)h * w;
  const int nparts = cdiv(hw, kEpePix);
  FCVSR_CHECK_ARG(scratch_bytes >= (long long)P * nparts * 8, "scratch: fcvsr_flow_epe_scratch_bytes(P, h, w) bytes");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(epe_partial_kernel, dim3((unsigned)nparts, (unsigned)P), dim3(kThreads), 0, st, (const float2*)flow_a,
                     (const float2*)flow_b, hw, (double*)scratch);
  FCVSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(epe_finish_kernel, dim3((unsigned)P), dim3(kThreads), 0, st, (const double*)scratch, nparts, hw, out);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
