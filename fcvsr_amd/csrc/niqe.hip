// NIQE block features on the device, and the MATLAB-style antialiased bicubic down-scale NIQE needs between its two scales.
// Replaces the per-frame CPU loop of the reference's no-reference scoring (mmedit/core/evaluation/metrics.py:398-590
// estimate_aggd_param / compute_feature / niqe_core / niqe; mmedit/datasets/pipelines/matlab_like_resize.py); the contract is
// fcvsr_amd/harness/niqe.py.  The 36 x 36 multivariate-Gaussian distance stays on the host.
//
// fcvsr_niqe_features, five launches on one stream, no host sync:
//   1. plane      the scored plane (crop_border off each side, then the top-left multiple of 96) as f64 integers: uint8 samples, or
//                 f32 samples quantised as the frame metrics do, or the rounded Y of RGB;
//   2. mscn       scale 1: mu and sigma from the 7 x 7 window with replicated borders (49 taps from a haloed LDS tile, accumulated
//                 from 0 in row-major tap order as the contract does), mscn = (img - mu) / (sigma + 1), f64;
//   3. downscale  the 2x down-scale of plane / 255, times 255;
//   4. mscn       scale 2;
//   5. block      one workgroup per (96/s x 96/s block, scale, frame): the six sums of each of the five distributions (the block and
//                 its four circularly shifted products), a fixed-shape reduction (xor butterflies inside a wave, then the four waves
//                 in order: no atomics, the same input gives the same bits), the 9801-entry grid search for alpha (first minimum;
//                 index 0 when the target is NaN) and the 18 features.
// The planes travel through HBM as f64: 2.5 planes written and read per frame (scratch), 16.8 MB for the 672 x 1248 scored plane of
// a 720 x 1280 frame.
// The down-scale has the reference's arithmetic and so its bits: each pass reads f32, every tap's product is an f32 and the
// products are added in tap order in f32 (no FMA: the library is built with -ffp-contract=off).  fcvsr_bicubic_downscale is the
// same device function at 2x or 4x on uint8 / f32 planes, both passes in one launch.
#include "common.h"

namespace {

constexpr int kBlock = 96, kGrid = 9801, kMY = 16, kMX = 64, kHalo = 3, kOY = 8, kOX = 32;

struct NiqeSrc {
  const void* p;
  long long sn, sc, sy, sx;
  int quantise, to_y, crop;
};

struct Window49 {
  double f[49];                          // the correlation taps: the model's window flipped in both axes
};

// one sample as the uint8 frame the harness would write (quality.hip sr_value)
__device__ inline double niqe_sample(const NiqeSrc& a, long long off) {
  if (a.quantise == FCVSR_QUANT_NONE) return (double)((const unsigned char*)a.p)[off];
  const float q = fminf(fmaxf(((const float*)a.p)[off], 0.f), 1.f) * 255.0f;
  return (double)(a.quantise == FCVSR_QUANT_TRUNCATE ? truncf(q) : rintf(q));
}

__global__ __launch_bounds__(256) void niqe_plane_kernel(NiqeSrc a, int Hc, int Wc, double* __restrict__ plane) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= Wc) return;
  const long long off = n * a.sn + (long long)(a.crop + y) * a.sy + (long long)(a.crop + x) * a.sx;
  double v;
  if (a.to_y) {
    // Y of YCbCr as quality.hip y_of (metrics.py to_y_channel), then round half to even as the reference's niqe() does
    const double r = niqe_sample(a, off), g = niqe_sample(a, off + a.sc), b = niqe_sample(a, off + 2 * a.sc);
    v = rint((b / 255.0) * 24.966 + (g / 255.0) * 128.553 + (r / 255.0) * 65.481 + 16.0);
  } else {
    v = niqe_sample(a, off);
  }
  plane[((long long)n * Hc + y) * Wc + x] = v;
}

__global__ __launch_bounds__(256) void niqe_mscn_kernel(const double* __restrict__ img, int H, int W, Window49 w,
                                                        double* __restrict__ out) {
  __shared__ double s[kMY + 2 * kHalo][kMX + 2 * kHalo];
  const int y0 = blockIdx.y * kMY, x0 = blockIdx.x * kMX;
  const double* p = img + (long long)blockIdx.z * H * W;
  double* o = out + (long long)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < (kMY + 2 * kHalo) * (kMX + 2 * kHalo); i += 256) {
    const int r = i / (kMX + 2 * kHalo), q = i % (kMX + 2 * kHalo);
    const int yy = min(max(y0 + r - kHalo, 0), H - 1), xx = min(max(x0 + q - kHalo, 0), W - 1);     // replicated border
    s[r][q] = p[(long long)yy * W + xx];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kMY * kMX; i += 256) {
    const int r = i / kMX, q = i % kMX;
    if (y0 + r >= H || x0 + q >= W) continue;
    double mu = 0.0, e2 = 0.0;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const double v = s[r + ky][q + kx];
        mu += w.f[ky * 7 + kx] * v;
        e2 += w.f[ky * 7 + kx] * (v * v);
      }
    const double sigma = sqrt(fabs(e2 - mu * mu));
    o[(long long)(y0 + r) * W + x0 + q] = (s[r + kHalo][q + kHalo] - mu) / (sigma + 1.0);
  }
}

// antialiased cubic taps F * cubic(x / F): multiples of 1/256 (2x) and 1/4096 (4x), exact in f32
template <int F> struct Taps;
template <> struct Taps<2> {
  static constexpr int K = 8;
  __device__ static float w(int k) {
    constexpr float t[8] = {-3.f / 256, -9.f / 256, 29.f / 256, 111.f / 256, 111.f / 256, 29.f / 256, -9.f / 256, -3.f / 256};
    return t[k];
  }
};
template <> struct Taps<4> {
  static constexpr int K = 16;
  __device__ static float w(int k) {
    constexpr float t[16] = {-7.f / 4096,  -45.f / 4096, -75.f / 4096, -49.f / 4096, 93.f / 4096,  399.f / 4096, 745.f / 4096, 987.f / 4096,
                             987.f / 4096, 745.f / 4096, 399.f / 4096, 93.f / 4096,  -49.f / 4096, -75.f / 4096, -45.f / 4096, -7.f / 4096};
    return t[k];
  }
};

// out-of-range indices reflected with edge repeat (-1 -> 0, -2 -> 1, n -> n-1), periodic in 2n as the reference's index table
__device__ inline int reflect(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

enum { SRC_U8 = 0, SRC_F32 = 1, SRC_NIQE = 2 };   // SRC_NIQE: f64 plane of integers, read as f32(v / 255), stored as f64 * 255

// One launch, both passes: a workgroup makes kOY x kOX outputs of one plane.  Rows first (dim 0), then columns; every pass's input
// is an f32, products are f32 and are added in tap order.
template <int F, int MODE>
__global__ __launch_bounds__(256) void downscale_kernel(const void* __restrict__ src, int H, int W, void* __restrict__ dst) {
  constexpr int K = Taps<F>::K, first = F / 2 - K / 2;      // tap 0 of output i reads input F i + first
  constexpr int IY = (kOY - 1) * F + K, IX = (kOX - 1) * F + K;
  __shared__ float in[IY][IX];
  __shared__ float mid[kOY][IX];
  const int Ho = H / F, Wo = W / F;
  const int oy0 = blockIdx.y * kOY, ox0 = blockIdx.x * kOX;
  const long long pl = blockIdx.z;
  for (int i = threadIdx.x; i < IY * IX; i += 256) {
    const int r = i / IX, q = i % IX;
    const long long off = pl * H * W + (long long)reflect(oy0 * F + first + r, H) * W + reflect(ox0 * F + first + q, W);
    float v;
    if constexpr (MODE == SRC_U8) v = (float)((const unsigned char*)src)[off];
    else if constexpr (MODE == SRC_F32) v = ((const float*)src)[off];
    else v = (float)(((const double*)src)[off] / 255.0);
    in[r][q] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kOY * IX; i += 256) {
    const int r = i / IX, q = i % IX;
    float acc = Taps<F>::w(0) * in[r * F][q];
#pragma unroll
    for (int k = 1; k < K; ++k) acc = acc + Taps<F>::w(k) * in[r * F + k][q];
    mid[r][q] = acc;
  }
  __syncthreads();
  const int r = threadIdx.x / kOX, c = threadIdx.x % kOX;   // 256 threads = kOY x kOX outputs
  if (oy0 + r < Ho && ox0 + c < Wo) {
    float acc = Taps<F>::w(0) * mid[r][c * F];
#pragma unroll
    for (int k = 1; k < K; ++k) acc = acc + Taps<F>::w(k) * mid[r][c * F + k];
    const long long o = pl * Ho * Wo + (long long)(oy0 + r) * Wo + ox0 + c;
    if constexpr (MODE == SRC_NIQE) ((double*)dst)[o] = (double)acc * 255.0;
    else ((float*)dst)[o] = acc;
  }
}
static_assert(kOY * kOX == 256, "one thread per output");

template <int F, int MODE>
void launch_downscale(const void* src, long long planes, int H, int W, void* dst, hipStream_t stream) {
  const long long in_elem = MODE == SRC_U8 ? 1 : MODE == SRC_F32 ? 4 : 8, out_elem = MODE == SRC_NIQE ? 8 : 4;
  const int Ho = H / F, Wo = W / F;
  for (long long p0 = 0; p0 < planes; p0 += 65535) {        // grid.z holds 65535 planes
    const long long np = planes - p0 < 65535 ? planes - p0 : 65535;
    hipLaunchKernelGGL((downscale_kernel<F, MODE>), dim3((unsigned)fcvsr::cdiv(Wo, kOX), (unsigned)fcvsr::cdiv(Ho, kOY), (unsigned)np),
                       dim3(256), 0, stream, (const void*)((const char*)src + p0 * H * W * in_elem), H, W,
                       (void*)((char*)dst + p0 * Ho * Wo * out_elem));
  }
}

__device__ inline double wave_sum(double v) {
  // xor butterfly: every lane ends with the same sum, formed in a fixed shape
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct BlockArgs {
  const double* m1;                      // (N, Hc, Wc) MSCN at scale 1
  const double* m2;                      // (N, Hc/2, Wc/2) MSCN at scale 2
  int Hc, Wc, nbw, nb;
  const double* tab;                     // (4, 9801): r_gam, sqrt(G(1/g) / G(3/g)), G(2/g) / G(1/g), g
  double* out;                           // (N, nb, 36)
};

__global__ __launch_bounds__(256) void niqe_block_kernel(BlockArgs a) {
  __shared__ double sums[4][30];
  __shared__ double best_v[4][5];
  __shared__ int best_i[4][5];
  const int b = blockIdx.x, s = blockIdx.y, n = blockIdx.z;
  const int bs = kBlock >> s, H = a.Hc >> s, W = a.Wc >> s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* base = (s ? a.m2 : a.m1) + (long long)n * H * W + (long long)(b / a.nbw) * bs * W + (b % a.nbw) * bs;

  // per distribution: count and sum of squares of the negatives, of the positives, sum |v|, sum v^2
  double acc[5][6];
#pragma unroll
  for (int d = 0; d < 5; ++d)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[d][k] = 0.0;
  for (int i = threadIdx.x; i < bs * bs; i += 256) {
    const int r = i / bs, c = i % bs;
    const int rm = r ? r - 1 : bs - 1, cm = c ? c - 1 : bs - 1, cp = c + 1 < bs ? c + 1 : 0;   // np.roll: circular in the block
    const double v = base[(long long)r * W + c];
    const double vals[5] = {v, v * base[(long long)r * W + cm], v * base[(long long)rm * W + c], v * base[(long long)rm * W + cm],
                            v * base[(long long)rm * W + cp]};
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const double x = vals[d], sq = x * x;
      if (x < 0) { acc[d][0] += 1.0; acc[d][1] += sq; }
      else if (x > 0) { acc[d][2] += 1.0; acc[d][3] += sq; }
      acc[d][4] += fabs(x);
      acc[d][5] += sq;
    }
  }
#pragma unroll
  for (int d = 0; d < 5; ++d)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double t = wave_sum(acc[d][k]);
      if (lane == 0) sums[wave][d * 6 + k] = t;
    }
  __syncthreads();

  // estimate_aggd_param up to the grid search's target, in every thread
  const double cnt = (double)(bs * bs);
  double left[5], right[5], target[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    double t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = ((sums[0][d * 6 + k] + sums[1][d * 6 + k]) + sums[2][d * 6 + k]) + sums[3][d * 6 + k];
    left[d] = sqrt(t[1] / t[0]);         // 0 / 0 = NaN for an empty side, as the mean of an empty slice
    right[d] = sqrt(t[3] / t[2]);
    const double gh = left[d] / right[d], g2 = gh * gh, ma = t[4] / cnt;
    const double rhat = (ma * ma) / (t[5] / cnt);
    target[d] = (rhat * (g2 * gh + 1.0) * (gh + 1.0)) / ((g2 + 1.0) * (g2 + 1.0));
  }

  // argmin over the grid of (r_gam - target)^2: first minimum; a NaN target never compares below, which leaves index 0
  double bv[5];
  int bi[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) { bv[d] = INFINITY; bi[d] = threadIdx.x; }
  for (int i = threadIdx.x; i < kGrid; i += 256) {
    const double rg = a.tab[i];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const double df = rg - target[d], d2 = df * df;
      if (d2 < bv[d]) { bv[d] = d2; bi[d] = i; }
    }
  }
#pragma unroll
  for (int d = 0; d < 5; ++d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv[d], o);
      const int oi = __shfl_xor(bi[d], o);
      if (ov < bv[d] || (ov == bv[d] && oi < bi[d])) { bv[d] = ov; bi[d] = oi; }
    }
    if (lane == 0) { best_v[wave][d] = bv[d]; best_i[wave][d] = bi[d]; }
  }
  __syncthreads();

  if (threadIdx.x < 5) {
    const int d = threadIdx.x;
    double v = best_v[0][d];
    int idx = best_i[0][d];
    for (int wv = 1; wv < 4; ++wv)
      if (best_v[wv][d] < v || (best_v[wv][d] == v && best_i[wv][d] < idx)) { v = best_v[wv][d]; idx = best_i[wv][d]; }
    const double beta = a.tab[kGrid + idx], mean = a.tab[2 * kGrid + idx], alpha = a.tab[3 * kGrid + idx];
    const double bl = left[d] * beta, br = right[d] * beta;
    double* o = a.out + ((long long)n * a.nb + b) * 36 + 18 * s;
    if (d == 0) {
      o[0] = alpha;
      o[1] = (bl + br) / 2;
    } else {
      o += 2 + 4 * (d - 1);
      o[0] = alpha;
      o[1] = (br - bl) * mean;
      o[2] = bl;
      o[3] = br;
    }
  }
}

struct NiqeGeometry {
  int Hc, Wc, nbh, nbw;
};

NiqeGeometry niqe_geometry(int H, int W, int crop) {
  NiqeGeometry g;
  g.nbh = H - 2 * crop > 0 ? (H - 2 * crop) / kBlock : 0;
  g.nbw = W - 2 * crop > 0 ? (W - 2 * crop) / kBlock : 0;
  g.Hc = g.nbh * kBlock;
  g.Wc = g.nbw * kBlock;
  return g;
}

}  // namespace

namespace fcvsr {
// the NIQE form of the down-scale for brisque.hip: f64 planes of integers in, f64(f32 result) * 255 out
void niqe_downscale2_f64(const double* src, long long planes, int H, int W, double* dst, hipStream_t stream) {
  launch_downscale<2, SRC_NIQE>(src, planes, H, W, dst, stream);
}
}  // namespace fcvsr

extern "C" long long fcvsr_niqe_scratch_bytes(int N, int H, int W, int crop_border) {
  if (N < 1 || H < 1 || W < 1 || crop_border < 0) return 0;
  const NiqeGeometry g = niqe_geometry(H, W, crop_border);
  const long long px = (long long)N * g.Hc * g.Wc;
  return (2 * px + 2 * (px / 4)) * (long long)sizeof(double);
}

extern "C" int fcvsr_niqe_features(const void* frames, const int64_t* host_strides, int quantise, int N, int C, int H, int W,
                                   int crop_border, int to_y, const double* host_window, const double* tables, double* out,
                                   void* scratch, long long scratch_bytes, void* stream) {
  FCVSR_CHECK_ARG(frames && tables && out && scratch, "null device pointer");
  FCVSR_CHECK_ARG(host_strides && host_window, "null host pointer");
  FCVSR_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "empty frames");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE || quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "bad quantise mode");
  FCVSR_CHECK_ARG((to_y == 0 && C == 1) || (to_y == 1 && C == 3), "one plane: C = 1, or C = 3 (RGB) with to_y");
  FCVSR_CHECK_ARG(crop_border >= 0, "negative crop_border");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE || ((uintptr_t)frames % 4) == 0, "f32 frames must be 4-byte aligned");
  const NiqeGeometry g = niqe_geometry(H, W, crop_border);
  FCVSR_CHECK_ARG((long long)g.nbh * g.nbw >= 2, "fewer than two 96x96 blocks after the crop");
  FCVSR_CHECK_ARG(N <= 65535 && g.Hc <= 65535 && (long long)g.nbh * g.nbw <= 0x7fffffff, "too many frames or rows for one call");
  FCVSR_CHECK_ARG(((uintptr_t)out % 8) == 0 && ((uintptr_t)scratch % 8) == 0 && ((uintptr_t)tables % 8) == 0,
                  "out / scratch / tables must be 8-byte aligned");
  FCVSR_CHECK_ARG(scratch_bytes >= fcvsr_niqe_scratch_bytes(N, H, W, crop_border), "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const long long px = (long long)N * g.Hc * g.Wc;
  double* plane1 = (double*)scratch;
  double* mscn1 = plane1 + px;
  double* plane2 = mscn1 + px;
  double* mscn2 = plane2 + px / 4;
  NiqeSrc s;
  s.p = frames;
  s.sn = host_strides[0]; s.sc = host_strides[1]; s.sy = host_strides[2]; s.sx = host_strides[3];
  s.quantise = quantise; s.to_y = to_y; s.crop = crop_border;
  Window49 w;
  for (int k = 0; k < 49; ++k) w.f[k] = host_window[k];
  hipLaunchKernelGGL(niqe_plane_kernel, dim3((unsigned)fcvsr::cdiv(g.Wc, 256), (unsigned)g.Hc, (unsigned)N), dim3(256), 0, st, s, g.Hc, g.Wc,
                     plane1);
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)fcvsr::cdiv(g.Wc, kMX), (unsigned)fcvsr::cdiv(g.Hc, kMY), (unsigned)N), dim3(256), 0, st,
                     (const double*)plane1, g.Hc, g.Wc, w, mscn1);
  launch_downscale<2, SRC_NIQE>(plane1, N, g.Hc, g.Wc, plane2, st);
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)fcvsr::cdiv(g.Wc / 2, kMX), (unsigned)fcvsr::cdiv(g.Hc / 2, kMY), (unsigned)N), dim3(256),
                     0, st, (const double*)plane2, g.Hc / 2, g.Wc / 2, w, mscn2);
  BlockArgs b;
  b.m1 = mscn1; b.m2 = mscn2;
  b.Hc = g.Hc; b.Wc = g.Wc; b.nbw = g.nbw; b.nb = g.nbh * g.nbw;
  b.tab = tables;
  b.out = out;
  hipLaunchKernelGGL(niqe_block_kernel, dim3((unsigned)b.nb, 2, (unsigned)N), dim3(256), 0, st, b);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_bicubic_downscale(const void* src, int src_dtype, long long planes, int H, int W, int factor, float* out,
                                       void* stream) {
  FCVSR_CHECK_ARG(src && out, "null device pointer");
  FCVSR_CHECK_ARG(src_dtype == FCVSR_U8 || src_dtype == FCVSR_F32, "src_dtype: FCVSR_U8 or FCVSR_F32");
  FCVSR_CHECK_ARG(factor == 2 || factor == 4, "factor: 2 or 4");
  FCVSR_CHECK_ARG(planes >= 1 && H >= factor && W >= factor && H % factor == 0 && W % factor == 0, "H and W: positive multiples of factor");
  FCVSR_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20), "plane too large");
  FCVSR_CHECK_ARG(((uintptr_t)out % 4) == 0 && (src_dtype == FCVSR_U8 || ((uintptr_t)src % 4) == 0), "f32 planes must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (factor == 2) {
    if (src_dtype == FCVSR_U8) launch_downscale<2, SRC_U8>(src, planes, H, W, out, st);
    else launch_downscale<2, SRC_F32>(src, planes, H, W, out, st);
  } else {
    if (src_dtype == FCVSR_U8) launch_downscale<4, SRC_U8>(src, planes, H, W, out, st);
    else launch_downscale<4, SRC_F32>(src, planes, H, W, out, st);
  }
  FCVSR_LAUNCH_CHECK();
  return 0;
}
