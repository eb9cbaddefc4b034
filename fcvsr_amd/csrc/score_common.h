// What the frame scores share on the device.  quality.hip (PSNR / SSIM) uses the frame sample and the YCbCr luma; niqe.hip and
// brisque.hip use the whole natural-scene-statistics front end as well: frame -> f64 plane of integers -> 7 x 7 MSCN, the wave sums
// and the pick that ends the 9801-entry first-minimum search.  Every reduction here has a fixed shape (xor butterflies inside a
// wave, then the four waves in order): no atomics, the same input gives the same bits.
#pragma once
#include "resize.h"
#include "u8.h"

namespace fcvsr {

constexpr int kGrid = 9801, kMY = 16, kMX = 64, kHalo = 3;   // the shape grid; the MSCN tile and its halo

// (N,C,H,W) frames with any strides (in elements): uint8 / uint16 samples with FCVSR_QUANT_NONE, else f32 quantised on the way in
struct FrameSrc {
  const void* p;
  long long sn, sc, sy, sx;
  int quantise, to_y, crop;
};

// One sample as the integer frame the harness would write: the stored sample (uint8 for PEAK 255, uint16 for 1023), or an f32
// quantised as u8.h's out rule.  T: double, or int where integer arithmetic follows.
template <int PEAK, class T = double>
__device__ inline T frame_sample(const FrameSrc& a, long long off) {
  if (a.quantise == FCVSR_QUANT_NONE) return (T)((const typename SampleOf<PEAK>::type*)a.p)[off];
  return (T)quantised<PEAK>(((const float*)a.p)[off], a.quantise);
}

// Y of YCbCr (metrics.py to_y_channel of the BGR-flipped frame): (24.966 B + 128.553 G + 65.481 R) / 255 + 16, in f64
__device__ inline double ycbcr_y(double r, double g, double b) {
  return (b / 255.0) * 24.966 + (g / 255.0) * 128.553 + (r / 255.0) * 65.481 + 16.0;
}

// The luma rules of plane_kernel: the sample type they work in and the integer luma of an RGB sample.
struct LumaYCbCr {                       // NIQE: ycbcr_y, then round half to even as the reference's niqe() does
  typedef double sample;
  __device__ static double of(double r, double g, double b) { return rint(ycbcr_y(r, g, b)); }
};
struct LumaYIQ {                         // BRISQUE: round_half_even((299 R + 587 G + 114 B) / 1000), in integers
  typedef int sample;
  __device__ static int of(int r, int g, int b) {
    const int s = 299 * r + 587 * g + 114 * b;
    const int q = s / 1000, m = s % 1000;
    return q + ((m > 500 || (m == 500 && (q & 1))) ? 1 : 0);
  }
};

// The scored plane as f64 integers: Hc x Wc samples from (crop, crop) of each frame; 8-bit samples, or the luma of RGB with to_y.
template <class LUMA>
__global__ __launch_bounds__(256) void plane_kernel(FrameSrc a, int Hc, int Wc, double* __restrict__ plane) {
  typedef typename LUMA::sample S;
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= Wc) return;
  const long long off = n * a.sn + (long long)(a.crop + y) * a.sy + (long long)(a.crop + x) * a.sx;
  S v;
  if (a.to_y) {
    const S r = frame_sample<kPeak8, S>(a, off), g = frame_sample<kPeak8, S>(a, off + a.sc), b = frame_sample<kPeak8, S>(a, off + 2 * a.sc);
    v = LUMA::of(r, g, b);
  } else {
    v = frame_sample<kPeak8, S>(a, off);
  }
  plane[((long long)n * Hc + y) * Wc + x] = (double)v;
}

struct Window49 {
  double f[49];                          // the correlation taps (NIQE: the model's window flipped in both axes)
};

// mscn = (img - mu) / (sigma + 1): mu and E[x^2] from the 7 x 7 window, 49 taps from a haloed LDS tile, accumulated from 0 in
// row-major tap order as the contracts do.  ZERO_BORDER: the plane is zero-padded (BRISQUE), else its border is replicated (NIQE).
// EPS_UNDER_ROOT: sigma = sqrt(|E[x^2] - mu^2| + 2^-23) (BRISQUE), else sqrt(|E[x^2] - mu^2|) (NIQE).
template <bool ZERO_BORDER, bool EPS_UNDER_ROOT>
__global__ __launch_bounds__(256) void mscn_kernel(const double* __restrict__ img, int H, int W, Window49 w, double* __restrict__ out) {
  __shared__ double s[kMY + 2 * kHalo][kMX + 2 * kHalo];
  const int y0 = blockIdx.y * kMY, x0 = blockIdx.x * kMX;
  const double* p = img + (long long)blockIdx.z * H * W;
  double* o = out + (long long)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < (kMY + 2 * kHalo) * (kMX + 2 * kHalo); i += 256) {
    const int r = i / (kMX + 2 * kHalo), q = i % (kMX + 2 * kHalo);
    if constexpr (ZERO_BORDER) {
      const int yy = y0 + r - kHalo, xx = x0 + q - kHalo;
      s[r][q] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? p[(long long)yy * W + xx] : 0.0;
    } else {
      const int yy = min(max(y0 + r - kHalo, 0), H - 1), xx = min(max(x0 + q - kHalo, 0), W - 1);
      s[r][q] = p[(long long)yy * W + xx];
    }
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
    double var = fabs(e2 - mu * mu);
    if constexpr (EPS_UNDER_ROOT) var = var + 0x1p-23;
    o[(long long)(y0 + r) * W + x0 + q] = (s[r + kHalo][q + kHalo] - mu) / (sqrt(var) + 1.0);
  }
}

template <bool ZERO_BORDER, bool EPS_UNDER_ROOT>
inline void launch_mscn(const double* img, int N, int H, int W, const Window49& w, double* out, hipStream_t stream) {
  hipLaunchKernelGGL((mscn_kernel<ZERO_BORDER, EPS_UNDER_ROOT>), dim3((unsigned)cdiv(W, kMX), (unsigned)cdiv(H, kMY), (unsigned)N), dim3(256),
                     0, stream, img, H, W, w, out);
}

// xor butterfly: every lane ends with the same sum, formed in a fixed shape
template <class T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The end of the five first-minimum searches of a 256-thread workgroup.  Each thread brings the least value bv[d] it met scanning
// the grid and its index bi[d] (its first such index: it scanned upwards with <); thread d < 5 gets the index of search d, the
// others 0.  Lower value, then lower index: across the wave by xor butterfly, then the four waves in order.  A NaN never compares
// below, so a search that met nothing keeps the least index any thread started from.  All threads must call (it has a barrier).
__device__ inline int first_min_pick(double (&bv)[5], int (&bi)[5]) {
  __shared__ double best_v[4][5];
  __shared__ int best_i[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
  int idx = 0;
  if (threadIdx.x < 5) {
    const int d = threadIdx.x;
    double v = best_v[0][d];
    idx = best_i[0][d];
    for (int wv = 1; wv < 4; ++wv)
      if (best_v[wv][d] < v || (best_v[wv][d] == v && best_i[wv][d] < idx)) { v = best_v[wv][d]; idx = best_i[wv][d]; }
  }
  return idx;
}

}  // namespace fcvsr
