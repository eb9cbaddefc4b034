// Frame quality metrics on the device: per-frame squared-error sums (PSNR) and SSIM-map sums, f64, for N SR / HR frame pairs.
// Replaces the per-frame CPU scoring of the reference's evaluation (CVSR_train/metric/psnr_ssim.py:278-398 calculate_psnr /
// _ssim / calculate_ssim, applied per frame by cal_psnr_ssim :447-485); the contract is fcvsr_amd/harness/metrics.py.
//
// Per plane (a frame's channel, or its Y channel): the PSNR region is the image with `crop` pixels removed on each side (Hc x Wc);
// the SSIM map is the 'valid' 11x11 Gaussian correlation over it (Hm x Wm = (Hc - 10) x (Wc - 10)).  One workgroup per
// (plane, 16 x 64 tile of the map): the haloed 26 x 74 window of both images goes to LDS as f64 (quantised / Y-converted on the
// way), a vertical then a horizontal 11-tap pass build mu1, mu2 and the three second moments in the order of _filter_valid
// (so the map values are those of the CPU function), and the tile's map sum and squared-error sum go to a partial slot.  The
// squared errors cover PSNR-region pixels: a tile owns its 16 x 64 map rectangle, and the last tile of a row / column also the
// 10 extra rows / columns its halo already holds, so every PSNR pixel is counted exactly once.  A second launch adds each
// frame's partials in a fixed order (no atomics: bit-reproducible).
// U16 (fcvsr_frame_metrics_u16): the frames hold 10-bit samples in uint16; f32 SR values are quantised with the 1023 scale and the
// SSIM constants come from the caller's peak (1023, or HM's 1020); there is no Y conversion.
#include "score_common.h"

using namespace fcvsr;

namespace {

constexpr int kTY = 16, kTX = 64, kWin = 11, kLY = kTY + kWin - 1, kLX = kTX + kWin - 1;

struct QualityArgs {
  FrameSrc sr;
  const unsigned char* hr;
  long long h_sn, h_sc, h_sy, h_sx;
  int planes_per_frame, Hc, Wc, Hm, Wm, tiles_x, tiles;
  double peak;                           // U16: the peak of the SSIM constants
  double g[kWin];
  double* part;                          // [plane][tile][2] = {squared-error sum, SSIM-map sum}
};

// SR value of one sample as the uint8 frame harness/infer.py would produce: clamp(v, 0, 1) * 255.0f (f32 multiply), then
// truncation toward zero (tensor.to(torch.uint8)) or round-half-to-even (torch.round); uint8 input is used as it is.
// (U16: uint16 samples, scale 1023.0f)
template <bool U16>
__device__ inline double sr_value(const QualityArgs& a, long long off) {
  return frame_sample<U16 ? kPeak10 : kPeak8>(a.sr, off);
}

__device__ inline double block_sum(double v, double* sm) {
  // fixed-shape tree over the 256 threads: the same input gives the same bits
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  const double t = sm[0];
  __syncthreads();
  return t;
}

template <bool U16>
__global__ __launch_bounds__(256) void quality_tile_kernel(QualityArgs a) {
  __shared__ double sx[kLY][kLX], sy[kLY][kLX];    // SR, HR window (zero past the crop edge)
  __shared__ double vs[5][kTY][kLX];               // vertical pass: x, y, x*x, y*y, x*y
  const int tile = blockIdx.x, plane = blockIdx.y;
  const int n = plane / a.planes_per_frame, c = plane % a.planes_per_frame;
  const int ty = tile / a.tiles_x, tx = tile % a.tiles_x;
  const int my0 = ty * kTY, mx0 = tx * kTX;        // map origin of the tile = cropped-image origin of its window
  const int ly = min(kLY, a.Hc - my0), lx = min(kLX, a.Wc - mx0);

  for (int i = threadIdx.x; i < kLY * kLX; i += 256) {
    const int r = i / kLX, q = i % kLX;
    double xv = 0.0, yv = 0.0;
    if (r < ly && q < lx) {
      const long long iy = a.sr.crop + my0 + r, ix = a.sr.crop + mx0 + q;
      const long long so = n * a.sr.sn + iy * a.sr.sy + ix * a.sr.sx, ho = n * a.h_sn + iy * a.h_sy + ix * a.h_sx;
      if constexpr (U16) {
        xv = sr_value<true>(a, so + c * a.sr.sc);
        yv = (double)((const unsigned short*)a.hr)[ho + c * a.h_sc];
      } else if (a.sr.to_y) {
        xv = ycbcr_y(sr_value<false>(a, so), sr_value<false>(a, so + a.sr.sc), sr_value<false>(a, so + 2 * a.sr.sc));
        yv = ycbcr_y((double)a.hr[ho], (double)a.hr[ho + a.h_sc], (double)a.hr[ho + 2 * a.h_sc]);
      } else {
        xv = sr_value<false>(a, so + c * a.sr.sc);
        yv = (double)a.hr[ho + c * a.h_sc];
      }
    }
    sx[r][q] = xv;
    sy[r][q] = yv;
  }
  __syncthreads();

  // squared errors of the PSNR pixels this tile owns
  const int oy = ty == (a.tiles / a.tiles_x) - 1 ? ly : kTY, ox = tx == a.tiles_x - 1 ? lx : kTX;
  double sse = 0.0;
  for (int i = threadIdx.x; i < oy * ox; i += 256) {
    const int r = i / ox, q = i % ox;
    const double d = sx[r][q] - sy[r][q];
    sse += d * d;
  }

  // vertical 11-tap pass (rows of _filter_valid: accumulated from 0 in tap order, products formed before weighting)
  for (int i = threadIdx.x; i < kTY * kLX; i += 256) {
    const int r = i / kLX, q = i % kLX;
    double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double x = sx[r + k][q], y = sy[r + k][q];
      m1 += a.g[k] * x;
      m2 += a.g[k] * y;
      e11 += a.g[k] * (x * x);
      e22 += a.g[k] * (y * y);
      e12 += a.g[k] * (x * y);
    }
    vs[0][r][q] = m1; vs[1][r][q] = m2; vs[2][r][q] = e11; vs[3][r][q] = e22; vs[4][r][q] = e12;
  }
  __syncthreads();

  // horizontal pass and the SSIM map of _ssim_plane, summed over this tile's valid map pixels
  const double peak = U16 ? a.peak : 255.0;
  const double k1 = 0.01 * peak, k2 = 0.03 * peak, c1 = k1 * k1, c2 = k2 * k2;
  const int ro = min(kTY, a.Hm - my0), co = min(kTX, a.Wm - mx0);
  double ssum = 0.0;
  for (int i = threadIdx.x; i < ro * co; i += 256) {
    const int r = i / co, q = i % co;
    double mu1 = 0.0, mu2 = 0.0, f11 = 0.0, f22 = 0.0, f12 = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      mu1 += a.g[k] * vs[0][r][q + k];
      mu2 += a.g[k] * vs[1][r][q + k];
      f11 += a.g[k] * vs[2][r][q + k];
      f22 += a.g[k] * vs[3][r][q + k];
      f12 += a.g[k] * vs[4][r][q + k];
    }
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = f11 - mu1_sq, s2 = f22 - mu2_sq, s12 = f12 - mu12;
    ssum += ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2));
  }

  double* red = &sx[0][0];                         // the windows are no longer read after the vertical pass
  const double t_sse = block_sum(sse, red), t_ssim = block_sum(ssum, red);
  if (threadIdx.x == 0) {
    double* p = a.part + ((long long)plane * a.tiles + tile) * 2;
    p[0] = t_sse;
    p[1] = t_ssim;
  }
}

// out[n] = {sum of frame n's squared-error partials, sum of its SSIM partials}: strided per-thread sums, then a fixed tree
__global__ __launch_bounds__(256) void quality_finish_kernel(const double* __restrict__ part, long long per_frame, double* __restrict__ out) {
  __shared__ double sm[256];
  const double* p = part + (long long)blockIdx.x * per_frame * 2;
  double s0 = 0.0, s1 = 0.0;
  for (long long i = threadIdx.x; i < per_frame; i += 256) {
    s0 += p[2 * i];
    s1 += p[2 * i + 1];
  }
  const double t0 = block_sum(s0, sm), t1 = block_sum(s1, sm);
  if (threadIdx.x == 0) {
    out[2 * (long long)blockIdx.x] = t0;
    out[2 * (long long)blockIdx.x + 1] = t1;
  }
}

struct Geometry {
  int Hc, Wc, Hm, Wm, tiles_x, tiles_y, P;
};

Geometry geometry(int C, int H, int W, int crop, int to_y) {
  Geometry g;
  g.Hc = H - 2 * crop;
  g.Wc = W - 2 * crop;
  g.Hm = g.Hc - (kWin - 1);
  g.Wm = g.Wc - (kWin - 1);
  g.tiles_x = g.Wm > 0 ? (g.Wm + kTX - 1) / kTX : 0;
  g.tiles_y = g.Hm > 0 ? (g.Hm + kTY - 1) / kTY : 0;
  g.P = to_y ? 1 : C;
  return g;
}

}  // namespace

extern "C" long long fcvsr_frame_metrics_scratch_bytes(int N, int C, int H, int W, int crop_border, int to_y) {
  if (N < 1 || C < 1 || crop_border < 0) return 0;
  const Geometry g = geometry(C, H, W, crop_border, to_y);
  return (long long)N * g.P * g.tiles_x * g.tiles_y * 2 * (long long)sizeof(double);
}

template <bool U16>
static int frame_metrics_launch(const void* sr, const int64_t* host_sr_strides, int quantise, const void* hr, const int64_t* host_hr_strides,
                         int N, int C, int H, int W, int crop_border, int to_y, const double* host_window, double peak, double* out,
                         void* scratch, long long scratch_bytes, void* stream) {
  FCVSR_CHECK_ARG(sr && hr && out && scratch, "null device pointer");
  FCVSR_CHECK_ARG(host_sr_strides && host_hr_strides && host_window, "null host pointer");
  FCVSR_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "empty frames");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE || quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "bad quantise mode");
  FCVSR_CHECK_ARG(to_y == 0 || (to_y == 1 && C == 3), "Y conversion needs 3 channels (RGB)");
  FCVSR_CHECK_ARG(!(U16 && to_y), "Y conversion is not defined for 10-bit frames");
  FCVSR_CHECK_ARG(!U16 || (peak > 0.0 && peak <= 65535.0), "peak: positive");
  FCVSR_CHECK_ARG(!U16 || (((uintptr_t)hr % 2) == 0 && (quantise != FCVSR_QUANT_NONE || ((uintptr_t)sr % 2) == 0)),
                  "uint16 frames must be 2-byte aligned");
  FCVSR_CHECK_ARG(crop_border >= 0, "negative crop_border");
  const Geometry g = geometry(C, H, W, crop_border, to_y);
  FCVSR_CHECK_ARG(g.Hm >= 1 && g.Wm >= 1, "frame too small for crop_border + the 11x11 SSIM window");
  FCVSR_CHECK_ARG((long long)N * g.P <= 65535, "too many planes for one call (N * channels <= 65535)");
  FCVSR_CHECK_ARG(((uintptr_t)out % 8) == 0 && ((uintptr_t)scratch % 8) == 0, "out / scratch must be 8-byte aligned");
  FCVSR_CHECK_ARG(scratch_bytes >= fcvsr_frame_metrics_scratch_bytes(N, C, H, W, crop_border, to_y), "scratch too small");
  QualityArgs a;
  a.sr.p = sr;
  a.sr.sn = host_sr_strides[0]; a.sr.sc = host_sr_strides[1]; a.sr.sy = host_sr_strides[2]; a.sr.sx = host_sr_strides[3];
  a.sr.quantise = quantise; a.sr.to_y = to_y; a.sr.crop = crop_border;
  a.hr = (const unsigned char*)hr;
  a.h_sn = host_hr_strides[0]; a.h_sc = host_hr_strides[1]; a.h_sy = host_hr_strides[2]; a.h_sx = host_hr_strides[3];
  a.planes_per_frame = g.P;
  a.Hc = g.Hc; a.Wc = g.Wc; a.Hm = g.Hm; a.Wm = g.Wm;
  a.tiles_x = g.tiles_x;
  a.tiles = g.tiles_x * g.tiles_y;
  a.peak = peak;
  for (int k = 0; k < kWin; ++k) a.g[k] = host_window[k];
  a.part = (double*)scratch;
  hipLaunchKernelGGL(quality_tile_kernel<U16>, dim3((unsigned)a.tiles, (unsigned)(N * g.P)), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(quality_finish_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const double*)scratch,
                     (long long)g.P * a.tiles, out);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_frame_metrics(const void* sr, const int64_t* host_sr_strides, int quantise, const uint8_t* hr,
                                   const int64_t* host_hr_strides, int N, int C, int H, int W, int crop_border, int to_y,
                                   const double* host_window, double* out, void* scratch, long long scratch_bytes, void* stream) {
  return frame_metrics_launch<false>(sr, host_sr_strides, quantise, hr, host_hr_strides, N, C, H, W, crop_border, to_y, host_window,
                                     255.0, out, scratch, scratch_bytes, stream);
}

extern "C" int fcvsr_frame_metrics_u16(const void* sr, const int64_t* host_sr_strides, int quantise, const uint16_t* hr,
                                       const int64_t* host_hr_strides, int N, int C, int H, int W, int crop_border, int to_y,
                                       const double* host_window, double peak, double* out, void* scratch, long long scratch_bytes,
                                       void* stream) {
  return frame_metrics_launch<true>(sr, host_sr_strides, quantise, hr, host_hr_strides, N, C, H, W, crop_border, to_y, host_window,
                                    peak, out, scratch, scratch_bytes, stream);
}
