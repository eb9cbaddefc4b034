// BRISQUE features on the device: the 36 whole-plane GGD / AGGD statistics of the reference's second no-reference score
// (CVSR_train/metric/brisque.py natural_scene_statistics / estimate_ggd_param / estimate_aggd_param / normalize_img_with_guass, used
// by CVSR_train/metric/cal_VideoLQ.py); the contract is fcvsr_amd/harness/brisque.py.  The range scaling and the RBF regressor stay
// on the host.
//
// fcvsr_brisque_features, eight launches on one stream, no host sync:
//   1. plane      the whole frame as f64 integers: uint8 samples, or f32 samples quantised as the frame metrics do, or the integer
//                 YIQ luma of RGB (score_common.h plane_kernel, crop 0);
//   2. mscn       mu and E[x^2] from the 7 x 7 window over a ZERO-padded plane, sigma = sqrt(|E[x^2] - mu^2| + 2^-23),
//                 mscn = (img - mu) / (sigma + 1) (score_common.h mscn_kernel);
//   3. stats      one pass over the MSCN plane: a workgroup owns a fixed 32 x 64 tile, reads it with the rows above and below and
//                 the column to the left, their coordinates wrapped modulo H and W (the four products are circular over the whole
//                 plane), and forms 22 sums (x^2, |x|; per product the counts and squared sums of the negatives and of the
//                 positives and sum |p|), reduced in a fixed shape (xor butterflies inside a wave, then the four waves in order)
//                 into one row of partials per tile: no atomics, the same input gives the same bits;
//   4. finish     one workgroup per frame: the tile partials (staged through LDS 128 tiles at a time) added in tile order, the
//                 five 9801-entry first-minimum searches (index 0 for a NaN target) and the 18 features of the scale;
//   5. downscale  the 2x down-scale of plane / 255, times 255 (resize.hip), then 2, 3 and 4 on the half-size plane.
// The planes travel through HBM as f64.  LDS tiles are rows of f64 read by 32 consecutive lanes at consecutive addresses: a
// ds_read_b64 of half a wave then covers the 64 dword banks once, whatever the row pitch.
#include "score_common.h"

using namespace fcvsr;

namespace {

constexpr int kSY = 32, kSX = 64, kDbl = 14, kCnt = 8, kChunk = 128;

// Partials of one tile.  dsum: x^2, |x|, then per product (p^2 where p < 0, p^2 where p > 0, |p|); cnt: per product (p < 0, p > 0).
__global__ __launch_bounds__(256) void brisque_stats_kernel(const double* __restrict__ mscn, int H, int W, int tiles,
                                                            double* __restrict__ dsum, long long* __restrict__ cnt) {
  __shared__ double s[kSY + 2][kSX + 1];               // rows y0-1 .. y0+kSY, columns x0-1 .. x0+kSX-1
  __shared__ double wd[4][kDbl];
  __shared__ int wc[4][kCnt];
  const int y0 = blockIdx.y * kSY, x0 = blockIdx.x * kSX, n = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* p = mscn + (long long)n * H * W;
  for (int i = threadIdx.x; i < (kSY + 2) * (kSX + 1); i += 256) {
    const int r = i / (kSX + 1), q = i % (kSX + 1);
    // np.roll over the whole plane: coordinates wrapped modulo H and W (a tile past the last row / column wraps to valid samples
    // that no sample of the plane reads)
    const int yy = (y0 + r - 1 + H) % H, xx = (x0 + q - 1 + W) % W;
    s[r][q] = p[(long long)yy * W + xx];
  }
  __syncthreads();
  double ad[kDbl];
  int ac[kCnt];
#pragma unroll
  for (int k = 0; k < kDbl; ++k) ad[k] = 0.0;
#pragma unroll
  for (int k = 0; k < kCnt; ++k) ac[k] = 0;
  for (int i = threadIdx.x; i < kSY * kSX; i += 256) {
    const int r = i / kSX, q = i % kSX;
    if (y0 + r >= H || x0 + q >= W) continue;
    const double v = s[r + 1][q + 1];
    // roll by (0,1), (1,0), (1,1), (-1,1): the neighbours to the left, above, above left and below left
    const double prod[4] = {v * s[r + 1][q], v * s[r][q + 1], v * s[r][q], v * s[r + 2][q]};
    ad[0] += v * v;
    ad[1] += fabs(v);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const double x = prod[d], sq = x * x;
      if (x < 0) { ac[2 * d] += 1; ad[2 + 3 * d] += sq; }
      else if (x > 0) { ac[2 * d + 1] += 1; ad[3 + 3 * d] += sq; }
      ad[4 + 3 * d] += fabs(x);
    }
  }
#pragma unroll
  for (int k = 0; k < kDbl; ++k) {
    const double t = wave_sum(ad[k]);
    if (lane == 0) wd[wave][k] = t;
  }
#pragma unroll
  for (int k = 0; k < kCnt; ++k) {
    const int t = wave_sum(ac[k]);
    if (lane == 0) wc[wave][k] = t;
  }
  __syncthreads();
  const long long tile = (long long)n * tiles + (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x < kDbl) {
    const int k = threadIdx.x;
    dsum[tile * kDbl + k] = ((wd[0][k] + wd[1][k]) + wd[2][k]) + wd[3][k];
  } else if (threadIdx.x < kDbl + kCnt) {
    const int k = threadIdx.x - kDbl;
    cnt[tile * kCnt + k] = (long long)(((wc[0][k] + wc[1][k]) + wc[2][k]) + wc[3][k]);
  }
}

// One workgroup per frame: the 18 features of one scale from the tile partials.
__global__ __launch_bounds__(256) void brisque_finish_kernel(const double* __restrict__ dsum, const long long* __restrict__ cnt, int tiles,
                                                             int H, int W, const double* __restrict__ tab, double* __restrict__ out) {
  __shared__ double sd[kDbl];
  __shared__ long long sc[kCnt];
  __shared__ double stage_d[kChunk * kDbl];
  __shared__ long long stage_c[kChunk * kCnt];
  const int n = blockIdx.x;
  // the partials of kChunk tiles at a time come into LDS with coalesced loads; one thread per sum then adds them in tile order
  const double* pd = dsum + (long long)n * tiles * kDbl;
  const long long* pc = cnt + (long long)n * tiles * kCnt;
  double td = 0.0;
  long long tc = 0;
  for (int t0 = 0; t0 < tiles; t0 += kChunk) {
    const int nt = min(kChunk, tiles - t0);
    for (int i = threadIdx.x; i < nt * kDbl; i += 256) stage_d[i] = pd[(long long)t0 * kDbl + i];
    for (int i = threadIdx.x; i < nt * kCnt; i += 256) stage_c[i] = pc[(long long)t0 * kCnt + i];
    __syncthreads();
    if (threadIdx.x < kDbl) {
#pragma unroll 8
      for (int i = 0; i < nt; ++i) td += stage_d[i * kDbl + threadIdx.x];
    } else if (threadIdx.x < kDbl + kCnt) {
#pragma unroll 8
      for (int i = 0; i < nt; ++i) tc += stage_c[i * kCnt + (threadIdx.x - kDbl)];
    }
    __syncthreads();
  }
  if (threadIdx.x < kDbl) sd[threadIdx.x] = td;
  else if (threadIdx.x < kDbl + kCnt) sc[threadIdx.x - kDbl] = tc;
  __syncthreads();

  // the five grid-search targets, in every thread: rho of the GGD fit, rhatnorm of the four AGGD fits
  const double px = (double)H * (double)W;
  double left[5], right[5], target[5];
  const double sigma_sq = sd[0] / px, e = sd[1] / px;
  left[0] = right[0] = 0.0;
  target[0] = sigma_sq / (e * e);
#pragma unroll
  for (int d = 1; d < 5; ++d) {
    const double sq_l = sd[2 + 3 * (d - 1)], sq_r = sd[3 + 3 * (d - 1)], ma = sd[4 + 3 * (d - 1)] / px;
    left[d] = sqrt(sq_l / (double)sc[2 * (d - 1)]);      // 0 / 0 = NaN for an empty side
    right[d] = sqrt(sq_r / (double)sc[2 * (d - 1) + 1]);
    const double gh = left[d] / right[d], g2 = gh * gh;
    const double rhat = (ma * ma) / ((sq_l + sq_r) / px);
    target[d] = (rhat * (g2 * gh + 1.0) * (gh + 1.0)) / ((g2 + 1.0) * (g2 + 1.0));
  }

  // argmin over the grid of |r - target|: first minimum; a NaN target never compares below, which leaves index 0
  double bv[5];
  int bi[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) { bv[d] = INFINITY; bi[d] = threadIdx.x; }
#pragma unroll 4
  for (int i = threadIdx.x; i < kGrid; i += 256) {
    const double r_ggd = tab[i], r_aggd = tab[kGrid + i];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const double df = fabs((d == 0 ? r_ggd : r_aggd) - target[d]);
      if (df < bv[d]) { bv[d] = df; bi[d] = i; }
    }
  }
  const int idx = first_min_pick(bv, bi);

  if (threadIdx.x < 5) {
    const int d = threadIdx.x;
    const double alpha = tab[3 * kGrid + idx];
    double* o = out + (long long)n * 36;
    if (d == 0) {
      o[0] = alpha;
      o[1] = sigma_sq;
    } else {
      o += 2 + 4 * (d - 1);
      o[0] = alpha;
      o[1] = (right[d] - left[d]) * tab[2 * kGrid + idx];
      o[2] = left[d] * left[d];
      o[3] = right[d] * right[d];
    }
  }
}

long long tiles_of(int H, int W) { return (long long)cdiv(H, kSY) * cdiv(W, kSX); }

}  // namespace

extern "C" long long fcvsr_brisque_scratch_bytes(int N, int H, int W) {
  if (N < 1 || H < 2 || W < 2) return 0;
  const long long px = (long long)N * H * W, px2 = (long long)N * (H / 2) * (W / 2);
  // plane, MSCN (both scales in turn), half-size plane, tile partials (both scales in turn)
  return (2 * px + px2 + (long long)N * tiles_of(H, W) * (kDbl + kCnt)) * (long long)sizeof(double);
}

extern "C" int fcvsr_brisque_features(const void* frames, const int64_t* host_strides, int quantise, int N, int C, int H, int W,
                                      int to_y, const double* host_window, const double* tables, void* scratch,
                                      long long scratch_bytes, double* out, void* stream) {
  FCVSR_CHECK_ARG(frames && tables && out && scratch, "null device pointer");
  FCVSR_CHECK_ARG(host_strides && host_window, "null host pointer");
  FCVSR_CHECK_ARG(N >= 1, "empty frames");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE || quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "bad quantise mode");
  FCVSR_CHECK_ARG((to_y == 0 && C == 1) || (to_y == 1 && C == 3), "one plane: C = 1, or C = 3 (RGB) with to_y");
  FCVSR_CHECK_ARG(H >= 16 && W >= 16 && H % 2 == 0 && W % 2 == 0, "H and W: even and at least 16");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE || ((uintptr_t)frames % 4) == 0, "f32 frames must be 4-byte aligned");
  FCVSR_CHECK_ARG(N <= 65535 && H <= 65535 && W <= (1 << 20), "too many frames, rows or columns for one call");
  FCVSR_CHECK_ARG(((uintptr_t)out % 8) == 0 && ((uintptr_t)scratch % 8) == 0 && ((uintptr_t)tables % 8) == 0,
                  "out / scratch / tables must be 8-byte aligned");
  FCVSR_CHECK_ARG(scratch_bytes >= fcvsr_brisque_scratch_bytes(N, H, W), "scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const long long px = (long long)N * H * W, px2 = (long long)N * (H / 2) * (W / 2);
  double* plane1 = (double*)scratch;
  double* mscn = plane1 + px;
  double* plane2 = mscn + px;
  double* dsum = plane2 + px2;
  long long* cnt = (long long*)(dsum + (long long)N * tiles_of(H, W) * kDbl);
  FrameSrc s;
  s.p = frames;
  s.sn = host_strides[0]; s.sc = host_strides[1]; s.sy = host_strides[2]; s.sx = host_strides[3];
  s.quantise = quantise; s.to_y = to_y; s.crop = 0;
  Window49 w;
  for (int k = 0; k < 49; ++k) w.f[k] = host_window[k];
  hipLaunchKernelGGL(plane_kernel<LumaYIQ>, dim3((unsigned)cdiv(W, 256), (unsigned)H, (unsigned)N), dim3(256), 0, st, s, H, W, plane1);
  for (int scale = 0; scale < 2; ++scale) {
    const int h = H >> scale, wd = W >> scale;
    const double* plane = scale ? plane2 : plane1;
    const int tiles = (int)tiles_of(h, wd);
    if (scale) downscale2_f64(plane1, N, H, W, plane2, st);
    launch_mscn<true, true>(plane, N, h, wd, w, mscn, st);
    hipLaunchKernelGGL(brisque_stats_kernel, dim3((unsigned)cdiv(wd, kSX), (unsigned)cdiv(h, kSY), (unsigned)N), dim3(256), 0, st,
                       (const double*)mscn, h, wd, tiles, dsum, cnt);
    hipLaunchKernelGGL(brisque_finish_kernel, dim3((unsigned)N), dim3(256), 0, st, (const double*)dsum, (const long long*)cnt, tiles, h, wd,
                       tables, out + 18 * scale);
  }
  FCVSR_LAUNCH_CHECK();
  return 0;
}
