// Focal frequency loss (the FFL of the reference's Charbonnier_FFL_Loss, CVSR_train/opt/deep_learning.py:192-220) around the library's own
// transforms.  The loss is a function of the spectrum of pred - target only, so ONE real transform of the difference replaces the two
// complex transforms of the images, and Hermitian symmetry leaves half of it to visit (column weights cw: 1 on the self-conjugate
// columns kx = 0 and kx = w / 2, 2 elsewhere).  Per plane, with U = rfft2(d) unnormalised, N = h w and s = |U|^2:
//     wgt = (s / max s)^(alpha / 2)                      (= u^alpha / max u^alpha with u = |U| / sqrt(N); 0 where max s = 0)
//     loss = loss_weight / (P N) * sum cw * wgt * s / N
//     d loss / d d = 2 loss_weight / (P N) * c2r(wgt * U)                   (wgt detached; c2r = fcvsr_irfft2 with its 1 / N)
// The planes (batch x patch x channel) are the CHANNELS of one NHWC image (1, h, w, P), the layout the FFT kernels spread over lanes.
//
//   fcvsr_ffl_diff    NCHW pred / target planes (patch crops of them) -> NHWC d, zero planes beyond P
//   fcvsr_ffl_weight  max s per plane (two stages; max is order-independent), then one pass that writes wgt * U over U and sums
//                     cw * wgt * s in the fixed order of reduce.h (tile partials, one final reduce per plane), then the planes in order
//   fcvsr_ffl_grad    c2r(wgt * U) NHWC -> NCHW gradient planes, scaled by 2 loss_weight / (P N) and the upstream gradient (device scalar)
// No float atomics, no host read-back: the loss is a device scalar.
#include "reduce.h"

namespace fcvsr {
namespace {

constexpr int kFflThreads = 256;

// Offset of plane p's element (0, 0) in a contiguous (B, C, H, W) tensor.  p = (b * f * f + i * f + j) * C + c: patch (i, j) of image b,
// channel c  (the stack order of the restatement, fcvsr_amd/train/loss.py ffl_reference).
__device__ __forceinline__ long long plane_base(int p, int C, int H, int W, int f, int h, int w) {
  const int c = p % C, q = p / C;
  const int j = q % f, i = (q / f) % f, b = q / (f * f);
  return (((long long)b * C + c) * H + (long long)i * h) * W + (long long)j * w;
}

// One thread per pixel of the patch grid (x fastest: the NCHW reads of a plane are coalesced), channel groups of four on the NHWC side.
template <bool VEC>
__global__ __launch_bounds__(kFflThreads) void ffl_diff_kernel(const float* __restrict__ pred, const float* __restrict__ target, int C,
                                                               int H, int W, int f, int h, int w, int P, int Pp,
                                                               float* __restrict__ d) {
  const long long pix = (long long)blockIdx.x * kFflThreads + threadIdx.x;
  if (pix >= (long long)h * w) return;
  const int y = (int)(pix / w), x = (int)(pix % w);
  const long long in = (long long)y * W + x;
  float* o = d + pix * Pp;
  for (int p0 = 0; p0 < Pp; p0 += 4) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = p0 + k;
      v[k] = 0.f;
      if (p < P) {
        const long long a = plane_base(p, C, H, W, f, h, w) + in;
        v[k] = pred[a] - target[a];
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(o + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p0 + k < Pp) o[p0 + k] = v[k];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kFflThreads) void ffl_grad_kernel(const float* __restrict__ r, const float* __restrict__ g_up, float scale,
                                                               int C, int H, int W, int f, int h, int w, int P, int Pp,
                                                               float* __restrict__ gp, float* __restrict__ gt) {
  const long long pix = (long long)blockIdx.x * kFflThreads + threadIdx.x;
  if (pix >= (long long)h * w) return;
  const float s = g_up[0] * scale;
  const int y = (int)(pix / w), x = (int)(pix % w);
  const long long out = (long long)y * W + x;
  const float* q = r + pix * Pp;
  for (int p0 = 0; p0 < P; p0 += 4) {
    float v[4];
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(q + p0);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = p0 + k < P ? q[p0 + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = p0 + k;
      if (p < P) {
        const long long a = plane_base(p, C, H, W, f, h, w) + out;
        const float g = s * v[k];
        if (gp) gp[a] = g;
        if (gt) gt[a] = -g;
      }
    }
  }
}

// Planes are handled in chunks of CH <= 256 (chunk = blockIdx.y, the "batch" index of the reduce.h kernels); thread (sub, c) as there.
struct SpecRef {
  float* spec;
  long long ps;
  int im_off, re_off, P, CH;
};

// pmax[chunk][blk][c] = max of s over the block's kRedPix pixels.  fmaxf drops NaNs: a plane of NaNs keeps 0, and the weight pass
// then multiplies its NaNs by weight 0, which is still NaN.
__global__ __launch_bounds__(kRedThreads) void ffl_max_stage1(SpecRef u, long long npix, float* __restrict__ pmax) {
  __shared__ float sm[kRedThreads];
  const int chunk = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int R = kRedThreads / u.CH;
  const int sub = threadIdx.x / u.CH, c = threadIdx.x % u.CH;
  const int plane = chunk * u.CH + c;
  float m = 0.f;
  if (sub < R && plane < u.P) {
    const long long p0 = (long long)blk * kRedPix;
    const long long p1 = (p0 + kRedPix < npix) ? p0 + kRedPix : npix;
    // (the loop vectoriser paired two iterations into packed-FP32 multiplies, which no code object of the library may hold)
#pragma clang loop vectorize(disable) interleave(disable)
    for (long long p = p0 + sub; p < p1; p += R) {
      const float* q = u.spec + p * u.ps;
      const float im = q[u.im_off + plane], re = q[u.re_off + plane];
      m = fmaxf(m, re * re + im * im);
    }
  }
  sm[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x < u.CH) {
    float t = 0.f;
    for (int r = 0; r < R; ++r) t = fmaxf(t, sm[r * u.CH + threadIdx.x]);
    pmax[((long long)chunk * nblk + blk) * u.CH + threadIdx.x] = t;
  }
}

// smax[chunk][c] = max over blocks
__global__ __launch_bounds__(kRedThreads) void ffl_max_stage2(const float* __restrict__ pmax, int nblk, int CH, float* __restrict__ smax) {
  __shared__ float sm[kRedThreads];
  const int chunk = blockIdx.x;
  const int R = kRedThreads / CH;
  const int sub = threadIdx.x / CH, c = threadIdx.x % CH;
  float m = 0.f;
  if (sub < R)
    for (int blk = sub; blk < nblk; blk += R) m = fmaxf(m, pmax[((long long)chunk * nblk + blk) * CH + c]);
  sm[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x < CH) {
    float t = 0.f;
    for (int r = 0; r < R; ++r) t = fmaxf(t, sm[r * CH + threadIdx.x]);
    smax[(long long)chunk * CH + threadIdx.x] = t;
  }
}

// The element function of reduce_stage1: visits every (pixel, plane) once, replaces U by wgt * U and returns cw * wgt * s.
// MODE 1: alpha = 1 (sqrt), 2: alpha = 2 (the ratio itself), 0: powf(ratio, alpha / 2).
template <int MODE>
struct WeightTerm {
  SpecRef u;
  const float* smax;
  float half_alpha;
  int Wf, nyq;                                                     // nyq: the column kx = w / 2 of an even w, else -1
  __device__ void operator()(int chunk, long long pix, int c, float* v) const {
    const int plane = chunk * u.CH + c;
    v[0] = 0.f;
    if (plane >= u.P) return;
    float* q = u.spec + pix * u.ps;
    const float im = q[u.im_off + plane], re = q[u.re_off + plane];
    const float s = re * re + im * im;
    const float mx = smax[plane];
    const float ratio = mx > 0.f ? s / mx : 0.f;
    float wgt = MODE == 1 ? sqrtf(ratio) : MODE == 2 ? ratio : powf(ratio, half_alpha);
    wgt = wgt == wgt ? fminf(wgt, 1.f) : 0.f;                      // NaN -> 0, then the clamp to [0, 1] (wgt >= 0 by construction)
    q[u.im_off + plane] = wgt * im;
    q[u.re_off + plane] = wgt * re;
    const int kx = (int)(pix % Wf);
    const float cw = (kx == 0 || kx == nyq) ? 1.f : 2.f;
    v[0] = cw * (wgt * s);
  }
};

// loss = scale * (planesum[0] + planesum[1] + ...): strided per thread, then thread 0 adds the 256 in order
__global__ __launch_bounds__(kFflThreads) void ffl_finish_kernel(const float* __restrict__ planesum, int n, float scale,
                                                                 float* __restrict__ loss) {
  __shared__ float sm[kFflThreads];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kFflThreads) s += planesum[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kFflThreads; ++i) t += sm[i];
    loss[0] = scale * t;
  }
}

struct Chunks { int CH, n; long long nblk; };
Chunks chunks_of(int h, int w, int P) {
  Chunks c;
  c.CH = P < kRedThreads ? P : kRedThreads;
  c.n = cdiv(P, c.CH);
  c.nblk = red_blocks((long long)h * (w / 2 + 1));
  return c;
}

bool ffl_sizes_ok(int B, int C, int H, int W, int f) {
  return B > 0 && C > 0 && H > 0 && W > 0 && f > 0 && H % f == 0 && W % f == 0 && (long long)B * C * H * W < (1ll << 40) &&
         (long long)B * f * f * C <= 0x7fffffffll / 4;
}

}  // namespace
}  // namespace fcvsr

using namespace fcvsr;

extern "C" long long fcvsr_ffl_workspace_elems(int h, int w, int P) {
  if (h < 1 || w < 2 || P < 1) return 0;
  const Chunks c = chunks_of(h, w, P);
  return 2ll * c.n * c.CH * (c.nblk + 1);
}

extern "C" int fcvsr_ffl_diff(const float* pred, const float* target, int B, int C, int H, int W, int patch_factor, float* d,
                              int d_channels, void* stream) {
  FCVSR_CHECK_ARG(pred && target && d, "null pointer");
  FCVSR_CHECK_ARG(ffl_sizes_ok(B, C, H, W, patch_factor), "bad sizes (patch_factor must divide H and W)");
  const int f = patch_factor, h = H / f, w = W / f, P = B * f * f * C;
  FCVSR_CHECK_ARG(d_channels >= P, "d_channels: at least B * patch_factor^2 * C");
  const long long npix = (long long)h * w;
  FCVSR_CHECK_ARG(cdiv(npix, kFflThreads) > 0 && npix <= 0x7fffffffll * kFflThreads, "image too large");
  const dim3 grid((unsigned)cdiv(npix, kFflThreads));
  hipStream_t st = (hipStream_t)stream;
  if (d_channels % 4 == 0 && ((uintptr_t)d % 16) == 0)
    hipLaunchKernelGGL((ffl_diff_kernel<true>), grid, dim3(kFflThreads), 0, st, pred, target, C, H, W, f, h, w, P, d_channels, d);
  else
    hipLaunchKernelGGL((ffl_diff_kernel<false>), grid, dim3(kFflThreads), 0, st, pred, target, C, H, W, f, h, w, P, d_channels, d);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_ffl_weight(float* spec, int64_t pix_stride, int im_off, int re_off, int h, int w, int P, float alpha,
                                float loss_weight, float* workspace, long long workspace_elems, float* loss, void* stream) {
  FCVSR_CHECK_ARG(spec && workspace && loss, "null pointer");
  FCVSR_CHECK_ARG(h > 0 && w > 1 && P > 0 && P <= 0x7fffffff / 4, "bad sizes");
  FCVSR_CHECK_ARG(alpha > 0.f, "alpha must be positive");
  FCVSR_CHECK_ARG(im_off >= 0 && re_off >= 0 && (long long)im_off + P <= pix_stride && (long long)re_off + P <= pix_stride &&
                      (im_off + P <= re_off || re_off + P <= im_off),
                  "imaginary and real channel ranges must lie inside a pixel and not overlap");
  FCVSR_CHECK_ARG(workspace_elems >= fcvsr_ffl_workspace_elems(h, w, P), "workspace: fcvsr_ffl_workspace_elems(h, w, P) floats");
  const Chunks c = chunks_of(h, w, P);
  const int Wf = w / 2 + 1;
  const long long npix = (long long)h * Wf;
  FCVSR_CHECK_ARG(c.nblk <= 0x7fffffffll && c.n <= 65535, "image too large");
  const long long plane_elems = (long long)c.n * c.CH;
  float* smax = workspace;
  float* pmax = smax + plane_elems;
  float* psum = pmax + plane_elems * c.nblk;
  float* planesum = psum + plane_elems * c.nblk;
  hipStream_t st = (hipStream_t)stream;
  const SpecRef u{spec, (long long)pix_stride, im_off, re_off, P, c.CH};
  const dim3 grid((unsigned)c.nblk, (unsigned)c.n);
  hipLaunchKernelGGL(ffl_max_stage1, grid, dim3(kRedThreads), 0, st, u, npix, pmax);
  FCVSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ffl_max_stage2, dim3((unsigned)c.n), dim3(kRedThreads), 0, st, (const float*)pmax, (int)c.nblk, c.CH, smax);
  FCVSR_LAUNCH_CHECK();
  const int nyq = w % 2 == 0 ? w / 2 : -1;
  if (alpha == 1.f)
    hipLaunchKernelGGL((reduce_stage1<1, WeightTerm<1>>), grid, dim3(kRedThreads), 0, st, WeightTerm<1>{u, smax, 0.5f, Wf, nyq}, c.n, npix,
                       c.CH, psum);
  else if (alpha == 2.f)
    hipLaunchKernelGGL((reduce_stage1<1, WeightTerm<2>>), grid, dim3(kRedThreads), 0, st, WeightTerm<2>{u, smax, 1.f, Wf, nyq}, c.n, npix,
                       c.CH, psum);
  else
    hipLaunchKernelGGL((reduce_stage1<1, WeightTerm<0>>), grid, dim3(kRedThreads), 0, st, WeightTerm<0>{u, smax, 0.5f * alpha, Wf, nyq}, c.n,
                       npix, c.CH, psum);
  FCVSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(reduce_stage2, dim3((unsigned)c.n), dim3(kRedThreads), 0, st, (const float*)psum, c.n, (int)c.nblk, c.CH, planesum);
  FCVSR_LAUNCH_CHECK();
  const double N = (double)h * (double)w;
  const float scale = (float)((double)loss_weight / ((double)P * N * N));
  hipLaunchKernelGGL(ffl_finish_kernel, dim3(1), dim3(kFflThreads), 0, st, (const float*)planesum, (int)plane_elems, scale, loss);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_ffl_grad(const float* r, int r_channels, const float* g_up, float loss_weight, int B, int C, int H, int W,
                              int patch_factor, float* grad_pred, float* grad_target, void* stream) {
  FCVSR_CHECK_ARG(r && g_up, "null pointer");
  FCVSR_CHECK_ARG(ffl_sizes_ok(B, C, H, W, patch_factor), "bad sizes (patch_factor must divide H and W)");
  const int f = patch_factor, h = H / f, w = W / f, P = B * f * f * C;
  FCVSR_CHECK_ARG(r_channels >= P, "r_channels: at least B * patch_factor^2 * C");
  if (!grad_pred && !grad_target) return 0;
  const long long npix = (long long)h * w;
  FCVSR_CHECK_ARG(npix <= 0x7fffffffll * kFflThreads, "image too large");
  const float scale = (float)(2.0 * (double)loss_weight / ((double)P * (double)npix));
  const dim3 grid((unsigned)cdiv(npix, kFflThreads));
  hipStream_t st = (hipStream_t)stream;
  if (r_channels % 4 == 0 && P % 4 == 0 && ((uintptr_t)r % 16) == 0)
    hipLaunchKernelGGL((ffl_grad_kernel<true>), grid, dim3(kFflThreads), 0, st, r, g_up, scale, C, H, W, f, h, w, P, r_channels, grad_pred,
                       grad_target);
  else
    hipLaunchKernelGGL((ffl_grad_kernel<false>), grid, dim3(kFflThreads), 0, st, r, g_up, scale, C, H, W, f, h, w, P, r_channels, grad_pred,
                       grad_target);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
