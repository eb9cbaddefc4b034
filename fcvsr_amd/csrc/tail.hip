// Up-sampler tail helpers (reference CVSR_freq.py:2633-2645): PixelShuffle(2) of a dense NHWC tensor and the x4 bilinear
// base skip F.interpolate(shortcut[:, T//2], scale_factor=4, mode='bilinear') (align_corners=False).
#include "common.h"
#include "mfma_util.h"
#include "bilinear.h"

namespace fcvsr {

// dst[b][2h+i][2w+j][c] = src[b][h][w][4c+2i+j]
__global__ void pixel_shuffle_kernel(const float* src, float* dst, int B, int H, int W, int C) {
  const long long total = (long long)B * H * W * C;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int ci = (int)(t % C);
  const long long pg = t / C;
  const int x = (int)(pg % W);
  const int y = (int)((pg / W) % H);
  const int b = (int)(pg / ((long long)W * H));
  const int c2 = ci >> 2, i = (ci >> 1) & 1, j = ci & 1;
  const int Co = C / 4;
  dst[(((long long)b * 2 * H + 2 * y + i) * 2 * W + 2 * x + j) * Co + c2] = src[t];
}

// The same shuffle into channels [0, C/4) of a 16-bit destination view whose channels [C/4, dst.c) are written as zeros: the
// narrow pyramid level l3_2 stored straight into the dense 16-bit input of upconv_fuse, zero pad included.  Rounded with
// cvt4, as the consumer's staging of an f32 source rounds.  One thread = one pixel x 8 channels = one 16-byte store.
template <bool BF16>
__global__ void pixel_shuffle16_kernel(const float* src, View dst, int B, int H, int W, int C) {
  const int ng = dst.c >> 3;
  const long long total = (long long)B * 4 * H * W * ng;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t % ng);
  const long long pg = t / ng;
  const int X = (int)(pg % (2 * W));
  const int Y = (int)((pg / (2 * W)) % (2 * H));
  const int b = (int)(pg / (4ll * W * H));
  const float* sp = src + (((long long)b * H + (Y >> 1)) * W + (X >> 1)) * C + 2 * (Y & 1) + (X & 1);
  const int Co = C / 4;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = 8 * g + k;
    v[k] = c < Co ? sp[4 * c] : 0.f;
  }
  const uint2 lo = cvt4<BF16>(make_float4(v[0], v[1], v[2], v[3])), hi = cvt4<BF16>(make_float4(v[4], v[5], v[6], v[7]));
  *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(dst.p) + (long long)b * dst.sb + (long long)Y * dst.sy + (long long)X * dst.sx + 8 * g) =
      make_uint4(lo.x, lo.y, hi.x, hi.y);
}

template <int SRC>
__device__ __forceinline__ void bilinear_up4_px(View src, const float* tab, int B, int H, int W, View dst) {
  const int Ho = 4 * H, Wo = 4 * W;
  const long long total = (long long)B * Ho * Wo * dst.c;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  // x fastest so that NCHW destinations are written coalesced
  const int ox = (int)(t % Wo);
  const int oy = (int)((t / Wo) % Ho);
  const int c = (int)((t / ((long long)Wo * Ho)) % dst.c);
  const int b = (int)(t / ((long long)Wo * Ho * dst.c));
  const float v = bilinear_up4_at<SRC>(src, tab, H, W, b, c, oy, ox);
  dst.p[(long long)b * dst.sb + (long long)oy * dst.sy + (long long)ox * dst.sx + (long long)c * dst.sc] = v;
}

__global__ void bilinear_up4_kernel(View src, int B, int H, int W, View dst) { bilinear_up4_px<kSrcF32>(src, nullptr, B, H, W, dst); }

__global__ void bilinear_up4_u8_kernel(View src, const float* tab, int B, int H, int W, View dst) {
  bilinear_up4_px<kSrcU8>(src, tab, B, H, W, dst);
}

__global__ void bilinear_up4_u16_kernel(View src, const float* tab, int B, int H, int W, View dst) {
  bilinear_up4_px<kSrcU16>(src, tab, B, H, W, dst);
}

}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_pixel_shuffle(const float* src, float* dst, int B, int H, int W, int C, void* stream) {
  FCVSR_CHECK_ARG(src && dst, "null pointer");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "C%4==0 required");
  const long long total = (long long)B * H * W * C;
  hipLaunchKernelGGL(pixel_shuffle_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, B, H, W, C);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_pixel_shuffle16(const float* src, const fcvsr_view* dst, int B, int H, int W, int C, void* stream) {
  FCVSR_CHECK_ARG(src && dst && dst->ptr, "null pointer");
  FCVSR_CHECK_ARG(dst->dtype == FCVSR_BF16 || dst->dtype == FCVSR_F16, "16-bit destination");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && dst->c % 8 == 0 && dst->c >= C / 4, "C%4==0, dst.c%8==0, dst.c>=C/4");
  FCVSR_CHECK_ARG(dst->sc == 1 && dst->sx % 8 == 0 && dst->sy % 8 == 0 && dst->sb % 8 == 0 && ((uintptr_t)dst->ptr % 16) == 0,
                  "dst: channel-contiguous, 16-byte-aligned pixels");
  const long long total = (long long)B * 4 * H * W * (dst->c / 8);
  if (dst->dtype == FCVSR_BF16)
    hipLaunchKernelGGL(pixel_shuffle16_kernel<true>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, to_view(*dst), B, H, W, C);
  else
    hipLaunchKernelGGL(pixel_shuffle16_kernel<false>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, to_view(*dst), B, H, W, C);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_bilinear_up4(const fcvsr_view* src, int B, int H, int W, const fcvsr_view* dst, void* stream) {
  FCVSR_CHECK_ARG(src && dst && src->ptr && dst->ptr, "null pointer");
  FCVSR_CHECK_ARG(src->dtype == FCVSR_F32 && dst->dtype == FCVSR_F32, "f32 only");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && src->c == dst->c && dst->c > 0, "bad sizes");
  const long long total = (long long)B * 16 * H * W * dst->c;
  hipLaunchKernelGGL(bilinear_up4_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, to_view(*src), B, H, W,
                     to_view(*dst));
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_bilinear_up4_u8(const fcvsr_view* src, const float* tab, int B, int H, int W, const fcvsr_view* dst, void* stream) {
  FCVSR_CHECK_ARG(src && dst && src->ptr && dst->ptr && tab, "null pointer");
  FCVSR_CHECK_ARG(src->dtype == FCVSR_U8 && dst->dtype == FCVSR_F32, "uint8 source, f32 destination");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && src->c == dst->c && dst->c > 0, "bad sizes");
  const long long total = (long long)B * 16 * H * W * dst->c;
  hipLaunchKernelGGL(bilinear_up4_u8_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, to_view(*src), tab, B, H,
                     W, to_view(*dst));
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_bilinear_up4_u16(const fcvsr_view* src, const float* tab, int B, int H, int W, const fcvsr_view* dst, void* stream) {
  FCVSR_CHECK_ARG(src && dst && src->ptr && dst->ptr && tab, "null pointer");
  FCVSR_CHECK_ARG(src->dtype == FCVSR_U16 && dst->dtype == FCVSR_F32, "uint16 source, f32 destination");
  FCVSR_CHECK_ARG(((uintptr_t)src->ptr % 2) == 0, "src: 2-byte aligned");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && src->c == dst->c && dst->c > 0, "bad sizes");
  const long long total = (long long)B * 16 * H * W * dst->c;
  hipLaunchKernelGGL(bilinear_up4_u16_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, to_view(*src), tab, B, H,
                     W, to_view(*dst));
  FCVSR_LAUNCH_CHECK();
  return 0;
}
