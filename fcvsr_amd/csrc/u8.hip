// Integer frame conversions around the model, and the 4x chroma up-sampler of the YUV 4:2:0 sequence path.  Every kernel exists for
// 8-bit frames (uint8, peak 255) and for 10-bit samples in 16-bit containers (uint16, peak 1023: the *_u16 entry points); below,
// "255" stands for the peak of the format.
//   * u8_to_f32: uint8 window -> f32 (pixel k -> tab[k], u8.h) for the configurations whose first layer reads f32 (exact-f32 mode,
//     the RGB twins' 21-channel feat_extract);
//   * quantise_u8: f32 result -> uint8 frame (u8.h) where the last layer is the generic convolution (f32 mode);
//   * chroma_up4: one 8-bit plane x4, defined as F.interpolate(p.float() / 255, scale_factor=4, mode="bicubic",
//     align_corners=False), clamp, * 255, rounded half to even.  The weights are torch's (A = -0.75, source x = (X + 0.5) / 4 - 0.5,
//     taps clamped to the plane), separable: rows first, then the column.  A thread makes the 4 output pixels of one input column
//     in one output row (one 4-byte store, 8 bytes for uint16); they read input columns x-2 .. x+2.
#include "common.h"
#include "u8.h"

namespace fcvsr {

template <class T, int PEAK>
__global__ void int_to_f32_kernel(const T* src, const float* tab, long long n, float* dst) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = sample_value<PEAK>(tab, src[t]);
}

template <int Q, class T, int PEAK>
__global__ void quantise_kernel(const float* src, long long n, T* dst) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = quantise<Q, PEAK, T>(src[t]);
}

__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
  const float A = -0.75f;
  const float x1 = t + 1.0f, x2 = 1.0f - t, x3 = x2 + 1.0f;
  c[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
  c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

template <class T, int PEAK>
__global__ void chroma_up4_kernel(const T* src, const float* tab, int P, int h, int w, T* dst) {
  const int Ho = 4 * h, Wo = 4 * w;
  const long long total = (long long)P * Ho * w;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int ix = (int)(t % w);
  const int oy = (int)((t / w) % Ho);
  const int p = (int)(t / ((long long)w * Ho));
  const T* sp = src + (long long)p * h * w;
  const float ry = 0.25f * ((float)oy + 0.5f) - 0.5f;
  const float fy = floorf(ry);
  const int iy = (int)fy;
  float cy[4];
  cubic_coeffs(ry - fy, cy);
  // rows iy-1 .. iy+2 and columns ix-2 .. ix+2, clamped to the plane
  float v[4][5];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int yy = iy - 1 + r;
    yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      int xx = ix - 2 + k;
      xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
      v[r][k] = sample_value<PEAK>(tab, sp[(long long)yy * w + xx]);
    }
  }
  T o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float rx = 0.25f * ((float)(4 * ix + j) + 0.5f) - 0.5f;
    const float fx = floorf(rx);
    const int k0 = (int)fx - ix + 1;                       // first of the 4 taps in v[][] (0 for j < 2, 1 otherwise)
    float cx[4];
    cubic_coeffs(rx - fx, cx);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float row = v[r][k0] * cx[0] + v[r][k0 + 1] * cx[1] + v[r][k0 + 2] * cx[2] + v[r][k0 + 3] * cx[3];
      s = r == 0 ? row * cy[0] : s + row * cy[r];
    }
    o[j] = quantise<FCVSR_QUANT_ROUND, PEAK, T>(s);
  }
  T* dp = dst + (long long)p * Ho * Wo + (long long)oy * Wo + 4 * ix;
  if constexpr (sizeof(T) == 1) *reinterpret_cast<uchar4*>(dp) = make_uchar4(o[0], o[1], o[2], o[3]);
  else *reinterpret_cast<ushort4*>(dp) = make_ushort4(o[0], o[1], o[2], o[3]);
}

}  // namespace fcvsr

using namespace fcvsr;

template <class T, int PEAK>
static int int_to_f32_launch(const T* src, const float* tab, long long n, float* dst, void* stream) {
  FCVSR_CHECK_ARG(src && tab && dst && n > 0, "null pointer or empty");
  FCVSR_CHECK_ARG(((uintptr_t)src % sizeof(T)) == 0, "src: aligned to its sample size");
  hipLaunchKernelGGL((int_to_f32_kernel<T, PEAK>), dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, src, tab, n, dst);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

template <class T, int PEAK>
static int quantise_launch(const float* src, long long n, int quantise, T* dst, void* stream) {
  FCVSR_CHECK_ARG(src && dst && n > 0, "null pointer or empty");
  FCVSR_CHECK_ARG(((uintptr_t)dst % sizeof(T)) == 0, "dst: aligned to its sample size");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  const dim3 grid(cdiv(n, 256));
  if (quantise == FCVSR_QUANT_TRUNCATE)
    hipLaunchKernelGGL((quantise_kernel<FCVSR_QUANT_TRUNCATE, T, PEAK>), grid, dim3(256), 0, (hipStream_t)stream, src, n, dst);
  else
    hipLaunchKernelGGL((quantise_kernel<FCVSR_QUANT_ROUND, T, PEAK>), grid, dim3(256), 0, (hipStream_t)stream, src, n, dst);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

template <class T, int PEAK>
static int chroma_up4_launch(const T* src, const float* tab, int P, int h, int w, T* dst, void* stream) {
  FCVSR_CHECK_ARG(src && tab && dst, "null pointer");
  FCVSR_CHECK_ARG(P > 0 && h > 0 && w > 0, "bad sizes");
  FCVSR_CHECK_ARG(((uintptr_t)src % sizeof(T)) == 0, "src: aligned to its sample size");
  FCVSR_CHECK_ARG(((uintptr_t)dst % (4 * sizeof(T))) == 0, "dst: aligned to four samples (4 bytes, 8 for uint16)");
  const long long total = (long long)P * 4 * h * w;
  FCVSR_CHECK_ARG(total < (1ll << 40), "too large");
  hipLaunchKernelGGL((chroma_up4_kernel<T, PEAK>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, src, tab, P, h, w, dst);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_u8_to_f32(const uint8_t* src, const float* tab, long long n, float* dst, void* stream) {
  return int_to_f32_launch<uint8_t, kPeak8>(src, tab, n, dst, stream);
}

extern "C" int fcvsr_u16_to_f32(const uint16_t* src, const float* tab, long long n, float* dst, void* stream) {
  return int_to_f32_launch<uint16_t, kPeak10>(src, tab, n, dst, stream);
}

extern "C" int fcvsr_quantise_u8(const float* src, long long n, int quantise, uint8_t* dst, void* stream) {
  return quantise_launch<uint8_t, kPeak8>(src, n, quantise, dst, stream);
}

extern "C" int fcvsr_quantise_u16(const float* src, long long n, int quantise, uint16_t* dst, void* stream) {
  return quantise_launch<uint16_t, kPeak10>(src, n, quantise, dst, stream);
}

extern "C" int fcvsr_chroma_up4(const uint8_t* src, const float* tab, int P, int h, int w, uint8_t* dst, void* stream) {
  return chroma_up4_launch<uint8_t, kPeak8>(src, tab, P, h, w, dst, stream);
}

extern "C" int fcvsr_chroma_up4_u16(const uint16_t* src, const float* tab, int P, int h, int w, uint16_t* dst, void* stream) {
  return chroma_up4_launch<uint16_t, kPeak10>(src, tab, P, h, w, dst, stream);
}
