// The device pieces of the MATLAB-style bicubic up-scale that resize.hip (upscale_kernel) and active.hip (active_compose_kernel)
// share: the taps, the border rule, how a sample is read and how a result is rounded and stored.  Both kernels therefore have the
// reference's arithmetic and its bits: f32 products added in tap order (the library is built with -ffp-contract=off).
#pragma once
#include "common.h"

namespace fcvsr {
namespace bicubic_up {

template <int F> struct UpTaps;
template <> struct UpTaps<2> {
  __device__ static float w(int phase, int k) {
    constexpr float t[2][4] = {{-3.f / 128, 29.f / 128, 111.f / 128, -9.f / 128}, {-9.f / 128, 111.f / 128, 29.f / 128, -3.f / 128}};
    return t[phase][k];
  }
};
template <> struct UpTaps<4> {
  __device__ static float w(int phase, int k) {
    constexpr float t[4][4] = {{-45.f / 1024, 399.f / 1024, 745.f / 1024, -75.f / 1024},
                               {-7.f / 1024, 93.f / 1024, 987.f / 1024, -49.f / 1024},
                               {-49.f / 1024, 987.f / 1024, 93.f / 1024, -7.f / 1024},
                               {-75.f / 1024, 745.f / 1024, 399.f / 1024, -45.f / 1024}};
    return t[phase][k];
  }
};

// out-of-range indices reflected with edge repeat (-1 -> 0, -2 -> 1, n -> n-1), periodic in 2n as the reference's index table
__device__ inline int reflect(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

__device__ inline float up_sample(const unsigned char* p, long long off) { return (float)p[off]; }
__device__ inline float up_sample(const unsigned short* p, long long off) {   // 10-bit: a sample above 1023 reads as 1023
  const unsigned short v = p[off];
  return (float)(v > 1023 ? 1023 : v);
}
__device__ inline float up_sample(const float* p, long long off) { return p[off]; }

// np.around(np.clip(v, 0, peak)) for the integer forms; f32 as it is.  A NaN gives sample 0 because of the clamp order (fmaxf
// drops it for the 0), and rintf is half to even: v is a sum of exact dyadic products, so ties are met and compared exactly.
__device__ inline void up_result(float v, float& o) { o = v; }
__device__ inline void up_result(float v, unsigned char& o) { o = (unsigned char)rintf(fminf(fmaxf(v, 0.f), 255.f)); }
__device__ inline void up_result(float v, unsigned short& o) { o = (unsigned short)rintf(fminf(fmaxf(v, 0.f), 1023.f)); }

__device__ inline void up_store4(float* p, const float o[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }
__device__ inline void up_store4(unsigned char* p, const unsigned char o[4]) {
  *reinterpret_cast<uchar4*>(p) = make_uchar4(o[0], o[1], o[2], o[3]);
}
__device__ inline void up_store4(unsigned short* p, const unsigned short o[4]) {
  *reinterpret_cast<ushort4*>(p) = make_ushort4(o[0], o[1], o[2], o[3]);
}

}  // namespace bicubic_up
}  // namespace fcvsr
