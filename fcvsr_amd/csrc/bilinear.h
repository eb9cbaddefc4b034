// One output value of the x4 bilinear base skip F.interpolate(scale_factor=4, mode='bilinear', align_corners=False) (reference
// CVSR_freq.py:2644), shared by the stand-alone kernels (tail.hip) and the fused up-sampler tail (tail_fused.hip), which evaluates
// it for the pixel a thread owns instead of reading a stored base: one expression, so both give the same bits.
#pragma once
#include "common.h"
#include "u8.h"

namespace fcvsr {

// The four source values and the two weights of one output value: fetched where the loads can be issued early, blended (in the
// one order every caller shares) where the value is needed.
struct BilinearTaps { float v00, v01, v10, v11, ly, lx; };

// SRC != kSrcF32: src holds integer frames (uint8, or 10-bit samples in uint16), sample k read through the table (u8.h) - the same
// arithmetic on the same f32 values as the f32 source
template <int SRC>
__device__ __forceinline__ BilinearTaps bilinear_up4_fetch(const View& src, const float* tab, int H, int W, int b, int c, int oy, int ox) {
  float sy = 0.25f * ((float)oy + 0.5f) - 0.5f; sy = sy < 0.f ? 0.f : sy;
  float sx = 0.25f * ((float)ox + 0.5f) - 0.5f; sx = sx < 0.f ? 0.f : sx;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  BilinearTaps t;
  t.ly = sy - (float)y0; t.lx = sx - (float)x0;
  const long long o00 = (long long)y0 * src.sy + (long long)x0 * src.sx, o01 = (long long)y0 * src.sy + (long long)x1 * src.sx;
  const long long o10 = (long long)y1 * src.sy + (long long)x0 * src.sx, o11 = (long long)y1 * src.sy + (long long)x1 * src.sx;
  if constexpr (SRC != kSrcF32) {
    typedef typename SrcFormat<SRC>::type T;
    constexpr int PEAK = SrcFormat<SRC>::peak;
    const T* sp = reinterpret_cast<const T*>(src.p) + (long long)b * src.sb + (long long)c * src.sc;
    t.v00 = sample_value<PEAK>(tab, sp[o00]); t.v01 = sample_value<PEAK>(tab, sp[o01]);
    t.v10 = sample_value<PEAK>(tab, sp[o10]); t.v11 = sample_value<PEAK>(tab, sp[o11]);
  } else {
    const float* sp = src.p + (long long)b * src.sb + (long long)c * src.sc;
    t.v00 = sp[o00]; t.v01 = sp[o01]; t.v10 = sp[o10]; t.v11 = sp[o11];
  }
  return t;
}

__device__ __forceinline__ float bilinear_up4_blend(const BilinearTaps& t) {
  return (1.f - t.ly) * ((1.f - t.lx) * t.v00 + t.lx * t.v01) + t.ly * ((1.f - t.lx) * t.v10 + t.lx * t.v11);
}

template <int SRC>
__device__ __forceinline__ float bilinear_up4_at(const View& src, const float* tab, int H, int W, int b, int c, int oy, int ox) {
  return bilinear_up4_blend(bilinear_up4_fetch<SRC>(src, tab, H, W, b, c, oy, ox));
}

}  // namespace fcvsr
