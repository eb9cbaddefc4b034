// Integer frame I/O helpers shared by the *_u8 and *_u16 entry points.  A sample format is a storage type and a peak:
// uint8_t / 255 (8-bit frames) or uint16_t / 1023 (10-bit samples in 16-bit containers).
//   in:  sample k enters as tab[min(k, PEAK)], a (PEAK + 1)-entry f32 table the host builds with torch (k -> .float() / PEAK), so a
//        kernel fed integer frames sees exactly the floats the f32 path is fed when the caller converts on the host; the min keeps
//        a 16-bit container's out-of-range samples inside the table (the float path's x.clamp(max=1023)) and folds away for uint8;
//   out: the f32 value v the f32 path stores becomes clamp(v, 0, 1) * PEAK (f32 multiply), truncated toward zero or rounded
//        half to even - the samples the harness's torch passes (clamp, * PEAK, optional round, cast) make from it.
#pragma once
#include "common.h"

namespace fcvsr {

constexpr int kPeak8 = 255, kPeak10 = 1023;

// how a kernel's frames are stored: f32, or integer samples read through the table
enum { kSrcF32 = 0, kSrcU8 = 1, kSrcU16 = 2 };

template <int PEAK> struct SampleOf;
template <> struct SampleOf<kPeak8> { typedef uint8_t type; };
template <> struct SampleOf<kPeak10> { typedef uint16_t type; };

template <int SRC> struct SrcFormat;
template <> struct SrcFormat<kSrcU8> { typedef uint8_t type; static constexpr int peak = kPeak8; };
template <> struct SrcFormat<kSrcU16> { typedef uint16_t type; static constexpr int peak = kPeak10; };

template <int PEAK, class T>
__device__ __forceinline__ float sample_value(const float* tab, T k) {
  const int i = (int)k;
  return tab[i < PEAK ? i : PEAK];
}

// the out rule, in f32; `mode` is FCVSR_QUANT_TRUNCATE or FCVSR_QUANT_ROUND, known at compile time (quantise) or at run time
// (score_common.h frame_sample).  A NaN gives sample 0 because of the clamp order (fmaxf drops it for the 0 before fminf sees it),
// and the samples equal the harness's at ties (v * PEAK == k + 0.5) because the product is one f32 multiply: no fma, no f64.
template <int PEAK>
__device__ __forceinline__ float quantised(float v, int mode) {
  const float q = fminf(fmaxf(v, 0.f), 1.f) * (float)PEAK;
  return mode == FCVSR_QUANT_TRUNCATE ? truncf(q) : rintf(q);
}

template <int Q, int PEAK, class T>
__device__ __forceinline__ T quantise(float v) {
  static_assert(Q == FCVSR_QUANT_TRUNCATE || Q == FCVSR_QUANT_ROUND, "quantise mode");
  return (T)quantised<PEAK>(v, Q);
}

template <int Q>
__device__ __forceinline__ uint8_t quantise_u8(float v) {
  return quantise<Q, kPeak8, uint8_t>(v);
}

}  // namespace fcvsr
