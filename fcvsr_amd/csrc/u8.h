// uint8 frame I/O helpers shared by the *_u8 entry points.
//   in:  pixel k enters as tab[k], a 256-entry f32 table the host builds with torch (uint8 -> .float() / 255), so a kernel fed
//        uint8 frames sees exactly the floats the f32 path is fed when the caller converts on the host;
//   out: the f32 value v the f32 path stores becomes clamp(v, 0, 1) * 255.0f (f32 multiply), truncated toward zero or rounded
//        half to even - the bytes the harness's torch passes (clamp, * 255, optional round, .to(uint8)) make from it.
#pragma once
#include "common.h"

namespace fcvsr {

template <int Q>
__device__ __forceinline__ uint8_t quantise_u8(float v) {
  static_assert(Q == FCVSR_QUANT_TRUNCATE || Q == FCVSR_QUANT_ROUND, "quantise mode");
  const float q = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;
  return (uint8_t)(Q == FCVSR_QUANT_TRUNCATE ? truncf(q) : rintf(q));
}

}  // namespace fcvsr
