// The resizer form the no-reference scores call between their two scales (resize.hip).
#pragma once
#include "common.h"

namespace fcvsr {

// MATLAB-style antialiased 2x down-scale of f64 planes of integers: read as f32(v / 255), stored as f64(f32 result) * 255
void downscale2_f64(const double* src, long long planes, int H, int W, double* dst, hipStream_t stream);

}  // namespace fcvsr
