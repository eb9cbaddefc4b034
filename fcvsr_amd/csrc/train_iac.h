// What train_iac.hip shares with train_iac_det.hip: the argument test of the kernel view and the source pass of the atomic-free
// IAC warp backward (iac_bwd_warp_kernel with its scatter switched off).
#pragma once
#include "common.h"

namespace fcvsr {

// k1 / gk: f32 view with 3*C contiguous channels, strides multiples of 4, 16-byte aligned
bool iac_k1_ok(const fcvsr_view* v, int C);

// g_s (B,H,W,C), g_off (B,H,W,2), and per pixel p: key_out[p] = destination cell, id_out[p] = p.  C in {32, 64}; arguments checked
// by the caller.  One launch on `stream`.
void iac_bwd_warp_source_launch(const float* gv, const fcvsr_view& k1, const float* prev, const fcvsr_view& off, int B, int H, int W, int C,
                                float* goff, float* gs_out, unsigned* key_out, unsigned* id_out, hipStream_t stream);

}  // namespace fcvsr
