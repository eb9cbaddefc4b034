// Planner of fcvsr_conv2d_mfma (conv_plan.hip): which of the six 16-bit convolution kernels serves a problem, and the final
// argument block of that kernel.  Pure host arithmetic on the descriptors: no HIP call, no environment, no tensor access.
#pragma once
#include "common.h"

namespace fcvsr {

// tile rows (one per wave: 4-row tiles leave room for more co-resident workgroups in different phases; 8-row tiles measured
// 0.85-1.0x), tile cols, channel chunk, padded LDS row (halfwords)
constexpr int kTH = 4, kTW = 32, kCK = 64, kLD = kCK + 8;

struct MGroup {
  View src[3];
  View res[2];
  View dst;
  float* gc_partial;   // [B][tiles_per_image*4][cout+2] (nullptr = off)
  int B, H, W;         // spatial size (stride-1 "same" conv: output size == input size)
  int tiles_x, tiles_y;
  int tile_begin;      // first flattened tile id of this group
};

struct MfmaArgs {
  int n_groups;
  MGroup g[3];
  int n_src, n_res;
  int seg_c[3];        // channels per source segment
  int cin_total, cin16, cin_pad, cout, cout_pad, n_nblk;
  const uint16_t* w;   // [taps][cout_pad][cin_pad]
  const float* bias;
  int act;
  float slope;
  const float* slope_ptr;
  float rs[2];
  int ps;
  int flat;            // 1x1: treat pixels as a flat list of B*H*W
  int src16, dst16;    // sources / destination stored in the MFMA dtype (16-bit) instead of f32
  int dstbf;           // the 16-bit destination format is bf16 (generic kernel: may differ from the MFMA dtype)
  int res16;           // residual inputs stored in the MFMA dtype (lean 3x3 kernel only: 16-bit trunk)
  int gc16;            // lean 3x3 kernel with ContextBlock fusion: the 4-couts-per-lane epilogue stores the MFMA dtype (8 bytes)
  const float* gc_wmask;   // ContextBlock fusion: per-wave online-softmax partials of the output (cout <= 64, 3x3)
  int planar;          // single f32 source with arbitrary channel stride (the NCHW frames of feat_extract), cin <= 64
  int sub2;            // stride-2 convolution: evaluate at full resolution, keep the even output pixels only
};

// In order of precedence, highest first: kRes1PS > kLean3S2 > kLean1 > kRes3 > kLean3 > kGeneric.
enum ConvPath {
  kGeneric,    // conv_mfma_kernel: everything the argument checks admit
  kLean3,      // conv3_lean_kernel: 3x3 stride 1, one dense source of a multiple of 64 channels
  kLean3S2,    // conv3s2_lean_kernel: 3x3 stride 2, the same source, cout a multiple of 64, no residuals
  kLean1,      // conv1_lean_kernel: 1x1, every source a multiple of 64 channels
  kRes1PS,     // conv1ps_res_kernel: 1x1 pixel-shuffle up-convolution 64 -> cout <= 256, resident weights, 16-bit in and out
  kRes3        // conv3_res_kernel (conv_res.hip): 3x3 stride 1, 64 or 128 dense 16-bit input channels, resident weights
};

// lean: 0 no lean kernel (kLean3, kLean3S2, kLean1, and with them kRes1PS and every kRes3 layer that is not pixel-shuffled), 1 allowed
// res (resident-weight kernels): 0 never, 1 whenever eligible, 2 kRes3 by size (kResMinTiles workgroup-tiles), kRes1PS whenever eligible
struct ConvPolicy { int lean, res; };
struct ConvPlan {
  ConvPath path;
  bool bf16;          // MFMA operand type (else f16)
  int nt;             // output channels per workgroup (32 or 64) of the generic and lean kernels
  int total_tiles;    // pixel tiles of all groups, as args.g[].tile_begin counts them
  MfmaArgs args;      // final, for the chosen path
};

// 0 and *plan, or FCVSR_E_ARG with the error text set.  Looks at descriptor fields and pointer alignment only.
int plan_conv2d_mfma(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, ConvPolicy policy, ConvPlan* plan);
// the name fcvsr_last_conv_kernel() reports for the plan: the kernel with its template arguments (bench.py groups by it)
void format_kernel_name(const ConvPlan& plan, char* out, size_t cap);

}  // namespace fcvsr
