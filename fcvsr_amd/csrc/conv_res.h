// LDS-resident-weight 3x3 MFMA convolution (conv_res.hip): argument block shared with the dispatcher in conv_mfma.hip.
#pragma once
#include "common.h"

namespace fcvsr {

struct ResGroup {
  View src, res[2], dst;
  float* gc_partial;      // ContextBlock partials [B][tiles_y*tiles_x*4][cout+2] (one per wave pair of rows), or nullptr
  int B, H, W;
  int tiles_x, tiles_y;   // 8 x 32 pixel tiles
  int tile_begin;
};

struct ResArgs {
  int n_groups;
  ResGroup g[3];
  int total_tiles;
  int cin, cout, cout_pad, cin_pad;
  const uint16_t* w;      // [tap][cout_pad][cin_pad], 16-bit, cin contiguous (pack_conv_weight_mfma)
  const float* bias;
  int act;
  float slope;
  const float* slope_ptr;
  float rs[2];
  int n_res, res16;
  int ps;                 // PixelShuffle(2) store (cin 64, cout % 256 == 0, rows packed sub-pixel-major): cout block nb is sub-pixel nb / (cout/256)
  const void* zeros;      // >= 16 zero bytes: source of the halo pixels that lie outside the image
};

// returns hipSuccess, or hipErrorInvalidValue when the shape is not one the kernel is built for
hipError_t launch_conv3_res(const ResArgs& a, bool bf16, bool dst16, hipStream_t st);
bool conv3_res_supports(int cin, int cout);
// the instantiation conv3_res_kernel<BF16, mode, nch, nsu> that serves a problem (the launch and the reported kernel name use it).
// mode: 0 f32 destination, 1 16-bit destination with residuals, 2 16-bit without; nch: 64-channel input chunks; nsu: how much
// the host knows about the activation's negative slope ns: 2 none (identity), 1 0 <= ns <= 1 (act(x) = max(x, ns * x)), 0 neither
// (PReLU: the slope is in device memory)
struct ResVariant { int mode, nch, nsu; };
ResVariant conv3_res_variant(int cin, int n_res, int act, float slope, bool dst16);
// *zeros: this device's 256 zero bytes (ResArgs::zeros), created on first use; hipErrorStreamCaptureUnsupported when that first
// use is inside a stream capture
hipError_t conv3_res_zero_page(hipStream_t st, const void** zeros);
// 8 x 32 tiles of one problem
inline int conv3_res_tiles(int B, int H, int W) { return B * ((H + 7) / 8) * ((W + 31) / 32); }

}  // namespace fcvsr
