// plan_conv2d_mfma: argument checks, path decision and path-specific retiling of fcvsr_conv2d_mfma, and the kernel name of a plan.
// Host arithmetic only (conv_plan.h); fcvsr_conv2d_mfma_plan exposes it, so a dispatch decision can be tested without a GPU.
#include "conv_plan.h"
#include "conv_res.h"

namespace fcvsr {
namespace {

// FCVSR_CHECK_ARG under the name of the entry point the caller used
#define PLAN_CHECK(cond, msg) \
  do { if (!(cond)) { set_error("fcvsr_conv2d_mfma: %s (%s:%d)", msg, __FILE__, __LINE__); return FCVSR_E_ARG; } } while (0)

// the resident-weight 3x3 kernel pays once a launch has this many workgroup-tiles (tiles x cout blocks): below it, the lean kernel
constexpr int kResMinTiles = 768;

bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
bool strides_mod(const fcvsr_view& v, int g) { return v.sx % g == 0 && v.sy % g == 0 && v.sb % g == 0; }
// channel-contiguous res/dst views are accessed as quads: 16 bytes of f32, 8 bytes of a 16-bit type
bool vec_view_ok(const fcvsr_view& v) {
  return v.sc != 1 || v.c < 4 || (strides_mod(v, 4) && ((uintptr_t)v.ptr % (v.dtype == FCVSR_F32 ? 16 : 8)) == 0);
}

// sources: f32 (converted while staging, 4 channels = 16 bytes per lane) or already in the MFMA dtype (8 channels per lane)
bool src_ok(const fcvsr_view& v, int mma_dtype) {
  if (!v.ptr || v.sc != 1 || !aligned16(v.ptr)) return false;
  const int g = v.dtype == FCVSR_F32 ? 4 : 8;
  if (v.dtype != FCVSR_F32 && v.dtype != mma_dtype) return false;
  return v.c % g == 0 && strides_mod(v, g);
}

// the lean kernels store f32 or the MFMA dtype only
bool dst_native(const fcvsr_conv_desc& d0, int mma_dtype) { return d0.dst.dtype == FCVSR_F32 || d0.dst.dtype == mma_dtype; }
// 3x3 of the given stride with one dense source of a multiple of 64 channels
bool dense3(const fcvsr_conv_desc& d0, const MfmaArgs& a, int stride) { return d0.kh == 3 && d0.stride == stride && a.n_src == 1 && !a.planar && a.cin_total % 64 == 0; }
// channel-contiguous destination on 16-byte granules (quads of f32, octets of a 16-bit type)
bool dst_vec16(const fcvsr_view& v, bool dst16) { return v.sc == 1 && strides_mod(v, dst16 ? 8 : 4) && aligned16(v.ptr); }

// kLean3: 3x3 stride 1, one dense source, cin multiple of 64, plain channel-contiguous destination and residuals
bool lean3_ok(const fcvsr_conv_desc* descs, int n, const MfmaArgs& a, int mma_dtype) {
  bool ok = dst_native(descs[0], mma_dtype) && dense3(descs[0], a, 1) && !a.ps && (!a.dst16 || a.cout % 8 == 0) && (a.gc_wmask == nullptr || a.cout % 4 == 0);
  for (int g = 0; g < n && ok; ++g) {
    const fcvsr_conv_desc& d = descs[g];
    long long ext = (long long)d.B * d.H * d.W * (long long)(d.src[0].sx > d.dst.sx ? d.src[0].sx : d.dst.sx);
    if (d.dst.sc != 1) ext = (long long)d.B * d.dst.sb;                 // strided (e.g. NCHW) destination
    ok = (!a.dst16 || d.dst.sc == 1) && ext < (1ll << 29);
    for (int q = 0; q < d.n_res; ++q) ok = ok && (d.res[q].dtype == FCVSR_F32 || d.res[q].sc == 1) && (!a.dst16 || d.res[q].sc == 1);
  }
  return ok;
}

// kLean1: 1x1 (flat), every source a multiple of 64 channels, channel-contiguous destination, f32 residuals; pixel shuffle only without residuals
bool lean1_ok(const fcvsr_conv_desc* descs, int n, const MfmaArgs& a, int mma_dtype) {
  const fcvsr_conv_desc& d0 = descs[0];
  bool ok = dst_native(d0, mma_dtype) && d0.kh == 1 && a.cout % 8 == 0 && !a.planar;
  for (int s = 0; s < a.n_src; ++s) ok = ok && d0.src[s].c % 64 == 0;
  ok = ok && (!a.ps || (a.n_res == 0 && (a.cout / 4) % 8 == 0));
  for (int g = 0; g < n && ok; ++g) {
    const fcvsr_conv_desc& d = descs[g];
    long long maxsx = d.dst.sx;
    for (int s = 0; s < d.n_src; ++s) maxsx = d.src[s].sx > maxsx ? d.src[s].sx : maxsx;
    ok = d.dst.sc == 1 && (long long)d.B * d.H * d.W * maxsx * 4 < (1ll << 31);
    for (int q = 0; q < d.n_res; ++q) ok = ok && d.res[q].sc == 1 && d.res[q].dtype == FCVSR_F32 && (long long)d.B * d.H * d.W * d.res[q].sx < (1ll << 31);
  }
  return ok;
}

// kRes1PS, given kLean1: pixel-shuffle up-convolution 64 -> cout (<= 256), one 16-bit source, 16-bit destination
bool res1ps_ok(const fcvsr_conv_desc* descs, int n, const MfmaArgs& a) {
  return a.ps && a.src16 && a.dst16 && n == 1 && a.cin_total == 64 && a.cout % 32 == 0 && a.cout <= 256 && strides_mod(descs[0].dst, 8) && aligned16(descs[0].dst.ptr);
}

// kLean3S2: 3x3 stride 2, one dense source of a multiple of 64 channels, cout a multiple of 64, channel-contiguous destination, no residuals
bool lean3s2_ok(const fcvsr_conv_desc* descs, int n, const MfmaArgs& a, int mma_dtype) {
  bool ok = dst_native(descs[0], mma_dtype) && dense3(descs[0], a, 2) && a.cout % 64 == 0 && a.n_res == 0 && a.gc_wmask == nullptr;
  for (int g = 0; g < n && ok; ++g)
    ok = dst_vec16(descs[g].dst, a.dst16) && (long long)descs[g].B * descs[g].H * descs[g].W * descs[g].src[0].sx < (1ll << 29);
  return ok;
}

// Pixel-shuffled 3x3 layers (the up-convs of the full / RGB models, 64 -> 256) on kRes3 without being lean: with sub-pixel-major
// rows a 64-cout block is one sub-pixel, so PixelShuffle is only a different destination pixel (no residuals, 16-bit in and out)
bool res3ps_ok(const fcvsr_conv_desc* descs, const MfmaArgs& a, int mma_dtype) {
  return a.ps && dst_native(descs[0], mma_dtype) && dense3(descs[0], a, 1) && a.cin_total == 64 && a.cout % 256 == 0 && a.n_res == 0 && a.dst16 && a.src16 && a.gc_wmask == nullptr;
}

// kRes3, given kLean3 or res3ps_ok: one dense 16-bit source of 64 or 128 channels, cout a multiple of 64, channel-contiguous
// 16-byte-aligned destination and residuals, no ContextBlock fusion.  *wg_tiles: 8 x 32 tiles x cout blocks of the launch.
bool res3_ok(const fcvsr_conv_desc* descs, int n, const MfmaArgs& a, bool ps, int* wg_tiles) {
  bool ok = a.src16 && conv3_res_supports(a.cin_total, a.cout) && a.gc_wmask == nullptr && a.cout % 64 == 0;
  int tiles = 0;
  for (int g = 0; g < n && ok; ++g) {
    const fcvsr_conv_desc& d = descs[g];
    ok = dst_vec16(d.dst, a.dst16) && strides_mod(d.src[0], 8);
    for (int q = 0; q < d.n_res; ++q) ok = ok && d.res[q].sc == 1 && strides_mod(d.res[q], d.res[q].dtype == FCVSR_F32 ? 4 : 8) && aligned16(d.res[q].ptr);
    tiles += conv3_res_tiles(d.B, d.H, d.W);
    // (destination element offsets are formed in 32-bit arithmetic and widened before the byte scaling: < 2^30 elements keeps
    // every intermediate positive; 16 clips of 720 x 1280 x 64 are 0.94 * 2^30)
    if (ps) ok = ok && d.dst.c == a.cout / 4 && (long long)d.B * d.dst.sb < (1ll << 30) && (long long)d.B * d.src[0].sb < (1ll << 29) &&
                 d.src[0].sc == 1 && aligned16(d.src[0].ptr);
  }
  *wg_tiles = tiles * (a.cin_total == 64 ? a.cout / 64 : a.cout / 32);
  return ok;
}

}  // namespace

int plan_conv2d_mfma(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, ConvPolicy policy, ConvPlan* plan) {
  PLAN_CHECK(descs != nullptr && n_groups >= 1 && n_groups <= 3, "1..3 problem groups");
  PLAN_CHECK(mma_dtype == FCVSR_BF16 || mma_dtype == FCVSR_F16, "mma_dtype must be BF16 or F16");
  const fcvsr_conv_desc& d0 = descs[0];
  PLAN_CHECK(d0.kh == d0.kw && (d0.kh == 1 || d0.kh == 3) && d0.pad == d0.kh / 2 && (d0.stride == 1 || (d0.stride == 2 && d0.kh == 3 && !d0.pixel_shuffle)),
             "MFMA path: 1x1 or 3x3 stride 1, or 3x3 stride 2, same padding");
  PLAN_CHECK(d0.n_src >= 1 && d0.n_src <= 3 && d0.n_res >= 0 && d0.n_res <= 2 && d0.cout > 0, "bad descriptor");
  PLAN_CHECK(d0.weight != nullptr && d0.cout_pad % 128 == 0 && d0.cout_pad >= d0.cout, "weight must be MFMA-packed");
  PLAN_CHECK(!(d0.act == FCVSR_ACT_PRELU) || d0.slope_ptr != nullptr, "PReLU needs slope_ptr");
  PLAN_CHECK(!d0.pixel_shuffle || d0.cout % 16 == 0, "pixel_shuffle needs cout%16==0 (sub-pixel-major packing)");
  MfmaArgs& a = plan->args;
  a.src16 = d0.src[0].dtype != FCVSR_F32;
  a.res16 = (d0.n_res > 0 && d0.res[0].dtype != FCVSR_F32) ? 1 : 0;
  a.sub2 = d0.stride == 2; a.ps = d0.pixel_shuffle; a.flat = d0.kh == 1 ? 1 : 0; a.gc_wmask = d0.gc_wmask; a.gc16 = 0;
  a.planar = (d0.n_src == 1 && d0.src[0].sc != 1) ? 1 : 0;
  PLAN_CHECK(!a.planar || (d0.src[0].dtype == FCVSR_F32 && d0.src[0].c <= 32 && d0.kh == 3),
             "planar (channel-strided) source: one f32 source with <= 32 channels, 3x3");
  a.dst16 = d0.dst.dtype != FCVSR_F32; a.dstbf = d0.dst.dtype == FCVSR_BF16;
  a.n_groups = n_groups; a.n_src = d0.n_src; a.n_res = d0.n_res;
  int cin = 0;
  for (int s = 0; s < 3; ++s) a.seg_c[s] = s < d0.n_src ? d0.src[s].c : (1 << 30);
  for (int s = 0; s < d0.n_src; ++s) cin += d0.src[s].c;
  a.cin_total = cin; a.cin16 = (cin + 15) / 16 * 16;
  a.cin_pad = (cin + 63) / 64 * 64;   // packer pads cin to a multiple of 64 (16-byte weight loads stay in bounds)
  a.cout = d0.cout; a.cout_pad = d0.cout_pad;
  // N tile: measured faster with <= 64 couts per workgroup (register pressure of 128-cout accumulators costs more than
  // re-staging the input tile for the second N-block)
  plan->nt = d0.cout > 32 ? 64 : 32;
  a.n_nblk = (d0.cout + plan->nt - 1) / plan->nt;
  a.w = (const uint16_t*)d0.weight; a.bias = d0.bias;
  a.act = d0.act; a.slope = d0.slope; a.slope_ptr = d0.slope_ptr; a.rs[0] = d0.res_scale[0]; a.rs[1] = d0.res_scale[1];
  PLAN_CHECK(d0.gc_wmask == nullptr || (d0.kh == 3 && d0.stride == 1 && d0.cout <= 64 && !d0.pixel_shuffle && aligned16(d0.gc_wmask)),
             "ContextBlock fusion: 3x3 stride-1 layer with cout <= 64");
  int tiles = 0;
  for (int g = 0; g < n_groups; ++g) {
    const fcvsr_conv_desc& d = descs[g];
    PLAN_CHECK(d.kh == d0.kh && d.kw == d0.kw && d.stride == d0.stride && d.n_src == d0.n_src && d.n_res == d0.n_res && d.cout == d0.cout &&
                   d.weight == d0.weight && d.bias == d0.bias && d.act == d0.act && d.pixel_shuffle == d0.pixel_shuffle,
               "groups must share weights and epilogue");
    PLAN_CHECK(d.B > 0 && d.H > 0 && d.W > 0, "empty problem");
    MGroup& G = a.g[g];
    for (int s = 0; s < d.n_src; ++s) {
      PLAN_CHECK((a.planar ? (d.src[s].ptr != nullptr && d.src[s].sc != 1) : src_ok(d.src[s], mma_dtype)) &&
                     d.src[s].c == d0.src[s].c && d.src[s].dtype == d0.src[0].dtype,
                 "src: f32 or MFMA dtype (all alike), channel-contiguous, 16-byte aligned, c%4==0 (f32) / c%8==0 (16-bit)");
      G.src[s] = to_view(d.src[s]);
      if (a.flat) PLAN_CHECK(d.src[s].sy == d.src[s].sx * d.W && d.src[s].sb == d.src[s].sy * d.H, "1x1 needs uniformly strided pixels");
    }
    for (int q = 0; q < d.n_res; ++q) {
      PLAN_CHECK(d.res[q].ptr && (d.res[q].dtype == FCVSR_F32 || d.res[q].dtype == mma_dtype) && d.res[q].dtype == d0.res[0].dtype && vec_view_ok(d.res[q]),
                 "res must be f32 or the MFMA dtype (all alike), vector-aligned");
      G.res[q] = to_view(d.res[q]);
      if (a.flat) PLAN_CHECK(d.res[q].sy == d.res[q].sx * d.W && d.res[q].sb == d.res[q].sy * d.H, "1x1 needs uniformly strided res");
    }
    PLAN_CHECK(d.dst.ptr && (d.dst.dtype == FCVSR_F32 || d.dst.dtype == FCVSR_BF16 || d.dst.dtype == FCVSR_F16) &&
                   d.dst.dtype == d0.dst.dtype && vec_view_ok(d.dst), "dst must be f32 / bf16 / f16, vector-aligned");
    PLAN_CHECK(d.bias == nullptr || aligned16(d.bias), "bias must be 16-byte aligned");
    G.dst = to_view(d.dst);
    if (a.flat && !d.pixel_shuffle) PLAN_CHECK(d.dst.sy == d.dst.sx * d.W && d.dst.sb == d.dst.sy * d.H, "1x1 needs uniformly strided dst");
    G.gc_partial = d.gc_partial;
    PLAN_CHECK((d.gc_wmask == nullptr) == (d.gc_partial == nullptr) && d.gc_wmask == d0.gc_wmask, "gc fields: all groups alike");
    G.B = d.B; G.H = d.H; G.W = d.W; G.tile_begin = tiles;
    G.tiles_x = a.flat ? 1 : cdiv(d.W, kTW);
    G.tiles_y = a.flat ? 1 : cdiv(d.H, kTH);
    tiles += a.flat ? cdiv((long long)d.B * d.H * d.W, kTH * kTW) : d.B * G.tiles_x * G.tiles_y;
  }
  // the path: the first of the chain whose conditions hold
  const bool lean3 = policy.lean && lean3_ok(descs, n_groups, a, mma_dtype);
  const bool lean1 = policy.lean && lean1_ok(descs, n_groups, a, mma_dtype);
  const bool res3ps = res3ps_ok(descs, a, mma_dtype);
  int wg_tiles = 0;
  ConvPath path = kGeneric;
  if (policy.res && lean1 && res1ps_ok(descs, n_groups, a)) path = kRes1PS;
  else if (policy.lean && lean3s2_ok(descs, n_groups, a, mma_dtype)) path = kLean3S2;
  else if (lean1) path = kLean1;
  else if (policy.res && (lean3 || res3ps) && res3_ok(descs, n_groups, a, res3ps, &wg_tiles) && (policy.res == 1 || wg_tiles >= kResMinTiles))
    path = kRes3;
  else if (lean3) path = kLean3;
  // two layouts only some kernels read: rejected where the policy leaves them to a kernel that cannot
  const bool gc16 = a.gc_wmask != nullptr && a.dst16;
  PLAN_CHECK(!gc16 || (path == kLean3 && a.n_res == 0), "ContextBlock fusion with a 16-bit destination needs the lean 3x3 path, no residuals");
  PLAN_CHECK(!a.res16 || path == kLean3 || path == kRes3, "16-bit residuals are only supported by the lean 3x3 path");
  // path-specific retiling: the plan holds the arguments of the kernel that runs
  if (gc16) a.gc16 = 1, a.dst16 = 0;      // ContextBlock partials come out of the 4-couts-per-lane epilogue: it stores the 16-bit values
  if (path == kLean3S2) {     // tiles are 2 x 32 pixels of the OUTPUT, cout blocks of 64
    a.n_nblk = a.cout / 64;
    tiles = 0;
    for (int g = 0; g < n_groups; ++g) {
      MGroup& G = a.g[g];
      G.tiles_x = cdiv((G.W + 1) / 2, kTW); G.tiles_y = cdiv((G.H + 1) / 2, 2); G.tile_begin = tiles;
      tiles += G.B * G.tiles_x * G.tiles_y;
    }
  }
  for (int g = n_groups; g < 3; ++g) a.g[g] = a.g[0];
  plan->path = path; plan->bf16 = mma_dtype == FCVSR_BF16; plan->total_tiles = tiles;
  return 0;
}

void format_kernel_name(const ConvPlan& p, char* out, size_t cap) {
  const MfmaArgs& a = p.args;
  auto tf = [](int v) { return v ? "true" : "false"; };
  const char* bf = tf(p.bf16);
  switch (p.path) {
    case kGeneric: snprintf(out, cap, "conv_mfma_kernel<%s, %d, %d>", bf, p.nt, a.flat ? 1 : 3); break;
    case kLean3: snprintf(out, cap, "conv3_lean_kernel<%s, %d, %s, %s>%s", bf, p.nt, tf(a.src16), tf(a.dst16), a.gc_wmask ? " +gc" : ""); break;
    case kLean3S2: snprintf(out, cap, "conv3s2_lean_kernel<%s, %s, %s>", bf, tf(a.src16), tf(a.dst16)); break;
    case kLean1: snprintf(out, cap, "conv1_lean_kernel<%s, %d, %s, %s, %s>", bf, p.nt, tf(a.src16), tf(a.dst16), tf(a.ps)); break;
    case kRes1PS: snprintf(out, cap, "conv1ps_res_kernel<%s>", bf); break;
    case kRes3: {
      const ResVariant v = conv3_res_variant(a.cin_total, a.n_res, a.act, a.slope, a.dst16 != 0);
      snprintf(out, cap, "conv3_res_kernel<%s, %d, %d, %d>", bf, v.mode, v.nch, v.nsu);
    }
  }
}

}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_conv2d_mfma_plan(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, int lean, int res, char* kernel_name, int cap) {
  FCVSR_CHECK_ARG(kernel_name != nullptr && cap > 0 && (lean == 0 || lean == 1) && res >= 0 && res <= 2, "lean 0/1, res 0/1/2, a name buffer");
  ConvPlan plan;
  const int rc = plan_conv2d_mfma(descs, n_groups, mma_dtype, ConvPolicy{lean, res}, &plan);
  if (rc == 0) format_kernel_name(plan, kernel_name, (size_t)cap);
  return rc;
}
