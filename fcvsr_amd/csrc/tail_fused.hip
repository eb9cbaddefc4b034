// Fused end of the up-sampler of GShiftNet_S (reference CVSR_freq.py:2605-2607, :2642-2645):
//     out += conv_last0( PReLU( PixelShuffle2( upconv2(u1) ) ) )          upconv2: 1x1, 64 -> 256; conv_last0: 3x3, 64 -> 1
// The 64-channel tensor at the output resolution (B x 4H x 4W x 64: the largest activation of the whole path, 118 MB per
// clip in 16-bit) is never written.  One workgroup produces an 8 x 32 tile of output pixels:
//   1. GEMM 1 (v_mfma 32x32x16): wave w owns sub-pixel (sy, sx) = (w >> 1, w & 1), i.e. rows w*64 .. w*64+63 of the
//      sub-pixel-major packing, so PixelShuffle is just the LDS address the result is written to.  Of the 6 x 18 pixels of u1
//      under the tile's 10 x 34 halo a sub-pixel lands inside the halo for 5 x 17 only (sy = 0 misses it from u1 row 0, sy = 1
//      from row 5; columns 0 / 17 likewise with sx), so each wave multiplies its own 5 x 17 = 85 live pixels (three 32-pixel
//      fragments; 4 x 85 = 340: every halo position is produced exactly once) by its 64 x 64 weight block.  Bias, PReLU, zero
//      padding outside the image and the rounding to the MFMA dtype (what the stand-alone layer would have stored) happen on
//      the way.  A u2 value is the chain of the same four MFMAs over the same 16-channel steps for the same weight rows and
//      the same pixel, whichever column of whichever fragment the pixel sits in, and bias, PReLU and rounding are per value:
//      the result has the bits of a GEMM over all 108 pixels.
//   2. GEMM 2 (v_mfma 16x16x32): conv_last0 as "taps are output columns": P[pixel][tap] = sum_c u2[pixel][c] * w[tap][c] for
//      the 340 halo pixels - 44 small MFMAs instead of 576 multiply-adds per output pixel on the vector ALU.
//   3. out[y][x] += bias + sum_tap P[y+dy][x+dx][tap]   (out holds the bilinear x4 base skip).
// HBM traffic per output pixel: 14 bytes of u1 (with halo) + 8 bytes of out, instead of 128 written + ~170 read.
// BASE != 0 (fcvsr_tail_fused_base, _base_u8): the base skip is not read from `out` but evaluated for the thread's pixel from the
// centre LR frame (bilinear.h: four cached loads from a 230 KB frame; BASE == 2: a uint8 frame, BASE == 3: a frame of 10-bit samples
// in uint16, both read through the table of u8.h), so the result is write-only and no kernel has to pre-fill an f32 base.
// Q != 0 (fcvsr_tail_fused_u8, _u16): `out` is only read (the f32 base) and the sum goes, quantised to PEAK (u8.h), to the integer
// frame out8 (uint8 for PEAK = 255, uint16 for PEAK = 1023).
#include "common.h"
#include "mfma_util.h"
#include "bilinear.h"
#include "u8.h"
#include <type_traits>

namespace fcvsr {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int kTfTH = 8, kTfTW = 32;                       // output tile: one thread per output pixel
constexpr int kTfHH = kTfTH + 2, kTfHW = kTfTW + 2;        // halo of the 3x3 convolution (output resolution)
constexpr int kTfNHP = kTfHH * kTfHW;                      // 340
constexpr int kTfUH = kTfTH / 2 + 2, kTfUW = kTfTW / 2 + 2;   // 6 x 18 pixels of u1
constexpr int kTfLH = kTfUH - 1, kTfLW = kTfUW - 1;        // 5 x 17 of them put a given sub-pixel inside the halo: a wave's live pixels
constexpr int kTfNL = kTfLH * kTfLW;                       // 85
constexpr int kTfNF = (kTfNL + 31) / 32;                   // 32-pixel fragments of GEMM 1: 3 (the last one holds 21 pixels)
static_assert(4 * kTfNL == kTfNHP, "the four sub-pixels' live pixels cover the halo exactly once");
static_assert(kTfTH * kTfTW == 256, "one thread per output pixel");
constexpr int kTfRow = 64 + 8;                             // halfwords per halo pixel in LDS (padded: conflict-free fragments)
constexpr int kTfPRow = 9;                                 // floats per pixel of the tap table (odd stride)
constexpr int kTfNPT = (kTfNHP + 15) / 16;                 // 22 pixel tiles of GEMM 2

struct TailArgs {
  View u1;                 // (B, H2, W2, 64), 16-bit
  const uint16_t* w2;      // [256][64] upconv2, rows sub-pixel-major ((2i+j)*64 + c), MFMA dtype
  const float* b2;         // [256] bias in the same row order (may be null)
  const float* slope;      // PReLU slope (one shared scalar, :2609)
  const uint16_t* wl;      // [16][64] conv_last0: row = tap (ky*3+kx), rows 9..15 zero
  const float* bl;         // conv_last0 bias (1 value, may be null)
  View out;                // (B, 2*H2, 2*W2, 1) f32, read-modify-write (Q != 0: read only)
  View out8;               // Q != 0: (B, 2*H2, 2*W2, 1) uint8 / uint16 destination
  View centre;             // BASE: (B, H2/2, W2/2, 1) centre LR frame (source of the bilinear x4 base skip): f32, uint8 (BASE == 2) or
                           // uint16 (BASE == 3)
  const float* tab;        // BASE >= 2: the table of the integer entry points (256 or 1024 floats)
  int B, H2, W2, tiles_x, tiles_y;
  int ntiles;              // B * tiles_x * tiles_y, split into contiguous runs over the launched workgroups
};

template <bool BF16>
__device__ __forceinline__ f32x4_t mfma16(uint4 a, uint4 b, f32x4_t c) {
  if (BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

template <bool BF16, int Q = 0, int BASE = 0, int PEAK = kPeak8>
__global__ __launch_bounds__(256, 3) void tail_fused_kernel(TailArgs a) {
  static_assert(BASE >= 0 && BASE <= 3, "BASE - 1 is the centre frame's format (kSrcF32, kSrcU8, kSrcU16)");
  // 48 KiB: the tap table P of step 2 overwrites the u2 tile it was computed from (3 workgroups per CU)
  __shared__ __align__(16) uint16_t u2_s[kTfNHP * kTfRow];
  float* p_s = reinterpret_cast<float*>(u2_s);
  static_assert(kTfNPT * 16 * kTfPRow * 4 <= kTfNHP * kTfRow * 2, "tap table must fit into the u2 tile");
  __shared__ __align__(16) float b2_s[256];
  // Tile runs: a workgroup (three per CU) walks a contiguous run of tiles with its wave's 64 x 64 block of upconv2 weights in
  // registers and the bias in LDS for the whole run.  One tile per workgroup re-read the 32 KB weight block from L2 for every
  // 256 output pixels: 128 bytes per output pixel, six times the 22 bytes the pixel itself moves.
  int t_begin, t_end;
  {                                                        // contiguous runs of tiles per XCD (halo rows of u1 hit its L2)
    const int g = blockIdx.x, nwg = gridDim.x, q = nwg >> 3, rr = nwg & 7, xcd = g & 7, loc = g >> 3;
    const int ci = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc;
    t_begin = (int)((long long)ci * a.ntiles / nwg);
    t_end = (int)((long long)(ci + 1) * a.ntiles / nwg);
  }
  uint4 wf[2][4], wl0, wl1;
  {
    const int tid0 = threadIdx.x, lane0 = tid0 & 63, wave0 = tid0 >> 6, r0 = lane0 & 31, h0 = lane0 >> 5;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint16_t* wp = a.w2 + ((wave0 * 2 + q) * 32 + r0) * 64 + h0 * 8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) wf[q][kk] = *reinterpret_cast<const uint4*>(wp + kk * 16);
    }
    wl0 = *reinterpret_cast<const uint4*>(a.wl + (lane0 & 15) * 64 + (lane0 >> 4) * 8);
    wl1 = *reinterpret_cast<const uint4*>(a.wl + (lane0 & 15) * 64 + (lane0 >> 4) * 8 + 32);
    b2_s[tid0] = a.b2 ? a.b2[tid0] : 0.f;
  }
  const float slope = a.slope[0];
  // PReLU(x) = max(x, slope*x) whenever 0 <= slope <= 1 (one multiply and one max per value; x >= 0: slope*x <= x, x < 0:
  // slope*x >= x, and slope*x is the product the generic form rounds).  Wave-uniform; any other slope takes the generic form.
  const bool slope01 = slope >= 0.f && slope <= 1.f;
  const float blast = a.bl ? a.bl[0] : 0.f;
  const int per_img = a.tiles_x * a.tiles_y;
  const int HH = 2 * a.H2, WW = 2 * a.W2;
  __syncthreads();
  // The wave's live pixels: p in [0, 85) is u1 pixel uy = (1 - sy) + p / 17, ux = (1 - sx) + p % 17 of the 6 x 18 under the tile,
  // and its sub-pixel (sy, sx) is halo position hr = 2 uy + sy - 1 in [0, 10), hc = 2 ux + sx - 1 in [0, 34).
  // u2_off: where lane r of fragment nt stores that value inside the 10 x 34 halo (halfwords; -1: one of the 11 surplus slots of
  // the last fragment): the same for every tile
  int u2_off[kTfNF];
#pragma unroll
  for (int nt = 0; nt < kTfNF; ++nt) {
    const int p = nt * 32 + (threadIdx.x & 31);
    const int sy = threadIdx.x >> 7, sx = (threadIdx.x >> 6) & 1;
    const int py = p / kTfLW;
    const int uy = 1 - sy + py, ux = 1 - sx + (p - py * kTfLW);
    const int hr = 2 * uy + sy - 1, hc = 2 * ux + sx - 1;
    u2_off[nt] = p < kTfNL ? (hr * kTfHW + hc) * kTfRow + 4 * (int)((threadIdx.x >> 5) & 1) : -1;
  }
  // the slope is the same for every tile: the whole tile loop exists once per PReLU form
  auto run_tiles = [&](auto s01_c) {
  constexpr bool S01 = decltype(s01_c)::value;
#pragma unroll 1
  for (int t = t_begin; t < t_end; ++t) {
  // lane-derived offsets are recomputed per tile: hoisted out of the loop they cost registers the tile body has no room for
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  const int b = t / per_img;
  const int t2 = t - b * per_img;
  const int Y0 = (t2 / a.tiles_x) * kTfTH, X0 = (t2 % a.tiles_x) * kTfTW;
  // this thread's output pixel.  BASE == 0: its current value (the base skip) is requested now and consumed at the very end;
  // the f32 tensor `out` exists only where it is read (BASE == 0) or written (Q == 0)
  const int oy = Y0 + (tid >> 5), ox = X0 + (tid & 31);
  const bool olive = oy < HH && ox < WW;
  float* op = nullptr;
  if constexpr (BASE == 0 || Q == 0)
    op = a.out.p + (long long)b * a.out.sb + (long long)(olive ? oy : 0) * a.out.sy + (long long)(olive ? ox : 0) * a.out.sx;
  float base = 0.f;
  if constexpr (BASE == 0) base = *op;

  // ---- GEMM 1: u2 = PReLU(W2 . u1 + b2), wave = sub-pixel -----------------------------------------------------------------
  {
    const int r = lane & 31, h = lane >> 5;
    const uint16_t* ub = reinterpret_cast<const uint16_t*>(a.u1.p) + (long long)b * a.u1.sb + h * 8;
    const int sy = wave >> 1, sx = wave & 1;                // this wave's sub-pixel
    uint4 kf[kTfNF][4];
#pragma unroll
    for (int nt = 0; nt < kTfNF; ++nt) {
      int p = nt * 32 + r;
      p = p < kTfNL ? p : kTfNL - 1;                         // surplus slots load a valid pixel and are never stored
      const int py = p / kTfLW;
      const int uy = 1 - sy + py, ux = 1 - sx + (p - py * kTfLW);
      int gy = (Y0 >> 1) - 1 + uy, gx = (X0 >> 1) - 1 + ux;
      gy = gy < 0 ? 0 : (gy > a.H2 - 1 ? a.H2 - 1 : gy);    // clamped pixels only feed halo positions outside the image,
      gx = gx < 0 ? 0 : (gx > a.W2 - 1 ? a.W2 - 1 : gx);    // which are stored as zeros below
      const uint16_t* up = ub + (long long)gy * a.u1.sy + (long long)gx * a.u1.sx;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) kf[nt][kk] = *reinterpret_cast<const uint4*>(up + kk * 16);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float4 bq[4];
#pragma unroll
      for (int g = 0; g < 4; ++g)
        bq[g] = *reinterpret_cast<const float4*>(b2_s + wave * 64 + q * 32 + 8 * g + 4 * h);
#pragma unroll
      for (int nt = 0; nt < kTfNF; ++nt) {
        f32x16_t acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = mfma<BF16>(wf[q][kk], kf[nt][kk], acc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = q * 32 + 8 * g;                      // acc[4g..4g+3] = channels c + 4h .. c + 4h + 3 of sub-pixel `wave`
          // the bias is added last (products first, as the stand-alone layer stores them): as the MFMA's C operand it would be
          // rounded into every partial sum and change the f32 result
          float4 v = make_float4(acc[4 * g] + bq[g].x, acc[4 * g + 1] + bq[g].y, acc[4 * g + 2] + bq[g].z, acc[4 * g + 3] + bq[g].w);
          if constexpr (S01) {
            v.x = fmaxf(v.x, slope * v.x); v.y = fmaxf(v.y, slope * v.y);
            v.z = fmaxf(v.z, slope * v.z); v.w = fmaxf(v.w, slope * v.w);
          } else {
            // PReLU as max(x,0) + slope*min(x,0): the same values as the select form
            v.x = fmaf(slope, fminf(v.x, 0.f), fmaxf(v.x, 0.f)); v.y = fmaf(slope, fminf(v.y, 0.f), fmaxf(v.y, 0.f));
            v.z = fmaf(slope, fminf(v.z, 0.f), fmaxf(v.z, 0.f)); v.w = fmaf(slope, fminf(v.w, 0.f), fmaxf(v.w, 0.f));
          }
          if (u2_off[nt] >= 0) *reinterpret_cast<uint2*>(u2_s + u2_off[nt] + c) = cvt4<BF16>(v);
        }
      }
    }
    // zero padding of conv_last0, only in tiles whose 10 x 34 halo leaves the image (7 % of them at 720 x 1280; a uniform
    // branch): every lane overwrites the positions outside the image that it has just stored (same lane, same addresses: in order)
    if (Y0 < 1 || Y0 + kTfTH + 1 > HH || X0 < 1 || X0 + kTfTW + 1 > WW) {
#pragma unroll 1
      for (int nt = 0; nt < kTfNF; ++nt) {
        const int p = nt * 32 + r;
        const int py = p / kTfLW;
        const int uy = 1 - sy + py, ux = 1 - sx + (p - py * kTfLW);
        const int hr = 2 * uy + sy - 1, hc = 2 * ux + sx - 1;
        const int Y = Y0 - 1 + hr, X = X0 - 1 + hc;
        const bool inside = Y >= 0 && Y < HH && X >= 0 && X < WW;
        if (p < kTfNL && !inside) {
#pragma unroll
          for (int c8 = 0; c8 < 8; ++c8)
            *reinterpret_cast<uint2*>(u2_s + (hr * kTfHW + hc) * kTfRow + 8 * c8 + 4 * h) = make_uint2(0u, 0u);
        }
      }
    }
  }
  // the base skip's four source values are requested now (the fragment registers of GEMM 1 are free) and blended at the very end
  BilinearTaps taps = {};
  if constexpr (BASE != 0)
    taps = bilinear_up4_fetch<BASE - 1>(a.centre, a.tab, a.H2 >> 1, a.W2 >> 1, b, 0, olive ? oy : 0, olive ? ox : 0);
  __syncthreads();

  // ---- GEMM 2: P[pixel][tap] = u2[pixel][:] . wl[tap][:] ---------------------------------------------------------------------
  {
    const int r16 = lane & 15, g4 = lane >> 4;
    f32x4_t pacc[(kTfNPT + 3) / 4];
#pragma unroll
    for (int j = 0; j < (kTfNPT + 3) / 4; ++j) {
      const int pt = wave + 4 * j;
      int px = pt * 16 + r16;
      px = px < kTfNHP ? px : kTfNHP - 1;
      const uint4 a0 = *reinterpret_cast<const uint4*>(u2_s + px * kTfRow + g4 * 8);
      const uint4 a1 = *reinterpret_cast<const uint4*>(u2_s + px * kTfRow + g4 * 8 + 32);
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      acc = mfma16<BF16>(a0, wl0, acc);
      pacc[j] = mfma16<BF16>(a1, wl1, acc);
    }
    __syncthreads();                                       // every wave has read its u2 pixels: the tile may be overwritten
    // D[row][col]: col = lane & 15 (tap), row = 4 * (lane >> 4) + i (pixel within the 16-pixel tile)
#pragma unroll
    for (int j = 0; j < (kTfNPT + 3) / 4; ++j) {
      const int pt = wave + 4 * j;
      if (pt < kTfNPT && r16 < 9) {
#pragma unroll
        for (int i = 0; i < 4; ++i) p_s[(pt * 16 + 4 * g4 + i) * kTfPRow + r16] = pacc[j][i];
      }
    }
  }
  __syncthreads();

  // ---- out += bias + sum over the 9 taps ---------------------------------------------------------------------------------------
  {
    const int ty = tid >> 5, tx = tid & 31;
    if (olive) {
      if constexpr (BASE != 0) base = bilinear_up4_blend(taps);
      float s = base + blast;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) s += p_s[((ty + dy) * kTfHW + tx + dx) * kTfPRow + dy * 3 + dx];
      if constexpr (Q == 0) {
        *op = s;
      } else {
        typedef typename SampleOf<PEAK>::type OT;
        reinterpret_cast<OT*>(a.out8.p)[(long long)b * a.out8.sb + (long long)oy * a.out8.sy + (long long)ox * a.out8.sx] =
            quantise<Q, PEAK, OT>(s);
      }
    }
  }
  __syncthreads();                                         // the tap table is read: the next tile's u2 overwrites it
  }
  };
  if (slope01) run_tiles(std::true_type{});
  else run_tiles(std::false_type{});
}

}  // namespace fcvsr

using namespace fcvsr;

template <int Q, int BASE = 0, int PEAK = kPeak8>
static int tail_fused_launch(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl, const float* bl,
                             int B, int H2, int W2, const fcvsr_view* out, const fcvsr_view* out8, void* stream,
                             const fcvsr_view* centre = nullptr, const float* tab = nullptr) {
  if (Q != 0 && BASE != 0) out = out8;                     // no f32 tensor at all: `out` is neither read nor written
  FCVSR_CHECK_ARG(u1 && u1->ptr && w2 && slope && wl && out && out->ptr, "null argument");
  FCVSR_CHECK_ARG((u1->dtype == FCVSR_BF16 || u1->dtype == FCVSR_F16) && u1->c == 64 && u1->sc == 1 &&
                      ((uintptr_t)u1->ptr % 16) == 0 && u1->sx % 8 == 0 && u1->sy % 8 == 0 && u1->sb % 8 == 0,
                  "u1: 64 contiguous 16-bit channels, 16-byte aligned");
  FCVSR_CHECK_ARG((out->dtype == FCVSR_F32 || out == out8) && out->c == 1, "out: one f32 channel");
  FCVSR_CHECK_ARG(((uintptr_t)w2 % 16) == 0 && ((uintptr_t)wl % 16) == 0 && (b2 == nullptr || ((uintptr_t)b2 % 16) == 0),
                  "weights / bias must be 16-byte aligned");
  FCVSR_CHECK_ARG(B > 0 && H2 > 0 && W2 > 0, "bad sizes");
  TailArgs a;
  a.u1 = to_view(*u1); a.w2 = (const uint16_t*)w2; a.b2 = b2; a.slope = slope; a.wl = (const uint16_t*)wl; a.bl = bl;
  a.out = to_view(*out); a.B = B; a.H2 = H2; a.W2 = W2;
  a.out8 = out8 ? to_view(*out8) : a.out;
  a.centre = a.out;
  a.tab = tab;
  if (BASE != 0) {
    FCVSR_CHECK_ARG(centre && centre->ptr && centre->c == 1 &&
                        centre->dtype == (BASE == 3 ? FCVSR_U16 : BASE == 2 ? FCVSR_U8 : FCVSR_F32),
                    "centre: one channel, f32 (uint8 for the _u8 entry point, uint16 for _u16)");
    FCVSR_CHECK_ARG(BASE < 2 || tab, "integer centre frame needs the table");
    FCVSR_CHECK_ARG(BASE != 3 || ((uintptr_t)centre->ptr % 2) == 0, "uint16 centre frame: 2-byte aligned");
    FCVSR_CHECK_ARG(H2 % 2 == 0 && W2 % 2 == 0, "u1 is the x2 level of the centre frame: H2, W2 even");
    a.centre = to_view(*centre);
  }
  a.tiles_x = cdiv(2 * W2, kTfTW);
  a.tiles_y = cdiv(2 * H2, kTfTH);
  a.ntiles = B * a.tiles_x * a.tiles_y;
  static int wgs[64] = {0};                                // three workgroups per CU (set by the 48 KB of LDS; 142-150 registers)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!wgs[dev]) {
    hipDeviceProp_t prop;
    wgs[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? 3 * prop.multiProcessorCount : 768;
  }
  int nwg = wgs[dev];
  nwg = nwg < 8 ? 8 : nwg / 8 * 8;
  dim3 grid(nwg < a.ntiles ? nwg : a.ntiles);
  hipStream_t st = (hipStream_t)stream;
  if (u1->dtype == FCVSR_BF16) hipLaunchKernelGGL((tail_fused_kernel<true, Q, BASE, PEAK>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((tail_fused_kernel<false, Q, BASE, PEAK>), grid, dim3(256), 0, st, a);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_tail_fused(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                const float* bl, int B, int H2, int W2, const fcvsr_view* out, void* stream) {
  return tail_fused_launch<0>(u1, w2, b2, slope, wl, bl, B, H2, W2, out, nullptr, stream);
}

extern "C" int fcvsr_tail_fused_base(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                     const float* bl, const fcvsr_view* centre, int B, int H2, int W2, const fcvsr_view* out,
                                     void* stream) {
  return tail_fused_launch<0, 1>(u1, w2, b2, slope, wl, bl, B, H2, W2, out, nullptr, stream, centre);
}

extern "C" int fcvsr_tail_fused_base_u8(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                        const float* bl, const fcvsr_view* centre, const float* tab, int B, int H2, int W2,
                                        const fcvsr_view* out, int quantise, void* stream) {
  FCVSR_CHECK_ARG(out && out->ptr && out->dtype == FCVSR_U8 && out->c == 1, "out: one uint8 channel");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  if (quantise == FCVSR_QUANT_TRUNCATE)
    return tail_fused_launch<FCVSR_QUANT_TRUNCATE, 2>(u1, w2, b2, slope, wl, bl, B, H2, W2, nullptr, out, stream, centre, tab);
  return tail_fused_launch<FCVSR_QUANT_ROUND, 2>(u1, w2, b2, slope, wl, bl, B, H2, W2, nullptr, out, stream, centre, tab);
}

extern "C" int fcvsr_tail_fused_u8(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                   const float* bl, int B, int H2, int W2, const fcvsr_view* base, const fcvsr_view* out, int quantise,
                                   void* stream) {
  FCVSR_CHECK_ARG(out && out->ptr && out->dtype == FCVSR_U8 && out->c == 1, "out: one uint8 channel");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  if (quantise == FCVSR_QUANT_TRUNCATE)
    return tail_fused_launch<FCVSR_QUANT_TRUNCATE>(u1, w2, b2, slope, wl, bl, B, H2, W2, base, out, stream);
  return tail_fused_launch<FCVSR_QUANT_ROUND>(u1, w2, b2, slope, wl, bl, B, H2, W2, base, out, stream);
}

extern "C" int fcvsr_tail_fused_base_u16(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                         const float* bl, const fcvsr_view* centre, const float* tab, int B, int H2, int W2,
                                         const fcvsr_view* out, int quantise, void* stream) {
  FCVSR_CHECK_ARG(out && out->ptr && out->dtype == FCVSR_U16 && out->c == 1 && ((uintptr_t)out->ptr % 2) == 0,
                  "out: one uint16 channel, 2-byte aligned");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  if (quantise == FCVSR_QUANT_TRUNCATE)
    return tail_fused_launch<FCVSR_QUANT_TRUNCATE, 3, kPeak10>(u1, w2, b2, slope, wl, bl, B, H2, W2, nullptr, out, stream, centre, tab);
  return tail_fused_launch<FCVSR_QUANT_ROUND, 3, kPeak10>(u1, w2, b2, slope, wl, bl, B, H2, W2, nullptr, out, stream, centre, tab);
}

extern "C" int fcvsr_tail_fused_u16(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                                    const float* bl, int B, int H2, int W2, const fcvsr_view* base, const fcvsr_view* out, int quantise,
                                    void* stream) {
  FCVSR_CHECK_ARG(out && out->ptr && out->dtype == FCVSR_U16 && out->c == 1 && ((uintptr_t)out->ptr % 2) == 0,
                  "out: one uint16 channel, 2-byte aligned");
  FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  if (quantise == FCVSR_QUANT_TRUNCATE)
    return tail_fused_launch<FCVSR_QUANT_TRUNCATE, 0, kPeak10>(u1, w2, b2, slope, wl, bl, B, H2, W2, base, out, stream);
  return tail_fused_launch<FCVSR_QUANT_ROUND, 0, kPeak10>(u1, w2, b2, slope, wl, bl, B, H2, W2, base, out, stream);
}
