// Tiled inference (specification: fcvsr_amd/harness/tiles.py): the model runs on overlapping tiles of the frame and the tile outputs
// are blended with separable feathered weights.  All geometry is in LR pixels on the frame zero-padded at its bottom / right to
// multiples of 4 (Hp x Wp); every tile of a frame has one shape th x tw (multiples of 4, th <= Hp, tw <= Wp), tile (ky, kx) starts at
// (ys[ky], xs[kx]).  The start tables are DEVICE memory: a start outside [0, Hp - th] / [0, Wp - tw] is clamped into it, so no table
// content can move an access out of its buffer.
//
// tile_windows_kernel: all tile windows (b,ny,nx,T,C,th,tw) f32 of a batch of windows in one launch, straight from the resident
// UNPADDED sequence (N,C,h,w) (f32, uint8 or uint16 samples read through the format's table, u8.h) through the device index table
// (b,T): the plain full-frame windows are never materialised.  One workgroup makes one 64 x 64 block of one output plane, a thread 4
// neighbouring samples in 4 rows: the samples are read with en_load4 (window_load.h: integer samples out of aligned dwords, so no
// load touches memory beyond the pages of the sequence), all of a thread's loads in flight before the first store, and leave as one
// 16-byte store, zeros where the padding is: every output element is stored exactly once.  Nothing is transposed: no LDS.
//
// tile_merge_kernel: crop, weighted fixed-order blend and quantisation of the tile outputs (b,ny,nx,C,4th,4tw) in one launch.  wy
// (ny,4Hp) and wx (nx,4Wp) are the normalised per-axis f32 weights the host made (0 where a tile does not reach).  For an output
// pixel (Y, X), in f32:
//   acc = 0;  for ky ascending, then kx ascending over the tiles that cover it:  acc = acc + (wy[ky][Y] * wx[kx][X]) * v
// each of the three operations rounded once (-ffp-contract=off), v the tile's value at (Y - 4 ys[ky], X - 4 xs[kx]).  One workgroup
// makes one 64 x 64 block of one output plane (4h x 4w), a thread 4 neighbouring pixels in 4 rows.  A tile starts at a whole LR
// pixel, i.e. at a multiple of 4 SR pixels, and is a multiple of 16 SR pixels wide: a thread's 4 pixels are covered by the same
// tiles, and they are one aligned float4 of every tile row and of wx.  The covering tiles of an axis are a contiguous index range
// (at most 3 tiles on a pixel for the grids of the specification); the block's range is found by a uniform
// scan of the start table and a thread tests its own rows / columns inside it.  The result leaves as 4 floats (16 bytes), or
// quantised (u8.h) as 4 uint16 (8 bytes) / 4 uint8 (4 bytes), as ensemble_merge_kernel's does.  No LDS.
#include "common.h"
#include "u8.h"
#include "window_load.h"

namespace fcvsr {

__device__ __forceinline__ int tile_start(const int32_t* starts, int k, int last) { return min(max(starts[k], 0), last); }

template <int SRC>
__global__ __launch_bounds__(EN_THREADS) void tile_windows_kernel(const void* src, const float* tab, const int32_t* idx, int N, int C,
                                                                  int h, int w, int T, const int32_t* ys, int ny, const int32_t* xs,
                                                                  int nx, int th, int tw, int blocks_x, int blocks, float* out) {
  // plane p of the output: ((bi * ny + ky) * nx + kx) * T + ti) * C + c
  const int p = blockIdx.x / blocks, t = blockIdx.x % blocks;
  const int c = p % C, ti = (p / C) % T;
  const int k = p / (C * T);                                                // (bi * ny + ky) * nx + kx
  const int kx = k % nx, ky = (k / nx) % ny, bi = k / (nx * ny);
  const int ay = tile_start(ys, ky, ceil4(h) - th), ax = tile_start(xs, kx, ceil4(w) - tw);
  const int n = min(max(idx[bi * T + ti], 0), N - 1);
  const long long plane = ((long long)n * C + c) * h * w;
  const int oy0 = (t / blocks_x) * EN_TILE, ox0 = (t % blocks_x) * EN_TILE; // the block's corner in the tile plane
  const int x = ox0 + (threadIdx.x % EN_LANES) * 4;                         // this thread's 4 columns of the tile plane
  const int y0 = oy0 + threadIdx.x / EN_LANES;
  const int nv = min(4, w - (ax + x));                                      // its samples inside the frame: <= 0 in the padding
  float v[EN_PASSES][4];
#pragma unroll
  for (int q = 0; q < EN_PASSES; ++q) {                                     // all loads of the thread in flight before the first store
    const int y = y0 + q * EN_ROWS;
    const bool live = y < th && x < tw && ay + y < h && nv > 0;             // a thread with nothing to read re-reads the plane's first sample
    en_load4<SRC>(src, plane + (live ? (long long)(ay + y) * w + ax + x : 0), live ? nv : 1, tab, v[q]);
  }
  float* dst = out + (long long)p * th * tw;
#pragma unroll
  for (int q = 0; q < EN_PASSES; ++q) {
    const int y = y0 + q * EN_ROWS;
    if (y < th && x < tw) {
      const int m = ay + y < h ? nv : 0;
      *reinterpret_cast<float4*>(dst + (long long)y * tw + x) =
          make_float4(0 < m ? v[q][0] : 0.f, 1 < m ? v[q][1] : 0.f, 2 < m ? v[q][2] : 0.f, 3 < m ? v[q][3] : 0.f);
    }
  }
}

// O = float: the f32 blend; uint8_t / uint16_t: quantised with mode Q at peak PEAK
template <class O, int PEAK, int Q>
__global__ __launch_bounds__(EN_THREADS) void tile_merge_kernel(const float* tiles, const int32_t* ys, int ny, const int32_t* xs, int nx,
                                                                int th, int tw, const float* wy, const float* wx, int C, int h, int w,
                                                                int blocks_x, int blocks, O* out) {
  const int H4 = 4 * h, W4 = 4 * w;
  const int Hp = ceil4(h), Wp = ceil4(w);
  const int TH = 4 * th, TW = 4 * tw;                                       // a tile output plane
  const int p = blockIdx.x / blocks, t = blockIdx.x % blocks;               // p = bi * C + c
  const int bi = p / C, c = p % C;
  const int Y0 = (t / blocks_x) * EN_TILE, X0 = (t % blocks_x) * EN_TILE;
  const int bh = min(EN_TILE, H4 - Y0), bw = min(EN_TILE, W4 - X0);         // multiples of 4
  const int x = (threadIdx.x % EN_LANES) * 4, y0 = threadIdx.x / EN_LANES;
  const int X = X0 + x;
  // the tiles that touch the block: a contiguous range per axis, the same for every thread
  int ky0 = ny, ky1 = -1, kx0 = nx, kx1 = -1;
  for (int k = 0; k < ny; ++k) {
    const int a = 4 * tile_start(ys, k, Hp - th);
    if (a < Y0 + bh && a + TH > Y0) { ky0 = min(ky0, k); ky1 = max(ky1, k); }
  }
  for (int k = 0; k < nx; ++k) {
    const int a = 4 * tile_start(xs, k, Wp - tw);
    if (a < X0 + bw && a + TW > X0) { kx0 = min(kx0, k); kx1 = max(kx1, k); }
  }
  float acc[EN_PASSES][4];
#pragma unroll
  for (int q = 0; q < EN_PASSES; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[q][e] = 0.f;
  if (x < bw) {
    for (int ky = ky0; ky <= ky1; ++ky) {
      const int ay = 4 * tile_start(ys, ky, Hp - th);
      for (int kx = kx0; kx <= kx1; ++kx) {
        const int ax = 4 * tile_start(xs, kx, Wp - tw);
        if (X < ax || X >= ax + TW) continue;                               // X and ax are multiples of 4: all 4 pixels or none
        const float4 gx = *reinterpret_cast<const float4*>(wx + (long long)kx * 4 * Wp + X);
        const float* src = tiles + ((((long long)bi * ny + ky) * nx + kx) * C + c) * TH * TW + (X - ax);
        float4 v[EN_PASSES];
        float gy[EN_PASSES];
        bool on[EN_PASSES];
#pragma unroll
        for (int q = 0; q < EN_PASSES; ++q) {                               // the 4 rows' loads in flight together
          const int Y = Y0 + y0 + q * EN_ROWS;
          on[q] = y0 + q * EN_ROWS < bh && Y >= ay && Y < ay + TH;
          const int ly = on[q] ? Y - ay : 0;
          v[q] = *reinterpret_cast<const float4*>(src + (long long)ly * TW);
          gy[q] = wy[(long long)ky * 4 * Hp + (on[q] ? Y : 0)];
        }
#pragma unroll
        for (int q = 0; q < EN_PASSES; ++q) {
          if (on[q]) {
            acc[q][0] = acc[q][0] + (gy[q] * gx.x) * v[q].x;
            acc[q][1] = acc[q][1] + (gy[q] * gx.y) * v[q].y;
            acc[q][2] = acc[q][2] + (gy[q] * gx.z) * v[q].z;
            acc[q][3] = acc[q][3] + (gy[q] * gx.w) * v[q].w;
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < EN_PASSES; ++q) {
    const int y = y0 + q * EN_ROWS;
    if (y < bh && x < bw) {
      O* dp = out + ((long long)p * H4 + Y0 + y) * W4 + X;
      if constexpr (sizeof(O) == 4) {
        *reinterpret_cast<float4*>(dp) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
      } else {
        O o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = quantise<Q, PEAK, O>(acc[q][e]);
        if constexpr (sizeof(O) == 1) *reinterpret_cast<uchar4*>(dp) = make_uchar4(o[0], o[1], o[2], o[3]);
        else *reinterpret_cast<ushort4*>(dp) = make_ushort4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

}  // namespace fcvsr

using namespace fcvsr;

constexpr int kTileMaxSide = 1 << 24;                                        // keeps 4 * ceil4(side) and every block count in an int

#define FCVSR_TILE_GRID_CHECKS()                                                                                          \
  FCVSR_CHECK_ARG(h > 0 && w > 0 && h <= kTileMaxSide && w <= kTileMaxSide, "frame: sides in 1 .. 2^24");                  \
  FCVSR_CHECK_ARG(ny > 0 && nx > 0 && ny <= kTileMaxSide && nx <= kTileMaxSide, "ny, nx: positive");                      \
  FCVSR_CHECK_ARG(th > 0 && tw > 0 && th % 4 == 0 && tw % 4 == 0, "th, tw: positive multiples of 4");                     \
  FCVSR_CHECK_ARG(th <= ceil4(h) && tw <= ceil4(w), "th, tw: at most the padded frame");                                   \
  FCVSR_CHECK_ARG(ys && xs && ((uintptr_t)ys % 4) == 0 && ((uintptr_t)xs % 4) == 0, "ys, xs: non-null, 4-byte aligned")

template <int SRC>
static int tile_windows_launch(const void* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                               const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, float* out, void* stream) {
  FCVSR_CHECK_ARG(src && idx && out && (SRC == kSrcF32 || tab), "null pointer");
  FCVSR_CHECK_ARG(N > 0 && C > 0 && b > 0 && T > 0, "sizes: all positive");
  FCVSR_TILE_GRID_CHECKS();
  FCVSR_CHECK_ARG(((uintptr_t)src % (SRC == kSrcF32 ? 4 : SRC == kSrcU16 ? 2 : 1)) == 0, "src: aligned to its sample size");
  FCVSR_CHECK_ARG(((uintptr_t)idx % 4) == 0, "idx: 4-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)out % 16) == 0, "out: 16-byte aligned");
  const int blocks_x = cdiv(tw, EN_TILE);
  const long long blocks = (long long)blocks_x * cdiv(th, EN_TILE);
  const long long planes = (long long)b * ny * nx * T * C;
  FCVSR_CHECK_ARG((long long)b * ny * nx < (1ll << 31) && (long long)T * C < (1ll << 31) && planes < (1ll << 31) &&
                      planes * blocks < (1ll << 31),
                  "too many blocks for one launch");
  hipLaunchKernelGGL((tile_windows_kernel<SRC>), dim3((unsigned)(planes * blocks)), dim3(EN_THREADS), 0, (hipStream_t)stream, src, tab,
                     idx, N, C, h, w, T, ys, ny, xs, nx, th, tw, blocks_x, (int)blocks, out);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_tile_windows(const float* src, int N, int C, int h, int w, const int32_t* idx, int b, int T, const int32_t* ys,
                                  int ny, const int32_t* xs, int nx, int th, int tw, float* out, void* stream) {
  return tile_windows_launch<kSrcF32>(src, nullptr, N, C, h, w, idx, b, T, ys, ny, xs, nx, th, tw, out, stream);
}

extern "C" int fcvsr_tile_windows_u8(const uint8_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                                     const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, float* out, void* stream) {
  return tile_windows_launch<kSrcU8>(src, tab, N, C, h, w, idx, b, T, ys, ny, xs, nx, th, tw, out, stream);
}

extern "C" int fcvsr_tile_windows_u16(const uint16_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b,
                                      int T, const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, float* out,
                                      void* stream) {
  return tile_windows_launch<kSrcU16>(src, tab, N, C, h, w, idx, b, T, ys, ny, xs, nx, th, tw, out, stream);
}

template <class O, int PEAK, int Q>
static void tile_merge_go(const float* tiles, const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, const float* wy,
                          const float* wx, int planes, int C, int h, int w, int blocks_x, int blocks, void* out, void* stream) {
  hipLaunchKernelGGL((tile_merge_kernel<O, PEAK, Q>), dim3((unsigned)((long long)planes * blocks)), dim3(EN_THREADS), 0,
                     (hipStream_t)stream, tiles, ys, ny, xs, nx, th, tw, wy, wx, C, h, w, blocks_x, blocks, reinterpret_cast<O*>(out));
}

extern "C" int fcvsr_tile_merge(const float* tiles, const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, const float* wy,
                                const float* wx, int b, int C, int h, int w, int out_dtype, int quantise, void* out, void* stream) {
  FCVSR_CHECK_ARG(tiles && wy && wx && out, "null pointer");
  FCVSR_CHECK_ARG(b > 0 && C > 0, "sizes: all positive");
  FCVSR_TILE_GRID_CHECKS();
  FCVSR_CHECK_ARG(out_dtype == FCVSR_F32 || out_dtype == FCVSR_U8 || out_dtype == FCVSR_U16, "out_dtype: FCVSR_F32, _U8 or _U16");
  if (out_dtype == FCVSR_F32) FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE, "quantise: FCVSR_QUANT_NONE for an f32 result");
  else FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  FCVSR_CHECK_ARG(((uintptr_t)tiles % 16) == 0 && ((uintptr_t)wx % 16) == 0, "tiles, wx: 16-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)wy % 4) == 0, "wy: 4-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)out % (out_dtype == FCVSR_F32 ? 16 : out_dtype == FCVSR_U16 ? 8 : 4)) == 0,
                  "out: aligned to four samples (16 bytes f32, 8 uint16, 4 uint8)");
  const int blocks_x = cdiv(4ll * w, EN_TILE);
  const long long blocks = (long long)blocks_x * cdiv(4ll * h, EN_TILE);
  const long long planes = (long long)b * C;
  FCVSR_CHECK_ARG(planes < (1ll << 29) && blocks < (1ll << 31) && planes * blocks < (1ll << 31), "too many blocks for one launch");
  FCVSR_CHECK_ARG((long long)b * ny * nx < (1ll << 31), "too many tiles");
  const int pl = (int)planes, bl = (int)blocks;
  if (out_dtype == FCVSR_F32)
    tile_merge_go<float, 0, FCVSR_QUANT_TRUNCATE>(tiles, ys, ny, xs, nx, th, tw, wy, wx, pl, C, h, w, blocks_x, bl, out, stream);
  else if (out_dtype == FCVSR_U8 && quantise == FCVSR_QUANT_TRUNCATE)
    tile_merge_go<uint8_t, kPeak8, FCVSR_QUANT_TRUNCATE>(tiles, ys, ny, xs, nx, th, tw, wy, wx, pl, C, h, w, blocks_x, bl, out, stream);
  else if (out_dtype == FCVSR_U8)
    tile_merge_go<uint8_t, kPeak8, FCVSR_QUANT_ROUND>(tiles, ys, ny, xs, nx, th, tw, wy, wx, pl, C, h, w, blocks_x, bl, out, stream);
  else if (quantise == FCVSR_QUANT_TRUNCATE)
    tile_merge_go<uint16_t, kPeak10, FCVSR_QUANT_TRUNCATE>(tiles, ys, ny, xs, nx, th, tw, wy, wx, pl, C, h, w, blocks_x, bl, out, stream);
  else
    tile_merge_go<uint16_t, kPeak10, FCVSR_QUANT_ROUND>(tiles, ys, ny, xs, nx, th, tw, wy, wx, pl, C, h, w, blocks_x, bl, out, stream);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
