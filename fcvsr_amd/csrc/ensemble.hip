// Test-time self-ensemble (the reference's SpatialTemporalEnsemble, mmedit_train/mmedit/models/common/ensemble.py): the model runs on
// the 8 flips / transposes of a window and the 8 results are flipped back and averaged.  Specification: fcvsr_amd/harness/ensemble.py.
//   variant i of a frame f (h x w):  A[r][c] = f[i & 2 ? h-1-r : r][i & 1 ? w-1-c : c],   v_i = i & 4 ? A^T : A
//   its inverse on an output o:      i & 4 ? transpose, then i & 2 ? reverse rows, then i & 1 ? reverse columns
//
// ensemble_windows_kernel: all 8 variants of a batch of windows in one launch, straight from the resident sequence (N,C,h,w) (f32,
// uint8 or uint16 samples read through the format's table, u8.h) through a device index table (b,T).  Variants 0..3 of a plane are
// ceil4(h) x ceil4(w), variants 4..7 ceil4(w) x ceil4(h): each is zero-padded at ITS OWN bottom / right, so a pass sees what a plain
// run on the flipped video would see.  One workgroup makes one 64 x 64 tile of one output plane, the way clip_batch.hip makes a
// crop: it reads the tile's samples along SOURCE rows, 4 neighbouring samples per lane (16 lanes cover a row of the tile; a flip only
// mirrors where they go), converts them and drops them at their OUTPUT position in an f32 LDS tile; the tile is read back along
// output rows and leaves as one 16-byte store per thread, zeros where the padding is: every output element is stored exactly once.
// Frames start at any sample (h*w odd, w % 4 != 0), so integer samples are taken out of the ALIGNED dwords around them with a funnel
// shift; a dword is loaded only if it holds at least one sample the lane needs, and an aligned dword lies in one page, so no load
// touches memory beyond the pages of the sequence.  f32 samples are loaded one by one (a row starts at any multiple of 4 bytes).
// LDS rows are 65 floats: in the transposed case the 16 lanes of a source row write LDS rows 4 apart, i.e. 260 dwords = 4 banks
// (mod 32) apart: 8 distinct banks, a 2-way conflict on the dword stores (at a pitch of 64 all 16 would meet on one bank; 68, which
// would keep rows 16-byte aligned, puts them on 2 banks); on the way out a thread's 4 floats are 4 dword reads, 2-way as well.
//
// ensemble_merge_kernel: crop, inverse transform, fixed-order sum and quantisation of the 8 (or 16) model outputs in one launch.
//   acc = o_0; acc = acc + o_i (i = 1..7), each sum rounded once in f32 (-ffp-contract=off);  mean8 = acc * 0.125f;
//   with the time-reversed passes: (mean8_fwd + mean8_rev) * 0.5f.
// One workgroup makes one 64 x 64 tile of one output plane (4h x 4w), a thread 4 neighbouring pixels in 4 rows.  Outputs 0..3 are
// read directly, 16 bytes per lane, the column reversal folded into the address (4w - 4 - x is a multiple of 4) and the order of the
// 4 floats; outputs 4..7 go through the LDS tile one after the other (read along their rows, 16 bytes per lane, written transposed
// and mirrored, 2-way conflict as above), so the sum order is the same for every pixel.  The result leaves as 4 floats (16 bytes), or
// quantised (u8.h) as 4 uint16 (8 bytes) / 4 uint8 (4 bytes): rows of a dense 4w-wide integer frame are aligned to 4 samples only.
#include "common.h"
#include "u8.h"
#include "window_load.h"

namespace fcvsr {

constexpr int EN_PITCH = EN_TILE + 1;

template <int SRC>
__global__ __launch_bounds__(EN_THREADS) void ensemble_windows_kernel(const void* src, const float* tab, const int32_t* idx, int N,
                                                                      int C, int h, int w, int b, int T, int reverse, int tiles,
                                                                      float* out_a, float* out_t) {
  __shared__ float tile[EN_TILE * EN_PITCH];
  const int P = b * T * C;
  const int i = blockIdx.x / (P * tiles);                                   // the variant
  const int p = (blockIdx.x / tiles) % P;
  const int t = blockIdx.x % tiles;
  const bool cf = i & 1, rf = i & 2, tr = i & 4;
  const int R = tr ? w : h, Cn = tr ? h : w;                                // the variant's own rows and columns
  const int Rp = ceil4(R), Cp = ceil4(Cn);
  const int tcols = (Cp + EN_TILE - 1) / EN_TILE;
  const int oy0 = (t / tcols) * EN_TILE, ox0 = (t % tcols) * EN_TILE;       // the tile's corner in the output plane
  const int oh = min(EN_TILE, Rp - oy0), ow = min(EN_TILE, Cp - ox0);       // multiples of 4
  const int vh = min(oh, R - oy0), vw = min(ow, Cn - ox0);                  // the part that is not padding: at least 1 x 1
  // the tile of A behind it: rows i0 .. i0+ah, columns j0 .. j0+aw
  const int i0 = tr ? ox0 : oy0, j0 = tr ? oy0 : ox0;
  const int ah = tr ? vw : vh, aw = tr ? vh : vw;
  // its columns are the frame's columns c0 .. c0+aw, ascending in memory; reversed, column c0+m is A's column j0+aw-1-m
  const int c0 = cf ? w - j0 - aw : j0;
  const int bi = p / (T * C), ti = (p / C) % T, c = p % C;
  const int n = min(max(idx[bi * T + (reverse ? T - 1 - ti : ti)], 0), N - 1);
  const long long plane = ((long long)n * C + c) * h * w;
  const int m0 = (threadIdx.x % EN_LANES) * 4;                              // this lane's 4 samples of a source row
  const int li0 = threadIdx.x / EN_LANES;
  float v[EN_PASSES][4];
#pragma unroll
  for (int k = 0; k < EN_PASSES; ++k) {                                     // all loads of the thread in flight before the first use
    const int li = li0 + k * EN_ROWS;
    const bool live = li < ah && m0 < aw;                                   // a lane outside the tile re-reads the tile's first sample
    const int lli = live ? li : 0, lm = live ? m0 : 0;
    const int r = rf ? h - 1 - (i0 + lli) : i0 + lli;
    en_load4<SRC>(src, plane + (long long)r * w + c0 + lm, live ? min(4, aw - m0) : 1, tab, v[k]);
  }
#pragma unroll
  for (int k = 0; k < EN_PASSES; ++k) {
    const int li = li0 + k * EN_ROWS;
    if (li < ah) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (m0 + e < aw) {
          const int lj = cf ? aw - 1 - (m0 + e) : m0 + e;                   // A's column inside the tile
          tile[tr ? lj * EN_PITCH + li : li * EN_PITCH + lj] = v[k][e];
        }
      }
    }
  }
  __syncthreads();
  float* out = (tr ? out_t : out_a) + ((long long)(i & 3) * P + p) * Rp * Cp;
  const int x = (threadIdx.x % EN_LANES) * 4;
#pragma unroll
  for (int k = 0; k < EN_PASSES; ++k) {
    const int y = threadIdx.x / EN_LANES + k * EN_ROWS;
    if (y < oh && x < ow) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (y < vh && x + e < vw) ? tile[y * EN_PITCH + x + e] : 0.f;
      *reinterpret_cast<float4*>(out + (long long)(oy0 + y) * Cp + ox0 + x) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// T = float: the f32 mean; uint8_t / uint16_t: quantised with mode Q at peak PEAK
template <class T, int PEAK, int Q>
__global__ __launch_bounds__(EN_THREADS) void ensemble_merge_kernel(const float* a, const float* at, const float* ra, const float* rat,
                                                                    int planes, int h, int w, int tiles_x, int tiles, T* out) {
  __shared__ float tile[EN_TILE * EN_PITCH];
  const int H4 = 4 * h, W4 = 4 * w;
  const int rows_a = 4 * ceil4(h), pitch_a = 4 * ceil4(w);                  // outputs 0..3: (4, planes, rows_a, pitch_a)
  const int rows_t = pitch_a, pitch_t = rows_a;                             // outputs 4..7: (4, planes, rows_t, pitch_t)
  const int p = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int Y0 = (t / tiles_x) * EN_TILE, X0 = (t % tiles_x) * EN_TILE;
  const int th = min(EN_TILE, H4 - Y0), tw = min(EN_TILE, W4 - X0);         // multiples of 4
  const int x = (threadIdx.x % EN_LANES) * 4, y0 = threadIdx.x / EN_LANES;
  float res[EN_PASSES][4];
  const int npass = ra ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const float* pa = pass ? ra : a;
    const float* pt = pass ? rat : at;
    float acc[EN_PASSES][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool cf = i & 1, rf = i & 2;
      const float* src = pa + ((long long)i * planes + p) * rows_a * pitch_a;
      const int xs = cf ? W4 - 4 - (X0 + x) : X0 + x;
#pragma unroll
      for (int k = 0; k < EN_PASSES; ++k) {
        const int y = y0 + k * EN_ROWS;
        if (y < th && x < tw) {
          const int ys = rf ? H4 - 1 - (Y0 + y) : Y0 + y;
          const float4 q = *reinterpret_cast<const float4*>(src + (long long)ys * pitch_a + xs);
          const float o[4] = {cf ? q.w : q.x, cf ? q.z : q.y, cf ? q.y : q.z, cf ? q.x : q.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[k][e] = i == 0 ? o[e] : acc[k][e] + o[e];
        }
      }
    }
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      const bool cf = i & 1, rf = i & 2;
      // output rows are this input's columns and the other way round: its rows xs0 .. xs0+tw, columns ys0 .. ys0+th
      const int xs0 = cf ? W4 - X0 - tw : X0, ys0 = rf ? H4 - Y0 - th : Y0;
      const float* src = pt + (((long long)i * planes + p) * rows_t + xs0) * pitch_t + ys0;
      float4 q[EN_PASSES];
#pragma unroll
      for (int k = 0; k < EN_PASSES; ++k) {
        const int r = y0 + k * EN_ROWS;
        q[k] = (r < tw && x < th) ? *reinterpret_cast<const float4*>(src + (long long)r * pitch_t + x) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();                                                      // the previous input's tile has been read
#pragma unroll
      for (int k = 0; k < EN_PASSES; ++k) {
        const int r = y0 + k * EN_ROWS;
        if (r < tw && x < th) {
          const int ox = cf ? tw - 1 - r : r;
          const float o[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) tile[(rf ? th - 1 - (x + e) : x + e) * EN_PITCH + ox] = o[e];
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < EN_PASSES; ++k) {
        const int y = y0 + k * EN_ROWS;
        if (y < th && x < tw) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[k][e] = acc[k][e] + tile[y * EN_PITCH + x + e];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EN_PASSES; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m = acc[k][e] * 0.125f;
        res[k][e] = pass == 0 ? m : (res[k][e] + m) * 0.5f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < EN_PASSES; ++k) {
    const int y = y0 + k * EN_ROWS;
    if (y < th && x < tw) {
      T* dp = out + ((long long)p * H4 + Y0 + y) * W4 + X0 + x;
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(dp) = make_float4(res[k][0], res[k][1], res[k][2], res[k][3]);
      } else {
        T o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = quantise<Q, PEAK, T>(res[k][e]);
        if constexpr (sizeof(T) == 1) *reinterpret_cast<uchar4*>(dp) = make_uchar4(o[0], o[1], o[2], o[3]);
        else *reinterpret_cast<ushort4*>(dp) = make_ushort4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

}  // namespace fcvsr

using namespace fcvsr;

constexpr int kEnMaxSide = 1 << 24;                                          // keeps 4 * ceil4(side) and every tile count in an int

template <int SRC>
static int ensemble_windows_launch(const void* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                                   int reverse, float* out_a, float* out_t, void* stream) {
  FCVSR_CHECK_ARG(src && idx && out_a && out_t && (SRC == kSrcF32 || tab), "null pointer");
  FCVSR_CHECK_ARG(N > 0 && C > 0 && h > 0 && w > 0 && b > 0 && T > 0, "sizes: all positive");
  FCVSR_CHECK_ARG(h <= kEnMaxSide && w <= kEnMaxSide, "frame too large");
  FCVSR_CHECK_ARG(reverse == 0 || reverse == 1, "reverse: 0 or 1");
  FCVSR_CHECK_ARG(((uintptr_t)src % (SRC == kSrcF32 ? 4 : SRC == kSrcU16 ? 2 : 1)) == 0, "src: aligned to its sample size");
  FCVSR_CHECK_ARG(((uintptr_t)idx % 4) == 0, "idx: 4-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)out_a % 16) == 0 && ((uintptr_t)out_t % 16) == 0, "out_a, out_t: 16-byte aligned");
  const long long tiles = (long long)cdiv(ceil4(h), EN_TILE) * cdiv(ceil4(w), EN_TILE);
  const long long blocks = 8ll * b * T * C * tiles;
  FCVSR_CHECK_ARG((long long)b * T * C < (1ll << 31) && blocks < (1ll << 31), "too many tiles for one launch");
  hipLaunchKernelGGL((ensemble_windows_kernel<SRC>), dim3((unsigned)blocks), dim3(EN_THREADS), 0, (hipStream_t)stream, src, tab, idx, N,
                     C, h, w, b, T, reverse, (int)tiles, out_a, out_t);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_ensemble_windows(const float* src, int N, int C, int h, int w, const int32_t* idx, int b, int T, int reverse,
                                      float* out_a, float* out_t, void* stream) {
  return ensemble_windows_launch<kSrcF32>(src, nullptr, N, C, h, w, idx, b, T, reverse, out_a, out_t, stream);
}

extern "C" int fcvsr_ensemble_windows_u8(const uint8_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b,
                                         int T, int reverse, float* out_a, float* out_t, void* stream) {
  return ensemble_windows_launch<kSrcU8>(src, tab, N, C, h, w, idx, b, T, reverse, out_a, out_t, stream);
}

extern "C" int fcvsr_ensemble_windows_u16(const uint16_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b,
                                          int T, int reverse, float* out_a, float* out_t, void* stream) {
  return ensemble_windows_launch<kSrcU16>(src, tab, N, C, h, w, idx, b, T, reverse, out_a, out_t, stream);
}

template <class T, int PEAK, int Q>
static void ensemble_merge_go(const float* a, const float* at, const float* ra, const float* rat, int planes, int h, int w, int tiles_x,
                              int tiles, void* out, void* stream) {
  hipLaunchKernelGGL((ensemble_merge_kernel<T, PEAK, Q>), dim3((unsigned)((long long)planes * tiles)), dim3(EN_THREADS), 0,
                     (hipStream_t)stream, a, at, ra, rat, planes, h, w, tiles_x, tiles, reinterpret_cast<T*>(out));
}

extern "C" int fcvsr_ensemble_merge(const float* a, const float* at, const float* ra, const float* rat, int b, int C, int h, int w,
                                    int out_dtype, int quantise, void* out, void* stream) {
  FCVSR_CHECK_ARG(a && at && out, "null pointer");
  FCVSR_CHECK_ARG((ra == nullptr) == (rat == nullptr), "ra, rat: both or neither");
  FCVSR_CHECK_ARG(b > 0 && C > 0 && h > 0 && w > 0, "sizes: all positive");
  FCVSR_CHECK_ARG(h <= kEnMaxSide && w <= kEnMaxSide, "frame too large");
  FCVSR_CHECK_ARG(out_dtype == FCVSR_F32 || out_dtype == FCVSR_U8 || out_dtype == FCVSR_U16, "out_dtype: FCVSR_F32, _U8 or _U16");
  if (out_dtype == FCVSR_F32) FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_NONE, "quantise: FCVSR_QUANT_NONE for an f32 result");
  else FCVSR_CHECK_ARG(quantise == FCVSR_QUANT_TRUNCATE || quantise == FCVSR_QUANT_ROUND, "quantise: FCVSR_QUANT_TRUNCATE or _ROUND");
  FCVSR_CHECK_ARG(((uintptr_t)a % 16) == 0 && ((uintptr_t)at % 16) == 0 && ((uintptr_t)ra % 16) == 0 && ((uintptr_t)rat % 16) == 0,
                  "a, at, ra, rat: 16-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)out % (out_dtype == FCVSR_F32 ? 16 : out_dtype == FCVSR_U16 ? 8 : 4)) == 0,
                  "out: aligned to four samples (16 bytes f32, 8 uint16, 4 uint8)");
  const int tiles_x = cdiv(4ll * w, EN_TILE);
  const long long tiles = (long long)tiles_x * cdiv(4ll * h, EN_TILE);
  const long long planes = (long long)b * C;
  FCVSR_CHECK_ARG(planes < (1ll << 29) && tiles < (1ll << 31) && planes * tiles < (1ll << 31), "too many tiles for one launch");
  const int pl = (int)planes, tl = (int)tiles;
  if (out_dtype == FCVSR_F32) ensemble_merge_go<float, 0, FCVSR_QUANT_TRUNCATE>(a, at, ra, rat, pl, h, w, tiles_x, tl, out, stream);
  else if (out_dtype == FCVSR_U8 && quantise == FCVSR_QUANT_TRUNCATE)
    ensemble_merge_go<uint8_t, kPeak8, FCVSR_QUANT_TRUNCATE>(a, at, ra, rat, pl, h, w, tiles_x, tl, out, stream);
  else if (out_dtype == FCVSR_U8)
    ensemble_merge_go<uint8_t, kPeak8, FCVSR_QUANT_ROUND>(a, at, ra, rat, pl, h, w, tiles_x, tl, out, stream);
  else if (quantise == FCVSR_QUANT_TRUNCATE)
    ensemble_merge_go<uint16_t, kPeak10, FCVSR_QUANT_TRUNCATE>(a, at, ra, rat, pl, h, w, tiles_x, tl, out, stream);
  else
    ensemble_merge_go<uint16_t, kPeak10, FCVSR_QUANT_ROUND>(a, at, ra, rat, pl, h, w, tiles_x, tl, out, stream);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
