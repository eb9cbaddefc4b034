// Training batches from device-resident uint8 / uint16 sequences: crop + flips + transpose + uint8 -> f32 of a whole batch in one launch
// (the reference's RandomCrop / Augment / ToTensor, CVSR_train/opt/data_LD_LR.py:248-344, with the draws made on the host).
//   out[y][x] = tab[ A[x][y] ] (transpose bit) or tab[ A[y][x] ],   A[i][j] = crop[vflip ? s-1-i : i][hflip ? s-1-j : j],
//   crop[r][c] = src[(top + r) * pitch + left + c]
// One workgroup makes one 64 x 64 tile of one output plane.  It reads the tile's source bytes along SOURCE rows, 4 neighbouring
// bytes per lane (16 lanes cover a row of the tile, in all 8 flag combinations: a flip only mirrors where the bytes go), and
// drops them at their OUTPUT position in an LDS tile; the tile is then read back along output rows, 4 bytes per thread, and
// leaves as one 16-byte f32 store per thread.  A source row starts at any byte, so a lane takes its 4 bytes out of the two
// ALIGNED dwords around them; a dword is loaded only if it holds at least one byte of the window, and an aligned dword lies
// in one page, so no load touches memory beyond the pages of the window.  The 256-float table is copied to LDS first.
// LDS rows are 68 bytes (17 dwords): in the transposed case the 16 lanes of a source row write LDS rows 4 apart, i.e. 68 dwords
// = 4 banks apart, a 2-way conflict on the byte stores (at a pitch of 64 bytes all 16 would meet on one bank).
//
// 10-bit sequences (uint16 containers, clip_batch_u16_kernel): the same kernel for 2-byte samples.  A descriptor's pitch / top /
// left count SAMPLES, its src is 2-byte aligned; the table has 1024 entries (4 KB of LDS) and the index is min(sample, 1023),
// unsigned, so 0x8000 .. 0xFFFF read entry 1023.  A lane's 4 samples are 8 bytes at an address that is 0 or 2 mod 4: it takes them
// out of the two or three ALIGNED dwords around them with a funnel shift by 16 bits.  The first two dwords always hold samples of
// the lane; the third is loaded only when the address is 2 mod 4 (else the second is read again), so again a dword is loaded only
// if it holds at least one sample of the window, an aligned dword lies in one page, and no load touches memory beyond the pages
// of the window.  hflip reverses the four 16-bit samples (swap the dwords, rotate each by 16), not the bytes.
// LDS rows are 132 bytes (33 dwords, 66 samples): in the transposed case the 16 lanes of a source row write LDS rows 4 apart,
// i.e. 4 * 132 B = 132 dwords = 4 banks (mod 32) apart: 8 distinct banks, a 2-way conflict on the 2-byte stores, as in the uint8
// kernel (at 128 bytes all 16 would meet on one bank; 136 bytes, which would keep rows 8-byte aligned, puts them 8 banks apart:
// 4-way; 16 distinct banks need a pitch of 2 mod 4 bytes, which leaves every other row misaligned for the dword reads on the way
// out).  Rows are 4-byte aligned: a thread's 4 samples come back as two dword reads.
#include "common.h"

namespace fcvsr {

constexpr int CB_TILE = 64;
constexpr int CB_PITCH = CB_TILE + 4;
constexpr int CB_THREADS = 256;
typedef __attribute__((address_space(1))) uint32_t global_u32;

__global__ __launch_bounds__(CB_THREADS) void clip_batch_u8_kernel(const fcvsr_crop_desc* desc, const float* tab, int s, int tiles,
                                                                   float* dst) {
  __shared__ float ltab[256];
  __shared__ __attribute__((aligned(16))) uint8_t tile[CB_TILE * CB_PITCH];
  static_assert(CB_THREADS == 256, "one table entry per thread");
  ltab[threadIdx.x] = tab[threadIdx.x];
  const int p = blockIdx.x / (tiles * tiles);
  const int t = blockIdx.x % (tiles * tiles);
  const int oy0 = (t / tiles) * CB_TILE, ox0 = (t % tiles) * CB_TILE;      // the tile's corner in the output plane
  const int oh = min(CB_TILE, s - oy0), ow = min(CB_TILE, s - ox0);        // multiples of 4 (s % 4 == 0)
  const fcvsr_crop_desc d = desc[p];
  const bool hflip = d.flags & FCVSR_CROP_HFLIP, vflip = d.flags & FCVSR_CROP_VFLIP, tr = d.flags & FCVSR_CROP_TRANSPOSE;
  // the tile of A behind this output tile: rows i0 .. i0+ah, columns j0 .. j0+aw
  const int i0 = tr ? ox0 : oy0, j0 = tr ? oy0 : ox0;
  const int ah = tr ? ow : oh, aw = tr ? oh : ow;
  // its columns are the crop's columns c0 .. c0+aw, ascending in memory; under hflip column c0+m is A's column j0+aw-1-m
  const int c0 = hflip ? s - j0 - aw : j0;
  const uint8_t* src = d.src + (long long)d.top * d.pitch + d.left + c0;
  const int m0 = (threadIdx.x % (CB_TILE / 4)) * 4;                         // this lane's 4 bytes of a source row
  const int li0 = threadIdx.x / (CB_TILE / 4);
  constexpr int ROWS = CB_THREADS / (CB_TILE / 4), PASSES = CB_TILE / ROWS;
  uint32_t v[PASSES];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {                                        // all loads of the thread in flight before the first use
    const int li = li0 + k * ROWS;
    const bool live = li < ah && m0 < aw;                                   // a lane outside the tile re-reads the tile's first bytes
    const int r = vflip ? s - 1 - (i0 + (live ? li : 0)) : i0 + (live ? li : 0);
    const uintptr_t a = (uintptr_t)(src + (long long)r * d.pitch + (live ? m0 : 0));
    const unsigned sh = (unsigned)(a & 3);
    const global_u32* w = reinterpret_cast<const global_u32*>(a - sh);      // the pointer came out of memory: say that it is global
    const uint32_t lo = w[0];
    const uint32_t hi = w[sh ? 1 : 0];                                      // bytes a+4-sh .. a+3 of the window live there (none: sh = 0)
    v[k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
  }
  const int lj0 = hflip ? aw - 4 - m0 : m0;                                 // A's column (inside the tile) of the lane's LOWEST one
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int li = li0 + k * ROWS;
    if (li < ah && m0 < aw) {
      const uint32_t q = hflip ? __builtin_bswap32(v[k]) : v[k];            // bytes in the order of A's columns lj0 .. lj0+3
      if (!tr) {
        *reinterpret_cast<uint32_t*>(tile + li * CB_PITCH + lj0) = q;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(lj0 + e) * CB_PITCH + li] = (uint8_t)(q >> (8 * e));
      }
    }
  }
  __syncthreads();
  float* out = dst + (long long)p * s * s;
  const int x = (threadIdx.x % (CB_TILE / 4)) * 4;
#pragma unroll
  for (int k = 0; k < CB_TILE * CB_TILE / 4 / CB_THREADS; ++k) {
    const int y = threadIdx.x / (CB_TILE / 4) + k * (CB_THREADS / (CB_TILE / 4));
    if (y < oh && x < ow) {
      const uint32_t q = *reinterpret_cast<const uint32_t*>(tile + y * CB_PITCH + x);
      *reinterpret_cast<float4*>(out + (long long)(oy0 + y) * s + ox0 + x) =
          make_float4(ltab[q & 255u], ltab[(q >> 8) & 255u], ltab[(q >> 16) & 255u], ltab[q >> 24]);
    }
  }
}

constexpr int CB16_PITCH = CB_TILE + 2;                                       // in samples: 132 bytes
constexpr int CB16_TAB = 1024;

__global__ __launch_bounds__(CB_THREADS) void clip_batch_u16_kernel(const fcvsr_crop_desc* desc, const float* tab, int s, int tiles,
                                                                    float* dst) {
  __shared__ float ltab[CB16_TAB];
  __shared__ __attribute__((aligned(16))) uint16_t tile[CB_TILE * CB16_PITCH];
  static_assert(CB16_TAB % CB_THREADS == 0 && CB16_PITCH % 2 == 0, "whole table passes; 4-byte aligned LDS rows");
#pragma unroll
  for (int k = 0; k < CB16_TAB / CB_THREADS; ++k) ltab[threadIdx.x + k * CB_THREADS] = tab[threadIdx.x + k * CB_THREADS];
  const int p = blockIdx.x / (tiles * tiles);
  const int t = blockIdx.x % (tiles * tiles);
  const int oy0 = (t / tiles) * CB_TILE, ox0 = (t % tiles) * CB_TILE;      // the tile's corner in the output plane
  const int oh = min(CB_TILE, s - oy0), ow = min(CB_TILE, s - ox0);        // multiples of 4 (s % 4 == 0)
  const fcvsr_crop_desc d = desc[p];
  const bool hflip = d.flags & FCVSR_CROP_HFLIP, vflip = d.flags & FCVSR_CROP_VFLIP, tr = d.flags & FCVSR_CROP_TRANSPOSE;
  // the tile of A behind this output tile: rows i0 .. i0+ah, columns j0 .. j0+aw
  const int i0 = tr ? ox0 : oy0, j0 = tr ? oy0 : ox0;
  const int ah = tr ? ow : oh, aw = tr ? oh : ow;
  // its columns are the crop's columns c0 .. c0+aw, ascending in memory; under hflip column c0+m is A's column j0+aw-1-m
  const int c0 = hflip ? s - j0 - aw : j0;
  const uint8_t* src = d.src + 2 * ((long long)d.top * d.pitch + d.left + c0);   // pitch, top, left in samples
  const int m0 = (threadIdx.x % (CB_TILE / 4)) * 4;                         // this lane's 4 samples of a source row
  const int li0 = threadIdx.x / (CB_TILE / 4);
  constexpr int ROWS = CB_THREADS / (CB_TILE / 4), PASSES = CB_TILE / ROWS;
  uint32_t v0[PASSES], v1[PASSES];
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {                                        // all loads of the thread in flight before the first use
    const int li = li0 + k * ROWS;
    const bool live = li < ah && m0 < aw;                                   // a lane outside the tile re-reads the tile's first samples
    const int r = vflip ? s - 1 - (i0 + (live ? li : 0)) : i0 + (live ? li : 0);
    const uintptr_t a = (uintptr_t)(src + 2 * ((long long)r * d.pitch + (live ? m0 : 0)));
    const unsigned sh = (unsigned)(a & 2);                                  // src is 2-byte aligned: a is 0 or 2 mod 4
    const global_u32* w = reinterpret_cast<const global_u32*>(a - sh);      // the pointer came out of memory: say that it is global
    const uint32_t w0 = w[0];                                               // samples 0, 1 (sh = 0) or sample 0 in its high half
    const uint32_t w1 = w[1];                                               // samples 2, 3 or 1, 2
    const uint32_t w2 = w[sh ? 2 : 1];                                      // sample 3 lives there (nothing new: sh = 0)
    v0[k] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * sh));
    v1[k] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> (8 * sh));
  }
  const int lj0 = hflip ? aw - 4 - m0 : m0;                                 // A's column (inside the tile) of the lane's LOWEST one
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int li = li0 + k * ROWS;
    if (li < ah && m0 < aw) {
      // samples in the order of A's columns lj0 .. lj0+3: hflip reverses the four 16-bit samples
      const uint32_t q0 = hflip ? (v1[k] >> 16) | (v1[k] << 16) : v0[k];
      const uint32_t q1 = hflip ? (v0[k] >> 16) | (v0[k] << 16) : v1[k];
      if (!tr) {
        uint32_t* row = reinterpret_cast<uint32_t*>(tile + li * CB16_PITCH + lj0);
        row[0] = q0;
        row[1] = q1;
      } else {
        tile[(lj0 + 0) * CB16_PITCH + li] = (uint16_t)q0;
        tile[(lj0 + 1) * CB16_PITCH + li] = (uint16_t)(q0 >> 16);
        tile[(lj0 + 2) * CB16_PITCH + li] = (uint16_t)q1;
        tile[(lj0 + 3) * CB16_PITCH + li] = (uint16_t)(q1 >> 16);
      }
    }
  }
  __syncthreads();
  float* out = dst + (long long)p * s * s;
  const int x = (threadIdx.x % (CB_TILE / 4)) * 4;
#pragma unroll
  for (int k = 0; k < CB_TILE * CB_TILE / 4 / CB_THREADS; ++k) {
    const int y = threadIdx.x / (CB_TILE / 4) + k * (CB_THREADS / (CB_TILE / 4));
    if (y < oh && x < ow) {
      const uint32_t* row = reinterpret_cast<const uint32_t*>(tile + y * CB16_PITCH + x);
      const uint32_t q0 = row[0], q1 = row[1];
      *reinterpret_cast<float4*>(out + (long long)(oy0 + y) * s + ox0 + x) =
          make_float4(ltab[min(q0 & 0xffffu, 1023u)], ltab[min(q0 >> 16, 1023u)], ltab[min(q1 & 0xffffu, 1023u)],
                      ltab[min(q1 >> 16, 1023u)]);
    }
  }
}

}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_clip_batch_u8(const fcvsr_crop_desc* desc, const float* tab, int P, int s, float* dst, void* stream) {
  FCVSR_CHECK_ARG(desc && tab && dst, "null pointer");
  FCVSR_CHECK_ARG(P > 0, "P: at least one plane");
  FCVSR_CHECK_ARG(s > 0 && s % 4 == 0, "s: a positive multiple of 4");
  FCVSR_CHECK_ARG(((uintptr_t)dst % 16) == 0, "dst: 16-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)desc % 8) == 0, "desc: 8-byte aligned");
  const int tiles = cdiv(s, CB_TILE);
  FCVSR_CHECK_ARG((long long)P * tiles * tiles < (1ll << 31), "too many tiles for one launch");
  hipLaunchKernelGGL(clip_batch_u8_kernel, dim3(P * tiles * tiles), dim3(CB_THREADS), 0, (hipStream_t)stream, desc, tab, s, tiles, dst);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_clip_batch_u16(const fcvsr_crop_desc* desc, const float* tab, int P, int s, float* dst, void* stream) {
  FCVSR_CHECK_ARG(desc && tab && dst, "null pointer");
  FCVSR_CHECK_ARG(P > 0, "P: at least one plane");
  FCVSR_CHECK_ARG(s > 0 && s % 4 == 0, "s: a positive multiple of 4");
  FCVSR_CHECK_ARG(((uintptr_t)dst % 16) == 0, "dst: 16-byte aligned");
  FCVSR_CHECK_ARG(((uintptr_t)desc % 8) == 0, "desc: 8-byte aligned");
  const int tiles = cdiv(s, CB_TILE);
  FCVSR_CHECK_ARG((long long)P * tiles * tiles < (1ll << 31), "too many tiles for one launch");
  hipLaunchKernelGGL(clip_batch_u16_kernel, dim3(P * tiles * tiles), dim3(CB_THREADS), 0, (hipStream_t)stream, desc, tab, s, tiles, dst);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
