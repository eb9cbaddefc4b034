// Shared by the kernels that build model windows straight from the resident sequence (ensemble.hip, tiles.hip): the 64 x 64 tile
// geometry of one workgroup (256 threads, 16 lanes of 4 samples per tile row, 4 passes of 16 rows) and en_load4, which takes up to 4
// neighbouring samples of a frame row as the floats the model reads.  Frames start at any sample (h*w odd, w % 4 != 0), so integer
// samples are taken out of the ALIGNED dwords around them with a funnel shift; a dword is loaded only if it holds at least one
// sample the lane needs, and an aligned dword lies in one page, so no load touches memory beyond the pages of the sequence.  f32
// samples are loaded one by one (a row starts at any multiple of 4 bytes).
#pragma once
#include "common.h"
#include "u8.h"

namespace fcvsr {

constexpr int EN_TILE = 64;
constexpr int EN_THREADS = 256;
constexpr int EN_LANES = EN_TILE / 4;                  // lanes per tile row, 4 samples each
constexpr int EN_ROWS = EN_THREADS / EN_LANES;         // tile rows per pass
constexpr int EN_PASSES = EN_TILE / EN_ROWS;
typedef __attribute__((address_space(1))) uint32_t en_global_u32;

__host__ __device__ inline int ceil4(int v) { return (v + 3) & ~3; }

// The nv (1..4) samples at src[off .. off+nv) as the floats the model reads; v[nv..] is unspecified.
template <int SRC>
__device__ __forceinline__ void en_load4(const void* src, long long off, int nv, const float* tab, float v[4]) {
  if constexpr (SRC == kSrcF32) {
    const float* p = reinterpret_cast<const float*>(src) + off;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p[e < nv ? e : 0];
  } else if constexpr (SRC == kSrcU8) {
    const uintptr_t a = (uintptr_t)(reinterpret_cast<const uint8_t*>(src) + off);
    const unsigned sh = (unsigned)(a & 3);
    const en_global_u32* w = reinterpret_cast<const en_global_u32*>(a - sh);
    const uint32_t lo = w[0];
    const uint32_t hi = w[sh + nv > 4 ? 1 : 0];                              // bytes a+4-sh .. of the lane live there
    const uint32_t q = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tab[(q >> (8 * e)) & 255u];
  } else {
    const uintptr_t a = (uintptr_t)(reinterpret_cast<const uint16_t*>(src) + off);   // 2-byte aligned: 0 or 2 mod 4
    const unsigned sh = (unsigned)(a & 2);
    const en_global_u32* w = reinterpret_cast<const en_global_u32*>(a - sh);
    const unsigned nb = sh + 2 * nv;                                         // bytes from the aligned dword to the lane's last sample
    const int i1 = nb > 4 ? 1 : 0, i2 = nb > 8 ? 2 : i1;
    const uint32_t w0 = w[0], w1 = w[i1], w2 = w[i2];
    const uint32_t q0 = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * sh));
    const uint32_t q1 = (uint32_t)((((uint64_t)w2 << 32) | w1) >> (8 * sh));
    v[0] = tab[min(q0 & 0xffffu, (uint32_t)kPeak10)];
    v[1] = tab[min(q0 >> 16, (uint32_t)kPeak10)];
    v[2] = tab[min(q1 & 0xffffu, (uint32_t)kPeak10)];
    v[3] = tab[min(q1 >> 16, (uint32_t)kPeak10)];
  }
}

}  // namespace fcvsr
