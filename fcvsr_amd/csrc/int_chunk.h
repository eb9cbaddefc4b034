// What the exact-integer statistics over resident uint8 / uint16 frames share (shots.hip, active.hip, plane_sse.hip and the tile
// comparison of tiles.hip): a lane takes kChunk bytes of a row in one
// global_load_dwordx4 from an address that carries the sample's alignment only, a tail shorter than a chunk is read byte by byte
// and zero-filled, uint16 samples are read as min(k, 1023), and u64 partial sums are added by a second launch in a fixed order:
// integer arithmetic only, no atomics.  A wave sum is the one-line
// __shfl_xor loop where it is needed, not a function of this header: behind a call (by value or by reference, inlined or not) the
// compiler orders the instructions around it differently in every kernel, the sum kernel below included, and these kernels are
// kept instruction for instruction (profiles/NOTES.md has the per-kernel table).
#pragma once
#include "common.h"

namespace fcvsr {
namespace int_chunk {

constexpr int kLanes = 64;                      // a wave
constexpr int kChunk = 16;                      // bytes per lane and load
constexpr int kSumThreads = 256;                // of the launch that adds the partial sums

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 halves(unsigned w) {
  u16x2 v;
  __builtin_memcpy(&v, &w, 4);
  return v;
}

// uint16 samples are read as min(k, 1023), both halves of a word at once (v_pk_min_u16, an unsigned minimum)
__device__ __forceinline__ unsigned clamp10(unsigned w) {
  u16x2 v = __builtin_elementwise_min(halves(w), u16x2{1023, 1023});
  __builtin_memcpy(&w, &v, 4);
  return w;
}

// A chunk as its samples are read: uint16 (E == 2) clamped, bytes as they are
template <int E>
__device__ __forceinline__ u32x4 clamp_chunk(u32x4 v) {
  return E == 2 ? u32x4{clamp10(v.x), clamp10(v.y), clamp10(v.z), clamp10(v.w)} : v;
}

// The raw bits of the lane's 16 bytes of one row, samples of E bytes.  left: bytes of the row from p on - a whole chunk (>= kChunk),
// a tail that is read byte by byte and zero-filled (two rows agree in the fill, and it adds nothing to a sum), or nothing (<= 0: p
// is never dereferenced).
// A16: every chunk address is a multiple of 16; otherwise the 16-byte load carries the sample's alignment only.
// WHOLE: every lane has a whole chunk and the load is unconditional (a tile inside the frame, as shots.hip's all but the last).
template <int E, bool A16 = false, bool WHOLE = false>
__device__ __forceinline__ u32x4 load_raw(const unsigned char* p, long long left) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (WHOLE || left >= kChunk) {
    if (A16) v = *reinterpret_cast<const u32x4*>(p);
    else __builtin_memcpy(&v, __builtin_assume_aligned(p, E), kChunk);
  } else if (left > 0) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (j < left) w[j / 4] |= (unsigned)p[j] << (8 * (j % 4));
    v = u32x4{w[0], w[1], w[2], w[3]};
  }
  return v;
}

// The same chunk as samples: uint16 read as min(k, 1023)
template <int E, bool A16, bool WHOLE = false>
__device__ __forceinline__ u32x4 load_chunk(const unsigned char* p, long long left) {
  return clamp_chunk<E>(load_raw<E, A16, WHOLE>(p, left));
}

// grid (outputs), THREADS threads.  out[i] = the sum of the nparts partials of output i: strided per thread, then the wave, then the
// waves in ascending order.  A template, so only a file that launches it holds it in its code object.
template <int THREADS = kSumThreads>
static __global__ __launch_bounds__(THREADS) void partial_sum_kernel(const unsigned long long* __restrict__ partial, int nparts,
                                                                      long long* __restrict__ out) {
  __shared__ unsigned long long sm[THREADS / kLanes];
  const unsigned long long* pp = partial + (long long)blockIdx.x * nparts;
  unsigned long long s = 0;
  for (int t = threadIdx.x; t < nparts; t += THREADS) s += pp[t];
  for (int o = kLanes / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x % kLanes == 0) sm[threadIdx.x / kLanes] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < THREADS / kLanes; ++w) t += sm[w];
    out[blockIdx.x] = (long long)t;
  }
}

}  // namespace int_chunk
}  // namespace fcvsr
