// Scene-cut statistic: the sum of absolute sample differences of every pair of consecutive frames, in exact integers
// (the contract is fcvsr_amd/harness/shots.py, pair_sad_host).  Integer arithmetic only, no atomics: every workgroup writes its own
// u64 partial sums and a second launch adds them.
//
// A workgroup is one wave.  It owns one tile of kTile bytes of the frame (16 bytes per lane: one global_load_dwordx4) and walks a run
// of kRun consecutive pairs, i.e. kRun + 1 frames, keeping the previous frame's 16 bytes in registers: a frame is read once by the run
// it belongs to, and the first frame of a run a second time by the run before it (1 / kRun more traffic, and that line is usually
// still in L2).  DESIGN.md section 4 has the arithmetic behind kRun and the one-wave workgroup.
#include "common.h"
#include "int_chunk.h"

namespace fcvsr {
namespace {

using int_chunk::kChunk;                        // bytes per lane and frame
using int_chunk::kLanes;                        // one wave per workgroup: no LDS, no barrier
using int_chunk::kSumThreads;
using int_chunk::u32x4;
// load_chunk<E, A16, WHOLE>: the lane's 16 bytes of one frame, uint16 samples as min(k, 1023).  WHOLE: the tile lies inside the frame.
// A16 fails where the frame size is no multiple of 16 bytes: every second frame is then off the 16-byte grid.
using int_chunk::load_chunk;
constexpr int kTile = kLanes * kChunk;          // bytes of a frame per workgroup
constexpr int kRun = 8;                         // pairs per workgroup (kRun + 1 frames read)

static_assert(kTile == FCVSR_PAIR_SAD_TILE_BYTES, "the header's tile size sizes the caller's scratch array");
// Per pair a lane adds kChunk differences of at most 255 (uint8) or kChunk / 2 of at most 1023 (uint16, samples clamped to 1023) into
// a u32, and the wave reduction adds kLanes such sums in u32: both stay far below 2^32.
constexpr unsigned long long kLaneMax = (kChunk * 255ull > (kChunk / 2) * 1023ull) ? kChunk * 255ull : (kChunk / 2) * 1023ull;
static_assert(kLaneMax * kLanes <= 0xffffffffull, "a wave's sum of one pair must fit in 32 bits");

template <int E>
__device__ __forceinline__ unsigned sad_word(unsigned a, unsigned b, unsigned acc) {
  return E == 1 ? __builtin_amdgcn_sad_u8(a, b, acc) : __builtin_amdgcn_sad_u16(a, b, acc);
}

template <int E>
__device__ __forceinline__ unsigned sad_chunk(u32x4 a, u32x4 b) {
  return sad_word<E>(a.w, b.w, sad_word<E>(a.z, b.z, sad_word<E>(a.y, b.y, sad_word<E>(a.x, b.x, 0u))));
}

// One run of one tile: partial[pair][tile] for the run's n pairs.
template <int E, bool A16, bool WHOLE>
__device__ __forceinline__ void pair_sad_run(const unsigned char* p, long long fbytes, long long left, int n,
                                             unsigned long long* out, long long out_stride) {
  unsigned acc[kRun];
  if (n == kRun) {                                                 // a whole run: all kRun + 1 loads are issued before the first use
    u32x4 f[kRun + 1];
#pragma unroll
    for (int k = 0; k <= kRun; ++k) f[k] = load_chunk<E, A16, WHOLE>(p + k * fbytes, left);
#pragma unroll
    for (int k = 0; k < kRun; ++k) acc[k] = sad_chunk<E>(f[k], f[k + 1]);
  } else {
    u32x4 prev = load_chunk<E, A16, WHOLE>(p, left);
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
      acc[k] = 0u;
      if (k < n) {                                                 // the same in every lane
        const u32x4 cur = load_chunk<E, A16, WHOLE>(p + (k + 1) * fbytes, left);
        acc[k] = sad_chunk<E>(prev, cur);
        prev = cur;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRun; ++k) {
    unsigned v = acc[k];
    for (int o = kLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (threadIdx.x == 0 && k < n) out[k * out_stride] = v;
  }
}

// grid (tiles, runs).  partial[pair][tile] = this tile's sum of pair `pair` = |frame[pair + 1] - frame[pair]|.
template <int E, bool A16>
__global__ __launch_bounds__(kLanes) void pair_sad_kernel(const unsigned char* __restrict__ frames, long long fbytes, int npairs,
                                                          unsigned long long* __restrict__ partial) {
  const int lane = threadIdx.x, tile = blockIdx.x, tiles = gridDim.x;
  const int p0 = blockIdx.y * kRun;
  const int n = npairs - p0 < kRun ? npairs - p0 : kRun;           // pairs of this run, >= 1
  const long long off = (long long)tile * kTile + lane * kChunk;
  const long long left = fbytes - off;
  const unsigned char* p = frames + (long long)p0 * fbytes + off;  // frame p0; the run reads frames p0 .. p0 + n <= npairs
  unsigned long long* out = partial + (long long)p0 * tiles + tile;
  if ((long long)(tile + 1) * kTile <= fbytes) pair_sad_run<E, A16, true>(p, fbytes, left, n, out, tiles);    // every tile but the last
  else pair_sad_run<E, A16, false>(p, fbytes, left, n, out, tiles);
}

template <int E>
void launch_pair_sad(const void* frames, long long fbytes, int npairs, int tiles, unsigned long long* partial, hipStream_t st) {
  const dim3 grid((unsigned)tiles, (unsigned)cdiv(npairs, kRun));
  const unsigned char* f = (const unsigned char*)frames;
  if ((uintptr_t)frames % kChunk == 0 && fbytes % kChunk == 0)
    hipLaunchKernelGGL((pair_sad_kernel<E, true>), grid, dim3(kLanes), 0, st, f, fbytes, npairs, partial);
  else
    hipLaunchKernelGGL((pair_sad_kernel<E, false>), grid, dim3(kLanes), 0, st, f, fbytes, npairs, partial);
}

}  // namespace
}  // namespace fcvsr

extern "C" int fcvsr_frame_pair_sad(const void* frames, int elem_size, int N, long long samples, void* scratch,
                                    long long scratch_bytes, long long* out, void* stream) {
  using namespace fcvsr;
  FCVSR_CHECK_ARG(elem_size == 1 || elem_size == 2, "elem_size: 1 (uint8) or 2 (uint16)");
  FCVSR_CHECK_ARG(N >= 1 && samples >= 1, "N and samples: at least 1");
  if (N == 1) return 0;                                            // no pair, nothing to write
  FCVSR_CHECK_ARG(frames && out && scratch, "null device pointer");
  FCVSR_CHECK_ARG(((uintptr_t)frames % elem_size) == 0, "frames: aligned to its sample size");
  FCVSR_CHECK_ARG(((uintptr_t)scratch % 8) == 0 && ((uintptr_t)out % 8) == 0, "scratch and out: 8-byte aligned");
  FCVSR_CHECK_ARG(samples <= (1ll << 40), "frame too large");
  const long long fbytes = samples * elem_size;
  const long long tiles = (fbytes + kTile - 1) / kTile;
  const int npairs = N - 1;
  FCVSR_CHECK_ARG(tiles <= 0x7fffffffll, "frame too large: more than 2^31 - 1 tiles");
  FCVSR_CHECK_ARG(cdiv(npairs, kRun) <= 65535, "too many frames");
  FCVSR_CHECK_ARG(scratch_bytes >= (long long)npairs * tiles * 8, "scratch: (N - 1) * ceil(frame bytes / FCVSR_PAIR_SAD_TILE_BYTES) * 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  if (elem_size == 1) launch_pair_sad<1>(frames, fbytes, npairs, (int)tiles, (unsigned long long*)scratch, st);
  else launch_pair_sad<2>(frames, fbytes, npairs, (int)tiles, (unsigned long long*)scratch, st);
  FCVSR_LAUNCH_CHECK();
  // out[pair] = the sum over tiles of partial[pair][tile]
  hipLaunchKernelGGL(int_chunk::partial_sum_kernel<kSumThreads>, dim3((unsigned)npairs), dim3(kSumThreads), 0, st,
                     (const unsigned long long*)scratch, (int)tiles, out);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
