// Training path: atomic-free backward of the IAC warp (reference CVSR_freq.py:1230-1250, flow_warp :1188-1227).  Same mathematics as
// fcvsr_iac_bwd_warp (train_iac.hip), with the bilinear scatter into g_prev replaced by a gather in a fixed order, so that two runs
// give the same bits:
//   1. source pass   iac_bwd_warp_kernel<.., false>: g_s, g_off (the bits of the scatter form) and per source pixel the key of its
//                    cell (b, y0 + 1, x0 + 1) on the (H+1) x (W+1) grid; one dump key above all cells for a pixel without a tap inside
//   2. inverted index: stable radix sort of (key, pixel) pairs (rocPRIM), then cell_start[k] = first sorted position with key >= k:
//                    the sources of a cell are contiguous and in ascending pixel order
//   3. gather pass   iac_gather_kernel: thread = (destination pixel, 4 channels); walks the four cells (yi + 1 - dy, xi + 1 - dx) in the
//                    order (dy,dx) = (0,0), (0,1), (1,0), (1,1), each in ascending position, recomputes the source's weights with the
//                    float expressions of warp_kernel and adds w * g_s.  Every element of g_prev is stored once (zeros where no
//                    source lands): no zero fill, no float atomics.  The build has -ffp-contract=off: each product is the float the
//                    scatter form adds, the two forms differ in summation order only.
// Work is linear in the input for any offset field: a cell that collects n sources costs its four destinations a walk of n.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include "train_iac.h"

namespace fcvsr {

// cell_start[k], k in [0, ncells]: lower bound of k in the sorted keys (cell k's sources are [cell_start[k], cell_start[k+1]))
__global__ __launch_bounds__(256) void iac_cell_start_kernel(const unsigned* __restrict__ keys, unsigned n, unsigned ncells,
                                                             unsigned* __restrict__ cell_start) {
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > ncells) return;
  unsigned lo = 0, hi = n;
  while (lo < hi) {
    const unsigned mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  cell_start[k] = lo;
}

// thread = (destination pixel, 4 consecutive channels).  gs, gprev: dense (B,H,W,C); off: view with 2 channels; ids: the sorted
// source pixels; cell_start: B (H+1) (W+1) + 1 entries.
template <int C>
__global__ __launch_bounds__(256) void iac_gather_kernel(const float* __restrict__ gs, View off, const unsigned* __restrict__ ids,
                                                         const unsigned* __restrict__ cell_start, int B, int H, int W, float* __restrict__ gprev) {
  constexpr int CQ = C / 4;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * H * W * CQ) return;
  const int cq = (int)(t % CQ);
  const long long pixg = t / CQ;
  const int xi = (int)(pixg % W);
  const int yi = (int)((pixg / W) % H);
  const int b = (int)(pixg / ((long long)W * H));
  // cells (yi + 1 - dy, xi + 1 - dx): the two of a row are neighbours, dx = 1 first in memory
  const unsigned* cs0 = cell_start + ((long long)b * (H + 1) + yi + 1) * (W + 1) + xi;      // dy = 0
  const unsigned* cs1 = cs0 - (W + 1);                                                      // dy = 1
  const unsigned e00[3] = {cs0[0], cs0[1], cs0[2]}, e10[3] = {cs1[0], cs1[1], cs1[2]};
  const float* offb = off.p + (long long)b * off.sb;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const unsigned beg = dy ? e10[1 - dx] : e00[1 - dx], end = dy ? e10[2 - dx] : e00[2 - dx];
      for (unsigned i = beg; i < end; ++i) {
        const unsigned src = ids[i];
        const int sx = (int)(src % (unsigned)W);
        const int sy = (int)((src / (unsigned)W) % (unsigned)H);
        // sampling position (same arithmetic as warp_kernel / iac_bwd_warp_kernel)
        const float* op = offb + (long long)sy * off.sy + (long long)sx * off.sx;
        const float fx = (float)sx + op[0];
        const float fy = (float)sy + op[off.sc];
        const float x0f = floorf(fx), y0f = floorf(fy);
        const float wx1 = fx - x0f, wy1 = fy - y0f;
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float w = (dy ? wy1 : wy0) * (dx ? wx1 : wx0);
        const float4 g = *reinterpret_cast<const float4*>(gs + (long long)src * C + cq * 4);
        a0 += w * g.x; a1 += w * g.y; a2 += w * g.z; a3 += w * g.w;
      }
    }
  *reinterpret_cast<float4*>(gprev + pixg * C + cq * 4) = make_float4(a0, a1, a2, a3);
}

namespace {

constexpr size_t kAlign = 256;
inline size_t up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct DetLayout {
  size_t gs, keys_in, keys_out, ids_in, ids_out, cell_start, sort_tmp, sort_bytes, total;
  unsigned npix, ncells, end_bit;
};

// false: the sizes do not fit (32-bit keys and pixel ids) or the sort's size query failed (err then holds its status)
bool det_layout(int B, int H, int W, int C, DetLayout& L, hipError_t& err) {
  err = hipSuccess;
  const long long npix = (long long)B * H * W, ncells = (long long)B * (H + 1) * (W + 1);
  if (B <= 0 || H <= 0 || W <= 0 || ncells >= 0x7fffffffLL) return false;
  L.npix = (unsigned)npix;
  L.ncells = (unsigned)ncells;
  L.end_bit = 1;
  while ((1ull << L.end_bit) < (unsigned long long)ncells + 1) ++L.end_bit;          // keys take the values 0 .. ncells
  L.sort_bytes = 0;
  err = rocprim::radix_sort_pairs(nullptr, L.sort_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                  (unsigned*)nullptr, L.npix, 0u, L.end_bit, (hipStream_t)0, false);
  if (err != hipSuccess) return false;
  size_t o = 0;
  L.gs = o;         o += up((size_t)npix * C * sizeof(float));
  L.keys_in = o;    o += up((size_t)npix * 4);
  L.keys_out = o;   o += up((size_t)npix * 4);
  L.ids_in = o;     o += up((size_t)npix * 4);
  L.ids_out = o;    o += up((size_t)npix * 4);
  L.cell_start = o; o += up(((size_t)ncells + 1) * 4);
  L.sort_tmp = o;   o += up(L.sort_bytes);
  L.total = o;
  return true;
}

}  // namespace
}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_iac_bwd_warp_det_workspace(int B, int H, int W, int C, size_t* bytes) {
  FCVSR_CHECK_ARG(bytes, "null pointer");
  FCVSR_CHECK_ARG(C == 32 || C == 64, "C in {32, 64}");
  DetLayout L;
  hipError_t err;
  if (!det_layout(B, H, W, C, L, err)) {
    if (err != hipSuccess) {
      set_error("%s: size query of the sort failed: %s", __func__, hipGetErrorString(err));
      return (int)err;
    }
    FCVSR_CHECK_ARG(false, "B, H, W must be positive and B (H+1) (W+1) must stay below 2^31 (32-bit cell keys)");
  }
  *bytes = L.total;
  return 0;
}

extern "C" int fcvsr_iac_bwd_warp_det(const float* gv, const fcvsr_view* k1, const float* prev, const fcvsr_view* off, int B, int H, int W, int C,
                                      float* gprev, float* goff, void* workspace, size_t workspace_bytes, void* stream) {
  FCVSR_CHECK_ARG(gv && prev && gprev && goff, "null pointer");
  FCVSR_CHECK_ARG((C == 32 || C == 64) && iac_k1_ok(k1, C), "C in {32, 64}; k1: f32 view with 3*C contiguous channels");
  FCVSR_CHECK_ARG(off && off->ptr && off->c >= 2 && off->dtype == FCVSR_F32, "off needs 2 f32 channels");
  FCVSR_CHECK_ARG(((uintptr_t)gprev % 16) == 0, "gprev must be 16-byte aligned");
  FCVSR_CHECK_ARG(workspace && ((uintptr_t)workspace % 16) == 0, "workspace: null or not 16-byte aligned");
  DetLayout L;
  hipError_t err;
  if (!det_layout(B, H, W, C, L, err)) {
    if (err != hipSuccess) {
      set_error("%s: size query of the sort failed: %s", __func__, hipGetErrorString(err));
      return (int)err;
    }
    FCVSR_CHECK_ARG(false, "B, H, W must be positive and B (H+1) (W+1) must stay below 2^31 (32-bit cell keys)");
  }
  FCVSR_CHECK_ARG(workspace_bytes >= L.total, "workspace smaller than fcvsr_iac_bwd_warp_det_workspace asks for");
  char* ws = (char*)workspace;
  float* gs = (float*)(ws + L.gs);
  unsigned *keys_in = (unsigned*)(ws + L.keys_in), *keys_out = (unsigned*)(ws + L.keys_out), *ids_in = (unsigned*)(ws + L.ids_in),
           *ids_out = (unsigned*)(ws + L.ids_out), *cell_start = (unsigned*)(ws + L.cell_start);
  hipStream_t st = (hipStream_t)stream;
  iac_bwd_warp_source_launch(gv, *k1, prev, *off, B, H, W, C, goff, gs, keys_in, ids_in, st);
  FCVSR_LAUNCH_CHECK();
  size_t sort_bytes = L.sort_bytes;
  err = rocprim::radix_sort_pairs((void*)(ws + L.sort_tmp), sort_bytes, (const unsigned*)keys_in, keys_out, (const unsigned*)ids_in, ids_out,
                                  L.npix, 0u, L.end_bit, st, false);
  if (err != hipSuccess) {
    set_error("%s: sort failed: %s", __func__, hipGetErrorString(err));
    return (int)err;
  }
  hipLaunchKernelGGL(iac_cell_start_kernel, dim3(cdiv((long long)L.ncells + 1, 256)), dim3(256), 0, st, (const unsigned*)keys_out, L.npix, L.ncells,
                     cell_start);
  const long long total = (long long)L.npix * (C / 4);
  if (C == 64)
    hipLaunchKernelGGL(iac_gather_kernel<64>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)gs, to_view(*off), (const unsigned*)ids_out,
                       (const unsigned*)cell_start, B, H, W, gprev);
  else
    hipLaunchKernelGGL(iac_gather_kernel<32>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)gs, to_view(*off), (const unsigned*)ids_out,
                       (const unsigned*)cell_start, B, H, W, gprev);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
