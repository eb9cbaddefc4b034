// One ConvBlk head of MGAAbk (reference CVSR_freq.py:344-357, applied at :1494-1498) on the 4-channel offset spectra:
//     u   = conv2( PReLU( conv1(x) ) )                  k x k, 4 -> 4, no bias, k = 2*index+1
//     out = (CA(u) + u) * sim                           CALayer(4, reduction 1, no bias), split into (real, imag) planes
// in two launches instead of six (conv1, conv2, 2-stage channel sums, gate, tail): the tensors are tiny (16 bytes per
// pixel), so the stand-alone launches were pure latency.
//   1. convblk_conv_kernel<K>: 16 x 16 output pixels per workgroup; the input tile with a 2*(K/2) halo and the PReLU'd
//      intermediate with a K/2 halo live in LDS (zero padding of BOTH convolutions reproduced: the intermediate is zero outside
//      the image); weights are wave-uniform scalar loads; per-workgroup channel sums of u in a fixed tree order.
//   2. convblk_tail_kernel2: every workgroup first reduces the partial sums of its batch item (fixed order) and evaluates the
//      4 -> 4 -> 4 gate, then applies it.  Deterministic: no atomics anywhere.
#include "common.h"

namespace fcvsr {

constexpr int kCbT = 16;                                  // output tile side

template <int K>
__global__ __launch_bounds__(256) void convblk_conv_kernel(const float4* x, const float* __restrict__ w1,
                                                           const float* __restrict__ w2, const float* slope_p, float4* u,
                                                           float4* partial, int H, int W, int tiles_x, int tiles_y) {
  constexpr int P = K / 2;
  constexpr int XS = kCbT + 4 * P, TT = kCbT + 2 * P;
  __shared__ float4 xs[XS * XS];
  __shared__ float4 ts[TT * TT];
  __shared__ float4 red[256];
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * kCbT, tx0 = (blockIdx.x % tiles_x) * kCbT;
  const float4* xn = x + (long long)n * H * W;
  const float slope = slope_p[0];
  for (int idx = tid; idx < XS * XS; idx += 256) {
    const int yy = idx / XS, xx = idx - yy * XS;
    const int gy = ty0 - 2 * P + yy, gx = tx0 - 2 * P + xx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xn[(long long)gy * W + gx];
    xs[idx] = v;
  }
  __syncthreads();
  // weights: [tap][cin][16] f32 (cout padded to 16 by pack_conv_weight); uniform addresses -> scalar loads
  for (int idx = tid; idx < TT * TT; idx += 256) {
    const int yy = idx / TT, xx = idx - yy * TT;
    const int gy = ty0 - P + yy, gx = tx0 - P + xx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const float4 v = xs[(yy + ky) * XS + xx + kx];
          const float* wt = w1 + (ky * K + kx) * 64;
          const float vi[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) {
            a0 = fmaf(vi[ci], wt[ci * 16 + 0], a0); a1 = fmaf(vi[ci], wt[ci * 16 + 1], a1);
            a2 = fmaf(vi[ci], wt[ci * 16 + 2], a2); a3 = fmaf(vi[ci], wt[ci * 16 + 3], a3);
          }
        }
      }
      a0 = a0 >= 0.f ? a0 : a0 * slope; a1 = a1 >= 0.f ? a1 : a1 * slope;
      a2 = a2 >= 0.f ? a2 : a2 * slope; a3 = a3 >= 0.f ? a3 : a3 * slope;
    }
    ts[idx] = make_float4(a0, a1, a2, a3);                // zero outside the image = zero padding of conv2
  }
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  const int gy = ty0 + ly, gx = tx0 + lx;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gy < H && gx < W) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const float4 v = ts[(ly + ky) * TT + lx + kx];
        const float* wt = w2 + (ky * K + kx) * 64;
        const float vi[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          a0 = fmaf(vi[ci], wt[ci * 16 + 0], a0); a1 = fmaf(vi[ci], wt[ci * 16 + 1], a1);
          a2 = fmaf(vi[ci], wt[ci * 16 + 2], a2); a3 = fmaf(vi[ci], wt[ci * 16 + 3], a3);
        }
      }
    }
    o = make_float4(a0, a1, a2, a3);
    u[((long long)n * H + gy) * W + gx] = o;
  }
  red[tid] = o;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      const float4 p = red[tid], q = red[tid + st];
      red[tid] = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
    }
    __syncthreads();
  }
  if (tid == 0) partial[(long long)n * gridDim.x + blockIdx.x] = red[0];
}

// out = (u*gate + u) * sim -> (real, imag) planes; gate = sigmoid(W2 relu(W1 mean(u)))  (CALayer :1812-1828, C = CR = 4)
__global__ __launch_bounds__(256) void convblk_tail_kernel2(const float4* u, const float4* partial, int nblk, float inv_hw,
                                                            const float* ca_w1, const float* ca_w2, const float4* sim, int B,
                                                            long long HW, float* spec, long long ps, int re_off, int im_off,
                                                            int g_stride, int g0) {
  __shared__ float4 red[256];
  __shared__ float gate_s[4];
  const int tid = threadIdx.x;
  const int bn = blockIdx.y;                              // dir * B + b
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = tid; k < nblk; k += 256) {
    const float4 p = partial[(long long)bn * nblk + k];
    s = make_float4(s.x + p.x, s.y + p.y, s.z + p.z, s.w + p.w);
  }
  red[tid] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      const float4 p = red[tid], q = red[tid + st];
      red[tid] = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
    }
    __syncthreads();
  }
  if (tid < 4) {
    const float4 t = red[0];
    const float mean[4] = {t.x * inv_hw, t.y * inv_hw, t.z * inv_hw, t.w * inv_hw};
    float hid[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) a = fmaf(ca_w1[h * 4 + c], mean[c], a);
      hid[h] = fmaxf(a, 0.f);
    }
    float a = 0.f;
#pragma unroll
    for (int h = 0; h < 4; ++h) a = fmaf(ca_w2[tid * 4 + h], hid[h], a);
    gate_s[tid] = 1.f / (1.f + expf(-a));
  }
  __syncthreads();
  const long long pix = (long long)blockIdx.x * 256 + tid;
  if (pix >= HW) return;
  const int dir = bn / B, b = bn - dir * B;
  const float4 uu = u[(long long)bn * HW + pix];
  const float4 ss = sim[(long long)b * HW + pix];
  const float o0 = fmaf(uu.x, gate_s[0], uu.x) * ss.x;
  const float o1 = fmaf(uu.y, gate_s[1], uu.y) * ss.y;
  const float o2 = fmaf(uu.z, gate_s[2], uu.z) * ss.z;
  const float o3 = fmaf(uu.w, gate_s[3], uu.w) * ss.w;
  float* px = spec + ((long long)b * HW + pix) * ps;
  const int gi = (g0 + dir * g_stride) * 2;
  if (((ps | re_off | im_off) & 1) == 0 && (reinterpret_cast<uintptr_t>(spec) & 7) == 0) {   // gi is even: 8-byte pairs
    *reinterpret_cast<float2*>(px + re_off + gi) = make_float2(o0, o1);
    *reinterpret_cast<float2*>(px + im_off + gi) = make_float2(o2, o3);
  } else {
    px[re_off + gi] = o0;
    px[re_off + gi + 1] = o1;
    px[im_off + gi] = o2;
    px[im_off + gi + 1] = o3;
  }
}

// ---- all A heads of one MGAA call in two launches ---------------------------------------------------------------------------
// Head i has k = 2i+1.  The conv launch stages the x tile once with the halo of the largest head and runs the heads one after
// the other (per head exactly the arithmetic of convblk_conv_kernel<2i+1>: same FMA order, same 256-value tree); the tail
// launch evaluates all 2A gates, reads sim once and stores whole [re: 4A | im: 4A] records.
constexpr int kCbMaxHeads = 6;
// The weights are read-only for the whole launch.  Read through the constant address space they stay wave-uniform scalar loads
// in every head; as plain global pointers the loads that follow an earlier head's stores of u come out as vector loads.
typedef const __attribute__((address_space(4))) float cb_cfloat_t;
__device__ __forceinline__ cb_cfloat_t* cb_const(const float* p) { return reinterpret_cast<cb_cfloat_t*>(reinterpret_cast<uintptr_t>(p)); }

struct ConvBlkHeadsArgs {
  const float* w1[kCbMaxHeads];
  const float* w2[kCbMaxHeads];
  const float* slope[kCbMaxHeads];
  const float* ca_w1[kCbMaxHeads];
  const float* ca_w2[kCbMaxHeads];
};

// xs: the x tile with halo 2*(A-1), side 16 + 4*(A-1); ts / red as in convblk_conv_kernel
template <int A, int I>
__device__ __forceinline__ void convblk_one_head(const float4* xs, float4* ts, float4* red, cb_cfloat_t* w1, cb_cfloat_t* w2, float slope, float4* __restrict__ un,
                                                 float4* __restrict__ partial_out, int H, int W, int ty0, int tx0, int tid) {
  constexpr int K = 2 * I + 1, P = I;
  constexpr int XS = kCbT + 4 * (A - 1), TT = kCbT + 2 * P;
  constexpr int D = 2 * (A - 1) - 2 * P;                  // this head's 2P halo starts D pixels inside the staged one
  for (int idx = tid; idx < TT * TT; idx += 256) {
    const int yy = idx / TT, xx = idx - yy * TT;
    const int gy = ty0 - P + yy, gx = tx0 - P + xx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const float4 v = xs[(yy + ky + D) * XS + xx + kx + D];
          cb_cfloat_t* wt = w1 + (ky * K + kx) * 64;
          const float vi[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) {
            a0 = fmaf(vi[ci], wt[ci * 16 + 0], a0); a1 = fmaf(vi[ci], wt[ci * 16 + 1], a1);
            a2 = fmaf(vi[ci], wt[ci * 16 + 2], a2); a3 = fmaf(vi[ci], wt[ci * 16 + 3], a3);
          }
        }
      }
      a0 = a0 >= 0.f ? a0 : a0 * slope; a1 = a1 >= 0.f ? a1 : a1 * slope;
      a2 = a2 >= 0.f ? a2 : a2 * slope; a3 = a3 >= 0.f ? a3 : a3 * slope;
    }
    ts[idx] = make_float4(a0, a1, a2, a3);
  }
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  const int gy = ty0 + ly, gx = tx0 + lx;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gy < H && gx < W) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const float4 v = ts[(ly + ky) * TT + lx + kx];
        cb_cfloat_t* wt = w2 + (ky * K + kx) * 64;
        const float vi[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          a0 = fmaf(vi[ci], wt[ci * 16 + 0], a0); a1 = fmaf(vi[ci], wt[ci * 16 + 1], a1);
          a2 = fmaf(vi[ci], wt[ci * 16 + 2], a2); a3 = fmaf(vi[ci], wt[ci * 16 + 3], a3);
        }
      }
    }
    o = make_float4(a0, a1, a2, a3);
    un[(long long)gy * W + gx] = o;
  }
  red[tid] = o;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      const float4 p = red[tid], q = red[tid + st];
      red[tid] = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
    }
    __syncthreads();                                      // the last one also frees ts and red for the next head
  }
  if (tid == 0) *partial_out = red[0];
}

template <int A, int I>
__device__ __forceinline__ void convblk_heads_from(const float4* xs, float4* ts, float4* red, const ConvBlkHeadsArgs& a, float4* u,
                                                   float4* partial, int N, int n, int H, int W, int ty0, int tx0, int tid) {
  // u: [A][N][H][W], partial: [A][N][tiles]
  convblk_one_head<A, I>(xs, ts, red, cb_const(a.w1[I]), cb_const(a.w2[I]), cb_const(a.slope[I])[0], u + ((long long)I * N + n) * H * W,
                         partial + ((long long)I * N + n) * gridDim.x + blockIdx.x, H, W, ty0, tx0, tid);
  if constexpr (I + 1 < A) convblk_heads_from<A, I + 1>(xs, ts, red, a, u, partial, N, n, H, W, ty0, tx0, tid);
}

template <int A>
__global__ __launch_bounds__(256) void convblk_heads_conv_kernel(const float4* x, ConvBlkHeadsArgs a, float4* u, float4* partial,
                                                                 int N, int H, int W, int tiles_x) {
  constexpr int PM = 2 * (A - 1);
  constexpr int XS = kCbT + 2 * PM, TT = kCbT + PM;
  __shared__ float4 xs[XS * XS];
  __shared__ float4 ts[TT * TT];
  __shared__ float4 red[256];
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * kCbT, tx0 = (blockIdx.x % tiles_x) * kCbT;
  const float4* xn = x + (long long)n * H * W;
  for (int idx = tid; idx < XS * XS; idx += 256) {
    const int yy = idx / XS, xx = idx - yy * XS;
    const int gy = ty0 - PM + yy, gx = tx0 - PM + xx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xn[(long long)gy * W + gx];
    xs[idx] = v;
  }
  __syncthreads();
  convblk_heads_from<A, 0>(xs, ts, red, a, u, partial, N, n, H, W, ty0, tx0, tid);
}

// thread = spectrum pixel of batch item blockIdx.y: gates of all 2A (dir, head) pairs (per pair the sums and the gate of
// convblk_tail_kernel2, the 2A trees side by side), then the whole record of the pixel
template <int A>
__global__ __launch_bounds__(256) void convblk_heads_tail_kernel(const float4* __restrict__ u, const float4* __restrict__ partial,
                                                                 int nblk, float inv_hw, ConvBlkHeadsArgs a,
                                                                 const float4* __restrict__ sim, int B, long long HW,
                                                                 float* __restrict__ spec, long long ps, int re_off, int im_off) {
  constexpr int NP = 2 * A;                               // pair p = dir * A + i: channels 2p, 2p+1 of the re and im blocks
  __shared__ float4 red[NP][256];
  __shared__ float gate_s[NP][4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const long long pix = (long long)blockIdx.x * 256 + tid;
  const bool live = pix < HW;
  // the pixel's own reads go out first: they do not depend on the gates
  float4 uu[NP], ss = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const long long bn = (long long)(p % A) * 2 * B + (p / A) * B + b;
    uu[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) uu[p] = u[bn * HW + pix];
  }
  if (live) ss = sim[(long long)b * HW + pix];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const long long bn = (long long)(p % A) * 2 * B + (p / A) * B + b;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = tid; k < nblk; k += 256) {
      const float4 q = partial[bn * nblk + k];
      s = make_float4(s.x + q.x, s.y + q.y, s.z + q.z, s.w + q.w);
    }
    red[p][tid] = s;
  }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const float4 q0 = red[p][tid], q1 = red[p][tid + st];
        red[p][tid] = make_float4(q0.x + q1.x, q0.y + q1.y, q0.z + q1.z, q0.w + q1.w);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if ((tid >> 2) == p) {
      const float* ca_w1 = a.ca_w1[p % A];
      const float* ca_w2 = a.ca_w2[p % A];
      const int row = tid & 3;
      const float4 t = red[p][0];
      const float mean[4] = {t.x * inv_hw, t.y * inv_hw, t.z * inv_hw, t.w * inv_hw};
      float hid[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = fmaf(ca_w1[h * 4 + c], mean[c], acc);
        hid[h] = fmaxf(acc, 0.f);
      }
      float acc = 0.f;
#pragma unroll
      for (int h = 0; h < 4; ++h) acc = fmaf(ca_w2[row * 4 + h], hid[h], acc);
      gate_s[p][row] = 1.f / (1.f + expf(-acc));
    }
  }
  __syncthreads();
  if (!live) return;
  float o[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    o[p][0] = fmaf(uu[p].x, gate_s[p][0], uu[p].x) * ss.x;
    o[p][1] = fmaf(uu[p].y, gate_s[p][1], uu[p].y) * ss.y;
    o[p][2] = fmaf(uu[p].z, gate_s[p][2], uu[p].z) * ss.z;
    o[p][3] = fmaf(uu[p].w, gate_s[p][3], uu[p].w) * ss.w;
  }
  float* px = spec + ((long long)b * HW + pix) * ps;
#pragma unroll
  for (int q = 0; q < A; ++q)
    *reinterpret_cast<float4*>(px + re_off + 4 * q) = make_float4(o[2 * q][0], o[2 * q][1], o[2 * q + 1][0], o[2 * q + 1][1]);
#pragma unroll
  for (int q = 0; q < A; ++q)
    *reinterpret_cast<float4*>(px + im_off + 4 * q) = make_float4(o[2 * q][2], o[2 * q][3], o[2 * q + 1][2], o[2 * q + 1][3]);
}

template <int A>
static void launch_convblk_heads(hipStream_t st, const float4* x, const ConvBlkHeadsArgs& a, float4* u, float4* partial,
                                 const float4* sim, int B, int H, int W, float* spec, long long ps, int re_off, int im_off) {
  const int tx = cdiv(W, kCbT), ty = cdiv(H, kCbT);
  const int nblk = tx * ty, N = 2 * B;
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(convblk_heads_conv_kernel<A>, dim3(nblk, N), dim3(256), 0, st, x, a, u, partial, N, H, W, tx);
  hipLaunchKernelGGL(convblk_heads_tail_kernel<A>, dim3(cdiv(HW, 256), B), dim3(256), 0, st, (const float4*)u,
                     (const float4*)partial, nblk, 1.0f / (float)HW, a, sim, B, HW, spec, ps, re_off, im_off);
}

template <int K>
static void launch_convblk_conv(dim3 grid, hipStream_t st, const float4* x, const float* w1, const float* w2, const float* slope,
                                float4* u, float4* partial, int H, int W, int tx, int ty) {
  hipLaunchKernelGGL(convblk_conv_kernel<K>, grid, dim3(256), 0, st, x, w1, w2, slope, u, partial, H, W, tx, ty);
}

}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_convblk(const float* x, const float* w1, const float* w2, const float* prelu_slope, int ksize,
                             const float* ca_w1, const float* ca_w2, const float* sim, int B, int ndir, int H, int Wf,
                             float* u_scratch, float* partial_scratch, int64_t partial_elems, float* spec, int64_t pix_stride,
                             int re_off, int im_off, int g_stride, int g0, void* stream) {
  FCVSR_CHECK_ARG(x && w1 && w2 && prelu_slope && ca_w1 && ca_w2 && sim && u_scratch && partial_scratch && spec, "null pointer");
  FCVSR_CHECK_ARG(B > 0 && ndir > 0 && H > 0 && Wf > 0, "bad sizes");
  FCVSR_CHECK_ARG(ksize % 2 == 1 && ksize >= 1 && ksize <= 11, "kernel size: odd, 1..11");
  FCVSR_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)u_scratch % 16) == 0 && ((uintptr_t)sim % 16) == 0 &&
                      ((uintptr_t)partial_scratch % 16) == 0, "16-byte alignment");
  const int tx = cdiv(Wf, kCbT), ty = cdiv(H, kCbT);
  const int nblk = tx * ty, N = ndir * B;
  FCVSR_CHECK_ARG(partial_elems >= 4ll * N * nblk, "partial scratch too small");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(nblk, N);
  const float4* x4 = (const float4*)x;
  float4* u4 = (float4*)u_scratch;
  float4* p4 = (float4*)partial_scratch;
  switch (ksize) {
    case 1: launch_convblk_conv<1>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
    case 3: launch_convblk_conv<3>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
    case 5: launch_convblk_conv<5>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
    case 7: launch_convblk_conv<7>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
    case 9: launch_convblk_conv<9>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
    default: launch_convblk_conv<11>(grid, st, x4, w1, w2, prelu_slope, u4, p4, H, Wf, tx, ty); break;
  }
  FCVSR_LAUNCH_CHECK();
  const long long HW = (long long)H * Wf;
  hipLaunchKernelGGL(convblk_tail_kernel2, dim3(cdiv(HW, 256), N), dim3(256), 0, st, (const float4*)u4, (const float4*)p4, nblk,
                     1.0f / (float)HW, ca_w1, ca_w2, (const float4*)sim, B, HW, spec, (long long)pix_stride, re_off, im_off,
                     g_stride, g0);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_convblk_heads(const float* x, int n_heads, const float* const* w1, const float* const* w2,
                                   const float* const* prelu_slope, const float* const* ca_w1, const float* const* ca_w2,
                                   const float* sim, int B, int H, int Wf, float* u, float* partial, int64_t partial_elems,
                                   float* spec, int64_t pix_stride, int re_off, int im_off, void* stream) {
  FCVSR_CHECK_ARG(x && w1 && w2 && prelu_slope && ca_w1 && ca_w2 && sim && u && partial && spec, "null pointer");
  FCVSR_CHECK_ARG(n_heads >= 1 && n_heads <= kCbMaxHeads, "heads: 1..6");
  FCVSR_CHECK_ARG(B > 0 && H > 0 && Wf > 0, "bad sizes");
  FCVSR_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)u % 16) == 0 && ((uintptr_t)sim % 16) == 0 &&
                      ((uintptr_t)partial % 16) == 0 && ((uintptr_t)spec % 16) == 0, "16-byte alignment");
  FCVSR_CHECK_ARG(pix_stride % 4 == 0 && re_off % 4 == 0 && im_off % 4 == 0 && re_off >= 0 && im_off >= 0 &&
                      re_off + 4 * n_heads <= pix_stride && im_off + 4 * n_heads <= pix_stride &&
                      (re_off + 4 * n_heads <= im_off || im_off + 4 * n_heads <= re_off), "record: two disjoint 16-byte aligned blocks");
  const long long nblk = (long long)cdiv(Wf, kCbT) * cdiv(H, kCbT);
  FCVSR_CHECK_ARG(partial_elems >= 4ll * n_heads * 2 * B * nblk, "partial scratch too small");
  ConvBlkHeadsArgs a = {};
  for (int i = 0; i < n_heads; ++i) {
    FCVSR_CHECK_ARG(w1[i] && w2[i] && prelu_slope[i] && ca_w1[i] && ca_w2[i], "null head pointer");
    a.w1[i] = w1[i]; a.w2[i] = w2[i]; a.slope[i] = prelu_slope[i]; a.ca_w1[i] = ca_w1[i]; a.ca_w2[i] = ca_w2[i];
  }
  hipStream_t st = (hipStream_t)stream;
  const float4* x4 = (const float4*)x;
  const float4* s4 = (const float4*)sim;
  float4* u4 = (float4*)u;
  float4* p4 = (float4*)partial;
  const long long ps = (long long)pix_stride;
  switch (n_heads) {
    case 1: launch_convblk_heads<1>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
    case 2: launch_convblk_heads<2>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
    case 3: launch_convblk_heads<3>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
    case 4: launch_convblk_heads<4>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
    case 5: launch_convblk_heads<5>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
    default: launch_convblk_heads<6>(st, x4, a, u4, p4, s4, B, H, Wf, spec, ps, re_off, im_off); break;
  }
  FCVSR_LAUNCH_CHECK();
  return 0;
}
