// Adam (torch.optim.Adam's L2 form: no amsgrad, no decoupled decay) over every parameter of a model in ONE launch.
//
// The gradients already live in one flat f32 buffer (train/step.py FlatGradAllReduce); the two moments live in two more with the same
// offsets, so the whole optimizer state is two tensors.  A device table (4 x int64 per parameter) maps blocks to parameters the way
// pack_weight_multi_kernel (train_ops.hip) maps them to weights.
//
// Arithmetic, all f32, every operation rounded once (the build passes -ffp-contract=off), in this order:
//     g' = g + wd * p
//     m' = m + (g' - m) * (1 - b1)
//     v' = v * b2 + (g' * g') * (1 - b2)
//     den = sqrt(v') / bc2_sqrt + eps
//     p' = p - step_size * (m' / den)
// `/` and sqrtf are the correctly rounded ones (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt) and f32 subnormals are
// kept (hipcc's default for gfx9: no flush), so the result equals fcvsr_amd/train/optim.py adam_step_host bit for bit.
//
// Traffic: 16 B read (p, g, m, v) and 12 B written (p, m, v) per element; no atomics, no LDS.
#include "common.h"

namespace fcvsr {

// table row: {parameter pointer (f32, contiguous, 16-byte aligned), offset of the parameter in the flat buffers (elements),
// element count, first block}; a block updates kAdamElems consecutive elements of its parameter.
constexpr int kAdamElems = 2048;
constexpr int kAdamThreads = 256;

struct AdamScalars {
  float one_minus_b1, b2, one_minus_b2, eps, wd, step_size, bc2_sqrt;
};

__device__ __forceinline__ void adam_one(float& p, const float g, float& m, float& v, const AdamScalars& s) {
  const float wp = s.wd * p;
  const float g1 = g + wp;
  const float d = g1 - m;
  const float dm = d * s.one_minus_b1;
  const float m1 = m + dm;
  const float vb = v * s.b2;
  const float gg = g1 * g1;
  const float gs = gg * s.one_minus_b2;
  const float v1 = vb + gs;
  const float r = sqrtf(v1);
  const float q = r / s.bc2_sqrt;
  const float den = q + s.eps;
  const float u = m1 / den;
  const float su = s.step_size * u;
  p = p - su;
  m = m1;
  v = v1;
}

__global__ __launch_bounds__(kAdamThreads) void adam_multi_kernel(const long long* __restrict__ tab, int n_items,
                                                                   const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                   float* __restrict__ exp_avg_sq, AdamScalars s) {
  int lo = 0, hi = n_items - 1;
  while (lo < hi) {                                        // last item whose first block is <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid * 4 + 3] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const long long* it = tab + lo * 4;
  float* __restrict__ p = reinterpret_cast<float*>(it[0]);
  const long long off = it[1], count = it[2];
  const long long e0 = ((long long)blockIdx.x - it[3]) * kAdamElems;
  if (e0 < 0 || e0 >= count) return;                       // (a table whose block counts are too large: nothing to do)
  const int n = (int)(count - e0 < kAdamElems ? count - e0 : kAdamElems);
  p += e0;
  const float* __restrict__ g = grad + off + e0;
  float* __restrict__ m = exp_avg + off + e0;
  float* __restrict__ v = exp_avg_sq + off + e0;
  // e0 is a multiple of kAdamElems and the parameter is 16-byte aligned: the block's slice of the flat buffers is 16-byte
  // aligned exactly when the parameter's flat offset is a multiple of 4
  int done = 0;
  if ((off & 3) == 0) {
    const int n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
#pragma unroll
    for (int k = 0; k < kAdamElems / 4 / kAdamThreads; ++k) {
      const int i = k * kAdamThreads + (int)threadIdx.x;
      if (i < n4) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam_one(pp.x, gg.x, mm.x, vv.x, s);
        adam_one(pp.y, gg.y, mm.y, vv.y, s);
        adam_one(pp.z, gg.z, mm.z, vv.z, s);
        adam_one(pp.w, gg.w, mm.w, vv.w, s);
        p4[i] = pp;
        m4[i] = mm;
        v4[i] = vv;
      }
    }
    done = n4 << 2;                                        // the n % 4 tail goes one element per lane below
  }
  // (the loop vectoriser would pair two iterations of this loop into packed-FP32 instructions, which no code object of this
  // library may contain: build.py)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int i = done + (int)threadIdx.x; i < n; i += kAdamThreads) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_one(pp, g[i], mm, vv, s);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

}  // namespace fcvsr

using namespace fcvsr;

extern "C" int fcvsr_adam_multi_block_elems(void) { return kAdamElems; }

/* One Adam step t over n_items parameters.  tab (device memory, 4 x int64 per item): parameter pointer (f32, contiguous, 16-byte
 * aligned), offset of the parameter in grad / exp_avg / exp_avg_sq (elements), element count, first block; item i owns the blocks
 * [first_i, first_i + ceil(count_i / fcvsr_adam_multi_block_elems())); total_blocks = their sum.  The caller rounds the scalars
 * once from f64: step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t). */
extern "C" int fcvsr_adam_multi(const long long* tab, int n_items, int total_blocks, const float* grad, float* exp_avg,
                                float* exp_avg_sq, int t, float step_size, float bc2_sqrt, float one_minus_b1, float b2,
                                float one_minus_b2, float eps, float wd, void* stream) {
  FCVSR_CHECK_ARG(tab && grad && exp_avg && exp_avg_sq, "null pointer");
  FCVSR_CHECK_ARG(n_items >= 1 && total_blocks >= n_items, "empty table");
  FCVSR_CHECK_ARG(t >= 1, "the step count starts at 1");
  FCVSR_CHECK_ARG(((uintptr_t)grad % 16) == 0 && ((uintptr_t)exp_avg % 16) == 0 && ((uintptr_t)exp_avg_sq % 16) == 0,
                  "flat buffers 16-byte aligned");
  AdamScalars s;
  s.one_minus_b1 = one_minus_b1; s.b2 = b2; s.one_minus_b2 = one_minus_b2; s.eps = eps; s.wd = wd;
  s.step_size = step_size; s.bc2_sqrt = bc2_sqrt;
  hipLaunchKernelGGL(adam_multi_kernel, dim3(total_blocks), dim3(kAdamThreads), 0, (hipStream_t)stream, tab, n_items, grad,
                     exp_avg, exp_avg_sq, s);
  FCVSR_LAUNCH_CHECK();
  return 0;
}
