// The MATLAB-style bicubic resizers (imresize, a = -0.5, symmetric border) at scale 2 or 4: the reference's
// mmedit/datasets/pipelines/matlab_like_resize.py MATLABLikeResize.  The contracts are fcvsr_amd/harness/niqe.py bicubic_upscale and
// bicubic_downscale.  Both have the reference's arithmetic and so its bits: every pass reads f32, every tap's product is an f32 and
// the products are added in tap order in f32 (no FMA: the library is built with -ffp-contract=off).
//
// Up-scale (the "Bicubic" row of SR tables).
// Output o of an axis has its centre at c = (o + 0.5) / F - 0.5 and reads the inputs floor(c) - 1 .. floor(c) + 2, reflected with
// edge repeat, with the weights cubic(c - i): they depend on o mod F only and are exact in f32 (UpTaps below).  The reference runs
// two passes (rows, then columns) through an f64 buffer that holds f32 values; here both passes are one launch and the intermediate
// stays in registers, with the same roundings: for one output row the vertical f32 sum of every source column (products added in
// tap order), then the horizontal f32 sum of four of those.
//
// A pure streaming kernel that writes F^2 times what it reads, so it is shaped for the stores.  A thread owns 4 consecutive, 4-aligned
// outputs of a row (one input column at 4x, two at 2x): one 16-byte store for f32, 8 bytes for uint16, 4 for uint8, and consecutive
// lanes write consecutive groups.  The aligned group 4q .. 4q+3 straddles two source-column groups (outputs 4m+2 .. 4m+5 share
// their four columns), so a thread holds the 5 (4x) or 6 (2x) columns its outputs touch.  It makes the F output rows F n + F/2 ..
// F n + 3F/2 - 1, which share their four source rows n-1 .. n+2 (n = -1 .. H-1: the first and last row group are half outside and
// skip those rows), so the 4 x 5 samples are loaded once for 16 outputs.  The loads hit L1 / L2 (neighbours share columns); no LDS,
// no atomics, no scratch.  At 2x with an odd W a row is 2 W = 4k + 2 outputs long: rows are then not 4-aligned and the last thread
// of a row owns one column, so that shape takes scalar stores.
//
// Down-scale (antialiased; NIQE and BRISQUE need it between their two scales).  Output i of an axis reads the 4 F inputs from
// F i + F/2 - 2F with the weights cubic(x / F) / F (Taps below), reflected the same way.  One launch makes both passes: a workgroup
// brings the inputs of 8 x 32 outputs to LDS, makes the row pass there and the column pass from it.  fcvsr_bicubic_downscale runs
// it on uint8 / f32 planes; downscale2_f64 (resize.h) is the 2x form on the f64 planes of integers of the scores.
//
// Any size (fcvsr_imresize; the contract is fcvsr_amd/harness/resize.py imresize_host).  The same operator with scale= or
// output_shape= free: the taps are no longer constants but two per-axis tables (f32 weights and the first, unreflected input of every
// output) that the host computes with the reference's arithmetic and uploads once per size.  One launch, table-driven, both passes
// through an LDS tile, the axis with the smaller scale first (rows on a tie) - see imresize_kernel below.  The rule is the same
// everywhere: f32 products added in TAP ORDER.  The reference itself leaves that order in one degenerate class - a pass of 8 or
// more stored taps over a plane whose other extent is 1, where numpy collapses the axes and sums pairwise in blocks of 8, 1 ulp
// away; the contract and this kernel keep tap order there too.
#include "bicubic_up.h"
#include "resize.h"

namespace {

// the taps, the border rule, the sample reads and the rounding of the up-scale: shared with active.hip
using namespace fcvsr::bicubic_up;

// (H + 1) * Wq threads per plane (blockIdx.y), Wq = ceil(W / CPT): thread (n + 1, q) makes output rows F n + F/2 + j (j < F) x output
// columns 4q .. 4q+3.
template <int F, class TI, class TO>
__global__ __launch_bounds__(256) void upscale_kernel(const TI* __restrict__ src, int H, int W, TO* __restrict__ dst) {
  constexpr int CPT = 4 / F, NC = CPT + 4;                  // input columns a thread owns; source columns it reads: m0-2 .. m0+CPT+1
  const int Wq = (W + CPT - 1) / CPT, Ho = F * H, Wo = F * W;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)(H + 1) * (unsigned)Wq) return;
  const int q = (int)(t % (unsigned)Wq);
  const int n = (int)(t / (unsigned)Wq) - 1;
  const long long p = blockIdx.y;
  const TI* sp = src + p * H * W;
  const int m0 = q * CPT;
  int cx[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) cx[k] = reflect(m0 - 2 + k, W);
  float v[4][NC];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = (long long)reflect(n - 1 + r, H) * W;
#pragma unroll
    for (int k = 0; k < NC; ++k) v[r][k] = up_sample(sp, row + cx[k]);
  }
  const bool vec = (W % CPT) == 0;                          // every row 4-aligned and whole (always at 4x)
#pragma unroll
  for (int j = 0; j < F; ++j) {
    const int oy = F * n + F / 2 + j, py = (F / 2 + j) % F;
    if (oy < 0 || oy >= Ho) continue;
    float s[NC];                                            // the row pass of the contract at output row oy, per source column
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      float a = UpTaps<F>::w(py, 0) * v[0][k];
#pragma unroll
      for (int r = 1; r < 4; ++r) a = a + UpTaps<F>::w(py, r) * v[r][k];
      s[k] = a;
    }
    TO o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int px = i % F, k0 = i / F + (px >= F / 2 ? 1 : 0);   // output 4q + i = F (m0 + i / F) + px reads s[k0 .. k0+3]
      float a = UpTaps<F>::w(px, 0) * s[k0];
#pragma unroll
      for (int k = 1; k < 4; ++k) a = a + UpTaps<F>::w(px, k) * s[k0 + k];
      up_result(a, o[i]);
    }
    TO* dp = dst + p * Ho * Wo + (long long)oy * Wo + 4 * q;
    if (vec) {
      up_store4(dp, o);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * q + i < Wo) dp[i] = o[i];
    }
  }
}

template <int F, class TI, class TO>
void launch_upscale(const void* src, long long planes, int H, int W, void* dst, hipStream_t stream) {
  const long long per_plane = (long long)(H + 1) * ((W + 4 / F - 1) / (4 / F));
  for (long long p0 = 0; p0 < planes; p0 += 65535) {        // grid.y holds 65535 planes
    const long long np = planes - p0 < 65535 ? planes - p0 : 65535;
    hipLaunchKernelGGL((upscale_kernel<F, TI, TO>), dim3((unsigned)((per_plane + 255) / 256), (unsigned)np), dim3(256), 0, stream,
                       (const TI*)src + p0 * H * W, H, W, (TO*)dst + p0 * H * W * F * F);
  }
}

template <int F>
void dispatch_upscale(const void* src, int src_dtype, long long planes, int H, int W, void* out, int out_dtype, hipStream_t st) {
  if (src_dtype == FCVSR_U8) {
    if (out_dtype == FCVSR_U8) launch_upscale<F, unsigned char, unsigned char>(src, planes, H, W, out, st);
    else launch_upscale<F, unsigned char, float>(src, planes, H, W, out, st);
  } else if (src_dtype == FCVSR_U16) {
    if (out_dtype == FCVSR_U16) launch_upscale<F, unsigned short, unsigned short>(src, planes, H, W, out, st);
    else launch_upscale<F, unsigned short, float>(src, planes, H, W, out, st);
  } else {
    launch_upscale<F, float, float>(src, planes, H, W, out, st);
  }
}

// antialiased cubic taps cubic(x / F) / F: multiples of 1/256 (2x) and 1/4096 (4x), exact in f32
template <int F> struct Taps;
template <> struct Taps<2> {
  static constexpr int K = 8;
  __device__ static float w(int k) {
    constexpr float t[8] = {-3.f / 256, -9.f / 256, 29.f / 256, 111.f / 256, 111.f / 256, 29.f / 256, -9.f / 256, -3.f / 256};
    return t[k];
  }
};
template <> struct Taps<4> {
  static constexpr int K = 16;
  __device__ static float w(int k) {
    constexpr float t[16] = {-7.f / 4096,  -45.f / 4096, -75.f / 4096, -49.f / 4096, 93.f / 4096,  399.f / 4096, 745.f / 4096, 987.f / 4096,
                             987.f / 4096, 745.f / 4096, 399.f / 4096, 93.f / 4096,  -49.f / 4096, -75.f / 4096, -45.f / 4096, -7.f / 4096};
    return t[k];
  }
};

constexpr int kOY = 8, kOX = 32;
enum { SRC_U8 = 0, SRC_F32 = 1, SRC_NIQE = 2 };   // SRC_NIQE: f64 plane of integers, read as f32(v / 255), stored as f64 * 255

// One launch, both passes: a workgroup makes kOY x kOX outputs of one plane.  Rows first (dim 0), then columns; every pass's input
// is an f32, products are f32 and are added in tap order.
template <int F, int MODE>
__global__ __launch_bounds__(256) void downscale_kernel(const void* __restrict__ src, int H, int W, void* __restrict__ dst) {
  constexpr int K = Taps<F>::K, first = F / 2 - K / 2;      // tap 0 of output i reads input F i + first
  constexpr int IY = (kOY - 1) * F + K, IX = (kOX - 1) * F + K;
  __shared__ float in[IY][IX];
  __shared__ float mid[kOY][IX];
  const int Ho = H / F, Wo = W / F;
  const int oy0 = blockIdx.y * kOY, ox0 = blockIdx.x * kOX;
  const long long pl = blockIdx.z;
  for (int i = threadIdx.x; i < IY * IX; i += 256) {
    const int r = i / IX, q = i % IX;
    const long long off = pl * H * W + (long long)reflect(oy0 * F + first + r, H) * W + reflect(ox0 * F + first + q, W);
    float v;
    if constexpr (MODE == SRC_U8) v = (float)((const unsigned char*)src)[off];
    else if constexpr (MODE == SRC_F32) v = ((const float*)src)[off];
    else v = (float)(((const double*)src)[off] / 255.0);
    in[r][q] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kOY * IX; i += 256) {
    const int r = i / IX, q = i % IX;
    float acc = Taps<F>::w(0) * in[r * F][q];
#pragma unroll
    for (int k = 1; k < K; ++k) acc = acc + Taps<F>::w(k) * in[r * F + k][q];
    mid[r][q] = acc;
  }
  __syncthreads();
  const int r = threadIdx.x / kOX, c = threadIdx.x % kOX;   // 256 threads = kOY x kOX outputs
  if (oy0 + r < Ho && ox0 + c < Wo) {
    float acc = Taps<F>::w(0) * mid[r][c * F];
#pragma unroll
    for (int k = 1; k < K; ++k) acc = acc + Taps<F>::w(k) * mid[r][c * F + k];
    const long long o = pl * Ho * Wo + (long long)(oy0 + r) * Wo + ox0 + c;
    if constexpr (MODE == SRC_NIQE) ((double*)dst)[o] = (double)acc * 255.0;
    else ((float*)dst)[o] = acc;
  }
}
static_assert(kOY * kOX == 256, "one thread per output");

template <int F, int MODE>
void launch_downscale(const void* src, long long planes, int H, int W, void* dst, hipStream_t stream) {
  const long long in_elem = MODE == SRC_U8 ? 1 : MODE == SRC_F32 ? 4 : 8, out_elem = MODE == SRC_NIQE ? 8 : 4;
  const int Ho = H / F, Wo = W / F;
  for (long long p0 = 0; p0 < planes; p0 += 65535) {        // grid.z holds 65535 planes
    const long long np = planes - p0 < 65535 ? planes - p0 : 65535;
    hipLaunchKernelGGL((downscale_kernel<F, MODE>), dim3((unsigned)fcvsr::cdiv(Wo, kOX), (unsigned)fcvsr::cdiv(Ho, kOY), (unsigned)np),
                       dim3(256), 0, stream, (const void*)((const char*)src + p0 * H * W * in_elem), H, W,
                       (void*)((char*)dst + p0 * Ho * Wo * out_elem));
  }
}

// The general resize (fcvsr_imresize): any output size, from two per-axis tap tables the host makes (harness/resize.py
// resize_taps).  Output o of an axis reads the P consecutive inputs first[o] .. first[o] + P - 1, reflected, with the weights
// w[o][0 .. P-1].  One launch makes both passes: a workgroup owns kOY x kOX outputs of one plane, brings its slices of the two tables
// to LDS, makes the first pass for the source span of its tile straight from global memory into an LDS tile, and the second pass
// from there.  The first pass is the axis with the smaller scale (ROWS_FIRST: the row pass, dim 0), as the reference orders them.
// The first pass reads a tap as one 8-byte LDS word, its weight and the REFLECTED input it reads (the row's offset in the plane
// when rows go first, the column otherwise; reflection is applied once per workgroup, when the tables are staged), adds the
// element's own reflected column or row offset and loads; offsets inside a plane are 32-bit.
// Neighbouring outputs are at most kMaxStep inputs apart (scale >= 1/8) and P <= kMaxTaps, which bounds the span of a tile; the
// span is read off the table and clamped to that bound, and the first LDS index of an output is clamped so that its P taps stay
// inside the tile: a table that breaks the rule gives wrong samples, never an access outside the tile.
constexpr int kMaxTaps = 34, kMaxStep = 8;
constexpr int kSpanY = (kOY - 1) * kMaxStep + 2 + kMaxTaps, kSpanX = (kOX - 1) * kMaxStep + 2 + kMaxTaps;   // 92 rows, 284 columns

struct Tap {
  float w;
  int off;
};

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// i / n for 0 <= i < 4096, 1 <= n <= 4096 without the integer division: (i + 0.5) / n is at least 0.5 / n from an integer and the
// two f32 roundings move it by less than 2^-22 of its value
__device__ inline int small_div(int i, float inv_n) { return (int)(((float)i + 0.5f) * inv_n); }

// The sum over k < P of w(k) * v(k), one f32 product per tap, products added in tap order.  A dependent load per tap would make the
// loop a chain of P memory round trips, so the terms are fetched kChunk at a time, their loads in flight together, and then added in
// order; a tap past the end re-reads the last one and is not added.
constexpr int kChunk = 4;
template <class Term>
__device__ inline float tap_sum(int P, Term term) {
  float a = 0.f;
  for (int k0 = 0; k0 < P; k0 += kChunk) {
    float w[kChunk], v[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) term(k0 + j < P ? k0 + j : P - 1, w[j], v[j]);
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const float p = w[j] * v[j];
      if (k0 + j == 0) a = p;
      else if (k0 + j < P) a = a + p;
    }
  }
  return a;
}

// grid.x: the tiles of a plane, row-major (tiles_x per row); grid.y: planes
template <bool ROWS_FIRST, class TI, class TO>
__global__ __launch_bounds__(256) void imresize_kernel(const TI* __restrict__ src, int H, int W, int Ho, int Wo,
                                                       const float* __restrict__ wy, const int* __restrict__ firsty, int Py,
                                                       const float* __restrict__ wx, const int* __restrict__ firstx, int Px,
                                                       int tiles_x, TO* __restrict__ dst) {
  // first-pass taps: rows first [row of the tile][tap], off = reflected row * W; columns first [tap][column of the tile], off =
  // reflected column.  second-pass weights: rows first [tap][column]; columns first [row][tap]
  constexpr int kTap1 = ROWS_FIRST ? kOY * kMaxTaps : kMaxTaps * kOX, kW2 = ROWS_FIRST ? kMaxTaps * kOX : kOY * kMaxTaps;
  __shared__ float mid[ROWS_FIRST ? kOY * kSpanX : kSpanY * kOX];
  __shared__ Tap tap1[kTap1];
  __shared__ float w2[kW2];
  __shared__ int sfy[kOY], sfx[kOX];
  const int tid = threadIdx.x;
  const int oy0 = (int)(blockIdx.x / (unsigned)tiles_x) * kOY, ox0 = (int)(blockIdx.x % (unsigned)tiles_x) * kOX;
  const int ny = Ho - oy0 < kOY ? Ho - oy0 : kOY, nx = Wo - ox0 < kOX ? Wo - ox0 : kOX;
  const long long pl = blockIdx.y;
  const TI* sp = src + pl * H * W;
  const int r = tid / kOX, c = tid % kOX;                   // 256 threads = kOY x kOX outputs
  const bool live = r < ny && c < nx;
  if (r < ny) {                                             // the tables of the tile: thread (r, c) brings taps c, c + 32 of row r
    const int f = firsty[oy0 + r];
    if (c == 0) sfy[r] = f;
    for (int k = c; k < Py; k += kOX) {
      const float w = wy[(long long)(oy0 + r) * Py + k];
      if constexpr (ROWS_FIRST) tap1[r * Py + k] = Tap{w, reflect(f + k, H) * W};
      else w2[r * Py + k] = w;
    }
  }
  if (c < nx) {                                             // ... and taps r, r + 8, .. of column c
    const int f = firstx[ox0 + c];
    if (r == 0) sfx[c] = f;
    for (int k = r; k < Px; k += kOY) {
      const float w = wx[(long long)(ox0 + c) * Px + k];
      if constexpr (ROWS_FIRST) w2[k * kOX + c] = w;
      else tap1[k * kOX + c] = Tap{w, reflect(f + k, W)};
    }
  }
  __syncthreads();
  float acc = 0.f;
  if constexpr (ROWS_FIRST) {
    const int lox = sfx[0], span = clampi(sfx[nx - 1] - lox + Px, 0, kSpanX);
    const float inv = 1.f / (float)span;
    for (int i = tid; i < ny * span; i += 256) {            // the row pass at the tile's output rows, per source column of its span
      const int rr = small_div(i, inv), q = i - rr * span;
      const unsigned col = (unsigned)reflect(lox + q, W);
      const Tap* tp = tap1 + rr * Py;
      mid[rr * kSpanX + q] = tap_sum(Py, [&](int k, float& w, float& v) {
        const Tap t = tp[k];
        w = t.w;
        v = up_sample(sp, (unsigned)t.off + col);
      });
    }
    __syncthreads();
    if (live) {
      const float* m = mid + r * kSpanX + clampi(sfx[c] - lox, 0, kSpanX - Px);
      acc = tap_sum(Px, [&](int k, float& w, float& v) {
        w = w2[k * kOX + c];
        v = m[k];
      });
    }
  } else {
    const int loy = sfy[0], span = clampi(sfy[ny - 1] - loy + Py, 0, kSpanY);
    const float inv = 1.f / (float)nx;
    for (int i = tid; i < span * nx; i += 256) {            // the column pass at the tile's output columns, per source row of its span
      const int q = small_div(i, inv), cc = i - q * nx;
      const unsigned row = (unsigned)(reflect(loy + q, H) * W);
      const Tap* tp = tap1 + cc;
      mid[q * kOX + cc] = tap_sum(Px, [&](int k, float& w, float& v) {
        const Tap t = tp[k * kOX];
        w = t.w;
        v = up_sample(sp, row + (unsigned)t.off);
      });
    }
    __syncthreads();
    if (live) {
      const float* m = mid + clampi(sfy[r] - loy, 0, kSpanY - Py) * kOX + c;
      acc = tap_sum(Py, [&](int k, float& w, float& v) {
        w = w2[r * Py + k];
        v = m[k * kOX];
      });
    }
  }
  if (live) up_result(acc, dst[pl * Ho * Wo + (long long)(oy0 + r) * Wo + ox0 + c]);
}

struct ResizeArgs {
  const void* src;
  long long planes;
  int H, W, Ho, Wo;
  const float *wy, *wx;
  const int *firsty, *firstx;
  int Py, Px;
  void* out;
};

template <bool ROWS_FIRST, class TI, class TO>
void launch_imresize(const ResizeArgs& a, hipStream_t stream) {
  const int tiles_x = fcvsr::cdiv(a.Wo, kOX), tiles_y = fcvsr::cdiv(a.Ho, kOY);
  for (long long p0 = 0; p0 < a.planes; p0 += 65535) {      // grid.y holds 65535 planes
    const long long np = a.planes - p0 < 65535 ? a.planes - p0 : 65535;
    hipLaunchKernelGGL((imresize_kernel<ROWS_FIRST, TI, TO>), dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)np), dim3(256), 0,
                       stream, (const TI*)a.src + p0 * a.H * a.W, a.H, a.W, a.Ho, a.Wo, a.wy, a.firsty, a.Py, a.wx, a.firstx, a.Px,
                       tiles_x, (TO*)a.out + p0 * a.Ho * a.Wo);
  }
}

template <class TI, class TO>
void order_imresize(const ResizeArgs& a, int rows_first, hipStream_t stream) {
  if (rows_first) launch_imresize<true, TI, TO>(a, stream);
  else launch_imresize<false, TI, TO>(a, stream);
}

}  // namespace

void fcvsr::downscale2_f64(const double* src, long long planes, int H, int W, double* dst, hipStream_t stream) {
  launch_downscale<2, SRC_NIQE>(src, planes, H, W, dst, stream);
}

extern "C" int fcvsr_bicubic_downscale(const void* src, int src_dtype, long long planes, int H, int W, int factor, float* out,
                                       void* stream) {
  FCVSR_CHECK_ARG(src && out, "null device pointer");
  FCVSR_CHECK_ARG(src_dtype == FCVSR_U8 || src_dtype == FCVSR_F32, "src_dtype: FCVSR_U8 or FCVSR_F32");
  FCVSR_CHECK_ARG(factor == 2 || factor == 4, "factor: 2 or 4");
  FCVSR_CHECK_ARG(planes >= 1 && H >= factor && W >= factor && H % factor == 0 && W % factor == 0, "H and W: positive multiples of factor");
  FCVSR_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20), "plane too large");
  FCVSR_CHECK_ARG(((uintptr_t)out % 4) == 0 && (src_dtype == FCVSR_U8 || ((uintptr_t)src % 4) == 0), "f32 planes must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (factor == 2) {
    if (src_dtype == FCVSR_U8) launch_downscale<2, SRC_U8>(src, planes, H, W, out, st);
    else launch_downscale<2, SRC_F32>(src, planes, H, W, out, st);
  } else {
    if (src_dtype == FCVSR_U8) launch_downscale<4, SRC_U8>(src, planes, H, W, out, st);
    else launch_downscale<4, SRC_F32>(src, planes, H, W, out, st);
  }
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_bicubic_upscale(const void* src, int src_dtype, long long planes, int H, int W, int factor, void* out, int out_dtype,
                                     void* stream) {
  FCVSR_CHECK_ARG(src && out, "null device pointer");
  FCVSR_CHECK_ARG(src_dtype == FCVSR_U8 || src_dtype == FCVSR_U16 || src_dtype == FCVSR_F32, "src_dtype: FCVSR_U8, FCVSR_U16 or FCVSR_F32");
  FCVSR_CHECK_ARG(out_dtype == FCVSR_F32 || (out_dtype == src_dtype), "out_dtype: FCVSR_F32, or the integer src_dtype");
  FCVSR_CHECK_ARG(factor == 2 || factor == 4, "factor: 2 or 4");
  FCVSR_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1, "planes, H and W: at least 1");
  // a thread per 4 outputs of a row and `factor` rows, numbered in 32 bits inside a plane
  FCVSR_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20) && (long long)(H + 1) * W < (1ll << 31), "plane too large");
  const int src_elem = src_dtype == FCVSR_U8 ? 1 : src_dtype == FCVSR_U16 ? 2 : 4;
  const int out_elem = out_dtype == FCVSR_U8 ? 1 : out_dtype == FCVSR_U16 ? 2 : 4;
  FCVSR_CHECK_ARG(((uintptr_t)src % src_elem) == 0, "src: aligned to its sample size");
  FCVSR_CHECK_ARG(((uintptr_t)out % (4 * out_elem)) == 0, "out: aligned to four samples (16 bytes for f32, 8 for uint16, 4 for uint8)");
  hipStream_t st = (hipStream_t)stream;
  if (factor == 2) dispatch_upscale<2>(src, src_dtype, planes, H, W, out, out_dtype, st);
  else dispatch_upscale<4>(src, src_dtype, planes, H, W, out, out_dtype, st);
  FCVSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int fcvsr_imresize(const void* src, int src_dtype, long long planes, int H, int W, int Ho, int Wo, const float* wy,
                              const int* firsty, int Py, const float* wx, const int* firstx, int Px, int rows_first, void* out,
                              int out_dtype, void* stream) {
  FCVSR_CHECK_ARG(src && out && wy && firsty && wx && firstx, "null device pointer");
  FCVSR_CHECK_ARG(src_dtype == FCVSR_U8 || src_dtype == FCVSR_U16 || src_dtype == FCVSR_F32, "src_dtype: FCVSR_U8, FCVSR_U16 or FCVSR_F32");
  FCVSR_CHECK_ARG(out_dtype == FCVSR_F32 || (out_dtype == src_dtype), "out_dtype: FCVSR_F32, or the integer src_dtype");
  FCVSR_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "planes, H, W, Ho and Wo: at least 1");
  FCVSR_CHECK_ARG(Py >= 1 && Py <= kMaxTaps && Px >= 1 && Px <= kMaxTaps, "Py and Px: 1 .. 34 taps");
  // 32-bit offsets inside a plane
  FCVSR_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20) && Ho <= (1 << 20) && Wo <= (1 << 20) && (long long)H * W < (1ll << 31),
                  "plane too large");
  // neighbouring outputs at most 8 inputs apart (the span of a tile in LDS)
  FCVSR_CHECK_ARG((long long)H <= 8ll * Ho && (long long)W <= 8ll * Wo && (long long)Ho <= 8ll * H && (long long)Wo <= 8ll * W,
                  "per-axis scale outside [1/8, 8]");
  FCVSR_CHECK_ARG((long long)fcvsr::cdiv(Wo, kOX) * fcvsr::cdiv(Ho, kOY) < (1ll << 31), "too many tiles in a plane");
  const int src_elem = src_dtype == FCVSR_U8 ? 1 : src_dtype == FCVSR_U16 ? 2 : 4;
  const int out_elem = out_dtype == FCVSR_U8 ? 1 : out_dtype == FCVSR_U16 ? 2 : 4;
  FCVSR_CHECK_ARG(((uintptr_t)src % src_elem) == 0 && ((uintptr_t)out % out_elem) == 0, "src and out: aligned to their sample size");
  FCVSR_CHECK_ARG(((uintptr_t)wy % 4) == 0 && ((uintptr_t)wx % 4) == 0 && ((uintptr_t)firsty % 4) == 0 && ((uintptr_t)firstx % 4) == 0,
                  "tables: 4-byte aligned");
  const ResizeArgs a{src, planes, H, W, Ho, Wo, wy, wx, firsty, firstx, Py, Px, out};
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == FCVSR_U8) {
    if (out_dtype == FCVSR_U8) order_imresize<unsigned char, unsigned char>(a, rows_first, st);
    else order_imresize<unsigned char, float>(a, rows_first, st);
  } else if (src_dtype == FCVSR_U16) {
    if (out_dtype == FCVSR_U16) order_imresize<unsigned short, unsigned short>(a, rows_first, st);
    else order_imresize<unsigned short, float>(a, rows_first, st);
  } else {
    order_imresize<float, float>(a, rows_first, st);
  }
  FCVSR_LAUNCH_CHECK();
  return 0;
}
