// 3x3 implicit-GEMM convolution with LDS-RESIDENT weights for the 64 / 128-channel layers that carry the FLOPs of the path
// (BlockRCB / RCB bodies, conv_KP, F.0, group convs, recorb0, conv3: reference CVSR_freq.py:705-803, :1409-1416, :1430, :2608).
//
// conv3_lean_kernel (conv_mfma.hip) re-stages the 72 KiB weight block through LDS for every 4 x 32 pixel tile, tap by tap behind
// two barriers per tap, and a wave owns 1 x 2 MFMA fragments (1.5 ds_read_b128 per MFMA): counting the weight re-staging the
// LDS pipe is oversubscribed, which is what held it at 30 % of the MFMA roof.  Here:
//   * persistent workgroups, one per CU (512 threads = 8 waves, two per SIMD); the 9 taps x 64 cin x 64 cout weight block
//     (73,728 bytes, or 2 cin chunks x 9 taps x 32 couts for the 128-input-channel layers) is copied into LDS ONCE per workgroup;
//   * the workgroup walks 8 x 32 pixel tiles.  Its two wave groups (waves 0-3 / 4-7: one wave of each per SIMD) alternate roles
//     every phase: one group multiplies its tile (2 rows x all couts per wave) while the other stores its previous tile straight
//     from the accumulators and copies its next 10 x 34 halo tile into its own LDS buffer by LDS-DMA (global_load_lds_dwordx4:
//     no staging registers, no ds_write).  ONE barrier per phase;
//   * the multiply loop issues v_mfma_f32_16x16x32: a wave's 64 couts x 64 pixels are 4 x 4 fragments of 16 x 16 (2 x 4 for
//     the 32 couts of a 128-input-channel layer), the k loop is 9 taps x 2 steps of 32 channels, tap-major, channels ascending,
//     each step's fragments read two steps ahead (0.5 ds_read_b128 per MFMA, the LDS bytes per FLOP of the 32x32x16 form it
//     replaced).  Same cycles per FLOP as 32x32x16, but under load the chip holds a higher clock on this shape: 7-9 % less
//     time per layer (profiles/r04_conv3_res_mfma_shape_ab.txt).  The results equal those of the 32x32x16 form bit for bit;
//   * operand roles are swapped (weights = MFMA A operand, pixels = B operand), so lane group l >> 4 ends up with 4 consecutive
//     output channels of pixel l & 15; a v_permlane16_swap of two cout fragments pairs the groups l >> 4 and (l >> 4) ^ 1 into
//     8 consecutive channels = one 16-byte store (16-bit destination).  No LDS transpose, hence no epilogue barrier and no
//     epilogue LDS;
//   * LDS-DMA writes 64 lanes x 16 bytes linearly, so rows cannot be padded: bank conflicts are avoided by an XOR swizzle on the
//     per-lane SOURCE address (16-byte chunk c of halo column hx lands in slot c ^ res_swz(hx); weights: by cout), which makes
//     the 16 lanes of every ds_read_b128 phase hit 16 distinct 16-byte bank groups;
//   * the 32 workgroups of one XCD (blockIdx % 8) share a contiguous range of tiles, so halo rows and both cout blocks of a
//     tile hit in that XCD's L2.
// LDS: 73,728 (weights) + 2 x 44,032 (halo tiles) + 256 (bias) + 384 (group parameters) = 162,432 of 163,840 bytes.
#include <type_traits>
#include "conv_res.h"
#include "mfma_util.h"

namespace fcvsr {

constexpr int kRTH = 8, kRTW = 32, kRHW = kRTW + 2, kRHH = kRTH + 2;
constexpr int kRNHP = kRHH * kRHW;                 // 340 halo pixels of 64 channels = 128 bytes each
constexpr int kRNG = (kRNHP + 7) / 8;              // 43 LDS-DMA wave-instructions (8 pixels = 1 KiB each)
constexpr int kRXBytes = kRNG * 1024;              // 44,032
constexpr int kRWRows = 576;                       // weight rows of 64 cin (128 bytes)
constexpr int kRWBytes = kRWRows * 128;            // 73,728
constexpr int kRRowB = kRHW * 128;                 // bytes per halo row
constexpr int kRBiasOff = kRWBytes + 2 * kRXBytes;  // 64 bias floats
constexpr int kRTabOff = kRBiasOff + 256;           // per-group parameter table: 3 x 32 dwords
constexpr size_t kRLds = (size_t)kRTabOff + 3 * 32 * 4;

// LDS slot of 16-byte chunk c of halo column / weight row x: c ^ res_swz(x).  A ds_read_b128 runs in four phases of 16 lanes,
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same +32; the 16x16x32 operand read gives lane l row (or column) x0 + (l & 15)
// and chunk c0 + (l >> 4).  Bank group of a read: 8 (x & 1) + (c ^ res_swz(x)).  For every start x0 the 16 lanes of each phase
// hit 16 distinct bank groups (x0 = 0, 1, 2 and 16, 17, 18 are the multiply loop's reads); the plain (x >> 1) & 7 of a 32x32x16
// layout leaves these reads 2-way.
__device__ __forceinline__ int res_swz(int x) { return ((x >> 1) & 3) | ((x << 1) & 4); }

// Per-group parameters as 32-bit words.  The kernel reads them from LDS: indexing the kernel-argument block by a run-time group
// index makes hipcc fetch it with VECTOR loads, whose s_waitcnt vmcnt(0) also waits for the stores of the previous tile that the
// storing role leaves in flight on purpose (measured: 5-6 k of a 9 k-cycle phase).  Offsets are 32-bit: the dispatcher checks
// that every tensor spans < 2^29 elements.
enum {
  kTSrcLo = 0, kTSrcHi, kTSrcSb2, kTSrcSy2, kTSrcSx2, kTH, kTW, kTTilesX, kTPerImg, kTTileBegin,
  kTDstLo = 12, kTDstHi, kTDstSb, kTDstSy, kTDstSx, kTR0Lo, kTR0Hi, kTR0Sb, kTR0Sy, kTR0Sx, kTR1Lo, kTR1Hi, kTR1Sb, kTR1Sy, kTR1Sx
};

struct ResK {                                        // kernel arguments
  int n_groups, total_tiles, cout, cout_pad, cin_pad, act, n_res, res16, ps;
  float slope, rs[2];
  const float* slope_ptr;
  const uint16_t* w;
  const float* bias;
  const void* zeros;
  int tab[3][32];
};

struct ResTile {
  int gi, b, ty0, tx0;
};

__device__ __forceinline__ ResTile res_decode(const int* tabL, int n_groups, int tile) {
  ResTile t;
  t.gi = 0;
  if (n_groups > 1 && tile >= tabL[32 + kTTileBegin]) t.gi = 1;
  if (n_groups > 2 && tile >= tabL[64 + kTTileBegin]) t.gi = 2;
  const int* T = tabL + t.gi * 32;
  const int tl = tile - T[kTTileBegin];
  const int per_img = T[kTPerImg], tiles_x = T[kTTilesX];
  t.b = tl / per_img;
  const int t2 = tl - t.b * per_img;
  const int ty = t2 / tiles_x;
  t.ty0 = ty * kRTH;
  t.tx0 = (t2 - ty * tiles_x) * kRTW;
  return t;
}

// Pointers rebuilt from table words are declared GLOBAL (address space 1): a generic pointer makes hipcc emit flat_load /
// flat_store, which count on lgkmcnt as well and turn every counted LDS wait of the multiply loop into lgkmcnt(0).
typedef __attribute__((address_space(1))) char gchar_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;      // plain vectors (f32x4_t: mfma_util.h): HIP's uint4 / float4
                                                                   // classes have no address-space-qualified assignment operators
typedef __attribute__((address_space(1))) u32x4_t guint4_t;
typedef __attribute__((address_space(1))) f32x4_t gfloat4_t;
__device__ __forceinline__ void gstore(gchar_t* p, uint4 v) { *reinterpret_cast<guint4_t*>(p) = u32x4_t{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void gstore(gchar_t* p, float4 v) { *reinterpret_cast<gfloat4_t*>(p) = f32x4_t{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ uint4 gload_u4(const gchar_t* p) { const u32x4_t v = *reinterpret_cast<const guint4_t*>(p); return make_uint4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float4 gload_f4(const gchar_t* p) { const f32x4_t v = *reinterpret_cast<const gfloat4_t*>(p); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ gchar_t* tab_ptr(const int* T, int lo) {
  return reinterpret_cast<gchar_t*>(((unsigned long long)(unsigned)T[lo + 1] << 32) | (unsigned)T[lo]);
}

// One LDS-DMA wave-instruction: lane l copies 16 bytes from its own global address to LDS byte (lds_off + 16 l).
// Inline asm on purpose: with the builtin the compiler orders every later LDS read behind the copy (vmcnt(0)), which would
// serialise the copy of the next tile with the multiplication of the current one.  The kernel waits for its copies itself.
__device__ __forceinline__ void glds16(const void* src, unsigned lds_off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_off) : "memory");
}

// global -> LDS copy of the 64-channel chunk `ch` of a halo tile by the 4 waves of one group (wq = 0..3), 10-11 wave-instructions
// each, straight-line (halo pixels outside the image, and the 4 pixels past the tile in the last instruction, read the zero page).
__device__ __forceinline__ void res_stage(const int* tabL, const void* zeros, const ResTile& t, int ch, unsigned xoff, int wq, int lane) {
  const int* T = tabL + t.gi * 32;
  const char* sbase = (const char*)(tab_ptr(T, kTSrcLo) + (long long)t.b * T[kTSrcSb2] + ch * 128);
  const int sy2 = T[kTSrcSy2], sx2 = T[kTSrcSx2];
  const int H = T[kTH], W = T[kTW];
  const int sub = lane >> 3, cl = lane & 7;
#pragma unroll
  for (int i = 0; i < (kRNG + 3) / 4; ++i) {
    const int g = wq + 4 * i;
    if (i * 4 + 3 < kRNG || g < kRNG) {              // only the last round (i = 10) has a (wave-uniform) condition
      const int p = g * 8 + sub;
      const int hy = __mul24(p, 241) >> 13;         // p / 34 for p < 344
      const int hx = p - __mul24(hy, kRHW);
      const int iy = t.ty0 - 1 + hy, ix = t.tx0 - 1 + hx;
      const int c = cl ^ res_swz(hx);
      const bool ok = (p < kRNHP) && ((unsigned)iy < (unsigned)H) && ((unsigned)ix < (unsigned)W);
      const int off = __mul24(iy, sy2) + __mul24(ix, sx2) + c * 16;
      const char* src = ok ? sbase + off : reinterpret_cast<const char*>(zeros);
      glds16(src, __builtin_amdgcn_readfirstlane(xoff + g * 1024));
    }
  }
}

// NCH = input-channel chunks of 64 (1 or 2); a workgroup owns CO = 64 / NCH output channels of every tile it visits.
// MODE: 0 = f32 destination, 1 = 16-bit destination, 2 = 16-bit destination without residuals (the multiplying wave packs).
// NSU: 1 = the activation's negative-side factor lies in [0, 1] (ReLU, LeakyReLU): act(x) = max(x, ns * x); 2 = no activation at
// all (half of the BlockRCB layers): the multiply + max per value is skipped, same bits as max(x, 1 * x); 0 = general (PReLU).
// Both are template parameters because hipcc re-merges wave-uniform run-time variants into one body with a scalar branch
// per 4 values (SimplifyCFG hoists the common code of the arms): ~40 branches per tile in the epilogue.
template <bool BF16, int MODE, int NCH, int NSU>
__global__ __launch_bounds__(512, 2) void conv3_res_kernel(ResK a) {
  constexpr bool DST16 = MODE != 0;
  constexpr bool FAST = MODE == 2;
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int CO = 64 / NCH;                       // couts per workgroup
  constexpr int MF = CO / 32;                        // weight (A operand) fragments per wave
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: tile decoding and role branches stay on the SALU
  const int grp = wave >> 2, wq = wave & 3;          // role group (0: waves 0-3, 1: waves 4-7), row pair inside the tile
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds;

  // ---- schedule: the workgroups of one XCD (blockIdx % 8) share a contiguous range of tiles; NB cout blocks per tile ------
  const int NB = a.cout / CO;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int nb = loc % NB, slot = loc / NB, nslots = (gridDim.x >> 3) / NB;
  const int tb = (int)((long long)xcd * a.total_tiles / 8), te = (int)((long long)(xcd + 1) * a.total_tiles / 8);
  const int n0 = nb * CO;
  const int ntile = (tb + slot < te) ? (te - tb - slot + nslots - 1) / nslots : 0;     // tiles of this workgroup
  if (ntile == 0) return;                                                               // uniform per workgroup
  const int nmine = (ntile - grp + 1) >> 1;          // tiles of my group: list indices grp, grp + 2, ...
  const int NU = nmine * NCH;                        // my units (tile, chunk)
  const int plast = 2 * ((ntile + 1) >> 1) * NCH;    // last phase (group 0's final epilogue / group 1's last compute + 1)

  // ---- resident weights: rows [(ch*9 + tap) * CO + co] of 64 cin, chunk c of a row in slot c ^ ((co >> 1) & 7) -----------
  {
    const int sub = lane >> 3, cl = lane & 7;
#pragma unroll
    for (int i = 0; i < kRWRows / 8 / 8; ++i) {
      const int g = wave + 8 * i;
      const int row = g * 8 + sub;
      const int q = row / CO, co = row - q * CO;     // CO is a power of two
      const int ch = q / 9, tap = q - ch * 9;
      const int c = cl ^ res_swz(co);
      const uint16_t* src = a.w + ((long long)tap * a.cout_pad + n0 + co) * a.cin_pad + ch * 64 + c * 8;
      glds16(src, __builtin_amdgcn_readfirstlane(lds0 + g * 1024));
    }
  }
  if (tid < CO) reinterpret_cast<float*>(lds + kRBiasOff)[tid] = a.bias ? a.bias[n0 + tid] : 0.f;
  if (tid >= 128 && tid < 128 + 96) reinterpret_cast<int*>(lds + kRTabOff)[tid - 128] = a.tab[(tid - 128) >> 5][(tid - 128) & 31];
  const int* tabL = reinterpret_cast<const int*>(lds + kRTabOff);
  const unsigned xoff = lds0 + kRWBytes + grp * kRXBytes;                // my group's halo buffer
  __syncthreads();                                   // the parameter table is in LDS
  ResTile tcur = res_decode(tabL, a.n_groups, tb + slot + grp * nslots < te ? tb + slot + grp * nslots : tb + slot);   // the tile my group staged last
  if (grp == 0) res_stage(tabL, a.zeros, tcur, 0, xoff, wq, lane);

  // Activation as max(x, ns * x) (0 <= ns <= 1) or max(x, 0) + ns * min(x, 0) with ns = 0 (ReLU), slope (LeakyReLU / PReLU) or 1 (none): the same values as the
  // branchy form, and no per-element scalar branch on `act` (hipcc does not unswitch it: 64 branches per tile row).
  // The PReLU slope is read by an explicitly GLOBAL load: a flat_load (address space not provable) stays "pending" in the
  // compiler's wait-count bookkeeping for the rest of the kernel and turns every counted lgkmcnt(N) of the multiply loop into
  // lgkmcnt(0).
  float ns = 1.f;
  if (a.act == FCVSR_ACT_RELU) ns = 0.f;
  else if (a.act == FCVSR_ACT_LEAKY) ns = a.slope;
  else if (a.act == FCVSR_ACT_PRELU) ns = *reinterpret_cast<const __attribute__((address_space(1))) float*>(reinterpret_cast<uintptr_t>(a.slope_ptr));
  const bool r16 = a.res16 != 0;

  // ---- fragment addresses (LDS byte offsets relative to lds): lane (p16, G) reads row / column p16, chunk 4 ks + G ---------
  const int p16 = lane & 15, G = lane >> 4;
  constexpr int MF16 = CO / 16;                      // weight (A operand) fragments per wave; 4 pixel fragments (2 rows x 2 halves)
  unsigned wb[2], xb[3][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    wb[ks] = p16 * 128 + (((4 * ks + G) ^ res_swz(p16)) << 4);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)                   // the second pixel half (+16 columns) has the same swizzle: + 2048 bytes
      xb[kx][ks] = kRWBytes + grp * kRXBytes + (2 * wq * kRHW + p16 + kx) * 128 + (((4 * ks + G) ^ res_swz(p16 + kx)) << 4);
  }
  f32x4_t acc[MF16][4];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                   // weights and group 0's first tile have landed

  int k = 0;                                         // my next unit to multiply
#pragma unroll 1
  for (int p = 0;; ++p) {
    if ((p & 1) == grp) {
      // ================= multiply unit k: tile list index 2 * (k / NCH) + grp, chunk k % NCH ==========================
      if (k < NU) {
        const int ch = (NCH == 1) ? 0 : (k & (NCH - 1));
        if (ch == 0) {
#pragma unroll
          for (int mf = 0; mf < MF16; ++mf)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_s_setprio(2);   // the multiplying wave wins VALU/MFMA issue over its SIMD partner's epilogue
        const unsigned wch = ch * (9 * CO * 128);
        uint4 wf[3][MF16], xf[3][4];                 // fragments are read two 32-deep steps ahead of their MFMAs
        // step S = 2 tap + ks: channels 32 ks + [0, 32) of tap (ky, kx), tap-major, ascending channels
#define FCVSR_RES_LOAD(S, SLOT)                                                                                  \
  do {                                                                                                           \
    constexpr int tap_ = (S) / 2, ks_ = (S) % 2, ky_ = tap_ / 3, kx_ = tap_ % 3;                                 \
    _Pragma("unroll") for (int mf = 0; mf < MF16; ++mf)                                                          \
        wf[SLOT][mf] = *reinterpret_cast<const uint4*>(lds + wb[ks_] + wch + (tap_ * CO + mf * 16) * 128);       \
    _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                                                             \
        xf[SLOT][nf] = *reinterpret_cast<const uint4*>(lds + xb[kx_][ks_] + ((nf >> 1) + ky_) * kRRowB + (nf & 1) * 2048); \
  } while (0)
#define FCVSR_RES_STEP(S)                                                                                        \
  do {                                                                                                           \
    if ((S) + 2 < 18) FCVSR_RES_LOAD(((S) + 2) % 18, ((S) + 2) % 3);                                             \
    _Pragma("unroll") for (int mf = 0; mf < MF16; ++mf)                                                          \
        _Pragma("unroll") for (int nf = 0; nf < 4; ++nf)                                                         \
            acc[mf][nf] = mfma16x16x32<BF16>(wf[(S) % 3][mf], xf[(S) % 3][nf], acc[mf][nf]);                      \
    if ((S) + 2 < 18) {                                                                                          \
      _Pragma("unroll") for (int i_ = 0; i_ < MF16 + 4; ++i_) {                                                  \
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * MF16 / (MF16 + 4), 0);                                   \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                       \
      }                                                                                                          \
      if (4 * MF16 > (MF16 + 4) * (4 * MF16 / (MF16 + 4)))                                                       \
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * MF16 - (MF16 + 4) * (4 * MF16 / (MF16 + 4)), 0);         \
    } else {                                                                                                     \
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * MF16, 0);                                                  \
    }                                                                                                            \
  } while (0)
        FCVSR_RES_LOAD(0, 0);
        FCVSR_RES_LOAD(1, 1);
        __builtin_amdgcn_sched_barrier(0);
        FCVSR_RES_STEP(0);  FCVSR_RES_STEP(1);  FCVSR_RES_STEP(2);  FCVSR_RES_STEP(3);  FCVSR_RES_STEP(4);  FCVSR_RES_STEP(5);
        FCVSR_RES_STEP(6);  FCVSR_RES_STEP(7);  FCVSR_RES_STEP(8);  FCVSR_RES_STEP(9);  FCVSR_RES_STEP(10); FCVSR_RES_STEP(11);
        FCVSR_RES_STEP(12); FCVSR_RES_STEP(13); FCVSR_RES_STEP(14); FCVSR_RES_STEP(15); FCVSR_RES_STEP(16); FCVSR_RES_STEP(17);
#undef FCVSR_RES_STEP
#undef FCVSR_RES_LOAD
        __builtin_amdgcn_s_setprio(0);
        // Bias and activation on the multiplying side, in the accumulator layout (lane = pixel p16 of fragment nf, registers
        // 0..3 = couts mf*16 + 4G + [0, 4)).  With a 16-bit destination and no residual the values are packed into registers 0, 1.
        if (ch == NCH - 1) {
          const float* bias_a = reinterpret_cast<const float*>(lds + kRBiasOff) + 4 * G;
#pragma unroll
          for (int mf = 0; mf < MF16; ++mf) {
            const float4 b4 = *reinterpret_cast<const float4*>(bias_a + mf * 16);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
              float v[4] = {acc[mf][nf][0] + b4.x, acc[mf][nf][1] + b4.y, acc[mf][nf][2] + b4.z, acc[mf][nf][3] + b4.w};
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (NSU != 2) v[e] = NSU == 1 ? fmaxf(v[e], ns * v[e]) : fmaxf(v[e], 0.f) + ns * fminf(v[e], 0.f);
              if (FAST) {
                const uint2 pk = cvt4<BF16>(make_float4(v[0], v[1], v[2], v[3]));
                acc[mf][nf][0] = __uint_as_float(pk.x);
                acc[mf][nf][1] = __uint_as_float(pk.y);
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[mf][nf][e] = v[e];
              }
            }
          }
        }
      }
      ++k;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my LDS reads are complete before the other phase's copy overwrites
    } else {
      // ================= copy unit k into my buffer; store the tile whose last chunk was unit k - 1 =======================
      ResTile tn = tcur;                             // one decode per tile: the copy below and the stores two phases later share it
      if (k < NU) {
        const int ch = (NCH == 1) ? 0 : (k & (NCH - 1));
        if (ch == 0 && k > 0) tn = res_decode(tabL, a.n_groups, tb + slot + (2 * (k / NCH) + grp) * nslots);
        res_stage(tabL, a.zeros, tn, ch, xoff, wq, lane);
      }
      int nst = 0;                                   // store wave-instructions issued below (wave-uniform)
      if (k >= 1 && k <= NU && ((k - 1) & (NCH - 1)) == NCH - 1) {
        // Branch-free up to the stores: every load of a tile row (bias from LDS, residuals from HBM) is issued before the first
        // use, so a row costs one memory round trip instead of one per 8-channel chunk.
        const ResTile t = tcur;
        const int* T = tabL + t.gi * 32;
        const int GH = T[kTH], GW = T[kTW];
        gchar_t* dbase = tab_ptr(T, kTDstLo);
        const gchar_t* r0base = tab_ptr(T, kTR0Lo);
        const gchar_t* r1base = tab_ptr(T, kTR1Lo);
        // v_permlane16_swap of fragments (2m, nf) and (2m+1, nf) of the lane groups G, G^1 -> 8 consecutive couts
        // 32m + 16 (G & 1) + 8 (G >> 1) + [0, 8) of pixel p16 of fragment nf = one 16-byte store
        const int cl8 = 16 * (G & 1) + 8 * (G >> 1);
        const int cq4 = a.cout >> 2, sp = a.ps ? n0 / cq4 : 0, nch = a.ps ? n0 - sp * cq4 : n0;
        typedef __attribute__((ext_vector_type(2))) unsigned u2_t;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j) __builtin_amdgcn_sched_barrier(0);    // one row at a time: hoisting both rows' loads spills
          const int py = t.ty0 + 2 * wq + j;
          bool ok[2];
          unsigned dpix[2], rpix[2][2];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const int px = t.tx0 + 16 * hf + p16;
            ok[hf] = (py < GH) && (px < GW);
            // lanes outside the image read the residuals of the image's first pixel (always a valid address) and store nothing
            const int pyc = ok[hf] ? py : 0, pxc = ok[hf] ? px : 0;
            // PixelShuffle(2): rows are packed sub-pixel-major, so this workgroup's 64 couts are 64 consecutive channels of ONE
            // sub-pixel (i, j): the same store at pixel (2y + i, 2x + j), channel n0 % (cout/4)
            const int dyy = a.ps ? 2 * pyc + (sp >> 1) : pyc, dxx = a.ps ? 2 * pxc + (sp & 1) : pxc;
            dpix[hf] = (unsigned)(t.b * T[kTDstSb] + dyy * T[kTDstSy] + dxx * T[kTDstSx] + nch + cl8);   // elements
            rpix[0][hf] = (unsigned)(t.b * T[kTR0Sb] + pyc * T[kTR0Sy] + pxc * T[kTR0Sx] + n0 + cl8);
            rpix[1][hf] = (unsigned)(t.b * T[kTR1Sb] + pyc * T[kTR1Sy] + pxc * T[kTR1Sx] + n0 + cl8);
            if (__builtin_amdgcn_ballot_w64(ok[hf]) != 0) nst += MF * (DST16 ? 1 : 2);   // the stores below run iff some lane is live
          }
          if (FAST) {
            // packed by the multiplying wave: registers 0, 1 of fragments (2m, nf), (2m+1, nf) -> one 16-byte store
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
              for (int m = 0; m < MF; ++m) {
                const int nf = 2 * j + hf;
                const u2_t s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * m][nf][0]), __float_as_uint(acc[2 * m + 1][nf][0]), false, false);
                const u2_t s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * m][nf][1]), __float_as_uint(acc[2 * m + 1][nf][1]), false, false);
                if (ok[hf]) gstore(dbase + (size_t)(dpix[hf] + 32 * m) * 2, make_uint4(s0.x, s1.x, s0.y, s1.y));
              }
            continue;
          }
          float x[2][MF][8];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int m = 0; m < MF; ++m)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int nf = 2 * j + hf;
                const u2_t sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[2 * m][nf][e]), __float_as_uint(acc[2 * m + 1][nf][e]), false, false);
                x[hf][m][e] = __uint_as_float(sw.x);
                x[hf][m][4 + e] = __uint_as_float(sw.y);
              }
#pragma unroll
          for (int ri = 0; ri < 2; ++ri) {
            if (ri < a.n_res) {
              const gchar_t* rp = ri == 0 ? r0base : r1base;
              const float rs = a.rs[ri];
              if (r16) {
                uint4 v[2][MF];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                  for (int m = 0; m < MF; ++m) v[hf][m] = gload_u4(rp + (size_t)(rpix[ri][hf] + 32 * m) * 2);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                  for (int m = 0; m < MF; ++m) {
                    float rr[8];
                    cvt16x4_to_f32<BF16>(make_uint2(v[hf][m].x, v[hf][m].y), rr);
                    cvt16x4_to_f32<BF16>(make_uint2(v[hf][m].z, v[hf][m].w), rr + 4);
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[hf][m][e] = fmaf(rs, rr[e], x[hf][m][e]);
                  }
              } else {
                float4 v[2][MF][2];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                  for (int m = 0; m < MF; ++m) {
                    v[hf][m][0] = gload_f4(rp + (size_t)(rpix[ri][hf] + 32 * m) * 4);
                    v[hf][m][1] = gload_f4(rp + (size_t)(rpix[ri][hf] + 32 * m + 4) * 4);
                  }
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                  for (int m = 0; m < MF; ++m) {
                    const float4 u0 = v[hf][m][0], u1 = v[hf][m][1];
                    float* xx = x[hf][m];
                    xx[0] = fmaf(rs, u0.x, xx[0]); xx[1] = fmaf(rs, u0.y, xx[1]); xx[2] = fmaf(rs, u0.z, xx[2]); xx[3] = fmaf(rs, u0.w, xx[3]);
                    xx[4] = fmaf(rs, u1.x, xx[4]); xx[5] = fmaf(rs, u1.y, xx[5]); xx[6] = fmaf(rs, u1.z, xx[6]); xx[7] = fmaf(rs, u1.w, xx[7]);
                  }
              }
            }
          }
#pragma unroll
          for (int hf = 0; hf < 2; ++hf)
            if (ok[hf]) {
#pragma unroll
              for (int m = 0; m < MF; ++m) {
                const float* xx = x[hf][m];
                if (DST16) {
                  const uint2 lo = cvt4<BF16>(make_float4(xx[0], xx[1], xx[2], xx[3])), hi = cvt4<BF16>(make_float4(xx[4], xx[5], xx[6], xx[7]));
                  gstore(dbase + (size_t)(dpix[hf] + 32 * m) * 2, make_uint4(lo.x, lo.y, hi.x, hi.y));
                } else {
                  gstore(dbase + (size_t)(dpix[hf] + 32 * m) * 4, make_float4(xx[0], xx[1], xx[2], xx[3]));
                  gstore(dbase + (size_t)(dpix[hf] + 32 * m + 4) * 4, make_float4(xx[4], xx[5], xx[6], xx[7]));
                }
              }
            }
        }
      }
      tcur = tn;
      // My copies must have landed before the barrier; my stores need not have.  vmcnt counts loads, LDS-DMA and stores
      // together in issue order, and the stores are the youngest operations: leave exactly them outstanding (waiting for them
      // too exposes a full HBM write round trip per phase - measured 78 vs 54 us on a 64->64 layer).
      constexpr int SH = MF * (DST16 ? 1 : 2);        // stores per half tile row (16 pixels)
      if (nst == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (nst == SH) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SH) : "memory");
      else if (nst == 2 * SH) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * SH) : "memory");
      else if (nst == 3 * SH) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * SH) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * SH) : "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (p >= plast) break;
  }
}


bool conv3_res_supports(int cin, int cout) { return (cin == 64 && cout % 64 == 0) || (cin == 128 && cout % 32 == 0); }

template <bool BF16, int MODE, int NCH, int NSU>
static hipError_t launch_res(const ResArgs& a, hipStream_t st) {
  static DevOnce attr;
  int dev = 0;
  hipError_t e = once_per_device(attr, [&] {
    return hipFuncSetAttribute((const void*)conv3_res_kernel<BF16, MODE, NCH, NSU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRLds);
  }, &dev);
  if (e != hipSuccess) return e;
  const int cus = device_cu_count(dev);
  if (cus <= 0) return hipErrorInvalidDevice;
  const int n_cu = cus > 8 ? cus / 8 * 8 : 8;
  const int NB = a.cout / (64 / NCH);
  // one persistent workgroup per CU; the grid is a multiple of 8 * NB (every XCD gets whole slots of NB cout blocks)
  int grid = n_cu / (8 * NB) * (8 * NB);
  if (grid < 8 * NB) grid = 8 * NB;
  const int need = (a.total_tiles + 7) / 8 * 8 * NB;
  if (grid > need) grid = need;
  ResK k;
  k.n_groups = a.n_groups; k.total_tiles = a.total_tiles; k.cout = a.cout; k.cout_pad = a.cout_pad; k.cin_pad = a.cin_pad;
  k.act = a.act; k.n_res = a.n_res; k.res16 = a.res16; k.ps = a.ps; k.slope = a.slope; k.rs[0] = a.rs[0]; k.rs[1] = a.rs[1];
  k.slope_ptr = a.slope_ptr; k.w = a.w; k.bias = a.bias; k.zeros = a.zeros;
  for (int g = 0; g < 3; ++g) {
    const ResGroup& G = a.g[g < a.n_groups ? g : 0];
    int* T = k.tab[g];
    for (int i = 0; i < 32; ++i) T[i] = 0;
    auto put = [&](int lo, const void* p) { T[lo] = (int)(unsigned)((uintptr_t)p & 0xffffffffu); T[lo + 1] = (int)(unsigned)((uintptr_t)p >> 32); };
    put(kTSrcLo, G.src.p);
    T[kTSrcSb2] = (int)(G.src.sb * 2); T[kTSrcSy2] = (int)(G.src.sy * 2); T[kTSrcSx2] = (int)(G.src.sx * 2);
    T[kTH] = G.H; T[kTW] = G.W; T[kTTilesX] = G.tiles_x; T[kTPerImg] = G.tiles_x * G.tiles_y;
    T[kTTileBegin] = g < a.n_groups ? G.tile_begin : 0x7fffffff;
    put(kTDstLo, G.dst.p); T[kTDstSb] = (int)G.dst.sb; T[kTDstSy] = (int)G.dst.sy; T[kTDstSx] = (int)G.dst.sx;
    const View& r0 = a.n_res > 0 ? G.res[0] : G.dst;      // unused residual slots alias the destination (valid addresses)
    const View& r1 = a.n_res > 1 ? G.res[1] : G.dst;
    put(kTR0Lo, r0.p); T[kTR0Sb] = (int)r0.sb; T[kTR0Sy] = (int)r0.sy; T[kTR0Sx] = (int)r0.sx;
    put(kTR1Lo, r1.p); T[kTR1Sb] = (int)r1.sb; T[kTR1Sy] = (int)r1.sy; T[kTR1Sx] = (int)r1.sx;
  }
  hipLaunchKernelGGL((conv3_res_kernel<BF16, MODE, NCH, NSU>), dim3(grid), dim3(512), kRLds, st, k);
  return hipGetLastError();
}

ResVariant conv3_res_variant(int cin, int n_res, int act, float slope, bool dst16) {
  // act(x) = max(x, ns * x) needs 0 <= ns <= 1: known on the host for every activation but PReLU (slope in device memory)
  const bool ns01 = act == FCVSR_ACT_RELU || (act == FCVSR_ACT_LEAKY && slope >= 0.f && slope <= 1.f);
  return ResVariant{!dst16 ? 0 : (n_res == 0 ? 2 : 1), cin / 64, act == FCVSR_ACT_NONE ? 2 : (ns01 ? 1 : 0)};
}

template <bool BF16, int NCH, int NSU>
static hipError_t launch_res_mode(const ResArgs& a, int mode, hipStream_t st) {
  return mode == 0 ? launch_res<BF16, 0, NCH, NSU>(a, st) : mode == 1 ? launch_res<BF16, 1, NCH, NSU>(a, st) : launch_res<BF16, 2, NCH, NSU>(a, st);
}

template <bool BF16, int NCH>
static hipError_t launch_res_nsu(const ResArgs& a, const ResVariant& v, hipStream_t st) {
  return v.nsu == 2   ? launch_res_mode<BF16, NCH, 2>(a, v.mode, st)
         : v.nsu == 1 ? launch_res_mode<BF16, NCH, 1>(a, v.mode, st) : launch_res_mode<BF16, NCH, 0>(a, v.mode, st);
}

hipError_t launch_conv3_res(const ResArgs& a, bool bf16, bool dst16, hipStream_t st) {
  if (!conv3_res_supports(a.cin, a.cout)) return hipErrorInvalidValue;
  const ResVariant v = conv3_res_variant(a.cin, a.n_res, a.act, a.slope, dst16);
  if (v.nch == 1) return bf16 ? launch_res_nsu<true, 1>(a, v, st) : launch_res_nsu<false, 1>(a, v, st);
  return bf16 ? launch_res_nsu<true, 2>(a, v, st) : launch_res_nsu<false, 2>(a, v, st);
}

// 256 zero bytes per DEVICE (the source of halo pixels outside the image), created on first use.  hipMalloc / hipMemset are not
// capturable: the engine runs every configuration eagerly before it captures a hipGraph, so this never happens inside a
// capture; a capture that does reach it is refused rather than handed another device's page.
hipError_t conv3_res_zero_page(hipStream_t st, const void** zeros) {
  static void* page[64] = {nullptr};
  static DevOnce made;
  int dev = 0;
  const hipError_t e = once_per_device(made, [&] {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
    const hipError_t ez = hipMalloc(&page[dev], 256);
    return ez != hipSuccess ? ez : hipMemset(page[dev], 0, 256);
  }, &dev);
  if (e == hipSuccess) *zeros = page[dev];
  return e;
}

}  // namespace fcvsr
