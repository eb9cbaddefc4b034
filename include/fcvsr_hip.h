/*
 * fcvsr_hip.h - C ABI of libfcvsr_hip.so: the MI355X (gfx950) hot path of FCVSR's per-frame forward.
 *
 * The reference (QZ1-boy/FCVSR) has no FFI/plugin boundary: its hot path is the Python method
 * GShiftNet_S.forward / GShiftNet.forward (CVSR_train/arch/CVSR_freq.py:2611-2646, :2688-2756) built from
 * stock torch ops.  The drop-in seam is therefore the Python nn.Module (fcvsr_amd/arch/CVSR_freq.py);
 * *below* that seam every arithmetic step is one of the entry points declared here.  Each entry point cites
 * the reference function(s) it replaces.  INTEGRATION.md shows the ctypes binding a reference maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers (HBM) unless named host_*;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue, never synchronise;
 *  - every function returns 0 on success, a negative FCVSR_E_* code on bad arguments, or a positive
 *    hipError_t when a launch fails; fcvsr_last_error() returns a human-readable message (thread-local);
 *  - activations are described by `fcvsr_view`: a strided 4-D (b,y,x,c) window into a buffer, so NCHW boundary
 *    tensors, NHWC internal tensors, channel slices and channel concatenations need no copies.
 *    Internal layout is NHWC (channels innermost) so that a pixel's channels are one contiguous HBM segment.
 */
#ifndef FCVSR_HIP_H
#define FCVSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCVSR_ABI_VERSION 2

enum { FCVSR_E_ARG = -1, FCVSR_E_UNSUPPORTED = -2, FCVSR_E_NOGPU = -3 };
enum { FCVSR_F32 = 0, FCVSR_BF16 = 1, FCVSR_F16 = 2 };
enum { FCVSR_U8 = 3 };   /* uint8 frames: accepted only by the *_u8 entry points */
enum { FCVSR_U16 = 4 };  /* 10-bit samples in uint16 containers: accepted only by the *_u16 entry points */
enum { FCVSR_ACT_NONE = 0, FCVSR_ACT_RELU = 1, FCVSR_ACT_LEAKY = 2, FCVSR_ACT_PRELU = 3 };

/* strided (b,y,x,c) window; strides in ELEMENTS of `dtype`; ptr already points at element (0,0,0,0) */
typedef struct fcvsr_view {
  void*   ptr;
  int64_t sb, sy, sx, sc;
  int32_t c;      /* number of channels in this window */
  int32_t dtype;  /* FCVSR_F32 | FCVSR_BF16 | FCVSR_F16 (| FCVSR_U8 | FCVSR_U16) */
} fcvsr_view;

/* One 2-D convolution with fused epilogue.  Replaces nn.Conv2d call sites of the path
 * (CVSR_freq.py:2589 feat_extract, :1371-1396 convfuse/convcorr/convcrt, :344-357 ConvBlk convs, :1409-1416
 * conv_KP/F, :1430 conv3, :2594-2609 rconcat/upconv/conv_last0, :705-803 RCB/BlockRCB/SCGroupbk convs) together with
 * the elementwise ops the reference launches around them (bias, ReLU/LeakyReLU/PReLU, residual adds,
 * torch.cat of inputs, nn.PixelShuffle(2) of the output).
 *   dst = PS?( act(conv(cat(src[0..n_src)), W) + bias) + sum_i res_scale[i]*res[i] )
 */
typedef struct fcvsr_conv_desc {
  int32_t     n_src;          /* 1..3 inputs concatenated along channels (torch.cat(dim=1)) */
  fcvsr_view  src[3];
  int32_t     B, H, W;        /* input spatial size */
  int32_t     kh, kw, stride, pad;
  int32_t     cout;
  const void* weight;         /* packed by fcvsr_pack_conv_weight layout: [kh*kw][cin_total][cout_pad] (f32) */
  int32_t     cout_pad;       /* row length of packed weight (multiple of 16) */
  const float* bias;          /* cout floats or NULL */
  int32_t     act;            /* FCVSR_ACT_* */
  float       slope;          /* LEAKY slope */
  const float* slope_ptr;     /* PRELU: device pointer to the scalar slope (nn.PReLU(), :2590) */
  int32_t     n_res;          /* 0..2 residual inputs at OUTPUT (pre-shuffle) resolution with cout channels */
  fcvsr_view  res[2];
  float       res_scale[2];
  fcvsr_view  dst;            /* output window; if pixel_shuffle: (2*Ho, 2*Wo) spatial, cout/4 channels */
  int32_t     pixel_shuffle;  /* 0/1: out[c,2h+i,2w+j] = conv[4c+2i+j,h,w] (:2633-2642) */
  /* fcvsr_conv2d_mfma only: ContextBlock fusion (:657-701).  When both are non-NULL the epilogue also emits, per workgroup,
   * online-softmax partials of the layer output r: sum_p exp(l_p - m) r_p[c], m = max l_p, sum exp, with l_p = <r_p, gc_wmask>.
   * gc_partial: [B][ceil(H/4)*ceil(W/32)][cout+2] floats (one per 4x32 tile); combine with fcvsr_gc_finish. */
  const float* gc_wmask;
  float*       gc_partial;
} fcvsr_conv_desc;

const char* fcvsr_last_error(void);
int  fcvsr_abi_version(void);
/* number of HIP devices visible (0 when there is no GPU); never throws */
int  fcvsr_device_count(void);

/* direct (VALU, f32) convolution: any kernel size / channel count; used for skinny layers and as the exact-f32 path */
int fcvsr_conv2d(const fcvsr_conv_desc* d, void* stream);

/* Matrix-core (MFMA) implicit-GEMM convolution: 1x1 or 3x3, stride 1, "same" padding, f32 activations in HBM converted
 * to `mma_dtype` (FCVSR_BF16 | FCVSR_F16) while staging through LDS, f32 accumulate and f32 epilogue.
 * `descs[0..n_groups)` (1..3) are problems that share weights/epilogue but have their own tensors and sizes (the three
 * pyramid levels of BlockRCB, CVSR_freq.py:766-777) and run in ONE launch.
 * weight: 16-bit [kh*kw][cout_pad][cin_pad], cout_pad = ceil128(cout), cin_pad = ceil64(cin), zero padded.
 * src views may be f32 or already `mma_dtype` (all alike); dst may be f32 or `mma_dtype` (16-bit storage for tensors whose
 * only consumers are further MFMA convolutions: bit-identical results, half the HBM bytes); res views are f32.
 * With pixel_shuffle the weight/bias rows must be ordered sub-pixel-major: row (2*i+j)*(cout/4)+c holds original output
 * channel 4*c+2*i+j, so that one lane's 4 consecutive couts land in one pixel of the shuffled output.
 *
 * One of six kernels runs: the first path of this list whose conditions hold for every group (DESIGN.md section 4 spells
 * the conditions out; csrc/conv_plan.hip has one predicate per path).
 *   1 conv1ps_res_kernel    1x1 pixel-shuffle up-convolution 64 -> cout <= 256, 16-bit source and destination, one group
 *   2 conv3s2_lean_kernel   3x3 stride 2, one dense source of a multiple of 64 channels, cout % 64 == 0, no residuals
 *   3 conv1_lean_kernel     1x1, every source a multiple of 64 channels, f32 residuals, channel-contiguous destination
 *   4 conv3_res_kernel      3x3 stride 1, one dense 16-bit source of 64 / 128 channels, cout % 64 == 0, everything on 16-byte
 *                           granules, no ContextBlock fusion; launches of at least 768 workgroup-tiles
 *   5 conv3_lean_kernel     3x3 stride 1, one dense source of a multiple of 64 channels, no pixel shuffle
 *   6 conv_mfma_kernel      everything else the argument checks admit
 * 16-bit residuals and ContextBlock fusion into a 16-bit destination are layouts of paths 4 and 5 only: a problem that has one
 * and would run on path 6 is rejected (FCVSR_E_ARG).
 * Test and benchmark seam, read once per call: FCVSR_MFMA_LEAN = 0 switches paths 2, 3 and 5 off (and with them path 1 and every
 * path-4 layer but the pixel-shuffled 64 -> 256 ones), any other value or unset leaves them on; FCVSR_MFMA_RES = 0 switches
 * paths 1 and 4 off, any other number takes path 4 at every size, unset applies the size rule. */
int fcvsr_conv2d_mfma(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, void* stream);
/* The decision fcvsr_conv2d_mfma would take under the policy (lean: 0 | 1 as FCVSR_MFMA_LEAN, res: 0 | 1, or 2 = unset, as
 * FCVSR_MFMA_RES), without launching, without a GPU and whatever the environment says: writes the kernel name
 * fcvsr_last_conv_kernel() would report into kernel_name[cap] and returns 0, or returns the rejection with fcvsr_last_error()
 * set.  Tensor pointers are looked at for alignment only. */
int fcvsr_conv2d_mfma_plan(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, int lean, int res, char* kernel_name, int cap);
/* Name (template instance) of the kernel the calling thread's last fcvsr_conv2d_mfma call launched, e.g.
 * "conv3_res_kernel<true, 2, 1, 1>": measurement aid for bench.py's per-kernel roofline, not part of the data path. */
const char* fcvsr_last_conv_kernel(void);
/* fcvsr_conv2d on the matrix cores with f32 operands (v_mfma_f32_32x32x2_f32: exact f32, bit-equal to an fmaf chain): the
 * arithmetic of the exact-f32 mode for 3x3 / 1x1 stride-1 layers with one dense NHWC f32 source of a multiple of 32 channels,
 * no pixel shuffle.  weight: f32 [kh*kw][cout_pad][cin], cout_pad a multiple of 64 (zero rows past cout); every other field as
 * in fcvsr_conv2d.  fcvsr_conv2d_f32mfma_eligible returns 1 when the descriptor qualifies. */
int fcvsr_conv2d_f32mfma_eligible(const fcvsr_conv_desc* d);
int fcvsr_conv2d_f32mfma(const fcvsr_conv_desc* d, void* stream);
/* Backward of the convolutions (reference: `loss.backward()` through nn.Conv2d, CVSR_train/train_LD_freqCVSR_S_22.py:250).
 * The input gradient of a stride-1 "same" convolution is itself such a convolution of the output gradient with the transposed,
 * tap-flipped weight, so it goes through fcvsr_conv2d / fcvsr_conv2d_mfma; the weight gradient is this entry point:
 *   dw[co][ci][ky][kx] = sum_{b,oy,ox} gy[b,oy,ox,co] * x[b, oy*stride - pad + ky, ox*stride - pad + kx, ci]
 * x: (B,H,W,cin), gy: (B,Ho,Wo,cout), both channel-contiguous f32 views; dw: f32 (cout,cin,kh,kw) = nn.Conv2d.weight layout;
 * scratch: >= fcvsr_conv2d_wgrad_scratch_elems(...) floats.  Exact f32, fixed summation order (bit-reproducible).
 * accumulate = 1 ADDS the sum to dw instead of overwriting it (the same for every `accumulate` argument of the training path: the
 * training step keeps every parameter gradient in one flat, pre-zeroed buffer and lets the reductions add straight into it). */
long long fcvsr_conv2d_wgrad_scratch_elems(int B, int Ho, int Wo, int cin, int cout, int kh, int kw);
int fcvsr_conv2d_wgrad(const fcvsr_view* x, const fcvsr_view* gy, int B, int H, int W, int kh, int kw, int stride, int pad,
                       float* dw, float* scratch, long long scratch_elems, int accumulate, void* stream);
/* The same weight gradient with bf16 products on the matrix cores (f32 accumulation, deterministic slab order): 3x3 / 1x1,
 * stride 1, cin and cout multiples of 64 (fcvsr_conv2d_wgrad_mfma_eligible); same arguments and result layout.  dbias != NULL: the
 * kernel also writes (dbias_accumulate = 0) or adds (1) dL/dbias[cout] = sum over pixels of gy (nn.Conv2d bias gradient; f32, fixed
 * summation order) - it has the gy tiles in registers anyway.  dbias = NULL: no bias gradient. */
int fcvsr_conv2d_wgrad_mfma_eligible(int cin, int cout, int kh, int kw, int stride, int pad);
long long fcvsr_conv2d_wgrad_mfma_scratch_elems(int B, int Ho, int Wo, int cin, int cout, int kh, int kw);
int fcvsr_conv2d_wgrad_mfma(const fcvsr_view* x, const fcvsr_view* gy, int B, int H, int W, int kh, int kw, int stride, int pad,
                            float* dw, float* dbias, float* scratch, long long scratch_elems, int dw_accumulate, int dbias_accumulate,
                            void* stream);
/* Training-path helpers (reference: the per-layer work of `loss.backward()` + `optimizer.step()`, train_LD_freqCVSR_S_22.py:244-251).
 * fcvsr_pack_weight_mfma: nn.Conv2d.weight (cout,cin,kh,kw) f32 -> the 16-bit operand layout of fcvsr_conv2d_mfma,
 *   [kh*kw][rows_pad][cols_pad] zero padded; transposed = 0: rows = cout, cols = cin (forward); transposed = 1: rows = cin,
 *   cols = cout, taps flipped (the input-gradient convolution).  One launch (the weights change every optimizer step).
 * fcvsr_act_bwd: out = g * (y > 0 ? 1 : slope), y = the activation's output (LeakyReLU / ReLU backward), any n >= 0 (16-byte aligned pointers), out may alias g.
 * fcvsr_colsum: out[c] = sum over the npix rows of a dense (npix, C) f32 matrix (bias gradient), deterministic two-stage. */
int fcvsr_pack_weight_mfma(const float* w, int cout, int cin, int kh, int kw, void* dst, int rows_pad, int cols_pad, int dtype,
                           int transposed, void* stream);
/* The same packing for n_items weights in ONE launch (a training pass re-packs ~200 weights).  tab: device memory, 9 x int64 per item =
 * {source pointer (f32 contiguous (cout,cin,kh,kw)), destination pointer, cout, cin, kh*kw, rows_pad, cols_pad, transposed, first block};
 * item i owns ceil(kh*kw*rows_pad*cols_pad / fcvsr_pack_weights_multi_block_elems()) consecutive blocks; total_blocks = their sum. */
int fcvsr_pack_weights_multi_block_elems(void);
int fcvsr_pack_weights_mfma_multi(const long long* tab, int n_items, int total_blocks, int dtype, void* stream);
/* One Adam step (torch.optim.Adam's L2 form: no amsgrad, no decoupled decay) over n_items parameters in ONE launch.  grad (read),
 * exp_avg and exp_avg_sq (read and written) are flat f32 buffers, 16-byte aligned, that share one set of offsets.  tab: device memory,
 * 4 x int64 per item = {parameter pointer (f32 contiguous, 16-byte aligned), offset of the parameter in the flat buffers (elements),
 * element count, first block}; item i owns ceil(count / fcvsr_adam_multi_block_elems()) consecutive blocks; total_blocks = their sum.
 * Per element, in f32 with every operation rounded once, correctly rounded division and square root, subnormals kept:
 *   g' = g + wd * p;  m' = m + (g' - m) * one_minus_b1;  v' = v * b2 + (g' * g') * one_minus_b2;
 *   p' = p - step_size * (m' / (sqrt(v') / bc2_sqrt + eps))
 * with step_size = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) computed by the caller in f64 and rounded once (t >= 1 is the
 * number of this step).  A null pointer, an empty table or t < 1 is FCVSR_E_ARG. */
int fcvsr_adam_multi_block_elems(void);
int fcvsr_adam_multi(const long long* tab, int n_items, int total_blocks, const float* grad, float* exp_avg, float* exp_avg_sq,
                     int t, float step_size, float bc2_sqrt, float one_minus_b1, float b2, float one_minus_b2, float eps, float wd,
                     void* stream);
int fcvsr_act_bwd(const float* g, const float* y, float* out, float slope, long long n, void* stream);
long long fcvsr_colsum_scratch_elems(long long npix, int C);
int fcvsr_colsum(const float* x, long long npix, int C, float* out, float* scratch, long long scratch_elems, int accumulate, void* stream);
/* RCB tail with the ContextBlock under training (CVSR_freq.py:657-701 inside RCB.forward :705-725), dense (B, HW, 64) f32:
 *   out = LeakyReLU_slope(r + add(r)) + z,  add = W2 . LeakyReLU_slope(W1 . ctx),  ctx = sum_p softmax_p(wmask . r[p]) r[p].
 * forward: three launches; stats (B x fcvsr_rcbt_stat_elems() floats) is what the backward needs besides r;
 *   scratch >= B * fcvsr_rcbt_nblk(HW) * 66 floats.
 * backward: g = dL/dout -> gr = dL/dr (dL/dz = g), dwmask[64], dw1[64x64], dw2[64x64] (row-major like the 1x1 conv weights);
 *   scratch >= B * nblk * 64 + B * 65 + 4 + 2 * B * 4096 floats.  Two-stage fixed-order reductions (bit-reproducible). */
int fcvsr_rcbt_nblk(int HW);
int fcvsr_rcbt_stat_elems(void);
int fcvsr_rcbt_forward(const float* r, const float* z, const float* wmask, const float* w1, const float* w2, float slope, int B, int HW,
                       int C, float* out, float* stats, float* scratch, long long scratch_elems, void* stream);
int fcvsr_rcbt_backward(const float* r, const float* g, const float* wmask, const float* w1, const float* w2, const float* stats,
                        float slope, int B, int HW, int C, float* gr, float* dwmask, float* dw1, float* dw2, float* scratch,
                        long long scratch_elems, int accumulate /* 1: dwmask / dw1 / dw2 += */, void* stream);

/* One DivEnh band (i >= 1) of MultiFreq_Refinment with its running sums, forward and backward (training path; reference
 * CVSR_freq.py:2104-2133 applied at :2201-2254 with CALayer :1812-1828):  t = f - Sf + 0.2 So, e1 = (0.2 a t + b) f, e2 = (0.2 a So + b) f,
 * So' = So + e1 CA(e1) + e2 CA(e2), Sf' = Sf + f.  Tensors dense (B, HW, C) f32, C in {32, 64}; w1 (C/16, C), w2 (C, C/16).
 * forward scratch >= B * nblk * 2C floats; backward scratch >= B * nblk * 2C + 2BC + 2BC(C/16) floats; stats = B * stat_elems(C) floats. */
int fcvsr_divenh_band_nblk(int HW);
int fcvsr_divenh_band_stat_elems(int C);
int fcvsr_divenh_band_forward(const float* f, const float* sf, const float* so, const float* a, const float* b, const float* w1,
                              const float* w2, int B, int HW, int C, float* sf_out, float* so_out, float* stats, float* scratch,
                              long long scratch_elems, void* stream);
int fcvsr_divenh_band_backward(const float* f, const float* sf, const float* so, const float* a, const float* b, const float* w1,
                               const float* w2, const float* stats, const float* gsf, const float* gso, int B, int HW, int C, float* gf,
                               float* gsf_out, float* gso_out, float* ga, float* gb, float* dw1, float* dw2, float* scratch,
                               long long scratch_elems, int accumulate, void* stream);
/* backward of fcvsr_corr_lookup: g = dL/dcorr on the first x_count columns; gx1 / gx2 dense (B,H,Wf,pix_stride), ZEROED by the caller */
int fcvsr_corr_lookup_bwd(const float* x1f, const float* x2f, int64_t pix_stride, int B, int H, int Wf, int C, int radius, int x_count,
                          const fcvsr_view* g, float* gx1_zeroed, float* gx2_zeroed, void* stream);
/* PReLU with one shared slope (nn.PReLU(), CVSR_freq.py:2590 / ConvBlk :349), slope in device memory:
 *   fcvsr_prelu_fwd: y = x > 0 ? x : slope[0] * x;   fcvsr_prelu_bwd: gx and gslope[0] (two-stage sum; scratch >= 2048 floats). */
int fcvsr_prelu_fwd(const float* x, const float* slope, float* y, long long n, void* stream);
int fcvsr_prelu_bwd(const float* g, const float* x, const float* slope, float* gx, float* gslope, float* scratch, long long n, void* stream);
/* Weight gradient of a 3x3 "same" convolution with ONE output channel (conv_last0, :2607): x dense (B,H,W,C) f32, gy dense (B,H,W) f32,
 * dw (1,C,3,3); C in {16, 32, 64}; x is read once; fixed summation order. */
long long fcvsr_wgrad_cout1_scratch_elems(int B, int H, int C);
int fcvsr_wgrad_cout1(const float* x, const float* gy, int B, int H, int W, int C, float* dw, float* scratch, long long scratch_elems,
                      int accumulate, void* stream);
/* Backward of one IAC iteration under training (CVSR_freq.py:1230-1250; forward = fcvsr_warp, fcvsr_sac_v, fcvsr_sac_h, which leave
 * s = flow_warp(prev, off) and v = SAC_v(s) in memory).  All tensors f32 NHWC; gy, yout (the iteration's output), v, s, gfin, gv, prev,
 * gprev dense (B,H,W,C); k1 / gk: views of the iteration's 3*C kernel channels inside the predictor output / its gradient.
 *   fcvsr_iac_bwd_sac : gfin (+)= gy * lrelu'(yout);  gv = transposed horizontal pass;  gk (+)= both passes' kernel gradients
 *   fcvsr_iac_bwd_warp: gs = transposed vertical pass of gv;  gprev += bilinear scatter of gs (float atomics: gprev must be zeroed);
 *                       goff (B,H,W,2) = d/d(off) of the bilinear sample.  C in {32, 64}. */
int fcvsr_iac_bwd_sac(const float* gy, const float* yout, const float* v, const float* s, const fcvsr_view* k1, float slope, int B, int H,
                      int W, int C, float* gfin, int fin_accumulate, float* gv, const fcvsr_view* gk, int k_accumulate, void* stream);
int fcvsr_iac_bwd_warp(const float* gv, const fcvsr_view* k1, const float* prev, const fcvsr_view* off, int B, int H, int W, int C,
                       float* gprev_zeroed, float* goff, void* stream);
/* fcvsr_iac_bwd_warp without float atomics (flow_warp backward, CVSR_freq.py:1188-1227 inside :1230-1250): same gs, same goff bits, and
 * gprev summed by a gather in a fixed order - two calls on the same inputs give the same bits; against the scatter form only the order
 * of the additions differs.  Three steps on `stream`: the source pass (gs, goff, one destination-cell key per pixel), a stable radix
 * sort of (key, pixel) pairs, the gather.  gprev is written completely (zeros where no source lands) and need not be zeroed.
 * workspace: device memory, 16-byte aligned, at least the byte count the _workspace query returns for the same B, H, W, C; it holds gs,
 * the keys and pixel ids (both sort buffers), the cell index and the sort's scratch, and may be reused by the next call on the stream.
 * C in {32, 64}; B (H+1) (W+1) < 2^31.  A null, misaligned or too small workspace is FCVSR_E_ARG and nothing is launched. */
int fcvsr_iac_bwd_warp_det_workspace(int B, int H, int W, int C, size_t* bytes);
int fcvsr_iac_bwd_warp_det(const float* gv, const fcvsr_view* k1, const float* prev, const fcvsr_view* off, int B, int H, int W, int C,
                           float* gprev, float* goff, void* workspace, size_t workspace_bytes, void* stream);
/* fcvsr_conv2d_wgrad_mfma summed over 1..3 problems that share the weight (the pyramid levels of a BlockRCB layer): one launch per
 * problem into consecutive slab ranges of one scratch buffer and ONE ordered reduction (no per-level gradient tensors). */
long long fcvsr_conv2d_wgrad_mfma_groups_scratch_elems(const int* B, const int* H, const int* W, int n_groups, int cin, int cout, int kh,
                                                       int kw);
int fcvsr_conv2d_wgrad_mfma_groups(const fcvsr_view* xs, const fcvsr_view* gys, const int* B, const int* H, const int* W, int n_groups, int kh,
                                   int kw, int pad, float* dw, float* dbias, float* scratch, long long scratch_elems, int dw_accumulate,
                                   int dbias_accumulate, void* stream);
/* Adjoints of the two resamplings inside fcvsr_xscale (BlockRCB cross-scale sum under training), f32 NHWC:
 *   fcvsr_up2_adjoint:   g (B,2H,2W,C) -> (B,H,W,C), transposed x2 bilinear up-sampling (align_corners = False, clamped);
 *   fcvsr_pool2_adjoint: g (B,H,W,C) -> (B,2H,2W,C), transposed 2x2 mean. */
int fcvsr_up2_adjoint(const float* g, float* out, int B, int H, int W, int C, void* stream);
int fcvsr_pool2_adjoint(const float* g, float* out, int B, int H, int W, int C, void* stream);
/* ---- frequency transforms: torch.fft.rfft2 / irfft2 (norm='backward') of NHWC channel groups -------------
 * Spectrum layout: buffer [B][H][Wf][pix_stride] with Wf=W/2+1; channel c of the group has its imaginary part at
 * channel im_off+c and its real part at re_off+c (the reference packs [imag, real], CVSR_freq.py:1456-1465).
 * fcvsr_rfft2 : real src (B,H,W,n; f32 or 16-bit storage) -> f32 spectrum  (replaces :1452-1465 and the fftn of :2082-2084)
 * fcvsr_irfft2: spectrum (optionally multiplied by a real (H,Wf) mask per group of `mask_every` channels...)
 *               -> real dst (B,H,W,n), scaled 1/(H*W)     (replaces :1497-1505 and the ifftn(...).real of :2085-2090)
 *   work: scratch buffer of the same size as the spectrum region used (B*H*Wf*2n floats), or NULL to run the
 *   column pass in place (destroys the spectrum).  mask: (H,Wf) floats or NULL.
 */
int fcvsr_rfft2(const fcvsr_view* src, int B, int H, int W, int n,
                float* spec, int64_t pix_stride, int im_off, int re_off, void* stream);
int fcvsr_irfft2(const float* spec, int64_t pix_stride, int im_off, int re_off, int B, int H, int W, int n,
                 const float* mask, float* work, const fcvsr_view* dst, void* stream);
/* Band split of MultiFreq_Refinment (reference :2082-2090) in one call: dst[m] = irfft2(spec * masks[m]) for m < n_bands.
 * masks: n_bands contiguous (H,Wf) real masks; work: n_bands * B*H*Wf*pix_stride floats; dst: n_bands f32 views (B,H,W,>=n).
 * When H has a two-stage factorisation the spectrum columns are read once for all bands (results identical to n_bands
 * calls of fcvsr_irfft2, which is also the fallback). */
int fcvsr_irfft2_bands(const float* spec, int64_t pix_stride, int im_off, int re_off, int B, int H, int W, int n,
                       const float* masks, int n_bands, float* work, const fcvsr_view* dst, void* stream);
/* The kernels the calling thread's last successful fcvsr_rfft2 / fcvsr_irfft2 / fcvsr_irfft2_bands call launched: its passes in
 * launch order, joined by ';'.  A pass is "name<R1,R2>/L<lanes>" for a two-stage kernel (length R1 * R2, <lanes> channel lanes per
 * workgroup) or "name/L<lanes>/vec<0|1>" for a multi-stage plan kernel (vec1 = 16-byte accesses); name is the kernel's name without
 * "_kernel".  E.g. "rfft_rows2<16,20>/L16;fft_cols2<12,15>/L32" or "fft_cols/L8/vec1;irfft_rows/L4/vec0".  fcvsr_irfft2_bands on its
 * fused column pass reports "fft_cols2_bands<R1,R2>/L<lanes>" and then the row pass once (not once per band); on its band-by-band
 * fallback the string is that of the last fcvsr_irfft2 call.  "" before the first call.  Test and measurement aid like
 * fcvsr_last_conv_kernel(), not part of the data path. */
const char* fcvsr_last_fft_path(void);
/* ---- focal frequency loss (training): FFL of the reference's Charbonnier_FFL_Loss (CVSR_train/opt/deep_learning.py:192-220) -------
 * For pred, target (B,C,H,W) contiguous f32 and patch_factor f (f | H, f | W): h = H/f, w = W/f, P = B*f*f*C planes, plane
 * p = (b*f*f + i*f + j)*C + c being patch (i,j) of channel c of image b.  With U = rfft2 of pred - target per plane (unnormalised),
 * N = h*w, s = |U|^2 and cw = 1 on the columns kx = 0 and kx = w/2 (even w), 2 elsewhere:
 *   wgt = (s / max over the plane of s)^(alpha/2), 0 where the max is 0;   loss = loss_weight / (P*N*N) * sum cw * wgt * s
 * which equals loss_weight * mean(wgt * |fft2(pred, ortho) - fft2(target, ortho)|^2) over the full spectra, and
 *   d loss / d pred = 2*loss_weight / (P*N) * irfft2 of wgt * U  (wgt taken as a constant),   d loss / d target = -d loss / d pred.
 * Call order: fcvsr_ffl_diff, fcvsr_rfft2 on d as one image (1,h,w,d_channels), fcvsr_ffl_weight; for the gradients fcvsr_irfft2 on the
 * spectrum fcvsr_ffl_weight left, then fcvsr_ffl_grad.  Sums run in a fixed order (no float atomics): results are bit-repeatable.
 * Nothing synchronises or allocates; the loss and the upstream gradient are device scalars.
 *
 * fcvsr_ffl_diff:   d (h,w,d_channels) NHWC f32, d_channels >= P: channel p = the difference of plane p, channels beyond P zero.
 * fcvsr_ffl_weight: spec as fcvsr_rfft2 wrote it for B = 1 (plane p: imaginary part at im_off+p, real at re_off+p, the two ranges
 *                   disjoint); on return it holds wgt * U and *loss the loss.  workspace: at least the number of floats the
 *                   _workspace_elems query returns for the same h, w, P.  alpha > 0.
 * fcvsr_ffl_grad:   r (h,w,r_channels) NHWC f32 = fcvsr_irfft2 of that spectrum; g_up: the upstream gradient (one f32 on the device);
 *                   grad_pred / grad_target: (B,C,H,W) contiguous f32, either may be NULL; grad_target is the exact negation. */
long long fcvsr_ffl_workspace_elems(int h, int w, int P);
int fcvsr_ffl_diff(const float* pred, const float* target, int B, int C, int H, int W, int patch_factor, float* d, int d_channels,
                   void* stream);
int fcvsr_ffl_weight(float* spec, int64_t pix_stride, int im_off, int re_off, int h, int w, int P, float alpha, float loss_weight,
                     float* workspace, long long workspace_elems, float* loss, void* stream);
int fcvsr_ffl_grad(const float* r, int r_channels, const float* g_up, float loss_weight, int B, int C, int H, int W, int patch_factor,
                   float* grad_pred, float* grad_target, void* stream);

/* feat_extract (:2589, Conv2d(Cin, n_blk*64, 3, 1, 1), Cin = 7: 9*Cin <= 64) as one K = 64 GEMM step per output tile.
 * x: (B,H,W,Cin) f32 view of the planar frames; w: [n_blk*64][64] f16, column k = tap*Cin + c (zero beyond 9*Cin);
 * output block i (64 channels) goes to dst[i] (16-bit, dtype dst_dtype) at channel offset dst_ch_off[i], pixels
 * dst_pix_stride[i] elements apart (flat pixel index (b*H + y)*W + x). */
int fcvsr_feat_extract(const fcvsr_view* x, int B, int H, int W, const void* w, const float* bias, int n_blk,
                       void* const* dst, const int64_t* dst_pix_stride, const int32_t* dst_ch_off, int dst_dtype,
                       void* stream);

/* ---- MGAAbk pieces (CVSR_freq.py:1365-1547) ---------------------------------------------------------------- */
/* CorrBlock lookup on the integer grid (:1279-1337): x1f,x2f NHWC (B,H,Wf,C) with pixel stride
 * pix_stride (floats); dst (B,H,x_count,>=81); channels beyond (2r+1)^2 are zero-filled.  Only the first x_count
 * columns are produced (x_count = Wf for the whole map): the lookup is identically zero for x > radius+1, because the
 * reference samples a (C/2 x 2)-pixel image (column index x+i-r must be 0 or 1), so callers may evaluate a strip only */
int fcvsr_corr_lookup(const float* x1f, const float* x2f, int64_t pix_stride, int B, int H, int Wf, int C, int radius,
                      int x_count, const fcvsr_view* dst, void* stream);
/* per-(b,c) sums over (y,x) of a view, deterministic two-stage: out[b][c] (f32).  scratch: B*nblk*C floats */
int fcvsr_channel_sum(const fcvsr_view* src, int B, int H, int W, float* out, float* scratch, int64_t scratch_elems,
                      void* stream);
/* CALayer gate (:1812-1828): gate[b][c] = sigmoid(W2 relu(W1 (sum[b][:]*inv_hw)));  W1 (cr x c), W2 (c x cr) row-major */
int fcvsr_ca_gate(const float* sum, float inv_hw, const float* w1, const float* w2, int B, int c, int cr,
                  float* gate, void* stream);
/* ConvBlk tail + similarity + complex packing (:344-357 `CA(out)+out`, :1495-1498):
 *   o = (u*gate + u) * sim;  u,sim (Bn,H,Wf,4) with u's batch = dir*B+b and sim's batch = b;
 *   writes re (o[0:2]) to spec channel re_off + 2*g + j and im (o[2:4]) to im_off + 2*g + j, g = dir*A + i */
int fcvsr_convblk_tail(const float* u, const float* gate, const float* sim, int B, int ndir, int H, int Wf,
                       float* spec, int64_t pix_stride, int re_off, int im_off, int g_stride, int g0, void* stream);
/* One whole ConvBlk head (:344-357 applied at :1494-1498) in two launches:
 *   u = conv2(PReLU(conv1(x)))  (k x k, 4 -> 4, no bias; w1 / w2 in the direct packing [k*k][4][16] f32, one PReLU slope),
 *   then what fcvsr_convblk_tail does, with the CALayer gate (4 -> 4 -> 4, ca_w1 / ca_w2 row-major, no bias) evaluated from
 *   per-tile channel sums inside the second launch.  x, u_scratch: (ndir*B, H, Wf, 4) f32 dense; sim: (B, H, Wf, 4);
 *   partial_scratch: 4 * ndir*B * ceil(H/16)*ceil(Wf/16) floats. */
int fcvsr_convblk(const float* x, const float* w1, const float* w2, const float* prelu_slope, int ksize, const float* ca_w1,
                  const float* ca_w2, const float* sim, int B, int ndir, int H, int Wf, float* u_scratch,
                  float* partial_scratch, int64_t partial_elems, float* spec, int64_t pix_stride, int re_off, int im_off,
                  int g_stride, int g0, void* stream);
/* All n_heads (1..6) ConvBlk heads of one MGAA call in two launches; head i has k = 2i+1 and the arguments of fcvsr_convblk
 * at index i of w1 / w2 / prelu_slope / ca_w1 / ca_w2 (host arrays of n_heads device pointers).  Two directions (x batch =
 * dir*B + b).  Per head the arithmetic of fcvsr_convblk, in its order: results are bit-identical to n_heads calls with
 * g_stride = n_heads, g0 = i.  u: (n_heads, 2B, H, Wf, 4); partial: (n_heads, 2B, tiles, 4), tiles = ceil(H/16)*ceil(Wf/16).
 * The record of a pixel is written whole: re block [re_off, re_off + 4 n_heads), im block [im_off, im_off + 4 n_heads), channel
 * (dir*n_heads + i)*2 + j inside each; spec, pix_stride, re_off, im_off 16-byte aligned. */
int fcvsr_convblk_heads(const float* x, int n_heads, const float* const* w1, const float* const* w2,
                        const float* const* prelu_slope, const float* const* ca_w1, const float* const* ca_w2, const float* sim,
                        int B, int H, int Wf, float* u, float* partial, int64_t partial_elems, float* spec, int64_t pix_stride,
                        int re_off, int im_off, void* stream);
/* flow_warp (:1188-1227): bilinear, zeros padding, sample at (x+off[0], y+off[1]) */
int fcvsr_warp(const fcvsr_view* src, const fcvsr_view* off, int B, int H, int W, const fcvsr_view* dst, void* stream);
/* SAC (:1253-1276) vertical pass: v = sum_t s[clamp(y+t-1)] * k1[c*3+t] */
int fcvsr_sac_v(const fcvsr_view* s, const fcvsr_view* k1, int B, int H, int W, const fcvsr_view* dst, void* stream);
/* SAC horizontal pass (kernel1 again, :1273) + IAC residual and LeakyReLU(0.1) (:1243-1248) */
int fcvsr_sac_h(const fcvsr_view* v, const fcvsr_view* k1, const fcvsr_view* feat_in, float slope,
                int B, int H, int W, const fcvsr_view* dst, void* stream);

/* One fused IAC iteration (:1230-1250): dst = LeakyReLU_slope(SAC_h(SAC_v(flow_warp(prev, off), k1), k1) + feat_in).
 * k1: the 3*C kernel1 channels of this iteration, f32 or 16-bit; prev / feat_in / dst: f32 or 16-bit (all alike);
 * off f32.  C % 32 == 0. */
int fcvsr_iac_step(const fcvsr_view* prev, const fcvsr_view* off, const fcvsr_view* k1, const fcvsr_view* feat_in,
                   float slope, int B, int H, int W, const fcvsr_view* dst, void* stream);
/* The same iteration for BOTH alignment directions in one launch: prev, off, feat_in and dst point at arrays of 2 views
 * (forward, backward); the two directions share k1 (:1524-1545), which is then read once.  C % 64 == 0. */
int fcvsr_iac_step2(const fcvsr_view* prev, const fcvsr_view* off, const fcvsr_view* k1, const fcvsr_view* feat_in,
                    float slope, int B, int H, int W, const fcvsr_view* dst, void* stream);
/* fcvsr_iac_step2 with the last kernel-predictor layer (F[1], a 1x1 convolution, :1416) folded in: the 3*C adaptive
 * kernel channels of the iteration are computed per tile on the matrix cores from k0 (the 64-channel, 16-bit input of
 * F[1]) and never stored.  wk: this iteration's 192 x 64 weight rows in k0's dtype (cin contiguous, i.e. a row block of
 * the MFMA packing of F[1]); kbias: their 192 f32 biases.  C == 64. */
int fcvsr_iac_step2_fused(const fcvsr_view* prev, const fcvsr_view* off, const fcvsr_view* k0, const void* wk,
                          const float* kbias, const fcvsr_view* feat_in, float slope, int B, int H, int W,
                          const fcvsr_view* dst, void* stream);

/* The whole convfuse stack (:1371-1377, applied at :1472-1474) for up to two alignment directions in one launch:
 *   dst[d] = (xa[d] - xb[d]) + W4 . relu(W2 . relu(W0 . [xa[d] | xb[d]]))     1x1, no bias, 128 channels (n_feats = 64)
 * xa[d], xb[d]: f32 spectra, npix pixels of 128 contiguous channels, src_pix_stride floats apart; dst[d]: bf16, 128 channels,
 * dst_pix_stride halfwords apart; w0 [128][256], w2 / w4 [128][128] bf16 with cin contiguous (the MFMA packing of the three
 * layers).  The two hidden tensors stay on chip. */
int fcvsr_freq_mlp3(const float* const* xa, const float* const* xb, int n_dirs, int64_t src_pix_stride, int64_t npix,
                    const void* w0, const void* w2, const void* w4, void* const* dst, int64_t dst_pix_stride, void* stream);

/* The narrow 1x1 stacks on the spectrum grid as one launch each: out(npix,4) f32 = W_last . relu([W_mid . relu](W_0 . x)),
 * x (npix, 128 channels, x_pix_stride elements apart) f32 or bf16, hidden width 64, bf16 operands / f32 accumulate.
 * w0 [>=64][128], w_mid [>=64][64] or NULL, w_last [>=32][64] (rows 0..3 live) bf16 with cin contiguous (MFMA packing).
 * convcrt (:1392-1396): w_mid = NULL on the centre spectrum; convcorr (:1379-1385) away from the CorrBlock strip: the
 * offset spectra with the first 128 input columns of convcorr.0. */
int fcvsr_freq_head(const void* x, int x_dtype, int64_t x_pix_stride, int64_t npix, const void* w0, const void* w_mid,
                    const void* w_last, float* out, void* stream);
/* convcorr (128 + 84 -> 64 -> 64 -> 4, relu between) on the strip x < xs of the spectrum grid, where the CorrBlock lookup is
 * not identically zero, written into off4 in place (columns >= xs untouched): one launch for both directions.
 * off: (2B, H, Wf, 128) bf16 dense; corr: (B, H, xs, 84) f32 dense (fcvsr_corr_lookup with x_count = xs), shared by the two
 * directions; w0: [>=64][256] bf16 rows = convcorr.0 on the concatenation [off | corr]; w_mid, w_last as in fcvsr_freq_head.
 * The sums run in the order of the generic 1x1 MFMA kernel on that concatenation, so the result equals the separate launches
 * bit for bit. */
int fcvsr_convcorr_strip(const void* off, const float* corr, int B, int H, int Wf, int xs, const void* w0, const void* w_mid,
                         const void* w_last, float* off4, void* stream);

/* ---- MultiFreq_Refinment pieces (CVSR_freq.py:2104-2133, :2201-2254) ---------------------------------------- */
/* DivEnh expressions, i==0 (first=1): t=f-mean_f; e1=0.2*a*t*f+b*f.  i>0: t=f-s_f+0.2*s_o; e1 as above;
 * e2=0.2*a*s_o*f+b*f.   mode 0: write per-(b,c) sums of e1,e2 to sums[2][B][C] (two-stage, deterministic);
 * mode 1: o=e1*g1(+e2*g2); s_f+=f; s_o+=o (in place). All tensors dense NHWC (B,H,W,C). */
int fcvsr_divenh(int mode, int first, const float* f, float* s_f, float* s_o, const float* a, const float* b,
                 const float* mean_f_sum, float inv_hw, const float* g1, const float* g2,
                 float* sums, float* scratch, int64_t scratch_elems, int B, int H, int W, int C, void* stream);
/* mode 1 of fcvsr_divenh for band i fused with the reduction the next step needs (s_f, s_o are touched once):
 *   f_next != NULL: sums[2][B][C] = per-(b,c) sums of e1, e2 of band i+1 (= mode 0 of the next block, bit-identical);
 *   f_next == NULL: sums[0][B][C] = per-(b,c) sums of the updated s_o (input of the final CALayer), sums[1] = 0. */
int fcvsr_divenh_apply_next(int first, const float* f, float* s_f, float* s_o, const float* a, const float* b,
                            const float* mean_f_sum, float inv_hw, const float* g1, const float* g2,
                            const float* f_next, const float* a_next, const float* b_next, float* sums,
                            float* scratch, int64_t scratch_elems, int B, int H, int W, int C, void* stream);
/* One stage of the DivEnh chain without the round trip of the running sums: s_f, s_o are a pointwise recurrence over the
 * bands (s_f_j = s_f_{j-1} + f_j, s_o_j = s_o_{j-1} + e1_j*g1_j + e2_j*g2_j), so the stage for band i replays bands j0..i in
 * registers from the bands themselves (n_bands = i - j0 + 1 <= 4, with the arithmetic of fcvsr_divenh_apply_next) and then
 * accumulates the reduction the next step needs, in fcvsr_divenh_apply_next's partition and order: sums[2][B][C] has the bits
 * the chain of fcvsr_divenh_apply_next calls gives.
 *   ck_s_f, ck_s_o: the running sums after band j0-1 (both NULL: j0 == 0, band f[0] is the first band and g2[0] is not read);
 *   f[k], a[k], b[k], g1[k], g2[k]: band j0+k, its parameters [C] and its gates [B][C];
 *   f_next, a_next, b_next: band i+1 (sums = its e1, e2 sums), or all NULL (sums[0] = channel sums of s_o_i, sums[1] = 0);
 *   out_s_f, out_s_o: where s_f_i / s_o_i are stored, each may be NULL (nothing but the partial sums is written then).
 * C % 4 == 0, 256 % (C/4) == 0, every tensor dense NHWC (B,H,W,C) f32 and 16-byte aligned; scratch >= 2*B*ceil(H*W/256)*C
 * floats.  Other shapes: FCVSR_E_ARG (callers use fcvsr_divenh_apply_next there). */
typedef struct {
  const float* ck_s_f;
  const float* ck_s_o;
  const float* f[4];
  const float* a[4];
  const float* b[4];
  const float* g1[4];
  const float* g2[4];
  const float* mean_f_sum;  /* [B][C] sums of the first band (read when j0 == 0) */
  const float* f_next;
  const float* a_next;
  const float* b_next;
  float*       out_s_f;
  float*       out_s_o;
  float*       sums;
  float*       scratch;
  int64_t      scratch_elems;
  float        inv_hw;
  int32_t      n_bands, B, H, W, C;
} fcvsr_divenh_stage_args;
int fcvsr_divenh_stage(const fcvsr_divenh_stage_args* a, void* stream);
/* out = z*gate[b][c] + x   (final CALayer of MFFR, :2229-2230); x read as x_dtype, out stored as out_dtype */
int fcvsr_scale_add(const float* z, const float* gate, const void* x, int x_dtype, void* out, int out_dtype, int B, int H,
                    int W, int C, void* stream);

/* ---- SCNetbk pieces (CVSR_freq.py:657-822) ------------------------------------------------------------------- */
/* ContextBlock (:657-701): add[b][c] = W2 lrelu0.2(W1 ctx), ctx = sum_p r[p]*softmax_p(r[p].wmask)
 *   scratch: B*nblk*(C+2) floats */
int fcvsr_gc_context(const float* r, const float* wmask, const float* w1, const float* w2, int B, int H, int W, int C,
                     float* add, float* scratch, int64_t scratch_elems, void* stream);
/* second half of fcvsr_gc_context for partials produced by the fused conv epilogue (or any producer of the same layout) */
int fcvsr_gc_finish(const float* partial, int nparts, const float* w1, const float* w2, int B, int C, float* add,
                    void* stream);
/* RCB tail (:722-725): out = lrelu0.2(r + add[b][c]) + z; r is f32, z and out are f32 or 16-bit (io_dtype: trunk16 mode) */
int fcvsr_gc_apply(const float* r, const float* add, const void* z, void* out, int io_dtype, float slope,
                   int B, int H, int W, int C, void* stream);
/* BlockRCB cross-scale sum (:766-777): out = x + r_scale*r + avgpool2(dn) + bilinear_up2(up); dn/up may be NULL.
 * dn is (B,2H,2W,C), up is (B,H/2,W/2,C); all tensors f32 or all 16-bit (io_dtype) */
int fcvsr_xscale(const void* x, const void* r, float r_scale, const void* dn, const void* up, void* out, int io_dtype,
                 int B, int H, int W, int C, void* stream);

/* The three calls above for all pyramid levels of a BlockRCB in ONE launch each (the small levels are launch-latency bound).
 * fcvsr_gc_apply_levels can also emit pool = avgpool2(out) (the bilinear x0.5 of Interpolate, :623-632): the cross-scale
 * 1x1 convolution commutes with that average, so the caller convolves the pooled tensor (a quarter of the pixels) and
 * fcvsr_xscale_levels adds the result as dn at the level's own resolution (dn_pooled = 1). */
typedef struct {
  const float* partial;   /* [B][nparts][C+2] */
  float*       add;       /* [B][C] */
  int32_t      nparts;
} fcvsr_gc_finish_level;
int fcvsr_gc_finish_levels(const fcvsr_gc_finish_level* lv, int n_levels, const float* w1, const float* w2, int B, int C,
                           void* stream);
typedef struct {
  const void*  r;         /* (B,H,W,C), r_dtype: f32 or io_dtype */
  const float* add;       /* [B][C] */
  const void*  z;         /* (B,H,W,C) io_dtype */
  void*        out;       /* (B,H,W,C) io_dtype */
  void*        pool;      /* (B,H/2,W/2,C) io_dtype or NULL (needs even H, W) */
  int32_t      B, H, W;
} fcvsr_gc_apply_level;
int fcvsr_gc_apply_levels(const fcvsr_gc_apply_level* lv, int n_levels, int io_dtype, int r_dtype, float slope, int C,
                          void* stream);
typedef struct {
  const void* x;          /* (B,H,W,C) */
  const void* r;
  const void* dn;         /* NULL, or (B,H,W,C) when dn_pooled, else (B,2H,2W,C) */
  const void* up;         /* NULL or (B,H/2,W/2,C) */
  void*       out;
  float       r_scale;
  int32_t     dn_pooled;
  int32_t     B, H, W;
} fcvsr_xscale_level;
int fcvsr_xscale_levels(const fcvsr_xscale_level* lv, int n_levels, int io_dtype, int C, void* stream);

/* Full-resolution level of BlockRCB's second half in one pass (reference CVSR_freq.py:722-725 + :766-777, level 0; 16-bit
 * storage modes):  R = lrelu(r + add[b], slope) + z  is formed in registers (rounded to the storage type, as the two-kernel
 * sequence fcvsr_gc_apply_levels -> fcvsr_xscale_levels stores it: results are bit-identical to that sequence),
 *   pool = avg_pool2x2(R)            [B, H/2, W/2, C]   (input of down.0, which commutes with the pooling)
 *   out  = x + r_scale * R + bilinear_x2(up)            (up = up.0(R of level 1), [B, H/2, W/2, C], align_corners=False)
 * x, r, z, up, out, pool are NHWC in io_dtype (FCVSR_BF16 / FCVSR_F16), add is f32 [B, C]; C % 8 == 0, H and W even. */
int fcvsr_rcb_level0(const void* x, const void* r, const float* add, const void* z, const void* up, void* out, void* pool,
                     float slope, float r_scale, int io_dtype, int B, int H, int W, int C, void* stream);

/* All of BlockRCB's second half after the ContextBlock terms in two launches (reference :722-725, :766-777; 16-bit storage
 * modes, C = 64).  With R_l = lrelu(r_l + add_l[b], slope) + z_l rounded to the storage type at each level l:
 *   launch 1 (tiles of level 1):  r1 = R1,  u1 = up.0(R1),  u2 = up.0(R2),  out2 = x2 + 2 R2 + down.0(avg_pool2x2(R1))
 *   launch 2 (tiles of level 0):  out0 = x0 + 2 R0 + bilinear_x2(u1),  out1 = x1 + R1 + down.0(avg_pool2x2(R0)) + bilinear_x2(u2)
 * Bit-identical to fcvsr_gc_apply_levels (levels 1, 2, pooled R1) -> fcvsr_conv2d_mfma (up.0 on R1, R2) -> fcvsr_rcb_level0 ->
 * fcvsr_conv2d_mfma (down.0 on the pooled R0, R1) -> fcvsr_xscale_levels (levels 1, 2): values are rounded where that
 * sequence stores them and the 1x1 layers run its lean 1x1 kernel's MFMA sequence.  Level 0 is (B, H, W, 64), level 1
 * (B, H/2, W/2, 64), level 2 (B, H/4, W/4, 64), H and W multiples of 4; every tensor NHWC in io_dtype (FCVSR_BF16 /
 * FCVSR_F16), 16-byte aligned; add[l] f32 [B][64].  w_up / w_dn: the layers' weights as packed for fcvsr_conv2d_mfma in
 * io_dtype (row co = cout co, 64 cin per row); b_up / b_dn f32 [64] or NULL.  r1, u1, u2 are scratch of levels 1, 1, 2
 * written by launch 1 and read by launch 2; no written tensor may alias another tensor of the call. */
typedef struct {
  const void*  x[3];      /* block inputs */
  const void*  r[3];      /* RCB.body.2 outputs */
  const void*  z[3];      /* body.2 outputs */
  const float* add[3];    /* ContextBlock terms */
  void*        out[3];
  void*        r1;
  void*        u1;
  void*        u2;
  const void*  w_up;
  const float* b_up;
  const void*  w_dn;
  const float* b_dn;
  int32_t      B, H, W;   /* level 0 */
} fcvsr_rcb_tail_args;
int fcvsr_rcb_tail(const fcvsr_rcb_tail_args* a, float slope, int io_dtype, int C, void* stream);

/* ---- tail ------------------------------------------------------------------------------------------------------ */
/* nn.PixelShuffle(2) of a dense NHWC tensor (B,H,W,C) -> (B,2H,2W,C/4) (:2634-2635) */
/* ContextBlock softmax-pool partials (:657-701) from a STORED 16-bit r, all pyramid levels in one launch: one [C+2] record per
 * 4 x 32 pixel tile (sum_p exp(l_p - m) r_p[c], m = max l_p, sum exp; l_p = <r_p, wmask>), the layout fcvsr_conv2d_mfma's fused
 * epilogue writes - fcvsr_gc_finish_levels consumes either.  r: dense (B,H,W,64) in r_dtype (BF16 / F16);
 * partial: [B][ceil(H/4)*ceil(W/32)][66] floats. */
typedef struct {
  const void* r;
  float*      partial;
  int32_t     B, H, W;
} fcvsr_gc_partial_level;
int fcvsr_gc_partial_levels(const fcvsr_gc_partial_level* lv, int n_levels, int r_dtype, const float* wmask, int C, void* stream);

int fcvsr_pixel_shuffle(const float* src, float* dst, int B, int H, int W, int C, void* stream);
/* PixelShuffle(2) of a dense f32 (B,H,W,C) tensor into channels [0, C/4) of a 16-bit (bf16 / f16) view (B,2H,2W,dst.c);
 * channels [C/4, dst.c) of the view are written as zeros.  dst.c % 8 == 0, 16-byte-aligned channel-contiguous pixels. */
int fcvsr_pixel_shuffle16(const float* src, const fcvsr_view* dst, int B, int H, int W, int C, void* stream);
/* F.interpolate(scale_factor=4, bilinear, align_corners=False) (:2644): src view (B,H,W,c) -> dst view (B,4H,4W,c) */
int fcvsr_bilinear_up4(const fcvsr_view* src, int B, int H, int W, const fcvsr_view* dst, void* stream);

/* Fused end of the S-model up-sampler (:2605-2607, :2642-2645):
 *   out += conv_last0( PReLU( PixelShuffle2( upconv2(u1) ) ) ),   upconv2 1x1 64->256, conv_last0 3x3 64->1.
 * u1 (B,H2,W2,64) 16-bit; w2 [256][64] in u1's dtype, rows sub-pixel-major (row (2i+j)*64+c = original channel 4c+2i+j),
 * b2 its 256 biases in the same order (or NULL); slope: the shared PReLU scalar; wl [16][64] in u1's dtype, row = tap
 * ky*3+kx of conv_last0 (rows 9..15 zero); bl: its bias (or NULL); out (B,2*H2,2*W2,1) f32 is read-modify-written (it
 * holds the bilinear base skip).  The (B,2*H2,2*W2,64) intermediate is never stored. */
int fcvsr_tail_fused(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                     const float* bl, int B, int H2, int W2, const fcvsr_view* out, void* stream);
/* The same with the bilinear x4 base skip (:2644) evaluated inside the kernel from the centre LR frame, centre (B,H2/2,W2/2,1)
 * f32 (any strides), H2 and W2 even: out is only written, with the bits of fcvsr_bilinear_up4 followed by fcvsr_tail_fused. */
int fcvsr_tail_fused_base(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                          const float* bl, const fcvsr_view* centre, int B, int H2, int W2, const fcvsr_view* out, void* stream);
/* conv_last0 alone (:2607 / :2683; the RGB twins' 3-channel variant): out += bias + conv3x3(u), u (B,H,W,64) dense 16-bit at the
 * OUTPUT resolution, out a (B,H,W,C) f32 view (any strides: the NCHW result), C = 1..3.  w: [16 (C = 1) or 32][64] in u's dtype,
 * row tap*C + c (tap = ky*3 + kx), zero rows past 9C.  Used where fcvsr_tail_fused does not apply (3x3 up-convs). */
int fcvsr_conv_last(const fcvsr_view* u, const void* w, const float* bias, int B, int H, int W, int C, const fcvsr_view* out, void* stream);

/* ---- quality metrics of the evaluation harness (reference CVSR_train/metric/psnr_ssim.py:278-398 calculate_psnr / _ssim /
 * calculate_ssim, applied per frame by cal_psnr_ssim :447-485; the contract is fcvsr_amd/harness/metrics.py) ----------------
 * N frame pairs (N,C,H,W) with element strides host_*_strides[4] = {n, c, y, x}:
 *   sr: quantise = FCVSR_QUANT_NONE: uint8 frames; FCVSR_QUANT_TRUNCATE / _ROUND: f32 in [0,1], quantised in the kernel as
 *       clamp(v, 0, 1) * 255.0f (f32), then truncated toward zero / rounded half-to-even;
 *   hr: uint8 frames.
 * to_y = 1 (C = 3, RGB channel order): both are scored on Y = (65.481 R + 128.553 G + 24.966 B) / 255 + 16 (f64); otherwise every
 * channel is a plane.  PSNR region: crop_border pixels removed on each side; SSIM region: that, shrunk by 5 more per side.
 *   out[2n]   = sum over the PSNR region and the planes of frame n of (sr - hr)^2;
 *   out[2n+1] = sum over the SSIM region and the planes of the SSIM map (11x11 Gaussian host_window[11], C1 = (0.01*255)^2,
 *               C2 = (0.03*255)^2);
 * all in f64.  Per-tile partials go to scratch (>= fcvsr_frame_metrics_scratch_bytes(...) bytes) and are added in a fixed order:
 * two calls on the same input give the same bits.  FCVSR_E_ARG when the SSIM region is empty. */
enum { FCVSR_QUANT_NONE = 0, FCVSR_QUANT_TRUNCATE = 1, FCVSR_QUANT_ROUND = 2 };
long long fcvsr_frame_metrics_scratch_bytes(int N, int C, int H, int W, int crop_border, int to_y);
int fcvsr_frame_metrics(const void* sr, const int64_t* host_sr_strides, int quantise, const uint8_t* hr,
                        const int64_t* host_hr_strides, int N, int C, int H, int W, int crop_border, int to_y,
                        const double* host_window, double* out, void* scratch, long long scratch_bytes, void* stream);
/* The same for 10-bit frames: hr uint16; sr uint16 (FCVSR_QUANT_NONE) or f32 quantised as clamp(v, 0, 1) * 1023.0f.  peak sets
 * the SSIM constants C1 = (0.01*peak)^2, C2 = (0.03*peak)^2 (1023 full scale; HM's 1020 if the caller scores that way; the host
 * makes PSNR = 20 log10(peak / sqrt(mse)) from out[2n]).  to_y is not defined for 10-bit frames: to_y != 0 is FCVSR_E_ARG.
 * Scratch size as fcvsr_frame_metrics_scratch_bytes(..., to_y = 0). */
int fcvsr_frame_metrics_u16(const void* sr, const int64_t* host_sr_strides, int quantise, const uint16_t* hr,
                            const int64_t* host_hr_strides, int N, int C, int H, int W, int crop_border, int to_y,
                            const double* host_window, double peak, double* out, void* scratch, long long scratch_bytes,
                            void* stream);

/* ---- uint8 frame I/O (8-bit decoded frames in, 8-bit SR frames out; contract: Engine.forward_u8 in fcvsr_amd/engine.py) -------
 * tab: a device table of 256 floats, tab[k] = the f32 of pixel value k (the host builds it with torch as
 * uint8 -> .float() / 255), so that a uint8 source enters exactly as the f32 frames of a caller converting on the host.
 * quantise: FCVSR_QUANT_TRUNCATE / _ROUND - an f32 result v is stored as clamp(v, 0, 1) * 255.0f (f32), truncated toward zero /
 * rounded half to even: the bytes the f32 path's output gives after clamp, * 255, optional round and the cast to uint8. */
/* feat_extract with a uint8 (B,H,W,7) view x (dtype FCVSR_U8, strides in bytes); every other argument as the f32 entry point. */
int fcvsr_feat_extract_u8(const fcvsr_view* x, const float* tab, int B, int H, int W, const void* w, const float* bias, int n_blk,
                          void* const* dst, const int64_t* dst_pix_stride, const int32_t* dst_ch_off, int dst_dtype, void* stream);
/* bilinear x4 base from a uint8 (B,H,W,c) view into an f32 (B,4H,4W,c) view */
int fcvsr_bilinear_up4_u8(const fcvsr_view* src, const float* tab, int B, int H, int W, const fcvsr_view* dst, void* stream);
/* the fused S up-sampler tail with a uint8 result: base (B,2*H2,2*W2,1) f32 holds the bilinear base and is only read; the value
 * the f32 entry point would store into it is quantised into out (B,2*H2,2*W2,1), dtype FCVSR_U8. */
int fcvsr_tail_fused_u8(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                        const float* bl, int B, int H2, int W2, const fcvsr_view* base, const fcvsr_view* out, int quantise,
                        void* stream);
/* uint8 frames in, uint8 result, no f32 base at all: centre (B,H2/2,W2/2,1) uint8 is the centre LR frame, read through tab; out
 * gets the bytes of fcvsr_bilinear_up4_u8 followed by fcvsr_tail_fused_u8. */
int fcvsr_tail_fused_base_u8(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                             const float* bl, const fcvsr_view* centre, const float* tab, int B, int H2, int W2,
                             const fcvsr_view* out, int quantise, void* stream);
/* conv_last0 with a uint8 result: base (B,H,W,C) f32 view (the bilinear base, only read), out (B,H,W,C) uint8 view. */
int fcvsr_conv_last_u8(const fcvsr_view* u, const void* w, const float* bias, int B, int H, int W, int C, const fcvsr_view* base,
                       const fcvsr_view* out, int quantise, void* stream);
/* n contiguous uint8 values -> f32 through tab (the window of the configurations whose first layer reads f32) */
int fcvsr_u8_to_f32(const uint8_t* src, const float* tab, long long n, float* dst, void* stream);
/* n contiguous f32 values -> quantised uint8 (the result of the generic conv_last0 of f32 mode) */
int fcvsr_quantise_u8(const float* src, long long n, int quantise, uint8_t* dst, void* stream);
/* chroma up-sampler of the YUV 4:2:0 path: P dense uint8 planes (P,h,w) -> (P,4h,4w), defined as
 * F.interpolate(p.float() / 255, scale_factor=4, mode="bicubic", align_corners=False), clamp(0, 1), * 255, rounded half to even;
 * dst 4-byte aligned. */
int fcvsr_chroma_up4(const uint8_t* src, const float* tab, int P, int h, int w, uint8_t* dst, void* stream);

/* ---- 10-bit frame I/O (10-bit samples in little-endian 16-bit containers in, 10-bit SR samples out; contract:
 * Engine.forward_u16 in fcvsr_amd/engine.py).  The entry points mirror the uint8 ones one for one, with
 *   views of dtype FCVSR_U16 (strides in ELEMENTS, pointers 2-byte aligned);
 *   tab: a device table of 1024 floats, tab[k] = the f32 of sample k (torch: k -> .float() / 1023; full scale 2^10 - 1), 16-byte
 *        aligned.  A sample above 1023 reads tab[1023] (an index clamp, not a mask): the float path's x.clamp(max=1023);
 *   quantise: an f32 result v is stored as clamp(v, 0, 1) * 1023.0f (f32), truncated toward zero / rounded half to even. */
int fcvsr_feat_extract_u16(const fcvsr_view* x, const float* tab, int B, int H, int W, const void* w, const float* bias, int n_blk,
                           void* const* dst, const int64_t* dst_pix_stride, const int32_t* dst_ch_off, int dst_dtype, void* stream);
int fcvsr_bilinear_up4_u16(const fcvsr_view* src, const float* tab, int B, int H, int W, const fcvsr_view* dst, void* stream);
int fcvsr_tail_fused_u16(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                         const float* bl, int B, int H2, int W2, const fcvsr_view* base, const fcvsr_view* out, int quantise,
                         void* stream);
/* out gets the samples of fcvsr_bilinear_up4_u16 followed by fcvsr_tail_fused_u16 */
int fcvsr_tail_fused_base_u16(const fcvsr_view* u1, const void* w2, const float* b2, const float* slope, const void* wl,
                              const float* bl, const fcvsr_view* centre, const float* tab, int B, int H2, int W2,
                              const fcvsr_view* out, int quantise, void* stream);
int fcvsr_conv_last_u16(const fcvsr_view* u, const void* w, const float* bias, int B, int H, int W, int C, const fcvsr_view* base,
                        const fcvsr_view* out, int quantise, void* stream);
int fcvsr_u16_to_f32(const uint16_t* src, const float* tab, long long n, float* dst, void* stream);
int fcvsr_quantise_u16(const float* src, long long n, int quantise, uint16_t* dst, void* stream);
/* P dense uint16 planes (P,h,w) -> (P,4h,4w): the bicubic kernel of fcvsr_chroma_up4 on k / 1023, clamp(0, 1), * 1023, rounded
 * half to even; the four samples of a thread are one 8-byte store: dst 8-byte aligned. */
int fcvsr_chroma_up4_u16(const uint16_t* src, const float* tab, int P, int h, int w, uint16_t* dst, void* stream);

/* ---- training batches from device-resident uint8 / uint16 sequences (reference CVSR_train/opt/data_LD_LR.py:248-344: RandomCrop, Augment,
 * ToTensor; the draws are made on the host, contract: fcvsr_amd/train/data.py) -----------------------------------------------
 * One descriptor per output plane, in DEVICE memory: an s x s window of a uint8 plane whose rows are `pitch` bytes apart,
 *   crop[r][c] = src[(top + r) * pitch + left + c],   A[i][j] = crop[vflip ? s-1-i : i][hflip ? s-1-j : j],
 *   out[y][x]  = tab[ transpose ? A[x][y] : A[y][x] ]          (hflip, then vflip, then transpose(0, 2, 1), as the reference)
 * `src` is the plane's first byte (any alignment).  The library cannot see the descriptors: the caller guarantees that every
 * window lies inside its plane.
 * fcvsr_clip_batch_u16 reads the same descriptor as a window of a plane of 2-byte samples (10-bit values in uint16 containers):
 * `src` is the address of the plane's first sample and must be 2-byte aligned (it need not be 4-byte aligned); `pitch`, `top`
 * and `left` count SAMPLES (the "strides in elements" convention of FCVSR_U16 views),
 *   crop[r][c] = ((const uint16_t*)src)[(top + r) * pitch + left + c],
 * and a sample k reads tab[min(k, 1023)] (an unsigned index clamp, not a mask: 0x8000 .. 0xFFFF read tab[1023]). */
enum { FCVSR_CROP_HFLIP = 1, FCVSR_CROP_VFLIP = 2, FCVSR_CROP_TRANSPOSE = 4 };
typedef struct fcvsr_crop_desc {
  const uint8_t* src;
  int32_t        pitch;     /* bytes (u8) / samples (u16) between rows of the source plane */
  int32_t        top, left;
  int32_t        flags;     /* FCVSR_CROP_* */
} fcvsr_crop_desc;
/* P planes of s x s f32, dense in dst (plane p at dst + p*s*s), one launch; desc: P descriptors (device); tab as above;
 * s % 4 == 0, dst 16-byte aligned. */
int fcvsr_clip_batch_u8(const fcvsr_crop_desc* desc, const float* tab, int P, int s, float* dst, void* stream);
/* the same for planes of uint16 samples; tab: the 1024-float table of the uint16 entry points above */
int fcvsr_clip_batch_u16(const fcvsr_crop_desc* desc, const float* tab, int P, int s, float* dst, void* stream);

/* ---- YUV 4:2:0 <-> planar RGB for the RGB models (specification: fcvsr_amd/harness/colour.py, which the kernels equal bit for
 * bit) ---------------------------------------------------------------------------------------------------------------------------
 * Integer arithmetic with 14-bit fixed-point coefficients r(x) = floor(x * 2^14 + 0.5), which the HOST computes for a matrix
 * (Kr, Kb), a range and a bit depth d (P = 2^d - 1, s = 2^(d-8); limited range: y_off = 16s, luma span 219s, chroma span 224s; full
 * range: y_off = 0, both spans P; c_off = 2^(d-1)); RGB is always full range 0..P.  `>>` is an arithmetic shift:
 *   decode   Yt = cy*(y - y_off) + 2^13, U = up(u) - c_off, V = up(v) - c_off,
 *            R = clip((Yt + rv*V) >> 14), G = clip((Yt - gu*U - gv*V) >> 14), B = clip((Yt + bu*U) >> 14)           (clip to 0..P)
 *   encode   Y = clip(((kr*R + kg*G + kb*B + 2^13) >> 14) + y_off),
 *            cb = -ur*R - ug*G + ub*B and cr = vr*R - vg*G - vb*B at full resolution, unrounded, summed over the two rows of a
 *            chroma sample and over its columns, rounded once, + c_off, clipped.
 * Chroma up-sampling (h x w -> 2h x 2w, indices clamped to the plane) is centre-sited vertically (taps 3 : 1) and, horizontally,
 * FCVSR_CHROMA_CENTER: taps 3 : 1 (JPEG / MPEG-1 siting; the encoder averages the 2x2 block), or FCVSR_CHROMA_LEFT: co-sited with
 * the even luma columns (MPEG-2 / H.264 / HEVC type 0; even columns take the sample, odd ones the mean of two; the encoder weighs
 * columns 2i-1, 2i, 2i+1 by 1, 2, 1 with column -1 read as column 0).
 * The struct is read on the host at call time. */
enum { FCVSR_CHROMA_LEFT = 0, FCVSR_CHROMA_CENTER = 1 };
typedef struct fcvsr_colour {
  int32_t shift;                        /* fixed-point bits of every coefficient: 14 */
  int32_t chroma_loc;                   /* FCVSR_CHROMA_* */
  int32_t y_off, c_off;
  int32_t cy, rv, gu, gv, bu;           /* decode */
  int32_t kr, kg, kb;                   /* encode, luma */
  int32_t ur, ug, ub, vr, vg, vb;       /* encode, chroma */
} fcvsr_colour;
/* N frames: planes y (H x W), u and v (H/2 x W/2), rows dense, frame n of a plane at base + n * stride (strides in samples: a
 * batch of I420 frames in one buffer has y_stride = u_stride = v_stride = H*W*3/2) -> rgb, dense planar (N,3,H,W).  H, W even.
 * One launch.  Rows are moved 8 or 16 bytes at a time when W % 8 == 0, the strides are multiples of 8 (y) and 4 (u, v) samples
 * and the pointers are aligned to 8 (y, rgb) and 4 (u, v) samples; any other even W and any sample-aligned pointers take the
 * scalar form of the same kernel.  The _u16 entry points take 10-bit samples in 16-bit containers (peak 1023; a sample above 1023
 * reads as 1023), the others 8-bit samples. */
int fcvsr_yuv420_to_rgb(const uint8_t* y, const uint8_t* u, const uint8_t* v, int N, int H, int W, long long y_stride,
                        long long u_stride, long long v_stride, const fcvsr_colour* colour, uint8_t* rgb, void* stream);
int fcvsr_yuv420_to_rgb_u16(const uint16_t* y, const uint16_t* u, const uint16_t* v, int N, int H, int W, long long y_stride,
                            long long u_stride, long long v_stride, const fcvsr_colour* colour, uint16_t* rgb, void* stream);
/* The other direction: rgb dense planar (N,3,H,W) -> planes y, u, v addressed as above. */
int fcvsr_rgb_to_yuv420(const uint8_t* rgb, int N, int H, int W, const fcvsr_colour* colour, long long y_stride,
                        long long u_stride, long long v_stride, uint8_t* y, uint8_t* u, uint8_t* v, void* stream);
int fcvsr_rgb_to_yuv420_u16(const uint16_t* rgb, int N, int H, int W, const fcvsr_colour* colour, long long y_stride,
                            long long u_stride, long long v_stride, uint16_t* y, uint16_t* u, uint16_t* v, void* stream);

/* ---- test-time self-ensemble (reference mmedit_train/mmedit/models/common/ensemble.py, SpatialTemporalEnsemble; specification:
 * fcvsr_amd/harness/ensemble.py, which the kernels equal bit for bit) -------------------------------------------------------------
 * Variant i = 0..7 of a frame f (h x w):  A[r][c] = f[i & 2 ? h-1-r : r][i & 1 ? w-1-c : c],  v_i = i & 4 ? transpose(A) : A
 * (reverse columns, then rows, then transpose: the list order of the reference).
 * fcvsr_ensemble_windows: all 8 variants of b windows of T frames, one launch.  src: the dense UNPADDED sequence (N,C,h,w); idx: a
 * DEVICE table (b,T) of frame numbers (a number outside 0..N-1 is clamped), row bi read backwards when reverse = 1.
 *   out_a (4,b,T,C,ceil4(h),ceil4(w)) f32: variants 0..3;   out_t (4,b,T,C,ceil4(w),ceil4(h)) f32: variants 4..7
 * (ceil4: the next multiple of 4), each variant zero-padded at its own bottom / right; every element is written, the padding
 * included.  h and w are arbitrary.  out_a, out_t 16-byte aligned.  The _u8 / _u16 entry points read uint8 / uint16 samples through
 * tab, the table of the uint8 / uint16 entry points above (a uint16 sample above 1023 reads tab[1023]). */
int fcvsr_ensemble_windows(const float* src, int N, int C, int h, int w, const int32_t* idx, int b, int T, int reverse,
                           float* out_a, float* out_t, void* stream);
int fcvsr_ensemble_windows_u8(const uint8_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                              int reverse, float* out_a, float* out_t, void* stream);
int fcvsr_ensemble_windows_u16(const uint16_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                               int reverse, float* out_a, float* out_t, void* stream);
/* The other end, one launch: a (4,b,C,4 ceil4(h),4 ceil4(w)) and at (4,b,C,4 ceil4(w),4 ceil4(h)), dense f32, 16-byte aligned, are
 * the model's outputs o_i for variants 0..3 and 4..7.  Each is cropped to its top-left 4h x 4w (4w x 4h), the inverse of its variant
 * is applied (transpose if i & 4, then reverse rows if i & 2, then reverse columns if i & 1), and
 *   acc = o_0;  acc = acc + o_i for i = 1..7 (each sum rounded once in f32, no FMA);  mean8 = acc * 0.125f.
 * ra / rat (both or neither): the same pair for the time-reversed windows; the result is then (mean8 + mean8_rev) * 0.5f.
 * out: dense (b,C,4h,4w).  out_dtype FCVSR_F32 (quantise = FCVSR_QUANT_NONE; 16-byte aligned), FCVSR_U8 or FCVSR_U16 (quantise =
 * FCVSR_QUANT_TRUNCATE / _ROUND: clamp(v, 0, 1) * 255.0f or * 1023.0f, as the uint8 / uint16 entry points above; aligned to 4
 * samples). */
int fcvsr_ensemble_merge(const float* a, const float* at, const float* ra, const float* rat, int b, int C, int h, int w,
                         int out_dtype, int quantise, void* out, void* stream);
/* ---- tiled inference (specification: fcvsr_amd/harness/tiles.py, which the kernels equal bit for bit) ---------------------------
 * Geometry in LR pixels on the frame zero-padded at its bottom / right to multiples of 4, Hp x Wp = ceil4(h) x ceil4(w).  Every tile
 * is th x tw (multiples of 4, th <= Hp, tw <= Wp); tile (ky, kx) of the ny x nx grid starts at (ys[ky], xs[kx]).  ys (ny) and xs (nx)
 * are int32 DEVICE tables; a start outside [0, Hp - th] / [0, Wp - tw] is clamped into it.
 * fcvsr_tile_windows: all tile windows of b windows of T frames, one launch.  src: the dense UNPADDED sequence (N,C,h,w); idx: a
 * DEVICE table (b,T) of frame numbers (a number outside 0..N-1 is clamped).  out (b,ny,nx,T,C,th,tw) f32, 16-byte aligned: sample
 * (y, x) of tile (ky, kx) is the frame's sample (ys[ky] + y, xs[kx] + x), 0 outside h x w; every element is written.  The _u8 / _u16
 * entry points read uint8 / uint16 samples through tab, as fcvsr_ensemble_windows_u8 / _u16 do. */
int fcvsr_tile_windows(const float* src, int N, int C, int h, int w, const int32_t* idx, int b, int T, const int32_t* ys, int ny,
                       const int32_t* xs, int nx, int th, int tw, float* out, void* stream);
int fcvsr_tile_windows_u8(const uint8_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                          const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, float* out, void* stream);
int fcvsr_tile_windows_u16(const uint16_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                           const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, float* out, void* stream);
/* The other end, one launch: tiles (b,ny,nx,C,4th,4tw), dense f32, 16-byte aligned, are the model's outputs for the tile windows;
 * wy (ny,4Hp) and wx (nx,4Wp; 16-byte aligned) are the normalised per-axis f32 blend weights (harness/tiles.py axis_weights).  For
 * the output pixel (Y, X) of plane (bi, c), in f32, each operation rounded once, no FMA:
 *   acc = 0;  for ky ascending, then kx ascending, over the tiles with 4 ys[ky] <= Y < 4 (ys[ky] + th), 4 xs[kx] <= X < 4 (xs[kx] + tw):
 *     acc = acc + (wy[ky][Y] * wx[kx][X]) * tiles[bi][ky][kx][c][Y - 4 ys[ky]][X - 4 xs[kx]]
 * out: dense (b,C,4h,4w) (the crop of the padded frame), out_dtype / quantise / alignment as fcvsr_ensemble_merge. */
int fcvsr_tile_merge(const float* tiles, const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, const float* wy,
                     const float* wx, int b, int C, int h, int w, int out_dtype, int quantise, void* out, void* stream);
/* ---- static tiles (harness/tiles.py, static_map_host): tile windows that did not change are not run again ----------------------
 * fcvsr_tile_pairs_equal: pairs is a DEVICE table (P,2) of frame numbers (clamped into 0..N-1).  out (P,ny,nx) uint8: 1 where the
 * two frames of the pair hold the same bits - bytes, 16-bit words (the raw word, not min(k, 1023)) or 32-bit patterns (+0.0 and
 * -0.0 differ, equal NaN patterns agree) - in every sample of all C planes on the tile's rectangle clipped to the frame,
 * [ys[ky], min(ys[ky] + th, h)) x [xs[kx], min(xs[kx] + tw, w)); 0 otherwise.  No load leaves that rectangle.  Two launches, no
 * atomics: scratch (device, any alignment) takes one flag per tile segment, scratch_bytes >=
 * P * ny * nx * ceil(C * th * ceil(tw * sample bytes / 16) / FCVSR_TILE_EQ_SEG_CHUNKS). */
#define FCVSR_TILE_EQ_SEG_CHUNKS 1024
int fcvsr_tile_pairs_equal(const float* src, int N, int C, int h, int w, const int32_t* pairs, int P, const int32_t* ys, int ny,
                           const int32_t* xs, int nx, int th, int tw, uint8_t* scratch, long long scratch_bytes, uint8_t* out,
                           void* stream);
int fcvsr_tile_pairs_equal_u8(const uint8_t* src, int N, int C, int h, int w, const int32_t* pairs, int P, const int32_t* ys, int ny,
                              const int32_t* xs, int nx, int th, int tw, uint8_t* scratch, long long scratch_bytes, uint8_t* out,
                              void* stream);
int fcvsr_tile_pairs_equal_u16(const uint16_t* src, int N, int C, int h, int w, const int32_t* pairs, int P, const int32_t* ys, int ny,
                               const int32_t* xs, int nx, int th, int tw, uint8_t* scratch, long long scratch_bytes, uint8_t* out,
                               void* stream);
/* fcvsr_tile_windows_sel: the tile windows a DEVICE table sel (n,3) of int32 rows (bi, ky, kx) names, each entry clamped into its
 * range; rows may repeat and come in any order.  out (n,T,C,th,tw) f32, 16-byte aligned: out[k] holds the bits of
 * fcvsr_tile_windows' out[bi][ky][kx].  Everything else as fcvsr_tile_windows. */
int fcvsr_tile_windows_sel(const float* src, int N, int C, int h, int w, const int32_t* idx, int b, int T, const int32_t* ys, int ny,
                           const int32_t* xs, int nx, int th, int tw, const int32_t* sel, int n, float* out, void* stream);
int fcvsr_tile_windows_sel_u8(const uint8_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                              const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, const int32_t* sel, int n,
                              float* out, void* stream);
int fcvsr_tile_windows_sel_u16(const uint16_t* src, const float* tab, int N, int C, int h, int w, const int32_t* idx, int b, int T,
                               const int32_t* ys, int ny, const int32_t* xs, int nx, int th, int tw, const int32_t* sel, int n,
                               float* out, void* stream);
/* fcvsr_tile_merge_sel: fcvsr_tile_merge on tiles[bi][ky][kx] = pool[slots[bi][ky][kx]] without that tensor: pool (n,C,4th,4tw)
 * dense f32, 16-byte aligned; slots a DEVICE table (b,ny,nx) of int32 (clamped into 0..n-1).  The same blend, order, quantisers. */
int fcvsr_tile_merge_sel(const float* pool, int n, const int32_t* slots, const int32_t* ys, int ny, const int32_t* xs, int nx, int th,
                         int tw, const float* wy, const float* wx, int b, int C, int h, int w, int out_dtype, int quantise, void* out,
                         void* stream);
/* ---- NIQE block features and the MATLAB-style bicubic down-scale (reference mmedit/core/evaluation/metrics.py:398-590
 * estimate_aggd_param / compute_feature / niqe_core / niqe, used by CVSR_train/metric/cal_VideoLQ.py; the down-scale is
 * mmedit/datasets/pipelines/matlab_like_resize.py; the contract is fcvsr_amd/harness/niqe.py) ------------------------------------
 * frames: N frames (N,C,H,W) with element strides host_strides[4] = {n, c, y, x}: uint8 (quantise = FCVSR_QUANT_NONE), or f32 in
 * [0,1] quantised as fcvsr_frame_metrics does (FCVSR_QUANT_TRUNCATE / _ROUND).  C = 1 (to_y = 0), or C = 3 in RGB order with
 * to_y = 1: the plane is then Y = (65.481 R + 128.553 G + 24.966 B) / 255 + 16 rounded half to even (metrics.py:576-585).
 * The scored plane is the frame with crop_border pixels removed on each side, cropped to the top-left (floor(h/96) 96,
 * floor(w/96) 96); FCVSR_E_ARG when it holds fewer than 2 blocks.  host_window[49]: the 7 x 7 MSCN window as CORRELATION taps
 * (the model's gaussian_window flipped in both axes), borders replicated.  tables: DEVICE (4, 9801) f64 over the grid
 * g = 0.2, 0.201 .. 10: G(2/g)^2 / (G(1/g) G(3/g)), sqrt(G(1/g) / G(3/g)), G(2/g) / G(1/g), g (harness/niqe.py aggd_tables).
 * out: DEVICE (N, blocks, 36) f64, blocks in row-major order: per block the 18 AGGD features of compute_feature (:428-451) at
 * scale 1, then at scale 2 (the 2x down-scale below applied to plane / 255, times 255; blocks of 48 x 48).  A block side with no
 * sample (no negative or no positive value) gives alpha = 0.2 and NaN in the block's other entries of that distribution, as the
 * reference's argmin over NaN does.  Everything from the integer samples on is f64 except the down-scale, which has the
 * reference's f32 arithmetic; reductions have a fixed shape and use no atomics: two calls give the same bits.  No host sync.
 * scratch: >= fcvsr_niqe_scratch_bytes(...) bytes, 8-byte aligned. */
long long fcvsr_niqe_scratch_bytes(int N, int H, int W, int crop_border);
int fcvsr_niqe_features(const void* frames, const int64_t* host_strides, int quantise, int N, int C, int H, int W, int crop_border,
                        int to_y, const double* host_window, const double* tables, double* out, void* scratch,
                        long long scratch_bytes, void* stream);
/* ---- BRISQUE features (reference CVSR_train/metric/brisque.py natural_scene_statistics / estimate_ggd_param /
 * estimate_aggd_param / normalize_img_with_guass; the contract is fcvsr_amd/harness/brisque.py) -----------------------------------
 * frames, host_strides, quantise as fcvsr_niqe_features.  C = 1 (to_y = 0), or C = 3 in RGB order with to_y = 1: the plane is then
 * the luma of YIQ in integers, round_half_even((299 R + 587 G + 114 B) / 1000) - not the Y of YCbCr that NIQE scores.  The whole
 * frame is scored; H and W even and >= 16, else FCVSR_E_ARG.  host_window[49]: the 7 x 7 MSCN window as correlation taps; the
 * plane's border is ZERO-padded and sigma = sqrt(|E[x^2] - mu^2| + 2^-23).  tables: DEVICE (4, 9801) f64 over the grid
 * g = 0.2, 0.201 .. 10: G(1/g) G(3/g) / G(2/g)^2, G(2/g)^2 / (G(1/g) G(3/g)), G(2/g) / sqrt(G(1/g) G(3/g)), g (harness/brisque.py
 * brisque_tables).
 * out: DEVICE (N, 36) f64: per scale (the frame, then the 2x down-scale above applied to plane / 255, times 255) alpha and sigma^2
 * of the MSCN plane's GGD fit and (alpha, eta, sigma_l^2, sigma_r^2) of the AGGD fit of the MSCN plane times itself rolled by
 * (0,1), (1,0), (1,1), (-1,1) circularly over the whole plane.  A product with no negative or no positive sample gives
 * alpha = 0.2 and NaN where the formulas give NaN.  f64 from the integer samples on, except the down-scale; reductions have a fixed
 * shape and use no atomics: two calls give the same bits.  No host sync.
 * scratch: >= fcvsr_brisque_scratch_bytes(...) bytes, 8-byte aligned. */
long long fcvsr_brisque_scratch_bytes(int N, int H, int W);
int fcvsr_brisque_features(const void* frames, const int64_t* host_strides, int quantise, int N, int C, int H, int W, int to_y,
                           const double* host_window, const double* tables, void* scratch, long long scratch_bytes, double* out,
                           void* stream);
/* MATLABLikeResize at scale 1/factor (matlab_like_resize.py:72-165), factor 2 or 4, of `planes` dense H x W planes (H, W multiples
 * of factor; src_dtype FCVSR_U8 or FCVSR_F32) into dense f32 (H/factor, W/factor) planes, both passes in one launch: rows first,
 * then columns; output i reads the 4 factor inputs factor i - 3 factor / 2 .. with the antialiased cubic taps
 * [-3,-9,29,111,111,29,-9,-3]/256 (2x) or [-7,-45,-75,-49,93,399,745,987,...mirrored]/4096 (4x), out-of-range indices reflected
 * with edge repeat (-1 -> 0, n -> n-1).  The reference's arithmetic and bits: f32 products added in tap order in f32, no FMA.  At 4x
 * this is the standard "BI" LR maker. */
int fcvsr_bicubic_downscale(const void* src, int src_dtype, long long planes, int H, int W, int factor, float* out, void* stream);
/* MATLABLikeResize at scale factor (matlab_like_resize.py:72-165), factor 2 or 4: MATLAB imresize's bicubic (a = -0.5), the
 * "Bicubic" row of SR tables.  `planes` dense H x W planes (any H, W >= 1; src_dtype FCVSR_U8, FCVSR_U16 or FCVSR_F32; a uint16
 * sample above 1023 reads as 1023) into dense (factor H, factor W) planes, both passes in one launch: rows first, then columns.
 * Output o has its centre at c = (o + 0.5) / factor - 0.5 and reads the 4 inputs floor(c) - 1 .. floor(c) + 2 with the cubic taps of
 * phase o mod factor,
 *   2x: [-3,29,111,-9]/128, [-9,111,29,-3]/128
 *   4x: [-45,399,745,-75]/1024, [-7,93,987,-49]/1024, [-49,987,93,-7]/1024, [-75,745,399,-45]/1024
 * out-of-range indices reflected with edge repeat (-1 -> 0, -2 -> 1, n -> n-1; period 2n).  The reference's arithmetic and bits: f32
 * products added in tap order in f32, no FMA.  out_dtype FCVSR_F32: the sums as they are, on the input's scale (out 16-byte
 * aligned).  out_dtype = src_dtype for FCVSR_U8 / FCVSR_U16: clipped to [0, 255] / [0, 1023] and rounded half to even, what imresize
 * returns for an integer image (out aligned to four samples).  FCVSR_E_ARG: a null pointer, another factor or dtype pair, H, W or
 * planes < 1. */
int fcvsr_bicubic_upscale(const void* src, int src_dtype, long long planes, int H, int W, int factor, void* out, int out_dtype,
                          void* stream);
/* MATLABLikeResize at any output size (matlab_like_resize.py:72-250, scale= or output_shape=): `planes` dense H x W planes (src_dtype
 * FCVSR_U8, FCVSR_U16 or FCVSR_F32; a uint16 sample above 1023 reads as 1023) into dense Ho x Wo planes, both passes in one launch.
 * The taps come from two DEVICE tables per axis that the host makes (fcvsr_amd/harness/resize.py resize_tables): output o of the
 * row axis reads the Py consecutive input rows firsty[o] .. firsty[o] + Py - 1, out-of-range indices reflected with edge repeat
 * (period 2 H), with the f32 weights wy[o * Py + k]; wx (Wo, Px) and firstx (Wo) do the same for columns.  firsty / firstx do not
 * decrease, and neighbouring outputs are at most 8 inputs apart (per-axis scale >= 1/8).  rows_first != 0: the row pass (dim 0)
 * first, then the column pass; 0: columns first - the reference runs the axis with the smaller scale first, rows on a tie.  The
 * reference's arithmetic and bits: the first pass reads the samples as f32, every product is an f32, products are added in tap
 * order in f32 (no FMA), the intermediate is an f32.  out_dtype FCVSR_F32: the sums as they are; out_dtype = src_dtype for FCVSR_U8 /
 * FCVSR_U16: clipped to [0, 255] / [0, 1023] and rounded half to even.  Scalar stores: src and out aligned to their sample size, the
 * tables to 4 bytes.  FCVSR_E_ARG before any device call: a null pointer, a size < 1, Py or Px outside 1 .. 34, another dtype pair,
 * Ho / H or Wo / W outside [1/8, 8], a misaligned pointer. */
int fcvsr_imresize(const void* src, int src_dtype, long long planes, int H, int W, int Ho, int Wo, const float* wy, const int* firsty,
                   int Py, const float* wx, const int* firstx, int Px, int rows_first, void* out, int out_dtype, void* stream);
/* ---- scene-cut statistic (no counterpart in the reference, whose clips are single shots; the contract is
 * fcvsr_amd/harness/shots.py, pair_sad_host) ----------------------------------------------------------------------------------------
 * frames: N dense frames of `samples` samples each (samples = C H W, any value >= 1), elem_size 1 (uint8) or 2 (uint16, a sample
 * above 1023 reads as 1023); aligned to elem_size.  out: DEVICE (N - 1) int64, out[i] = sum over all samples of
 * |frame[i + 1] - frame[i]|, in exact integers: two launches, u64 partial sums per workgroup added in a fixed order, no atomics.
 * N = 1 writes nothing.  scratch: DEVICE, 8-byte aligned, at least (N - 1) * ceil(samples * elem_size / FCVSR_PAIR_SAD_TILE_BYTES) * 8
 * bytes.  No host sync.  FCVSR_E_ARG: a null pointer, another elem_size, N or samples < 1, a scratch that is too small. */
#define FCVSR_PAIR_SAD_TILE_BYTES 1024
int fcvsr_frame_pair_sad(const void* frames, int elem_size, int N, long long samples, void* scratch, long long scratch_bytes,
                         long long* out, void* stream);
/* ---- letterbox-aware SR (no counterpart in the reference, whose clips carry no bars; the contract is
 * fcvsr_amd/harness/active.py, line_sums_host / compose_host) ------------------------------------------------------------------------
 * Line sums.  frames: N dense frames of C planes of H x W samples, elem_size 1 (uint8) or 2 (uint16, a sample above 1023 reads as
 * 1023); aligned to elem_size, nothing more.  rows: DEVICE (N, H) int64, rows[n][h] = sum over all channels and columns of row h;
 * cols: DEVICE (N, W) int64, the same over all channels and rows, in exact integers: every sample is read once, a workgroup writes
 * u32 partial sums and a second launch adds them in a fixed order, no atomics.  scratch: DEVICE, 4-byte aligned, at least
 * N * (ceil(W * elem_size / FCVSR_LINE_SUMS_SPAN_BYTES) * H + ceil(H / FCVSR_LINE_SUMS_ROWS) * W) * 4 bytes.  No host sync.
 * FCVSR_E_ARG: a null pointer, another elem_size, a size < 1, N > 65535, C > 4096, a scratch that is too small. */
#define FCVSR_LINE_SUMS_SPAN_BYTES 1024
#define FCVSR_LINE_SUMS_ROWS 128
int fcvsr_frame_line_sums(const void* frames, int elem_size, int N, int C, int H, int W, void* scratch, long long scratch_bytes,
                          long long* rows, long long* cols, void* stream);
/* Compose.  out: dense (B, C, 4H, 4W) frames of `dtype` (FCVSR_U8, FCVSR_U16 or FCVSR_F32), every sample written once, one launch.
 * Rows 4 top .. 4 bottom x columns 4 left .. 4 right are copied from `sr`, the (B, C, 4 (bottom - top), 4 (right - left)) frames of a
 * resolver that saw the box only, with the strides sr_s* (in samples; a view is fine).  Everything else is fcvsr_bicubic_upscale at
 * factor 4 of the LR centre frames, bit for bit (integer dtypes: clipped and rounded half to even; FCVSR_F32: the f32 sums): frame
 * k of the group is frame centres[k] (DEVICE int32, B of them, each a valid frame number of `frames`: the caller checks) of the
 * resident frames, whose frame, plane and row pitch are f_sb, f_sc, f_sy samples; H, W are the true frame size, at which the border
 * is reflected.  FCVSR_E_ARG: a null pointer, another dtype, a size < 1, B * C > 65535, a box outside the frame, a negative stride,
 * a misaligned pointer (out: four samples). */
int fcvsr_active_compose(const void* sr, long long sr_sb, long long sr_sc, long long sr_sy, long long sr_sx, const void* frames,
                         const int* centres, long long f_sb, long long f_sc, long long f_sy, int dtype, int B, int C, int H, int W,
                         int top, int bottom, int left, int right, void* out, void* stream);
/* ---- raw 4:2:0 surfaces <-> plane rings: the two ends of the streamed YUV path (no counterpart in the reference; the contract is
 * fcvsr_amd/harness/surfaces.py, unpack_host / pack_host) -------------------------------------------------------------------------
 * The formats carry ffmpeg's names: planar I420 in 8 bits and in little-endian 16-bit words (10-bit value in the low bits), NV12
 * (Y plane, then H/2 rows of W bytes U0 V0 U1 V1 ...) and P010 (the NV12 layout in 16-bit words, the 10-bit value in the HIGH bits:
 * word = value << 6; the low six bits are ignored on the way in and zero on the way out).  A frame is H W 3/2 samples, H and W even.
 *
 * fcvsr_surface_unpack: raw holds n frames back to back as they were read (aligned to the sample size, nothing more); slots n
 * DEVICE ints.  The luma of frame i goes to slot slots[i] of ring_y, R slots of Hp x Wp samples (Hp >= H, Wp >= W: the rows and
 * columns beyond H, W are never written), U and V to the same slot of ring_u / ring_v, R slots of H/2 x W/2 samples.  Planar 16-bit
 * samples pass through unchanged, values above 1023 included.  A slot number outside [0, R) writes nothing; two frames of one call
 * must not share a slot.
 * fcvsr_surface_pack: y (b,H,W), u and v (b,H/2,W/2), dense planes whose frames are y_stride / u_stride / v_stride SAMPLES apart
 * (three tensors, or the planes of a batch of I420 frames) -> out, b dense frames of the format's layout.
 * One launch each on `stream`, no host sync; neither reads or writes outside a frame.  FCVSR_E_ARG before any device call: an
 * unknown format, an odd or non-positive size, more than 65535 frames, a null or misaligned pointer, a ring smaller than a frame. */
enum fcvsr_surface { FCVSR_SURFACE_YUV420P = 0, FCVSR_SURFACE_YUV420P10LE = 1, FCVSR_SURFACE_NV12 = 2, FCVSR_SURFACE_P010LE = 3 };
int fcvsr_surface_unpack(const void* raw, int fmt, int n, int H, int W, const int* slots, int R, int Hp, int Wp, void* ring_y,
                         void* ring_u, void* ring_v, void* stream);
int fcvsr_surface_pack(const void* y, const void* u, const void* v, long long y_stride, long long u_stride, long long v_stride,
                       int fmt, int b, int H, int W, void* out, void* stream);
/* ---- full-reference scoring of delivered planes (the reference's cal_psnr_ssim works on files on the host; the contract is
 * fcvsr_amd/harness/reference.py, plane_sse_host) ----------------------------------------------------------------------------------
 * a, b: P planes each of h x w samples with dense rows, whose planes are a_stride / b_stride SAMPLES apart (three tensors, the Y, U
 * or V planes of a batch of I420 frames, slices of a ring: read where they lie); elem_size 1 (uint8) or 2 (uint16, a sample above
 * 1023 reads as 1023); aligned to elem_size, nothing more.  out: DEVICE (P) int64, out[p] = sum of (a - b)^2 over the rows
 * [crop, h - crop) and columns [crop, w - crop) of plane p, in exact integers: two launches, u64 partial sums per workgroup added in
 * a fixed order, no atomics, no float.  Nothing outside the cropped region is read.  P = 0 writes nothing.  scratch: DEVICE, 8-byte
 * aligned, at least P * ceil((w - 2 crop) * elem_size / FCVSR_PLANE_SSE_SPAN_BYTES) * ceil((h - 2 crop) / FCVSR_PLANE_SSE_ROWS) * 8
 * bytes.  No host sync.  FCVSR_E_ARG before any device call: another elem_size, P outside 0 .. 65535, h or w outside 1 .. 2^20,
 * crop < 0 or 2 crop >= min(h, w), a negative stride, a null or misaligned pointer, a scratch that is too small. */
#define FCVSR_PLANE_SSE_SPAN_BYTES 1024
#define FCVSR_PLANE_SSE_ROWS 32
int fcvsr_plane_sse(const void* a, const void* b, int elem_size, int P, int h, int w, long long a_stride, long long b_stride, int crop,
                    void* scratch, long long scratch_bytes, long long* out, void* stream);
/* ---- tOF: dense Farneback flow and the end-point distance of two flows (csrc/flow.hip; the contract is fcvsr_amd/harness/tof.py,
 * farneback_host: a restatement of cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0) by reading; cv2 was never
 * run against it) -----------------------------------------------------------------------------------------------------------------
 * prev, next: P planes each of h x w samples with dense rows, stride_prev / stride_next SAMPLES apart (planes[:-1] and planes[1:] of
 * one buffer are the two arguments).  elem: FCVSR_FLOW_U8, _U16 (a sample above 1023 reads as 1023), _F32, or _RGB8: every "plane"
 * is three dense uint8 planes R, G, B (3 h w samples) read as the float Y ((65.481 R + 128.553 G) + 24.966 B) / 255 + 16.
 * flow_out: DEVICE f32 (P,h,w,2), [dx, dy] from prev to next.  All arithmetic is f32 in a fixed order that depends on neither P nor
 * the launch geometry: the flow of a pair is the same bits in any batch.  No atomics, no host sync.  scratch: DEVICE, 16-byte
 * aligned, at least fcvsr_farneback_scratch_bytes(P, h, w) bytes (-1 for sizes outside the limits below).
 * Layouts: a polynomial expansion R is (images,h,w,FCVSR_FLOW_R_CHANNELS) f32, channels (y, x, yy, xx, xy, 0, 0, 0): one pixel is
 * two 16-byte words, which is what the four-neighbour gather and the stores want; the matrices M are planar (P,5,h,w) f32 (g11, g12,
 * g22, h1, h2), what the 15x15 box sums read row by row.
 * FCVSR_E_ARG before any device call: another elem, P outside 0 .. 65535, h or w outside 2 .. 16384, a negative stride, a null or
 * misaligned pointer, a scratch that is too small.  P = 0 writes nothing. */
enum fcvsr_flow_elem { FCVSR_FLOW_U8 = 0, FCVSR_FLOW_U16 = 1, FCVSR_FLOW_F32 = 2, FCVSR_FLOW_RGB8 = 3 };
#define FCVSR_FLOW_R_CHANNELS 8
long long fcvsr_farneback_scratch_bytes(int P, int h, int w);
int fcvsr_farneback_flow(const void* prev, const void* next, int elem, int P, int h, int w, long long stride_prev, long long stride_next,
                         void* scratch, long long scratch_bytes, float* flow_out, void* stream);
/* flow_a, flow_b: DEVICE f32 (P,h,w,2), dense.  out: DEVICE f64 (P), out[p] = the mean over pixels of sqrt(ddx^2 + ddy^2), each
 * value in f32 (a correctly rounded square root), added in f64: fixed-order partial sums per workgroup, then a second launch.
 * scratch: DEVICE, 8-byte aligned, at least fcvsr_flow_epe_scratch_bytes(P, h, w) bytes. */
long long fcvsr_flow_epe_scratch_bytes(int P, int h, int w);
int fcvsr_flow_epe(const float* flow_a, const float* flow_b, int P, int h, int w, void* scratch, long long scratch_bytes, double* out,
                   void* stream);
/* The stages of fcvsr_farneback_flow, one launch each, as the whole flow runs them (the tests pin each to the host contract).
 * level_image: P planes -> out (P,hl,wl), the blurred and resized image of pyramid level `level` (0 .. 3; hl = round_half_even(h /
 * 2^level)).  poly_exp: img (n,h,w) -> R (n,h,w,8).  matrices: R0, R1 (P,h,w,8), flow (P,h,w,2) -> M (P,5,h,w).  box_solve: M ->
 * flow (P,h,w,2), the 15x15 box average and the 2x2 solve. */
int fcvsr_flow_level_image(const void* src, int elem, int P, int h, int w, long long stride, int level, float* out, void* stream);
int fcvsr_flow_poly_exp(const float* img, int n, int h, int w, float* R, void* stream);
int fcvsr_flow_matrices(const float* R0, const float* R1, const float* flow, int P, int h, int w, float* M, void* stream);
int fcvsr_flow_box_solve(const float* M, int P, int h, int w, float* flow, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* FCVSR_HIP_H */
