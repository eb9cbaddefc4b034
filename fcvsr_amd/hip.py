"""ctypes binding of libfcvsr_hip.so (C ABI declared in include/fcvsr_hip.h).

PyTorch is used only as the owner of device memory and streams: tensors are handed to the library as raw device
pointers + strides (``fcvsr_view``) and every call enqueues on ``torch.cuda.current_stream()``.
There is NO fallback: if the shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfcvsr_hip.so")

F32, BF16, F16, U8, U16 = 0, 1, 2, 3, 4
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_PRELU = 0, 1, 2, 3
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.uint8: U8, torch.uint16: U16}


class View(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("sb", C.c_int64), ("sy", C.c_int64), ("sx", C.c_int64), ("sc", C.c_int64),
                ("c", C.c_int32), ("dtype", C.c_int32)]


class GcFinishLevel(C.Structure):
    _fields_ = [("partial", C.c_void_p), ("add", C.c_void_p), ("nparts", C.c_int32)]


class GcPartialLevel(C.Structure):
    _fields_ = [("r", C.c_void_p), ("partial", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class GcApplyLevel(C.Structure):
    _fields_ = [("r", C.c_void_p), ("add", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p), ("pool", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class XscaleLevel(C.Structure):
    _fields_ = [("x", C.c_void_p), ("r", C.c_void_p), ("dn", C.c_void_p), ("up", C.c_void_p), ("out", C.c_void_p),
                ("r_scale", C.c_float), ("dn_pooled", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class RcbTailArgs(C.Structure):
    _fields_ = [("x", C.c_void_p * 3), ("r", C.c_void_p * 3), ("z", C.c_void_p * 3), ("add", C.c_void_p * 3),
                ("out", C.c_void_p * 3), ("r1", C.c_void_p), ("u1", C.c_void_p), ("u2", C.c_void_p), ("w_up", C.c_void_p),
                ("b_up", C.c_void_p), ("w_dn", C.c_void_p), ("b_dn", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32)]


class DivEnhStageArgs(C.Structure):
    """fcvsr_divenh_stage_args: one stage of the DivEnh chain (bands j0..i replayed in registers, see include/fcvsr_hip.h)."""
    _fields_ = [("ck_s_f", C.c_void_p), ("ck_s_o", C.c_void_p), ("f", C.c_void_p * 4), ("a", C.c_void_p * 4),
                ("b", C.c_void_p * 4), ("g1", C.c_void_p * 4), ("g2", C.c_void_p * 4), ("mean_f_sum", C.c_void_p),
                ("f_next", C.c_void_p), ("a_next", C.c_void_p), ("b_next", C.c_void_p), ("out_s_f", C.c_void_p),
                ("out_s_o", C.c_void_p), ("sums", C.c_void_p), ("scratch", C.c_void_p), ("scratch_elems", C.c_int64),
                ("inv_hw", C.c_float), ("n_bands", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("C", C.c_int32)]


class CropDesc(C.Structure):
    """fcvsr_crop_desc: one output plane of fcvsr_clip_batch_u8 / _u16 (``numpy.dtype(CropDesc)`` is its array form)."""
    _fields_ = [("src", C.c_void_p), ("pitch", C.c_int32), ("top", C.c_int32), ("left", C.c_int32), ("flags", C.c_int32)]


CROP_HFLIP, CROP_VFLIP, CROP_TRANSPOSE = 1, 2, 4


class Colour(C.Structure):
    """fcvsr_colour: the fixed-point constants of one YUV 4:2:0 <-> RGB conversion (`harness.colour.coefficients` makes them)."""
    _fields_ = [(n, C.c_int32) for n in ("shift", "chroma_loc", "y_off", "c_off", "cy", "rv", "gu", "gv", "bu", "kr", "kg", "kb",
                                         "ur", "ug", "ub", "vr", "vg", "vb")]


CHROMA_LEFT, CHROMA_CENTER = 0, 1


class ConvDesc(C.Structure):
    _fields_ = [("n_src", C.c_int32), ("src", View * 3), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("cout", C.c_int32), ("weight", C.c_void_p), ("cout_pad", C.c_int32), ("bias", C.c_void_p),
                ("act", C.c_int32), ("slope", C.c_float), ("slope_ptr", C.c_void_p), ("n_res", C.c_int32),
                ("res", View * 2), ("res_scale", C.c_float * 2), ("dst", View), ("pixel_shuffle", C.c_int32),
                ("gc_wmask", C.c_void_p), ("gc_partial", C.c_void_p)]


# bench.py instrumentation: when PROFILE is a list, every conv launch is bracketed by HIP events on the launch stream and
# (start, stop, algorithmic_flops) is appended.  None (default) = no instrumentation.
PROFILE = None
COMPUTE_DTYPE = "f32"
DOMINANT_KERNEL = "conv_direct_kernel"


class HipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None

# name -> argtypes (restype is always int unless listed in _RESTYPES)
_VP, _I, _I64, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_PV = C.POINTER(View)
SIGNATURES = {
    "fcvsr_last_error": [],
    "fcvsr_last_conv_kernel": [],
    "fcvsr_conv2d_wgrad_scratch_elems": [C.c_int] * 7,
    "fcvsr_conv2d_wgrad": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                           C.c_longlong, C.c_int, C.c_void_p],
    "fcvsr_conv2d_wgrad_mfma_eligible": [C.c_int] * 6,
    "fcvsr_conv2d_wgrad_mfma_scratch_elems": [C.c_int] * 7,
    "fcvsr_conv2d_wgrad_mfma": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p],
    "fcvsr_abi_version": [],
    "fcvsr_device_count": [],
    "fcvsr_conv2d": [C.POINTER(ConvDesc), _VP],
    "fcvsr_conv2d_f32mfma": [C.POINTER(ConvDesc), _VP],
    "fcvsr_conv2d_f32mfma_eligible": [C.POINTER(ConvDesc)],
    "fcvsr_conv2d_mfma": [C.POINTER(ConvDesc), _I, _I, _VP],
    "fcvsr_conv2d_mfma_plan": [C.POINTER(ConvDesc), _I, _I, _I, _I, C.c_char_p, _I],
    "fcvsr_rfft2": [_PV, _I, _I, _I, _I, _VP, _I64, _I, _I, _VP],
    "fcvsr_irfft2": [_VP, _I64, _I, _I, _I, _I, _I, _I, _VP, _VP, _PV, _VP],
    "fcvsr_irfft2_bands": [_VP, _I64, _I, _I, _I, _I, _I, _I, _VP, _I, _VP, _PV, _VP],
    "fcvsr_last_fft_path": [],
    "fcvsr_ffl_workspace_elems": [_I, _I, _I],
    "fcvsr_ffl_diff": [_VP, _VP, _I, _I, _I, _I, _I, _VP, _I, _VP],
    "fcvsr_ffl_weight": [_VP, _I64, _I, _I, _I, _I, _I, _F, _F, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_ffl_grad": [_VP, _I, _VP, _F, _I, _I, _I, _I, _I, _VP, _VP, _VP],
    "fcvsr_corr_lookup": [_VP, _VP, _I64, _I, _I, _I, _I, _I, _I, _PV, _VP],
    "fcvsr_channel_sum": [_PV, _I, _I, _I, _VP, _VP, _I64, _VP],
    "fcvsr_ca_gate": [_VP, _F, _VP, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_convblk_tail": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I64, _I, _I, _I, _I, _VP],
    "fcvsr_convblk": [_VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _I64, _VP, _I64, _I, _I, _I, _I, _VP],
    "fcvsr_convblk_heads": [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _I64, _VP, _I64, _I, _I, _VP],
    "fcvsr_warp": [_PV, _PV, _I, _I, _I, _PV, _VP],
    "fcvsr_sac_v": [_PV, _PV, _I, _I, _I, _PV, _VP],
    "fcvsr_sac_h": [_PV, _PV, _PV, _F, _I, _I, _I, _PV, _VP],
    "fcvsr_iac_step": [_PV, _PV, _PV, _PV, _F, _I, _I, _I, _PV, _VP],
    "fcvsr_feat_extract": [_PV, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP],
    "fcvsr_freq_head": [_VP, _I, _I64, _I64, _VP, _VP, _VP, _VP, _VP],
    "fcvsr_convcorr_strip": [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP],
    "fcvsr_freq_mlp3": [_VP, _VP, _I, _I64, _I64, _VP, _VP, _VP, _VP, _I64, _VP],
    "fcvsr_iac_step2": [_PV, _PV, _PV, _PV, _F, _I, _I, _I, _PV, _VP],
    "fcvsr_iac_step2_fused": [_PV, _PV, _PV, _VP, _VP, _PV, _F, _I, _I, _I, _PV, _VP],
    "fcvsr_divenh": [_I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, _VP, _VP, _VP, _I64, _I, _I, _I, _I, _VP],
    "fcvsr_divenh_apply_next": [_I, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I, _I, _I, _I, _VP],
    "fcvsr_divenh_stage": [C.POINTER(DivEnhStageArgs), _VP],
    "fcvsr_scale_add": [_VP, _VP, _VP, _I, _VP, _I, _I, _I, _I, _I, _VP],
    "fcvsr_gc_context": [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _I64, _VP],
    "fcvsr_gc_finish": [_VP, _I, _VP, _VP, _I, _I, _VP, _VP],
    "fcvsr_gc_apply": [_VP, _VP, _VP, _VP, _I, _F, _I, _I, _I, _I, _VP],
    "fcvsr_xscale": [_VP, _VP, _F, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP],
    "fcvsr_gc_finish_levels": [C.POINTER(GcFinishLevel), _I, _VP, _VP, _I, _I, _VP],
    "fcvsr_gc_partial_levels": [C.POINTER(GcPartialLevel), _I, _I, _VP, _I, _VP],
    "fcvsr_gc_apply_levels": [C.POINTER(GcApplyLevel), _I, _I, _I, _F, _I, _VP],
    "fcvsr_xscale_levels": [C.POINTER(XscaleLevel), _I, _I, _I, _VP],
    "fcvsr_rcb_level0": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _F, _I, _I, _I, _I, _I, _VP],
    "fcvsr_rcb_tail": [C.POINTER(RcbTailArgs), _F, _I, _I, _VP],
    "fcvsr_pixel_shuffle": [_VP, _VP, _I, _I, _I, _I, _VP],
    "fcvsr_pixel_shuffle16": [_VP, _PV, _I, _I, _I, _I, _VP],
    "fcvsr_bilinear_up4": [_PV, _I, _I, _I, _PV, _VP],
    "fcvsr_tail_fused": [_PV, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _PV, _VP],
    "fcvsr_tail_fused_base": [_PV, _VP, _VP, _VP, _VP, _VP, _PV, _I, _I, _I, _PV, _VP],
    "fcvsr_conv_last": [_PV, _VP, _VP, _I, _I, _I, _I, _PV, _VP],
    "fcvsr_pack_weight_mfma": [_VP, _I, _I, _I, _I, _VP, _I, _I, _I, _I, _VP],
    "fcvsr_pack_weights_multi_block_elems": [],
    "fcvsr_pack_weights_mfma_multi": [_VP, _I, _I, _I, _VP],
    "fcvsr_adam_multi_block_elems": [],
    "fcvsr_adam_multi": [_VP, _I, _I, _VP, _VP, _VP, _I, _F, _F, _F, _F, _F, _F, _F, _VP],
    "fcvsr_act_bwd": [_VP, _VP, _VP, _F, C.c_longlong, _VP],
    "fcvsr_colsum_scratch_elems": [C.c_longlong, _I],
    "fcvsr_colsum": [_VP, C.c_longlong, _I, _VP, _VP, C.c_longlong, _I, _VP],
    "fcvsr_iac_bwd_sac": [_VP, _VP, _VP, _VP, _PV, _F, _I, _I, _I, _I, _VP, _I, _VP, _PV, _I, _VP],
    "fcvsr_iac_bwd_warp": [_VP, _PV, _VP, _PV, _I, _I, _I, _I, _VP, _VP, _VP],
    "fcvsr_iac_bwd_warp_det_workspace": [_I, _I, _I, _I, C.POINTER(C.c_size_t)],
    "fcvsr_iac_bwd_warp_det": [_VP, _PV, _VP, _PV, _I, _I, _I, _I, _VP, _VP, _VP, C.c_size_t, _VP],
    "fcvsr_prelu_fwd": [_VP, _VP, _VP, C.c_longlong, _VP],
    "fcvsr_prelu_bwd": [_VP, _VP, _VP, _VP, _VP, _VP, C.c_longlong, _VP],
    "fcvsr_wgrad_cout1_scratch_elems": [_I, _I, _I],
    "fcvsr_wgrad_cout1": [_VP, _VP, _I, _I, _I, _I, _VP, _VP, C.c_longlong, _I, _VP],
    "fcvsr_conv2d_wgrad_mfma_groups_scratch_elems": [_VP, _VP, _VP, _I, _I, _I, _I, _I],
    "fcvsr_conv2d_wgrad_mfma_groups": [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, C.c_longlong, _I, _I, _VP],
    "fcvsr_up2_adjoint": [_VP, _VP, _I, _I, _I, _I, _VP],
    "fcvsr_pool2_adjoint": [_VP, _VP, _I, _I, _I, _I, _VP],
    "fcvsr_rcbt_nblk": [_I],
    "fcvsr_rcbt_stat_elems": [],
    "fcvsr_rcbt_forward": [_VP, _VP, _VP, _VP, _VP, _F, _I, _I, _I, _VP, _VP, _VP, C.c_longlong, _VP],
    "fcvsr_rcbt_backward": [_VP, _VP, _VP, _VP, _VP, _VP, _F, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, C.c_longlong, _I, _VP],
    "fcvsr_divenh_band_nblk": [_I],
    "fcvsr_divenh_band_stat_elems": [_I],
    "fcvsr_divenh_band_forward": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, C.c_longlong, _VP],
    "fcvsr_divenh_band_backward": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                   C.c_longlong, _I, _VP],
    "fcvsr_corr_lookup_bwd": [_VP, _VP, _I64, _I, _I, _I, _I, _I, _I, _PV, _VP, _VP, _VP],
    "fcvsr_frame_metrics_scratch_bytes": [_I] * 6,
    "fcvsr_frame_metrics": [_VP, C.POINTER(C.c_int64), _I, _VP, C.POINTER(C.c_int64), _I, _I, _I, _I, _I, _I,
                            C.POINTER(C.c_double), _VP, _VP, C.c_longlong, _VP],
    "fcvsr_feat_extract_u8": [_PV, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP],
    "fcvsr_bilinear_up4_u8": [_PV, _VP, _I, _I, _I, _PV, _VP],
    "fcvsr_tail_fused_u8": [_PV, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _PV, _PV, _I, _VP],
    "fcvsr_tail_fused_base_u8": [_PV, _VP, _VP, _VP, _VP, _VP, _PV, _VP, _I, _I, _I, _PV, _I, _VP],
    "fcvsr_conv_last_u8": [_PV, _VP, _VP, _I, _I, _I, _I, _PV, _PV, _I, _VP],
    "fcvsr_u8_to_f32": [_VP, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_quantise_u8": [_VP, C.c_longlong, _I, _VP, _VP],
    "fcvsr_chroma_up4": [_VP, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_clip_batch_u8": [_VP, _VP, _I, _I, _VP, _VP],
    "fcvsr_clip_batch_u16": [_VP, _VP, _I, _I, _VP, _VP],
    "fcvsr_frame_metrics_u16": [_VP, C.POINTER(C.c_int64), _I, _VP, C.POINTER(C.c_int64), _I, _I, _I, _I, _I, _I,
                                C.POINTER(C.c_double), C.c_double, _VP, _VP, C.c_longlong, _VP],
    "fcvsr_feat_extract_u16": [_PV, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP],
    "fcvsr_bilinear_up4_u16": [_PV, _VP, _I, _I, _I, _PV, _VP],
    "fcvsr_tail_fused_u16": [_PV, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _PV, _PV, _I, _VP],
    "fcvsr_tail_fused_base_u16": [_PV, _VP, _VP, _VP, _VP, _VP, _PV, _VP, _I, _I, _I, _PV, _I, _VP],
    "fcvsr_conv_last_u16": [_PV, _VP, _VP, _I, _I, _I, _I, _PV, _PV, _I, _VP],
    "fcvsr_u16_to_f32": [_VP, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_quantise_u16": [_VP, C.c_longlong, _I, _VP, _VP],
    "fcvsr_chroma_up4_u16": [_VP, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_yuv420_to_rgb": [_VP, _VP, _VP, _I, _I, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(Colour), _VP, _VP],
    "fcvsr_yuv420_to_rgb_u16": [_VP, _VP, _VP, _I, _I, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(Colour), _VP, _VP],
    "fcvsr_rgb_to_yuv420": [_VP, _I, _I, _I, C.POINTER(Colour), C.c_longlong, C.c_longlong, C.c_longlong, _VP, _VP, _VP, _VP],
    "fcvsr_rgb_to_yuv420_u16": [_VP, _I, _I, _I, C.POINTER(Colour), C.c_longlong, C.c_longlong, C.c_longlong, _VP, _VP, _VP, _VP],
    "fcvsr_ensemble_windows": [_VP, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _VP, _VP],
    "fcvsr_ensemble_windows_u8": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _VP, _VP],
    "fcvsr_ensemble_windows_u16": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _VP, _VP],
    "fcvsr_ensemble_merge": [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP],
    "fcvsr_tile_windows": [_VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_tile_windows_u8": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_tile_windows_u16": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_tile_merge": [_VP, _VP, _I, _VP, _I, _I, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP],
    "fcvsr_tile_pairs_equal": [_VP, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _I, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_tile_pairs_equal_u8": [_VP, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _I, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_tile_pairs_equal_u16": [_VP, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, _I, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_tile_windows_sel": [_VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _I, _VP, _VP],
    "fcvsr_tile_windows_sel_u8": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _I, _VP, _VP],
    "fcvsr_tile_windows_sel_u16": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _I, _VP, _I, _I, _I, _VP, _I, _VP, _VP],
    "fcvsr_tile_merge_sel": [_VP, _I, _VP, _VP, _I, _VP, _I, _I, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP],
    "fcvsr_niqe_scratch_bytes": [_I] * 4,
    "fcvsr_niqe_features": [_VP, C.POINTER(C.c_int64), _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _VP, _VP, _VP, C.c_longlong,
                            _VP],
    "fcvsr_brisque_scratch_bytes": [_I] * 3,
    "fcvsr_brisque_features": [_VP, C.POINTER(C.c_int64), _I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _VP, _VP, C.c_longlong, _VP,
                               _VP],
    "fcvsr_bicubic_downscale": [_VP, _I, C.c_longlong, _I, _I, _I, _VP, _VP],
    "fcvsr_bicubic_upscale": [_VP, _I, C.c_longlong, _I, _I, _I, _VP, _I, _VP],
    "fcvsr_imresize": [_VP, _I, C.c_longlong, _I, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _I, _I, _VP, _I, _VP],
    "fcvsr_frame_pair_sad": [_VP, _I, _I, C.c_longlong, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_frame_line_sums": [_VP, _I, _I, _I, _I, _I, _VP, C.c_longlong, _VP, _VP, _VP],
    "fcvsr_active_compose": [_VP] + [C.c_longlong] * 4 + [_VP, _VP] + [C.c_longlong] * 3 + [_I] * 9 + [_VP, _VP],
    "fcvsr_surface_unpack": [_VP, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _VP, _VP, _VP],
    "fcvsr_surface_pack": [_VP, _VP, _VP, C.c_longlong, C.c_longlong, C.c_longlong, _I, _I, _I, _I, _VP, _VP],
    "fcvsr_plane_sse": [_VP, _VP, _I, _I, _I, _I, C.c_longlong, C.c_longlong, _I, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_farneback_scratch_bytes": [_I] * 3,
    "fcvsr_farneback_flow": [_VP, _VP, _I, _I, _I, _I, C.c_longlong, C.c_longlong, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_flow_epe_scratch_bytes": [_I] * 3,
    "fcvsr_flow_epe": [_VP, _VP, _I, _I, _I, _VP, C.c_longlong, _VP, _VP],
    "fcvsr_flow_level_image": [_VP, _I, _I, _I, _I, C.c_longlong, _I, _VP, _VP],
    "fcvsr_flow_poly_exp": [_VP, _I, _I, _I, _VP, _VP],
    "fcvsr_flow_matrices": [_VP, _VP, _VP, _I, _I, _I, _VP, _VP],
    "fcvsr_flow_box_solve": [_VP, _I, _I, _I, _VP, _VP],
}
_RESTYPES = {"fcvsr_last_error": C.c_char_p, "fcvsr_last_conv_kernel": C.c_char_p, "fcvsr_last_fft_path": C.c_char_p,
             "fcvsr_conv2d_wgrad_scratch_elems": C.c_longlong,
             "fcvsr_conv2d_wgrad_mfma_scratch_elems": C.c_longlong, "fcvsr_colsum_scratch_elems": C.c_longlong,
             "fcvsr_wgrad_cout1_scratch_elems": C.c_longlong, "fcvsr_conv2d_wgrad_mfma_groups_scratch_elems": C.c_longlong,
             "fcvsr_frame_metrics_scratch_bytes": C.c_longlong, "fcvsr_niqe_scratch_bytes": C.c_longlong,
             "fcvsr_brisque_scratch_bytes": C.c_longlong, "fcvsr_ffl_workspace_elems": C.c_longlong,
             "fcvsr_farneback_scratch_bytes": C.c_longlong, "fcvsr_flow_epe_scratch_bytes": C.c_longlong}


def lib() -> C.CDLL:
    """Load the shared library (built by ``fcvsr_amd.build``).  Raises if it is absent: there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} not found: run `python -m fcvsr_amd.build` (hipcc, gfx950). "
                           "fcvsr_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(l, name, None)
            if fn is None:                      # a library older than this binding: the call site raises AttributeError when reached
                continue                        # (tests/test_host_logic.py checks that the built library exports every declared symbol)
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, C.c_int)
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().fcvsr_last_error()
        raise HipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def view(t: torch.Tensor) -> View:
    """View of a 4-D tensor whose logical dims are (b, y, x, c) with arbitrary strides (zero-copy)."""
    assert t.dim() == 4, t.shape
    sb, sy, sx, sc = t.stride()
    if t.shape[3] == 1:
        sc = 1                                   # the stride of a size-1 dimension is arbitrary in torch (channels_last with C = 1)
    return View(t.data_ptr(), sb, sy, sx, sc, t.shape[3], _DT[t.dtype])


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, kh, kw) -> [kh*kw][Cin][cout_pad] f32, cout padded to a multiple of 16 (zero rows)."""
    cout, cin, kh, kw = w.shape
    cp = (cout + 15) // 16 * 16
    out = torch.zeros(kh * kw, cin, cp, dtype=torch.float32, device=w.device)
    out[:, :, :cout] = w.detach().float().permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    return out.contiguous()


def pack_conv_weight_f32mfma(w: torch.Tensor, ps: bool = False) -> torch.Tensor:
    """(Cout, Cin, kh, kw) -> f32 [kh*kw][ceil64(Cout)][Cin] (layout of fcvsr_conv2d_f32mfma), zero rows past Cout; with
    ps=True the rows are in the sub-pixel-major order of the pixel-shuffle epilogue (`ps_order`)."""
    if ps:
        w = w[ps_order(w.shape[0]).to(w.device)]
    cout, cin, kh, kw = w.shape
    cop = (cout + 63) // 64 * 64
    out = torch.zeros(kh * kw, cop, cin, dtype=torch.float32, device=w.device)
    out[:, :cout] = w.detach().float().permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    return out.contiguous()


def ps_order(cout: int) -> torch.Tensor:
    """Row permutation for pixel-shuffled MFMA layers: new row (2i+j)*(cout/4)+c <- original channel 4c+2i+j."""
    q = cout // 4
    return torch.tensor([4 * c + sp for sp in range(4) for c in range(q)], dtype=torch.long)


def pack_conv_weight_mfma(w: torch.Tensor, dtype: torch.dtype, ps: bool = False) -> torch.Tensor:
    """(Cout, Cin, kh, kw) -> 16-bit [kh*kw][ceil128(Cout)][ceil64(Cin)], zero padded (layout of fcvsr_conv2d_mfma)."""
    if ps:
        w = w[ps_order(w.shape[0]).to(w.device)]
    cout, cin, kh, kw = w.shape
    cop, cip = (cout + 127) // 128 * 128, (cin + 63) // 64 * 64
    out = torch.zeros(kh * kw, cop, cip, dtype=dtype, device=w.device)
    out[:, :cout, :cin] = w.detach().float().permute(2, 3, 0, 1).reshape(kh * kw, cout, cin).to(dtype)
    return out.contiguous()


def _fill_desc(d: "ConvDesc", srcs, wpacked, ksize, cout, cout_pad, dst, bias, stride, act, slope, slope_t, res,
               res_scale, pixel_shuffle) -> int:
    d.n_src = len(srcs)
    for i, s in enumerate(srcs):
        d.src[i] = view(s)
    d.B, d.H, d.W = srcs[0].shape[0], srcs[0].shape[1], srcs[0].shape[2]
    d.kh = d.kw = ksize
    d.stride = stride
    d.pad = ksize // 2
    d.cout = cout
    d.weight = wpacked.data_ptr()
    d.cout_pad = cout_pad
    d.bias = ptr(bias)
    d.act = act
    d.slope = slope
    d.slope_ptr = ptr(slope_t)
    d.n_res = len(res)
    for i, r in enumerate(res):
        d.res[i] = view(r)
        d.res_scale[i] = res_scale[i] if i < len(res_scale) else 1.0
    d.dst = view(dst)
    d.pixel_shuffle = int(pixel_shuffle)
    return sum(s.shape[3] for s in srcs)


def mfma_eligible(ksize: int, stride: int, groups) -> bool:
    """Can fcvsr_conv2d_mfma take this problem? (1x1/3x3, stride 1, channel-contiguous 16-byte-aligned f32 inputs)"""
    if ksize not in (1, 3) or stride not in (1, 2) or (stride == 2 and ksize != 3):
        return False
    for g in groups:
        if len(g["srcs"]) == 1 and g["srcs"][0].stride(3) != 1:       # planar (NCHW) source, e.g. feat_extract
            s0 = g["srcs"][0]
            if s0.dtype != torch.float32 or s0.shape[3] > 32 or ksize != 3 or stride != 1:
                return False
            continue
        for s in g["srcs"]:
            sb, sy, sx, sc = s.stride()
            gran = 4 if s.dtype == torch.float32 else 8
            if sc != 1 or s.shape[3] % gran or sx % gran or sy % gran or sb % gran or s.data_ptr() % 16:
                return False
            if ksize == 1 and (sy != sx * s.shape[2] or (s.shape[0] > 1 and sb != sy * s.shape[1])):
                return False
        for t in list(g.get("res", ())) + ([] if g.get("ps") else [g["dst"]]):
            sb, sy, sx, sc = t.stride()
            if ksize == 1 and (sy != sx * t.shape[2] or (t.shape[0] > 1 and sb != sy * t.shape[1])):
                return False
    return True


def _mfma_descs(groups, wpacked, ksize, cout, stride, bias, act, slope, slope_t, res_scale, pixel_shuffle, gc_wmask):
    """The descriptors of a grouped MFMA problem (conv2d_mfma and conv_plan fill them alike) and its algorithmic FLOPs."""
    descs = (ConvDesc * len(groups))()
    flops = 0.0
    for i, g in enumerate(groups):
        cin = _fill_desc(descs[i], g["srcs"], wpacked, ksize, cout, wpacked.shape[1], g["dst"], bias, stride, act, slope,
                         slope_t, g.get("res", ()), res_scale, pixel_shuffle)
        assert wpacked.shape[0] == ksize * ksize and wpacked.shape[2] >= cin, (wpacked.shape, ksize, cin)
        if gc_wmask is not None:
            descs[i].gc_wmask = gc_wmask.data_ptr()
            descs[i].gc_partial = g["gc_partial"].data_ptr()
        flops += 2.0 * descs[i].B * descs[i].H * descs[i].W * cout * cin * ksize * ksize / (stride * stride)
    return descs, flops


def conv_plan(groups, wpacked: torch.Tensor, ksize: int, cout: int, mma_dtype: int, *, lean: int = 1, res: int = 2, stride: int = 1,
              bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, slope: float = 0.0,
              slope_t: Optional[torch.Tensor] = None, res_scale: Sequence[float] = (), pixel_shuffle: bool = False,
              gc_wmask: Optional[torch.Tensor] = None, name: str = "") -> str:
    """The kernel conv2d_mfma would launch for this problem (the string fcvsr_last_conv_kernel() reports afterwards) under the
    policy lean (0 | 1, as FCVSR_MFMA_LEAN) and res (0 | 1, or 2 = unset, as FCVSR_MFMA_RES); HipError where it would be rejected.
    Nothing is launched and the environment is not read; the tensors are looked at for shape, strides and alignment only.  Takes
    conv2d_mfma's keywords (`name` is unused), so one argument set serves both."""
    descs, _ = _mfma_descs(groups, wpacked, ksize, cout, stride, bias, act, slope, slope_t, res_scale, pixel_shuffle, gc_wmask)
    name = C.create_string_buffer(96)
    check(lib().fcvsr_conv2d_mfma_plan(descs, len(groups), mma_dtype, lean, res, name, len(name)), "fcvsr_conv2d_mfma_plan")
    return name.value.decode()


def conv2d_mfma(groups, wpacked: torch.Tensor, ksize: int, cout: int, mma_dtype: int, *, stride: int = 1,
                bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, slope: float = 0.0,
                slope_t: Optional[torch.Tensor] = None, res_scale: Sequence[float] = (), pixel_shuffle: bool = False,
                gc_wmask: Optional[torch.Tensor] = None, name: str = ""):
    """groups: 1..3 dicts {srcs: [..], dst: t, res: [..]} sharing weights / epilogue (one launch)."""
    n = len(groups)
    descs, flops = _mfma_descs(groups, wpacked, ksize, cout, stride, bias, act, slope, slope_t, res_scale, pixel_shuffle, gc_wmask)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().fcvsr_conv2d_mfma(descs, n, mma_dtype, stream_ptr()), "fcvsr_conv2d_mfma")
        e1.record()
        nbytes = sum(t.numel() * t.element_size() for g in groups for t in list(g["srcs"]) + list(g.get("res", ())) + [g["dst"]])
        # the kernel the dispatcher actually launched (fcvsr_last_conv_kernel): bench.py groups the timings by it
        kname = lib().fcvsr_last_conv_kernel().decode()
        PROFILE.append((e0, e1, flops, "mfma", name, nbytes, kname))
        return
    check(lib().fcvsr_conv2d_mfma(descs, n, mma_dtype, stream_ptr()), "fcvsr_conv2d_mfma")


def conv2d(srcs: Sequence[torch.Tensor], wpacked: torch.Tensor, ksize: int, cout: int, dst: torch.Tensor, *,
           bias: Optional[torch.Tensor] = None, stride: int = 1, act: int = ACT_NONE, slope: float = 0.0,
           slope_t: Optional[torch.Tensor] = None, res: Sequence[torch.Tensor] = (),
           res_scale: Sequence[float] = (), pixel_shuffle: bool = False, name: str = "",
           w_f32mfma: Optional[torch.Tensor] = None, bias_f32mfma: Optional[torch.Tensor] = None) -> torch.Tensor:
    """srcs / res / dst are (b,y,x,c)-ordered tensors (any strides).  Exact f32: the direct VALU kernel, or - when
    `w_f32mfma` (pack_conv_weight_f32mfma) is given and the layer qualifies - the f32-operand matrix-core kernel."""
    if w_f32mfma is not None and len(srcs) == 1 and stride == 1 and PROFILE is None:
        dm = ConvDesc()              # (pixel-shuffled layers: w_f32mfma / bias_f32mfma are in sub-pixel-major row order)
        _fill_desc(dm, srcs, w_f32mfma, ksize, cout, w_f32mfma.shape[1], dst, bias_f32mfma if pixel_shuffle else bias, stride, act,
                   slope, slope_t, res, res_scale, pixel_shuffle)
        if lib().fcvsr_conv2d_f32mfma_eligible(C.byref(dm)):
            check(lib().fcvsr_conv2d_f32mfma(C.byref(dm), stream_ptr()), "fcvsr_conv2d_f32mfma")
            return dst
    d = ConvDesc()
    cin = _fill_desc(d, srcs, wpacked, ksize, cout, wpacked.shape[-1], dst, bias, stride, act, slope, slope_t, res,
                     res_scale, pixel_shuffle)
    assert wpacked.shape[0] == ksize * ksize and wpacked.shape[1] == cin, (wpacked.shape, ksize, cin)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().fcvsr_conv2d(C.byref(d), stream_ptr()), "fcvsr_conv2d")
        e1.record()
        ho = (d.H + 2 * d.pad - d.kh) // stride + 1
        wo = (d.W + 2 * d.pad - d.kw) // stride + 1
        PROFILE.append((e0, e1, 2.0 * d.B * ho * wo * cout * cin * ksize * ksize, "direct", name, 0, "direct"))
        return dst
    check(lib().fcvsr_conv2d(C.byref(d), stream_ptr()), "fcvsr_conv2d")
    return dst


QUANT_NONE, QUANT_TRUNCATE, QUANT_ROUND = 0, 1, 2
PEAK10 = 1023                      # full scale of a 10-bit sample: the divisor of the uint16 path (2^10 - 1, not HM's 1020)


def frame_metric_sums(sr: torch.Tensor, hr: torch.Tensor, quantise: int, crop_border: int, to_y: bool,
                      window: Sequence[float], peak: Optional[float] = None) -> torch.Tensor:
    """fcvsr_frame_metrics: sr (N,C,H,W) uint8 (QUANT_NONE) or f32 (any strides), hr uint8 (N,C,H,W) on the same device.
    uint16 hr (10-bit frames) goes to fcvsr_frame_metrics_u16: sr is then uint16 or f32, and `peak` (default 1023) sets the SSIM
    constants.  Returns f64 (N, 2) on the device: per frame the squared-error sum over the PSNR region and the SSIM-map sum, both
    over all scored planes.  Arguments are checked by the library (FCVSR_E_ARG -> HipError)."""
    N, Cc, H, W = sr.shape
    to_y = int(bool(to_y))
    nbytes = lib().fcvsr_frame_metrics_scratch_bytes(N, Cc, H, W, crop_border, to_y)
    scratch = torch.empty((max(1, nbytes) + 7) // 8, dtype=torch.float64, device=sr.device)
    out = torch.empty((N, 2), dtype=torch.float64, device=sr.device)
    s_st, h_st = (C.c_int64 * 4)(*sr.stride()), (C.c_int64 * 4)(*hr.stride())
    win = (C.c_double * 11)(*[float(v) for v in window])
    fmt = hr.dtype if hr.dtype in _INT_FORMATS else torch.uint8        # an hr of any other dtype: the uint8 form's check refuses it
    fn, name, _ = _entry("frame_metrics", fmt)
    pk = (float(PEAK10 if peak is None else peak),) if fmt == torch.uint16 else ()      # the SSIM peak: the uint8 form fixes it at 255
    check(fn(sr.data_ptr(), s_st, quantise, hr.data_ptr(), h_st, N, Cc, H, W, crop_border, to_y, win, *pk, out.data_ptr(),
             scratch.data_ptr(), scratch.numel() * 8, stream_ptr()), name)
    return out


def _score_args(frames: torch.Tensor, nbytes: int, taps, tables: torch.Tensor, tables_of: str):
    """What fcvsr_niqe_features and fcvsr_brisque_features take alike: the f64 scratch tensor, the frames' strides and the 49
    correlation taps as C arrays; `tables` is checked against the (4, 9801) f64 layout of `tables_of`."""
    scratch = torch.empty((max(8, nbytes) + 7) // 8, dtype=torch.float64, device=frames.device)
    strides = (C.c_int64 * 4)(*frames.stride())
    win = (C.c_double * 49)(*[float(v) for v in np.asarray(taps, dtype=np.float64).reshape(-1)])
    if tables.dtype != torch.float64 or tuple(tables.shape) != (4, 9801) or not tables.is_contiguous() or tables.device != frames.device:
        raise ValueError(f"tables must be the contiguous (4, 9801) f64 tensor of {tables_of} on the frames' device")
    return scratch, strides, win


def niqe_features(frames: torch.Tensor, quantise: int, crop_border: int, to_y: bool, taps, tables: torch.Tensor) -> torch.Tensor:
    """fcvsr_niqe_features: frames (N,C,H,W) uint8 (QUANT_NONE) or f32 (any strides) on the HIP device; `taps` the 7 x 7 MSCN window
    as correlation taps (the model's window flipped in both axes); `tables` the device (4, 9801) f64 tensor of
    `harness.niqe.aggd_tables`.  Returns the (N, blocks, 36) f64 block features on the device, with no host sync.  Arguments are
    checked by the library (FCVSR_E_ARG -> HipError)."""
    N, Cc, H, W = frames.shape
    blocks = (max(H - 2 * crop_border, 0) // 96) * (max(W - 2 * crop_border, 0) // 96)
    scratch, strides, win = _score_args(frames, lib().fcvsr_niqe_scratch_bytes(N, H, W, crop_border), taps, tables,
                                        "harness.niqe.aggd_tables")
    out = torch.empty((N, blocks, 36), dtype=torch.float64, device=frames.device)
    check(lib().fcvsr_niqe_features(frames.data_ptr(), strides, quantise, N, Cc, H, W, crop_border, int(bool(to_y)), win,
                                    tables.data_ptr(), out.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, stream_ptr()),
          "fcvsr_niqe_features")
    return out


def brisque_features(frames: torch.Tensor, quantise: int, to_y: bool, taps, tables: torch.Tensor) -> torch.Tensor:
    """fcvsr_brisque_features: frames (N,C,H,W) uint8 (QUANT_NONE) or f32 (any strides) on the HIP device; `taps` the 7 x 7 MSCN
    window as correlation taps; `tables` the device (4, 9801) f64 tensor of `harness.brisque.brisque_tables`.  Returns the (N, 36)
    f64 features on the device, with no host sync.  Arguments are checked by the library (FCVSR_E_ARG -> HipError)."""
    N, Cc, H, W = frames.shape
    scratch, strides, win = _score_args(frames, lib().fcvsr_brisque_scratch_bytes(N, H, W), taps, tables,
                                        "harness.brisque.brisque_tables")
    out = torch.empty((N, 36), dtype=torch.float64, device=frames.device)
    check(lib().fcvsr_brisque_features(frames.data_ptr(), strides, quantise, N, Cc, H, W, int(bool(to_y)), win, tables.data_ptr(),
                                       scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), stream_ptr()),
          "fcvsr_brisque_features")
    return out


def bicubic_downscale(x: torch.Tensor, factor: int) -> torch.Tensor:
    """fcvsr_bicubic_downscale: x (..., H, W) uint8 or f32 on the HIP device, H and W multiples of factor (2 or 4) -> f32
    (..., H/factor, W/factor), the MATLAB-style antialiased bicubic down-scale (`harness.niqe.bicubic_downscale` is the contract),
    one launch."""
    if not x.is_cuda:
        raise RuntimeError("bicubic_downscale runs on the HIP device only (there is no CPU fallback)")
    if x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"x must be uint8 or f32, got {x.dtype}")
    if factor not in (2, 4):
        raise ValueError(f"factor must be 2 or 4, got {factor!r}")
    if x.dim() < 2 or x.shape[-2] % factor or x.shape[-1] % factor or 0 in x.shape[-2:]:
        raise ValueError(f"the last two dimensions must be non-empty multiples of {factor}, got {tuple(x.shape)}")
    x = x.contiguous()
    H, W = x.shape[-2:]
    out = torch.empty((*x.shape[:-2], H // factor, W // factor), dtype=torch.float32, device=x.device)
    planes = out.numel() // ((H // factor) * (W // factor))
    if planes:
        with torch.cuda.device(x.device):
            check(lib().fcvsr_bicubic_downscale(x.data_ptr(), _DT[x.dtype], planes, H, W, factor, out.data_ptr(), stream_ptr()),
                  "fcvsr_bicubic_downscale")
    return out


def bicubic_upscale(x: torch.Tensor, factor: int, out: str = "f32") -> torch.Tensor:
    """fcvsr_bicubic_upscale: x (..., H, W) uint8, uint16 (10-bit samples) or f32 on the HIP device, any H, W >= 1 ->
    (..., factor H, factor W), the MATLAB-style bicubic up-scale at factor 2 or 4 (`harness.niqe.bicubic_upscale` is the contract),
    one launch.  out="f32": the f32 sums on x's scale; out="int" (integer x only): clipped to [0, peak], rounded half to even, in
    x's dtype.  Non-contiguous x is made dense first."""
    if not x.is_cuda:
        raise RuntimeError("bicubic_upscale runs on the HIP device only (there is no CPU fallback)")
    if x.dtype not in (torch.uint8, torch.uint16, torch.float32):
        raise ValueError(f"x must be uint8, uint16 or f32, got {x.dtype}")
    if factor not in (2, 4):
        raise ValueError(f"factor must be 2 or 4, got {factor!r}")
    if out not in ("f32", "int"):
        raise ValueError(f'out must be "f32" or "int", got {out!r}')
    if out == "int" and x.dtype == torch.float32:
        raise ValueError('out="int" needs uint8 or uint16 input, got f32')
    if x.dim() < 2:
        raise ValueError(f"expected (..., H, W), got {tuple(x.shape)}")
    src = bits16(x).contiguous()
    H, W = x.shape[-2:]
    odt = x.dtype if out == "int" else torch.float32
    res = torch.empty((*x.shape[:-2], factor * H, factor * W), dtype=odt, device=x.device)
    if res.numel():
        with torch.cuda.device(x.device):
            check(lib().fcvsr_bicubic_upscale(src.data_ptr(), _DT[x.dtype], res.numel() // (factor * factor * H * W), H, W, factor,
                                              res.data_ptr(), _DT[odt], stream_ptr()), "fcvsr_bicubic_upscale")
    return res


_RESIZE_TABLES = {}


def resize_device_tables(n_in: int, n_out: int, scale: float, device):
    """(weights f32 (n_out, P), first int32 (n_out,), P) of one axis of fcvsr_imresize on `device`: `harness.resize.resize_taps`,
    uploaded once per (n_in, n_out, scale, device) and kept, so a sequence of frames of one size uploads nothing after its first
    frame."""
    key = (int(n_in), int(n_out), float(scale), str(torch.device(device)))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        from .harness.resize import resize_taps
        w, first = resize_taps(n_in, n_out, scale)
        t = (torch.from_numpy(w).to(device), torch.from_numpy(first).to(device), int(w.shape[1]))
        torch.cuda.synchronize(device)          # readers on any stream find them complete
        _RESIZE_TABLES[key] = t
    return t


def imresize(x: torch.Tensor, scale=None, output_shape=None, out: str = "f32") -> torch.Tensor:
    """fcvsr_imresize: x (..., H, W) uint8, uint16 (10-bit samples) or f32 on the HIP device -> (..., Ho, Wo), MATLAB `imresize`
    at any size (`harness.resize.imresize_host` is the contract), one launch.  Exactly one of `scale` (output ceil(scale * n)) and
    `output_shape` = (Ho, Wo); per-axis scales in [1/8, 8].  out="f32": the f32 sums on x's scale; out="int" (integer x only):
    clipped to [0, peak], rounded half to even, in x's dtype.  Non-contiguous x is made dense first."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor")
    if not x.is_cuda:
        raise RuntimeError("imresize runs on the HIP device only (there is no CPU fallback)")
    if x.dtype not in (torch.uint8, torch.uint16, torch.float32):
        raise ValueError(f"x must be uint8, uint16 or f32, got {x.dtype}")
    if out not in ("f32", "int"):
        raise ValueError(f'out must be "f32" or "int", got {out!r}')
    if out == "int" and x.dtype == torch.float32:
        raise ValueError('out="int" needs uint8 or uint16 input, got f32')
    if x.dim() < 2:
        raise ValueError(f"expected (..., H, W), got {tuple(x.shape)}")
    from .harness.resize import resize_geometry
    H, W = x.shape[-2:]
    (Ho, Wo), (sy, sx), rows_first = resize_geometry(H, W, scale, output_shape)
    odt = x.dtype if out == "int" else torch.float32
    res = torch.empty((*x.shape[:-2], Ho, Wo), dtype=odt, device=x.device)
    if res.numel():
        src = bits16(x).contiguous()
        wy, fy, Py = resize_device_tables(H, Ho, sy, x.device)
        wx, fx, Px = resize_device_tables(W, Wo, sx, x.device)
        with torch.cuda.device(x.device):
            check(lib().fcvsr_imresize(src.data_ptr(), _DT[x.dtype], res.numel() // (Ho * Wo), H, W, Ho, Wo, wy.data_ptr(),
                                       fy.data_ptr(), Py, wx.data_ptr(), fx.data_ptr(), Px, int(rows_first), bits16(res).data_ptr(),
                                       _DT[odt], stream_ptr()), "fcvsr_imresize")
    return res


_INT_SAMPLES = (torch.uint8, torch.uint16, torch.int16)       # int16: the bits of uint16 samples (`bits16`)


def _int_samples(who: str, host: str, what: str, *tensors, dtypes=_INT_SAMPLES) -> None:
    """The argument check of the integer kernels: every tensor is of one of `dtypes` and has the dimensions `what` names, e.g.
    "(N,C,H,W) frames" (ValueError), and lies on the HIP device (RuntimeError: `who` runs there only, `host` says what the host has)."""
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != what.count(",") + 1:
            raise ValueError(f"expected uint8 or uint16 {what}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who} runs on the HIP device only ({host})")


PAIR_SAD_TILE_BYTES = 1024         # FCVSR_PAIR_SAD_TILE_BYTES of include/fcvsr_hip.h: sizes the scratch of fcvsr_frame_pair_sad


def frame_pair_sad(frames: torch.Tensor) -> torch.Tensor:
    """fcvsr_frame_pair_sad: frames (N,C,H,W) uint8, or uint16 (10-bit samples; int16 views of the same bits, `bits16`, are taken
    as uint16) on the HIP device -> (N-1,) int64 on the device, element i the sum over all channels and pixels of
    |frames[i+1] - frames[i]| in exact integers, uint16 samples read as min(k, 1023) (`harness.shots.pair_sad_host` is the
    contract).  Two launches, no host sync.  Any C, H, W >= 1; N = 1 gives an empty result; non-contiguous frames are made dense
    first."""
    _int_samples("frame_pair_sad", "the host path is harness.shots.pair_sad_host", "(N,C,H,W) frames", frames)
    N, samples = frames.shape[0], frames.shape[1] * frames.shape[2] * frames.shape[3]
    if N < 1 or samples < 1:
        raise ValueError(f"frames must hold at least one frame of at least one sample, got {tuple(frames.shape)}")
    out = torch.empty((N - 1,), dtype=torch.int64, device=frames.device)
    if N == 1:
        return out
    src = bits16(frames).contiguous()
    elem = src.element_size()
    tiles = (samples * elem + PAIR_SAD_TILE_BYTES - 1) // PAIR_SAD_TILE_BYTES
    scratch = torch.empty(((N - 1) * tiles,), dtype=torch.int64, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib().fcvsr_frame_pair_sad(src.data_ptr(), elem, N, samples, scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(),
                                         stream_ptr()), "fcvsr_frame_pair_sad")
    return out


LINE_SUMS_SPAN_BYTES, LINE_SUMS_ROWS = 1024, 128      # FCVSR_LINE_SUMS_* of include/fcvsr_hip.h: a workgroup's tile, sizes the scratch


def frame_line_sums(frames: torch.Tensor):
    """fcvsr_frame_line_sums: frames (N,C,H,W) uint8, or uint16 (10-bit samples; int16 views of the same bits, `bits16`, are taken
    as uint16) on the HIP device -> (rows (N,H), cols (N,W)) int64 on the device: the sums of every row and every column over all
    channels in exact integers, uint16 samples read as min(k, 1023) (`harness.active.line_sums_host` is the contract).  Two
    launches, every sample read once, no host sync.  Any N, C, H, W >= 1 and any start address a sample can have; non-contiguous
    frames are made dense first."""
    _int_samples("frame_line_sums", "the host path is harness.active.line_sums_host", "(N,C,H,W) frames", frames)
    N, Cn, H, W = frames.shape
    if min(N, Cn, H, W) < 1:
        raise ValueError(f"frames must hold at least one frame of at least one sample, got {tuple(frames.shape)}")
    src = bits16(frames).contiguous()
    elem = src.element_size()
    rows = torch.empty((N, H), dtype=torch.int64, device=frames.device)
    cols = torch.empty((N, W), dtype=torch.int64, device=frames.device)
    spans, tiles = -(-W * elem // LINE_SUMS_SPAN_BYTES), -(-H // LINE_SUMS_ROWS)
    scratch = torch.empty((N * (spans * H + tiles * W),), dtype=torch.int32, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib().fcvsr_frame_line_sums(src.data_ptr(), elem, N, Cn, H, W, scratch.data_ptr(), scratch.numel() * 4, rows.data_ptr(),
                                          cols.data_ptr(), stream_ptr()), "fcvsr_frame_line_sums")
    return rows, cols


def active_compose(sr_box: torch.Tensor, frames: torch.Tensor, centres, box, H: int, W: int) -> torch.Tensor:
    """fcvsr_active_compose: the (b,C,4H,4W) frames of a group whose resolver saw the box (top, bottom, left, right) only, one launch
    (`harness.active.compose_host` is the contract, bit for bit).  `sr_box`: (b,C,4(bottom-top),4(right-left)) uint8, uint16 or f32
    on the HIP device, any strides (a view is read in place); `frames`: the resident LR frames (N,C,>=H,>=W) of the same dtype, dense
    rows (the last stride 1), of which H x W is the true frame; `centres`: b frame numbers in [0, N), the LR centre frame of every
    `sr_box` frame (a list, uploaded here, or a device int32 tensor the caller has checked).  Inside the box the result is `sr_box`,
    outside it `bicubic_upscale(frames[centres, :, :H, :W], 4)` - out="int" for integer frames, the f32 sums for f32."""
    if not isinstance(sr_box, torch.Tensor) or not isinstance(frames, torch.Tensor) or sr_box.dim() != 4 or frames.dim() != 4:
        raise ValueError("expected (b,C,4hb,4wb) sr_box and (N,C,h,w) frames")
    if not (sr_box.is_cuda and frames.is_cuda):
        raise RuntimeError("active_compose runs on the HIP device only (the host path is harness.active.compose_host)")
    if frames.dtype not in (torch.uint8, torch.uint16, torch.float32) or sr_box.dtype != frames.dtype:
        raise ValueError(f"sr_box and frames must share one dtype of uint8, uint16, f32, got {sr_box.dtype} and {frames.dtype}")
    t, b, l, r = (int(v) for v in box)
    N, Cn = frames.shape[:2]
    H, W = int(H), int(W)
    if not (1 <= H <= frames.shape[2] and 1 <= W <= frames.shape[3] and 0 <= t < b <= H and 0 <= l < r <= W):
        raise ValueError(f"box {(t, b, l, r)} must lie in the {H}x{W} frame, and that in the resident {tuple(frames.shape[2:])} frames")
    B = sr_box.shape[0]
    if tuple(sr_box.shape) != (B, Cn, 4 * (b - t), 4 * (r - l)) or B < 1:
        raise ValueError(f"sr_box must be (b,{Cn},{4 * (b - t)},{4 * (r - l)}), got {tuple(sr_box.shape)}")
    if frames.stride(3) != 1:
        frames = bits16(frames).contiguous().view(frames.dtype)
    if isinstance(centres, torch.Tensor):
        if centres.dtype != torch.int32 or tuple(centres.shape) != (B,) or centres.device != frames.device:
            raise ValueError("centres: a device int32 tensor of b frame numbers")
        cdev = centres.contiguous()
    else:
        centres = [int(c) for c in centres]
        if len(centres) != B or any(not 0 <= c < N for c in centres):
            raise ValueError(f"centres: {B} frame numbers in 0..{N - 1}, got {centres}")
        cdev = torch.tensor(centres, dtype=torch.int32).to(frames.device)
    out = torch.empty((B, Cn, 4 * H, 4 * W), dtype=frames.dtype, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib().fcvsr_active_compose(bits16(sr_box).data_ptr(), *sr_box.stride(), bits16(frames).data_ptr(), cdev.data_ptr(),
                                         *frames.stride()[:3], _DT[frames.dtype], B, Cn, H, W, t, b, l, r, bits16(out).data_ptr(),
                                         stream_ptr()), "fcvsr_active_compose")
    return out


QUANTISE = {"truncate": QUANT_TRUNCATE, "round": QUANT_ROUND}

# the integer sample formats, the only description of them: dtype code, peak, and the host expression of table entry k
_INT_FORMATS = {torch.uint8: (U8, 255, lambda: torch.arange(256, dtype=torch.uint8).float() / 255),
                torch.uint16: (U16, PEAK10, lambda: torch.arange(PEAK10 + 1, dtype=torch.int32).float() / PEAK10)}
_SAMPLE_TABLES = {}


def sample_table(dtype: torch.dtype, device) -> torch.Tensor:
    """The f32 table the entry points of integer format `dtype` read their samples through, on `device` (`u8_table` / `u16_table`
    describe the two).  Built once per format and device, synchronised; create it outside stream fan-out and graph capture."""
    key = (dtype, str(torch.device(device)))
    t = _SAMPLE_TABLES.get(key)
    if t is None:
        t = _INT_FORMATS[dtype][2]().to(device)
        torch.cuda.synchronize(device)          # readers on any stream find it complete
        _SAMPLE_TABLES[key] = t
    return t


def u8_table(device) -> torch.Tensor:
    """The 256-entry f32 table of the uint8 entry points on `device`: entry k is the f32 that ``uint8 -> .float() / 255`` gives on
    the host, so a kernel fed uint8 frames sees the floats of a caller that converts its frames on the host.  Built once per device
    (create it outside stream fan-out and graph capture: Engine.forward_u8's first pass does)."""
    return sample_table(torch.uint8, device)


def u16_table(device) -> torch.Tensor:
    """The 1024-entry f32 table of the uint16 (10-bit) entry points on `device`: entry k is the f32 that ``k.float() / 1023`` gives
    on the host.  The kernels clamp the index to 1023, so a sample above 1023 in its 16-bit container reads the last entry (the
    float path's ``x.clamp(max=1023)``).  Built once per device, outside stream fan-out and graph capture, as `u8_table`."""
    return sample_table(torch.uint16, device)


def _family(name: str, f32: bool = True):
    """{dtype: symbol} of a kernel family with regular names: fcvsr_<name>_u8 / _u16 and, where there is one, fcvsr_<name> for f32."""
    d = {torch.uint8: f"fcvsr_{name}_u8", torch.uint16: f"fcvsr_{name}_u16"}
    return {torch.float32: f"fcvsr_{name}", **d} if f32 else d


# the entry point of every kernel family that has integer forms, by the dtype of the samples it reads (or, for the last kernels
# of the model, writes).  The names are stated here and nowhere else; `_entry` picks one.
_ENTRIES = {
    "samples_to_f32": {torch.uint8: "fcvsr_u8_to_f32", torch.uint16: "fcvsr_u16_to_f32"},        # the format is a prefix
    "chroma_up4": {torch.uint8: "fcvsr_chroma_up4", torch.uint16: "fcvsr_chroma_up4_u16"},       # the uint8 form has no suffix
    "frame_metrics": {torch.uint8: "fcvsr_frame_metrics", torch.uint16: "fcvsr_frame_metrics_u16"},      # by the dtype of hr
    "feat_extract": _family("feat_extract"),
    "bilinear_up4": _family("bilinear_up4"),
    "tail_fused": _family("tail_fused"),
    "tail_fused_base": _family("tail_fused_base"),
    "conv_last": _family("conv_last"),
    "quantise": _family("quantise", f32=False),
    "clip_batch": _family("clip_batch", f32=False),
    "ensemble_windows": _family("ensemble_windows"),
    "tile_windows": _family("tile_windows"),
    "tile_windows_sel": _family("tile_windows_sel"),
    "tile_pairs_equal": _family("tile_pairs_equal"),
}


def _entry(family: str, dtype: torch.dtype, table_on=None):
    """(function, its name, leading table arguments) of `family` for samples of `dtype`.  A family whose integer forms read through
    the sample table names the device in `table_on`; f32 forms, and families without a table, get no table argument."""
    name = _ENTRIES[family][dtype]
    tab = () if table_on is None or dtype == torch.float32 else (sample_table(dtype, table_on).data_ptr(),)
    return getattr(lib(), name), name, tab


def _out_format(dtype: torch.dtype, quantise: Optional[str]):
    """(dtype code, quantise mode) of a merge kernel's result: f32 without `quantise`, uint8 / uint16 with "truncate" / "round"."""
    if dtype == torch.float32:
        if quantise is not None:
            raise ValueError("quantise applies to uint8 / uint16 results only")
        return F32, QUANT_NONE
    if dtype in _INT_FORMATS:
        if quantise not in QUANTISE:
            raise ValueError(f'quantise must be "truncate" or "round", got {quantise!r}')
        return _INT_FORMATS[dtype][0], QUANTISE[quantise]
    raise ValueError(f"dtype: torch.float32, torch.uint8 or torch.uint16, got {dtype!r}")


def _resident_frames(frames) -> None:
    """`frames` is an f32, uint8 or uint16 (N,C,h,w) tensor (ValueError)."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.dtype not in (torch.float32, *_INT_FORMATS):
        raise ValueError(f"frames: expected an f32, uint8 or uint16 (N,C,h,w) tensor, got {getattr(frames, 'dtype', type(frames))} "
                         f"{tuple(getattr(frames, 'shape', ()))}")


def _gather_inputs(who: str, frames, idx) -> None:
    """What the window gathers take alike: `_resident_frames`, `idx` an int32 (b,T) tensor, both on one HIP device, neither empty."""
    _resident_frames(frames)
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int32:
        raise ValueError(f"idx: expected an int32 (b,T) tensor, got {getattr(idx, 'dtype', type(idx))}")
    if not frames.is_cuda or not idx.is_cuda:
        raise RuntimeError(f"{who} runs on the HIP device only (there is no CPU fallback)")
    if frames.device != idx.device:
        raise ValueError(f"frames on {frames.device}, idx on {idx.device}")
    if min(frames.shape) == 0 or idx.numel() == 0:
        raise ValueError(f"empty input: frames {tuple(frames.shape)}, idx {tuple(idx.shape)}")


def bits16(t: torch.Tensor) -> torch.Tensor:
    """torch's uint16 has thin operator coverage on the device: uint16 tensors are padded, stacked, gathered and copied as int16
    views of the same bits (no value is converted; view the result back with ``.view(torch.uint16)``).  Every other dtype is
    returned as it is."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def frames_to_numpy(t: torch.Tensor) -> np.ndarray:
    """Host numpy copy of a tensor of frames; uint16 frames travel as int16 bits (`bits16`) and come back as uint16."""
    a = bits16(t).cpu().numpy()
    return a.view(np.uint16) if t.dtype == torch.uint16 else a


def chroma_up4(planes: torch.Tensor) -> torch.Tensor:
    """fcvsr_chroma_up4 / fcvsr_chroma_up4_u16: (P,h,w) uint8 or uint16 (10-bit samples) planes on the HIP device -> (P,4h,4w) of
    the same dtype, one launch.  Defined as ``F.interpolate(p.float() / peak, scale_factor=4, mode="bicubic",
    align_corners=False)``, clamp(0, 1), * peak, rounded half to even, with peak = 255 or 1023 (within one code value of that torch
    expression: the kernel's f32 sums are not torch's).  uint16 samples above 1023 read as 1023."""
    _int_samples("chroma_up4", "there is no CPU fallback", "(P,h,w) planes", planes, dtypes=tuple(_INT_FORMATS))
    P, h, w = planes.shape
    src = bits16(planes).contiguous()
    out = torch.empty((P, 4 * h, 4 * w), dtype=planes.dtype, device=planes.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(planes.device):
        fn, name, tab = _entry("chroma_up4", planes.dtype, planes.device)
        check(fn(src.data_ptr(), *tab, P, h, w, out.data_ptr(), stream_ptr()), name)
    return out


# The model's first and last kernels (`Engine._forward`).  They run inside graph capture and stream fan-out: nothing here allocates
# or synchronises (the table is a cache hit, `Engine._forward_checked` built it), and the library checks the arguments.  A tensor's
# dtype selects the entry point and the table together; image tensors come as (b,y,x,c) views of any strides.

def samples_to_f32(x: torch.Tensor, out: torch.Tensor) -> None:
    """fcvsr_u8_to_f32 / fcvsr_u16_to_f32: the dense uint8 / uint16 samples of `x` through their table into the dense f32 `out`."""
    fn, name, tab = _entry("samples_to_f32", x.dtype, x.device)
    check(fn(x.data_ptr(), *tab, x.numel(), out.data_ptr(), stream_ptr()), name)


def feat_extract(src: torch.Tensor, B: int, H: int, W: int, wf: torch.Tensor, bf: Optional[torch.Tensor], dsts, n: int,
                 code: int) -> None:
    """fcvsr_feat_extract / _u8 / _u16: the dedicated first convolution on the window `src` (B,H,W,7), f32, uint8 or uint16.  Output
    block k goes to the dense tensor ``dsts[k]`` of `n` channels per pixel, stored as dtype code `code`."""
    fn, name, tab = _entry("feat_extract", src.dtype, src.device)
    xv, nb = view(src), len(dsts)
    check(fn(C.byref(xv), *tab, B, H, W, wf.data_ptr(), ptr(bf), nb, (C.c_void_p * nb)(*[d.data_ptr() for d in dsts]),
             (C.c_int64 * nb)(*([n] * nb)), (C.c_int32 * nb)(*([0] * nb)), code, stream_ptr()), name)


def bilinear_up4(centre: torch.Tensor, out: torch.Tensor) -> None:
    """fcvsr_bilinear_up4 / _u8 / _u16: the bilinear x4 base skip of `centre` (B,H,W,c), f32, uint8 or uint16, into the f32 `out`
    (B,4H,4W,c)."""
    fn, name, tab = _entry("bilinear_up4", centre.dtype, centre.device)
    cv, ov = view(centre), view(out)
    check(fn(C.byref(cv), *tab, *centre.shape[:3], C.byref(ov), stream_ptr()), name)


def tail_fused(u1: torch.Tensor, w2: torch.Tensor, b2: Optional[torch.Tensor], slope: torch.Tensor, wl: torch.Tensor,
               bl: Optional[torch.Tensor], B: int, H2: int, W2: int, out: torch.Tensor, *, base: Optional[torch.Tensor] = None,
               centre: Optional[torch.Tensor] = None, quant: Optional[int] = None) -> None:
    """fcvsr_tail_fused[_base][_u8|_u16]: the fused end of the S-model up-sampler into `out` (B,2 H2,2 W2,1), f32, or uint8 / uint16
    quantised by `quant`.  Exactly one of `base` and `centre`: `base` is the f32 tensor that holds the base skip (an f32 `out`
    accumulates in place, so `base` is then `out` itself; an integer `out` only reads it); `centre` is the LR centre frame
    (B,H2/2,W2/2,1) of `out`'s dtype, from which the kernel evaluates the base itself."""
    if (base is None) == (centre is None):
        raise ValueError("tail_fused takes exactly one of base and centre")
    integer = out.dtype != torch.float32
    if base is None:
        fn, name, tab = _entry("tail_fused_base", out.dtype, out.device)
    else:
        fn, name, tab = _entry("tail_fused", out.dtype)
    u1v, sv, ov = view(u1), view(centre if base is None else base), view(out)
    lead = (C.byref(sv), *tab) if base is None else ()                      # the centre frame and its table stand before the sizes,
    dst = (C.byref(sv), C.byref(ov)) if integer and base is not None else (C.byref(ov),)      # a base that is only read before out
    check(fn(C.byref(u1v), w2.data_ptr(), ptr(b2), slope.data_ptr(), wl.data_ptr(), ptr(bl), *lead, B, H2, W2, *dst,
             *((quant,) if integer else ()), stream_ptr()), name)


def conv_last(u2: torch.Tensor, wl: torch.Tensor, bias: Optional[torch.Tensor], B: int, H4: int, W4: int, Cimg: int,
              base: torch.Tensor, out: torch.Tensor, quant: Optional[int] = None) -> None:
    """fcvsr_conv_last / _u8 / _u16: conv_last0 over `u2` (B,H4,W4,64) on top of the f32 base skip `base` into `out` (B,H4,W4,Cimg):
    f32 (accumulated in place: `base` is `out` itself), or uint8 / uint16 quantised by `quant` (`base` is only read)."""
    fn, name, _ = _entry("conv_last", out.dtype)
    u2v, bv, ov = view(u2), view(base), view(out)
    tail = (C.byref(ov),) if out.dtype == torch.float32 else (C.byref(bv), C.byref(ov), quant)
    check(fn(C.byref(u2v), wl.data_ptr(), ptr(bias), B, H4, W4, Cimg, *tail, stream_ptr()), name)


def quantise(src: torch.Tensor, out: torch.Tensor, quant: int) -> None:
    """fcvsr_quantise_u8 / _u16: the dense f32 `src` into the dense uint8 / uint16 `out`, quantised by `quant`."""
    fn, name, _ = _entry("quantise", out.dtype)
    check(fn(src.data_ptr(), src.numel(), quant, out.data_ptr(), stream_ptr()), name)


SURFACE_FMTS = {"yuv420p": 0, "yuv420p10le": 1, "nv12": 2, "p010le": 3}      # enum fcvsr_surface of include/fcvsr_hip.h


def _surface_fmt(fmt):
    """(enum value, sample dtype) of a surface format name; ValueError for anything else."""
    if fmt not in SURFACE_FMTS:
        raise ValueError(f"pix_fmt must be one of {tuple(SURFACE_FMTS)}, got {fmt!r}")
    return SURFACE_FMTS[fmt], (torch.uint8 if fmt in ("yuv420p", "nv12") else torch.uint16)


def _surface_planes(name: str, dt: torch.dtype, *tensors):
    """The dtype and device checks of the two surface wrappers; int16 views of uint16 planes (`bits16`) are taken as uint16."""
    for t in tensors:
        ok = (torch.uint8,) if dt == torch.uint8 else (torch.uint16, torch.int16)
        if not isinstance(t, torch.Tensor) or t.dtype not in ok:
            raise ValueError(f"{name}: expected {dt} tensors, got {getattr(t, 'dtype', type(t))}")
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP device only (the host path is harness.surfaces)")
        if t.device != tensors[0].device:
            raise ValueError(f"{name}: tensors on {tensors[0].device} and {t.device}")


def surface_unpack(raw: torch.Tensor, fmt: str, width: int, height: int, slots: torch.Tensor, ring_y: torch.Tensor,
                   ring_u: torch.Tensor, ring_v: torch.Tensor) -> None:
    """fcvsr_surface_unpack: `raw`, a dense uint8 tensor on the HIP device holding n whole `width` x `height` frames of `fmt` as they
    were read, is taken apart into plane rings (`harness.surfaces.unpack_host` is the contract): the luma of frame i goes to slot
    ``slots[i]`` of `ring_y` (R,1,Hp,Wp) - Hp >= height, Wp >= width; the rows and columns beyond the frame are never written -, U
    and V to the same slot of `ring_u` / `ring_v` (R,height/2,width/2).  `slots`: n int32 on the device, distinct, each in
    [0, R) (a number outside the ring writes nothing).  The rings are contiguous uint8 (yuv420p, nv12) or uint16 (yuv420p10le,
    p010le) tensors.  One launch on the current stream, no host sync."""
    code, dt = _surface_fmt(fmt)
    if width <= 0 or height <= 0 or width % 2 or height % 2:
        raise ValueError(f"4:2:0 frames need an even, positive width and height, got {width}x{height}")
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8 or not raw.is_contiguous():
        raise ValueError(f"raw: expected a contiguous uint8 tensor, got {getattr(raw, 'dtype', type(raw))}")
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or slots.dim() != 1 or not slots.is_contiguous():
        raise ValueError(f"slots: expected a contiguous 1-D int32 tensor, got {getattr(slots, 'dtype', type(slots))}")
    _surface_planes("surface_unpack", dt, ring_y, ring_u, ring_v)
    if not raw.is_cuda or not slots.is_cuda:
        raise RuntimeError("surface_unpack runs on the HIP device only (the host path is harness.surfaces.unpack_host)")
    if raw.device != ring_y.device or slots.device != ring_y.device:
        raise ValueError(f"surface_unpack: raw on {raw.device}, slots on {slots.device}, rings on {ring_y.device}")
    n, fb = slots.numel(), width * height * 3 // 2 * (1 if dt == torch.uint8 else 2)
    if raw.numel() != n * fb:
        raise ValueError(f"raw holds {raw.numel()} bytes, {n} {width}x{height} {fmt} frames are {n * fb}")
    if ring_y.dim() != 4 or ring_y.shape[1] != 1 or ring_y.shape[2] < height or ring_y.shape[3] < width:
        raise ValueError(f"ring_y must be (R,1,Hp,Wp) with Hp >= {height}, Wp >= {width}, got {tuple(ring_y.shape)}")
    R, _, Hp, Wp = ring_y.shape
    for name, t in (("ring_u", ring_u), ("ring_v", ring_v)):
        if tuple(t.shape) != (R, height // 2, width // 2):
            raise ValueError(f"{name} must be (R,H/2,W/2) = {(R, height // 2, width // 2)}, got {tuple(t.shape)}")
    if R < 1 or not all(t.is_contiguous() for t in (ring_y, ring_u, ring_v)):
        raise ValueError("the rings must be contiguous and hold at least one slot")
    if n == 0:
        return
    with torch.cuda.device(raw.device):
        check(lib().fcvsr_surface_unpack(raw.data_ptr(), code, n, height, width, slots.data_ptr(), R, Hp, Wp, ring_y.data_ptr(),
                                         ring_u.data_ptr(), ring_v.data_ptr(), stream_ptr()), "fcvsr_surface_unpack")


def _dense_frames(t: torch.Tensor) -> torch.Tensor:
    """`t` (b,h,w) if its frames are dense (any frame stride: a plane of a batch of I420 frames), else a dense copy."""
    b, h, w = t.shape
    if t.stride(2) == 1 and t.stride(1) == w and (b == 1 or t.stride(0) >= h * w):
        return t
    return bits16(t).contiguous().view(t.dtype)


def surface_pack(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, fmt: str) -> torch.Tensor:
    """fcvsr_surface_pack: y (b,H,W), u and v (b,H/2,W/2) uint8 (yuv420p, nv12) or uint16 (yuv420p10le, p010le) planes on the HIP
    device -> a dense uint8 (b, frame bytes) buffer in the layout of `fmt`, equal to `harness.surfaces.pack_host`: one copy to
    the host and one ``write`` deliver the batch.  Planes whose frames are dense are read where they lie at any frame stride (three
    tensors, slices of one, or the planes `harness.colour.i420_planes` gives).  One launch on the current stream."""
    code, dt = _surface_fmt(fmt)
    _surface_planes("surface_pack", dt, y, u, v)
    if y.dim() != 3 or u.dim() != 3 or u.shape != v.shape:
        raise ValueError(f"expected Y (b,H,W), U and V (b,H/2,W/2), got {tuple(y.shape)}, {tuple(u.shape)}, {tuple(v.shape)}")
    b, H, W = y.shape
    if W <= 0 or H <= 0 or W % 2 or H % 2:
        raise ValueError(f"4:2:0 frames need an even, positive width and height, got {W}x{H}")
    if tuple(u.shape) != (b, H // 2, W // 2):
        raise ValueError(f"chroma planes must be (b,H/2,W/2) = {(b, H // 2, W // 2)}, got {tuple(u.shape)}")
    out = torch.empty((b, W * H * 3 // 2 * (1 if dt == torch.uint8 else 2)), dtype=torch.uint8, device=y.device)
    if b == 0:
        return out
    y, u, v = _dense_frames(y), _dense_frames(u), _dense_frames(v)
    with torch.cuda.device(y.device):
        check(lib().fcvsr_surface_pack(y.data_ptr(), u.data_ptr(), v.data_ptr(), y.stride(0), u.stride(0), v.stride(0), code, b, H,
                                       W, out.data_ptr(), stream_ptr()), "fcvsr_surface_pack")
    return out


PLANE_SSE_SPAN_BYTES, PLANE_SSE_ROWS = 1024, 32       # FCVSR_PLANE_SSE_* of include/fcvsr_hip.h: a workgroup's tile, sizes the scratch


def plane_sse(a: torch.Tensor, b: torch.Tensor, crop: int = 0) -> torch.Tensor:
    """fcvsr_plane_sse: `a` and `b` (P,h,w) uint8, or uint16 (10-bit samples; int16 views of the same bits, `bits16`, are taken as
    uint16) planes of one dtype on the HIP device -> (P,) int64 on the device, element p the sum of ``(a[p] - b[p]) ** 2`` over
    ``[crop:h-crop, crop:w-crop]`` in exact integers, uint16 samples read as min(k, 1023) (`harness.reference.plane_sse_host` is the
    contract).  Two launches, no host sync.  Planes whose rows are dense are read where they lie at any plane stride and any
    sample-aligned address (three tensors, slices of a ring, the Y / U / V views `harness.colour.i420_planes` gives); anything else
    is made dense first.  P = 0 gives an empty result; ``2 * crop < min(h, w)``."""
    _int_samples("plane_sse", "the host path is harness.reference.plane_sse_host", "(P,h,w) planes", a, b)
    a, b = bits16(a), bits16(b)
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"a and b must share dtype, shape and device, got {a.dtype} {tuple(a.shape)} on {a.device} and "
                         f"{b.dtype} {tuple(b.shape)} on {b.device}")
    P, h, w = a.shape
    crop = int(crop)
    if P > 65535 or h < 1 or w < 1 or crop < 0 or 2 * crop >= min(h, w):
        raise ValueError(f"plane_sse: at most 65535 planes of at least 1x1 and 0 <= 2 crop < min(h, w), got {tuple(a.shape)}, crop {crop}")
    out = torch.empty((P,), dtype=torch.int64, device=a.device)
    if P == 0:
        return out
    a, b = _dense_frames(a), _dense_frames(b)
    elem = a.element_size()
    parts = -(-(w - 2 * crop) * elem // PLANE_SSE_SPAN_BYTES) * -(-(h - 2 * crop) // PLANE_SSE_ROWS)
    scratch = torch.empty((P * parts,), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().fcvsr_plane_sse(a.data_ptr(), b.data_ptr(), elem, P, h, w, a.stride(0), b.stride(0), crop, scratch.data_ptr(),
                                    scratch.numel() * 8, out.data_ptr(), stream_ptr()), "fcvsr_plane_sse")
    return out


# ---- tOF: Farneback flow and the end-point distance (csrc/flow.hip; the contract is harness/tof.py) ---------------------------------

FLOW_U8, FLOW_U16, FLOW_F32, FLOW_RGB8 = 0, 1, 2, 3     # enum fcvsr_flow_elem
FLOW_R_CHANNELS = 8                                      # FCVSR_FLOW_R_CHANNELS: floats per pixel of a polynomial expansion, 5 live
FLOW_SCRATCH_BYTES = 1 << 30                             # `farneback_flow` scores larger batches in chunks of planes under this scratch
_FLOW_ELEM = {torch.uint8: FLOW_U8, torch.uint16: FLOW_U16, torch.float32: FLOW_F32}


def _flow_planes(who: str, t, rgb: bool):
    """(tensor with dense rows, elem code, h, w) of the (P,h,w) planes - (P,3,h,w) uint8 with `rgb` - of a flow entry point."""
    dims = 4 if rgb else 3
    if not isinstance(t, torch.Tensor) or t.dim() != dims or (rgb and (t.dtype != torch.uint8 or t.shape[1] != 3)):
        raise ValueError(f"{who}: expected {'(P,3,h,w) uint8 RGB frames' if rgb else '(P,h,w) planes'}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.dtype == torch.int16:
        t = t.view(torch.uint16)
    if t.dtype not in _FLOW_ELEM:
        raise ValueError(f"{who}: planes are uint8, uint16 (or its int16 bits) or float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on the HIP device only (the host path is harness.tof.farneback_host)")
    h, w = t.shape[-2:]
    if h < 2 or w < 2 or h > 16384 or w > 16384 or t.shape[0] > 65535:
        raise ValueError(f"{who}: at most 65535 planes of 2 .. 16384 samples a side, got {tuple(t.shape)}")
    dense = t.stride(-1) == 1 and t.stride(-2) == w and (not rgb or t.stride(1) == h * w) and (t.shape[0] < 2 or t.stride(0) >= 0)
    if not dense:
        t = bits16(t).contiguous()
        t = t.view(torch.uint16) if t.dtype == torch.int16 else t
    return t, (FLOW_RGB8 if rgb else _FLOW_ELEM[t.dtype]), h, w


def farneback_flow(prev: torch.Tensor, next: torch.Tensor, *, rgb: bool = False, **params) -> torch.Tensor:
    """fcvsr_farneback_flow: `prev` and `next` (P,h,w) uint8, uint16 (10-bit samples, read as min(k, 1023); int16 bits are taken as
    uint16) or f32 planes of one dtype on the HIP device - with ``rgb=True`` (P,3,h,w) uint8 RGB frames, read as the float Y of
    `harness.metrics` - -> f32 (P,h,w,2) on the device, the dense flow [dx, dy] of every pair (`harness.tof.farneback_host` is the
    contract: cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0) restated by reading).  The keywords of that
    call (``pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags``) are accepted at exactly these values; anything
    else is a ValueError.  Planes with dense rows are read where they lie at any plane stride: ``x[:-1]`` and ``x[1:]`` of one
    buffer need no copy.  The flow of a pair does not depend on the batch it is in.  No host sync."""
    from .harness.tof import check_params
    check_params(**params)
    prev, elem, h, w = _flow_planes("farneback_flow", prev, rgb)
    next, elem2, h2, w2 = _flow_planes("farneback_flow", next, rgb)
    if elem != elem2 or prev.shape != next.shape or prev.device != next.device:
        raise ValueError(f"prev and next must share dtype, shape and device, got {prev.dtype} {tuple(prev.shape)} on {prev.device} and "
                         f"{next.dtype} {tuple(next.shape)} on {next.device}")
    P = prev.shape[0]
    out = torch.empty((P, h, w, 2), dtype=torch.float32, device=prev.device)
    if P == 0:
        return out
    per = int(lib().fcvsr_farneback_scratch_bytes(1, h, w))
    step = max(1, min(P, FLOW_SCRATCH_BYTES // per))
    with torch.cuda.device(prev.device):
        nbytes = int(lib().fcvsr_farneback_scratch_bytes(step, h, w))
        scratch = torch.empty((nbytes // 4,), dtype=torch.float32, device=prev.device)
        sp, sn = (prev.stride(0) if P > 1 else 0), (next.stride(0) if P > 1 else 0)
        for i in range(0, P, step):
            n = min(step, P - i)
            check(lib().fcvsr_farneback_flow(prev[i:].data_ptr(), next[i:].data_ptr(), elem, n, h, w, sp, sn, scratch.data_ptr(), nbytes,
                                             out[i:].data_ptr(), stream_ptr()), "fcvsr_farneback_flow")
    return out


def _f32_dense(who: str, shape_doc: str, dims: int, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != dims:
            raise ValueError(f"{who}: expected float32 {shape_doc}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who} runs on the HIP device only (the host path is in harness.tof)")
    return [t.contiguous() for t in tensors]


def flow_epe(flow_a: torch.Tensor, flow_b: torch.Tensor) -> torch.Tensor:
    """fcvsr_flow_epe: two f32 (P,h,w,2) flow fields on the HIP device -> f64 (P,) on the device, per plane the mean over pixels of
    sqrt(ddx^2 + ddy^2), each value in f32, added in f64 in a fixed order (`harness.tof.epe_host`).  Two launches, no host sync."""
    a, b = _f32_dense("flow_epe", "(P,h,w,2) flows", 4, flow_a, flow_b)
    if a.shape != b.shape or a.shape[3] != 2 or a.device != b.device or a.shape[1] < 1 or a.shape[2] < 1 or a.shape[0] > 65535:
        raise ValueError(f"flow_epe: two (P,h,w,2) flows of one shape and device, got {tuple(a.shape)}, {tuple(b.shape)}")
    P, h, w, _ = a.shape
    out = torch.empty((P,), dtype=torch.float64, device=a.device)
    if P == 0:
        return out
    with torch.cuda.device(a.device):
        nbytes = int(lib().fcvsr_flow_epe_scratch_bytes(P, h, w))
        scratch = torch.empty((nbytes // 8,), dtype=torch.float64, device=a.device)
        check(lib().fcvsr_flow_epe(a.data_ptr(), b.data_ptr(), P, h, w, scratch.data_ptr(), nbytes, out.data_ptr(), stream_ptr()),
              "fcvsr_flow_epe")
    return out


def flow_level_size(h: int, w: int, level: int):
    from .harness.tof import level_geometry
    return level_geometry(h, w, level)[2]


def flow_level_image(planes: torch.Tensor, level: int, *, rgb: bool = False) -> torch.Tensor:
    """fcvsr_flow_level_image: stage (a) of the flow, (P,h,w) planes -> f32 (P,hl,wl), `harness.tof.level_image_host`."""
    planes, elem, h, w = _flow_planes("flow_level_image", planes, rgb)
    if level not in (0, 1, 2, 3):
        raise ValueError(f"level: 0 .. 3, got {level!r}")
    hl, wl = flow_level_size(h, w, level)
    P = planes.shape[0]
    out = torch.empty((P, hl, wl), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().fcvsr_flow_level_image(planes.data_ptr(), elem, P, h, w, planes.stride(0) if P > 1 else 0, level, out.data_ptr(),
                                           stream_ptr()), "fcvsr_flow_level_image")
    return out


def flow_poly_exp(img: torch.Tensor) -> torch.Tensor:
    """fcvsr_flow_poly_exp: stage (b), f32 (n,h,w) -> (n,h,w,8), channels (y, x, yy, xx, xy, 0, 0, 0); `harness.tof.poly_exp_host`."""
    img, = _f32_dense("flow_poly_exp", "(n,h,w) images", 3, img)
    n, h, w = img.shape
    R = torch.empty((n, h, w, FLOW_R_CHANNELS), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        check(lib().fcvsr_flow_poly_exp(img.data_ptr(), n, h, w, R.data_ptr(), stream_ptr()), "fcvsr_flow_poly_exp")
    return R


def flow_matrices(R0: torch.Tensor, R1: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """fcvsr_flow_matrices: stage (c) from a given flow, R0, R1 (P,h,w,8), flow (P,h,w,2) -> M (P,5,h,w); `harness.tof.matrices_host`."""
    R0, R1, flow = _f32_dense("flow_matrices", "(P,h,w,8) expansions and a (P,h,w,2) flow", 4, R0, R1, flow)
    P, h, w, _ = R0.shape
    if R0.shape[3] != FLOW_R_CHANNELS or R1.shape != R0.shape or tuple(flow.shape) != (P, h, w, 2):
        raise ValueError(f"flow_matrices: R0, R1 (P,h,w,8) and flow (P,h,w,2), got {tuple(R0.shape)}, {tuple(R1.shape)}, {tuple(flow.shape)}")
    M = torch.empty((P, 5, h, w), dtype=torch.float32, device=R0.device)
    with torch.cuda.device(R0.device):
        check(lib().fcvsr_flow_matrices(R0.data_ptr(), R1.data_ptr(), flow.data_ptr(), P, h, w, M.data_ptr(), stream_ptr()),
              "fcvsr_flow_matrices")
    return M


def flow_box_solve(M: torch.Tensor) -> torch.Tensor:
    """fcvsr_flow_box_solve: one iteration of stage (d) without the matrix update, M (P,5,h,w) -> flow (P,h,w,2);
    `harness.tof.box_solve_host`."""
    M, = _f32_dense("flow_box_solve", "(P,5,h,w) matrices", 4, M)
    P, c, h, w = M.shape
    if c != 5:
        raise ValueError(f"flow_box_solve: M (P,5,h,w), got {tuple(M.shape)}")
    flow = torch.empty((P, h, w, 2), dtype=torch.float32, device=M.device)
    with torch.cuda.device(M.device):
        check(lib().fcvsr_flow_box_solve(M.data_ptr(), P, h, w, flow.data_ptr(), stream_ptr()), "fcvsr_flow_box_solve")
    return flow


def clip_batch(desc: torch.Tensor, s: int, out: torch.Tensor, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
    """fcvsr_clip_batch_u8 / fcvsr_clip_batch_u16: `desc` is a uint8 tensor on the HIP device holding P = numel / sizeof(CropDesc)
    descriptors (the bytes of a ``numpy.dtype(CropDesc)`` array), `out` a contiguous f32 tensor of P * s * s elements on the same
    device: plane p becomes the s x s window descriptor p names, flipped / transposed by its flags, pixel k as ``u8_table[k]``.
    `dtype` is the sample type of the source planes: ``torch.uint16`` reads every descriptor as a window of 2-byte samples (`src`
    2-byte aligned, `pitch` / `top` / `left` in samples) and gives pixel k as ``u16_table[min(k, 1023)]``.  One launch on the
    current stream.  The descriptors are device memory nobody checks here: the caller keeps every window inside its plane (and keeps
    `desc` and the source planes alive until the launch has run)."""
    if dtype not in _INT_FORMATS:
        raise ValueError(f"dtype: the source planes are torch.uint8 or torch.uint16, got {dtype!r}")
    for name, t, dt in (("desc", desc, torch.uint8), ("out", out, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous {dt} tensor, got {getattr(t, 'dtype', type(t))}")
        if not t.is_cuda:
            raise RuntimeError("clip_batch runs on the HIP device only (there is no CPU fallback)")
    if desc.device != out.device:
        raise ValueError(f"desc on {desc.device}, out on {out.device}")
    P, rem = divmod(desc.numel(), C.sizeof(CropDesc))
    if rem or P == 0 or out.numel() != P * s * s:
        raise ValueError(f"{desc.numel()} descriptor bytes / {out.numel()} output elements do not make whole {s} x {s} planes")
    with torch.cuda.device(out.device):
        fn, name, tab = _entry("clip_batch", dtype, out.device)
        check(fn(desc.data_ptr(), *tab, P, s, out.data_ptr(), stream_ptr()), name)
    return out


def _ceil4(v: int) -> int:
    return (v + 3) // 4 * 4


def ensemble_windows(frames: torch.Tensor, idx: torch.Tensor, reverse: bool = False):
    """fcvsr_ensemble_windows / _u8 / _u16: the 8 self-ensemble variants (`harness.ensemble.variant_host`) of b windows, one launch.
    `frames` is the dense UNPADDED sequence (N,C,h,w) on the HIP device, f32, uint8 or uint16 (integer samples enter as
    ``u8_table`` / ``u16_table[min(k, 1023)]``); `idx` an int32 (b,T) tensor on the same device, row i the frame numbers of window
    i (``reverse`` reads every row backwards).  Returns f32 ``(4,b,T,C,ceil4(h),ceil4(w))`` (variants 0..3) and
    ``(4,b,T,C,ceil4(w),ceil4(h))`` (variants 4..7), each variant zero-padded at its own bottom / right."""
    _gather_inputs("ensemble_windows", frames, idx)
    N, Cc, h, w = frames.shape
    (b, T), dev = idx.shape, frames.device
    src, idx = bits16(frames).contiguous(), idx.contiguous()
    out_a = torch.empty((4, b, T, Cc, _ceil4(h), _ceil4(w)), dtype=torch.float32, device=dev)
    out_t = torch.empty((4, b, T, Cc, _ceil4(w), _ceil4(h)), dtype=torch.float32, device=dev)
    tail = (N, Cc, h, w, idx.data_ptr(), b, T, int(bool(reverse)), out_a.data_ptr(), out_t.data_ptr())
    with torch.cuda.device(dev):
        fn, name, tab = _entry("ensemble_windows", frames.dtype, dev)
        check(fn(src.data_ptr(), *tab, *tail, stream_ptr()), name)
    return out_a, out_t


def ensemble_merge(a: torch.Tensor, at: torch.Tensor, h: int, w: int, *, ra: Optional[torch.Tensor] = None,
                   rat: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float32, quantise: Optional[str] = None) -> torch.Tensor:
    """fcvsr_ensemble_merge: `a` (4,b,C,4 ceil4(h),4 ceil4(w)) and `at` (4,b,C,4 ceil4(w),4 ceil4(h)), f32 on the HIP device, are the
    model's outputs for variants 0..3 and 4..7 of b windows of h x w frames.  Returns the dense (b,C,4h,4w) self-ensemble result
    (`harness.ensemble.ensemble_host`: crop, inverse transform, the fixed-order f32 sum, * 0.125): f32, or - `dtype` uint8 / uint16
    with `quantise` "truncate" / "round" - quantised as the model's integer paths quantise.  `ra` / `rat`: the same pair for the
    time-reversed windows; the result is then the mean of the two means.  One launch."""
    ts = [("a", a), ("at", at)] + ([("ra", ra), ("rat", rat)] if ra is not None or rat is not None else [])
    for name, t in ts:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 5:
            raise ValueError(f"{name}: expected an f32 (4,b,C,rows,cols) tensor, got {getattr(t, 'dtype', type(t))}")
        if not t.is_cuda:
            raise RuntimeError("ensemble_merge runs on the HIP device only (there is no CPU fallback)")
    if h < 1 or w < 1:
        raise ValueError(f"h, w must be positive, got {h}, {w}")
    b, Cc = a.shape[1], a.shape[2]
    sa, st = (4, b, Cc, 4 * _ceil4(h), 4 * _ceil4(w)), (4, b, Cc, 4 * _ceil4(w), 4 * _ceil4(h))
    for name, t in ts:
        want = sa if name in ("a", "ra") else st
        if tuple(t.shape) != want or t.device != a.device:
            raise ValueError(f"{name}: expected {want} on {a.device}, got {tuple(t.shape)} on {t.device}")
    if b == 0 or Cc == 0:
        raise ValueError(f"empty input: {tuple(a.shape)}")
    code, q = _out_format(dtype, quantise)
    a, at = a.contiguous(), at.contiguous()
    ra, rat = (ra.contiguous(), rat.contiguous()) if ra is not None else (None, None)
    out = torch.empty((b, Cc, 4 * h, 4 * w), dtype=dtype, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), ptr(ra), ptr(rat), b, Cc, h, w, code, q, out.data_ptr(),
                                         stream_ptr()), "fcvsr_ensemble_merge")
    return out


TILE_EQ_SEG_CHUNKS = 1024                       # FCVSR_TILE_EQ_SEG_CHUNKS


def _tile_plan_for(plan, h: int, w: int, what: str):
    if (plan.h, plan.w) != (h, w):
        raise ValueError(f"{what}: the plan is for {plan.h} x {plan.w} frames, got {h} x {w}")


def tile_windows(frames: torch.Tensor, idx: torch.Tensor, plan, sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fcvsr_tile_windows / _u8 / _u16: the tile windows (`harness.tiles`) of b windows, one launch.  `frames` is the dense UNPADDED
    sequence (N,C,h,w) on the HIP device, f32, uint8 or uint16 (integer samples enter as ``u8_table`` / ``u16_table[min(k, 1023)]``);
    `idx` an int32 (b,T) tensor on the same device, row i the frame numbers of window i; `plan` the `harness.tiles.TilePlan` of
    h x w frames.  Returns f32 ``(b,ny,nx,T,C,th,tw)``: tile (ky,kx) is the window cut at ``(plan.ys[ky], plan.xs[kx])`` out of the
    frames zero-padded at the bottom / right to multiples of 4.

    `sel` (fcvsr_tile_windows_sel / _u8 / _u16): an int32 (n,3) tensor on the same device, rows ``(bi, ky, kx)`` in any order,
    repeats allowed.  Returns f32 ``(n,T,C,th,tw)``, row k the bits of ``tile_windows(frames, idx, plan)[bi, ky, kx]``; the other
    tile windows are not made."""
    _gather_inputs("tile_windows", frames, idx)
    if sel is not None:
        if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32 or sel.dim() != 2 or sel.shape[1] != 3 or sel.shape[0] < 1:
            raise ValueError(f"sel: expected an int32 (n,3) tensor with n >= 1, got {getattr(sel, 'dtype', type(sel))} "
                             f"{tuple(getattr(sel, 'shape', ()))}")
        if sel.device != frames.device:
            raise ValueError(f"frames on {frames.device}, sel on {sel.device}")
    N, Cc, h, w = frames.shape
    _tile_plan_for(plan, h, w, "tile_windows")
    (b, T), dev = idx.shape, frames.device
    src, idx = bits16(frames).contiguous(), idx.contiguous()
    ys, xs, _, _ = plan.device_tables(dev)
    if sel is None:
        family, extra = "tile_windows", ()
        out = torch.empty((b, plan.ny, plan.nx, T, Cc, plan.th, plan.tw), dtype=torch.float32, device=dev)
    else:
        sel = sel.contiguous()
        family, extra = "tile_windows_sel", (sel.data_ptr(), sel.shape[0])
        out = torch.empty((sel.shape[0], T, Cc, plan.th, plan.tw), dtype=torch.float32, device=dev)
    tail = (N, Cc, h, w, idx.data_ptr(), b, T, ys.data_ptr(), plan.ny, xs.data_ptr(), plan.nx, plan.th, plan.tw, *extra, out.data_ptr())
    with torch.cuda.device(dev):
        fn, name, tab = _entry(family, frames.dtype, dev)
        check(fn(src.data_ptr(), *tab, *tail, stream_ptr()), name)
    return out


def tile_eq_segments(Cc: int, th: int, tw: int, elem_size: int) -> int:
    """The flags per tile fcvsr_tile_pairs_equal writes into its scratch array (FCVSR_TILE_EQ_SEG_CHUNKS chunks of 16 bytes each)."""
    return -(-(Cc * th * -(-(tw * elem_size) // 16)) // TILE_EQ_SEG_CHUNKS)


def tile_pairs_equal(frames: torch.Tensor, pairs: torch.Tensor, plan) -> torch.Tensor:
    """fcvsr_tile_pairs_equal / _u8 / _u16: `frames` the dense UNPADDED sequence (N,C,h,w) on the HIP device, f32, uint8 or uint16;
    `pairs` an int32 (P,2) tensor of frame numbers on the same device; `plan` the `harness.tiles.TilePlan` of h x w frames.  Returns
    uint8 ``(P,ny,nx)``: 1 where the two frames of the pair hold the same bits (bytes, raw 16-bit words, 32-bit patterns) in every
    sample of every channel on the tile's rectangle clipped to the frame, 0 otherwise (`harness.tiles.static_map_host` is the
    specification).  Two launches, no host synchronisation."""
    _resident_frames(frames)
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
        raise ValueError(f"pairs: expected an int32 (P,2) tensor with P >= 1, got {getattr(pairs, 'dtype', type(pairs))} "
                         f"{tuple(getattr(pairs, 'shape', ()))}")
    if not frames.is_cuda or not pairs.is_cuda:
        raise RuntimeError("tile_pairs_equal runs on the HIP device only (there is no CPU fallback)")
    if frames.device != pairs.device:
        raise ValueError(f"frames on {frames.device}, pairs on {pairs.device}")
    if min(frames.shape) == 0:
        raise ValueError(f"empty input: frames {tuple(frames.shape)}")
    N, Cc, h, w = frames.shape
    _tile_plan_for(plan, h, w, "tile_pairs_equal")
    dev, P = frames.device, pairs.shape[0]
    src, pairs = bits16(frames).contiguous(), pairs.contiguous()
    ys, xs, _, _ = plan.device_tables(dev)
    nbytes = P * plan.ny * plan.nx * tile_eq_segments(Cc, plan.th, plan.tw, frames.element_size())
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = torch.empty((P, plan.ny, plan.nx), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        fn, name, _ = _entry("tile_pairs_equal", frames.dtype)      # compares bits: no table
        check(fn(src.data_ptr(), N, Cc, h, w, pairs.data_ptr(), P, ys.data_ptr(), plan.ny, xs.data_ptr(), plan.nx,
                                   plan.th, plan.tw, scratch.data_ptr(), nbytes, out.data_ptr(), stream_ptr()), name)
    return out


def tile_merge(tiles: torch.Tensor, plan, h: int, w: int, *, dtype: torch.dtype = torch.float32,
               quantise: Optional[str] = None, src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fcvsr_tile_merge: `tiles` (b,ny,nx,C,4th,4tw), f32 on the HIP device, are the model's outputs for the tile windows of b
    windows of h x w frames (`plan`: their `harness.tiles.TilePlan`).  Returns the dense (b,C,4h,4w) blend (`harness.tiles.blend_host`:
    crop, the normalised feathered weights, the fixed-order f32 sum): f32, or - `dtype` uint8 / uint16 with `quantise` "truncate" /
    "round" - quantised as the model's integer paths quantise.  One launch.

    `src` (fcvsr_tile_merge_sel): an int32 (b,ny,nx) tensor of slots on the same device; `tiles` is then a pool (n,C,4th,4tw) and
    the result is, bit for bit, ``tile_merge(tiles[src.long()], ...)`` without that tensor being made."""
    if src is None:
        if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.float32 or tiles.dim() != 6:
            raise ValueError(f"tiles: expected an f32 (b,ny,nx,C,4th,4tw) tensor, got {getattr(tiles, 'dtype', type(tiles))} "
                             f"{tuple(getattr(tiles, 'shape', ()))}")
    else:
        if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.float32 or tiles.dim() != 4 or tiles.shape[0] < 1:
            raise ValueError(f"tiles: with src expected an f32 pool (n,C,4th,4tw), got {getattr(tiles, 'dtype', type(tiles))} "
                             f"{tuple(getattr(tiles, 'shape', ()))}")
        if not isinstance(src, torch.Tensor) or src.dtype != torch.int32 or src.dim() != 3:
            raise ValueError(f"src: expected an int32 (b,ny,nx) tensor, got {getattr(src, 'dtype', type(src))} "
                             f"{tuple(getattr(src, 'shape', ()))}")
        if src.device != tiles.device:
            raise ValueError(f"tiles on {tiles.device}, src on {src.device}")
    if not tiles.is_cuda:
        raise RuntimeError("tile_merge runs on the HIP device only (there is no CPU fallback)")
    _tile_plan_for(plan, h, w, "tile_merge")
    if src is None:
        b, Cc = tiles.shape[0], tiles.shape[3]
        want = (b, plan.ny, plan.nx, Cc, 4 * plan.th, 4 * plan.tw)
    else:
        b, Cc = src.shape[0], tiles.shape[1]
        want = (tiles.shape[0], Cc, 4 * plan.th, 4 * plan.tw)
        if tuple(src.shape) != (b, plan.ny, plan.nx):
            raise ValueError(f"src: expected (b,{plan.ny},{plan.nx}), got {tuple(src.shape)}")
    if tuple(tiles.shape) != want:
        raise ValueError(f"tiles: expected {want}, got {tuple(tiles.shape)}")
    if b == 0 or Cc == 0:
        raise ValueError(f"empty input: {tuple(tiles.shape)}")
    code, q = _out_format(dtype, quantise)
    tiles = tiles.contiguous()
    ys, xs, wy, wx = plan.device_tables(tiles.device)
    out = torch.empty((b, Cc, 4 * h, 4 * w), dtype=dtype, device=tiles.device)
    grid = (ys.data_ptr(), plan.ny, xs.data_ptr(), plan.nx, plan.th, plan.tw, wy.data_ptr(), wx.data_ptr(), b, Cc, h, w, code, q,
            out.data_ptr())
    with torch.cuda.device(tiles.device):
        if src is None:
            check(lib().fcvsr_tile_merge(tiles.data_ptr(), *grid, stream_ptr()), "fcvsr_tile_merge")
        else:
            src = src.contiguous()
            check(lib().fcvsr_tile_merge_sel(tiles.data_ptr(), tiles.shape[0], src.data_ptr(), *grid, stream_ptr()),
                  "fcvsr_tile_merge_sel")
    return out
