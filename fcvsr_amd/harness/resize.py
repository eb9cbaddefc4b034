"""MATLAB-style antialiased bicubic down-scaling on the device (the reference's mmedit/datasets/pipelines/matlab_like_resize.py
MATLABLikeResize at scale 1/2 or 1/4): the step between NIQE's two scales, and at 4x the standard "BI" LR maker.  The CPU contract
is `harness.niqe.bicubic_downscale`; there is no CPU fallback behind the device function: host tensors raise."""
from __future__ import annotations

import torch

from .. import hip


def bicubic_downscale(x: torch.Tensor, factor: int) -> torch.Tensor:
    """x: (..., H, W) uint8 or f32 on the HIP device, H and W multiples of `factor` (2 or 4).  Returns f32 (..., H/factor, W/factor)
    on x's scale (uint8 frames give values around [0,255], not clipped or rounded), with the bits of the reference: rows first, then
    columns, f32 products added in tap order, out-of-range taps reflected with edge repeat.  One launch (fcvsr_bicubic_downscale)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor")
    return hip.bicubic_downscale(x, factor)
