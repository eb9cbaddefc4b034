"""MATLAB-style bicubic resizing on the device (the reference's mmedit/datasets/pipelines/matlab_like_resize.py MATLABLikeResize).
Down, at scale 1/2 or 1/4 (antialiased): the step between NIQE's two scales, and at 4x the standard "BI" LR maker.  Up, at scale 2
or 4: MATLAB `imresize`, the "Bicubic" baseline row of SR tables.  The CPU contracts are `harness.niqe.bicubic_downscale` and
`harness.niqe.bicubic_upscale`; there is no CPU fallback behind the device functions: host tensors raise."""
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


def bicubic_upscale(x: torch.Tensor, factor: int, *, out: str = "f32") -> torch.Tensor:
    """x: (..., H, W) uint8, uint16 (10-bit samples; above 1023 reads as 1023) or f32 on the HIP device, any H, W >= 1; `factor` 2 or
    4.  Returns (..., factor H, factor W) with the bits of the reference: rows first, then columns, a = -0.5 cubic taps, f32
    products added in tap order, out-of-range taps reflected with edge repeat.  out="f32": f32 on x's scale, not clipped or rounded.
    out="int" (integer x only): clipped to [0, 255] or [0, 1023], rounded half to even, in x's dtype - what `imresize` gives for an
    integer image, and the frame a bicubic baseline is scored on.  Non-contiguous x is made dense.  One launch
    (fcvsr_bicubic_upscale)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor")
    return hip.bicubic_upscale(x, factor, out)
