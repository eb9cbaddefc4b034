"""Quality metrics computed where the frames are: per-frame PSNR and SSIM of N SR / HR frame pairs on the HIP device
(fcvsr_frame_metrics; the CPU functions of `metrics.py` are the contract, reference CVSR_train/metric/psnr_ssim.py:278-398,
:447-485).  There is no CPU fallback: host tensors raise."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import hip
from .metrics import _gaussian_window

_QUANTISE = {None: hip.QUANT_NONE, "truncate": hip.QUANT_TRUNCATE, "round": hip.QUANT_ROUND}


def frame_metrics(sr: torch.Tensor, hr: torch.Tensor, *, crop_border: int = 4, quantise: Optional[str] = "truncate",
                  convert_to: Optional[str] = None, peak: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """sr: (N,C,H,W) f32 model output in [0,1] (any strides, e.g. a cropped view of the padded output), quantised in the
    kernel the way `super_resolve_sequence` does ("truncate": `.to(torch.uint8)`, "round": `.round()` first), or uint8 frames
    with `quantise=None`.  hr: uint8 (N,C,H,W).  convert_to="Y" scores the Y channel of RGB frames (C = 3).

    10-bit frames: hr uint16 (N,C,H,W), sr f32 (quantised in the kernel with the 1023 scale) or uint16 with `quantise=None`;
    fcvsr_frame_metrics_u16 scores them.  `peak` is the PSNR peak and the peak of the SSIM constants: None means 255 for uint8 hr and
    1023 for uint16 hr (full scale); a caller who scores the HM way passes 1020.  uint8 frames are scored at 255 only, and
    convert_to="Y" is not defined for uint16 frames (ValueError).

    Returns (psnr, ssim), two f64 device tensors of shape (N,): per frame, `metrics.psnr` and `metrics.ssim` of the HWC frames
    (PSNR over all channels, SSIM the mean of the per-channel SSIMs; PSNR is inf when the frames are equal)."""
    if quantise not in _QUANTISE:
        raise ValueError(f'quantise must be "truncate", "round" or None, got {quantise!r}')
    if convert_to is not None and not (isinstance(convert_to, str) and convert_to.lower() == "y"):
        raise ValueError('Wrong color model. Supported values are "Y" and None')
    to_y = convert_to is not None
    if not isinstance(sr, torch.Tensor) or not isinstance(hr, torch.Tensor):
        raise TypeError("sr and hr must be torch tensors")
    if not sr.is_cuda or not hr.is_cuda:
        raise RuntimeError("frame_metrics runs on the HIP device only (there is no CPU fallback)")
    if sr.device != hr.device:
        raise ValueError(f"sr and hr are on different devices: {sr.device}, {hr.device}")
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError(f"expected sr and hr of one (N,C,H,W) shape, got {tuple(sr.shape)}, {tuple(hr.shape)}")
    if hr.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f"hr must be uint8 or uint16, got {hr.dtype}")
    u16 = hr.dtype == torch.uint16
    if u16 and to_y:
        raise ValueError('convert_to="Y" is not defined for uint16 (10-bit) frames')
    if peak is None:
        peak = float(hip.PEAK10) if u16 else 255.0
    peak = float(peak)
    if not peak > 0:
        raise ValueError(f"peak must be positive, got {peak}")
    if not u16 and peak != 255.0:
        raise ValueError(f"uint8 frames are scored at peak 255, got peak={peak}")
    want = hr.dtype if quantise is None else torch.float32
    if sr.dtype != want:
        raise ValueError(f"sr must be {want} with quantise={quantise!r}, got {sr.dtype}")
    N, C, H, W = sr.shape
    if to_y and C != 3:
        raise ValueError(f"convert_to='Y' needs 3-channel (RGB) frames, got C={C}")
    if crop_border < 0:
        raise ValueError(f"crop_border must be >= 0, got {crop_border}")
    if min(H, W) - 2 * crop_border - 10 < 1:
        raise ValueError(f"{H}x{W} frames leave no SSIM region with crop_border={crop_border} and the 11x11 window")
    if N == 0:
        empty = torch.empty((0,), dtype=torch.float64, device=sr.device)
        return empty, empty.clone()
    with torch.cuda.device(sr.device):
        sums = hip.frame_metric_sums(sr, hr, _QUANTISE[quantise], int(crop_border), to_y, _gaussian_window(), peak=peak)
    planes = 1 if to_y else C
    mse = sums[:, 0] / float((H - 2 * crop_border) * (W - 2 * crop_border) * planes)
    psnr = torch.where(mse == 0, torch.full_like(mse, float("inf")), 20.0 * torch.log10(peak / torch.sqrt(mse)))
    ssim = sums[:, 1] / float((H - 2 * crop_border - 10) * (W - 2 * crop_border - 10) * planes)
    return psnr, ssim
