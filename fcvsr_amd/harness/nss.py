"""What the two no-reference scores (NIQE, `niqe.py`; BRISQUE, `brisque.py`) share on the host: the shape grid of their GGD / AGGD
fits, the 7 x 7 window loop of their MSCN stage, the per-device copy of their gamma tables and the checks of their device frames.
The device side of the same front end is csrc/score_common.h."""
from __future__ import annotations

from typing import Optional

import numpy as np

GAM = np.arange(0.2, 10.001, 0.001)                         # the shape grid of the GGD and AGGD fits, 9801 entries


def corr7(img: np.ndarray, taps: np.ndarray, pad_mode: str) -> np.ndarray:
    """Correlation of an (H,W) plane with 7 x 7 `taps`, the plane padded by 3 with np.pad's `pad_mode` ("edge": replicated border,
    "constant": zeros), accumulated from 0 in row-major tap order.  The device kernel adds in the same order."""
    H, W = img.shape
    p = np.pad(img, 3, mode=pad_mode)
    acc = np.zeros((H, W), dtype=np.float64)
    for ky in range(7):
        for kx in range(7):
            acc += taps[ky, kx] * p[ky:ky + H, kx:kx + W]
    return acc


_DEVICE_TABLES = {}


def device_tables(name: str, tables: np.ndarray, device):
    """The device copy of a score's (4, 9801) host table, uploaded once per (table name, device)."""
    import torch
    key = (name, str(torch.device(device)))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        t = torch.from_numpy(tables.copy()).to(device)
        torch.cuda.synchronize(device)                      # readers on any stream find it complete
        _DEVICE_TABLES[key] = t
    return t


def check_frames(frames, quantise: Optional[str], convert_to: Optional[str], what: str) -> bool:
    """The checks `frame_niqe_features` and `frame_brisque_features` share, `what` being "NIQE" or "BRISQUE": (N,C,H,W) device
    frames, uint8 with quantise=None or f32 with "truncate" / "round", C = 1 or 3 with convert_to="Y".  Returns to_y."""
    import torch
    from .device_metrics import _QUANTISE
    if quantise not in _QUANTISE:
        raise ValueError(f'quantise must be "truncate", "round" or None, got {quantise!r}')
    if convert_to is not None and not (isinstance(convert_to, str) and convert_to.lower() == "y"):
        raise ValueError('Wrong color model. Supported values are "Y" and None')
    to_y = convert_to is not None
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a torch tensor")
    if frames.dtype == torch.uint16:
        raise ValueError(f"{what} is defined on 8-bit frames: uint16 (10-bit) frames are not supported")
    if not frames.is_cuda:
        raise RuntimeError(f"frame_{what.lower()} runs on the HIP device only (there is no CPU fallback)")
    if frames.dim() != 4:
        raise ValueError(f"expected (N,C,H,W) frames, got shape {tuple(frames.shape)}")
    want = torch.uint8 if quantise is None else torch.float32
    if frames.dtype != want:
        raise ValueError(f"frames must be {want} with quantise={quantise!r}, got {frames.dtype}")
    if frames.shape[1] != (3 if to_y else 1):
        raise ValueError(f"{what} scores one plane: C must be 1, or 3 with convert_to='Y', got C={frames.shape[1]}")
    return to_y
