"""YUV 4:2:0 <-> RGB for the RGB models (`FCVSRNet`, `FCVSR_SNet`): the integer specification on the host, and the device wrappers of
the two kernels of csrc/colour.hip, which equal it bit for bit.

Everything is integer arithmetic with 14-bit fixed-point coefficients, so host and device can agree exactly (every intermediate is
below 2^27 in magnitude; ``>>`` is an arithmetic shift).  With d the bit depth (8 or 10), P = 2^d - 1, s = 2^(d-8) and
r(x) = floor(x * 2^14 + 0.5) in float64:

    constants   limited range: y_off = 16s, y_rng = 219s, c_rng = 224s; full range: y_off = 0, y_rng = c_rng = P; c_off = 2^(d-1);
                Kr, Kb of the matrix ("bt601" 0.299, 0.114; "bt709" 0.2126, 0.0722), Kg = 1 - Kr - Kb; RGB is full range 0..P
    decode      cy = r(P/y_rng), rv = r(2(1-Kr) P/c_rng), gu = r(2Kb(1-Kb)/Kg P/c_rng), gv = r(2Kr(1-Kr)/Kg P/c_rng),
                bu = r(2(1-Kb) P/c_rng);
                Yt = cy*(y - y_off) + 2^13, U = up(u) - c_off, V = up(v) - c_off,
                R = clip((Yt + rv*V) >> 14), G = clip((Yt - gu*U - gv*V) >> 14), B = clip((Yt + bu*U) >> 14)
    encode      kr = r(Kr y_rng/P), kb = r(Kb y_rng/P), kg = r(y_rng/P) - kr - kb; ur = r(Kr/(2(1-Kb)) c_rng/P),
                ug = r(Kg/(2(1-Kb)) c_rng/P), ub = ur + ug; vg = r(Kg/(2(1-Kr)) c_rng/P), vb = r(Kb/(2(1-Kr)) c_rng/P), vr = vg + vb;
                Y = clip(((kr*R + kg*G + kb*B + 2^13) >> 14) + y_off); cb = -ur*R - ug*G + ub*B, cr = vr*R - vg*G - vb*B at full
                resolution, unrounded; t[X] = cb[2j, X] + cb[2j+1, X];
                "center": Cb = clip(((t[2i] + t[2i+1] + 2^15) >> 16) + c_off)
                "left":   Cb = clip(((t[max(2i-1, 0)] + 2 t[2i] + t[2i+1] + 2^16) >> 17) + c_off);   Cr likewise from cr
    up(c)       h x w -> 2h x 2w, indices clamped: j = Y>>1, j' = j-1 (Y even) or j+1, vertical weights 3 : 1 (centre-sited);
                "center" (JPEG / MPEG-1): i = X>>1, i' = i-1 (X even) or i+1,
                          up = (3*(3c[j,i] + c[j,i']) + (3c[j',i] + c[j',i']) + 8) >> 4
                "left" (MPEG-2 / H.264 / HEVC type 0, co-sited with even luma columns): i' = i (X even) or i+1,
                          up = (3*(c[j,i] + c[j,i']) + (c[j',i] + c[j',i']) + 4) >> 3

A sample above P in a 16-bit container reads as P, as everywhere else in the project.  This module imports without a GPU; the device
wrappers raise RuntimeError for CPU tensors (there is no CPU fallback: the host functions are the specification, not a code path).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from .. import hip
from .surfaces import _check_size

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CHROMA_LOCS = {"left": hip.CHROMA_LEFT, "center": hip.CHROMA_CENTER}
SHIFT = 14


@dataclass(frozen=True)
class ColourSpec:
    """What a YUV 4:2:0 stream says about itself: the matrix, the range of its code values, where its chroma samples sit, and
    the bit depth.  The defaults are those of HD video (BT.709, limited range, chroma co-sited with the even luma columns)."""
    matrix: str = "bt709"
    full_range: bool = False
    chroma_loc: str = "left"
    bit_depth: int = 8

    def __post_init__(self):
        if self.matrix not in MATRICES:
            raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if self.chroma_loc not in CHROMA_LOCS:
            raise ValueError(f"chroma_loc must be one of {sorted(CHROMA_LOCS)}, got {self.chroma_loc!r}")
        if self.bit_depth not in (8, 10):
            raise ValueError(f"bit_depth must be 8 or 10, got {self.bit_depth!r}")
        if not isinstance(self.full_range, (bool, np.bool_)):
            raise ValueError(f"full_range must be a bool, got {self.full_range!r}")

    @property
    def peak(self) -> int:
        return (1 << self.bit_depth) - 1

    @property
    def dtype(self) -> torch.dtype:
        return torch.uint8 if self.bit_depth == 8 else torch.uint16


def _r(x: float) -> int:
    return int(np.floor(np.float64(x) * np.float64(1 << SHIFT) + np.float64(0.5)))


def coefficients(spec: ColourSpec) -> Dict[str, int]:
    """The integer constants of `spec` (the fields of ``fcvsr_colour``)."""
    kr_, kb_ = (np.float64(v) for v in MATRICES[spec.matrix])
    kg_ = 1.0 - kr_ - kb_
    P, s = spec.peak, 1 << (spec.bit_depth - 8)
    y_off, y_rng, c_rng = (0, P, P) if spec.full_range else (16 * s, 219 * s, 224 * s)
    c = {"shift": SHIFT, "chroma_loc": CHROMA_LOCS[spec.chroma_loc], "y_off": y_off, "c_off": 1 << (spec.bit_depth - 1)}
    c.update(cy=_r(P / y_rng), rv=_r(2 * (1 - kr_) * P / c_rng), gu=_r(2 * kb_ * (1 - kb_) / kg_ * P / c_rng),
             gv=_r(2 * kr_ * (1 - kr_) / kg_ * P / c_rng), bu=_r(2 * (1 - kb_) * P / c_rng))
    c.update(kr=_r(kr_ * y_rng / P), kb=_r(kb_ * y_rng / P))
    c["kg"] = _r(y_rng / P) - c["kr"] - c["kb"]
    c.update(ur=_r(kr_ / (2 * (1 - kb_)) * c_rng / P), ug=_r(kg_ / (2 * (1 - kb_)) * c_rng / P))
    c["ub"] = c["ur"] + c["ug"]
    c.update(vg=_r(kg_ / (2 * (1 - kr_)) * c_rng / P), vb=_r(kb_ / (2 * (1 - kr_)) * c_rng / P))
    c["vr"] = c["vg"] + c["vb"]
    return c


def _host_planes(spec: ColourSpec, *arrays):
    out = []
    for a in arrays:
        a = np.asarray(a)
        if a.dtype.kind not in "ui":
            raise ValueError(f"samples must be integers, got {a.dtype}")
        out.append(np.minimum(a.astype(np.int64), spec.peak))
    return out


def upsample_chroma_host(c: np.ndarray, chroma_loc: str) -> np.ndarray:
    """up(c) of the module docstring: (N,h,w) int64 -> (N,2h,2w) int64."""
    h, w = c.shape[-2:]
    Y, X = np.arange(2 * h), np.arange(2 * w)
    j, i = Y >> 1, X >> 1
    j2 = np.clip(np.where(Y % 2 == 0, j - 1, j + 1), 0, h - 1)
    if chroma_loc == "center":
        i2 = np.clip(np.where(X % 2 == 0, i - 1, i + 1), 0, w - 1)
    else:
        i2 = np.clip(np.where(X % 2 == 0, i, i + 1), 0, w - 1)
    a, b = c[..., j[:, None], i[None, :]], c[..., j[:, None], i2[None, :]]
    a2, b2 = c[..., j2[:, None], i[None, :]], c[..., j2[:, None], i2[None, :]]
    if chroma_loc == "center":
        return (3 * (3 * a + b) + (3 * a2 + b2) + 8) >> 4
    return (3 * (a + b) + (a2 + b2) + 4) >> 3


def yuv420_to_rgb_host(y, u, v, spec: ColourSpec = ColourSpec()) -> np.ndarray:
    """The decode specification in numpy int64: y (N,H,W), u and v (N,H/2,W/2) integer arrays -> (N,3,H,W) uint8 / uint16."""
    y, u, v = _host_planes(spec, y, u, v)
    if y.ndim != 3 or u.ndim != 3 or u.shape != v.shape:
        raise ValueError(f"expected Y (N,H,W), U and V (N,H/2,W/2), got {y.shape}, {u.shape}, {v.shape}")
    N, H, W = y.shape
    _check_size(W, H)
    if u.shape != (N, H // 2, W // 2):
        raise ValueError(f"chroma planes must be (N,H/2,W/2) = {(N, H // 2, W // 2)}, got {u.shape}")
    k, P = coefficients(spec), spec.peak
    yt = k["cy"] * (y - k["y_off"]) + (1 << (SHIFT - 1))
    U = upsample_chroma_host(u, spec.chroma_loc) - k["c_off"]
    V = upsample_chroma_host(v, spec.chroma_loc) - k["c_off"]
    rgb = np.stack([(yt + k["rv"] * V) >> SHIFT, (yt - k["gu"] * U - k["gv"] * V) >> SHIFT, (yt + k["bu"] * U) >> SHIFT], 1)
    return np.clip(rgb, 0, P).astype(np.uint8 if spec.bit_depth == 8 else np.uint16)


def rgb_to_yuv420_host(rgb, spec: ColourSpec = ColourSpec()) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The encode specification in numpy int64: (N,3,H,W) integer frames, H and W even -> y (N,H,W), u, v (N,H/2,W/2)."""
    (rgb,) = _host_planes(spec, rgb)
    if rgb.ndim != 4 or rgb.shape[1] != 3:
        raise ValueError(f"expected (N,3,H,W) frames, got {rgb.shape}")
    N, _, H, W = rgb.shape
    _check_size(W, H)
    k, P = coefficients(spec), spec.peak
    dt = np.uint8 if spec.bit_depth == 8 else np.uint16
    R, G, B = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    y = np.clip(((k["kr"] * R + k["kg"] * G + k["kb"] * B + (1 << (SHIFT - 1))) >> SHIFT) + k["y_off"], 0, P).astype(dt)
    out = [y]
    for c in (-k["ur"] * R - k["ug"] * G + k["ub"] * B, k["vr"] * R - k["vg"] * G - k["vb"] * B):
        t = c[:, 0::2] + c[:, 1::2]                                               # (N, H/2, W)
        if spec.chroma_loc == "center":
            q = ((t[..., 0::2] + t[..., 1::2] + (1 << (SHIFT + 1))) >> (SHIFT + 2))
        else:
            left = t[..., np.maximum(2 * np.arange(W // 2) - 1, 0)]
            q = ((left + 2 * t[..., 0::2] + t[..., 1::2] + (1 << (SHIFT + 2))) >> (SHIFT + 3))
        out.append(np.clip(q + k["c_off"], 0, P).astype(dt))
    return tuple(out)


# ---- device ----------------------------------------------------------------------------------------------------------------

def _colour_struct(spec: ColourSpec) -> hip.Colour:
    return hip.Colour(**coefficients(spec))


def _check_device(name: str, spec: ColourSpec, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != spec.dtype:
            raise ValueError(f"{name}: a {spec.bit_depth}-bit spec takes {spec.dtype} tensors, got {getattr(t, 'dtype', type(t))}")
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP device only (there is no CPU fallback; the *_host functions are the "
                               "specification)")
        if t.device != tensors[0].device:
            raise ValueError(f"{name}: tensors on {tensors[0].device} and {t.device}")


def _frame_strided(t: torch.Tensor) -> torch.Tensor:
    """`t` (N,h,w) if its frames are dense (rows and columns contiguous, any frame stride: a plane of an I420 batch buffer), else
    a dense copy (made on the int16 bits for uint16, `hip.bits16`)."""
    n, h, w = t.shape
    if t.stride(2) == 1 and t.stride(1) == w and (n == 1 or t.stride(0) >= h * w):
        return t
    return hip.bits16(t).contiguous().view(t.dtype)


def i420_frame_samples(H: int, W: int) -> int:
    _check_size(W, H)
    return H * W * 3 // 2


def i420_planes(frames: torch.Tensor, H: int, W: int):
    """The Y (N,H,W), U and V (N,H/2,W/2) planes of an (N, H*W*3/2) batch of I420 frames, as views (nothing is copied)."""
    fs = i420_frame_samples(H, W)
    if frames.dim() != 2 or frames.shape[1] != fs or frames.stride(1) != 1:
        raise ValueError(f"expected (N, {fs}) I420 frames of {W}x{H} with dense samples, got {tuple(frames.shape)}")
    n, hw, cw = frames.shape[0], H * W, (H // 2) * (W // 2)
    return (frames[:, :hw].unflatten(1, (H, W)), frames[:, hw:hw + cw].unflatten(1, (H // 2, W // 2)),
            frames[:, hw + cw:].unflatten(1, (H // 2, W // 2)))


def yuv420_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, spec: ColourSpec = ColourSpec()) -> torch.Tensor:
    """fcvsr_yuv420_to_rgb / _u16: y (N,H,W), u and v (N,H/2,W/2) uint8 (8-bit spec) or uint16 (10-bit) on the HIP device -> planar
    RGB (N,3,H,W) of the same dtype, equal to `yuv420_to_rgb_host`.  One launch on the current stream.  Planes with dense frames at
    any frame stride (the views `i420_planes` gives) are read where they lie."""
    _check_device("yuv420_to_rgb", spec, y, u, v)
    if y.dim() != 3 or u.dim() != 3 or u.shape != v.shape:
        raise ValueError(f"expected Y (N,H,W), U and V (N,H/2,W/2), got {tuple(y.shape)}, {tuple(u.shape)}, {tuple(v.shape)}")
    N, H, W = y.shape
    _check_size(W, H)
    if tuple(u.shape) != (N, H // 2, W // 2):
        raise ValueError(f"chroma planes must be (N,H/2,W/2) = {(N, H // 2, W // 2)}, got {tuple(u.shape)}")
    rgb = torch.empty((N, 3, H, W), dtype=spec.dtype, device=y.device)
    if N == 0:
        return rgb
    y, u, v = _frame_strided(y), _frame_strided(u), _frame_strided(v)
    fn, name = ((hip.lib().fcvsr_yuv420_to_rgb, "fcvsr_yuv420_to_rgb") if spec.bit_depth == 8 else
                (hip.lib().fcvsr_yuv420_to_rgb_u16, "fcvsr_yuv420_to_rgb_u16"))
    k = _colour_struct(spec)
    with torch.cuda.device(y.device):
        hip.check(fn(y.data_ptr(), u.data_ptr(), v.data_ptr(), N, H, W, y.stride(0), u.stride(0), v.stride(0), k, rgb.data_ptr(),
                     hip.stream_ptr()), name)
    return rgb


def rgb_to_i420(rgb: torch.Tensor, spec: ColourSpec = ColourSpec()) -> torch.Tensor:
    """fcvsr_rgb_to_yuv420 / _u16 into I420 frame layout: planar RGB (N,3,H,W) uint8 / uint16 on the HIP device, H and W even ->
    (N, H*W*3/2) frames, each ``Y | U | V`` as a file holds it; the planes equal `rgb_to_yuv420_host`.  One launch on the current
    stream (a frame tensor that is not dense is copied first)."""
    _check_device("rgb_to_yuv420", spec, rgb)
    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"expected (N,3,H,W) frames, got {tuple(rgb.shape)}")
    N, _, H, W = rgb.shape
    fs = i420_frame_samples(H, W)
    out = torch.empty((N, fs), dtype=spec.dtype, device=rgb.device)
    if N == 0:
        return out
    if not rgb.is_contiguous():
        rgb = hip.bits16(rgb).contiguous().view(rgb.dtype)
    y, u, v = i420_planes(out, H, W)
    fn, name = ((hip.lib().fcvsr_rgb_to_yuv420, "fcvsr_rgb_to_yuv420") if spec.bit_depth == 8 else
                (hip.lib().fcvsr_rgb_to_yuv420_u16, "fcvsr_rgb_to_yuv420_u16"))
    k = _colour_struct(spec)
    with torch.cuda.device(rgb.device):
        hip.check(fn(rgb.data_ptr(), N, H, W, k, fs, fs, fs, y.data_ptr(), u.data_ptr(), v.data_ptr(), hip.stream_ptr()), name)
    return out


def rgb_to_yuv420(rgb: torch.Tensor, spec: ColourSpec = ColourSpec()):
    """`rgb_to_i420`, returned as its planes y (N,H,W), u and v (N,H/2,W/2): views of one I420 batch buffer."""
    return i420_planes(rgb_to_i420(rgb, spec), rgb.shape[2], rgb.shape[3])
