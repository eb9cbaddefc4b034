"""Raw YUV 4:2:0 surface formats: the layouts a decoder hands out, as numpy functions (host logic; the contract the kernels
`fcvsr_surface_unpack` / `fcvsr_surface_pack` of csrc/surface.hip are pinned to).

The names and layouts are ffmpeg's ``-pix_fmt`` ones.  A frame of W x H (both even) is

    yuv420p       Y (H x W bytes), U (H/2 x W/2), V (H/2 x W/2): the I420 layout `harness.yuv` reads
    yuv420p10le   the same planes in little-endian 16-bit words, the 10-bit value in the LOW bits
    nv12          Y (H x W bytes), then H/2 rows of W bytes with U and V interleaved: U0 V0 U1 V1 ...
    p010le        the NV12 layout in little-endian 16-bit words, the 10-bit value in the HIGH bits: word = value << 6

frames back to back.  Reading P010 takes ``word >> 6`` (the low six bits are ignored, whatever they hold) and writing stores
``value << 6``.  Planar 10-bit samples pass through unchanged, values above 1023 included: the kernels downstream read them as
``min(k, 1023)`` (`super_resolve_u16`, the pair-SAD kernel), exactly as they do for a file read by `harness.yuv.read_yuv420`.

This module needs numpy only.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

PIX_FMTS = ("yuv420p", "yuv420p10le", "nv12", "p010le")
_BITS = {"yuv420p": 8, "yuv420p10le": 10, "nv12": 8, "p010le": 10}
_SEMI = {"yuv420p": False, "yuv420p10le": False, "nv12": True, "p010le": True}
P010_SHIFT = 6


def check_fmt(fmt: str) -> str:
    if fmt not in PIX_FMTS:
        raise ValueError(f"pix_fmt must be one of {PIX_FMTS}, got {fmt!r}")
    return fmt


def _check_size(w: int, h: int):
    if w <= 0 or h <= 0 or w % 2 or h % 2:
        raise ValueError(f"4:2:0 frames need an even, positive width and height, got {w}x{h}")


def bit_depth(fmt: str) -> int:
    """8 or 10."""
    return _BITS[check_fmt(fmt)]


def is_semi_planar(fmt: str) -> bool:
    """True for the formats whose chroma is one interleaved plane (nv12, p010le)."""
    return _SEMI[check_fmt(fmt)]


def sample_dtype(fmt: str) -> np.dtype:
    """The sample type of the planes: uint8, or little-endian uint16."""
    return np.dtype(np.uint8) if bit_depth(fmt) == 8 else np.dtype("<u2")


def frame_bytes(fmt: str, w: int, h: int) -> int:
    """Bytes of one w x h frame."""
    check_fmt(fmt)
    _check_size(w, h)
    return w * h * 3 // 2 * sample_dtype(fmt).itemsize


def unpack_host(raw, fmt: str, w: int, h: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """raw: the bytes of n whole frames (uint8 array, bytes or a buffer).  Returns y (n,h,w), u and v (n,h/2,w/2), uint8 or
    uint16.  P010 words are shifted right by 6; planar 10-bit words come back as they are."""
    fb = frame_bytes(fmt, w, h)
    raw = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
    if raw.dtype != np.uint8:
        raise ValueError(f"raw must be uint8 bytes, got {raw.dtype}")
    raw = np.ascontiguousarray(raw).reshape(-1)
    if raw.size % fb:
        raise ValueError(f"{raw.size} bytes is not a whole number of {w}x{h} {fmt} frames ({fb} bytes each)")
    n, dt = raw.size // fb, sample_dtype(fmt)
    s = raw.view(dt).reshape(n, w * h * 3 // 2)
    ys, h2, w2 = w * h, h // 2, w // 2
    y = s[:, :ys].reshape(n, h, w)
    if _SEMI[fmt]:
        uv = s[:, ys:].reshape(n, h2, w2, 2)
        u, v = uv[..., 0], uv[..., 1]
    else:
        u, v = s[:, ys:ys + h2 * w2].reshape(n, h2, w2), s[:, ys + h2 * w2:].reshape(n, h2, w2)
    out_dt = np.uint8 if dt.itemsize == 1 else np.uint16
    y, u, v = (np.ascontiguousarray(a).astype(out_dt, copy=False) for a in (y, u, v))
    if fmt == "p010le":
        y, u, v = y >> P010_SHIFT, u >> P010_SHIFT, v >> P010_SHIFT
    return y, u, v


def pack_host(y, u, v, fmt: str) -> bytes:
    """y (n,h,w), u and v (n,h/2,w/2) uint8 (8-bit formats) or uint16 (10-bit formats) -> the bytes of n frames of `fmt`.  P010
    stores ``value << 6`` in 16 bits."""
    check_fmt(fmt)
    y, u, v = (np.asarray(a) for a in (y, u, v))
    want = np.uint8 if bit_depth(fmt) == 8 else np.uint16
    if any(a.dtype != want for a in (y, u, v)):
        raise ValueError(f"{fmt} planes must be {np.dtype(want).name}, got {y.dtype}, {u.dtype}, {v.dtype}")
    if y.ndim != 3 or u.ndim != 3 or u.shape != v.shape:
        raise ValueError(f"expected Y (n,h,w), U and V (n,h/2,w/2), got {y.shape}, {u.shape}, {v.shape}")
    n, h, w = y.shape
    _check_size(w, h)
    if u.shape != (n, h // 2, w // 2):
        raise ValueError(f"chroma planes must be (n,h/2,w/2) = {(n, h // 2, w // 2)}, got {u.shape}")
    if fmt == "p010le":
        y, u, v = ((a << P010_SHIFT).astype(np.uint16) for a in (y, u, v))
    c = np.stack([u, v], -1).reshape(n, -1) if _SEMI[fmt] else np.concatenate([u.reshape(n, -1), v.reshape(n, -1)], 1)
    frames = np.concatenate([y.reshape(n, -1), c], 1)
    return np.ascontiguousarray(frames.astype(sample_dtype(fmt), copy=False)).tobytes()
