"""MATLAB-style bicubic resizing on the device (the reference's mmedit/datasets/pipelines/matlab_like_resize.py MATLABLikeResize).
Down, at scale 1/2 or 1/4 (antialiased): the step between NIQE's two scales, and at 4x the standard "BI" LR maker.  Up, at scale 2
or 4: MATLAB `imresize`, the "Bicubic" baseline row of SR tables.  The CPU contracts are `harness.niqe.bicubic_downscale` and
`harness.niqe.bicubic_upscale`; there is no CPU fallback behind the device functions: host tensors raise.

Any size: `imresize(x, scale=... | output_shape=...)` is the same operator with the scale free (per axis, in [1/8, 8]) - what
`output_shape=` of the sequence and YUV entry points delivers frames with.  Its CPU contract, `imresize_host`, and the tap tables
both sides use, `resize_tables` / `resize_taps`, live here."""
from __future__ import annotations

import numpy as np
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


# ---- any output size: MATLABLikeResize(scale=..., output_shape=...) -------------------------------------------------------------------
# The numpy functions below are the CPU contract of the device `imresize`; they restate the reference's arithmetic, dtype by dtype,
# and are pinned to its recorded outputs (tests/golden/imresize_cases.npz).  One rule everywhere: weights in f32, one f32 product per
# tap, products added in TAP ORDER in f32, the pass with the smaller scale first (rows on a tie), the intermediate an f32.  The
# reference departs from tap order in one degenerate class - a pass of 8 or more stored taps over a plane whose other extent is 1,
# where numpy collapses the axes and sums pairwise in blocks of 8 (1 ulp away); the contract keeps tap order there as well.
MIN_SCALE, MAX_SCALE = 1.0 / 8, 8.0                         # at most ceil(4 * 8) + 2 = 34 taps
MAX_TAPS = 34
_INT_PEAK = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 1023}


def _reflect(idx: np.ndarray, n: int) -> np.ndarray:
    """Out-of-range indices reflected with edge repeat (-1 -> 0, -2 -> 1, n -> n-1), period 2n."""
    m = np.mod(idx, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m).astype(np.int32)


def resize_geometry(H: int, W: int, scale=None, output_shape=None):
    """((Ho, Wo), (scale_y, scale_x), rows_first) of a resize of an H x W plane.  Exactly one of `scale` (one float for both axes,
    output ceil(scale * n)) and `output_shape` = (Ho, Wo) (per-axis scale Ho / H, Wo / W); every per-axis scale in [1/8, 8].
    rows_first: the row pass runs first when its scale is not the larger one."""
    if (scale is None) == (output_shape is None):
        raise ValueError("exactly one of scale and output_shape must be given")
    if H < 1 or W < 1:
        raise ValueError(f"the last two axes must be non-empty, got {H} x {W}")
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
            raise ValueError(f"scale must be a number, got {scale!r}")
        sy = sx = float(scale)
        if not MIN_SCALE <= sy <= MAX_SCALE:                    # also refuses NaN
            raise ValueError(f"scale must lie in [1/8, 8], got {scale!r}")
        Ho, Wo = int(np.ceil(sy * H)), int(np.ceil(sx * W))
    else:
        try:
            Ho, Wo = (int(v) for v in output_shape)
            exact = (Ho, Wo) == tuple(output_shape)
        except (TypeError, ValueError):
            exact = False
        if not exact or Ho < 1 or Wo < 1:
            raise ValueError(f"output_shape must be two positive integers (Ho, Wo), got {output_shape!r}")
        sy, sx = 1.0 * Ho / H, 1.0 * Wo / W
        if not (MIN_SCALE <= sy <= MAX_SCALE and MIN_SCALE <= sx <= MAX_SCALE):
            raise ValueError(f"output_shape {(Ho, Wo)} of a {H} x {W} plane: per-axis scales {sy:.4g}, {sx:.4g} outside [1/8, 8]")
    return (Ho, Wo), (sy, sx), sy <= sx


def resize_taps(n_in: int, n_out: int, scale: float):
    """(weights f32 (n_out, P), first int32 (n_out,)): output o of the axis reads the inputs first[o] .. first[o] + P - 1 (not yet
    reflected) with weights[o].  The reference's arithmetic and dtypes: f32 output coordinates 1 .. n_out, u = x / scale +
    0.5 (1 - 1 / scale) in f32, first = floor(u - kw / 2) with kw = 4, or 4 / scale when scale < 1 (the antialiased kernel
    scale * cubic(scale * x)); the distance u - index - 1 is an f64 that the cubic rounds to f32; the cubic and the division by the
    f32 row sum are f32.  ceil(kw) + 2 taps are computed; the leading and trailing taps that are zero for every output are left
    out (the reference drops all-zero columns; an inner one would add an exact zero)."""
    scale = float(scale)
    if n_in < 1 or n_out < 1 or not MIN_SCALE <= scale <= MAX_SCALE:
        raise ValueError(f"resize_taps: n_in, n_out >= 1 and scale in [1/8, 8], got {n_in}, {n_out}, {scale!r}")
    kw = 4.0 / scale if scale < 1 else 4.0
    x = np.arange(1, n_out + 1).astype(np.float32)
    u = x / scale + 0.5 * (1 - 1 / scale)
    first = np.floor(u - kw / 2).astype(np.int32)
    taps = int(np.ceil(kw)) + 2
    index = first[:, None] + np.arange(taps, dtype=np.int32)
    dist = u[:, None] - index - 1                               # f32 - int32: f64
    t = np.abs((scale * dist if scale < 1 else dist).astype(np.float32))
    t2 = t * t
    t3 = t2 * t
    w = (1.5 * t3 - 2.5 * t2 + 1) * (t <= 1) + (-0.5 * t3 + 2.5 * t2 - 4 * t + 2) * ((1 < t) & (t <= 2))
    if scale < 1:
        w = scale * w
    w = w / np.sum(w, axis=1)[:, None]
    assert u.dtype == np.float32 and w.dtype == np.float32 and dist.dtype == np.float64
    used = np.flatnonzero(np.any(w, axis=0))
    lo, hi = int(used[0]), int(used[-1]) + 1
    return np.ascontiguousarray(w[:, lo:hi]), (first + lo).astype(np.int32)


def resize_tables(n_in: int, n_out: int, scale: float):
    """(weights f32 (n_out, P), index int32 (n_out, P)) of one axis: `resize_taps` with the P consecutive indices of every output
    reflected with edge repeat into 0 .. n_in - 1 (period 2 n_in).  P <= ceil(kw) + 2 <= 34."""
    w, first = resize_taps(n_in, n_out, scale)
    return w, _reflect(first[:, None].astype(np.int64) + np.arange(w.shape[1]), n_in)


def imresize_host(img: np.ndarray, scale=None, output_shape=None, out: str = "f32") -> np.ndarray:
    """MATLAB `imresize` (bicubic, a = -0.5, antialiased when it shrinks, symmetric border) of the last two axes of (..., H, W)
    uint8, uint16 (10-bit: a sample above 1023 reads as 1023) or f32 input, to `output_shape` = (Ho, Wo) or by `scale` (output
    ceil(scale * n)); exactly one of the two.  Two passes, the axis with the smaller scale first (rows on a tie), with the bits of
    the reference's MATLABLikeResize: every pass reads f32, every tap's product is an f32, products are added in tap order in f32.
    out="f32": f64 in which every value is an f32, neither clipped nor rounded.  out="int" (integer input only): clipped to
    [0, peak] (255 or 1023), rounded half to even, in the input's dtype, as `niqe.bicubic_upscale` defines it.  Per-axis scales
    lie in [1/8, 8]."""
    if out not in ("f32", "int"):
        raise ValueError(f'out must be "f32" or "int", got {out!r}')
    x = np.asarray(img)
    if x.ndim < 2 or 0 in x.shape[-2:]:
        raise ValueError(f"the last two axes must be non-empty, got shape {x.shape}")
    if x.dtype not in (np.uint8, np.uint16, np.float32):
        raise ValueError(f"img must be uint8, uint16 or f32, got {x.dtype}")
    peak = _INT_PEAK.get(x.dtype)
    if out == "int" and peak is None:
        raise ValueError(f'out="int" needs uint8 or uint16 input, got {x.dtype}')
    (Ho, Wo), scales, rows_first = resize_geometry(x.shape[-2], x.shape[-1], scale, output_shape)
    src_dtype = x.dtype
    if x.dtype == np.uint16:
        x = np.minimum(x, 1023)
    x = x.astype(np.float32)
    for axis in ((-2, -1) if rows_first else (-1, -2)):
        w, idx = resize_tables(x.shape[axis], (Ho, Wo)[axis], scales[axis])
        shape = (-1, 1) if axis == -2 else (-1,)
        acc = w[:, 0].reshape(shape) * np.take(x, idx[:, 0], axis=axis)
        for k in range(1, w.shape[1]):
            acc = acc + w[:, k].reshape(shape) * np.take(x, idx[:, k], axis=axis)
        x = acc
    assert x.dtype == np.float32
    if out == "int":
        return np.around(np.clip(x, 0, peak)).astype(src_dtype)
    return x.astype(np.float64)


def imresize(x: torch.Tensor, scale=None, output_shape=None, *, out: str = "f32") -> torch.Tensor:
    """x: (..., H, W) uint8, uint16 (10-bit samples) or f32 on the HIP device -> (..., Ho, Wo): `imresize_host` on the device, bit
    for bit, in one launch (fcvsr_imresize).  out="f32": f32; out="int" (integer x only): x's dtype, clipped and rounded half to
    even.  The tap tables of a size are made once per device and cached.  Non-contiguous x is made dense; an empty batch gives an
    empty result.  There is no CPU fallback: host tensors raise."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor")
    return hip.imresize(x, scale, output_shape, out)


def check_output_shape(output_shape, H: int, W: int, even: bool = False):
    """Validate the `output_shape=` of a harness entry point against the H x W frame it resizes: None passes through; otherwise
    (Ho, Wo) as plain ints, per-axis scale in [1/8, 8] (ValueError), both even when `even` (4:2:0 frames)."""
    if output_shape is None:
        return None
    (Ho, Wo), _, _ = resize_geometry(H, W, output_shape=output_shape)
    if even and (Ho % 2 or Wo % 2):
        raise ValueError(f"output_shape must be even on both axes for 4:2:0 frames, got {(Ho, Wo)}")
    return Ho, Wo
