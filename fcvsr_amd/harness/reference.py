"""Full-reference scores of what a run writes, against a ground-truth video of the same size (``reference=``): the contract, as
numpy functions (host logic; the kernel `fcvsr_plane_sse` of csrc/plane_sse.hip is pinned to `plane_sse_host`).

What is scored are the integer planes of every delivered frame - Y (Ho,Wo), U and V (Ho/2,Wo/2), after every keyword that shapes
them - against the planes `surfaces.unpack_host` gives for the ground-truth frame of the same number; 10-bit samples read as
``min(k, 1023)`` on both sides.  The flow is the reference's evaluation (CVSR_train/test_LD_freqCVSR*.py, then metric/psnr_ssim.py
cal_psnr_ssim with crop_border=4): PSNR per plane from the exact integer sum of squared differences, by the very expression of
`metrics.psnr`, and SSIM of the luma plane (`metrics.ssim`).  Luma is cropped by `crop_border`, chroma by ``crop_border // 2``.

``psnr_yuv`` is the same expression on (sse_y + sse_u + sse_v) / (n_y + n_u + n_v): the "average" of ffmpeg's psnr filter, stated
here as a definition.  ``*_mean`` is the mean of the per-frame values, ``*_global`` comes from the sums over all frames; both are
exact functions of integers, so they do not depend on how the frames fell into groups.

This module needs numpy only.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

PEAKS = {8: 255, 10: 1023}
PLANES = ("y", "u", "v")
BASELINES = (None, "bicubic")
FRAME_KEYS = ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "ssim_y")          # per frame, f64 (N,); the columns of --scores-log


def check_crop(crop_border, height: int, width: int) -> int:
    """`crop_border` for height x width luma planes: an even integer >= 0 that leaves an SSIM region (the condition of
    `device_metrics.frame_metrics`: 11x11 window inside the cropped plane).  The chroma planes, cropped by half of it, are then not
    empty either."""
    if isinstance(crop_border, bool) or not isinstance(crop_border, (int, np.integer)) or crop_border < 0 or crop_border % 2:
        raise ValueError(f"crop_border must be an even integer >= 0 (chroma is cropped by half of it), got {crop_border!r}")
    if min(height, width) - 2 * crop_border - 10 < 1:
        raise ValueError(f"{height}x{width} frames leave no SSIM region with crop_border={crop_border} and the 11x11 window")
    return int(crop_border)


def plane_sizes(height: int, width: int, crop_border: int) -> Tuple[int, int, int]:
    """Samples of the cropped Y, U and V planes of a height x width 4:2:0 frame."""
    c2 = crop_border // 2
    n_y = (height - 2 * crop_border) * (width - 2 * crop_border)
    n_c = (height // 2 - 2 * c2) * (width // 2 - 2 * c2)
    return n_y, n_c, n_c


def read_samples(a) -> np.ndarray:
    """Integer planes as int64, uint16 samples (10-bit containers) read as min(k, 1023)."""
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"planes must be uint8 or uint16, got {a.dtype}")
    return np.minimum(a.astype(np.int64), 1023)


def plane_sse_host(a, b, crop: int = 0) -> np.ndarray:
    """a, b: (P,h,w) uint8 or uint16 planes -> int64 (P,), the exact sum of (a - b)^2 over [crop:h-crop, crop:w-crop]."""
    a, b = read_samples(a), read_samples(b)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError(f"expected two (P,h,w) arrays of one shape, got {a.shape}, {b.shape}")
    P, h, w = a.shape
    if crop < 0 or 2 * crop >= min(h, w):
        raise ValueError(f"crop must satisfy 0 <= 2 crop < min(h, w), got {crop} for {h}x{w}")
    d = a[:, crop:h - crop, crop:w - crop] - b[:, crop:h - crop, crop:w - crop]
    return (d * d).sum((1, 2), dtype=np.int64)


def _psnr(sse: int, n: int, peak: float) -> float:
    """`metrics.psnr` from the integer sum: np.mean of integer squares below 2^53 is sse / n rounded once."""
    mse = np.float64(int(sse)) / np.float64(int(n))
    if mse == 0:
        return float("inf")
    return float(20.0 * np.log10(float(peak) / np.sqrt(mse)))


def scores_from_sse(sse, sizes: Sequence[int], peak) -> dict:
    """sse: int64 (N,3), per frame the sums of the Y, U and V plane (`plane_sse_host`); sizes: the samples behind them
    (`plane_sizes`); peak: 255 or 1023.  Returns {"psnr_y", "psnr_u", "psnr_v", "psnr_yuv"}: f64 (N,), inf where the sum is 0; each
    per-plane value is bit-equal to ``metrics.psnr(plane_sr, plane_gt, crop, peak)``."""
    sse = np.asarray(sse)
    if sse.ndim != 2 or sse.shape[1] != 3 or sse.dtype.kind not in "iu":
        raise ValueError(f"sse must be an integer (N,3) array, got {sse.dtype} {sse.shape}")
    sizes = [int(n) for n in sizes]
    if len(sizes) != 3 or min(sizes) < 1:
        raise ValueError(f"sizes: three positive sample counts, got {sizes}")
    if peak not in (255, 1023):
        raise ValueError(f"peak must be 255 or 1023, got {peak!r}")
    out = {f"psnr_{p}": np.array([_psnr(s, sizes[k], peak) for s in sse[:, k]], dtype=np.float64) for k, p in enumerate(PLANES)}
    out["psnr_yuv"] = np.array([_psnr(int(r[0]) + int(r[1]) + int(r[2]), sum(sizes), peak) for r in sse], dtype=np.float64)
    return out


def sequence_scores(sse, ssim_y, sizes: Sequence[int], peak) -> dict:
    """The stats keys of ``reference=``: ``sse`` (int64 (N,3)), the per-frame ``psnr_*`` of `scores_from_sse` and ``ssim_y``, the
    ``*_mean`` of each, ``psnr_{y,u,v,yuv}_global`` from the sums over all frames, and ``reference_frames``."""
    sse = np.asarray(sse, dtype=np.int64).reshape(-1, 3)
    ssim_y = np.asarray(ssim_y, dtype=np.float64).reshape(-1)
    N = sse.shape[0]
    if ssim_y.shape[0] != N:
        raise ValueError(f"{N} frames of sums, {ssim_y.shape[0]} of SSIM")
    out = {"sse": sse, **scores_from_sse(sse, sizes, peak), "ssim_y": ssim_y}
    for k in FRAME_KEYS:
        out[k + "_mean"] = float(np.mean(out[k])) if N else float("nan")
    if N:
        total = [int(v) for v in sse.sum(0, dtype=np.int64)]
        glob = scores_from_sse(np.array([total], dtype=np.int64), [N * int(n) for n in sizes], peak)
        out.update({k + "_global": float(v[0]) for k, v in glob.items()})
    out["reference_frames"] = N
    return out


def check_reference(reference, dst_given: bool, crop_border, baseline, bit_depth: int, out_height: int, out_width: int,
                    reference_pix_fmt: Optional[str] = None) -> Optional[int]:
    """The ``reference=`` / ``crop_border=`` / ``baseline=`` / ``reference_pix_fmt=`` keywords and ``dst=None`` of a run that
    delivers `out_height` x `out_width` frames of `bit_depth` bits, before any device or file work.  Returns the validated crop
    border, or None without ``reference=`` (the other keywords must then be at their defaults, and a destination is needed)."""
    from . import surfaces
    if baseline not in BASELINES:
        raise ValueError(f'baseline must be None or "bicubic", got {baseline!r}')
    if reference is None:
        if baseline is not None:
            raise ValueError("baseline= compares against the ground truth: it needs reference=")
        if reference_pix_fmt is not None:
            raise ValueError("reference_pix_fmt= needs reference=")
        if not dst_given:
            raise ValueError("dst=None (scores only) needs reference=")
        return None
    if reference_pix_fmt is not None:
        surfaces.check_fmt(reference_pix_fmt)
        if surfaces.bit_depth(reference_pix_fmt) != bit_depth:
            raise ValueError(f"reference_pix_fmt {reference_pix_fmt!r} is {surfaces.bit_depth(reference_pix_fmt)}-bit, the run "
                             f"{bit_depth}-bit: the ground truth is compared at the delivered bit depth")
    if bit_depth not in PEAKS:
        raise ValueError(f"bit_depth must be 8 or 10, got {bit_depth!r}")
    return check_crop(crop_border, out_height, out_width)


def scores_csv(stats: dict) -> str:
    """One line per frame, ``frame,psnr_y,psnr_u,psnr_v,psnr_yuv,ssim_y``, from the stats of a run with ``reference=``; a run with
    ``tof=True`` has the further column ``tof``."""
    keys = FRAME_KEYS + (("tof",) if "tof" in stats else ())
    lines = ["frame," + ",".join(keys)]
    for i in range(int(stats["reference_frames"])):
        lines.append(f"{i}," + ",".join(repr(float(stats[k][i])) for k in keys))
    return "\n".join(lines) + "\n"
