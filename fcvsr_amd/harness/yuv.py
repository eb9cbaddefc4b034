"""Planar 8-bit and 10-bit YUV 4:2:0 (I420) sequences: reader, writer, the reference's file naming, and 4x super-resolution from
file to file (the test lists of reference CVSR_train/test_LD_freqCVSR_S_22.py:126-150 are raw sequences named ``Name_WxH_NF.yuv``).

Frame layout: Y (H x W), then U and V (H/2 x W/2 each), frames back to back; one byte per sample, or - ``bit_depth=10`` - two
bytes, little-endian, the 10-bit value in the low bits (the JVET / HM ``_10bit`` raw files).  Y is super-resolved by the model's
uint8 / uint16 path (windows of 7 frames, the reference's edge-replicate ``generate_input_index`` by default); U and V are
up-sampled 4x by the bicubic chroma kernel (``hip.chroma_up4``).  `upscale_yuv420` writes the bicubic baseline of a file (MATLAB
`imresize` on all three planes, no model): the "Bicubic" video to put next to the SR one.
"""
from __future__ import annotations

import contextlib
import os
import re
import time
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import hip
from .colour import ColourSpec, i420_planes, yuv420_to_rgb
from .shots import detect_cuts, resolve_cuts, windows_for
from .steps import (ScoreCollector, baseline_luma, check_keywords, check_reference, check_scores, deliver_luma, deliver_rgb,
                    group_boxes, pad_to_multiple, push_line_sums, run_stats, to_device)
from .surfaces import _check_size


class YuvName(NamedTuple):
    name: str               # everything before the _WxH token (e.g. "BasketballDrive_fps50")
    width: int
    height: int
    frames: Optional[int]   # the _NF token, None when the name carries none


_SIZE = re.compile(r"_(\d+)x(\d+)(?=_|\.|$)")
_FRAMES = re.compile(r"_(\d+)F(?=_|\.|$)")


def parse_yuv_name(path: str) -> YuvName:
    """``Traffic_640x400_300F.yuv`` -> YuvName("Traffic", 640, 400, 300); ``Kimono1_fps24_480x272_240F.yuv`` ->
    ("Kimono1_fps24", 480, 272, 240); ``Traffic_2560x1600_30.yuv`` (a frame rate, no frame count) -> (..., None)."""
    base = os.path.basename(path)
    stem = base[:-4] if base.lower().endswith(".yuv") else base
    m = _SIZE.search(stem)
    if m is None:
        raise ValueError(f"{base!r}: no _WxH size token (expected Name_WxH_NF.yuv)")
    f = _FRAMES.search(stem, m.end())
    return YuvName(stem[:m.start()], int(m.group(1)), int(m.group(2)), int(f.group(1)) if f else None)


_BIT10 = re.compile(r"_10bit(?=_|\.|$)", re.IGNORECASE)


def yuv_bit_depth(path: str) -> int:
    """10 when the file name carries a ``_10bit`` token (any letter case, e.g. ``MarketPlace_1920x1080_60fps_10bit_420.yuv``),
    else 8."""
    return 10 if _BIT10.search(os.path.basename(path)) else 8


def _sample_dtype(bit_depth: int):
    if bit_depth not in (8, 10):
        raise ValueError(f"bit_depth must be 8 or 10, got {bit_depth!r}")
    return np.dtype(np.uint8) if bit_depth == 8 else np.dtype("<u2")


def frame_bytes(width: int, height: int) -> int:
    _check_size(width, height)
    return width * height * 3 // 2


def _map_frames(path: str, width: int, height: int, frames: Optional[int] = None, bit_depth: int = 8) -> np.ndarray:
    """The (N, W*H*3/2) samples of an I420 file, one row per frame (``Y | U | V``): a read-only memory map."""
    dt = _sample_dtype(bit_depth)
    fs = frame_bytes(width, height)                     # samples per frame
    fb = fs * dt.itemsize
    size = os.path.getsize(path)
    if size % fb:
        raise ValueError(f"{path}: {size} bytes is not a whole number of {width}x{height} {bit_depth}-bit 4:2:0 frames "
                         f"({fb} bytes each)")
    n = size // fb
    if frames is not None:
        if frames < 0 or frames > n:
            raise ValueError(f"{path}: asked for {frames} frames, the file holds {n}")
        n = frames
    if n == 0:
        raise ValueError(f"{path}: no frames")
    return np.memmap(path, dtype=dt, mode="r", shape=(n, fs))


def read_yuv420(path: str, width: int, height: int, frames: Optional[int] = None,
                bit_depth: int = 8) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Y (N,H,W), U and V (N,H/2,W/2) uint8 arrays of an I420 file: strided views of one read-only memory map (nothing is
    copied).  `frames` reads the first N frames only.  ``bit_depth=10``: two bytes per sample, little-endian ``<u2`` views."""
    mm = _map_frames(path, width, height, frames, bit_depth)
    n = mm.shape[0]
    ys, cs = width * height, (width // 2) * (height // 2)
    y = mm[:, :ys].reshape(n, height, width)
    u = mm[:, ys:ys + cs].reshape(n, height // 2, width // 2)
    v = mm[:, ys + cs:].reshape(n, height // 2, width // 2)
    return y, u, v


def _write_frames(fh, y: np.ndarray, u: np.ndarray, v: np.ndarray):
    for i in range(y.shape[0]):
        for a in (y[i], u[i], v[i]):                      # uint16 planes go out little-endian whatever the host's byte order
            fh.write(np.ascontiguousarray(a if a.dtype.itemsize == 1 else a.astype("<u2", copy=False)).tobytes())


def _check_planes(y, u, v):
    y, u, v = (np.asarray(a) for a in (y, u, v))
    if any(a.dtype != np.uint8 for a in (y, u, v)) and any(a.dtype != np.uint16 for a in (y, u, v)):
        raise ValueError("planes must be all uint8 (8-bit 4:2:0) or all uint16 (10-bit 4:2:0)")
    if y.ndim == 2:
        y, u, v = y[None], u[None], v[None]
    if y.ndim != 3 or u.shape != v.shape or u.ndim != 3:
        raise ValueError(f"expected Y (N,H,W), U and V (N,H/2,W/2), got {y.shape}, {u.shape}, {v.shape}")
    n, h, w = y.shape
    _check_size(w, h)
    if u.shape != (n, h // 2, w // 2):
        raise ValueError(f"chroma planes must be (N,H/2,W/2) = {(n, h // 2, w // 2)}, got {u.shape}")
    return y, u, v


def write_yuv420(path: str, y: np.ndarray, u: np.ndarray, v: np.ndarray) -> None:
    """Write Y (N,H,W), U and V (N,H/2,W/2) uint8 planes (or single frames (H,W), (H/2,W/2)) as an I420 file; uint16 planes
    (10-bit samples) are written two bytes per sample, little-endian."""
    y, u, v = _check_planes(y, u, v)
    with open(path, "wb") as fh:
        _write_frames(fh, y, u, v)


def _map_reference(path: str, width: int, height: int, frames: int, bit_depth: int) -> np.ndarray:
    """The first `frames` frames of the ground-truth I420 file of ``reference=``, (frames, W*H*3/2) samples as a read-only memory
    map; ValueError when the file holds fewer whole frames (what follows them is never read)."""
    dt = _sample_dtype(bit_depth)
    fs = frame_bytes(width, height)
    have = os.path.getsize(path) // (fs * dt.itemsize)
    if have < frames:
        raise ValueError(f"{path}: the reference holds {have} whole {width}x{height} {bit_depth}-bit 4:2:0 frames, the source {frames}")
    return np.memmap(path, dtype=dt, mode="r", shape=(frames, fs))


def _reference_planes(g: np.ndarray, width: int, height: int, bit_depth: int, dev):
    """A group of mapped ground-truth frames on the device, laid out as `ReferenceCollector.score` takes them: Y (b,H,W) and the U
    planes followed by the V planes (2b,H/2,W/2)."""
    b, ys, cs = g.shape[0], width * height, (width // 2) * (height // 2)
    gy = to_device(g[:, :ys].reshape(b, height, width), bit_depth, dev)
    guv = to_device(np.concatenate([g[:, ys:ys + cs], g[:, ys + cs:]], 0).reshape(2 * b, height // 2, width // 2), bit_depth, dev)
    return gy, guv


def _open_dst(dst):
    """The destination file, or nothing to write to (``dst=None``: a scores-only run)."""
    return contextlib.nullcontext() if dst is None else open(dst, "wb")


def _check_niqe(niqe, bit_depth: int, width: int, height: int):
    """`steps.check_scores` of the `niqe=` keyword for width x height LR frames: the 4x frame is what is scored."""
    check_scores(niqe, None, bit_depth, 4 * height, 4 * width)


@torch.no_grad()
def super_resolve_yuv420(model, src: str, dst: str, width: int, height: int, *, batch: int = 8, padding: str = "replicate",
                         quantise: str = "truncate", num_frames: int = 7, bit_depth: int = 8,
                         ensemble: Optional[str] = None, niqe=None, brisque=None, cuts=None, cut_threshold: float = 10.0,
                         tile=None, tile_overlap=16, output_shape=None, active=None, static_tiles: bool = False,
                         reference: Optional[str] = None, crop_border: int = 4, tof: bool = False) -> dict:
    """Super-resolve the I420 sequence `src` (width x height) 4x into the I420 file `dst` (4 width x 4 height).

    `bit_depth` is 8 (one byte per sample, uint8) or 10 (two bytes per sample, uint16; `yuv_bit_depth` reads it off the file
    name), for both files.  Y: the frames go to the device once in their integer dtype, windows of `num_frames` frames (`padding`,
    as `super_resolve_sequence`) run through ``model.super_resolve_u8`` / ``super_resolve_u16`` in batches of `batch`, rows /
    columns padded to a multiple of 4 as the reference pads
    270 -> 272 and cropped off again.  U, V: ``hip.chroma_up4`` (bicubic) on both planes of a batch in one launch.  Frames are
    written in order as each batch completes.  Returns stats: frames, seconds, fps, bytes read and written.  No 10-bit
    output sample exceeds 1023.  ``ensemble`` (None, "spatial", "spatial+temporal": `harness.ensemble`) runs Y through the
    self-ensemble; chroma is unchanged.  ``niqe`` (a `harness.niqe.NiqeModel`) scores every SR luma frame with NIQE on the device
    before it is downloaded and adds ``"niqe"`` (per frame, f64) and ``"niqe_mean"`` to the stats; the written bytes are the same.
    NIQE is 8-bit only: ``bit_depth=10`` with ``niqe`` raises ValueError.  ``brisque`` (a `harness.brisque.BrisqueModel`) does the
    same with BRISQUE (``"brisque"``, ``"brisque_mean"``), 8-bit only as well; the two may be given together.  ``cuts``: None, a
    sequence of frame numbers at which a new shot starts, or "auto" (`shots.detect_cuts` with ``cut_threshold`` on the file's luma
    plane, on the device): every window then stays inside the shot of its centre frame (`shots.shot_window_indices`), and the list
    that was used is added to the stats as ``"cuts"``.  Chroma does not depend on it.  ``tile`` / ``tile_overlap`` as in
    `super_resolve_sequence` (`harness.tiles`): Y runs through the model in overlapping tiles, with ``ensemble`` every tile
    ensembled; chroma is unchanged.

    ``output_shape``: None, or (Ho, Wo), both even: the file is written at Wo x Ho in place of 4 width x 4 height.  The SR luma
    frames are resized on the device by `resize.imresize` (MATLAB `imresize`, out="int") before they are downloaded, as in
    `super_resolve_sequence`; U and V go ONCE from the LR chroma planes to (Ho/2, Wo/2) by the same function, in place of
    ``hip.chroma_up4``.  Ho / (4 height), Wo / (4 width) must lie in [1/8, 8] and the chroma step Ho / height, Wo / width in
    [1/8, 8] as well, so at most 2x beyond the 4x frame (ValueError before any model pass).  ``niqe`` / ``brisque`` score the 4x
    luma the model made, as without the keyword.  ``"out_size"`` is (Wo, Ho).

    ``active`` as in `super_resolve_sequence` (`harness.active`): None, a box (top, bottom, left, right) in luma samples, "auto" or
    an `ActiveSpec` (detection on the file's luma plane, on the device).  The model sees the active box of every window only; the
    luma outside it is the MATLAB-style bicubic up-scale of the LR frame, and ``niqe`` / ``brisque`` / ``output_shape`` act on the
    composed frame.  Chroma does not depend on it.  The (first frame, box) changes of the run are added to the stats as
    ``"active"``.

    ``static_tiles`` as in `super_resolve_sequence` (True needs ``tile``): tile windows that did not change inside a group are not
    run again; the file written is the same, and the stats gain ``"tiles_total"`` and ``"tiles_run"`` (tile windows delivered and
    run through the model).

    ``reference``: None, or the path of the ground-truth I420 file, of `bit_depth` and of the size that is written, with at least
    as many frames as `src` (ValueError before any model pass otherwise); it is mapped and uploaded group by group.  The planes
    that are written - Y, U and V after every other keyword - are scored against it on the device (`harness.reference` is the
    contract): the stats gain ``"sse"`` (int64 (N,3), exact), ``"psnr_y"``, ``"psnr_u"``, ``"psnr_v"``, ``"psnr_yuv"``, ``"ssim_y"``
    (f64 (N,)), their ``*_mean``, ``"psnr_{y,u,v,yuv}_global"`` and ``"reference_frames"``; the file written is the same.  Luma is
    cropped by ``crop_border`` (even; the reference's 4), chroma by half of it.  ``dst=None`` (needs ``reference``): nothing is
    downloaded or written, ``"bytes_written"`` is 0.  This function takes no ``baseline=`` (the "Bicubic" video of a file is
    `upscale_yuv420`'s); `harness.stream.stream_yuv420` scores the bicubic baseline next to the same numbers.

    ``tof=True`` (needs ``reference``, ValueError without): the stats gain ``"tof"`` (f64 (N,)), ``"tof_mean"`` and
    ``"tof_pairs_mean"``, the tOF of `harness.tof` of the delivered luma planes against the ground truth's, on the device: 0.0 at
    frame 0 and at every frame of ``cuts``, the last plane pair of a group carried to the next.  The file written is the same."""
    shape = _check_output_shape_420(output_shape, width, height)
    ref = check_reference(reference, dst, crop_border=crop_border, baseline=None, bit_depth=bit_depth, height=height,
                          width=width, out_shape=shape, tof=tof)
    brisque = check_scores(niqe, brisque, bit_depth, 4 * height, 4 * width)
    resolver = check_keywords(model, ensemble=ensemble, tile=tile, tile_overlap=tile_overlap, batch=batch, quantise=quantise,
                              cuts=cuts, frame_dtype="uint8", channels=(1,), who="super_resolve_yuv420", active=active,
                              frame_shape=(1, height, width), bit_depth=bit_depth, static_tiles=static_tiles)
    y, u, v = read_yuv420(src, width, height, bit_depth=bit_depth)
    N, H, W = y.shape
    Ho, Wo = (4 * H, 4 * W) if shape is None else shape
    gt = None if ref is None else _map_reference(reference, Wo, Ho, N, bit_depth)
    dev = next(model.parameters()).device
    t0 = time.perf_counter()
    x = to_device(y, bit_depth, dev)[:, None]                                             # (N,1,H,W)
    cuts = resolve_cuts(cuts, N, lambda: detect_cuts(x, threshold=cut_threshold))
    push_line_sums(resolver, x)
    x = pad_to_multiple(hip.bits16(x), resolver.multiple).view(x.dtype)                   # the resident frames, zero padded
    written, scores = 0, ScoreCollector(niqe, brisque)
    with _open_dst(dst) as fh:
        for s in range(0, N, batch):
            e = min(N, s + batch)
            idx = windows_for(range(s, e), num_frames, N, padding, cuts)
            sr = resolver.frames(x, idx, quantise, H, W, group_boxes(resolver, range(s, e), idx, N))          # (b,1,4H,4W)
            scores.add(scores.features(sr))
            uv = to_device(np.concatenate([u[s:e], v[s:e]], 0), bit_depth, dev)           # (2b, H/2, W/2)
            planes = deliver_luma(sr[:, 0], uv, shape)                                    # resized on the device
            if ref is not None:
                ref.add(ref.score(*planes, *_reference_planes(gt[s:e], Wo, Ho, bit_depth, dev),
                                  cuts=[c - s for c in cuts or () if s <= c < e]))
            if fh is not None:
                ysr, uvsr = (hip.frames_to_numpy(t) for t in planes)                      # downloaded
                _write_frames(fh, ysr, uvsr[:e - s], uvsr[e - s:])
                written += ysr.nbytes + uvsr.nbytes
    stats = scores.stats()
    return run_stats(N, time.perf_counter() - t0, N * frame_bytes(W, H) * (1 if bit_depth == 8 else 2), written, (Wo, Ho), stats,
                     cuts, resolver.boxes, resolver, ref)


def _check_output_shape_420(output_shape, width: int, height: int, chroma: bool = True):
    """The `output_shape=` of the SR entry points that write I420 files: None, or (Ho, Wo), both even, within [1/8, 8] of the 4x
    frame and - where the LR chroma planes are resized straight to (Ho/2, Wo/2) - within [1/8, 8] of the LR frame."""
    from .resize import check_output_shape
    shape = check_output_shape(output_shape, 4 * height, 4 * width, even=True)
    if shape is not None and chroma:
        check_output_shape(shape, height, width)
    return shape


@torch.no_grad()
def super_resolve_yuv420_rgb(model, src: str, dst: str, width: int, height: int, *, colour: ColourSpec = ColourSpec(),
                             batch: int = 8, padding: str = "replicate", quantise: str = "truncate", num_frames: int = 7,
                             ensemble: Optional[str] = None, niqe=None, brisque=None, cuts=None,
                             cut_threshold: float = 10.0, tile=None, tile_overlap=16, output_shape=None, active=None,
                             static_tiles: bool = False, reference: Optional[str] = None, crop_border: int = 4,
                             baseline: Optional[str] = None, tof: bool = False) -> dict:
    """Super-resolve the I420 sequence `src` (width x height) 4x into the I420 file `dst` (4 width x 4 height) with an RGB model
    (`FCVSRNet`, `FCVSR_SNet`).

    `colour` says how the stream maps to RGB (`harness.colour.ColourSpec`: matrix, range, chroma siting) and its bit depth, 8 or
    10, for both files.  The LR frames go to the device once, as the file holds them, and are decoded there to planar RGB by one
    launch (`harness.colour.yuv420_to_rgb`, reading the I420 frames in place); the RGB frames are zero-padded to a multiple of 4 as
    the Y path pads, windows of `num_frames` frames (`padding`, as `super_resolve_sequence`) run through
    ``model.super_resolve_u8`` / ``super_resolve_u16`` in batches of `batch`, and every batch of SR frames is cropped to
    4 height x 4 width, encoded on the device into I420 frame layout (`harness.colour.rgb_to_i420`), downloaded and written in
    order.  Returns the stats of `super_resolve_yuv420`.  ``ensemble`` (None, "spatial", "spatial+temporal") runs the decoded RGB
    frames through the self-ensemble (`harness.ensemble`) between the two colour conversions.  ``niqe`` as in
    `super_resolve_yuv420`: the Y of YCbCr of the SR RGB frames (convert_to="Y") is scored before the encode; 8-bit only.
    ``brisque`` as in `super_resolve_yuv420`: the YIQ luma of the SR RGB frames (BRISQUE's own "Y", not NIQE's) is scored before
    the encode; 8-bit only.  ``cuts`` / ``cut_threshold`` as in `super_resolve_yuv420`: "auto" detects on the luma plane of the file,
    before the colour conversion.  ``tile`` / ``tile_overlap`` as in `super_resolve_sequence` (`harness.tiles`): the decoded RGB
    frames run through the model in overlapping tiles between the two colour conversions.

    ``output_shape``: None, or (Ho, Wo), both even, Ho / (4 height) and Wo / (4 width) in [1/8, 8]: the SR RGB frames are resized
    plane by plane on the device (`resize.imresize`, out="int") before the encode, and the file is written at Wo x Ho.  ``niqe`` /
    ``brisque`` score the 4x frames, as without the keyword.

    ``active`` as in `super_resolve_yuv420`: "auto" detects on the luma plane of the file, before the colour conversion, and the
    same box is applied to the decoded RGB frames; outside it the frame is the bicubic up-scale of the decoded LR frame.

    ``static_tiles`` as in `super_resolve_sequence` (True needs ``tile``): tile windows that did not change inside a group are not
    run again; the file written is the same, and the stats gain ``"tiles_total"`` and ``"tiles_run"`` (tile windows delivered and
    run through the model).

    ``reference`` / ``crop_border`` / ``dst=None`` as in `super_resolve_yuv420`: the Y, U and V planes of the encoded frames are what
    is scored.  ``baseline="bicubic"`` (needs ``reference``) adds ``"baseline_psnr_y"`` / ``"baseline_ssim_y"`` and their means,
    without a model pass: `device_metrics.frame_metrics` of the luma of ``rgb_to_i420(imresize(decoded RGB LR frame, out="int"),
    colour)`` against the ground truth's.  ``tof=True`` as in `super_resolve_yuv420`, on the luma plane of the encoded frames; with
    ``baseline`` it adds ``"baseline_tof"``, ``"baseline_tof_mean"`` and ``"baseline_tof_pairs_mean"``."""
    shape = _check_output_shape_420(output_shape, width, height, chroma=False)
    bit_depth = colour.bit_depth if isinstance(colour, ColourSpec) else 8
    ref = check_reference(reference, dst, crop_border=crop_border, baseline=baseline, bit_depth=bit_depth, height=height,
                          width=width, out_shape=shape, tof=tof)
    brisque = check_scores(niqe, brisque, bit_depth, 4 * height, 4 * width)
    resolver = check_keywords(model, ensemble=ensemble, tile=tile, tile_overlap=tile_overlap, batch=batch, quantise=quantise,
                              cuts=cuts, frame_dtype="uint8", channels=(3,), who="super_resolve_yuv420_rgb", active=active,
                              frame_shape=(1, height, width), bit_depth=bit_depth, static_tiles=static_tiles)
    if not isinstance(colour, ColourSpec):
        raise ValueError(f"colour must be a ColourSpec, got {type(colour).__name__}")
    mm = _map_frames(src, width, height, bit_depth=bit_depth)
    N, H, W = mm.shape[0], height, width
    Ho, Wo = (4 * H, 4 * W) if shape is None else shape
    gt = None if ref is None else _map_reference(reference, Wo, Ho, N, bit_depth)
    dev = next(model.parameters()).device
    t0 = time.perf_counter()
    frames = to_device(mm, bit_depth, dev)                                                    # one host copy of the mapped file
    luma = lambda: hip.bits16(frames)[:, :H * W].reshape(N, 1, H, W).view(frames.dtype)       # the file's luma plane, made dense
    cuts = resolve_cuts(cuts, N, lambda: detect_cuts(luma(), threshold=cut_threshold))
    if resolver.boxes is not None and resolver.boxes.auto:
        push_line_sums(resolver, luma())
    x = yuv420_to_rgb(*i420_planes(frames, H, W), colour)                                     # (N,3,H,W)
    x = pad_to_multiple(hip.bits16(x), resolver.multiple).view(x.dtype)                       # the resident frames, zero padded
    written, scores = 0, ScoreCollector(niqe, brisque, "Y")
    with _open_dst(dst) as fh:
        for s in range(0, N, batch):
            idx = windows_for(range(s, min(N, s + batch)), num_frames, N, padding, cuts)
            e = s + len(idx)
            sr = resolver.frames(x, idx, quantise, H, W, group_boxes(resolver, range(s, e), idx, N))
            scores.add(scores.features(sr))
            out = deliver_rgb(sr, colour, shape)                                          # (b, Ho Wo 3/2)
            if ref is not None:
                ysr, usr, vsr = i420_planes(out, Ho, Wo)
                base = None if baseline is None else baseline_luma(hip.bits16(x)[s:e, :, :H, :W].view(x.dtype), shape, colour)
                ref.add(ref.score(ysr, torch.cat([hip.bits16(usr), hip.bits16(vsr)], 0),
                                  *_reference_planes(gt[s:e], Wo, Ho, bit_depth, dev), base,
                                  cuts=[c - s for c in cuts or () if s <= c < e]))
            if fh is not None:
                out = hip.frames_to_numpy(out)
                fh.write(np.ascontiguousarray(out if out.dtype.itemsize == 1 else out.astype("<u2", copy=False)).tobytes())
                written += out.nbytes
    stats = scores.stats()
    return run_stats(N, time.perf_counter() - t0, N * frame_bytes(W, H) * (1 if bit_depth == 8 else 2), written, (Wo, Ho), stats,
                     cuts, resolver.boxes, resolver, ref)


@torch.no_grad()
def upscale_yuv420(src: str, dst: str, width: int, height: int, *, factor: int = 4, bit_depth: int = 8, batch: int = 8,
                   device=None, output_shape=None) -> dict:
    """Write the bicubic baseline of the I420 sequence `src` (width x height) into the I420 file `dst` (factor width x factor
    height), `factor` 2 or 4: Y, U and V all go through `resize.bicubic_upscale(out="int")`, the MATLAB-style `imresize` (clipped to
    [0, peak], rounded half to even), on the device (`device`, default the current HIP device).  No model is involved.  `bit_depth`
    is 8 or 10 for both files, as in `super_resolve_yuv420`; frames are uploaded in their integer dtype, `batch` at a time, and
    written in order.  Returns the stats keys of `super_resolve_yuv420`.  No 10-bit output sample exceeds 1023.

    ``output_shape``: None, or (Ho, Wo), both even, Ho / height and Wo / width in [1/8, 8]: the file is written at Wo x Ho, Y through
    `resize.imresize(output_shape=(Ho, Wo), out="int")` and U, V to (Ho/2, Wo/2) - the bicubic baseline of any delivery size, 3x
    among them.  `factor` must then be left at its default (ValueError otherwise)."""
    from .resize import bicubic_upscale, check_output_shape, imresize
    if factor not in (2, 4):
        raise ValueError(f"factor must be 2 or 4, got {factor!r}")
    if output_shape is not None and factor != 4:
        raise ValueError(f"output_shape and factor cannot both be given (factor={factor!r})")
    shape = check_output_shape(output_shape, height, width, even=True)
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    y, u, v = read_yuv420(src, width, height, bit_depth=bit_depth)
    N, H, W = y.shape
    dev = torch.device("cuda" if device is None else device)

    def up(a, div=1):
        """Planes of the file through the kernel and back."""
        t = to_device(a, bit_depth, dev)
        if shape is not None:
            return hip.frames_to_numpy(imresize(t, output_shape=(shape[0] // div, shape[1] // div), out="int"))
        return hip.frames_to_numpy(bicubic_upscale(t, factor, out="int"))
    t0 = time.perf_counter()
    written = 0
    with open(dst, "wb") as fh:
        for s in range(0, N, batch):
            e = min(N, s + batch)
            ysr, uvsr = up(y[s:e]), up(np.concatenate([u[s:e], v[s:e]], 0), 2)           # (b, fH, fW), (2b, fH/2, fW/2)
            _write_frames(fh, ysr, uvsr[:e - s], uvsr[e - s:])
            written += ysr.nbytes + uvsr.nbytes
    return run_stats(N, time.perf_counter() - t0, N * frame_bytes(W, H) * (1 if bit_depth == 8 else 2), written,
                     (factor * W, factor * H) if shape is None else (shape[1], shape[0]))
