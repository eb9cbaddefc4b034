"""Letterbox-aware SR: where the picture is in a coded frame (host logic, numpy only; the contract the kernels
`fcvsr_frame_line_sums` and `fcvsr_active_compose` are pinned to).

Streaming video is often letterboxed (2.39:1 in a 16:9 frame) or pillarboxed (4:3 in 16:9).  The network is a whole-frame estimator
(README, "Tiled inference": MGAA and MFFR transform the frame, ContextBlock pools over it), so black bars change every output pixel
of the picture, and they cost what picture costs.  The ``active=`` keyword of the sequence entry points (`harness.infer`,
`harness.yuv`, `harness.stream`) lets the model - or whatever resolver ``ensemble=`` / ``tile=`` select - see the active box only; the
4x frame outside the box is the MATLAB-style bicubic up-scale of the LR centre frame, so a wrong detection degrades that region to
the bicubic baseline instead of losing it.  The reference has no counterpart (its clips carry no bars): this is a capability of this
harness with its own specification, like `harness.shots`.

The statistic is the sum of every row and every column of a frame over all channels, in exact integers (`line_sums_host`).  Row r is
picture iff

    float(rows[r]) > limit * 2.0 ** (bit_depth - 8) * (C * W)            (f64, in this order),

i.e. its mean sample lies above `limit` on the 8-bit scale; columns the same with C * H, over the full height.  The box of a frame
(`frame_box`) runs from the first to the last picture row and column, half-open (top, bottom, left, right).  The rule is the one of
ffmpeg's `cropdetect`; bit equality with ffmpeg is neither claimed nor tested.

The box only grows: `ActiveBoxes.upto(n)` is the union of the boxes of frames 0 .. n and never resets (a subtitle or a logo in a bar
enlarges it; there is no reset at cuts).  The box of a window is the one of the last frame it names (`window_box`), which is causal:
the whole-file functions and the stream apply the same rule and write the same bytes.  `used_box` aligns the union outward and falls
back to the whole frame where the detection is not to be trusted.

Limits.  The default limit 24.0 is `cropdetect`'s default on the same scale, a design default taken from there: nobody has validated it
on real footage in this project, and the effect of the keyword on quality is not measured either (there are no trained weights here).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .shots import PEAK10, _as_numpy, _bit_depth

Box = Tuple[int, int, int, int]                 # (top, bottom, left, right), half-open


@dataclass(frozen=True)
class ActiveSpec:
    """How ``active="auto"`` detects: `limit`, the mean sample (8-bit scale) a row or column must exceed to count as picture;
    `align`, the grid the box is widened to; `min_side`, the smallest box side that is believed (below it the whole frame is
    used)."""
    limit: float = 24.0
    align: int = 4
    min_side: int = 32

    def __post_init__(self):
        if isinstance(self.limit, bool) or not isinstance(self.limit, (int, float)) or not self.limit >= 0:
            raise ValueError(f"limit must be a number >= 0, got {self.limit!r}")
        for name in ("align", "min_side"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, got {v!r}")


def line_sums_host(frames) -> Tuple[np.ndarray, np.ndarray]:
    """frames: uint8 or uint16 (N,C,H,W).  Returns uint64 (rows (N,H), cols (N,W)): the sum of every row / column over all channels
    and the other axis, in exact integers.  uint16 samples are read as min(k, 1023), the contract of `shots.pair_sad_host`."""
    f = _as_numpy(frames)
    _bit_depth(f.dtype)
    if f.ndim != 4 or 0 in f.shape:
        raise ValueError(f"expected non-empty (N,C,H,W) frames, got {f.shape}")
    rows = np.zeros((f.shape[0], f.shape[2]), dtype=np.uint64)
    cols = np.zeros((f.shape[0], f.shape[3]), dtype=np.uint64)
    for i in range(f.shape[0]):
        a = np.minimum(f[i], PEAK10) if f.dtype == np.uint16 else f[i]
        rows[i] = a.sum(axis=(0, 2), dtype=np.uint64)
        cols[i] = a.sum(axis=(0, 1), dtype=np.uint64)
    return rows, cols


def frame_box(rows, cols, C: int, H: int, W: int, bit_depth: int, spec: ActiveSpec = ActiveSpec()) -> Optional[Box]:
    """The box of one frame from its line sums `rows` (H,) and `cols` (W,): first to last picture row and column (module docstring),
    None when there is no picture row or no picture column."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    if rows.shape != (H,) or cols.shape != (W,):
        raise ValueError(f"expected rows ({H},) and cols ({W},), got {rows.shape} and {cols.shape}")
    scale = spec.limit * 2.0 ** (bit_depth - 8)
    r = np.nonzero(rows.astype(np.float64) > scale * (C * W))[0]
    c = np.nonzero(cols.astype(np.float64) > scale * (C * H))[0]
    if r.size == 0 or c.size == 0:
        return None
    return int(r[0]), int(r[-1]) + 1, int(c[0]), int(c[-1]) + 1


def _union(a: Optional[Box], b: Optional[Box]) -> Optional[Box]:
    if a is None or b is None:
        return b if a is None else a
    return min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3])


class ActiveBoxes:
    """`frame_box` of a sequence, a chunk of line sums at a time (as `stream.AutoCuts` takes pair sums): `push(rows, cols)` adds the
    frames of a chunk, `upto(n)` is the union of the boxes of frames 0 .. n (None while no frame had picture).  It only grows."""

    def __init__(self, C: int, H: int, W: int, bit_depth: int, spec: ActiveSpec = ActiveSpec()):
        self.C, self.H, self.W, self.bit_depth, self.spec = int(C), int(H), int(W), int(bit_depth), spec
        self._unions: List[Optional[Box]] = []

    @property
    def frames(self) -> int:
        return len(self._unions)

    def push(self, rows, cols) -> None:
        rows, cols = np.asarray(rows), np.asarray(cols)
        if rows.ndim != 2 or cols.ndim != 2 or rows.shape[0] != cols.shape[0]:
            raise ValueError(f"expected rows (n,H) and cols (n,W), got {rows.shape} and {cols.shape}")
        for r, c in zip(rows, cols):
            last = self._unions[-1] if self._unions else None
            self._unions.append(_union(last, frame_box(r, c, self.C, self.H, self.W, self.bit_depth, self.spec)))

    def upto(self, n: int) -> Optional[Box]:
        if not 0 <= n < len(self._unions):
            raise ValueError(f"upto({n}): {len(self._unions)} frames have been pushed")
        return self._unions[n]


def used_box(box: Optional[Box], H: int, W: int, spec: ActiveSpec = ActiveSpec()) -> Box:
    """The box the model sees: `box` aligned outward to `spec.align` (top / left down, bottom / right up, clipped to the frame); the
    whole frame when `box` is None or a side of the aligned box is below `spec.min_side` - the detection is not trusted then."""
    if box is None:
        return 0, H, 0, W
    a = int(spec.align)
    t, l = (box[0] // a) * a, (box[2] // a) * a
    b, r = min(H, -(-box[1] // a) * a), min(W, -(-box[3] // a) * a)
    if b - t < spec.min_side or r - l < spec.min_side:
        return 0, H, 0, W
    return t, b, l, r


def check_active(active, dtype, H: int, W: int):
    """The early refusal of the ``active=`` keyword, before any device is touched, and its normal form: None (no keyword), an
    `ActiveSpec` ("auto" is `ActiveSpec()`; it needs uint8 / uint16 frames, as ``cuts="auto"`` does), or the explicit box
    (top, bottom, left, right): ints with 0 <= top < bottom <= H, 0 <= left < right <= W.  ValueError otherwise."""
    if active is None:
        return None
    if isinstance(active, str) or isinstance(active, ActiveSpec):
        if isinstance(active, str) and active != "auto":
            raise ValueError(f'active must be None, "auto", an ActiveSpec or a box (top, bottom, left, right), got {active!r}')
        try:
            _bit_depth(dtype)
        except ValueError:
            raise ValueError(f'active="auto" is defined on integer samples: frames must be uint8 or uint16, got {dtype} '
                             "(pass an explicit box for float frames)") from None
        return ActiveSpec() if isinstance(active, str) else active
    try:
        box = tuple(active)
    except TypeError:
        raise ValueError(f'active must be None, "auto", an ActiveSpec or a box (top, bottom, left, right), got {active!r}') from None
    if len(box) != 4 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in box):
        raise ValueError(f"active: a box is four ints (top, bottom, left, right), got {active!r}")
    t, b, l, r = (int(v) for v in box)
    if not (0 <= t < b <= H and 0 <= l < r <= W):
        raise ValueError(f"active: the box needs 0 <= top < bottom <= {H} and 0 <= left < right <= {W}, got {(t, b, l, r)}")
    return t, b, l, r


def window_box(boxes: ActiveBoxes, window: Sequence[int], seq_len: Optional[int] = None) -> Box:
    """The window rule: the used box of a centre frame is ``used_box(boxes.upto(max(window)))``, `window` the frame numbers of its
    window (a number below 0 counts from the end of the `seq_len` frames, as ``x[j]`` reads it)."""
    last = max(int(j) if j >= 0 else int(j) + int(seq_len) for j in window)
    return used_box(boxes.upto(last), boxes.H, boxes.W, boxes.spec)


def split_runs(boxes: Sequence[Box]) -> List[Tuple[int, int, Box]]:
    """[(first, end, box)]: the consecutive runs of one box in the boxes of a group's rows."""
    runs: List[Tuple[int, int, Box]] = []
    for i, b in enumerate(boxes):
        b = tuple(int(v) for v in b)
        if runs and runs[-1][2] == b:
            runs[-1] = (runs[-1][0], i + 1, b)
        else:
            runs.append((i, i + 1, b))
    return runs


class ActivePlan:
    """The ``active=`` keyword of one run, for H x W frames of C channels: the explicit box, or an `ActiveBoxes` that the entry point
    feeds with line sums (`auto`, `push`).  `group(centres, windows, seq_len)` gives the box of every row of a group and records
    where the box changes: `changes` is the list of (first centre frame, box) the stats report."""

    def __init__(self, active, C: int, H: int, W: int, bit_depth: int = 8):
        self.H, self.W = int(H), int(W)
        self.box = None if isinstance(active, ActiveSpec) else tuple(active)
        self.boxes = ActiveBoxes(C, H, W, bit_depth, active) if self.box is None else None
        self.changes: List[Tuple[int, Box]] = []

    @property
    def auto(self) -> bool:
        return self.box is None

    def push(self, rows, cols) -> None:
        self.boxes.push(rows, cols)

    def group(self, centres: Sequence[int], windows: Sequence[Sequence[int]], seq_len: Optional[int] = None) -> List[Box]:
        out = [self.box if self.box is not None else window_box(self.boxes, w, seq_len) for w in windows]
        for c, b in zip(centres, out):
            if not self.changes or self.changes[-1][1] != b:
                self.changes.append((int(c), b))
        return out


def compose_host(sr_box: np.ndarray, lr_centre: np.ndarray, box: Box) -> np.ndarray:
    """The 4x frames of a model pass that saw `box` only.  `lr_centre`: (..., H, W) LR centre frames, unpadded (the border rule sees the
    true edge, as in ``baseline="bicubic"``), uint8, uint16 or f32; `sr_box`: (..., 4 (bottom - top), 4 (right - left)) frames of the
    same dtype.  The result is `niqe.bicubic_upscale(lr_centre, 4, out="int")` - for f32 frames the f32 result, which is quantised
    later as the SR frames are - with ``[..., 4 top : 4 bottom, 4 left : 4 right]`` replaced by `sr_box`."""
    from .niqe import bicubic_upscale
    lr, sr = np.asarray(lr_centre), np.asarray(sr_box)
    t, b, l, r = (int(v) for v in box)
    H, W = lr.shape[-2:]
    if not (0 <= t < b <= H and 0 <= l < r <= W):
        raise ValueError(f"box {(t, b, l, r)} must lie in the {H}x{W} frame")
    if sr.shape != (*lr.shape[:-2], 4 * (b - t), 4 * (r - l)) or sr.dtype != lr.dtype:
        raise ValueError(f"sr_box must be {lr.dtype} {(*lr.shape[:-2], 4 * (b - t), 4 * (r - l))}, got {sr.dtype} {sr.shape}")
    if lr.dtype == np.float32:
        out = bicubic_upscale(lr, 4, out="f32").astype(np.float32)
    else:
        out = bicubic_upscale(lr, 4, out="int")
    out[..., 4 * t:4 * b, 4 * l:4 * r] = sr
    return out

