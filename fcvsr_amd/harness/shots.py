"""Scene cuts: detection on integer frames and 7-frame windows that stay inside a shot (host logic; the contract the kernel
`fcvsr_frame_pair_sad` is pinned to).

The reference never meets a cut (its test clips are single shots), so this is a capability of this harness with its own
specification, like "spatial+temporal" in the ensemble.  `harness.windows.window_indices` knows only the ends of the sequence: at a
cut, three frames on each side get windows that mix two unrelated shots.  `shot_window_indices` builds the window inside the shot
that holds the centre frame; the `cuts=` keyword of the sequence entry points (`harness.infer`, `harness.yuv`) selects it.

The statistic is the mean absolute frame difference on a 0..100 scale,

    mafd[i] = float(sad[i]) * 100.0 / count / 2**bit_depth,      sad[i] = sum |f[i+1] - f[i]|,  count = C*H*W,

and the score of pair i is the smaller of mafd[i] and its change against the previous pair, clipped to [0, 100].  It has the form of
ffmpeg's `scdet` filter (the minimum of the difference and its change ignores fades and steady motion); bit equality with ffmpeg
is neither claimed nor tested.  The first pair has no predecessor and is compared with its successor instead: with a predecessor
of 0 a fast pan would register as a cut at frame 1.

Limits.  The default threshold 10.0 is `scdet`'s default on the same scale, a design default taken from there: nobody has validated it
on real footage in this project.  A shot of one or two frames hides the cut that ends it, because the change term is small there:
pass explicit cuts for such material.
"""
from __future__ import annotations

from bisect import bisect_right
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .windows import window_indices

PEAK10 = 1023


def _as_numpy(frames) -> np.ndarray:
    """Host integer frames as a numpy array; torch's uint16 goes through its int16 bits."""
    if isinstance(frames, np.ndarray):
        return frames
    import torch
    if isinstance(frames, torch.Tensor):
        if frames.dtype == torch.uint16:
            return frames.view(torch.int16).cpu().numpy().view(np.uint16)
        return frames.cpu().numpy()
    return np.asarray(frames)


def _bit_depth(dtype) -> int:
    """8 for uint8 frames, 10 for uint16 frames (numpy or torch dtype); ValueError for anything else."""
    name = str(dtype).replace("torch.", "")
    if name == "uint8":
        return 8
    if name == "uint16":
        return 10
    raise ValueError(f"scene-cut detection is defined on integer samples: frames must be uint8 or uint16, got {name} "
                     "(pass explicit cuts for float frames)")


def pair_sad_host(frames) -> np.ndarray:
    """frames: uint8 or uint16 (N,C,H,W).  Returns uint64 (N-1,): element i is the sum over all channels and pixels of
    |frames[i+1] - frames[i]| in exact integers.  uint16 samples are read as min(k, 1023), the input contract of
    `super_resolve_u16`."""
    f = _as_numpy(frames)
    _bit_depth(f.dtype)
    if f.ndim != 4 or f.shape[0] < 1:
        raise ValueError(f"expected (N,C,H,W) frames with N >= 1, got {f.shape}")
    def samples(i):
        a = f[i].astype(np.int32)
        return np.minimum(a, PEAK10) if f.dtype == np.uint16 else a

    out = np.zeros((f.shape[0] - 1,), dtype=np.uint64)
    prev = samples(0)
    for i in range(1, f.shape[0]):
        cur = samples(i)
        out[i - 1] = np.abs(cur - prev).sum(dtype=np.uint64)
        prev = cur
    return out


def scene_scores(sad, count: int, bit_depth: int) -> np.ndarray:
    """f64 scores (len(sad),) on the 0..100 scale from the pair sums `sad` of frames of `count` = C*H*W samples of `bit_depth` bits:
    score[i] = clip(min(mafd[i], |mafd[i] - mafd[i-1]|), 0, 100), the first pair against its successor, 0.0 when it is the only one."""
    sad = np.asarray(sad)
    mafd = sad.astype(np.float64) * 100.0 / count / 2 ** bit_depth
    n = mafd.shape[0]
    score = np.zeros((n,), dtype=np.float64)
    if n >= 2:
        change = np.abs(np.diff(mafd))                              # change[i-1] = |mafd[i] - mafd[i-1]|
        score[1:] = np.minimum(mafd[1:], change)
        score[0] = min(mafd[0], change[0])
    return np.clip(score, 0.0, 100.0)


def cuts_from_sad(sad, count: int, bit_depth: int, threshold: float = 10.0) -> List[int]:
    """The cuts of a sequence from its pair sums: sorted frame numbers i+1 with score[i] >= threshold."""
    score = scene_scores(sad, count, bit_depth)
    return [int(i) + 1 for i in np.nonzero(score >= threshold)[0]]


def device_pair_sad(frames) -> np.ndarray:
    """`pair_sad_host` of device frames by the kernel (`hip.frame_pair_sad`), fetched to the host: uint64 (N-1,).  Zero padding
    that all frames share adds nothing to the sums."""
    from ..hip import frame_pair_sad
    return frame_pair_sad(frames).cpu().numpy().astype(np.uint64)


def detect_cuts(frames, *, threshold: float = 10.0) -> List[int]:
    """Sorted frame numbers at which a new shot starts in the uint8 / uint16 (N,C,H,W) sequence `frames`: i+1 for every pair with
    score[i] >= threshold (module docstring).  Tensors on the HIP device go through the kernel, numpy arrays and host tensors
    through `pair_sad_host`; both give the same list.  Float frames raise ValueError: the statistic is defined on integer samples.

    threshold=10.0 is `scdet`'s default on the same 0..100 scale; it has NOT been validated on real footage in this project.  A shot
    of one or two frames hides the cut that ends it: pass explicit cuts for such material."""
    dtype = getattr(frames, "dtype", None)
    if dtype is None:
        frames = np.asarray(frames)
        dtype = frames.dtype
    bit_depth = _bit_depth(dtype)
    if len(frames.shape) != 4 or frames.shape[0] < 1:
        raise ValueError(f"expected (N,C,H,W) frames with N >= 1, got {tuple(frames.shape)}")
    count = int(frames.shape[1]) * int(frames.shape[2]) * int(frames.shape[3])
    sad = device_pair_sad(frames) if getattr(frames, "is_cuda", False) else pair_sad_host(frames)
    return cuts_from_sad(sad, count, bit_depth, threshold)


def shot_ranges(seq_len: int, cuts: Sequence[int]) -> List[Tuple[int, int]]:
    """[(a, b)] half-open frame ranges of the shots of a `seq_len`-frame sequence cut at `cuts` (each the first frame of a new
    shot).  `cuts` must be ints, strictly increasing, each in [1, seq_len-1]; anything else raises ValueError."""
    if isinstance(cuts, (str, bytes)) or not hasattr(cuts, "__iter__"):
        raise ValueError(f"cuts must be a sequence of frame numbers, got {cuts!r}")
    cuts = list(cuts)
    last = 0
    for c in cuts:
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError(f"cuts must be ints, got {c!r}")
        if not last < c <= seq_len - 1:
            raise ValueError(f"cuts must be strictly increasing frame numbers in [1, {seq_len - 1}], got {cuts!r}")
        last = int(c)
    edges = [0] + [int(c) for c in cuts] + [int(seq_len)]
    return list(zip(edges[:-1], edges[1:]))


def shot_window_indices(center: int, num_frames: int, seq_len: int, cuts: Sequence[int], padding: str = "replicate") -> List[int]:
    """`window_indices` inside the shot [a, b) that holds `center`: the window of centre - a in a sequence of b - a frames, every
    index clipped into [0, b-a-1] ("reflection" and "circle" index outside a shot shorter than the window), plus a.  With `cuts`
    empty this is `window_indices(center, num_frames, seq_len, padding)` for every padding mode: the clip is a no-op there, except in
    a sequence shorter than the window under "reflection" / "reflection_circle" / "circle", where `window_indices` itself leaves the
    sequence; without cuts its answer is returned as it is, so that ``cuts=[]`` and ``cuts=None`` never differ."""
    ranges = shot_ranges(seq_len, cuts)
    if len(ranges) == 1:
        return window_indices(center, num_frames, seq_len, padding)
    a, b = ranges[bisect_right([r[0] for r in ranges], center) - 1] if 0 <= center < seq_len else (0, seq_len)
    return [a + min(max(j, 0), b - a - 1) for j in window_indices(center - a, num_frames, b - a, padding)]


def check_auto(cuts, dtype) -> None:
    """The early refusal of the `cuts=` keyword, before any device is touched: a string other than "auto", or "auto" with frames
    that are not uint8 / uint16."""
    if isinstance(cuts, str):
        if cuts != "auto":
            raise ValueError(f'cuts must be None, a sequence of frame numbers or "auto", got {cuts!r}')
        _bit_depth(dtype)


def resolve_cuts(cuts, seq_len: int, detect=None) -> Optional[List[int]]:
    """The `cuts=` keyword as the list that is used: None stays None, "auto" calls `detect()`, a sequence is validated by
    `shot_ranges`."""
    if cuts is None:
        return None
    if isinstance(cuts, str):
        check_auto(cuts, "uint8")
        cuts = detect()
    shot_ranges(seq_len, cuts)
    return [int(c) for c in cuts]


def windows_for(centres, num_frames: int, seq_len: int, padding: str, cuts: Optional[Sequence[int]]) -> List[List[int]]:
    """The windows of `centres`: `window_indices` with cuts None (nothing changes), else `shot_window_indices`."""
    if cuts is None:
        return [window_indices(i, num_frames, seq_len, padding) for i in centres]
    return [shot_window_indices(i, num_frames, seq_len, cuts, padding) for i in centres]
