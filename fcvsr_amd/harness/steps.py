"""The steps every harness entry point shares, each written once: `check_keywords` (the keyword prologue; it returns the resolver),
`Resolver` (what a batch of windows runs through: `PlainResolver` here, `ensemble.SelfEnsemble`, `tiles.TiledSuperResolver`, and
`ActiveResolver`, which wraps one of them for ``active=``),
`check_scores` / `ScoreCollector` (``niqe=`` / ``brisque=``), `check_reference` / `ReferenceCollector` (``reference=``),
`deliver_luma` / `deliver_rgb` (SR frames to the planes a file holds) and `run_stats`.  `harness.infer`, `harness.yuv` and `harness.stream` are loops around them; a new keyword goes into the step it
belongs to, not into the loops.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import hip
from . import brisque as brisque_mod
from . import niqe as niqe_mod
from .shots import check_auto

INT_FRAMES = (torch.uint8, torch.uint16)


def pad_to_multiple(frames: torch.Tensor, mult: int = 4) -> torch.Tensor:
    """(N,C,H,W) -> zero-padded at the bottom/right so that H, W are multiples of `mult`."""
    H, W = frames.shape[-2:]
    ph, pw = (-H) % mult, (-W) % mult
    if ph == 0 and pw == 0:
        return frames
    return torch.nn.functional.pad(frames, (0, pw, 0, ph))


def to_device(a, bit_depth: int, dev) -> torch.Tensor:
    """Samples of a file (any array of them; a copy is made, a file map is read-only) on the device as uint8 / uint16: uint16
    samples travel as int16 bits (`hip.bits16`)."""
    host_dt, sdt = (np.uint8, torch.uint8) if bit_depth == 8 else (np.uint16, torch.uint16)
    return hip.bits16(torch.from_numpy(np.array(a, dtype=host_dt))).to(dev).view(sdt)


# ---- resolvers -----------------------------------------------------------------------------------------------------------------

class Resolver:
    """What the harness runs a batch of windows through.  The contract is ``sequence(frames, idx, *, dtype=torch.float32,
    quantise=None)``: `frames` the resident sequence (N,C,h,w) on the model's device - f32 in [0,1], uint8 or uint16 (10-bit
    samples), zero-padded once at the bottom / right to a multiple of `multiple` (`pad_to_multiple`) -, `idx` b rows of T frame
    numbers; it returns (b,C,>=4h,>=4w): f32, or - `dtype` uint8 / uint16 with `quantise` - quantised as
    ``model.super_resolve_u8`` / ``_u16`` quantise.  `frames` is the group step of the entry points around it; the window forms
    (`__call__`, `super_resolve_u8`, `super_resolve_u16`) are for direct users."""
    multiple = 1
    boxes = None                               # the `active.ActivePlan` of an `ActiveResolver`; None: the model sees whole frames

    def frames(self, x: torch.Tensor, idx, quantise: str, H: int, W: int, boxes=None) -> torch.Tensor:
        """One group of windows of the resident x, cropped (a view) to the 4H x 4W of the unpadded frame: integer x gives quantised
        frames of its dtype, float x the f32 frames (the caller quantises them: `infer._quantised_dev`, or the metric kernels).
        `boxes`: the active box of every row, for an `ActiveResolver` only (`group_boxes`)."""
        sr = self.sequence(x, idx, dtype=x.dtype, quantise=quantise) if x.dtype in INT_FRAMES else self.sequence(x, idx)
        return sr[..., :4 * H, :4 * W]

    def _rows(self, frames, idx, dtype, quantise):
        """The `frames` / `idx` / `quantise` checks of the resolvers that run kernels on them; the index rows as lists."""
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise ValueError(f"expected (N,C,h,w) frames, got {tuple(getattr(frames, 'shape', ()))}")
        if not frames.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the HIP device only (there is no CPU fallback)")
        if dtype in INT_FRAMES and quantise not in hip.QUANTISE:
            raise ValueError(f'quantise must be "truncate" or "round", got {quantise!r}')
        rows = [[int(j) for j in r] for r in idx]
        N = frames.shape[0]
        if not rows or any(len(r) != len(rows[0]) or not r for r in rows) or any(not 0 <= j < N for r in rows for j in r):
            raise ValueError(f"idx: rows of equal length with frame numbers in 0..{N - 1}, got {rows}")
        return rows

    def _window(self, win: torch.Tensor, **kw) -> torch.Tensor:
        if not isinstance(win, torch.Tensor) or win.dim() != 5:
            raise ValueError(f"expected a (B,T,C,H,W) window, got {tuple(getattr(win, 'shape', ()))}")
        B, T = win.shape[:2]
        frames = hip.bits16(win).reshape(B * T, *win.shape[2:]).view(win.dtype)
        return self.sequence(frames, np.arange(B * T).reshape(B, T).tolist(), **kw)

    def __call__(self, win: torch.Tensor, **kw) -> torch.Tensor:
        return self._window(win, **kw)

    def super_resolve_u8(self, win: torch.Tensor, quantise: str = "truncate", **kw) -> torch.Tensor:
        """uint8 (B,T,C,H,W) window -> uint8 (B,C,4H,4W): ``q(clamp(self(win), 0, 1) * 255)``, q as ``model.super_resolve_u8``."""
        if not isinstance(win, torch.Tensor) or win.dtype != torch.uint8:
            raise ValueError(f"expected a uint8 tensor, got {getattr(win, 'dtype', type(win))}")
        return self._window(win, dtype=torch.uint8, quantise=quantise, **kw)

    def super_resolve_u16(self, win: torch.Tensor, quantise: str = "truncate", **kw) -> torch.Tensor:
        """uint16 (B,T,C,H,W) window of 10-bit samples -> uint16 (B,C,4H,4W) in [0, 1023], as ``model.super_resolve_u16``."""
        if not isinstance(win, torch.Tensor) or win.dtype != torch.uint16:
            raise ValueError(f"expected a uint16 tensor, got {getattr(win, 'dtype', type(win))}")
        return self._window(win, dtype=torch.uint16, quantise=quantise, **kw)


def super_resolve_int(model, win: torch.Tensor, quantise: str) -> torch.Tensor:
    """The model's integer path for a uint8 or uint16 window."""
    return model.super_resolve_u16(win, quantise) if win.dtype == torch.uint16 else model.super_resolve_u8(win, quantise)


def run_window(model, win: torch.Tensor, quantise: Optional[str] = None) -> torch.Tensor:
    """The model on a (b,T,C,Hp,Wp) window that exists: integer windows take its integer path (quantised by the last kernel), float
    windows its ``forward``."""
    return super_resolve_int(model, win, quantise) if win.dtype in INT_FRAMES else model(win)


class PlainResolver(Resolver):
    """The model itself: whole frames, one pass.  The resident frames carry the zero padding to a multiple of 4 (the reference
    pads 270 -> 272), so a window is a stack of rows and nothing is padded per batch; the output keeps the padding (4x), which
    `Resolver.frames` crops by view.  Integer frames take ``model.super_resolve_u8`` / ``_u16`` - the last kernel quantises -, float
    frames ``model(win)``; it runs wherever the model runs.  Index rows are used as ``x[j]`` uses them: a number below 0 counts from
    the end (a sequence shorter than its window)."""
    multiple = 4

    def __init__(self, model):
        self.model = model

    def sequence(self, frames: torch.Tensor, idx: Sequence[Sequence[int]], *, dtype: torch.dtype = torch.float32,
                 quantise: Optional[str] = None) -> torch.Tensor:
        xb = hip.bits16(frames)                                                   # no checks: negative numbers are meant
        return run_window(self.model, torch.stack([xb[j] for j in idx], 0).view(frames.dtype), quantise)   # (b, T, C, Hp, Wp)

    def _window(self, win: torch.Tensor, dtype=None, quantise: Optional[str] = None) -> torch.Tensor:
        return run_window(self.model, win, quantise)


class ActiveResolver(Resolver):
    """Another resolver on the active box of every window (``active=``, `harness.active`): a resolver that wraps a resolver.  Per
    run of rows with one box it takes the box out of the resident frames - of the frames the rows name, nothing else -, pads it to
    `inner.multiple` as `pad_to_multiple` pads a frame, runs `inner.frames` at the box size and composes the 4x frames
    (`hip.active_compose`): the inner result inside the box, the MATLAB-style bicubic up-scale of the LR centre frame (the middle of
    a row) outside it.  The resident frames carry no padding (`multiple` 1).  A box equal to the whole frame gives what `inner`
    gives on the whole frame, bit for bit.  `boxes`: the `active.ActivePlan` of the run; the caller asks it for the boxes of a
    group's rows (`group_boxes`) - the rows themselves may be ring slots - and hands them to `frames`."""
    multiple = 1

    def __init__(self, inner: Resolver, boxes):
        self.inner, self.boxes = inner, boxes

    def frames(self, x: torch.Tensor, idx, quantise: str, H: int, W: int, boxes=None) -> torch.Tensor:
        from .active import split_runs
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_cuda:
            raise RuntimeError("ActiveResolver runs on (N,C,H,W) frames on the HIP device only (there is no CPU fallback)")
        rows = [[int(j) for j in r] for r in idx]                     # a number below 0 counts from the end, as ``x[j]`` reads it
        if boxes is None or len(boxes) != len(rows):
            raise ValueError(f"ActiveResolver.frames needs the box of each of its {len(rows)} rows, got {boxes!r}")
        xb, N = hip.bits16(x), x.shape[0]
        out = []
        for s, e, box in split_runs(boxes):
            t, b, l, r = box
            run = [[j % N for j in row] for row in rows[s:e]]
            named = sorted({j for row in run for j in row})
            pos = {j: k for k, j in enumerate(named)}
            crop = xb[:, :, t:b, l:r].index_select(0, torch.tensor(named, dtype=torch.int64).to(x.device))    # dense: the box only
            crop = pad_to_multiple(crop, self.inner.multiple).view(x.dtype)
            sr = self.inner.frames(crop, [[pos[j] for j in row] for row in run], quantise, b - t, r - l)
            if (t, b, l, r) == (0, H, 0, W):
                out.append(sr)                                        # nothing lies outside the box
            else:
                out.append(hip.active_compose(sr, x, [row[len(row) // 2] for row in run], box, H, W))
        return out[0] if len(out) == 1 else torch.cat([hip.bits16(o) for o in out], 0).view(out[0].dtype)

    def sequence(self, frames: torch.Tensor, idx, *, dtype: torch.dtype = torch.float32, quantise: Optional[str] = None,
                 boxes=None) -> torch.Tensor:
        """The `Resolver` contract on unpadded frames; `boxes` may be left out where the run has one explicit box."""
        rows = self._rows(frames, idx, dtype, quantise)
        if boxes is None and self.boxes is not None and not self.boxes.auto:
            boxes = [self.boxes.box] * len(rows)
        return self.frames(frames, rows, quantise, *frames.shape[-2:], boxes=boxes)


def group_boxes(resolver: Resolver, centres, windows, seq_len=None):
    """The ``boxes=`` of `Resolver.frames` for one group: the active box of every row from the frame numbers of its window
    (`active.ActivePlan.group`; a number below 0 counts from the end of `seq_len` frames), None without ``active=``."""
    return None if resolver.boxes is None else resolver.boxes.group(centres, windows, seq_len)


def push_line_sums(resolver: Resolver, frames: torch.Tensor) -> None:
    """``active="auto"``: the line sums of the integer (n,C,H,W) device frames (`hip.frame_line_sums`, one small download) into the
    run's `active.ActivePlan`.  Nothing happens without the keyword or with an explicit box."""
    if resolver.boxes is not None and resolver.boxes.auto:
        rows, cols = hip.frame_line_sums(frames)
        resolver.boxes.push(rows.cpu().numpy(), cols.cpu().numpy())


# ---- the keyword prologue ------------------------------------------------------------------------------------------------------

_CHANNELS = {1: "one-channel (Y)", 3: "three-channel (RGB)"}


def check_keywords(model, *, ensemble, tile, tile_overlap, batch, quantise, cuts, frame_dtype, channels=None, who="",
                   active=None, frame_shape=None, bit_depth=None, static_tiles=False) -> Resolver:
    """What every entry point validates before any device or file work - ``ensemble``, ``cuts`` ("auto" needs integer frames:
    `frame_dtype`), the model's channel count where the entry point `who` needs one of `channels`, ``quantise``, ``batch``,
    ``tile`` / ``tile_overlap`` / ``static_tiles`` (True needs ``tile``), ``active`` (against `frame_dtype` and `frame_shape` =
    (C, H, W) of the planes "auto" detects on, of `bit_depth` bits where the dtype does not say it) - and the resolver of these values (`tiles.resolver_for`, inside an
    `ActiveResolver` with ``active``).  ValueError names the keyword."""
    from .active import ActivePlan, check_active
    from .ensemble import check_mode
    from .tiles import resolver_for
    check_mode(ensemble)
    check_auto(cuts, frame_dtype)
    if channels is not None and getattr(model, "_img_ch", None) not in channels:
        raise ValueError(f"{who} needs a {' or '.join(_CHANNELS[c] for c in channels)} model, got C={getattr(model, '_img_ch', None)}")
    if quantise not in hip.QUANTISE:
        raise ValueError(f'quantise must be "truncate" or "round", got {quantise!r}')
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    if active is not None:
        C, H, W = frame_shape
        active = check_active(active, frame_dtype, H, W)
    resolver = resolver_for(model, ensemble, tile, tile_overlap, batch, static_tiles)
    if active is None:
        return resolver
    if bit_depth is None:
        bit_depth = 10 if str(frame_dtype).replace("torch.", "") == "uint16" else 8
    return ActiveResolver(resolver, ActivePlan(active, C, H, W, bit_depth))


def check_scores(niqe, brisque, bit_depth: int, height: int, width: int):
    """The ``niqe=`` / ``brisque=`` keywords against the bit depth of the run and the height x width of the scored frames, before
    anything is read: both scores are 8-bit only, NIQE needs >= 2 blocks, BRISQUE a `BrisqueModel` and even sides >= 16.  Returns
    the validated BRISQUE model (None for None)."""
    if niqe is not None:
        if bit_depth != 8:
            raise ValueError("NIQE is defined on 8-bit frames: niqe= cannot be used with 10-bit (uint16) frames")
        niqe_mod.crop_geometry(height, width, 0)
    if brisque is not None:
        brisque = brisque_mod._check_model(brisque)
        if bit_depth != 8:
            raise ValueError("BRISQUE is defined on 8-bit frames: brisque= cannot be used with 10-bit (uint16) frames")
        brisque_mod._check_size(height, width)
    return brisque


# ---- scores --------------------------------------------------------------------------------------------------------------------

class ScoreCollector:
    """The no-reference scores of a run: `features` computes a batch's NIQE / BRISQUE feature tensors on the device (no host
    sync), `add` holds what it is given - the device tensors, or their host copies where the caller downloads per group -, and
    `stats` turns all of it into the scores, one download and one ``scores_from_features`` per score."""

    def __init__(self, niqe=None, brisque=None, convert_to: Optional[str] = None):
        self.niqe, self.brisque, self.convert_to = niqe, brisque, convert_to
        self.held = []

    def features(self, frames: torch.Tensor, quantise: Optional[str] = None):
        """(NIQE features, BRISQUE features) of (b,C,H,W) frames, None for a score that was not asked for.  `quantise`: None for
        integer frames, the rule of the run for f32 frames (quantised in the kernels)."""
        kw = dict(quantise=quantise, convert_to=self.convert_to)
        return (None if self.niqe is None else niqe_mod.frame_niqe_features(frames, self.niqe, **kw),
                None if self.brisque is None else brisque_mod.frame_brisque_features(frames, **kw))

    def add(self, feats) -> None:
        self.held.append(feats)

    def stats(self) -> dict:
        """{"niqe", "niqe_mean", "brisque", "brisque_mean"}: per-frame f64 scores and their means; absent scores, absent keys."""
        out = {}
        for k, (name, mod, model) in enumerate((("niqe", niqe_mod, self.niqe), ("brisque", brisque_mod, self.brisque))):
            if model is not None:
                f = [h[k] for h in self.held]
                f = torch.cat(f).cpu().numpy() if isinstance(f[0], torch.Tensor) else np.concatenate(f, 0)
                out[name] = mod.scores_from_features(f, model)
                out[name + "_mean"] = float(np.mean(out[name]))
        return out


def check_reference(reference, dst, *, crop_border, baseline, bit_depth: int, height: int, width: int, out_shape=None,
                    reference_pix_fmt=None, tof: bool = False) -> Optional["ReferenceCollector"]:
    """The ``reference=`` keyword and its companions (``crop_border``, ``baseline``, ``reference_pix_fmt``, and ``dst=None``, which
    needs it) of a run on `width` x `height` LR frames of `bit_depth` bits that delivers `out_shape` (None: the 4x frame), before
    any device or file work (`reference.check_reference` has the rules).  Returns the run's `ReferenceCollector`, None without the
    keyword."""
    from . import reference as reference_mod
    from .resize import check_output_shape
    Ho, Wo = (4 * height, 4 * width) if out_shape is None else out_shape
    crop = reference_mod.check_reference(reference, dst is not None, crop_border, baseline, bit_depth, Ho, Wo, reference_pix_fmt)
    if crop is None:
        if tof:
            raise ValueError("tof=True compares against the ground truth: it needs reference=")
        return None
    if baseline is not None and out_shape is not None:
        check_output_shape(out_shape, height, width)                  # the baseline goes from the LR frame straight to (Ho, Wo)
    return ReferenceCollector(crop, bit_depth, Ho, Wo, baseline, bool(tof))


# ---- full-reference scores -----------------------------------------------------------------------------------------------------

def _as_samples(t: torch.Tensor) -> torch.Tensor:
    """int16 views of uint16 planes (`hip.bits16`) back as uint16; everything else as it is."""
    return t.view(torch.uint16) if t.dtype == torch.int16 else t


def baseline_luma(lr: torch.Tensor, shape, colour=None) -> torch.Tensor:
    """The luma (b,Ho,Wo) of the bicubic baseline of a group (``baseline="bicubic"``), no model pass.  `lr`: the unpadded integer LR
    centre frames, (b,1,H,W) luma of the Y path - `resize.bicubic_upscale(., 4, out="int")`, or `imresize` straight to `shape` =
    (Ho, Wo): the baseline of `evaluate_sequence` - or, with `colour`, the decoded (b,3,H,W) RGB frames of the RGB path: the luma of
    ``rgb_to_i420(imresize(lr, out="int"), colour)``."""
    from .colour import i420_planes, rgb_to_i420
    from .resize import bicubic_upscale, imresize
    H, W = lr.shape[-2:]
    if colour is None:
        return (bicubic_upscale(lr, 4, out="int") if shape is None else imresize(lr, output_shape=shape, out="int"))[:, 0]
    Ho, Wo = (4 * H, 4 * W) if shape is None else shape
    return i420_planes(rgb_to_i420(imresize(lr, output_shape=(Ho, Wo), out="int"), colour), Ho, Wo)[0]


class ReferenceCollector:
    """The full-reference scores of a run (``reference=``; `harness.reference` is the contract).  `score` computes a group's numbers
    on the device with no host sync - the exact squared-error sums of the luma planes and of U and V together (`hip.plane_sse`, two
    calls), the luma SSIM (`device_metrics.frame_metrics`) and, with ``baseline``, the PSNR / SSIM of the baseline luma - and packs
    them into one int64 tensor of `words` rows of b (f64 values as their bits); `add` holds what it is given, that tensor or its
    host copy where the caller downloads per group; `stats` makes the scores, one ``scores_from_sse`` for the run.

    With `tof` (``tof=True``; `harness.tof` is the contract) `score` adds the tOF of every delivered luma plane against the ground
    truth's - and of the baseline luma with ``baseline`` - as further rows of the same tensor: the groups arrive in frame order, and
    the collector carries a copy of the last (delivered, ground truth) plane pair of a group to the next one."""

    def __init__(self, crop_border: int, bit_depth: int, height: int, width: int, baseline=None, tof: bool = False):
        self.crop, self.bit_depth, self.height, self.width, self.baseline = int(crop_border), int(bit_depth), height, width, baseline
        self.tof = bool(tof)
        # sse_y, sse_u, sse_v, ssim_y (, baseline psnr_y, ssim_y) (, tof (, baseline tof))
        self.words = (4 if baseline is None else 6) + (0 if not self.tof else 1 if baseline is None else 2)
        self.held = []
        self.carry, self.starts = None, []                            # tof: the last planes; per frame, whether it starts a shot

    def _read10(self, g: torch.Tensor) -> torch.Tensor:
        """Ground-truth samples of a 10-bit run as min(k, 1023) (the delivered ones never exceed it), on the int16 bits."""
        if self.bit_depth == 8:
            return g
        b = hip.bits16(g)
        return torch.where((b < 0) | (b > 1023), torch.full_like(b, 1023), b).view(torch.uint16)

    def score(self, y: torch.Tensor, uv: torch.Tensor, gy: torch.Tensor, guv: torch.Tensor, base=None, cuts=()) -> torch.Tensor:
        """y (b,Ho,Wo), uv (2b,Ho/2,Wo/2: U planes, then V planes): the delivered planes; gy, guv: the ground truth's, laid out
        alike; base: the baseline luma (b,Ho,Wo) with ``baseline``; cuts: which of the b frames start a shot (0 .. b-1; read with
        `tof` only).  Returns the packed (words * b,) int64 device tensor."""
        from .device_metrics import frame_metrics
        y, gy = _as_samples(y), self._read10(_as_samples(gy))
        parts = [hip.plane_sse(y, gy, self.crop), hip.plane_sse(uv, guv, self.crop // 2)]
        parts.append(frame_metrics(y[:, None], gy[:, None], crop_border=self.crop, quantise=None)[1].view(torch.int64))
        if self.baseline is not None:
            parts += [m.view(torch.int64) for m in frame_metrics(_as_samples(base)[:, None], gy[:, None], crop_border=self.crop,
                                                                 quantise=None)]
        if self.tof:
            from .tof import frame_tof
            cuts = sorted(int(c) for c in cuts)
            prev = self.carry                                         # (y, gy (, base)) of the frame before this group, or None
            self.starts += [(i in cuts) or (i == 0 and prev is None) for i in range(y.shape[0])]
            parts.append(frame_tof(y, gy, first=None if prev is None else prev[:2], cuts=cuts).view(torch.int64))
            if self.baseline is not None:
                base = _as_samples(base)
                parts.append(frame_tof(base, gy, first=None if prev is None else (prev[2], prev[1]), cuts=cuts).view(torch.int64))
            last = (y, gy) if self.baseline is None else (y, gy, base)
            self.carry = tuple(hip.bits16(t[-1]).clone() for t in last)                   # copies: the planes may lie in a ring
        return torch.cat(parts)

    def add(self, packed) -> None:
        self.held.append(packed)

    def stats(self) -> dict:
        """The keys of `reference.sequence_scores`, and ``baseline_psnr_y`` / ``baseline_ssim_y`` with their means."""
        from . import reference as reference_mod
        rows = [(h.cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)).reshape(self.words, -1) for h in self.held]
        a = np.concatenate(rows, 1) if rows else np.zeros((self.words, 0), dtype=np.int64)
        a = np.ascontiguousarray(a, dtype=np.int64)
        out = reference_mod.sequence_scores(a[:3].T, a[3].view(np.float64), reference_mod.plane_sizes(self.height, self.width, self.crop),
                                            reference_mod.PEAKS[self.bit_depth])
        if self.baseline is not None:
            for k, name in ((4, "baseline_psnr_y"), (5, "baseline_ssim_y")):
                out[name] = a[k].view(np.float64).copy()
                out[name + "_mean"] = float(np.mean(out[name])) if out[name].size else float("nan")
        if self.tof:
            k0 = 4 if self.baseline is None else 6
            pairs = ~np.array(self.starts[:a.shape[1]], dtype=bool)
            for k, pre in ((k0, ""), (k0 + 1, "baseline_"))[:1 if self.baseline is None else 2]:
                v = a[k].view(np.float64).copy()
                out.update({pre + "tof": v, pre + "tof_mean": float(v.mean()) if v.size else float("nan"),
                            pre + "tof_pairs_mean": float(v[pairs].mean()) if pairs.any() else float("nan")})
        return out


# ---- delivery ------------------------------------------------------------------------------------------------------------------

def deliver_luma(ysr: torch.Tensor, uv: torch.Tensor, shape):
    """The Y path's planes as they are written: `ysr` (b,4H,4W) SR luma and `uv` (2b,H/2,W/2) LR chroma, U planes then V planes ->
    (Y (b,Ho,Wo), U then V (2b,Ho/2,Wo/2)).  `shape` None: the 4x frame, chroma by ``hip.chroma_up4``; (Ho, Wo): luma resized from
    the 4x frame and chroma ONCE from the LR planes, by `hip.imresize`."""
    if shape is None:
        return ysr, hip.chroma_up4(uv)
    return (hip.imresize(ysr, output_shape=shape, out="int"),
            hip.imresize(uv, output_shape=(shape[0] // 2, shape[1] // 2), out="int"))


def deliver_rgb(sr: torch.Tensor, colour, shape) -> torch.Tensor:
    """The RGB path's frames as they are written: (b,3,4H,4W) SR frames -> (b, Ho*Wo*3/2) I420 frames, resized plane by plane
    before the encode when `shape` = (Ho, Wo) is given."""
    from .colour import rgb_to_i420
    if shape is not None:
        sr = hip.imresize(sr, output_shape=shape, out="int")
    return rgb_to_i420(sr, colour)


def run_stats(frames: int, seconds: float, bytes_read: int, bytes_written: int, out_size, scores=(), cuts=None, active=None,
              tiles=None, reference=None) -> dict:
    """The stats every file / stream entry point returns: `out_size` is (width, height); `scores` (`ScoreCollector.stats`),
    ``"cuts"`` and ``"active"`` (`active`: the run's `active.ActivePlan`; the list of (first frame, box) changes) are there when the
    keywords were; `tiles`: the run's resolver, whose ``"tiles_total"`` / ``"tiles_run"`` are added with ``static_tiles=True``
    (`tiles.tile_counts`); `reference`: the run's `ReferenceCollector`, whose scores are added with ``reference=`` only."""
    from .tiles import tile_counts
    return {"frames": frames, "seconds": seconds, "fps": frames / seconds if seconds > 0 else float("inf"), "bytes_read": bytes_read,
            "bytes_written": bytes_written, "out_size": out_size, **dict(scores), **({} if cuts is None else {"cuts": cuts}),
            **({} if active is None else {"active": list(active.changes)}), **({} if tiles is None else tile_counts(tiles)),
            **({} if reference is None else reference.stats())}
