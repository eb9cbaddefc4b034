"""Raw YUV 4:2:0 video of any length, from a pipe to a pipe: the scheduler (host logic, `StreamPlan` and `AutoCuts`: no torch, no
device) and the entry point `stream_yuv420` around it.

`harness.yuv.super_resolve_yuv420*` map a whole file and upload every frame before the first model pass; here the frames arrive in
chunks of at most `batch`, are taken apart on the device into a ring of frame slots (`hip.surface_unpack`), and leave as soon as
their window is complete.  Every resolver (`steps.Resolver`: `PlainResolver`, `SelfEnsemble`,
`TiledSuperResolver`) takes the ring as `frames` and rows of slot numbers as `idx`, unchanged.

The windows are those of the finished stream, ``shots.windows_for(range(N), num_frames, N, padding, cuts)``, although N is not known
while they are made.  Before the end a centre c is released when frame ``c + num_frames // 2`` has arrived (`window_indices` then no
longer looks at N), when every frame the window names has arrived (a window that names a frame - "circle" reaches to c + 6 at the
start of a shot - is only right if that frame exists, and only stays inside its shot if no cut lies before it) and, with
``cuts="auto"``, when every frame up to there is known to start a shot or not.  Such a window is computed with the end of the
stream infinitely far away; after the end every window is computed with the true N.  No window names a frame below
``c - (num_frames - 1)`` ("reflection_circle" and "circle" at the end of a shot), which is what `keep_from` returns for the next centre.
"""
from __future__ import annotations

import contextlib
import os
import time
from bisect import bisect_right
from collections import deque
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .colour import ColourSpec
from .shots import check_auto, scene_scores, shot_ranges, windows_for
from .windows import window_indices

FAR = 1 << 60                      # "the end of the stream is not in sight" as a sequence length / frame number


class AutoCuts:
    """`shots.cuts_from_sad`, one pair sum at a time.  `scene_scores` is causal except for score[0], which is taken against the
    second pair: whether frame k starts a shot is known once frame ``max(k, 2)`` has arrived, or at the end.  `push` and `end` return
    the cuts that became known, in order; `known_upto` is the largest frame number up to which every frame's status is known."""

    def __init__(self, count: int, bit_depth: int, threshold: float = 10.0):
        self.count, self.bit_depth, self.threshold = int(count), int(bit_depth), float(threshold)
        self.pairs, self.ended, self.cuts = 0, False, []
        self._first = self._last = None

    def _score(self, sads, i: int) -> float:
        return float(scene_scores(np.asarray(sads, dtype=np.uint64), self.count, self.bit_depth)[i])

    def push(self, sads) -> List[int]:
        new = []
        for s in sads:
            s, i = int(s), self.pairs
            if i == 0:
                self._first = s
            else:
                if i == 1 and self._score([self._first, s], 0) >= self.threshold:
                    new.append(1)
                if self._score([self._last, s], 1) >= self.threshold:
                    new.append(i + 1)
            self._last, self.pairs = s, i + 1
        self.cuts += new
        return new

    def end(self) -> List[int]:
        new = []
        if not self.ended and self.pairs == 1 and self._score([self._first], 0) >= self.threshold:
            new.append(1)
        self.ended = True
        self.cuts += new
        return new

    @property
    def known_upto(self) -> int:
        if self.ended:
            return FAR
        return self.pairs if self.pairs >= 2 else 0                  # pairs + 1 frames arrived: frames 0 .. pairs


class StreamPlan:
    """Which windows can run, given how much of a stream has arrived (module docstring).  `cuts`: None, a sequence of frame numbers
    (validated here as far as that goes without the length; `finish` validates it against the length), or "auto": the caller then
    reports cuts as they become known (`cuts_known`, fed from `AutoCuts`)."""

    def __init__(self, num_frames: int = 7, padding: str = "replicate", batch: int = 8, cuts=None):
        if num_frames < 1 or num_frames % 2 == 0:
            raise ValueError(f"num_frames must be odd and positive, got {num_frames}")
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        window_indices(0, num_frames, 1, padding)                         # ValueError for an unknown padding mode
        check_auto(cuts, "uint8")
        self.num_frames, self.padding, self.batch = int(num_frames), padding, int(batch)
        self.auto = isinstance(cuts, str)
        if cuts is None or self.auto:
            self.cuts = [] if self.auto else None
        else:
            shot_ranges(FAR, cuts)
            self.cuts = [int(c) for c in cuts]
        self._known = 0 if self.auto else FAR                             # every frame number <= this is known to be a cut or not
        self.frames, self.eof, self.next = 0, False, 0

    def arrived(self, n: int, eof: bool = False) -> None:
        """n more frames are there; eof: the stream has ended (with them)."""
        if n < 0 or self.eof:
            raise ValueError("arrived: n >= 0, and nothing arrives after the end of the stream")
        self.frames += int(n)
        self.eof = bool(eof)
        if self.eof and self.auto:
            self._known = FAR

    def cuts_known(self, cuts: Sequence[int], upto: int) -> None:
        """cuts="auto": `cuts` are further frames that start a shot, and every frame number <= `upto` is now known to be one or
        not."""
        if not self.auto:
            raise ValueError('cuts_known is for cuts="auto"')
        for c in cuts:
            if self.cuts and c <= self.cuts[-1]:
                raise ValueError(f"cuts must arrive in increasing order, got {c} after {self.cuts[-1]}")
            self.cuts.append(int(c))
        self._known = max(self._known, int(upto))

    def _window(self, c: int) -> List[int]:
        """The window of centre c under what is known: the true length after the end (cuts at or beyond it are `finish`'s business),
        an endless stream before.  `shot_window_indices` looks at the shot of c only, so it is given that shot's two cuts."""
        n = self.frames if self.eof else FAR
        cuts = self.cuts
        if cuts is not None:
            k = bisect_right(cuts, c)
            cuts = [x for x in cuts[max(k - 1, 0):k + 1] if x < n]
        return windows_for([c], self.num_frames, n, self.padding, cuts)[0]

    def ready(self) -> List[Tuple[List[int], List[List[int]]]]:
        """[(centres, rows)]: the next groups of `batch` consecutive centres whose windows are final, with the frame numbers of each
        window; after the end, all that is left, the last group as short as it comes."""
        groups = []
        half = self.num_frames // 2
        while self.next < self.frames:
            centres, rows = [], []
            for c in range(self.next, min(self.next + self.batch, self.frames)):
                row = self._window(c)
                if not self.eof:
                    need = max(max(row), c + half)
                    if need >= self.frames or need > self._known:
                        break
                centres.append(c)
                rows.append(row)
            if not centres or (len(centres) < self.batch and not self.eof):
                break
            groups.append((centres, rows))
            self.next += len(centres)
        return groups

    def keep_from(self) -> int:
        """The smallest frame number a window that has not been handed out yet can name: num_frames - 1 below the next centre, and
        never below the start of that centre's shot as far as the cuts are known."""
        if self.eof and self.next >= self.frames:
            return self.frames
        k = bisect_right(self.cuts, self.next) if self.cuts else 0
        return max(0, self.next - (self.num_frames - 1), self.cuts[k - 1] if k else 0)

    def finish(self) -> Optional[List[int]]:
        """After the end: the cut list of the stream (None without cuts); explicit cuts at or beyond the end raise ValueError, as
        `shots.shot_ranges` words it."""
        if not self.eof:
            raise ValueError("finish: the stream has not ended")
        if self.cuts is not None and self.frames:
            shot_ranges(self.frames, self.cuts)
        return None if self.cuts is None else list(self.cuts)


# ---- the entry point ---------------------------------------------------------------------------------------------------------------

def _read_into(fh, view: memoryview) -> int:
    """`readinto` until `view` is full or the stream ends; the number of bytes read."""
    got = 0
    while got < len(view):
        n = fh.readinto(view[got:])
        if not n:
            break
        got += n
    return got


def _write_all(fh, view: memoryview) -> None:
    while len(view):
        n = fh.write(view)
        if n is None or n >= len(view):
            return
        view = view[n:]


def stream_yuv420(model, src, dst, width: int, height: int, *, pix_fmt: str = "yuv420p", out_pix_fmt: Optional[str] = None,
                  colour: ColourSpec = ColourSpec(), batch: int = 8, padding: str = "replicate", quantise: str = "truncate", num_frames: int = 7,
                  ensemble: Optional[str] = None, niqe=None, brisque=None, cuts=None, cut_threshold: float = 10.0, tile=None,
                  tile_overlap=16, output_shape=None, max_frames: Optional[int] = None, active=None,
                  static_tiles: bool = False, reference=None, reference_pix_fmt: Optional[str] = None, crop_border: int = 4,
                  baseline: Optional[str] = None, tof: bool = False) -> dict:
    """Super-resolve raw 4:2:0 video of any length from `src` to `dst` 4x, a chunk of frames at a time.

    `src`: a path, or any binary object with ``readinto`` (``sys.stdin.buffer``, a pipe, a socket file); it is never seeked or
    asked for a size.  `dst`: a path, or any object with ``write``.  `pix_fmt` / `out_pix_fmt` (default: `pix_fmt`; it must have
    the same bit depth): ``harness.surfaces.PIX_FMTS``.  A one-channel model runs as `harness.yuv.super_resolve_yuv420` (Y through
    the model, U and V through ``hip.chroma_up4`` or `imresize`), a three-channel model as `super_resolve_yuv420_rgb` with `colour`
    (its bit depth must be the format's; a one-channel model ignores it).  Every other keyword means what it
    means there, and for yuv420p / yuv420p10le the bytes written and the stats entries ``frames``, ``out_size``, ``cuts``, ``active``,
    ``niqe``, ``niqe_mean``, ``brisque``, ``brisque_mean``, ``bytes_written`` are those of the whole-file function on a file of the
    same frames (``active="auto"``: one `hip.frame_line_sums` of the luma planes of every chunk and its small download; the box of a
    window is that of the last frame it names, which has arrived when the window runs); for nv12 / p010le they are
    `surfaces.pack_host` of that result on `surfaces.unpack_host` of the source.

    Frames are read in chunks of at most `batch` into two pinned staging buffers and uploaded on a side stream while the previous
    group is in the model; `hip.surface_unpack` puts them into a ring of ``2 batch + 2 (num_frames - 1)`` frame slots (`StreamPlan`
    says which windows can run and which frames may go), `hip.surface_pack` lays every group of SR frames out as the file holds
    them, and the group is written - one copy to one of two pinned buffers, one ``write`` - after the next one has been launched.
    Device and pinned memory do not depend on the length of the stream.

    The one difference from the whole-file functions: an explicit cut at or beyond the end of the stream raises ValueError at the
    end, when the length is known and the frames have been written.  A trailing partial frame: all whole frames are written, then
    ValueError names the stray bytes.  An empty stream raises ValueError.  ``max_frames=n`` stops after n frames and leaves the rest
    of a pipe unread.  Extra stats: ``ring_frames``, ``frames_uploaded`` (= frames), ``h2d_bytes``, ``d2h_bytes``, ``seconds``,
    ``fps``.

    ``static_tiles`` as in `super_resolve_sequence` (True needs ``tile``; stats ``"tiles_total"`` / ``"tiles_run"``).  Reuse stays
    inside a group: the ring slots of the previous group's oldest frames may already hold newer frames.  The comparison runs on
    the main stream at the head of the group's step, after the wait for the chunk's upload, and its small download is the one
    host synchronisation of the group.  Running the comparison and its download on the side stream instead, so that they do not
    wait behind the previous group's model pass, was measured against this placement and made no difference (profiles/NOTES.md).

    ``reference`` / ``crop_border`` as in `harness.yuv.super_resolve_yuv420`, with the same stats keys and values.
    ``baseline="bicubic"`` (needs ``reference``) adds ``"baseline_psnr_y"`` / ``"baseline_ssim_y"`` and their means, without a
    model pass: `device_metrics.frame_metrics` of the bicubic luma against the ground truth's - for a one-channel model the
    unpadded LR luma through `resize.bicubic_upscale(., 4, out="int")` (`imresize` straight to ``output_shape``), exactly the
    baseline of `evaluate_sequence`; for a three-channel model as in `super_resolve_yuv420_rgb`.  Chroma is not part of it.
    `reference` is a path, or any object with ``readinto`` (never seeked), whose frames have the delivered size in
    `reference_pix_fmt` (default `out_pix_fmt`; it must have the run's bit depth).  After every chunk of n source frames exactly n
    ground-truth frames are read into a second pair of pinned staging buffers, uploaded on the side stream and taken apart by
    `hip.surface_unpack` into a ring of their own with the slots and the bookkeeping of the frame ring: a frame's slot is free once
    its group has been scored, so device and pinned memory stay independent of the length.  A group's scores reach the host after
    its ``done`` event, one small pinned copy.  The ground truth must hold at least as many whole frames as the source: if it ends
    early every source frame is still written, and ValueError names both counts at the end; bytes beyond the last frame needed are
    left unread.  ``dst=None`` (needs ``reference``): no pack, no download, no write, ``bytes_written`` 0 - a pure evaluation
    run.

    ``tof=True`` (needs ``reference``) as in `harness.yuv.super_resolve_yuv420`: ``"tof"``, ``"tof_mean"``, ``"tof_pairs_mean"`` (and
    ``"baseline_tof*"`` with ``baseline``), the same values as the file entry point gives; one plane pair is carried from group to
    group on the device, and the values ride in the packed tensor of the group's other scores: no further host sync."""
    import torch

    from .. import hip
    from . import surfaces
    from .colour import i420_planes, yuv420_to_rgb
    from .steps import (ScoreCollector, baseline_luma, check_keywords, check_reference, check_scores, deliver_luma, deliver_rgb,
                        group_boxes, run_stats)
    from .yuv import _check_output_shape_420

    surfaces.check_fmt(pix_fmt)
    out_pix_fmt = pix_fmt if out_pix_fmt is None else surfaces.check_fmt(out_pix_fmt)
    bits = surfaces.bit_depth(pix_fmt)
    if surfaces.bit_depth(out_pix_fmt) != bits:
        raise ValueError(f"out_pix_fmt {out_pix_fmt!r} is {surfaces.bit_depth(out_pix_fmt)}-bit, pix_fmt {pix_fmt!r} {bits}-bit: "
                         "the model keeps the bit depth")
    W, H = int(width), int(height)
    fb_in = surfaces.frame_bytes(pix_fmt, W, H)
    C = getattr(model, "_img_ch", None)
    if C == 3:
        if not isinstance(colour, ColourSpec):
            raise ValueError(f"colour must be a ColourSpec, got {type(colour).__name__}")
        if colour.bit_depth != bits:
            raise ValueError(f"colour is {colour.bit_depth}-bit, pix_fmt {pix_fmt!r} {bits}-bit")
    shape = _check_output_shape_420(output_shape, W, H, chroma=C == 1)
    ref = check_reference(reference, dst, crop_border=crop_border, baseline=baseline, bit_depth=bits, height=H, width=W,
                          out_shape=shape, reference_pix_fmt=reference_pix_fmt, tof=tof)
    ref_fmt = out_pix_fmt if reference_pix_fmt is None else reference_pix_fmt
    brisque = check_scores(niqe, brisque, bits, 4 * H, 4 * W)
    resolver = check_keywords(model, ensemble=ensemble, tile=tile, tile_overlap=tile_overlap, batch=batch, quantise=quantise,
                              cuts=cuts, frame_dtype="uint8", channels=(1, 3), who="stream_yuv420", active=active,
                              frame_shape=(1, H, W), bit_depth=bits, static_tiles=static_tiles)
    act = resolver.boxes if resolver.boxes is not None and resolver.boxes.auto else None      # active="auto": fed per chunk
    if max_frames is not None and max_frames < 0:
        raise ValueError(f"max_frames must be >= 0, got {max_frames}")
    plan = StreamPlan(num_frames, padding, batch, cuts)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("stream_yuv420 runs on the HIP device only (there is no CPU fallback)")
    Ho, Wo = (4 * H, 4 * W) if shape is None else shape
    fb_out = surfaces.frame_bytes(out_pix_fmt, Wo, Ho)
    sdt, bdt = (torch.uint8, torch.uint8) if bits == 8 else (torch.uint16, torch.int16)       # frames travel as `hip.bits16`
    B, T, h2, w2 = plan.batch, plan.num_frames, H // 2, W // 2
    R = 2 * B + 2 * (T - 1)
    Hp, Wp = (n + (-n) % resolver.multiple for n in (H, W))              # the padding `pad_to_multiple` adds; zero for ever
    auto = AutoCuts(H * W, bits, cut_threshold) if plan.auto else None

    with contextlib.ExitStack() as stack, torch.no_grad(), torch.cuda.device(dev):
        fin = stack.enter_context(open(src, "rb", buffering=0)) if isinstance(src, (str, bytes, os.PathLike)) else src
        fout = stack.enter_context(open(dst, "wb")) if isinstance(dst, (str, bytes, os.PathLike)) else dst
        gin = stack.enter_context(open(reference, "rb", buffering=0)) if isinstance(reference, (str, bytes, os.PathLike)) else reference
        t0 = time.perf_counter()
        main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        # the ring the resolvers read (Y, or decoded RGB), the chroma rings of the Y path, the planes of one chunk for the RGB path
        ring = torch.zeros((R, C, Hp, Wp), dtype=bdt, device=dev)
        if C == 1:
            ring_y, ring_u, ring_v = ring, *(torch.zeros((R, h2, w2), dtype=bdt, device=dev) for _ in range(2))
        else:
            ring_y, ring_u, ring_v = (torch.zeros(s, dtype=bdt, device=dev) for s in ((B, 1, H, W), (B, h2, w2), (B, h2, w2)))
            chunk_slots = torch.arange(B, dtype=torch.int32, device=dev)
        raw_dev = torch.empty((B * fb_in,), dtype=torch.uint8, device=dev)
        slots_dev = torch.zeros((B,), dtype=torch.int32, device=dev)
        stage = [torch.empty((B * fb_in,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        slots_pin = [torch.zeros((B,), dtype=torch.int32, pin_memory=True) for _ in range(2)]
        out_pin = [torch.empty((B, fb_out), dtype=torch.uint8, pin_memory=True) for _ in range(2)] if fout is not None else None
        if ref is not None:
            # the ground truth's own ring (U and V in the two halves of one tensor: a group's chroma is one gather), staging and slots
            fb_ref, ho2, wo2 = surfaces.frame_bytes(ref_fmt, Wo, Ho), Ho // 2, Wo // 2
            gring_y = torch.zeros((R, 1, Ho, Wo), dtype=bdt, device=dev)
            gring_uv = torch.zeros((2 * R, ho2, wo2), dtype=bdt, device=dev)
            graw_dev = torch.empty((B * fb_ref,), dtype=torch.uint8, device=dev)
            gslots_dev = torch.zeros((B,), dtype=torch.int32, device=dev)
            gstage = [torch.empty((B * fb_ref,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            gslots_pin = [torch.zeros((B,), dtype=torch.int32, pin_memory=True) for _ in range(2)]
            score_pin = [torch.zeros((ref.words * B,), dtype=torch.int64, pin_memory=True) for _ in range(2)]
            gwhere, gresident, gfree = {}, deque(), list(range(R - 1, -1, -1))
        gt_frames, gt_short = 0, False
        uploaded = [torch.cuda.Event() for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        gathered = torch.cuda.Event()
        main.synchronize()                                                # the zeroed rings are complete before the side stream writes
        where, resident, free = {}, deque(), list(range(R - 1, -1, -1))   # frame -> slot; resident frames in order; free slots
        prev_y = None                                                     # RGB path, cuts="auto": the luma of the last frame
        written, groups_run, pending, last_up = 0, 0, None, 0
        scores = ScoreCollector(niqe, brisque, None if C == 1 else "Y")

        def upload(k: int, n: int, first: int, ng: int = 0) -> None:
            """Chunk k = frames first .. first + n - 1, staged in stage[k & 1]: into free slots on the side stream; with it the
            ground-truth frames first .. first + ng - 1, staged in gstage[k & 1]."""
            nonlocal prev_y, last_up
            last_up = k
            keep = plan.keep_from()
            while resident and resident[0] < keep:
                free.append(where.pop(resident.popleft()))
            if len(free) < n:
                raise RuntimeError(f"frame ring of {R} slots is full: {len(resident)} frames held from {keep}")   # a bug in StreamPlan
            slots = [free.pop() for _ in range(n)]
            for i, s in enumerate(slots):
                where[first + i] = s
                resident.append(first + i)
                slots_pin[k & 1][i] = s
            if ng:                                                        # a ground-truth frame stays until its group has been scored
                while gresident and gresident[0] < plan.next:
                    gfree.append(gwhere.pop(gresident.popleft()))
                if len(gfree) < ng:
                    raise RuntimeError(f"reference ring of {R} slots is full: {len(gresident)} frames held from {plan.next}")
                for i in range(ng):
                    gwhere[first + i] = gslots_pin[k & 1][i] = gfree.pop()
                    gresident.append(first + i)
            with torch.cuda.stream(side):
                side.wait_event(gathered)                                 # the gathers launched so far read the slots first
                raw = raw_dev[:n * fb_in]
                raw.copy_(stage[k & 1][:n * fb_in], non_blocking=True)
                sl = slots_dev[:n]
                sl.copy_(slots_pin[k & 1][:n], non_blocking=True)
                if C == 1:
                    hip.surface_unpack(raw, pix_fmt, W, H, sl, ring_y.view(sdt), ring_u.view(sdt), ring_v.view(sdt))
                    if auto is not None:
                        idx = ([where[first - 1]] if first else []) + slots
                        luma = ring[torch.tensor(idx, dtype=torch.int64).to(dev)]
                    if act is not None:                                   # the chunk's luma planes, without the padding
                        lines = hip.frame_line_sums(ring[torch.tensor(slots, dtype=torch.int64).to(dev)][:, :, :H, :W].view(sdt))
                else:
                    hip.surface_unpack(raw, pix_fmt, W, H, chunk_slots[:n], ring_y.view(sdt), ring_u.view(sdt), ring_v.view(sdt))
                    rgb = yuv420_to_rgb(ring_y[:n, 0].view(sdt), ring_u[:n].view(sdt), ring_v[:n].view(sdt), colour)
                    ring[sl.long(), :, :H, :W] = hip.bits16(rgb)
                    if auto is not None:
                        luma = ring_y[:n] if prev_y is None else torch.cat([prev_y, ring_y[:n]], 0)
                        prev_y = ring_y[n - 1:n].clone()
                    if act is not None:
                        lines = hip.frame_line_sums(ring_y[:n].view(sdt))
                if auto is not None:                                      # one small download per chunk; waits for this upload only
                    sad = hip.frame_pair_sad(luma.view(sdt)).cpu().numpy()
                    plan.cuts_known(auto.push(sad), auto.known_upto)
                if act is not None:                                       # the same: one small download per chunk
                    act.push(lines[0].cpu().numpy(), lines[1].cpu().numpy())
                if ng:
                    graw = graw_dev[:ng * fb_ref]
                    graw.copy_(gstage[k & 1][:ng * fb_ref], non_blocking=True)
                    gsl = gslots_dev[:ng]
                    gsl.copy_(gslots_pin[k & 1][:ng], non_blocking=True)
                    hip.surface_unpack(graw, ref_fmt, Wo, Ho, gsl, gring_y.view(sdt), gring_uv[:R].view(sdt), gring_uv[R:].view(sdt))
                uploaded[k & 1].record(side)

        def launch(centres, rows):
            """One group through the model, laid out as the file holds it, on its way to out_pin[g & 1]."""
            nonlocal groups_run
            g, b = groups_run, len(centres)
            main.wait_event(uploaded[last_up & 1])                         # the side stream is in order: every chunk so far
            # a frame number below 0 (a sequence shorter than the window, after its end) counts from the end, as ``x[j]`` does
            idx = [[where[f if f >= 0 else plan.frames + f] for f in row] for row in rows]
            sr = resolver.frames(ring.view(sdt), idx, quantise, H, W, group_boxes(resolver, centres, rows, plan.frames))
            scored = ref is not None and all(c in gwhere for c in centres)                 # not beyond the end of a short reference
            if C == 1 or (scored and baseline is not None):
                cs = torch.tensor([where[c] for c in centres], dtype=torch.int64).to(dev)
            if C == 1:
                uv = torch.cat([ring_u[cs], ring_v[cs]], 0).view(sdt)                      # (2b, H/2, W/2)
            if scored:                                                                    # the group's ground truth, out of its ring
                gs = torch.tensor([gwhere[c] for c in centres], dtype=torch.int64).to(dev)
                gy, guv = gring_y[gs][:, 0], gring_uv[torch.cat([gs, gs + R])]
                lrc = ring[cs][:, :, :H, :W].view(sdt) if baseline is not None else None   # the unpadded LR centre frames
            gathered.record(main)
            feats = scores.features(sr)
            if C == 1:
                ysr, uvsr = deliver_luma(sr[:, 0], uv, shape)
                planes = (ysr, uvsr[:b], uvsr[b:])
            else:
                planes = i420_planes(deliver_rgb(sr, colour, shape), Ho, Wo)
                if scored:
                    ysr, uvsr = planes[0], torch.cat([hip.bits16(planes[1]), hip.bits16(planes[2])], 0)
            words = 0
            if scored:                                                                    # its host copy is read after `done`
                base = None if baseline is None else baseline_luma(lrc, shape, None if C == 1 else colour)
                packed = ref.score(ysr, uvsr, gy, guv, base, cuts=[i for i, c in enumerate(centres) if c in (plan.cuts or ())])
                words = packed.numel()
                score_pin[g & 1][:words].copy_(packed, non_blocking=True)
            if fout is not None:
                out_pin[g & 1][:b].copy_(hip.surface_pack(*planes, out_pix_fmt), non_blocking=True)
            done[g & 1].record(main)
            groups_run += 1
            return g, b, feats, words

        def deliver(group) -> None:
            """The write of a launched group, and its scores' features to the host."""
            nonlocal written
            g, b, feats, words = group
            done[g & 1].synchronize()
            if fout is not None:
                _write_all(fout, memoryview(out_pin[g & 1][:b].numpy()).cast("B"))
                written += b * fb_out
            if words:
                ref.add(score_pin[g & 1][:words].numpy().copy())
            scores.add(tuple(f if f is None else f.cpu().numpy() for f in feats))      # after `done`: it waits for nothing newer

        k, stray, eof = 0, 0, False
        while not eof:
            want = B if max_frames is None else min(B, max_frames - plan.frames)
            if k >= 2:
                uploaded[k & 1].synchronize()                             # chunk k - 2 has left this staging buffer
            got = _read_into(fin, memoryview(stage[k & 1].numpy())[:want * fb_in]) if want else 0
            n, rest = divmod(got, fb_in)
            eof = got < want * fb_in or (max_frames is not None and plan.frames + n >= max_frames)
            stray = rest
            ng = 0
            if ref is not None and n and not gt_short:                    # exactly n ground-truth frames, as long as there are any
                ng = _read_into(gin, memoryview(gstage[k & 1].numpy())[:n * fb_ref]) // fb_ref
                gt_frames, gt_short = gt_frames + ng, ng < n
            if n:
                upload(k, n, plan.frames, ng)
            if eof and auto is not None:
                plan.cuts_known(auto.end(), FAR)
            plan.arrived(n, eof)
            for centres, rows in plan.ready():
                group = launch(centres, rows)
                if pending is not None:
                    deliver(pending)
                pending = group
            k += 1
        if pending is not None:
            deliver(pending)
        torch.cuda.synchronize(dev)
        N = plan.frames
        dt = time.perf_counter() - t0
    if N == 0 and not stray:
        raise ValueError("the stream holds no frames")
    if stray:
        raise ValueError(f"the stream ends with {stray} stray bytes after {N} whole {W}x{H} {pix_fmt} frames ({fb_in} bytes each)")
    if ref is not None and gt_frames < N:
        raise ValueError(f"the reference ends after {gt_frames} whole {Wo}x{Ho} {ref_fmt} frames, the source holds {N}: "
                         f"{N} frames were super-resolved, none of the scores is returned")
    used = plan.finish()                                                  # ValueError: an explicit cut at or beyond the end
    stats = run_stats(N, dt, N * fb_in, written, (Wo, Ho), scores.stats(), used, resolver.boxes, resolver, ref)
    stats.update(ring_frames=R, frames_uploaded=N, h2d_bytes=N * fb_in + (0 if ref is None else gt_frames * fb_ref),
                 d2h_bytes=written)                                       # the ground-truth frames are uploaded too
    return stats
