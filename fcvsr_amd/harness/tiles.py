"""Tiled inference: the model runs on overlapping tiles of the frame instead of the whole frame, and the tile outputs are blended with
feathered weights (the ``--tile`` / ``--tile_pad`` of SR toolboxes; here ``tile=`` / ``tile_overlap=`` on the harness entry points).
It bounds the memory of a model pass by the tile instead of the frame, and gives every model pass of a run one shape - one captured
hipGraph whatever the video's size (``model.use_graph``; a ragged last chunk of windows adds a second batch size, not a second
window shape).

A tiled result is NOT the full-frame result.  Several operators of the network are global - MGAA and MFFR transform the whole
frame, the Gaussian band split is relative to the frame size, ContextBlock pools over the frame - so the model on a tile is a
different estimator from the model on the frame, not an approximation of it that improves with the overlap.  The feathered overlap
hides seams; it does not make the two equal.  (The model is trained on 128 x 128 crops, so a tile near that size is inference at the
training size; which of the two is better on real footage has not been measured here.)

Specification.  All geometry is in LR pixels on the frame zero-padded at the bottom / right to multiples of 4 (Hp x Wp, the
harness's padding rule); the output is cropped to 4h x 4w of the unpadded frame.

Keywords.  ``tile``: None, an int, or (th, tw), each a positive multiple of 4.  ``tile_overlap``: an int or (oy, ox), default 16, with
``0 <= o <= t // 2`` per axis.  Anything else is a ValueError raised before any device work (`check_tile`).

Grid per axis (`axis_starts`), for padded length L, tile t, overlap o: one tile [0, L) if ``L <= t``; otherwise the starts are
``list(range(0, L - t, t - o)) + [L - t]`` and every tile has length t.  All tiles of a frame therefore have one shape,
``(min(th, Hp), min(tw, Wp))``: the last tile is shifted inward instead of being smaller.

Weights per axis (`axis_weights`), in SR pixels (scale 4), as integers first.  Tile k starts at a and has length tt; at local SR
coordinate q in [0, 4 tt):  ``left = q + 1`` if ``a > 0`` else infinity;  ``right = 4 tt - q`` if ``a + tt < L`` else infinity;
``w_k = min(left, right, max(4 o, 1))``.  The normalised weight is ``float32(float64(w_k) / float64(sum_k w_k))`` at each SR
coordinate: a pixel covered by one tile gets exactly 1.0f.  The covering tiles of a coordinate are a contiguous index range of at
most 3 tiles (L = 28, t = 16, o = 8: starts [0, 8, 12]).

Blend (`blend_host`).  For each output pixel, in f32: ``acc = 0``; for ky ascending, then kx ascending, over the tiles that cover
it, ``acc = acc + (wy[ky, y] * wx[kx, x]) * v`` - each of the three operations rounded once, no FMA - with v the f32 model output of
that tile at ``(y - 4 ay, x - 4 ax)``.  Then the quantisation of the self-ensemble's merge: none for f32, or the model's integer
rule to uint8 / 10-bit uint16 with "truncate" | "round".

Tile input.  The tile window is cut from the UNPADDED resident sequence (N,C,h,w) through the window index rows; samples outside
h x w (the multiple-of-4 padding) are 0.  Integer samples enter as the floats of ``hip.u8_table`` / ``hip.u16_table``, exactly as in
the self-ensemble.

With ``ensemble=``: each tile window goes through ``SelfEnsemble(model, temporal)`` in place of the model - tile, then ensemble each
tile.  Tiles are multiples of 4 on both sides, so the ensemble's own padding rule is idle.

Model passes.  The ``b * ny * nx`` tile windows of a harness step run through the model's float ``forward`` in chunks of at most
`batch` windows, so the peak memory of a pass is bounded by `batch` tile-sized windows (the engine's output does not depend on the
batch a window sits in).  The model always runs without autograd; ``use_graph`` and ``streams`` apply as usual.

`axis_starts`, `axis_weights`, `tile_plan`, `blend_host` and `tiled_host` are the specification (CPU tensors), not a code path:
`TiledSuperResolver` runs on the HIP device only.  Two kernels do the data movement (csrc/tiles.hip): ``hip.tile_windows`` builds all
tile windows of a batch straight from the resident sequence through the index table (the plain full-frame windows are never
materialised) and ``hip.tile_merge`` crops, blends in the fixed order and quantises.  The results equal the specification bit for
bit.

Static tiles (``static_tiles=True``, only together with ``tile=``).  The model is a pure function of a tile window, and the
engine's output does not depend on the batch a window sits in, so a tile window that holds the same bits as an earlier one has the
same output, and that output can be reused: the delivered frames are exactly those of ``static_tiles=False``.  Reuse is WITHIN one
call of `Resolver.sequence`, i.e. within one group of b index rows:

- row 0 of a group computes all its tiles;
- for r >= 1, tile (ky,kx) of row r is static iff for every i in 0..T-1 the frames ``rows[r][i]`` and ``rows[r-1][i]`` are the same
  frame number, or are bit-identical AS STORED, over all channels, on the tile's rectangle clipped to the frame,
  ``[ay, min(ay + th, h)) x [ax, min(ax + tw, w))``: bytes for uint8, the raw 16-bit words for uint16 (not ``min(k, 1023)``: two
  words above 1023 that differ count as different although the model reads both as 1023), the 32-bit patterns for f32 (``+0.0`` and
  ``-0.0`` differ; equal NaN patterns agree).  Raw comparison can only miss reuse, it can never reuse wrongly;
- a static tile takes the tile output of row r-1, which may itself be reused: chains end at a computed tile of the same group.

Reuse is not carried across groups: the `Resolver` contract is stateless, and in `stream_yuv420` the ring slots of the previous
group's oldest frames may already be overwritten.  So at least ``ny * nx`` tile windows run per group and the saving is capped at a
factor b (the `batch` of the entry points): the cost per group falls from ``b ny nx`` windows to no less than ``ny nx``, 1/b of it.
`static_pairs`, `static_sources` and `static_map_host` are this specification on the host.  On the device
(`TiledSuperResolver._sequence_static`): ``hip.tile_pairs_equal`` compares the pairs, one small download of its (P,ny,nx) flags is the
one host synchronisation of the group, ``hip.tile_windows(sel=)`` gathers only the computed windows in row-major (row, ky, kx)
order, the model passes fill a pool of tile outputs, and ``hip.tile_merge(src=)`` blends through the slot table.  The resolver
counts ``tiles_total`` and ``tiles_run``.  Not claimed: a speed-up on any real sequence - how many tiles of compressed footage are
bit-identical over 8 consecutive frames has not been measured; the claim is the mechanism and its exactness.

Out of scope: `StreamedSuperResolver` and ``fit(..., val_sequences=...)`` take no tile option; there is no temporal tiling and no
automatic choice of the tile size; no reuse across groups or calls, and no tolerance-based ("nearly static") reuse.
"""
from __future__ import annotations

import functools
import operator
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from .ensemble import SelfEnsemble, check_mode
from .steps import PlainResolver, Resolver

SCALE = 4


def _pair(v, name: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be an int or a pair, got {v!r}")
        vals = tuple(v)
    else:
        vals = (v, v)
    out = []
    for e in vals:
        if isinstance(e, bool):
            raise ValueError(f"{name} must be an int or a pair of ints, got {v!r}")
        try:
            out.append(operator.index(e))
        except TypeError:
            raise ValueError(f"{name} must be an int or a pair of ints, got {v!r}") from None
    return out[0], out[1]


def check_tile(tile, tile_overlap=16) -> Optional[Tuple[Tuple[int, int], Tuple[int, int]]]:
    """The harness keywords: None for ``tile=None`` (no tiling; the overlap is not looked at), else ``((th, tw), (oy, ox))`` -
    tiles positive multiples of 4, ``0 <= o <= t // 2`` per axis; anything else raises ValueError."""
    if tile is None:
        return None
    t = _pair(tile, "tile")
    o = _pair(tile_overlap, "tile_overlap")
    for tt, oo in zip(t, o):
        if tt <= 0 or tt % 4:
            raise ValueError(f"tile sides must be positive multiples of 4, got {tile!r}")
        if not 0 <= oo <= tt // 2:
            raise ValueError(f"tile_overlap must be in 0 .. tile // 2 per axis, got {tile_overlap!r} for tile {tile!r}")
    return t, o


def axis_starts(L: int, t: int, o: int) -> List[int]:
    """The tile starts along an axis of padded length L: [0] if ``L <= t``, else ``range(0, L - t, t - o)`` and the last tile
    shifted inward to ``L - t``."""
    if L <= 0 or t <= 0 or not 0 <= o <= t // 2:
        raise ValueError(f"axis_starts: L, t positive and 0 <= o <= t // 2, got L={L}, t={t}, o={o}")
    if L <= t:
        return [0]
    return list(range(0, L - t, t - o)) + [L - t]


def axis_weights(L: int, t: int, o: int, scale: int = SCALE):
    """``(starts, tt, wi, wn)`` of an axis: the tile starts, the tile length ``min(t, L)``, the integer weights ``wi`` (n, scale L)
    int64 (0 where a tile does not reach) and their normalised f32 form ``wn = float32(float64(wi) / float64(wi.sum(0)))``."""
    starts = axis_starts(L, t, o)
    tt = min(t, L)
    q = np.arange(scale * tt, dtype=np.int64)
    cap = max(scale * o, 1)
    wi = np.zeros((len(starts), scale * L), dtype=np.int64)
    for k, a in enumerate(starts):
        wk = np.full_like(q, cap)
        if a > 0:
            wk = np.minimum(wk, q + 1)
        if a + tt < L:
            wk = np.minimum(wk, scale * tt - q)
        wi[k, scale * a:scale * (a + tt)] = wk
    total = wi.sum(0)
    if int(total.min()) < 1:
        raise AssertionError(f"axis_weights: a coordinate is not covered (L={L}, t={t}, o={o})")
    wn = (wi.astype(np.float64) / total.astype(np.float64)[None, :]).astype(np.float32)
    return starts, tt, wi, wn


@dataclass(eq=False)
class TilePlan:
    """The tiling of h x w frames: padded size (Hp, Wp), the one tile shape (th, tw), the overlaps, the tile starts per axis and the
    normalised f32 weight tables wy (ny, 4 Hp) / wx (nx, 4 Wp).  `device_tables` uploads the four tables once per device."""
    h: int
    w: int
    Hp: int
    Wp: int
    th: int
    tw: int
    oy: int
    ox: int
    ys: List[int]
    xs: List[int]
    wy: np.ndarray
    wx: np.ndarray
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def ny(self) -> int:
        return len(self.ys)

    @property
    def nx(self) -> int:
        return len(self.xs)

    def device_tables(self, device):
        """(ys, xs) int32 and (wy, wx) f32 on `device`, built once per device and complete before they are returned (create them
        outside stream fan-out and graph capture, as `hip.u8_table`)."""
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            t = (torch.tensor(self.ys, dtype=torch.int32).to(device), torch.tensor(self.xs, dtype=torch.int32).to(device),
                 torch.from_numpy(self.wy).to(device), torch.from_numpy(self.wx).to(device))
            torch.cuda.synchronize(device)
            self._dev[key] = t
        return t


@functools.lru_cache(maxsize=16)
def _plan(h: int, w: int, t: Tuple[int, int], o: Tuple[int, int]) -> TilePlan:
    Hp, Wp = h + (-h) % 4, w + (-w) % 4
    ys, th, _, wy = axis_weights(Hp, t[0], o[0])
    xs, tw, _, wx = axis_weights(Wp, t[1], o[1])
    return TilePlan(h, w, Hp, Wp, th, tw, o[0], o[1], ys, xs, np.ascontiguousarray(wy), np.ascontiguousarray(wx))


def tile_plan(h: int, w: int, tile, overlap=16) -> TilePlan:
    """The `TilePlan` of h x w (unpadded) frames for the harness keywords ``tile`` / ``tile_overlap`` (validated by `check_tile`;
    ``tile=None`` raises).  Plans are cached: the same arguments give the same object and its device tables."""
    chk = check_tile(tile, overlap)
    if chk is None:
        raise ValueError("tile_plan needs a tile size, got tile=None")
    if h < 1 or w < 1:
        raise ValueError(f"h, w must be positive, got {h}, {w}")
    return _plan(int(h), int(w), *chk)


def blend_host(tiles: torch.Tensor, plan: TilePlan) -> torch.Tensor:
    """The blend of the specification on a CPU tensor: `tiles` (b,ny,nx,C,4th,4tw) f32 -> (b,C,4h,4w) f32, the fixed-order sum
    ``acc = acc + (wy * wx) * v`` over ky, then kx, one f32 rounding per operation, cropped to the unpadded frame."""
    tiles = tiles.float()
    b, ny, nx, C = tiles.shape[:4]
    if (ny, nx) != (plan.ny, plan.nx) or tuple(tiles.shape[4:]) != (SCALE * plan.th, SCALE * plan.tw):
        raise ValueError(f"tiles {tuple(tiles.shape)} do not fit the plan ({plan.ny} x {plan.nx} tiles of {plan.th} x {plan.tw})")
    wy, wx = torch.from_numpy(plan.wy), torch.from_numpy(plan.wx)
    acc = torch.zeros((b, C, SCALE * plan.Hp, SCALE * plan.Wp), dtype=torch.float32)
    TH, TW = SCALE * plan.th, SCALE * plan.tw
    for ky, ay in enumerate(plan.ys):
        Y = SCALE * ay
        for kx, ax in enumerate(plan.xs):
            X = SCALE * ax
            g = wy[ky, Y:Y + TH, None] * wx[kx, None, X:X + TW]
            acc[:, :, Y:Y + TH, X:X + TW] = acc[:, :, Y:Y + TH, X:X + TW] + g * tiles[:, ky, kx]
    return acc[:, :, :SCALE * plan.h, :SCALE * plan.w].contiguous()


def tiled_host(win: torch.Tensor, fn: Callable, plan: TilePlan, idx: Optional[Sequence[Sequence[int]]] = None) -> torch.Tensor:
    """The specification of tiled inference on CPU tensors.  `win`: a (B,T,C,h,w) f32 window - or, with `idx` (B rows of T frame
    numbers), the sequence (N,C,h,w) the windows are cut from.  `fn`: any window -> SR function, (B,T,C,th,tw) -> (B,C,4th,4tw).
    The frames are zero-padded at the bottom / right to multiples of 4, every tile window of `plan` goes through `fn`, and the
    outputs are blended by `blend_host`.  Returns (B,C,4h,4w) f32."""
    win = win.float()
    if idx is not None:
        win = win[torch.tensor([[int(j) for j in r] for r in idx], dtype=torch.long)]
    if win.dim() != 5 or tuple(win.shape[-2:]) != (plan.h, plan.w):
        raise ValueError(f"expected (B,T,C,{plan.h},{plan.w}) windows, got {tuple(win.shape)}")
    win = torch.nn.functional.pad(win, (0, plan.Wp - plan.w, 0, plan.Hp - plan.h))
    rows = []
    for ay in plan.ys:
        rows.append(torch.stack([fn(win[..., ay:ay + plan.th, ax:ax + plan.tw].contiguous()).float() for ax in plan.xs], 1))
    return blend_host(torch.stack(rows, 1), plan)


# ---- static tiles: the specification --------------------------------------------------------------------------------------------

def _index_rows(rows) -> List[List[int]]:
    rows = [[int(j) for j in r] for r in rows]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError(f"rows: b >= 1 rows of equal length T >= 1, got {rows}")
    return rows


def static_pairs(rows) -> List[Tuple[int, int]]:
    """The frame pairs ``static_tiles`` has to compare for a group of index rows (b rows of T frame numbers): the unique unordered
    pairs ``(fa, fb)``, ``fa < fb``, of ``rows[r][i]`` and ``rows[r - 1][i]`` for r >= 1 that are different numbers, sorted.  The
    same number on both sides is the same frame and is not compared."""
    rows = _index_rows(rows)
    return sorted({(min(a, b), max(a, b)) for prev, row in zip(rows, rows[1:]) for a, b in zip(prev, row) if a != b})


def static_sources(E, pairs, rows) -> np.ndarray:
    """``src`` (b,ny,nx) int32: the row whose COMPUTED tile output tile (ky,kx) of row r uses.  `E` (P,ny,nx): nonzero where the
    two frames of ``pairs[p]`` (`static_pairs` of `rows`) are bit-identical on the tile's rectangle.  Row 0 computes everything
    (``src[0] = 0``); tile (ky,kx) of row r >= 1 is static iff for every i the frames ``rows[r][i]`` and ``rows[r - 1][i]`` are the
    same number or an equal pair on that tile, and then ``src[r] = src[r - 1]`` - a chain ends at a computed tile -, else
    ``src[r] = r``."""
    rows = _index_rows(rows)
    E = np.asarray(E).astype(bool)
    pairs = [(int(a), int(b)) for a, b in pairs]
    if E.ndim != 3 or E.shape[0] != len(pairs):
        raise ValueError(f"E: expected ({len(pairs)},ny,nx), got {E.shape}")
    where = {p: k for k, p in enumerate(pairs)}
    src = np.zeros((len(rows),) + E.shape[1:], dtype=np.int32)
    for r in range(1, len(rows)):
        static = np.ones(E.shape[1:], dtype=bool)
        for a, b in zip(rows[r - 1], rows[r]):
            if a != b:
                static &= E[where[(min(a, b), max(a, b))]]
        src[r] = np.where(static, src[r - 1], r)
    return src


def _raw_bytes(frames) -> np.ndarray:
    """(N,C,h,w) frames as stored -> (N,C,h,w,itemsize) uint8."""
    if isinstance(frames, torch.Tensor):
        frames = hip.bits16(frames.detach().cpu()).contiguous().numpy()
    a = np.ascontiguousarray(frames)
    if a.ndim != 4:
        raise ValueError(f"expected (N,C,h,w) frames, got {a.shape}")
    return a.view(np.uint8).reshape(*a.shape, a.dtype.itemsize)


def static_map_host(frames, rows, plan: TilePlan) -> np.ndarray:
    """The whole specification of ``static_tiles`` on CPU frames: `frames` (N,C,h,w) - a CPU tensor or numpy array, uint8, uint16 or
    f32 -, `rows` the b index rows of one group, `plan` the `TilePlan` of h x w.  Returns `static_sources` of the exact comparison:
    a pair is equal on tile (ky,kx) iff the two frames hold the same bits - bytes, raw 16-bit words, 32-bit patterns - in all
    channels on ``[ay, min(ay + th, h)) x [ax, min(ax + tw, w))``.  ``(src == arange(b)[:, None, None])`` marks the tiles that run."""
    raw = _raw_bytes(frames)
    if raw.shape[2:4] != (plan.h, plan.w):
        raise ValueError(f"frames {raw.shape[:4]} do not fit the plan ({plan.h} x {plan.w})")
    rows = _index_rows(rows)
    if any(not 0 <= j < raw.shape[0] for r in rows for j in r):
        raise ValueError(f"rows: frame numbers in 0..{raw.shape[0] - 1}, got {rows}")
    pairs = static_pairs(rows)
    E = np.zeros((len(pairs), plan.ny, plan.nx), dtype=bool)
    for p, (fa, fb) in enumerate(pairs):
        for ky, ay in enumerate(plan.ys):
            for kx, ax in enumerate(plan.xs):
                y1, x1 = min(ay + plan.th, plan.h), min(ax + plan.tw, plan.w)
                E[p, ky, kx] = np.array_equal(raw[fa, :, ay:y1, ax:x1], raw[fb, :, ay:y1, ax:x1])
    return static_sources(E, pairs, rows)


def _graph_chunk(n: int, batch: int) -> int:
    """The pass size for a last chunk of n < batch windows under ``use_graph``: the next power of two, at most `batch`."""
    return min(1 << (n - 1).bit_length(), batch)


class TiledSuperResolver(Resolver):
    """Tiled inference around a model of this package; see the module docstring for the semantics.

    ``tsr = TiledSuperResolver(model, tile, tile_overlap=16, ensemble=None, batch=8)``; ``tsr(win)`` takes a (B,T,C,H,W) f32, uint8
    or uint16 window on the model's device (any H, W) and returns the f32 (B,C,4H,4W) blend; `super_resolve_u8` /
    `super_resolve_u16` return it quantised as ``model.super_resolve_u8`` / ``_u16`` quantise; `sequence` takes the resident
    sequence and window index rows instead of windows (`steps.Resolver`).  ``ensemble``: None, "spatial" or "spatial+temporal" -
    every tile window then goes through the `SelfEnsemble` of the model.  ``batch``: the most tile windows of one model pass; every
    call takes ``batch=`` to override it.  ``static_tiles=True``: inside a `sequence` call of b > 1 rows, a tile window whose frames
    hold the same bits as those of the previous row's is not run again (module docstring: exact, and capped at a factor b because
    nothing is carried from one call to the next).  ``tiles_total`` / ``tiles_run`` count the tile windows delivered / run through
    the per-window function since the caller last reset them."""

    def __init__(self, model, tile, tile_overlap=16, ensemble: Optional[str] = None, batch: int = 8, static_tiles: bool = False):
        chk = check_tile(tile, tile_overlap)
        if chk is None:
            raise ValueError("TiledSuperResolver needs a tile size, got tile=None")
        self.tile, self.tile_overlap = chk
        self.model, self.batch = model, batch
        self.ensemble = check_mode(ensemble)
        self.static_tiles = bool(static_tiles)
        self.tiles_total = self.tiles_run = 0          # tile windows delivered / run through the model; the caller resets them
        self._fn = model if ensemble is None else SelfEnsemble(model, temporal=ensemble == "spatial+temporal")

    def plan(self, h: int, w: int) -> TilePlan:
        return tile_plan(h, w, self.tile, self.tile_overlap)

    @torch.no_grad()
    def sequence(self, frames: torch.Tensor, idx: Sequence[Sequence[int]], *, dtype: torch.dtype = torch.float32,
                 quantise: Optional[str] = None, batch: Optional[int] = None) -> torch.Tensor:
        """`frames`: the dense UNPADDED sequence (N,C,h,w) on the model's device, f32 in [0,1], uint8, or uint16 (10-bit samples;
        integer samples enter as the floats of ``hip.u8_table`` / ``hip.u16_table``).  `idx`: b rows of T frame numbers
        (`harness.windows.window_indices`).  Returns (b,C,4h,4w): the f32 blend, or - `dtype` uint8 / uint16 with `quantise` - its
        quantised frames.  The ``b * ny * nx`` tile windows go through the model's float ``forward`` (or its `SelfEnsemble`),
        without autograd, in chunks of at most `batch` windows (default: the constructor's)."""
        rows = self._rows(frames, idx, dtype, quantise)
        batch = self.batch if batch is None else batch
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        C, h, w = frames.shape[1:]
        if frames.dtype not in (torch.uint8, torch.uint16):
            frames = frames.float()
        plan = self.plan(h, w)
        table = torch.tensor(rows, dtype=torch.int32).to(frames.device)
        self.tiles_total += len(rows) * plan.ny * plan.nx
        if self.static_tiles and len(rows) > 1:
            return self._sequence_static(frames, rows, table, plan, batch, dtype, quantise)
        wins = hip.tile_windows(frames, table, plan).flatten(0, 2)            # (b ny nx, T, C, th, tw)
        n = wins.shape[0]
        self.tiles_run += n
        outs = torch.empty((n, C, SCALE * plan.th, SCALE * plan.tw), dtype=torch.float32, device=frames.device)
        for s in range(0, n, batch):
            outs[s:s + batch] = self._fn(wins[s:s + batch])
        return hip.tile_merge(outs.unflatten(0, (len(rows), plan.ny, plan.nx)), plan, h, w, dtype=dtype, quantise=quantise)

    def _sequence_static(self, frames, rows, table, plan: TilePlan, batch: int, dtype, quantise) -> torch.Tensor:
        """`sequence` with ``static_tiles`` for b > 1 rows: compare (`hip.tile_pairs_equal`), one small download - the one host
        synchronisation of the group -, `static_sources`, then only the computed tile windows, in row-major (row, ky, kx) order,
        are gathered and run, and the merge reads every tile through the slot table.  Under ``model.use_graph`` the passes are
        full chunks of `batch` and a last chunk padded to the next power of two by repeating its last window, so at most
        ``1 + log2(batch)`` pass sizes are ever captured; eager runs use the exact remainder."""
        dev, b, C = frames.device, len(rows), frames.shape[1]
        pairs = static_pairs(rows)
        if pairs:
            E = hip.tile_pairs_equal(frames, torch.tensor(pairs, dtype=torch.int32).to(dev), plan).cpu().numpy()
        else:
            E = np.zeros((0, plan.ny, plan.nx), dtype=np.uint8)
        src = static_sources(E, pairs, rows)
        run = src == np.arange(b, dtype=np.int32)[:, None, None]
        sel = np.argwhere(run).astype(np.int32)                               # (n,3) rows (r, ky, kx), row-major
        n = sel.shape[0]
        slot = np.zeros(src.shape, dtype=np.int32)
        slot[run] = np.arange(n, dtype=np.int32)
        slots = np.take_along_axis(slot, src, 0)                              # the slot of the computed tile each tile uses
        wins = hip.tile_windows(frames, table, plan, sel=torch.from_numpy(sel).to(dev))      # (n, T, C, th, tw)
        pool = torch.empty((n, C, SCALE * plan.th, SCALE * plan.tw), dtype=torch.float32, device=dev)
        graph = bool(getattr(self.model, "use_graph", False))
        for s in range(0, n, batch):
            chunk = wins[s:s + batch]
            m = chunk.shape[0]
            if graph and m < batch and _graph_chunk(m, batch) > m:
                chunk = torch.cat([chunk, chunk[-1:].expand(_graph_chunk(m, batch) - m, *chunk.shape[1:])], 0)
            pool[s:s + m] = self._fn(chunk)[:m]
        self.tiles_run += n
        return hip.tile_merge(pool, plan, h=plan.h, w=plan.w, dtype=dtype, quantise=quantise, src=torch.from_numpy(slots).to(dev))


def check_static_tiles(static_tiles, tile) -> bool:
    """The ``static_tiles=`` keyword: a bool, and True only together with ``tile=``; anything else is a ValueError."""
    if not isinstance(static_tiles, (bool, np.bool_)):
        raise ValueError(f"static_tiles must be True or False, got {static_tiles!r}")
    if static_tiles and tile is None:
        raise ValueError("static_tiles=True needs tile=: reuse is per tile window")
    return bool(static_tiles)


def resolver_for(model, ensemble: Optional[str], tile, tile_overlap=16, batch: int = 8, static_tiles: bool = False) -> Resolver:
    """What the harness entry points run a batch of windows through, from their ``ensemble=`` / ``tile=`` / ``tile_overlap=`` /
    ``static_tiles=`` values (validated here, before any device work): the `PlainResolver` of the model, the `SelfEnsemble` of
    ``ensemble`` without tiles, or a `TiledSuperResolver` whose model passes take at most `batch` windows.  Always a
    `steps.Resolver`."""
    from .ensemble import for_mode
    check_mode(ensemble)
    static_tiles = check_static_tiles(static_tiles, tile)
    if check_tile(tile, tile_overlap) is None:
        return PlainResolver(model) if ensemble is None else for_mode(model, ensemble)
    return TiledSuperResolver(model, tile, tile_overlap, ensemble, batch, static_tiles)


def tile_counts(resolver: Resolver) -> dict:
    """``{"tiles_total", "tiles_run"}`` of the `TiledSuperResolver` a harness run used with ``static_tiles=True`` - the resolver
    itself or the one inside an `ActiveResolver` -, {} for any other run."""
    inner = getattr(resolver, "inner", resolver)
    if isinstance(inner, TiledSuperResolver) and inner.static_tiles:
        return {"tiles_total": inner.tiles_total, "tiles_run": inner.tiles_run}
    return {}
