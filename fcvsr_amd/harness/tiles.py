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

Out of scope: `StreamedSuperResolver` and ``fit(..., val_sequences=...)`` take no tile option; there is no temporal tiling and no
automatic choice of the tile size.
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


class TiledSuperResolver(Resolver):
    """Tiled inference around a model of this package; see the module docstring for the semantics.

    ``tsr = TiledSuperResolver(model, tile, tile_overlap=16, ensemble=None, batch=8)``; ``tsr(win)`` takes a (B,T,C,H,W) f32, uint8
    or uint16 window on the model's device (any H, W) and returns the f32 (B,C,4H,4W) blend; `super_resolve_u8` /
    `super_resolve_u16` return it quantised as ``model.super_resolve_u8`` / ``_u16`` quantise; `sequence` takes the resident
    sequence and window index rows instead of windows (`steps.Resolver`).  ``ensemble``: None, "spatial" or "spatial+temporal" -
    every tile window then goes through the `SelfEnsemble` of the model.  ``batch``: the most tile windows of one model pass; every
    call takes ``batch=`` to override it."""

    def __init__(self, model, tile, tile_overlap=16, ensemble: Optional[str] = None, batch: int = 8):
        chk = check_tile(tile, tile_overlap)
        if chk is None:
            raise ValueError("TiledSuperResolver needs a tile size, got tile=None")
        self.tile, self.tile_overlap = chk
        self.model, self.batch = model, batch
        self.ensemble = check_mode(ensemble)
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
        wins = hip.tile_windows(frames, table, plan).flatten(0, 2)            # (b ny nx, T, C, th, tw)
        n = wins.shape[0]
        outs = torch.empty((n, C, SCALE * plan.th, SCALE * plan.tw), dtype=torch.float32, device=frames.device)
        for s in range(0, n, batch):
            outs[s:s + batch] = self._fn(wins[s:s + batch])
        return hip.tile_merge(outs.unflatten(0, (len(rows), plan.ny, plan.nx)), plan, h, w, dtype=dtype, quantise=quantise)


def resolver_for(model, ensemble: Optional[str], tile, tile_overlap=16, batch: int = 8) -> Resolver:
    """What the harness entry points run a batch of windows through, from their ``ensemble=`` / ``tile=`` / ``tile_overlap=``
    values (validated here, before any device work): the `PlainResolver` of the model, the `SelfEnsemble` of ``ensemble`` without
    tiles, or a `TiledSuperResolver` whose model passes take at most `batch` windows.  Always a `steps.Resolver`."""
    from .ensemble import for_mode
    check_mode(ensemble)
    if check_tile(tile, tile_overlap) is None:
        return PlainResolver(model) if ensemble is None else for_mode(model, ensemble)
    return TiledSuperResolver(model, tile, tile_overlap, ensemble, batch)
