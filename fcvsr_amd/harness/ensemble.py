"""Test-time self-ensemble: the model runs on the 8 flips / transposes of a window and the 8 results are flipped back and averaged
(the reference's ``SpatialTemporalEnsemble``, mmedit_train/mmedit/models/common/ensemble.py, wired into its restorers by
``ensemble=dict(type='SpatialTemporalEnsemble', is_temporal_ensemble=False)``, restorers/basicvsr.py:53-65,176-177).

Semantics.  Variant ``i`` in 0..7 of a frame (h x w, any leading dimensions) is built in this order: ``i & 1`` reverses the columns
(the reference's 'vertical', ``flip(4)``), ``i & 2`` reverses the rows ('horizontal'), ``i & 4`` transposes h and w - the list order
of the reference class.  The inverse on a model output undoes them in the opposite order: transpose, reverse rows, reverse columns.
With ``o_i = restore(model(variant(win, i)), i)`` in f32 the mean is a fixed-order sum: ``acc = o_0``, ``acc = acc + o_i`` for i =
1..7 (each sum rounded once, no FMA), ``mean8 = acc * 0.125``.  The reference takes ``torch.stack(...).mean(0)``, whose summation
order is not promised; the two agree to a few f32 roundings.

Padding.  The model needs frame sides that are multiples of 4; the harness pads with zeros at the bottom / right and crops the SR
frame.  Under ensemble every variant is made from the UNPADDED frame and padded at its own bottom / right (a transposed variant of
h x w is w x h padded to ceil4(w) x ceil4(h)), and the model output is cropped to its own top-left 4h x 4w (4w x 4h) before the
inverse transform: every pass sees what a plain run on the flipped video would see.

Temporal option (``temporal=True``, the harness's ``ensemble="spatial+temporal"``): sixteen passes.  Passes 8..15 are the same eight
variants of the time-reversed window ``win.flip(1)``; their outputs are restored spatially only, and the result is
``(mean8_fwd + mean8_rev) * 0.5``.  This is an extension of this project: the reference's temporal mode flips a (n,t,c,h,w) OUTPUT
along t and cannot run on a model with a one-frame output (its ``_transform`` raises for 4-D tensors when the mode is on, and its
``outputs.flip(1)`` would flip channels).

`variant_host`, `restore_host` and `ensemble_host` are the specification (numpy arrays or CPU torch tensors), not a code path:
`SelfEnsemble` runs on the HIP device only.  Two kernels do the data movement (csrc/ensemble.hip): ``hip.ensemble_windows`` builds
all 8 variants of a batch of windows straight from the resident sequence through an index table (the plain windows are never
materialised), the model's unchanged float ``forward`` runs on the two 4b-window batches it produced, and ``hip.ensemble_merge``
crops, restores, sums in the fixed order and quantises.  The results equal the specification bit for bit.

hipGraph capture (``model.use_graph``) and ``model.streams`` apply to the model calls as usual.  A frame with H != W gives the model
two input shapes per batch size (4b x H x W and 4b x W x H), i.e. twice the captured graphs of a plain run against
``model.graph_cache_size`` (default 4): raise it when ragged last batches are also in play.

Out of scope: `StreamedSuperResolver` and ``fit(..., val_sequences=...)`` take no ensemble option.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

from .. import hip
from .steps import Resolver

MODES = (None, "spatial", "spatial+temporal")


def check_mode(ensemble: Optional[str]) -> Optional[str]:
    """The harness keyword: None (no ensemble), "spatial" (8 passes) or "spatial+temporal" (16); anything else raises."""
    if ensemble not in MODES:
        raise ValueError(f'ensemble must be None, "spatial" or "spatial+temporal", got {ensemble!r}')
    return ensemble


def _is_np(a) -> bool:
    return isinstance(a, np.ndarray)


def _flip(a, axis):
    return np.flip(a, axis) if _is_np(a) else a.flip(axis)


def _transpose(a):
    return np.swapaxes(a, -1, -2) if _is_np(a) else a.transpose(-1, -2)


def _dense(a):
    return np.ascontiguousarray(a) if _is_np(a) else a.contiguous()


def variant_host(a, i: int):
    """Variant i (0..7) of the frames in the last two dimensions of `a` (numpy or CPU torch): reverse columns if ``i & 1``, then
    reverse rows if ``i & 2``, then transpose if ``i & 4``."""
    if not 0 <= i < 8:
        raise ValueError(f"variant index must be in 0..7, got {i}")
    if i & 1:
        a = _flip(a, -1)
    if i & 2:
        a = _flip(a, -2)
    if i & 4:
        a = _transpose(a)
    return _dense(a)


def restore_host(a, i: int):
    """The inverse of `variant_host` applied to a model output: transpose if ``i & 4``, then reverse rows if ``i & 2``, then
    reverse columns if ``i & 1``."""
    if not 0 <= i < 8:
        raise ValueError(f"variant index must be in 0..7, got {i}")
    if i & 4:
        a = _transpose(a)
    if i & 2:
        a = _flip(a, -2)
    if i & 1:
        a = _flip(a, -1)
    return _dense(a)


def _mean8_host(win: torch.Tensor, fn: Callable, multiple: int) -> torch.Tensor:
    acc = None
    for i in range(8):
        v = variant_host(win, i)
        vh, vw = v.shape[-2:]
        v = torch.nn.functional.pad(v, (0, (-vw) % multiple, 0, (-vh) % multiple))
        o = fn(v).float()
        s = o.shape[-1] // v.shape[-1]                                # the model's scale
        o = restore_host(o[..., :s * vh, :s * vw], i)
        acc = o if acc is None else acc + o                           # one f32 rounding per sum, in this order
    return acc * 0.125


def ensemble_host(win: torch.Tensor, fn: Callable, temporal: bool = False, multiple: int = 1) -> torch.Tensor:
    """The specification of the self-ensemble: `win` (B,T,C,H,W) f32 CPU tensor, `fn` the model as a function of a window
    (B,T,C,H',W') -> (B,C,sH',sW').  Every variant is zero-padded at its own bottom / right to a multiple of `multiple` and the
    output cropped to its top-left before the inverse transform (``multiple=4``: the harness's padding rule).  ``temporal``:
    ``(mean8(win) + mean8(win.flip(1))) * 0.5``."""
    win = win.float()
    out = _mean8_host(win, fn, multiple)
    if temporal:
        out = (out + _mean8_host(win.flip(1), fn, multiple)) * 0.5
    return out


class SelfEnsemble(Resolver):
    """x8 (x16 with ``temporal``) self-ensemble around a model of this package; see the module docstring for the semantics.

    ``ens = SelfEnsemble(model)``; ``ens(win)`` takes a (B,T,C,H,W) f32, uint8 or uint16 window on the model's device (any H, W:
    the variants are padded to multiples of 4 inside) and returns the f32 (B,C,4H,4W) mean; `super_resolve_u8` /
    `super_resolve_u16` return it quantised as ``model.super_resolve_u8`` / ``_u16`` quantise; `sequence` takes the resident
    sequence and window index rows instead of windows (`steps.Resolver`)."""

    def __init__(self, model, temporal: bool = False):
        self.model, self.temporal = model, bool(temporal)

    @torch.no_grad()
    def sequence(self, frames: torch.Tensor, idx: Sequence[Sequence[int]], *, dtype: torch.dtype = torch.float32,
                 quantise: Optional[str] = None) -> torch.Tensor:
        """`frames`: the dense UNPADDED sequence (N,C,h,w) on the model's device, f32 in [0,1], uint8, or uint16 (10-bit samples;
        integer samples enter as the floats of ``hip.u8_table`` / ``hip.u16_table``).  `idx`: b rows of T frame numbers
        (`harness.windows.window_indices`).  Returns (b,C,4h,4w): the f32 mean, or - `dtype` uint8 / uint16 with `quantise` - its
        quantised frames.  The model always runs without autograd (with gradients enabled its ``forward`` is the training graph),
        through its float ``forward``, on the two batches of 4b windows the gather kernel made."""
        rows = self._rows(frames, idx, dtype, quantise)
        h, w = frames.shape[-2:]
        if frames.dtype not in (torch.uint8, torch.uint16):
            frames = frames.float()
        table = torch.tensor(rows, dtype=torch.int32).to(frames.device)
        outs = []
        for reverse in ((False, True) if self.temporal else (False,)):
            va, vt = hip.ensemble_windows(frames, table, reverse=reverse)
            outs += [self.model(v.flatten(0, 1)).unflatten(0, (4, len(rows))) for v in (va, vt)]
        return hip.ensemble_merge(outs[0], outs[1], h, w, ra=outs[2] if self.temporal else None,
                                  rat=outs[3] if self.temporal else None, dtype=dtype, quantise=quantise)


def for_mode(model, ensemble: Optional[str]) -> Optional[SelfEnsemble]:
    """The `SelfEnsemble` of a harness ``ensemble=`` value, None for None."""
    return None if check_mode(ensemble) is None else SelfEnsemble(model, temporal=ensemble == "spatial+temporal")
