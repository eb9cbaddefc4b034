"""Training checkpoints a run can continue from: one file `iter_%d.pth` per saved iteration.

A file holds {"iter", "model", "train_step", "schedule", "sampler", "loss_history"}:
    iter          number of updates done
    model         the plain `model.state_dict()` in the reference schema (loads strict=True into the reference classes)
    train_step    `TrainStep.state_dict()`: the optimizer state (moments, step count, learning rate) and the meta a resume must match
    schedule      {"name": ..., **arguments} of `fcvsr_amd.train.schedule`
    sampler       {"seed", "len", "batches", "world"}: what fixes the data order
    loss_history  the loss of every iteration so far
It is written under a temporary name in the same directory and moved into place with os.replace, so a kill in mid-write costs the
file being written and never an earlier one; `latest` only ever sees complete files.
"""
from __future__ import annotations

import os
import re
from typing import List, Optional

import torch

_NAME = re.compile(r"^iter_(\d+)\.pth$")
_TMP_SUFFIX = ".tmp"


def checkpoint_path(ckpt_dir: str, it: int) -> str:
    return os.path.join(ckpt_dir, "iter_%d.pth" % it)


def _iterations(ckpt_dir: str) -> List[int]:
    if not os.path.isdir(ckpt_dir):
        return []
    return sorted(int(m.group(1)) for m in (_NAME.match(f) for f in os.listdir(ckpt_dir)) if m)


def latest(ckpt_dir: str) -> Optional[str]:
    """Path of the complete checkpoint with the highest iteration in `ckpt_dir`, or None (temporary files of an interrupted write
    and other files are ignored)."""
    its = _iterations(ckpt_dir)
    return checkpoint_path(ckpt_dir, its[-1]) if its else None


def save_checkpoint(ckpt_dir: str, it: int, payload: dict, keep: Optional[int] = None, writer=torch.save) -> str:
    """Write `payload` (with "iter" = it) to `ckpt_dir/iter_<it>.pth` atomically, then remove all but the `keep` newest checkpoints
    (None or 0: keep all).  Call it on rank 0 only.  writer(obj, path): torch.save; a writer that raises leaves the directory's
    complete checkpoints as they were."""
    if keep is not None and keep < 0:
        raise ValueError(f"keep must be >= 0 or None, got {keep}")
    os.makedirs(ckpt_dir, exist_ok=True)
    final = checkpoint_path(ckpt_dir, it)
    tmp = final + _TMP_SUFFIX + ".%d" % os.getpid()
    try:
        writer(dict(payload, iter=int(it)), tmp)
        os.replace(tmp, final)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    if keep:
        for old in _iterations(ckpt_dir)[:-keep]:
            if old != it:
                os.remove(checkpoint_path(ckpt_dir, old))
    return final


def load_checkpoint(path: str) -> dict:
    """The payload of `save_checkpoint`, tensors on the host (every rank loads the same file: the update is replicated, so the
    moments are the same on all ranks)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    for key in ("iter", "model", "train_step", "schedule", "sampler", "loss_history"):
        if key not in ckpt:
            raise ValueError(f"{path} is not a training checkpoint: no `{key}` entry")
    return ckpt
