"""Learning-rate schedules as pure functions of the position: no state, so nothing to save and nothing to get wrong on a resume.

`multistep_lr` is the epoch loop's schedule (reference CVSR_train/train_LD_freqCVSR_S_22.py:205: MultiStepLR), `cosine_restart_lr` the
iteration loop's (reference CVSR_train/opt/deep_learning.py:289-358 CosineAnnealingRestartLR = mmcv's CosineRestart, the
`lr_config` of the mmedit configs: periods=[total_iters], restart_weights=[1], min_lr=1e-7).
tests/golden/lr_schedules.json holds both as recorded from torch's and the reference's scheduler classes.
"""
from __future__ import annotations

import math
from typing import Sequence


def multistep_lr(base_lr: float, milestones: Sequence[int], gamma: float, n: int) -> float:
    """The learning rate torch.optim.lr_scheduler.MultiStepLR(milestones, gamma) holds after `n` calls of scheduler.step():
    base_lr * gamma ** (number of milestones <= n, repeated milestones counted as often as they repeat)."""
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    return float(base_lr) * float(gamma) ** sum(1 for m in milestones if m <= n)


def cosine_restart_lr(base_lr: float, periods: Sequence[int], restart_weights: Sequence[float], min_lr: float, it: int) -> float:
    """Cosine annealing with restarts at iteration `it` (the reference scheduler's value after `it` steps):
        min_lr + w_k * 0.5 * (base_lr - min_lr) * (1 + cos(pi * (it - start_k) / periods[k]))
    with k the first cycle whose cumulative end is >= it (an iteration ON a boundary closes the old cycle: its lr is min_lr, the
    restart shows one iteration later) and start_k the sum of the periods before it."""
    if len(periods) != len(restart_weights) or not len(periods):
        raise ValueError("periods and restart_weights should have the same, non-zero length")
    if not (0 <= it <= sum(periods)):
        raise ValueError(f"iteration {it} outside the schedule's {sum(periods)} iterations")
    start = 0
    for period, weight in zip(periods, restart_weights):
        if it <= start + period:
            return min_lr + weight * 0.5 * (base_lr - min_lr) * (1 + math.cos(math.pi * ((it - start) / period)))
        start += period
    raise AssertionError("unreachable")


SCHEDULES = {"multistep": multistep_lr, "cosine_restart": cosine_restart_lr}


def schedule_lr(schedule: dict, base_lr: float, it: int) -> float:
    """The learning rate of position `it` under `schedule` = {"name": "cosine_restart" | "multistep", **its arguments} (the form kept
    in a checkpoint)."""
    args = dict(schedule)
    name = args.pop("name")
    if name not in SCHEDULES:
        raise ValueError(f"unknown schedule {name!r}: one of {sorted(SCHEDULES)}")
    return SCHEDULES[name](base_lr, it=it, **args) if name == "cosine_restart" else SCHEDULES[name](base_lr, n=it, **args)
