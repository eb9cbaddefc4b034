#!/usr/bin/env python3
"""Generate tests/golden/lr_schedules.json from the schedulers themselves (build container only).

Usage:  python tests/golden/make_golden_lr.py            (needs /root/reference; CPU, seconds)

`CosineAnnealingRestartLR` is imported read-only from /root/reference/CVSR_train/opt/deep_learning.py (the module needs torch and
numpy only), `MultiStepLR` from torch.  Short schedules are stepped live, one `optimizer.step(); scheduler.step()` per position, and
the learning rate of the optimizer's param group is recorded at every position.  The 600 000-iteration schedules of the two FCVSR
configs (mmedit_train/configs/restorers/fcvsr/fcvsr_s_redsLD_QP22.py:93-107 and fcvsr_redsLD_QP22.py:112-128) are sampled: the
reference's `get_lr()` is a function of `last_epoch` alone, so the script sets `last_epoch` to each sampled iteration and records
`get_lr()`.  Nothing of the reference is written into the repository: the fixture holds settings and recorded numbers.
"""
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OPT = "/root/reference/CVSR_train/opt"

COSINE_LIVE = [
    dict(base_lr=1e-4, periods=[6, 4], restart_weights=[1, 0.5], min_lr=1e-7),
    dict(base_lr=2e-4, periods=[5, 5, 7], restart_weights=[1, 0.5, 0.25], min_lr=0.0),
    dict(base_lr=1e-5, periods=[12], restart_weights=[1], min_lr=1e-7),
]
COSINE_SAMPLED = [        # the two FCVSR configs: periods=[total_iters], restart_weights=[1], min_lr=1e-7
    dict(base_lr=1e-5, periods=[600000], restart_weights=[1], min_lr=1e-7),
    dict(base_lr=0.5 * 1e-5, periods=[600000], restart_weights=[1], min_lr=1e-7),
]
SAMPLES = [0, 1, 2, 99, 100, 4999, 5000, 5001, 150000, 299999, 300000, 300001, 450000, 599998, 599999, 600000]
MULTISTEP = [
    dict(base_lr=1e-4, milestones=[2000, 8000, 12000, 20000], gamma=0.5, positions=[0, 1, 1999, 2000, 2001, 7999, 8000, 12000, 19999, 20000, 30000]),
    dict(base_lr=1e-3, milestones=[3, 7, 7, 12], gamma=0.1, positions=list(range(16))),
    dict(base_lr=3e-4, milestones=[1], gamma=0.3, positions=list(range(5))),
]


def _optimizer(base_lr):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_OPT)
    import deep_learning as ref
    warnings.simplefilter("ignore")
    out = {"cosine_restart": [], "multistep": []}
    for cfg in COSINE_LIVE:
        opt = _optimizer(cfg["base_lr"])
        sched = ref.CosineAnnealingRestartLR(opt, periods=list(cfg["periods"]), restart_weights=list(cfg["restart_weights"]),
                                             eta_min=cfg["min_lr"])
        its, lrs = [], []
        total = sum(cfg["periods"])
        for it in range(total + 1):
            its.append(it)
            lrs.append(float(opt.param_groups[0]["lr"]))
            if it < total:                                   # (the reference scheduler has no value past its last period)
                opt.step()
                sched.step()
        out["cosine_restart"].append(dict(cfg, it=its, lr=lrs, how="live"))
    for cfg in COSINE_SAMPLED:
        opt = _optimizer(cfg["base_lr"])
        sched = ref.CosineAnnealingRestartLR(opt, periods=list(cfg["periods"]), restart_weights=list(cfg["restart_weights"]),
                                             eta_min=cfg["min_lr"])
        lrs = []
        for it in SAMPLES:
            sched.last_epoch = it
            (lr,) = sched.get_lr()
            lrs.append(float(lr))
        out["cosine_restart"].append(dict(cfg, it=SAMPLES, lr=lrs, how="get_lr at last_epoch"))
    for cfg in MULTISTEP:
        opt = _optimizer(cfg["base_lr"])
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(cfg["milestones"]), gamma=cfg["gamma"])
        want, lrs = set(cfg["positions"]), {}
        for n in range(max(want) + 1):
            if n in want:
                lrs[n] = float(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        cfg = dict(cfg)
        pos = cfg.pop("positions")
        out["multistep"].append(dict(cfg, n=pos, lr=[lrs[n] for n in pos]))
    path = os.path.join(HERE, "lr_schedules.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
