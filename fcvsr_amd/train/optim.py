"""Adam over the flat buffers in one launch (csrc/optim.hip), and its specification in numpy float32.

`FlatGradAllReduce` keeps every gradient in one flat f32 buffer.  `HipAdam` keeps the two moments in two more with the same offsets
and updates every parameter with ONE kernel launch (torch's multi-tensor Adam walks the 295 tensors of the S model in several
launches per operation), then advances the parameters' version counters, which the inference engine's packed-weight cache is keyed on
(torch's fused=True Adam leaves them alone, which is why `TrainStep` cannot use it).  The optimizer state is two tensors, a step count
and a learning rate: what a resumable checkpoint needs.

`adam_step_host` is the arithmetic, operation by operation; the kernel equals it bit for bit.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from .. import hip


def adam_scalars(t: int, lr: float, betas: Tuple[float, float], eps: float, wd: float) -> Dict[str, np.float32]:
    """The seven f32 kernel arguments of step `t` (counted from 1), each computed in f64 and rounded once."""
    if t < 1:
        raise ValueError(f"the step count starts at 1, got {t}")
    b1, b2 = float(betas[0]), float(betas[1])
    return {"step_size": np.float32(float(lr) / (1.0 - b1 ** t)), "bc2_sqrt": np.float32(math.sqrt(1.0 - b2 ** t)),
            "one_minus_b1": np.float32(1.0 - b1), "b2": np.float32(b2), "one_minus_b2": np.float32(1.0 - b2),
            "eps": np.float32(eps), "wd": np.float32(wd)}


def adam_step_host(p: np.ndarray, g: np.ndarray, m: np.ndarray, v: np.ndarray, t: int, lr: float,
                   betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, wd: float = 0.0):
    """Step `t` of torch.optim.Adam's L2 form (no amsgrad, no decoupled decay) on float32 arrays: returns (p', m', v').  Every line is
    one IEEE f32 operation rounded once (numpy float32 arithmetic: correctly rounded division and square root, subnormals kept):
        g' = g + wd * p
        m' = m + (g' - m) * (1 - b1)
        v' = v * b2 + (g' * g') * (1 - b2)
        den = sqrt(v') / bc2_sqrt + eps
        p' = p - step_size * (m' / den)
    with the scalars of `adam_scalars`.  This is the specification of `fcvsr_adam_multi`."""
    p, g, m, v = (np.asarray(a) for a in (p, g, m, v))
    for a in (p, g, m, v):
        if a.dtype != np.float32:
            raise ValueError(f"float32 arrays only, got {a.dtype}")
    s = adam_scalars(t, lr, betas, eps, wd)
    with np.errstate(all="ignore"):
        wp = s["wd"] * p
        g1 = g + wp
        d = g1 - m
        dm = d * s["one_minus_b1"]
        m1 = m + dm
        vb = v * s["b2"]
        gg = g1 * g1
        gs = gg * s["one_minus_b2"]
        v1 = vb + gs
        r = np.sqrt(v1)
        q = r / s["bc2_sqrt"]
        den = q + s["eps"]
        u = m1 / den
        su = s["step_size"] * u
        p1 = p - su
    assert p1.dtype == np.float32 and m1.dtype == np.float32 and v1.dtype == np.float32
    return p1, m1, v1


class HipAdam:
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) (L2 form, no amsgrad) as one HIP launch per step.

    params: the f32 device parameters, in the order of the flat gradient buffer (`FlatGradAllReduce(params)`); names: one name per
    parameter, the keys of `state_dict()`.  `step(flat_grad)` updates every parameter from the flat gradient buffer on the current
    stream and advances the parameters' version counters.  `lr` is a plain attribute: set it between steps.  `t` is the number of
    steps taken.  CPU parameters raise RuntimeError: there is no CPU fallback (`adam_step_host` is the CPU specification)."""

    def __init__(self, params: Iterable[torch.nn.Parameter], names: Sequence[str], lr: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        self.params: List[torch.Tensor] = list(params)
        self.names = [str(n) for n in names]
        if not self.params:
            raise ValueError("HipAdam got an empty parameter list")
        if len(self.names) != len(self.params) or len(set(self.names)) != len(self.names):
            raise ValueError("HipAdam needs one distinct name per parameter")
        if any(not p.is_cuda for p in self.params):
            raise RuntimeError("HipAdam updates parameters on the HIP device only (there is no CPU fallback; "
                               "fcvsr_amd.train.optim.adam_step_host is the CPU specification)")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0.0 or weight_decay < 0.0 or lr < 0.0:
            raise ValueError(f"invalid Adam hyper-parameters: lr={lr}, betas={betas}, eps={eps}, weight_decay={weight_decay}")
        self.device = self.params[0].device
        for n, p in zip(self.names, self.params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                raise ValueError(f"parameter {n}: HipAdam needs contiguous float32 parameters on one device")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.sizes = [p.numel() for p in self.params]
        self.offsets = [int(o) for o in np.concatenate([[0], np.cumsum(self.sizes)[:-1]])]
        self.numel = int(sum(self.sizes))
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.t = 0
        self._table = None          # (device table, total blocks, the data pointers it was built from)

    def _plan(self):
        ptrs = [p.data_ptr() for p in self.params]
        if self._table is None or self._table[2] != ptrs:
            be = hip.lib().fcvsr_adam_multi_block_elems()
            rows, blk = [], 0
            for n, p, ptr, off, cnt in zip(self.names, self.params, ptrs, self.offsets, self.sizes):
                if ptr % 16 or not p.is_contiguous() or p.dtype != torch.float32 or p.device != self.device:
                    raise ValueError(f"parameter {n}: HipAdam needs 16-byte aligned contiguous float32 storage on {self.device}")
                if cnt == 0:
                    continue
                rows.append([ptr, off, cnt, blk])
                blk += (cnt + be - 1) // be
            if not rows:
                raise ValueError("HipAdam: every parameter is empty")
            tab = torch.tensor(rows, dtype=torch.int64).to(self.device)
            self._table = (tab, blk, ptrs)
        return self._table

    def step(self, flat_grad: torch.Tensor) -> None:
        """One Adam step from `flat_grad`, the flat f32 gradient buffer (numel = the parameters' total, their order)."""
        if (not isinstance(flat_grad, torch.Tensor) or flat_grad.dtype != torch.float32 or flat_grad.dim() != 1
                or flat_grad.numel() != self.numel or not flat_grad.is_contiguous() or flat_grad.device != self.device):
            raise ValueError(f"HipAdam.step needs the contiguous flat float32 gradient buffer of {self.numel} elements on {self.device}")
        for buf in (self.exp_avg, self.exp_avg_sq):
            if buf.numel() != self.numel or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != self.device:
                raise ValueError(f"HipAdam: a moment buffer is not the contiguous float32 buffer of {self.numel} elements on {self.device}")
        tab, blocks, _ = self._plan()
        s = adam_scalars(self.t + 1, self.lr, self.betas, self.eps, self.weight_decay)
        with torch.cuda.device(self.device):
            hip.check(hip.lib().fcvsr_adam_multi(tab.data_ptr(), tab.shape[0], blocks, flat_grad.data_ptr(), self.exp_avg.data_ptr(),
                                                 self.exp_avg_sq.data_ptr(), self.t + 1, float(s["step_size"]), float(s["bc2_sqrt"]),
                                                 float(s["one_minus_b1"]), float(s["b2"]), float(s["one_minus_b2"]), float(s["eps"]),
                                                 float(s["wd"]), hip.stream_ptr()), "fcvsr_adam_multi")
        self.t += 1
        # the kernel wrote through raw pointers: tell autograd and every cache keyed on `_version` (engine.py, WeightPacker)
        torch.autograd.graph.increment_version(self.params)

    def state_dict(self) -> dict:
        """{"kind": "hip_adam", "step", "lr", "betas", "eps", "weight_decay", "exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}}
        with host copies of the moments, keyed by parameter name and shaped like the parameters."""
        def split(flat):
            host = flat.detach().cpu()
            return {n: v.clone().view(p.shape) for n, v, p in zip(self.names, host.split(self.sizes), self.params)}
        return {"kind": "hip_adam", "step": self.t, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
                "weight_decay": self.weight_decay, "exp_avg": split(self.exp_avg), "exp_avg_sq": split(self.exp_avg_sq)}

    def load_state_dict(self, sd: dict) -> None:
        """Accepts `HipAdam.state_dict()`, or `torch.optim.Adam.state_dict()` of an optimizer over the same parameter list in the same
        order (one param group, no amsgrad), so a run started with torch's Adam can switch."""
        if sd.get("kind") == "hip_adam":
            for key in ("exp_avg", "exp_avg_sq"):
                if set(sd[key]) != set(self.names):
                    raise ValueError(f"optimizer state {key}: parameter names differ: {sorted(set(sd[key]) ^ set(self.names))[:4]}")
            moments = [[sd[key][n] for n in self.names] for key in ("exp_avg", "exp_avg_sq")]
            t, lr, betas, eps, wd = sd["step"], sd["lr"], sd["betas"], sd["eps"], sd["weight_decay"]
        elif "param_groups" in sd and "state" in sd:
            groups = sd["param_groups"]
            if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
                raise ValueError("a torch.optim.Adam state_dict must have one param group over the same parameter list")
            grp = groups[0]
            if grp.get("amsgrad") or grp.get("maximize") or grp.get("decoupled_weight_decay"):
                raise ValueError("HipAdam has no amsgrad, maximize or decoupled weight decay")
            state = [sd["state"].get(i) for i in grp["params"]]
            if all(st is None for st in state):                      # an optimizer that has not stepped yet
                moments = [[torch.zeros(p.shape) for p in self.params] for _ in range(2)]
                t = 0
            elif any(st is None for st in state):
                raise ValueError("a torch.optim.Adam state_dict with state for some parameters only")
            else:
                steps = {int(st["step"]) for st in state}
                if len(steps) != 1:
                    raise ValueError(f"a torch.optim.Adam state_dict whose parameters took different numbers of steps: {sorted(steps)}")
                t = steps.pop()
                moments = [[st[key] for st in state] for key in ("exp_avg", "exp_avg_sq")]
            lr, betas, eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
        else:
            raise ValueError("neither a HipAdam state_dict nor a torch.optim.Adam state_dict")
        for key, tensors in zip(("exp_avg", "exp_avg_sq"), moments):
            for n, p, v in zip(self.names, self.params, tensors):
                if tuple(v.shape) != tuple(p.shape) or v.dtype != torch.float32:
                    raise ValueError(f"optimizer state {key}[{n}]: expected float32 {tuple(p.shape)}, got {v.dtype} {tuple(v.shape)}")
        for flat, tensors in zip((self.exp_avg, self.exp_avg_sq), moments):
            flat.copy_(torch.cat([v.detach().reshape(-1).cpu() for v in tensors]))
        self.t, self.lr, self.betas, self.eps, self.weight_decay = int(t), float(lr), (float(betas[0]), float(betas[1])), float(eps), float(wd)
