"""The two tolerance helpers the f64-reference tests share: the summation bound tau(n) and the worst error-to-condition ratio."""
import math

import torch


def tau(n: int) -> float:
    return 2.0 ** -16 if n <= 4096 else 2.0 ** -22 * math.sqrt(n)


def worst_ratio(got, ref, S):
    """max over entries of |got - ref| / S; an entry with S = 0 must be exact."""
    err = (got.double().cpu() - ref).abs()
    r = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0
