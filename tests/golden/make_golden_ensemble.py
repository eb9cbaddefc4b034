#!/usr/bin/env python3
"""Record what the REFERENCE's self-ensemble does (build container only): the order of its eight variants and of their inverses.

Usage:  python tests/golden/make_golden_ensemble.py        (needs /root/reference; CPU, a second)

The reference class (mmedit_train/mmedit/models/common/ensemble.py, SpatialTemporalEnsemble) imports with torch alone and is loaded
read-only by file path.  ``SpatialTemporalEnsemble(False)`` runs on a seeded (1,7,2,6,10) window with a stand-in model that is NOT
equivariant under flips or transposes (a x4 nearest up-sampling of frame 3 plus half of frame 0, times a ramp over the output's own
grid), so a wrong variant, a wrong inverse or a wrong pairing of the two changes the result.  Stored in ensemble_order.npz: the
window (``x``), the eight tensors the model was handed in call order (``in_0`` .. ``in_7``) and the class's output (``out``).  Nothing
of the reference's text is written into the repository: data only.  tests/test_ensemble_cpu.py restates the stand-in model.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mmedit_train/mmedit/models/common/ensemble.py"


def standin(t: torch.Tensor) -> torch.Tensor:
    """(B,7,C,H,W) -> (B,C,4H,4W), not equivariant: the ramp is over the OUTPUT's rows (y) and columns (x)."""
    o = (t[:, 3] + 0.5 * t[:, 0]).repeat_interleave(4, -2).repeat_interleave(4, -1)
    y = torch.arange(o.shape[-2], dtype=torch.float32)[:, None]
    x = torch.arange(o.shape[-1], dtype=torch.float32)[None, :]
    return o * (1.0 + 0.01 * y + 0.0001 * x)


def main():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_ensemble", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    x = torch.from_numpy(np.random.RandomState(2024).rand(1, 7, 2, 6, 10).astype(np.float32))
    handed = []

    def model(t):
        handed.append(t.detach().clone())
        return standin(t)

    with torch.no_grad():
        out = ref.SpatialTemporalEnsemble(False)(x, model)
    assert len(handed) == 8 and tuple(out.shape) == (1, 2, 24, 40), (len(handed), out.shape)
    arrays = {"x": x.numpy(), "out": out.numpy().astype(np.float32)}
    arrays.update({f"in_{i}": t.numpy() for i, t in enumerate(handed)})
    np.savez_compressed(os.path.join(HERE, "ensemble_order.npz"), **arrays)
    print("ensemble_order.npz:", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
