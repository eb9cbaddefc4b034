"""What the x8 self-ensemble costs around the model, and what the two kernels of csrc/ensemble.hip save against torch operators.

One batch of --batch (4) windows of a resident 180 x 320 one-channel f32 sequence, FCVSR-S (GShiftNet_S), bf16, hipGraph replay on
--streams (2) streams.  Three forms alternate in one process:
  (a) model:    the model alone on the 32 variant windows, already built: two calls of 4 b windows (180 x 320 and 320 x 180);
  (b) ensemble: `SelfEnsemble.sequence` end to end from the resident sequence and the index rows - the gather kernel, the same two
                model calls, the merge kernel;
  (c) torch:    the same result the reference's way with torch operators on the device, without its .cpu() round trips:
                torch.stack of the plain windows, three rounds of flip / transpose + clone, one model call per variant, the inverse
                transforms, torch.stack and mean.
--repeats rounds of --calls calls each, every round timed by a host clock that ends in a device synchronise; the figure is the
median round, with the spread (max - min) / median next to it.  These are call times, not kernel times from a trace.  (b) and (c)
are also compared: they differ by the summation order of the mean only.  One JSON line.

    python scripts/bench_ensemble.py [--repeats 7] [--calls 10] [--batch 4] [--streams 2] [--graph 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_ensemble(model, x, idx):
    """The reference's spatial_ensemble on the device: plain windows, list-doubling transforms with clones, stack + mean."""
    win = torch.stack([x[j] for j in idx], 0)
    wins = [win]
    for mode in ("vertical", "horizontal", "transpose"):
        wins += [w.flip(4).clone() if mode == "vertical" else w.flip(3).clone() if mode == "horizontal" else
                 w.permute(0, 1, 2, 4, 3).clone() for w in wins]
    outs = [model(w) for w in wins]
    for i in range(8):
        if i > 3:
            outs[i] = outs[i].permute(0, 1, 3, 2).clone()
        if i % 4 > 1:
            outs[i] = outs[i].flip(2).clone()
        if i % 2 == 1:
            outs[i] = outs[i].flip(3).clone()
    return torch.stack(outs, 0).mean(0)


def _rounds(fns, repeats, calls):
    """{name: [ms per call, one per round]}: the forms alternate within every round."""
    ms = {n: [] for n in fns}
    for _ in range(repeats):
        for n, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) * 1e3 / calls)
    return ms


def _stats(ms):
    v = np.array(ms)
    med = float(np.median(v))
    return {"ms_median": round(med, 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
            "spread": round(float((v.max() - v.min()) / med), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5 or args.calls < 5:
        raise SystemExit("the protocol is the median of at least 5 rounds of at least 5 calls")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd import hip
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    from fcvsr_amd.harness.windows import window_indices
    from fcvsr_amd.weights import synthetic_state_dict

    b, H, W, N = args.batch, args.height, args.width, 16
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.streams, m.use_graph, m.graph_cache_size = "bf16", args.streams, bool(args.graph), 8
    x = torch.from_numpy(np.random.RandomState(31).rand(N, 1, H, W).astype(np.float32)).cuda()
    idx = [window_indices(i, 7, N, "replicate") for i in range(6, 6 + b)]
    ens = SelfEnsemble(m)
    with torch.no_grad():
        va, vt = hip.ensemble_windows(x, torch.tensor(idx, dtype=torch.int32).cuda())
        va, vt = va.flatten(0, 1), vt.flatten(0, 1)
        fns = {"model": lambda: (m(va), m(vt)), "ensemble": lambda: ens.sequence(x, idx), "torch": lambda: torch_ensemble(m, x, idx)}
        for f in fns.values():                                            # warm-up: every shape captured, every kernel loaded
            for _ in range(3):
                f()
        got, ref = fns["ensemble"](), fns["torch"]()
        diff = float((got - ref).abs().max())
        ms = _rounds(fns, args.repeats, args.calls)
    rec = {"shape": [b, 7, 1, H, W], "model": "GShiftNet_S", "precision": "bf16", "streams": args.streams, "hipgraph": bool(args.graph),
           "repeats": args.repeats, "calls_per_round": args.calls, "variant_windows": 8 * b}
    rec.update({n: _stats(v) for n, v in ms.items()})
    rec["ensemble_over_model"] = round(rec["ensemble"]["ms_median"] / rec["model"]["ms_median"], 4)
    rec["torch_over_ensemble"] = round(rec["torch"]["ms_median"] / rec["ensemble"]["ms_median"], 4)
    rec["ensemble_minus_model_ms"] = round(rec["ensemble"]["ms_median"] - rec["model"]["ms_median"], 4)
    rec["torch_minus_model_ms"] = round(rec["torch"]["ms_median"] - rec["model"]["ms_median"], 4)
    rec["ensemble_vs_torch_max_abs"] = diff
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
