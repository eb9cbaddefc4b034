"""The optimizer update of the S model (GShiftNet_S: every parameter, 243 unique tensors, 3.70 M elements; --trainable-only: the 235
of them that receive a gradient and that `TrainStep` updates, 3.56 M): torch's multi-tensor Adam, the form `TrainStep` uses by
default, against `HipAdam`, the same update in one launch over the flat buffers (csrc/optim.hip).

Both optimizers own a copy of the model's parameters and read the same gradients (views of one flat buffer, as in `TrainStep`).  They
alternate in one process: --warmup steps each, then --iters rounds of one step each, every step bracketed by device events on the
current stream (hipEventRecord before and after, elapsed time read after a synchronise).  The figure is the median step, with the
spread (p90 - p10) / median next to it.  An event pair spans the step's launches on the stream, the idle gaps between the ~10^2
launches of the multi-tensor form included: it is the time the update takes on the stream, which is what a training step pays; it
is not a kernel time from a trace.  Algorithmic bytes are 16 read + 12 written per element for either form (the multi-tensor form
moves more: every operation of its chain is a pass of its own).  One JSON line.

    python scripts/bench_adam.py [--iters 200] [--warmup 20] [--trainable-only] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(ms, nbytes):
    v = np.array(ms) * 1e3
    med = float(np.median(v))
    return {"us_median": round(med, 2), "us_min": round(float(v.min()), 2), "us_p10": round(float(np.percentile(v, 10)), 2),
            "us_p90": round(float(np.percentile(v, 90)), 2),
            "spread": round(float((np.percentile(v, 90) - np.percentile(v, 10)) / med), 4),
            "algorithmic_GBps": round(nbytes / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trainable-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 50 or args.warmup < 1:
        raise SystemExit("the protocol is warm-ups first, then the median of at least 50 iterations")
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.train import HipAdam
    from fcvsr_amd.weights import synthetic_state_dict

    model = GShiftNet_S()
    model.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    if args.trainable_only:
        from fcvsr_amd.train.step import trainable_parameters
        named = trainable_parameters(model.cuda())
    else:
        named = list(model.cuda().named_parameters())            # (named_parameters de-duplicates the aliased blocks)
    names, sizes = [n for n, _ in named], [p.numel() for _, p in named]
    numel = sum(sizes)
    g = torch.Generator(device="cuda").manual_seed(3)
    flat = torch.randn(numel, device="cuda", generator=g) * 1e-3
    kw = dict(lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-5)
    p_torch = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    for p, v in zip(p_torch, flat.split(sizes)):
        p.grad = v.view(p.shape)
    opt_torch = torch.optim.Adam(p_torch, **kw)
    p_hip = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    opt_hip = HipAdam(p_hip, names, **kw)
    steps = {"torch_multi_tensor": opt_torch.step, "hip_one_launch": lambda: opt_hip.step(flat)}

    for _ in range(args.warmup):
        for f in steps.values():
            f()
    torch.cuda.synchronize()
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(p_torch, p_hip))      # the two forms made the same updates
    events = {n: [] for n in steps}
    for _ in range(args.iters):
        for n, f in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            events[n].append((a, b))
    torch.cuda.synchronize()
    nbytes = 28 * numel
    rec = {"trainable_only": bool(args.trainable_only), "tensors": len(sizes), "elements": numel, "algorithmic_bytes": nbytes, "iters": args.iters, "warmup": args.warmup,
           "max_abs_weight_difference_after_warmup": worst}
    for n, ev in events.items():
        rec[n] = _stats([a.elapsed_time(b) for a, b in ev], nbytes)
    rec["torch_over_hip"] = round(rec["torch_multi_tensor"]["us_median"] / rec["hip_one_launch"]["us_median"], 2)
    rec["hip_no_slower_than_torch"] = rec["hip_one_launch"]["us_median"] <= rec["torch_multi_tensor"]["us_median"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not rec["hip_no_slower_than_torch"] or worst > 1e-5:
        raise SystemExit("the one-launch update is slower than the multi-tensor form, or the two made different updates")


if __name__ == "__main__":
    main()
