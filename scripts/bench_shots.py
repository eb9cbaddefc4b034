"""The pair-SAD kernel of scene-cut detection (hip.frame_pair_sad) on 100 frames of 180x320 and of 1080x1920, uint8 and uint16:
the whole call (scratch allocation and both launches), HIP-event timed with the device synchronised, as a median over timed calls
after warm-ups with the 10th / 90th percentile next to it; the same calls split by kernel (torch.profiler's device activity, summed
per kernel name over the timed calls) and the GB/s of the N*C*H*W*elem bytes of the sequence over the kernels' time; and the same
sums by the torch expression (a[1:].int() - a[:-1].int()).abs().sum((1, 2, 3)), timed the same way in the same process, the two
alternating.  The results of the two are compared exactly.  One JSON line.

    python scripts/bench_shots.py [--frames 100] [--channels 1] [--warmup 10] [--iters 50]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from fcvsr_amd import hip


def frames(rs, N, C, H, W, peak):
    """A panned pattern under noise, values in [0, peak]: uint8 for peak 255, else 10-bit samples as int16 bits."""
    yy, xx = np.mgrid[:H, :W]
    out = np.empty((N, C, H, W), np.uint8 if peak == 255 else np.int16)
    for i in range(N):
        base = 0.5 + 0.4 * np.sin((xx + i) / 9.0) * np.cos(yy / 13.0)
        out[i] = np.clip(np.round((base[None] + rs.randn(C, H, W) * 0.02) * peak), 0, peak)
    return out


def torch_sad(a):
    return (a[1:].int() - a[:-1].int()).abs().sum((1, 2, 3))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def event_ms(fns, warmup, iters):
    """Per function: (median, p10, p90) ms of one call, each call timed by its own pair of events, the functions alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(iters):
        for k, fn in enumerate(fns):
            t, outs[k] = timed(fn)
            times[k].append(t)
    return [tuple(float(np.percentile(t, q)) for q in (50, 10, 90)) for t in times], outs


def kernel_ms(fn, iters):
    """ms per call by kernel name (device time summed over `iters` calls, divided by iters)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        total_us = getattr(ev, "device_time_total", None)
        if total_us is None:
            total_us = getattr(ev, "cuda_time_total", 0.0)
        if total_us:
            name = ev.key.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            out[name] = out.get(name, 0.0) + total_us / 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shots needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed calls")
    N, C = args.frames, args.channels
    res = {"frames": N, "channels": C, "cases": []}
    for H, W in ((180, 320), (1080, 1920)):
        for peak in (255, 1023):
            x = torch.from_numpy(frames(np.random.RandomState(0), N, C, H, W, peak)).cuda()
            nbytes = x.numel() * x.element_size()
            (k_ms, t_ms), (got, ref) = event_ms([lambda: hip.frame_pair_sad(x), lambda: torch_sad(x)], args.warmup, args.iters)
            case = {"frame": [H, W], "dtype": "uint8" if peak == 255 else "uint16", "bytes": nbytes,
                    "equal_to_torch": bool(torch.equal(got, ref)),
                    "call_ms": [round(v, 4) for v in k_ms], "torch_ms": [round(v, 4) for v in t_ms],
                    "call_gbps": round(nbytes / k_ms[0] / 1e6, 1), "torch_gbps": round(nbytes / t_ms[0] / 1e6, 1)}
            try:
                by_kernel = kernel_ms(lambda: hip.frame_pair_sad(x), args.iters)
                mine = {k: v for k, v in by_kernel.items() if "pair_sad" in k or "partial_sum_kernel" in k}      # both launches
                case["kernel_ms"] = {k: round(v, 5) for k, v in sorted(mine.items())}
                case["kernels_gbps"] = round(nbytes / sum(mine.values()) / 1e6, 1) if mine else None
                case["torch_kernels_ms"] = round(sum(kernel_ms(lambda: torch_sad(x), args.iters).values()), 5)
            except Exception as exc:                           # a torch build without device tracing: the call times stand alone
                case["kernel_ms"] = f"unavailable: {type(exc).__name__}: {exc}"
            res["cases"].append(case)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
