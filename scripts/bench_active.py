"""Letterbox-aware SR (`active=`, `harness.active`): the two kernels on their own, and what the keyword buys end to end.

(a) Kernels at 1920 x 1080, 64 frames, uint8 and uint16, timed with device events after warm-up, median of --repeats rounds of
    --calls launches.  `hip.frame_line_sums`: bytes read (the frames) + written (the sums) per second, next to the rate of a plain
    device copy of the same frames (timed here the same way) and next to the torch pair ``x.sum(-1)`` / ``x.sum(-2)`` that gives
    the same numbers.  `hip.active_compose` for the 2.39:1 box of a 16:9 frame (rows 140 .. 940): bytes read (the resolver's frames
    and the LR samples outside the box) + written (the 4x frames) per second, next to a plain copy of the 4x frames.  Reported only.
(b) End to end: `stream_yuv420` on 256 frames of 320 x 180 with planted bars around a 320 x 136 picture, batch 16, FCVSR-S
    (GShiftNet_S) bf16, ``active=None`` against ``active="auto"``, alternating, --runs timed runs of each after one warm-up of each,
    every run timed by a host clock that ends in a device synchronise.  The convolution work is linear in pixels, so the expectation
    is a gain near the area ratio 180 / 136 = 1.32.  The bar: the "auto" median fps lies above the fastest ``None`` run.

    python scripts/bench_active.py [--frames 256] [--runs 5] [--calls 20] [--repeats 5] [--out FILE.json]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_us(fn, calls: int, repeats: int, warmup: int = 3):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(us)), float(min(us)), float(max(us))


def _rate(nbytes: int, us) -> dict:
    return {"us_median": round(us[0], 2), "us_min": round(us[1], 2), "us_max": round(us[2], 2), "bytes": int(nbytes),
            "TBps": round(nbytes / us[0] / 1e6, 3)}


def kernels(calls: int, repeats: int, n: int = 64, H: int = 1080, W: int = 1920, box=(140, 940, 0, 1920)):
    from fcvsr_amd import hip
    dev = torch.device("cuda:0")
    rec = {}
    t, b, l, r = box
    for name, sdt, bdt, peak in (("uint8", torch.uint8, torch.uint8, 256), ("uint16", torch.uint16, torch.int16, 1024)):
        x = torch.randint(0, peak, (n, 1, H, W), dtype=bdt, device=dev)
        e = x.element_size()
        other = torch.empty_like(x)
        rows, cols = hip.frame_line_sums(x.view(sdt))
        same = bool(torch.equal(rows, x.sum(-1, dtype=torch.int64).sum(1)) and torch.equal(cols, x.sum(-2, dtype=torch.int64).sum(1)))
        sums = _rate(x.numel() * e + n * (H + W) * 8, _event_us(lambda: hip.frame_line_sums(x.view(sdt)), calls, repeats))
        sums["equal_to_torch"] = same
        sums["copy_TBps"] = _rate(2 * x.numel() * e, _event_us(lambda: other.copy_(x), calls, repeats))["TBps"]
        sums["torch_pair"] = _rate(x.numel() * e + n * (H + W) * 8, _event_us(
            lambda: (x.sum(-1, dtype=torch.int64), x.sum(-2, dtype=torch.int64)), calls, repeats))
        rec[f"line_sums_{name}"] = sums
        del other
        sr = torch.randint(0, peak, (n, 1, 4 * (b - t), 4 * (r - l)), dtype=bdt, device=dev).view(sdt)
        centres = torch.arange(n, dtype=torch.int32, device=dev)
        out_bytes = n * 16 * H * W * e
        outside = n * (H * W - (b - t) * (r - l)) * e
        comp = _rate(sr.numel() * e + outside + out_bytes,
                     _event_us(lambda: hip.active_compose(sr, x.view(sdt), centres, box, H, W), max(calls // 4, 2), repeats))
        big, big2 = (torch.empty((out_bytes,), dtype=torch.uint8, device=dev) for _ in range(2))
        comp["copy_TBps"] = _rate(2 * out_bytes, _event_us(lambda: big2.copy_(big), max(calls // 4, 2), repeats))["TBps"]
        rec[f"compose_{name}"] = comp
        del sr, big, big2, x
    return rec


def _summary(v):
    v = np.array(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}


def end_to_end(frames: int, runs: int, batch: int = 16, H: int = 180, W: int = 320, picture: int = 136):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.streams, m.use_graph = "bf16", 2, True
    rs = np.random.RandomState(5)
    top = (H - picture) // 2
    y = rs.randint(0, 6, (frames, H, W))                                  # bars: noise below the limit
    y[:, top:top + picture] = rs.randint(40, 236, (frames, picture, W))
    c = rs.randint(100, 156, (frames, 2 * (H // 2) * (W // 2)))
    data = np.concatenate([y.reshape(frames, -1), c], 1).astype(np.uint8).tobytes()
    outs, stats = {}, {}

    def run(active):
        out = io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = stream_yuv420(m, io.BytesIO(data), out, W, H, batch=batch, active=active)
        torch.cuda.synchronize()
        return frames / (time.perf_counter() - t0), out.getvalue(), st
    modes = {"none": None, "auto": "auto"}
    for name, a in modes.items():                                         # warm-up: graphs and cached buffers of both frame sizes
        _, outs[name], stats[name] = run(a)
    fps = {name: [] for name in modes}
    for _ in range(runs):
        for name, a in modes.items():
            fps[name].append(run(a)[0])
    rec = {"frames": frames, "batch": batch, "size": [W, H], "picture": [W, picture], "runs": runs,
           "boxes": stats["auto"]["active"], "area_ratio": round(H / picture, 3),
           "none_fps": _summary(fps["none"]), "auto_fps": _summary(fps["auto"]),
           "none_fps_runs": [round(v, 2) for v in fps["none"]], "auto_fps_runs": [round(v, 2) for v in fps["auto"]],
           "same_size_output": len(outs["none"]) == len(outs["auto"])}
    rec["gain"] = round(rec["auto_fps"]["median"] / rec["none_fps"]["median"], 3)
    rec["auto_median_above_fastest_none_run"] = bool(rec["auto_fps"]["median"] > rec["none_fps"]["max"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 256 or args.runs < 5:
        raise SystemExit("the protocol is at least 256 frames and at least 5 alternating runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_active.py needs a HIP device (there is no CPU fallback)")
    rec = {"kernels_1080p": kernels(args.calls, args.repeats)}
    if not args.no_stream:
        with torch.no_grad():
            rec["end_to_end"] = end_to_end(args.frames, args.runs)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not args.no_stream and not rec["end_to_end"]["auto_median_above_fastest_none_run"]:
        raise SystemExit('the active="auto" median fps does not lie above the fastest active=None run')


if __name__ == "__main__":
    main()
