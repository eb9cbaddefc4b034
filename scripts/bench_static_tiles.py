"""Static-tile reuse (`static_tiles=`, `harness.tiles`): what the keyword buys on static content, what it costs on content where
nothing can be reused, and the compare kernel on its own.

(a) End to end: `stream_yuv420` from and to files in /dev/shm, 256 frames of 320 x 180, FCVSR-S (GShiftNet_S) bf16, batch 16,
    tile 128, overlap 16 (2 x 3 tiles a frame), ``static_tiles=False`` against ``True``, alternating, --runs timed runs of each after
    one warm-up of each, every run timed by a host clock that ends in a device synchronise.
    Content A: one fixed noise background and a 48 x 48 noise patch that moves every frame.  The bar: the ``True`` median fps lies
    above the fastest ``False`` run.  Reported: both, tiles_run / tiles_total, and how far the gain falls short of total / run.
    Content B: every frame fresh noise; nothing is reusable.  No bar: the ratio True / False is the price of the comparison and
    of its one host synchronisation per group.
(b) `hip.tile_pairs_equal` at 1920 x 1080: the 63 consecutive pairs of 64 uint8 frames (identical frames: no pair differs, every
    byte of both frames of every pair is read), tile 128, overlap 16, device events after warm-up, median of --repeats rounds of
    --calls launches; bytes read (2 frames a pair, the overlaps counted once) per second, next to a plain device copy of the
    same number of bytes timed the same way.  Reported only.

    python scripts/bench_static_tiles.py [--frames 256] [--runs 5] [--calls 10] [--repeats 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = dict(tile=128, tile_overlap=16)


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


def compare_kernel(calls: int, repeats: int, n: int = 64, H: int = 1080, W: int = 1920):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    dev = torch.device("cuda:0")
    plan = tile_plan(H, W, TILE["tile"], TILE["tile_overlap"])
    x = torch.randint(0, 256, (1, 1, H, W), dtype=torch.uint8, device=dev).repeat(n, 1, 1, 1).contiguous()
    pairs = torch.tensor([[i, i + 1] for i in range(n - 1)], dtype=torch.int32, device=dev)
    E = hip.tile_pairs_equal(x, pairs, plan)
    nbytes = 2 * (n - 1) * H * W
    rec = _rate(nbytes, _event_us(lambda: hip.tile_pairs_equal(x, pairs, plan), calls, repeats))
    rec.update(pairs=n - 1, tiles=[plan.ny, plan.nx], all_equal=bool(E.all()),
               bytes_loaded=int(2 * (n - 1) * sum(min(plan.th, H - ay) * min(plan.tw, W - ax) for ay in plan.ys for ax in plan.xs)))
    a, b = (torch.empty((nbytes // 2,), dtype=torch.uint8, device=dev) for _ in range(2))
    rec["copy_TBps"] = _rate(nbytes, _event_us(lambda: b.copy_(a), calls, repeats))["TBps"]     # reads and writes nbytes / 2 each
    return rec


def _summary(v):
    v = np.array(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}


def _content(kind: str, frames: int, H: int, W: int, patch: int = 48) -> bytes:
    rs = np.random.RandomState(5)
    if kind == "static":
        y = np.repeat(rs.randint(0, 256, (1, H, W)), frames, 0)
        for i in range(frames):                                          # the patch walks along a Lissajous figure
            t, l = int((H - patch) * (0.5 + 0.5 * np.sin(0.11 * i))), int((W - patch) * (0.5 + 0.5 * np.cos(0.07 * i)))
            y[i, t:t + patch, l:l + patch] = rs.randint(0, 256, (patch, patch))
    else:
        y = rs.randint(0, 256, (frames, H, W))
    c = np.repeat(rs.randint(100, 156, (1, 2 * (H // 2) * (W // 2))), frames, 0)
    return np.concatenate([y.reshape(frames, -1), c], 1).astype(np.uint8).tobytes()


def end_to_end(m, kind: str, frames: int, runs: int, batch: int = 16, H: int = 180, W: int = 320):
    from fcvsr_amd.harness.stream import stream_yuv420
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        src, dst = os.path.join(tmp, f"in_{W}x{H}.yuv"), os.path.join(tmp, "out.yuv")
        with open(src, "wb") as fh:
            fh.write(_content(kind, frames, H, W))
        outs, stats = {}, {}

        def run(flag):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = stream_yuv420(m, src, dst, W, H, batch=batch, static_tiles=flag, **TILE)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            with open(dst, "rb") as fh:
                return frames / dt, fh.read(), st
        for flag in (False, True):                                       # warm-up: graphs of every pass size, cached buffers
            _, outs[flag], stats[flag] = run(flag)
        fps = {False: [], True: []}
        for _ in range(runs):
            for flag in (False, True):
                fps[flag].append(run(flag)[0])
    total, ran = stats[True]["tiles_total"], stats[True]["tiles_run"]
    rec = {"content": kind, "frames": frames, "batch": batch, "size": [W, H], "runs": runs, "tiles_total": total, "tiles_run": ran,
           "work_ratio": round(total / ran, 3), "false_fps": _summary(fps[False]), "true_fps": _summary(fps[True]),
           "false_fps_runs": [round(v, 2) for v in fps[False]], "true_fps_runs": [round(v, 2) for v in fps[True]],
           "same_bytes": outs[False] == outs[True]}
    rec["gain"] = round(rec["true_fps"]["median"] / rec["false_fps"]["median"], 3)
    rec["gain_over_work_ratio"] = round(rec["gain"] / rec["work_ratio"], 3)
    rec["true_median_above_fastest_false_run"] = bool(rec["true_fps"]["median"] > rec["false_fps"]["max"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 256 or args.runs < 5:
        raise SystemExit("the protocol is at least 256 frames and at least 5 alternating runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_static_tiles.py needs a HIP device (there is no CPU fallback)")
    rec = {"pairs_equal_1080p": compare_kernel(args.calls, args.repeats)}
    if not args.no_stream:
        from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
        from fcvsr_amd.arch.schema import state_dict_shapes
        from fcvsr_amd.weights import synthetic_state_dict
        m = GShiftNet_S()
        m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
        m = m.cuda()
        m.precision, m.streams, m.use_graph = "bf16", 2, True
        with torch.no_grad():
            rec["static_background"] = end_to_end(m, "static", args.frames, args.runs)
            rec["all_dirty"] = end_to_end(m, "noise", args.frames, args.runs)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not args.no_stream:
        if not (rec["static_background"]["same_bytes"] and rec["all_dirty"]["same_bytes"]):
            raise SystemExit("static_tiles=True wrote other bytes than static_tiles=False")
        if not rec["static_background"]["true_median_above_fastest_false_run"]:
            raise SystemExit("static background: the static_tiles=True median fps does not lie above the fastest False run")


if __name__ == "__main__":
    main()
