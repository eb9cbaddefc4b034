"""The streamed YUV path (`harness.stream.stream_yuv420`) against the whole-file one, and the two surface kernels on their own.

(a) End to end: a synthetic 8-bit 320 x 180 I420 file of --frames frames (at least 256) in /dev/shm through `super_resolve_yuv420`
    and through `stream_yuv420` (file to file, the same GShiftNet_S: bf16, 2 streams, hipGraph), batch 16.  One warm-up pass of
    each, then --runs timed runs of each, alternating, every run timed by a host clock that ends in a device synchronise.  The
    streamed path does the same model work and overlaps reading, upload and writing with it, so it is expected to be no slower.
    The bar: its median fps must not lie below the slowest whole-file run - the margin is the spread those runs show themselves.
    The two outputs are compared byte for byte.
(b) Kernels: `hip.surface_unpack` into a ring and `hip.surface_pack` out of planes at 1920 x 1080, 64 frames (source plus
    destination exceed the 256 MiB Infinity Cache), all four formats, timed with device events over --calls launches, median of
    --repeats rounds.  Bytes read + written per second, next to the 6.3 TB/s a plain device copy reaches on this part.  Reported
    only.

    python scripts/bench_stream.py [--frames 256] [--runs 5] [--calls 50] [--repeats 5] [--out FILE.json]
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

COPY_TBPS = 6.3


def _summary(v):
    v = np.array(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}


def end_to_end(frames: int, runs: int, batch: int = 16):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    H, W = 180, 320
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.streams, m.use_graph = "bf16", 2, True
    rs = np.random.RandomState(5)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=shm) as tmp:
        src = os.path.join(tmp, f"Synth_{W}x{H}_{frames}F.yuv")
        outs = {n: os.path.join(tmp, f"{n}_{4 * W}x{4 * H}_{frames}F.yuv") for n in ("whole", "stream")}
        write_yuv420(src, rs.randint(0, 256, (frames, H, W)).astype(np.uint8), rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8),
                     rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8))
        fns = {"whole": lambda: super_resolve_yuv420(m, src, outs["whole"], W, H, batch=batch),
               "stream": lambda: stream_yuv420(m, src, outs["stream"], W, H, batch=batch)}
        for f in fns.values():                                            # warm-up: graphs, cached buffers, page cache
            f()
        with open(outs["whole"], "rb") as a, open(outs["stream"], "rb") as b:
            same = a.read() == b.read()
        fps = {n: [] for n in fns}
        for _ in range(runs):
            for n, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = f()
                torch.cuda.synchronize()
                fps[n].append(frames / (time.perf_counter() - t0))
    rec = {"frames": frames, "batch": batch, "size": [W, H], "runs": runs, "equal_bytes": same,
           "whole_file_fps": _summary(fps["whole"]), "streamed_fps": _summary(fps["stream"]),
           "whole_file_fps_runs": [round(x, 2) for x in fps["whole"]], "streamed_fps_runs": [round(x, 2) for x in fps["stream"]],
           "ring_frames": st["ring_frames"]}
    rec["streamed_median_not_below_slowest_whole_file_run"] = bool(rec["streamed_fps"]["median"] >= rec["whole_file_fps"]["min"])
    return rec


def kernels(calls: int, repeats: int, n: int = 64, H: int = 1080, W: int = 1920):
    from fcvsr_amd import hip
    from fcvsr_amd.harness import surfaces as sf
    dev = torch.device("cuda:0")
    rec = {}
    for fmt in sf.PIX_FMTS:
        fb = sf.frame_bytes(fmt, W, H)
        bdt = torch.uint8 if sf.bit_depth(fmt) == 8 else torch.int16
        sdt = torch.uint8 if sf.bit_depth(fmt) == 8 else torch.uint16
        raw = torch.randint(0, 256, (n * fb,), dtype=torch.uint8, device=dev)
        slots = torch.arange(n, dtype=torch.int32, device=dev).flip(0).contiguous()
        ry = torch.zeros((n, 1, H, W), dtype=bdt, device=dev).view(sdt)
        ru, rv = (torch.zeros((n, H // 2, W // 2), dtype=bdt, device=dev).view(sdt) for _ in range(2))
        fns = {"unpack": lambda: hip.surface_unpack(raw, fmt, W, H, slots, ry, ru, rv),
               "pack": lambda: hip.surface_pack(ry[:, 0], ru, rv, fmt)}
        for name, f in fns.items():
            for _ in range(5):
                f()
            us = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    f()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / calls)
            med = float(np.median(us))
            tbps = 2 * n * fb / med / 1e6
            rec[f"{name}_{fmt}"] = {"us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                                    "bytes_read_plus_written": 2 * n * fb, "TBps": round(tbps, 3),
                                    "share_of_copy_rate": round(tbps / COPY_TBPS, 3)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 256 or args.runs < 5:
        raise SystemExit("the protocol is at least 256 frames and at least 5 alternating runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream.py needs a HIP device (there is no CPU fallback)")
    rec = {"kernels_1080p": kernels(args.calls, args.repeats), "copy_TBps": COPY_TBPS}
    if not args.no_file:
        with torch.no_grad():
            rec["end_to_end"] = end_to_end(args.frames, args.runs)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not args.no_file and not (rec["end_to_end"]["equal_bytes"] and rec["end_to_end"]["streamed_median_not_below_slowest_whole_file_run"]):
        raise SystemExit("the streamed path differs from the whole-file path or is slower than its slowest run")


if __name__ == "__main__":
    main()
