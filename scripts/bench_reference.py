"""What ``reference=`` costs (`harness.stream.stream_yuv420`), and the plane-sum kernel on its own.

(a) End to end, on the protocol of scripts/bench_stream.py: a synthetic 8-bit 320 x 180 I420 file of --frames frames (at least 256)
    and a 1280 x 720 ground truth in /dev/shm through `stream_yuv420` (file to file, GShiftNet_S: bf16, 2 streams, hipGraph),
    batch 16, in three configurations: plain, ``reference=``, and ``reference=`` with ``dst=None``.  One warm-up pass of each, then
    --runs timed runs of each, alternating, every run timed by a host clock that ends in a device synchronise.  Median and range
    of each are reported, and whether the bytes written with the keyword equal those without it.  No ratio is fixed in advance.
(b) The kernel: `hip.plane_sse` on 64 pairs of 2160 x 3840 planes, uint8 and uint16 (1.06 / 2.12 GB read, beyond the 256 MiB
    Infinity Cache), timed with device events over --calls launches after warm-up, median of --repeats rounds; next to it a
    device copy of the same bytes (both operands, read and written) timed in the same run.  TB/s over the bytes read.  Reported only.

    python scripts/bench_reference.py [--frames 256] [--runs 5] [--calls 10] [--repeats 5] [--out FILE.json]
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


def _summary(v):
    v = np.array(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2)}


def end_to_end(frames: int, runs: int, batch: int = 16):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import write_yuv420
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
        gt = os.path.join(tmp, f"GT_{4 * W}x{4 * H}_{frames}F.yuv")
        outs = {n: os.path.join(tmp, f"{n}_{4 * W}x{4 * H}_{frames}F.yuv") for n in ("plain", "reference")}
        write_yuv420(src, rs.randint(0, 256, (frames, H, W)).astype(np.uint8), rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8),
                     rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8))
        with open(gt, "wb") as f:                                         # any bytes of the right size: the cost does not depend on them
            for _ in range(frames):
                f.write(rs.randint(0, 256, (4 * W * 4 * H * 3 // 2,), dtype=np.uint8).tobytes())
        fns = {"plain": lambda: stream_yuv420(m, src, outs["plain"], W, H, batch=batch),
               "reference": lambda: stream_yuv420(m, src, outs["reference"], W, H, batch=batch, reference=gt),
               "reference_scores_only": lambda: stream_yuv420(m, src, None, W, H, batch=batch, reference=gt)}
        stats = {n: f() for n, f in fns.items()}                          # warm-up: graphs, cached buffers, page cache
        with open(outs["plain"], "rb") as a, open(outs["reference"], "rb") as b:
            same = a.read() == b.read()
        same_scores = all(np.array_equal(stats["reference"][k], stats["reference_scores_only"][k]) for k in ("sse", "ssim_y"))
        fps = {n: [] for n in fns}
        for _ in range(runs):
            for n, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                fps[n].append(frames / (time.perf_counter() - t0))
    rec = {"frames": frames, "batch": batch, "size": [W, H], "runs": runs, "equal_bytes": same, "equal_scores": bool(same_scores),
           "psnr_yuv_global": stats["reference"]["psnr_yuv_global"]}
    for n in fns:
        rec[n + "_fps"] = _summary(fps[n])
        rec[n + "_fps_runs"] = [round(x, 2) for x in fps[n]]
    for n in ("reference", "reference_scores_only"):
        rec[n + "_median_over_plain_median"] = round(rec[n + "_fps"]["median"] / rec["plain_fps"]["median"], 4)
    return rec


def kernel(calls: int, repeats: int, P: int = 64, H: int = 2160, W: int = 3840):
    from fcvsr_amd import hip
    dev = torch.device("cuda:0")
    rec = {}

    def timed(f):
        for _ in range(3):
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
        return us
    for name, dt, top in (("uint8", torch.uint8, 256), ("uint16", torch.int16, 1024)):
        x = torch.randint(0, top, (P, H, W), dtype=dt, device=dev)
        y = torch.randint(0, top, (P, H, W), dtype=dt, device=dev)
        cx, cy = torch.empty_like(x), torch.empty_like(y)
        nbytes = 2 * x.numel() * x.element_size()

        def copy():
            cx.copy_(x)
            cy.copy_(y)
        for tag, f, moved in (("plane_sse", lambda: hip.plane_sse(x, y, 4), nbytes), ("copy", copy, 2 * nbytes)):
            us = timed(f)
            med = float(np.median(us))
            rec[f"{tag}_{name}"] = {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                                    "bytes_read": nbytes, "TBps_read": round(nbytes / med / 1e6, 3),
                                    "TBps_moved": round(moved / med / 1e6, 3)}
        del x, y, cx, cy
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 256 or args.runs < 5:
        raise SystemExit("the protocol is at least 256 frames and at least 5 alternating runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_reference.py needs a HIP device (there is no CPU fallback)")
    rec = {}
    if not args.no_kernel:
        rec["kernel_2160p"] = kernel(args.calls, args.repeats)
    if not args.no_file:
        with torch.no_grad():
            rec["end_to_end"] = end_to_end(args.frames, args.runs)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not args.no_file and not (rec["end_to_end"]["equal_bytes"] and rec["end_to_end"]["equal_scores"]):
        raise SystemExit("reference= changed the bytes written, or dst=None the scores")


if __name__ == "__main__":
    main()
