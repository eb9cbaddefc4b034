"""What tOF costs: the Farneback flow kernels on their own, and ``tof=True`` on `harness.stream.stream_yuv420`.

(a) The kernels: `hip.farneback_flow` on P = 32 pairs of 720 x 1280 uint8 planes (views ``x[:-1]``, ``x[1:]`` of one 33-plane
    buffer) and `hip.flow_epe` on the 32 flows against 32 others, timed with device events over --calls launches after warm-up,
    median of --repeats rounds.  Next to it the algorithmic bytes of one pair (`flow_bytes`: what every stage must read and write
    once, halos and the gather's reuse not counted) and a device copy timed in the same run, from which the time a copy of the same
    bytes takes follows.  Reported only.
(b) End to end, on the protocol of scripts/bench_reference.py: a synthetic 8-bit 320 x 180 I420 file of --frames frames (at least
    256) and a 1280 x 720 ground truth through `stream_yuv420(reference=...)` (GShiftNet_S: bf16, 2 streams, hipGraph), batch 16,
    without and with ``tof=True``: one warm-up pass of each, then --runs timed runs of each, alternating, every run timed by a host
    clock that ends in a device synchronise.  Median and range of each, and whether the bytes written and the other scores are equal.
    No bar is set for either number: nothing has measured this workload before.

One process; run it under a time limit (``timeout 900 python scripts/bench_tof.py --out profiles/tof_bench.json``).
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
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def flow_bytes(h: int, w: int, elem_size: int = 1) -> dict:
    """Algorithmic bytes of one pair, per stage, summed over the pyramid levels (DESIGN.md section 9 derives the per-pixel figures):
    level images 2 e hw read (the full-size planes, at every level) + 8 n written; expansion 8 n read, 64 n written; first matrices
    64 n of R, 8 n flow and 20 n M written; three iterations 3 (20 n M read + 8 n flow written) + 2 (64 n of R + 20 n M written)."""
    from fcvsr_amd.harness.tof import level_count, level_geometry
    out = {"level_image": 0, "poly_exp": 0, "first_matrices": 0, "iterations": 0}
    for k in range(level_count(h, w)):
        hl, wl = level_geometry(h, w, k)[2]
        n = hl * wl
        out["level_image"] += 2 * elem_size * h * w + 8 * n
        out["poly_exp"] += 72 * n
        out["first_matrices"] += 92 * n
        out["iterations"] += 252 * n
    out["total"] = sum(out.values())
    return out


def kernels(calls: int, repeats: int, P: int = 32, H: int = 720, W: int = 1280):
    from fcvsr_amd import hip
    dev = torch.device("cuda:0")

    def timed(f):
        for _ in range(2):
            f()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / calls)
        return ms
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randint(0, 256, (P + 1, H // 8, W // 8), dtype=torch.uint8, device=dev, generator=g).float()
    x = torch.nn.functional.interpolate(x[None], size=(H, W), mode="bicubic", align_corners=False)[0].clamp(0, 255).to(torch.uint8)
    flows = hip.farneback_flow(x[:-1], x[1:])
    other = flows.flip(0).contiguous()
    t_flow = timed(lambda: hip.farneback_flow(x[:-1], x[1:]))
    t_epe = timed(lambda: hip.flow_epe(flows, other))
    src = torch.empty((1 << 30,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src))
    per_pair = flow_bytes(H, W)
    med = float(np.median(t_flow))
    copy_rate = 2 * src.numel() / (float(np.median(t_copy)) * 1e-3)               # bytes moved per second
    return {"P": P, "size": [W, H], "flow_ms": _summary(t_flow), "flow_ms_per_pair": round(med / P, 4),
            "epe_ms": _summary(t_epe), "bytes_per_pair": per_pair, "flow_TBps_algorithmic": round(per_pair["total"] * P / med / 1e9, 3),
            "copy_TBps_moved": round(copy_rate / 1e12, 3), "copy_ms_same_bytes_per_pair": round(per_pair["total"] / copy_rate * 1e3, 4),
            "scratch_bytes_per_pair": int(hip.lib().fcvsr_farneback_scratch_bytes(1, H, W)),
            "pairs_per_chunk": int(max(1, hip.FLOW_SCRATCH_BYTES // hip.lib().fcvsr_farneback_scratch_bytes(1, H, W)))}


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
        outs = {n: os.path.join(tmp, f"{n}_{4 * W}x{4 * H}_{frames}F.yuv") for n in ("reference", "tof")}
        write_yuv420(src, rs.randint(0, 256, (frames, H, W)).astype(np.uint8), rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8),
                     rs.randint(0, 256, (frames, H // 2, W // 2)).astype(np.uint8))
        with open(gt, "wb") as f:                                         # any bytes of the right size: the cost does not depend on them
            for _ in range(frames):
                f.write(rs.randint(0, 256, (4 * W * 4 * H * 3 // 2,), dtype=np.uint8).tobytes())
        fns = {"reference": lambda: stream_yuv420(m, src, outs["reference"], W, H, batch=batch, reference=gt),
               "tof": lambda: stream_yuv420(m, src, outs["tof"], W, H, batch=batch, reference=gt, tof=True)}
        stats = {n: f() for n, f in fns.items()}                          # warm-up: graphs, cached buffers, page cache
        with open(outs["reference"], "rb") as a, open(outs["tof"], "rb") as b:
            same = a.read() == b.read()
        same_scores = all(np.array_equal(stats["reference"][k], stats["tof"][k]) for k in ("sse", "ssim_y"))
        fps = {n: [] for n in fns}
        for _ in range(runs):
            for n, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                fps[n].append(frames / (time.perf_counter() - t0))
    rec = {"frames": frames, "batch": batch, "size": [W, H], "runs": runs, "equal_bytes": same, "equal_scores": bool(same_scores),
           "tof_mean": stats["tof"]["tof_mean"]}
    for n in fns:
        rec[n + "_fps"] = _summary(fps[n])
        rec[n + "_fps_runs"] = [round(x, 2) for x in fps[n]]
    rec["tof_median_over_reference_median"] = round(rec["tof_fps"]["median"] / rec["reference_fps"]["median"], 4)
    rec["ms_per_frame_added"] = round(1e3 / rec["tof_fps"]["median"] - 1e3 / rec["reference_fps"]["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 256 or args.runs < 5:
        raise SystemExit("the protocol is at least 256 frames and at least 5 alternating runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tof.py needs a HIP device (there is no CPU fallback)")
    rec = {}
    if not args.no_kernel:
        rec["kernels_720p"] = kernels(args.calls, args.repeats)
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
        raise SystemExit("tof=True changed the bytes written or the other scores")


if __name__ == "__main__":
    main()
