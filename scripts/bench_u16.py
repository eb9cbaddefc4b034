"""Step time of the bench shape with f32, uint8 and uint16 (10-bit) frames, and the file-to-file rate of a 10-bit sequence.

Step: 16 windows of 7 x 180 x 320 -> 16 SR frames of 720 x 1280, FCVSR-S, bf16, 2 streams, hipGraph (bench.py's flagship
configuration).  The three input types alternate in one process (--repeats rounds of --steps calls each, after a warm-up that
captures every graph) so that drift of the box hits all alike; a round's time is a host clock around --steps calls that ends in a
device synchronise.  Reports per type the step time in ms (mean, min, max over the rounds, relative spread) and the ratios to
the f32 and uint8 steps, and checks that the uint16 result equals the float path's on the same frames.

File to file: a synthetic 10-bit 320 x 180 I420 sequence of --frames frames written to a temporary directory and super-resolved
with `super_resolve_yuv420(..., bit_depth=10)` (--file-repeats timed runs after one warm-up run): frames/s including the read, the
upload, the chroma kernel, the download and the write.  One JSON line.

    python scripts/bench_u16.py [--repeats 5] [--steps 10] [--frames 60] [--out FILE.json]
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


def _stats(ms):
    v = np.array(ms)
    return {"ms_mean": round(float(v.mean()), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3),
            "spread": round(float((v.max() - v.min()) / v.mean()), 4), "ms_runs": [round(float(x), 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_u16.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict

    H, W, B = 180, 320, args.batch
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.streams, m.use_graph = "bf16", args.streams, True
    rs = np.random.RandomState(55)
    a16 = rs.randint(0, 1024, (B, 7, 1, H, W)).astype(np.uint16)
    x16 = torch.from_numpy(a16.view(np.int16)).cuda().view(torch.uint16)
    x8 = torch.from_numpy((a16 >> 2).astype(np.uint8)).cuda()
    xf = (torch.from_numpy(a16.astype(np.float32)) / 1023).cuda()
    calls = {"f32": lambda: m(xf), "u8": lambda: m.super_resolve_u8(x8), "u16": lambda: m.super_resolve_u16(x16)}
    with torch.no_grad():
        outs = {k: f() for k, f in calls.items()}            # warm-up: weights packed, hipGraphs captured
        for f in calls.values():
            f()
        torch.cuda.synchronize()
        ref = (outs["f32"].clamp(0, 1) * 1023.0).to(torch.int16)
        same = bool(torch.equal(ref, outs["u16"].view(torch.int16)))
        ms = {k: [] for k in calls}
        for _ in range(args.repeats):
            for name, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    f()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    rec = {"workload": f"{B} x 7x{H}x{W} -> {B} x {4 * H}x{4 * W}, GShiftNet_S bf16, {args.streams} streams, hipGraph",
           "repeats": args.repeats, "steps_per_repeat": args.steps, "u16_equals_float_path": same,
           "in_bytes": {"f32": xf.numel() * 4, "u8": x8.numel(), "u16": x16.numel() * 2},
           "out_bytes": {"f32": B * 16 * H * W * 4, "u8": B * 16 * H * W, "u16": B * 16 * H * W * 2}}
    for name in calls:
        rec[name] = _stats(ms[name])
    rec["u16_over_u8"] = round(rec["u16"]["ms_mean"] / rec["u8"]["ms_mean"], 4)
    rec["u16_over_f32"] = round(rec["u16"]["ms_mean"] / rec["f32"]["ms_mean"], 4)

    # file to file, 10-bit
    N = args.frames
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, f"Synth_{W}x{H}_{N}F_10bit.yuv")
        dst = os.path.join(tmp, f"Synth_{4 * W}x{4 * H}_{N}F_10bit.yuv")
        write_yuv420(src, rs.randint(0, 1024, (N, H, W)).astype(np.uint16), rs.randint(0, 1024, (N, H // 2, W // 2)).astype(np.uint16),
                     rs.randint(0, 1024, (N, H // 2, W // 2)).astype(np.uint16))
        super_resolve_yuv420(m, src, dst, W, H, batch=B, bit_depth=10)      # warm-up (the ragged last batch's graph too)
        fps = []
        for _ in range(args.file_repeats):
            torch.cuda.synchronize()
            st = super_resolve_yuv420(m, src, dst, W, H, batch=B, bit_depth=10)
            fps.append(st["fps"])
        v = np.array(fps)
        rec["file_to_file_10bit"] = {"frames": N, "fps_mean": round(float(v.mean()), 2), "fps_min": round(float(v.min()), 2),
                                     "fps_max": round(float(v.max()), 2), "spread": round(float((v.max() - v.min()) / v.mean()), 4),
                                     "bytes_read": st["bytes_read"], "bytes_written": st["bytes_written"]}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
