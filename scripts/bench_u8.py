"""Streamed REDS4-shaped sequences with f32 and with uint8 LR frames (bench.py's `stream` record, BASELINE config 5):
4 sequences x 100 frames of 180x320 in pinned host memory -> uint8 720x1280 SR frames in pinned host memory, FCVSR-S, bf16,
batch 16, 2 streams, hipGraph.  The two input types alternate in one process (--repeats runs each) so that box-to-box drift hits
both alike; reports frames/s (mean, min, max, relative spread) and the H2D / D2H bytes per frame, one JSON line, and checks that
both inputs give identical SR frames.

    python scripts/bench_u8.py [--repeats 5] [--batch 16] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_u8.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.infer import StreamedSuperResolver
    from fcvsr_amd.weights import synthetic_state_dict

    H, W, N = 180, 320, args.frames
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.streams, m.use_graph = "bf16", args.streams, True
    gs = torch.Generator().manual_seed(55)
    seq8 = [torch.randint(0, 256, (N, 1, H, W), generator=gs, dtype=torch.uint8).pin_memory() for _ in range(4)]
    seqf = [(s.float() / 255).pin_memory() for s in seq8]
    runners = {"f32": (StreamedSuperResolver(m, batch=args.batch), seqf), "u8": (StreamedSuperResolver(m, batch=args.batch), seq8)}
    outs = {}
    for name, (r, seqs) in runners.items():                 # warm-up: buffers page-locked, hipGraphs captured
        outs[name] = r.run(seqs)
    torch.cuda.synchronize()
    same = all(np.array_equal(outs["f32"][s][1], outs["u8"][s][1]) for s in outs["f32"])
    fps = {k: [] for k in runners}
    for _ in range(args.repeats):
        for name, (r, seqs) in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = r.run(seqs)
            sec = time.perf_counter() - t0
            assert sum(v[1].shape[0] for v in out.values()) == 4 * N
            fps[name].append(4 * N / sec)
    rec = {"workload": f"4 x {N} LR frames {H}x{W}, pinned host -> uint8 {4 * H}x{4 * W} pinned host, GShiftNet_S bf16, "
                       f"batch {args.batch}, {args.streams} streams, hipGraph", "repeats": args.repeats, "identical_frames": same}
    for name, (r, _) in runners.items():
        v = np.array(fps[name])
        rec[name] = {"fps_mean": round(float(v.mean()), 2), "fps_min": round(float(v.min()), 2), "fps_max": round(float(v.max()), 2),
                     "spread": round(float((v.max() - v.min()) / v.mean()), 4), "fps_runs": [round(float(x), 2) for x in v],
                     "h2d_bytes_per_frame": r.stats["h2d_bytes"] // (4 * N), "d2h_bytes_per_frame": r.stats["d2h_bytes"] // (4 * N)}
    rec["u8_over_f32"] = round(rec["u8"]["fps_mean"] / rec["f32"]["fps_mean"], 4)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
