"""On-device NIQE (harness.niqe.frame_niqe_features + the host's 36 x 36 Gaussian distance) per 720x1280 frame at N = 1 and
N = 16, HIP-event timed with the device synchronised, as a median over timed calls after warm-ups, next to the CPU contract
(harness.niqe.niqe) on the same frames.  One JSON line.

    python scripts/bench_niqe.py --params niqe_pris_params.npz [--warmup 10] [--iters 50] [--cpu-reps 2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from fcvsr_amd.harness.niqe import NiqeModel, frame_niqe_features, niqe, scores_from_features


def frames(rs, N, H, W):
    yy, xx = np.mgrid[:H, :W]
    base = 128 + 70 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    return np.clip(np.round(base[None, None] + rs.randn(N, 1, H, W) * 8), 0, 255).astype(np.uint8)


def device_ms(x, model, warmup, iters):
    """Median ms of one frame_niqe_features call on x, each call timed by its own pair of events."""
    for _ in range(warmup):
        frame_niqe_features(x, model)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = frame_niqe_features(x, model)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", required=True, help="the pristine model npz (mmedit's niqe_pris_params.npz)")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_niqe needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed calls")
    model = NiqeModel.load(args.params)
    H, W = args.height, args.width
    host = frames(np.random.RandomState(0), 16, H, W)
    res = {"frame": [H, W], "blocks": (H // 96) * (W // 96)}
    for N in (1, 16):
        ms, feats = device_ms(torch.from_numpy(host[:N]).cuda(), model, args.warmup, args.iters)
        res[f"device_ms_per_frame_n{N}"] = round(ms / N, 5)
    feats = feats.cpu().numpy()
    t0 = time.perf_counter()
    dev_scores = scores_from_features(feats, model)
    res["host_mvg_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / 16, 4)
    t0 = time.perf_counter()
    cpu_scores = [niqe(host[i, 0], model) for i in range(args.cpu_reps)]
    res["cpu_s_per_frame"] = round((time.perf_counter() - t0) / args.cpu_reps, 3)
    res["max_abs_score_diff_vs_cpu"] = float(np.abs(dev_scores[:args.cpu_reps] - np.array(cpu_scores)).max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
