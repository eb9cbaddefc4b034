"""On-device PSNR + SSIM (harness.device_metrics.frame_metrics) per 720x1280 frame at batch 16, HIP-event timed, next to the CPU
functions of harness/metrics.py on the same frames.  One JSON line per case.

    python scripts/bench_metrics.py [--batch 16] [--warmup 10] [--iters 50] [--cpu-reps 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from fcvsr_amd.harness.device_metrics import frame_metrics
from fcvsr_amd.harness.metrics import psnr, ssim, to_y_channel


def frames(rs, N, C, H, W):
    yy, xx = np.mgrid[:H, :W]
    base = 128 + 70 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    hr = np.clip(base[None, None] + rs.randn(N, C, H, W) * 8, 0, 255).astype(np.uint8)
    sr = np.clip(hr.astype(np.int32) + rs.randint(-6, 7, hr.shape), 0, 255).astype(np.uint8)
    return sr, hr


def cpu_frame(sr, hr, to_y):
    """CPU psnr + ssim of one (C,H,W) frame pair, as the harness scores it."""
    if to_y:
        a, b = sr[::-1].transpose(1, 2, 0), hr[::-1].transpose(1, 2, 0)
        psnr(to_y_channel(a), to_y_channel(b), 4)
        return ssim(a, b, 4, convert_to="Y")
    psnr(sr[0], hr[0], 4)
    return ssim(sr[0], hr[0], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed calls")
    rs = np.random.RandomState(0)
    B, H, W = args.batch, args.height, args.width
    for name, C, to_y, quantise in (("C1_u8", 1, False, None), ("C1_f32_truncate", 1, False, "truncate"),
                                    ("C3_Y_u8", 3, True, None)):
        sr, hr = frames(rs, B, C, H, W)
        hr_d = torch.from_numpy(hr).cuda()
        sr_d = torch.from_numpy(sr).cuda()
        if quantise is not None:
            sr_d = (sr_d.float() + 0.25) / 255.0                  # f32 model output that truncates back to sr
        conv = "Y" if to_y else None
        run = lambda: frame_metrics(sr_d, hr_d, crop_border=4, quantise=quantise, convert_to=conv)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            out = run()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / args.iters / B
        t0 = time.perf_counter()
        ref = [cpu_frame(sr[i % B], hr[i % B], to_y) for i in range(args.cpu_reps)]
        cpu_ms = (time.perf_counter() - t0) * 1e3 / args.cpu_reps
        err = float(np.abs(out[1].cpu().numpy()[:len(ref)] - np.array(ref)).max())
        print(json.dumps({"case": name, "frame": [C, H, W], "batch": B, "device_ms_per_frame": round(dev_ms, 5),
                          "cpu_ms_per_frame": round(cpu_ms, 2), "speedup": round(cpu_ms / dev_ms, 1),
                          "max_abs_ssim_diff_vs_cpu": err}), flush=True)


if __name__ == "__main__":
    main()
