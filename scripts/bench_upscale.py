"""The MATLAB-style bicubic up-scale (fcvsr_bicubic_upscale) on a batch of 16 frames 180x320 -> 720x1280, for uint8 -> uint8,
uint8 -> f32 and uint16 -> uint16, next to fcvsr_chroma_up4 (torch's bicubic, uint8 -> uint8 and uint16 -> uint16) on the same planes in
the same run, and the numpy contract (harness.niqe.bicubic_upscale) on one frame.  One JSON line.

A call is some microseconds, less than the Python wrapper takes to allocate its result, so the entry points are called directly on
preallocated outputs, `--calls` back to back between one pair of HIP events, with the device synchronised before and after; the
figure of a form is the median over `--iters` such groups of the time per call, and `spread` is the (min, max) over the groups.  The
forms are timed alternately, group by group, so that a drift of the machine hits all of them.  GB/s is (bytes read + bytes written)
over that time.

    python scripts/bench_upscale.py [--warmup 10] [--iters 50] [--calls 20] [--cpu-reps 2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from fcvsr_amd import hip
from fcvsr_amd.harness.niqe import bicubic_upscale as contract


def frames(rs, N, H, W, peak):
    yy, xx = np.mgrid[:H, :W]
    base = peak * (0.5 + 0.27 * np.sin(xx / 9.0) * np.cos(yy / 13.0))
    return np.clip(np.round(base[None] + rs.randn(N, H, W) * peak / 32), 0, peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=180)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_upscale needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed groups")
    N, H, W = args.frames, args.height, args.width
    rs = np.random.RandomState(0)
    host8, host16 = frames(rs, N, H, W, 255).astype(np.uint8), frames(rs, N, H, W, 1023).astype(np.int16)
    x8, x16 = torch.from_numpy(host8).cuda(), torch.from_numpy(host16).cuda()            # uint16 samples as int16 bits
    out = {k: torch.empty((N, 4 * H, 4 * W), dtype=dt, device="cuda")
           for k, dt in (("u8", torch.uint8), ("f32", torch.float32), ("u16", torch.int16))}
    L, st = hip.lib(), hip.stream_ptr()
    t8, t16 = hip.u8_table("cuda"), hip.u16_table("cuda")
    px = N * H * W
    forms = {                                                # name -> (call, bytes written); all read 1 or 2 bytes per LR sample
        "upscale_u8_u8": (lambda: L.fcvsr_bicubic_upscale(x8.data_ptr(), hip.U8, N, H, W, 4, out["u8"].data_ptr(), hip.U8, st), 16 * px),
        "upscale_u8_f32": (lambda: L.fcvsr_bicubic_upscale(x8.data_ptr(), hip.U8, N, H, W, 4, out["f32"].data_ptr(), hip.F32, st), 64 * px),
        "upscale_u16_u16": (lambda: L.fcvsr_bicubic_upscale(x16.data_ptr(), hip.U16, N, H, W, 4, out["u16"].data_ptr(), hip.U16, st),
                            32 * px),
        "chroma_up4_u8": (lambda: L.fcvsr_chroma_up4(x8.data_ptr(), t8.data_ptr(), N, H, W, out["u8"].data_ptr(), st), 16 * px),
        "chroma_up4_u16": (lambda: L.fcvsr_chroma_up4_u16(x16.data_ptr(), t16.data_ptr(), N, H, W, out["u16"].data_ptr(), st), 32 * px),
    }
    for call, _ in forms.values():
        for _ in range(args.warmup):
            hip.check(call(), "warm-up")
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.iters):
        for name, (call, _) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)                    # us per call
    res = {"frames": N, "lr": [H, W], "sr": [4 * H, 4 * W], "calls_per_group": args.calls, "groups": args.iters}
    for name, (_, written) in forms.items():
        t = np.array(times[name])
        med, read = float(np.median(t)), px * (2 if "u16" in name else 1)
        res[name] = {"us_per_batch": round(med, 2), "spread_us": [round(float(t.min()), 2), round(float(t.max()), 2)],
                     "GBps": round((read + written) / med / 1e3, 1), "ps_per_output_byte": round(med * 1e6 / written, 3)}
    # the results of the timed calls are the contract's
    hip.check(forms["upscale_u8_u8"][0](), "fcvsr_bicubic_upscale")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.cpu_reps):
        ref = contract(host8[i], 4, out="int")
    res["numpy_contract_s_per_frame"] = round((time.perf_counter() - t0) / args.cpu_reps, 4)
    res["u8_equals_contract"] = bool(np.array_equal(out["u8"][args.cpu_reps - 1].cpu().numpy(), ref))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
