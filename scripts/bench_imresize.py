"""The any-size MATLAB `imresize` (fcvsr_imresize) on 16 uint8 planes at three delivery sizes: 720x1280 -> 540x960 (0.75x),
720x1280 -> 1080x1920 (1.5x) and 1440x2560 -> 1080x1920 (0.75x), uint8 -> uint8 (the form the harness delivers frames with), next to
`F.interpolate(x.float(), size, mode="bicubic", antialias=True)` on the same device in the same run - a different operator (A = -0.75,
other border, f32 in and out), there as a yardstick for the time only.  Then the device-to-host bytes per frame of
`super_resolve_yuv420` at 180x320 with and without output_shape=(540, 960).  One JSON line.

A call is tens of microseconds, so the entry point is called directly on a preallocated output with its cached tables, `--calls` back to
back between one pair of HIP events, with the device synchronised before and after; the figure of a form is the median over `--iters`
such groups of the time per call, and `spread` is the (min, max) over the groups.  The two forms of a size are timed alternately, group
by group, so that a drift of the machine hits both.  `hbm_share` is (bytes read + bytes written) / time over the 6.3 TB/s a copy
reaches on this device.

    python scripts/bench_imresize.py [--warmup 10] [--iters 50] [--calls 20]
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch
import torch.nn.functional as F

from fcvsr_amd import hip
from fcvsr_amd.harness.resize import imresize, imresize_host, resize_geometry

SIZES = (((720, 1280), (540, 960)), ((720, 1280), (1080, 1920)), ((1440, 2560), (1080, 1920)))
HBM_COPY_TBPS = 6.3


def frames(rs, N, H, W, peak=255):
    yy, xx = np.mgrid[:H, :W]
    base = peak * (0.5 + 0.27 * np.sin(xx / 9.0) * np.cos(yy / 13.0))
    return np.clip(np.round(base[None] + rs.randn(N, H, W) * peak / 32), 0, peak).astype(np.uint8)


def timed(forms, warmup, iters, calls):
    for call in forms.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(iters):
        for name, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / calls)                        # us per call
    return {k: np.array(v) for k, v in times.items()}


def d2h_per_frame():
    """Bytes that cross to the host per frame of super_resolve_yuv420 (every byte it downloads is a byte it writes)."""
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    N, H, W = 4, 180, 320
    rs = np.random.RandomState(1)
    y, u, v = frames(rs, N, H, W), frames(rs, N, H // 2, W // 2), frames(rs, N, H // 2, W // 2)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, f"Seq_{W}x{H}_{N}F.yuv")
        write_yuv420(src, y, u, v)
        full = super_resolve_yuv420(m, src, os.path.join(d, "x4.yuv"), W, H, batch=2)
        x3 = super_resolve_yuv420(m, src, os.path.join(d, "x3.yuv"), W, H, batch=2, output_shape=(540, 960))
    a, b = full["bytes_written"] // N, x3["bytes_written"] // N
    return {"lr": [H, W], "x4": {"out_size": list(full["out_size"]), "d2h_bytes_per_frame": a},
            "output_shape_540x960": {"out_size": list(x3["out_size"]), "d2h_bytes_per_frame": b}, "ratio": round(b / a, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imresize needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed groups")
    N = args.planes
    L, st = hip.lib(), hip.stream_ptr()
    rs = np.random.RandomState(0)
    res = {"planes": N, "calls_per_group": args.calls, "groups": args.iters, "hbm_copy_TBps": HBM_COPY_TBPS, "sizes": []}
    for (H, W), (Ho, Wo) in SIZES:
        host = frames(rs, N, H, W)
        x = torch.from_numpy(host).cuda()
        xf = x.float()[:, None]                                  # the yardstick's input, converted outside the timed window
        out = torch.empty((N, Ho, Wo), dtype=torch.uint8, device="cuda")
        _, (sy, sx), rows_first = resize_geometry(H, W, output_shape=(Ho, Wo))
        (wy, fy, Py), (wx, fx, Px) = hip.resize_device_tables(H, Ho, sy, "cuda"), hip.resize_device_tables(W, Wo, sx, "cuda")

        def call():
            hip.check(L.fcvsr_imresize(x.data_ptr(), hip.U8, N, H, W, Ho, Wo, wy.data_ptr(), fy.data_ptr(), Py, wx.data_ptr(),
                                       fx.data_ptr(), Px, int(rows_first), out.data_ptr(), hip.U8, st), "fcvsr_imresize")
        t = timed({"imresize_u8_u8": call,
                   "torch_interpolate_f32": lambda: F.interpolate(xf, size=(Ho, Wo), mode="bicubic", antialias=True)},
                  args.warmup, args.iters, args.calls)
        moved = N * (H * W + Ho * Wo)                            # uint8 read once + uint8 written
        med = float(np.median(t["imresize_u8_u8"]))
        tmed = float(np.median(t["torch_interpolate_f32"]))
        # the timed calls' result is the contract's (one plane: the numpy contract takes a while at these sizes)
        same = bool(np.array_equal(out[0].cpu().numpy(), imresize_host(host[0], output_shape=(Ho, Wo), out="int")))
        assert torch.equal(out, imresize(x, output_shape=(Ho, Wo), out="int"))
        res["sizes"].append({
            "in": [H, W], "out": [Ho, Wo], "taps": [Py, Px], "rows_first": bool(rows_first),
            "imresize_u8_u8": {"us_per_batch": round(med, 2),
                               "spread_us": [round(float(t["imresize_u8_u8"].min()), 2), round(float(t["imresize_u8_u8"].max()), 2)],
                               "bytes_moved": moved, "GBps": round(moved / med / 1e3, 1),
                               "hbm_share": round(moved / med / 1e6 / HBM_COPY_TBPS, 4)},
            "torch_interpolate_f32": {"us_per_batch": round(tmed, 2),
                                      "spread_us": [round(float(t["torch_interpolate_f32"].min()), 2),
                                                    round(float(t["torch_interpolate_f32"].max()), 2)]},
            "equals_contract": same})
    res["super_resolve_yuv420"] = d2h_per_frame()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
