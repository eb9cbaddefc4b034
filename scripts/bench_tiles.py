"""What tiled inference (harness.tiles) costs and saves: the two kernels of csrc/tiles.hip as streamers, next to the self-ensemble's
two kernels from the same run, and `super_resolve_sequence` tiled against untiled with the peak of allocated device memory of each.

FCVSR-S (GShiftNet_S), bf16, synthetic weights, a resident one-channel sequence of --frame (540x960) LR frames, --tile (256) with
--overlap (16).
  kernels: `hip.tile_windows` / `hip.tile_merge` on --windows (8) windows, and `hip.ensemble_windows` / `hip.ensemble_merge` on the
           same windows, for f32 frames / an f32 result and for uint8 frames / a uint8 result; device-event time of --calls calls,
           median of --repeats rounds, and the achieved GB/s of the ALGORITHMIC bytes: every output element written once plus, per
           output element of a gather, one source sample read (tile windows re-read the overlaps; the ensemble reads every frame 8
           times), and for a merge every model-output element read once.  Share of the 8.0 TB/s HBM peak next to it.  Call times by
           device events, not kernel times from a trace.
  end to end: `super_resolve_sequence` on --frames (4) centre frames, untiled with --batch (1) windows per pass and tiled with
           each of --tile-batch (1,4) tile windows per pass (the harness's `batch`: also the frames per step); host clock around the call (it ends with the frames on the host), median of
           --repeats runs that alternate, `torch.cuda.max_memory_allocated` of one run of each after `reset_peak_memory_stats`.
One JSON line.

    python scripts/bench_tiles.py [--frame 540x960] [--tile 256] [--overlap 16] [--repeats 5] [--calls 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0


def _event_ms(fn, repeats, calls):
    """Median over `repeats` rounds of the device-event time per call of `calls` calls."""
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return float(np.median(ms)), float((max(ms) - min(ms)) / np.median(ms))


def _kernel_row(fn, nbytes, repeats, calls):
    for _ in range(3):
        fn()
    ms, spread = _event_ms(fn, repeats, calls)
    gbs = nbytes / ms / 1e6
    return {"ms": round(ms, 4), "spread": round(spread, 3), "MB": round(nbytes / 1e6, 2), "GBps": round(gbs, 1),
            "hbm_peak_share": round(gbs / HBM_PEAK_GBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", default="540x960", help="LR frame, HxW")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--tile-batch", default="1,4", help="tile windows per model pass (and frames per harness step); a comma list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 3 or args.calls < 5:
        raise SystemExit("the protocol is the median of at least 3 rounds of at least 5 calls")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiles.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd import hip
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.tiles import tile_plan
    from fcvsr_amd.harness.windows import window_indices
    from fcvsr_amd.weights import synthetic_state_dict

    H, W = (int(v) for v in args.frame.lower().split("x"))
    N, b = 8, args.windows
    plan = tile_plan(H, W, args.tile, args.overlap)
    rs = np.random.RandomState(31)
    x8 = torch.from_numpy(rs.randint(0, 256, (N, 1, H, W)).astype(np.uint8)).cuda()
    xf = x8.float() / 255
    idx = torch.tensor([window_indices(i % N, 7, N, "replicate") for i in range(3, 3 + b)], dtype=torch.int32).cuda()
    rec = {"frame": [H, W], "tile": [plan.th, plan.tw], "overlap": [plan.oy, plan.ox], "grid": [plan.ny, plan.nx], "windows": b,
           "model": "GShiftNet_S", "precision": "bf16", "repeats": args.repeats, "calls_per_round": args.calls, "kernels": {}}

    # kernels as streamers
    tiles = torch.rand((b, plan.ny, plan.nx, 1, 4 * plan.th, 4 * plan.tw), device="cuda")
    Hq, Wq = H + (-H) % 4, W + (-W) % 4
    ea, et = torch.rand((4, b, 1, 4 * Hq, 4 * Wq), device="cuda"), torch.rand((4, b, 1, 4 * Wq, 4 * Hq), device="cuda")
    n_tw = b * plan.ny * plan.nx * 7 * plan.th * plan.tw                     # elements a tile gather writes
    n_ew = 8 * b * 7 * Hq * Wq                                               # elements an ensemble gather writes
    n_out = b * 16 * H * W
    K = rec["kernels"]
    for name, src, isz in (("f32", xf, 4), ("u8", x8, 1)):
        K[f"tile_windows_{name}"] = _kernel_row(lambda: hip.tile_windows(src, idx, plan), n_tw * (4 + isz), args.repeats, args.calls)
        K[f"ensemble_windows_{name}"] = _kernel_row(lambda: hip.ensemble_windows(src, idx), n_ew * (4 + isz), args.repeats, args.calls)
    for name, kw, osz in (("f32", {}, 4), ("u8", dict(dtype=torch.uint8, quantise="round"), 1)):
        K[f"tile_merge_{name}"] = _kernel_row(lambda: hip.tile_merge(tiles, plan, H, W, **kw), tiles.numel() * 4 + n_out * osz,
                                              args.repeats, args.calls)
        K[f"ensemble_merge_{name}"] = _kernel_row(lambda: hip.ensemble_merge(ea, et, H, W, **kw),
                                                  (ea.numel() + et.numel()) * 4 + n_out * osz, args.repeats, args.calls)
    for kind in ("windows", "merge"):
        for name in ("f32", "u8"):
            rec[f"tile_over_ensemble_{kind}_{name}_GBps"] = round(K[f"tile_{kind}_{name}"]["GBps"] / K[f"ensemble_{kind}_{name}"]["GBps"], 3)
    del tiles, ea, et
    torch.cuda.empty_cache()

    # end to end
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    centres = list(range(2, 2 + args.frames))
    forms = {"untiled": dict(batch=args.batch)}
    for tb in (int(v) for v in args.tile_batch.split(",")):
        forms[f"tiled_batch{tb}"] = dict(batch=tb, tile=args.tile, tile_overlap=args.overlap)
    run = {n: (lambda kw=kw: super_resolve_sequence(m, x8, centres=centres, **kw)) for n, kw in forms.items()}
    peak, out = {}, {}
    for n, f in run.items():                                                 # warm-up, and the memory peak of one run of each
        f()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out[n] = f()
        torch.cuda.synchronize()
        peak[n] = (torch.cuda.max_memory_allocated(), base)
    secs = {n: [] for n in run}
    for _ in range(args.repeats):
        for n, f in run.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[n].append(time.perf_counter() - t0)
    for n in run:
        med = float(np.median(secs[n]))
        rec[n] = {"batch": forms[n]["batch"], "frames": len(centres), "seconds_median": round(med, 4),
                  "spread": round((max(secs[n]) - min(secs[n])) / med, 3), "frames_per_s": round(len(centres) / med, 3),
                  "peak_allocated_MB": round(peak[n][0] / 2 ** 20, 1), "allocated_before_MB": round(peak[n][1] / 2 ** 20, 1)}
    for n in run:
        if n != "untiled":
            rec[n]["frames_per_s_over_untiled"] = round(rec[n]["frames_per_s"] / rec["untiled"]["frames_per_s"], 3)
            rec[n]["untiled_peak_over_this_peak"] = round(rec["untiled"]["peak_allocated_MB"] / rec[n]["peak_allocated_MB"], 3)
            d = np.abs(out[n].astype(np.int32) - out["untiled"].astype(np.int32))         # two estimators: not expected to be 0
            rec[n]["abs_diff_to_untiled_u8"] = {"max": int(d.max()), "mean": round(float(d.mean()), 4)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
