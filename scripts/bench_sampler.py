"""Training-batch production at bench.py's training shape (4 clips of 7x128x128 -> 512x512 from 32-frame 270x480 / 1080x1920
uint8 sequences, or with --bits 10 uint16 sequences of 10-bit samples): the device clip sampler against the host chain the
repository offered before it.

    python scripts/bench_sampler.py batch   [--batches 100] [--out FILE.json]
        (a) DeviceClipSampler: draws + descriptors + two launches, per batch, device-synchronised;
        (b) host chain: random_crop + augment + to_tensor per clip on frames ALREADY DECODED in RAM (no PNG decode: this flatters
            (b) against the reference loader), torch.stack, .to(device) from pageable and from pinned memory.
        The three alternate batch by batch in one process; medians, and the clips/s each sustains.
        --bits 10: the sequences are 10-bit, and a DeviceClipSampler over 8-bit sequences of the same shapes ("sampler_8bit") takes
        its turn in the same alternation: the 10-bit batch against the 8-bit batch in one run on one device.
    python scripts/bench_sampler.py fit     [--steps 64] [--out FILE.json]
        one `fit` epoch of --steps steps of 4 clips (eager step, no graph) fed by the sampler and by the host chain: time per step
        including the data, and the host time spent inside the data iterator; the two alternate --repeats times.
    rocprofv3 --kernel-trace --output-format csv -d DIR -o k -- python scripts/bench_sampler.py kernel --order DIR/order.json
    python scripts/bench_sampler.py summarise --trace DIR/..._kernel_trace.csv --order DIR/order.json [--out FILE.json]
        the kernel alone: launches of 4 and 64 clips, flag sets without and with the transpose bit, in a recorded order; `summarise`
        cuts the trace by that order: time per launch, bytes (1 read + 4 written per pixel; --bits 10: 2 read) and the share of
        HBM bandwidth.  Give `kernel` and `summarise` the same --bits.
"""
import argparse
import csv
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, H, W, CROP, FRAMES, CLIPS = 32, 270, 480, 128, 7, 4
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12          # spec peak and what streaming kernels reach on this card (bytes/s)
KERNELS = {8: "clip_batch_u8_kernel", 10: "clip_batch_u16_kernel"}
DTYPES = {8: np.uint8, 10: np.uint16}


def sequences(n, seed=0, bits=8):
    g = np.random.RandomState(seed)
    dt = DTYPES[bits]
    return [(g.randint(0, 1 << bits, (N, 1, H, W), dtype=dt), g.randint(0, 1 << bits, (N, 1, 4 * H, 4 * W), dtype=dt)) for _ in range(n)]


def host_clip(seqs, rnd):
    """One clip as the reference's __getitem__ + transforms make it, from decoded frames in RAM."""
    from fcvsr_amd.train.step import augment, random_crop, to_tensor
    lr, hr = seqs[rnd.randrange(len(seqs))]
    first = rnd.randint(0, N - FRAMES)
    sample = {"lr_imgs": lr[first:first + FRAMES, 0], "hr_imgs": hr[first + FRAMES // 2:first + FRAMES // 2 + 1, 0]}
    return to_tensor(augment(random_crop(sample, CROP)))


def host_batch(seqs, rnd, pinned, dev):
    clips = [host_clip(seqs, rnd) for _ in range(CLIPS)]
    out = {k: torch.stack([c[k] for c in clips]) for k in ("lr_imgs", "hr_imgs")}
    if pinned:
        return {k: v.pin_memory().to(dev, non_blocking=True) for k, v in out.items()}
    return {k: v.to(dev) for k, v in out.items()}


def forever(sampler):
    epoch = 0
    while True:
        yield from sampler(epoch)
        epoch += 1


def stats(ms):
    v = np.array(ms)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "p90_ms": round(float(np.percentile(v, 90)), 4),
            "clips_per_s": round(CLIPS / (float(np.median(v)) * 1e-3), 1)}


def mode_batch(args, dev):
    from fcvsr_amd.train import DeviceClipSampler
    seqs = sequences(args.sequences, bits=args.bits)
    sampler = DeviceClipSampler(seqs, batch=CLIPS, crop=CROP, seed=1, device=dev)
    dev_it, rnd = forever(sampler), random.Random(2)
    np.random.seed(3)
    random.seed(4)
    makers = {"sampler": lambda: next(dev_it), "host_pageable": lambda: host_batch(seqs, rnd, False, dev),
              "host_pinned": lambda: host_batch(seqs, rnd, True, dev)}
    if args.bits == 10:                                        # the 8-bit batch of the same shapes and draws, in the same alternation
        it8 = forever(DeviceClipSampler(sequences(args.sequences, bits=8), batch=CLIPS, crop=CROP, seed=1, device=dev))
        makers["sampler_8bit"] = lambda: next(it8)
    times = {k: [] for k in makers}
    for it in range(args.warmup + args.batches):
        for name, make in makers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = make()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert b["lr_imgs"].shape == (CLIPS, 1, FRAMES, CROP, CROP) and b["hr_imgs"].shape == (CLIPS, 1, 1, 4 * CROP, 4 * CROP)
            if it >= args.warmup:
                times[name].append(dt)
    rec = {"workload": f"{CLIPS} clips of {FRAMES}x{CROP}x{CROP} -> {4 * CROP}x{4 * CROP} from {args.sequences} {np.dtype(DTYPES[args.bits]).name} sequences of {N} frames "
                       f"{H}x{W} / {4 * H}x{4 * W}; per batch, device-synchronised, {args.batches} batches after {args.warmup} warm-up",
           "note": "host chain works on frames already decoded in RAM (no per-clip PNG decode as in the reference loader): flatters it",
           "bytes_uploaded_per_batch": {"sampler_descriptors": (CLIPS * FRAMES + CLIPS) * 24,
                                        "host_chain_f32": CLIPS * (FRAMES * CROP * CROP + 16 * CROP * CROP) * 4}}
    rec.update({k: stats(v) for k, v in times.items()})
    return rec


def mode_fit(args, dev):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.train import DeviceClipSampler
    from fcvsr_amd.train.step import fit
    from fcvsr_amd.weights import synthetic_state_dict
    seqs = sequences(args.sequences, bits=args.bits)
    from fcvsr_amd.hip import bits16
    resident = [tuple(bits16(torch.from_numpy(a)).to(dev).view(torch.from_numpy(a).dtype) for a in pair) for pair in seqs]   # uploaded once, shared below

    def model():
        m = GShiftNet_S()
        m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
        m = m.to(dev)
        m.train_precision = "bf16"
        return m

    n_items = args.steps * CLIPS                                # one epoch = --steps batches: items wrap round the sequences
    sampler = DeviceClipSampler([resident[i % len(seqs)] for i in range(n_items)], batch=CLIPS, crop=CROP, seed=1, device=dev)
    rnd = random.Random(2)

    def host(epoch):
        for _ in range(args.steps):
            yield host_batch(seqs, rnd, True, dev)

    out = {"sampler": [], "host_pinned": []}
    data_ms = {"sampler": [], "host_pinned": []}

    def timed(feed, acc):
        """`feed` with the host time spent inside it (making and enqueueing a batch; no device synchronisation) added to acc[0]."""
        def gen(epoch):
            it = iter(feed(epoch))
            while True:
                t0 = time.perf_counter()
                try:
                    b = next(it)
                except StopIteration:
                    return
                finally:
                    acc[0] += time.perf_counter() - t0
                yield b
        return gen

    fit(model(), lambda e: list(sampler(e))[:4], epochs=1, device=dev, log=lambda m: None)      # warm-up: kernels loaded, allocator grown
    for rep in range(args.repeats):
        for name, feed in (("sampler", sampler), ("host_pinned", host)):
            m, acc = model(), [0.0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hist = fit(m, timed(feed, acc), epochs=1, device=dev, log=lambda s: None)
            torch.cuda.synchronize()
            out[name].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 3))
            data_ms[name].append(round(acc[0] * 1e3 / args.steps, 3))
            assert np.isfinite(hist[0])
    return {"workload": f"one fit epoch of {args.steps} steps x {CLIPS} clips, GShiftNet_S bf16 training, eager step (use_graph=False), "
                        f"{len(seqs)} resident sequences; ms per step including data and the model / optimizer set-up of fit",
            "ms_per_step": out, "host_ms_per_step_inside_the_data_iterator": data_ms, "clips_per_s": {k: round(CLIPS / (min(v) * 1e-3), 1) for k, v in out.items()}}


KERNEL_CASES = [(clips, tr) for clips in (4, 64) for tr in (0, 1)]


def mode_kernel(args, dev):
    """Launches only (run under rocprofv3): per case `--iters` batches whose clips all carry flag sets without / with the transpose
    bit.  Every batch keeps its output alive, so a launch writes memory no earlier launch of the case wrote."""
    from fcvsr_amd.train import BatchPlan, DeviceClipSampler
    seqs = sequences(args.sequences, bits=args.bits)
    sampler = DeviceClipSampler(seqs, batch=64, crop=CROP, seed=1, device=dev)
    g = np.random.RandomState(7)
    order = []
    for clips, tr in KERNEL_CASES:
        keep = []
        for it in range(args.warmup + args.iters):
            fl = g.randint(0, 4, clips) + 4 * tr
            bp = BatchPlan(g.randint(0, len(seqs), clips), g.randint(0, N - FRAMES + 1, clips), g.randint(0, H - CROP, clips),
                           g.randint(0, W - CROP, clips), (fl & 1) > 0, (fl & 2) > 0, (fl & 4) > 0)
            keep.append(sampler.build(bp))
            for s in (CROP, 4 * CROP):                                  # the LR launch, then the HR launch
                order.append({"clips": clips, "transpose": tr, "s": s, "planes": clips * (FRAMES if s == CROP else 1),
                              "timed": it >= args.warmup})
        torch.cuda.synchronize()
        del keep
    with open(args.order, "w") as f:
        json.dump(order, f)
    return {"launches": len(order), "order_file": args.order}


def mode_summarise(args):
    order = json.load(open(args.order))
    KERNEL, src_bytes = KERNELS[args.bits], np.dtype(DTYPES[args.bits]).itemsize
    rows = [r for r in csv.DictReader(open(args.trace)) if KERNEL in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(order), f"{len(rows)} dispatches of {KERNEL} in the trace, {len(order)} launches recorded"
    groups = {}
    for o, r in zip(order, rows):
        if o["timed"]:
            groups.setdefault((o["clips"], o["transpose"], o["s"]), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = []
    for (clips, tr, s), ns in sorted(groups.items()):
        planes = clips * (FRAMES if s == CROP else 1)
        nbytes = planes * s * s * (src_bytes + 4)
        med = float(np.median(ns))
        out.append({"clips": clips, "transpose": tr, "plane": s, "planes": planes, "launches": len(ns), "median_us": round(med / 1e3, 2),
                    "min_us": round(min(ns) / 1e3, 2), "bytes": nbytes, "GB_per_s": round(nbytes / med, 1),
                    "share_of_8TBs_peak": round(nbytes / (med * 1e-9) / HBM_PEAK, 3),
                    "share_of_6.3TBs_streaming": round(nbytes / (med * 1e-9) / HBM_STREAM, 3)})
    return {"kernel": KERNEL, "source": "rocprofv3 --kernel-trace", "bytes_model": f"{src_bytes} byte(s) read + 4 bytes written per output pixel",
            "cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["batch", "fit", "kernel", "summarise"])
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sequences", type=int, default=None)
    ap.add_argument("--bits", type=int, choices=[8, 10], default=8, help="sample depth of the sequences (10: uint16 containers)")
    ap.add_argument("--order", default="order.json")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "summarise":
        rec = mode_summarise(args)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_sampler.py needs a HIP device (there is no CPU fallback)")
        if args.sequences is None:
            args.sequences = 8
        rec = {"batch": mode_batch, "fit": mode_fit, "kernel": mode_kernel}[args.mode](args, torch.device("cuda:0"))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
