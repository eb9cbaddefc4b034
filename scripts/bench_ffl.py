"""Focal frequency loss on the device: forward + backward of `focal_frequency_loss` (csrc/ffl.hip around the library's transforms)
against the plain torch restatement `ffl_reference` in f32 on the same device, at the HR crops of the training batch, (4,1,512,512)
and (4,3,512,512); HIP-event timed with the device synchronised, medians over timed calls after warm-ups, and the HIP calls split by
kernel (torch.profiler's device activity summed per kernel name).  Then the cost of the loss inside a training step: FCVSR-S on 4 clips
of 7x128x128 -> 512x512 (the training shape of bench.py), `TrainStep` (hipGraph replay, `HipAdam`) with `charbonnier_ffl_loss` against
`charbonnier_loss_mmedit`.
One JSON line.

    python scripts/bench_ffl.py [--warmup 10] [--iters 50] [--step-warmup 3] [--step-iters 10] [--no-step]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from fcvsr_amd.train import TrainStep, charbonnier_ffl_loss, charbonnier_loss_mmedit, ffl_reference, focal_frequency_loss


def event_ms(fn, warmup, iters):
    """Median ms of one call of fn, each call timed by its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def kernel_ms(fn, iters):
    """ms per call by kernel name (device time summed over `iters` calls, divided by iters)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        total_us = getattr(ev, "device_time_total", None)
        if total_us is None:
            total_us = getattr(ev, "cuda_time_total", 0.0)
        if total_us:
            name = ev.key.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            out[name] = out.get(name, 0.0) + total_us / 1e3 / iters
    return out


def fwd_bwd(loss_fn, pred, target):
    def run():
        pred.grad = None
        loss = loss_fn(pred, target)
        loss.backward()
        return loss.detach(), pred.grad
    return run


def train_step_ms(loss_fn, precision, warmup, iters):
    from fcvsr_amd.arch import CVSR_freq as A
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    model = A.GShiftNet_S()
    model.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    model = model.cuda()
    model.train_precision = precision
    g = torch.Generator().manual_seed(300)
    x = torch.rand(4, 7, 1, 128, 128, generator=g).cuda()
    hr = torch.rand(4, 1, 512, 512, generator=g).cuda()
    step = TrainStep(model, lr=1e-4, weight_decay=1e-5, loss_fn=loss_fn, reduce_op="mean", use_graph=True, optimizer="hip")

    def run():
        loss = step.local_backward(x, hr)
        step.reduce_and_update()
        return loss
    first = float(run().detach())                            # the loss of the first step (same weights and batch for either loss)
    ms, last = event_ms(run, warmup, iters)
    return ms, first, float(last.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--train-precision", choices=["f32", "bf16", "f16"], default="bf16")
    ap.add_argument("--no-step", action="store_true", help="skip the training-step comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ffl needs a HIP device")
    if args.warmup < 10 or args.iters < 50:
        raise SystemExit("use >= 10 warm-up and >= 50 timed calls")
    res = {}
    for shape in ((4, 1, 512, 512), (4, 3, 512, 512)):
        g = torch.Generator().manual_seed(sum(shape))
        pred = torch.rand(shape, generator=g).cuda().requires_grad_(True)
        target = torch.rand(shape, generator=g).cuda()
        tag = "x".join(str(v) for v in shape)
        hip_run, ref_run = fwd_bwd(focal_frequency_loss, pred, target), fwd_bwd(ffl_reference, pred, target)
        ms, (loss, grad) = event_ms(hip_run, args.warmup, args.iters)
        grad = grad.clone()
        res[f"hip_fwd_bwd_ms_{tag}"] = round(ms, 4)
        try:
            res[f"hip_kernel_ms_{tag}"] = {k: round(v, 4) for k, v in sorted(kernel_ms(hip_run, args.iters).items())}
        except Exception as exc:                               # a torch build without device tracing: the totals stand alone
            res[f"hip_kernel_ms_{tag}"] = f"unavailable: {type(exc).__name__}: {exc}"
        ms, (rloss, rgrad) = event_ms(ref_run, args.warmup, args.iters)
        res[f"torch_f32_fwd_bwd_ms_{tag}"] = round(ms, 4)
        res[f"loss_rel_diff_{tag}"] = float((loss - rloss).abs() / rloss.abs())
        res[f"grad_max_diff_over_max_{tag}"] = float((grad - rgrad).abs().max() / rgrad.abs().max())
    if not args.no_step:
        ms_ffl, loss_ffl, last_ffl = train_step_ms(charbonnier_ffl_loss, args.train_precision, args.step_warmup, args.step_iters)
        ms_cb, loss_cb, last_cb = train_step_ms(charbonnier_loss_mmedit, args.train_precision, args.step_warmup, args.step_iters)
        res["train_step"] = {"shape": "4 x 7x128x128 -> 512x512, FCVSR-S, hipGraph replay + HipAdam", "precision": args.train_precision,
                             "charbonnier_ffl_ms": round(ms_ffl, 3), "charbonnier_mmedit_ms": round(ms_cb, 3),
                             "ffl_cost_ms": round(ms_ffl - ms_cb, 3), "loss_first_last_charbonnier_ffl": [loss_ffl, last_ffl],
                             "loss_first_last_charbonnier_mmedit": [loss_cb, last_cb]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
