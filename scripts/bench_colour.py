"""The two colour kernels (csrc/colour.hip) against the same integer specification written with torch operators on the same device,
and the file-to-file rate of an RGB model on a YUV 4:2:0 sequence.

Kernels: 16 frames, decode (YUV 4:2:0 -> planar RGB) at 180 x 320 and encode (RGB -> I420 frames) at 720 x 1280, the LR and SR
frames of the bench shape, at 8 and 10 bit, BT.709 limited range, both chroma sitings.  There is no earlier implementation, so the
yardstick is `harness.colour`'s specification in torch int32 operators (gathers for the up-sampler, slices for the down-sampler),
which is also checked to give the kernel's samples.  Kernel and torch form alternate in one process: --repeats rounds of --calls
calls each, every round timed by a host clock that ends in a device synchronise; the figure is the median round, with the spread
(max - min) / median next to it.  Algorithmic bytes are 1.5 + 3 samples per pixel.  The times are call times (launch included), not
kernel times from a trace: they say nothing about a share of HBM peak.

File to file: a synthetic 8-bit 320 x 180 I420 sequence of --frames frames through `super_resolve_yuv420_rgb` with FCVSR_SNet
(bf16, 2 streams, hipGraph), frames/s including read, upload, both conversions, download and write, next to the model-only rate
(`super_resolve_u8` on resident windows, the same batches).  One JSON line.

    python scripts/bench_colour.py [--repeats 7] [--calls 50] [--frames 60] [--no-file] [--out FILE.json]
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


def _i32(t, P):
    """uint8 / uint16 device tensor -> int32 samples clamped to P (uint16 through its int16 bits)."""
    if t.dtype == torch.uint16:
        return (t.view(torch.int16).to(torch.int32) & 0xFFFF).clamp_(max=P)
    return t.to(torch.int32)


def _out(t, dtype):
    return t.to(torch.uint8) if dtype == torch.uint8 else t.to(torch.int16).view(torch.uint16)


class TorchColour:
    """The specification of harness.colour in torch int32 operators on the device."""

    def __init__(self, spec, h, w, device):
        from fcvsr_amd.harness.colour import coefficients
        self.k, self.P, self.spec = coefficients(spec), spec.peak, spec
        Y, X = torch.arange(2 * h, device=device), torch.arange(2 * w, device=device)
        self.j, self.i = Y >> 1, X >> 1
        self.j2 = torch.where(Y % 2 == 0, self.j - 1, self.j + 1).clamp_(0, h - 1)
        i2 = torch.where(X % 2 == 0, self.i - 1, self.i + 1) if spec.chroma_loc == "center" else torch.where(X % 2 == 0, self.i, self.i + 1)
        self.i2 = i2.clamp_(0, w - 1)
        self.left = (2 * torch.arange(w, device=device) - 1).clamp_(min=0)

    def up(self, c):
        a, b = c.index_select(1, self.j), c.index_select(1, self.j2)
        if self.spec.chroma_loc == "center":
            r = 3 * a + b
            return (3 * r.index_select(2, self.i) + r.index_select(2, self.i2) + 8) >> 4
        r = 3 * a + b
        return (r.index_select(2, self.i) + r.index_select(2, self.i2) + 4) >> 3

    def decode(self, y, u, v):
        k, P = self.k, self.P
        yt = k["cy"] * (_i32(y, P) - k["y_off"]) + (1 << 13)
        U, V = self.up(_i32(u, P)) - k["c_off"], self.up(_i32(v, P)) - k["c_off"]
        rgb = torch.stack([(yt + k["rv"] * V) >> 14, (yt - k["gu"] * U - k["gv"] * V) >> 14, (yt + k["bu"] * U) >> 14], 1)
        return _out(rgb.clamp_(0, P), y.dtype)

    def encode(self, rgb):
        k, P = self.k, self.P
        x = _i32(rgb, P)
        R, G, B = x[:, 0], x[:, 1], x[:, 2]
        N, H, W = R.shape
        y = (((k["kr"] * R + k["kg"] * G + k["kb"] * B + (1 << 13)) >> 14) + k["y_off"]).clamp_(0, P)
        planes = [y.reshape(N, -1)]
        for c in (-k["ur"] * R - k["ug"] * G + k["ub"] * B, k["vr"] * R - k["vg"] * G - k["vb"] * B):
            t = c[:, 0::2] + c[:, 1::2]
            if self.spec.chroma_loc == "center":
                q = (t[..., 0::2] + t[..., 1::2] + (1 << 15)) >> 16
            else:
                q = (t.index_select(2, self.left) + 2 * t[..., 0::2] + t[..., 1::2] + (1 << 16)) >> 17
            planes.append((q + k["c_off"]).clamp_(0, P).reshape(N, -1))
        return _out(torch.cat(planes, 1), rgb.dtype)


def _rounds(fns, repeats, calls):
    """{name: [us per call, one per round]}: the functions alternate within every round."""
    us = {n: [] for n in fns}
    for _ in range(repeats):
        for n, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            us[n].append((time.perf_counter() - t0) * 1e6 / calls)
    return us


def _stats(us, nbytes):
    v = np.array(us)
    med = float(np.median(v))
    return {"us_median": round(med, 2), "us_min": round(float(v.min()), 2), "us_max": round(float(v.max()), 2),
            "spread": round(float((v.max() - v.min()) / med), 4), "algorithmic_GBps": round(nbytes / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5 or args.calls < 50:
        raise SystemExit("the protocol is the median of at least 5 rounds of at least 50 calls")
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour.py needs a HIP device (there is no CPU fallback)")
    from fcvsr_amd import hip
    from fcvsr_amd.harness.colour import ColourSpec, i420_planes, rgb_to_i420, yuv420_to_rgb

    dev, N = torch.device("cuda:0"), 16
    rs = np.random.RandomState(77)
    rec = {"frames": N, "repeats": args.repeats, "calls_per_round": args.calls, "kernels": {}}
    for d in (8, 10):
        for loc in ("left", "center"):
            spec = ColourSpec(chroma_loc=loc, bit_depth=d)
            P, ndt, size = spec.peak, (np.uint8 if d == 8 else np.uint16), (1 if d == 8 else 2)
            for what, (H, W) in (("decode", (180, 320)), ("encode", (720, 1280))):
                tc = TorchColour(spec, H // 2, W // 2, dev)
                if what == "decode":
                    frames = hip.bits16(torch.from_numpy(rs.randint(0, P + 1, (N, H * W * 3 // 2)).astype(ndt))).to(dev).view(spec.dtype)
                    y, u, v = i420_planes(frames, H, W)
                    fns = {"kernel": lambda: yuv420_to_rgb(y, u, v, spec), "torch": lambda: tc.decode(y, u, v)}
                else:
                    rgb = hip.bits16(torch.from_numpy(rs.randint(0, P + 1, (N, 3, H, W)).astype(ndt))).to(dev).view(spec.dtype)
                    fns = {"kernel": lambda: rgb_to_i420(rgb, spec), "torch": lambda: tc.encode(rgb)}
                a, b = fns["kernel"](), fns["torch"]()                 # warm-up, and the two forms agree
                same = bool(torch.equal(hip.bits16(a), hip.bits16(b)))
                for f in fns.values():
                    for _ in range(5):
                        f()
                us = _rounds(fns, args.repeats, args.calls)
                nbytes = N * H * W * size * 9 // 2                       # 1.5 + 3 samples per pixel
                r = {n: _stats(v, nbytes) for n, v in us.items()}
                r["torch_over_kernel"] = round(r["torch"]["us_median"] / r["kernel"]["us_median"], 2)
                r["equal"] = same
                r["algorithmic_bytes"] = nbytes
                rec["kernels"][f"{what}_{H}x{W}_{d}bit_{loc}"] = r
    rec["all_equal"] = all(r["equal"] for r in rec["kernels"].values())
    rec["kernel_no_slower_than_torch"] = all(r["torch_over_kernel"] >= 1.0 for r in rec["kernels"].values())

    if not args.no_file:
        from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
        from fcvsr_amd.arch.schema import state_dict_shapes
        from fcvsr_amd.harness.windows import window_indices
        from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
        from fcvsr_amd.weights import synthetic_state_dict
        H, W, F, B = 180, 320, args.frames, args.batch
        m = FCVSR_SNet()
        m.load_state_dict(synthetic_state_dict(state_dict_shapes("FCVSR_SNet"), gain=0.5), strict=True)
        m = m.cuda()
        m.precision, m.streams, m.use_graph = "bf16", 2, True
        with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
            src, dst = os.path.join(tmp, f"Synth_{W}x{H}_{F}F.yuv"), os.path.join(tmp, f"Synth_{4 * W}x{4 * H}_{F}F.yuv")
            write_yuv420(src, rs.randint(0, 256, (F, H, W)).astype(np.uint8), rs.randint(0, 256, (F, H // 2, W // 2)).astype(np.uint8),
                         rs.randint(0, 256, (F, H // 2, W // 2)).astype(np.uint8))
            super_resolve_yuv420_rgb(m, src, dst, W, H, batch=B)          # warm-up (the ragged last batch's graph too)
            fps = []
            for _ in range(args.file_repeats):
                torch.cuda.synchronize()
                st = super_resolve_yuv420_rgb(m, src, dst, W, H, batch=B)
                fps.append(st["fps"])
            x = torch.from_numpy(rs.randint(0, 256, (F, 3, H, W)).astype(np.uint8)).to(dev)
            wins = [torch.stack([x[j] for j in [window_indices(i, 7, F, "replicate") for i in range(s, min(F, s + B))]], 0)
                    for s in range(0, F, B)]
            model_fps = []
            for _ in range(args.file_repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for w_ in wins:
                    m.super_resolve_u8(w_)
                torch.cuda.synchronize()
                model_fps.append(F / (time.perf_counter() - t0))
        v, mv = np.array(fps), np.array(model_fps)
        rec["file_to_file_8bit"] = {"frames": F, "batch": B, "fps_median": round(float(np.median(v)), 2), "fps_min": round(float(v.min()), 2),
                                    "fps_max": round(float(v.max()), 2), "model_only_fps_median": round(float(np.median(mv)), 2),
                                    "model_only_fps_min": round(float(mv.min()), 2), "model_only_fps_max": round(float(mv.max()), 2),
                                    "bytes_read": st["bytes_read"], "bytes_written": st["bytes_written"]}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not (rec["all_equal"] and rec["kernel_no_slower_than_torch"]):
        raise SystemExit("a kernel differs from the torch form or is slower than it")


if __name__ == "__main__":
    main()
