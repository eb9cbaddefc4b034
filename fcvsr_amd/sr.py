"""``python -m fcvsr_amd.sr``: raw 4:2:0 video in, 4x super-resolved raw video out, through pipes or files.

    ffmpeg -i in.mp4 -f rawvideo -pix_fmt nv12 - | \\
        python -m fcvsr_amd.sr --model FCVSR_SNet --weights fcvsr_s.pth --size 480x270 --pix-fmt nv12 - - | \\
        ffmpeg -f rawvideo -pix_fmt nv12 -s 1920x1080 -r 24 -i - out.mkv

Nothing but the model and `harness.stream.stream_yuv420` (its docstring says what every option means); the stats go to stderr as
one JSON line.  With ``--reference GT.yuv`` the frames that are written are scored against a ground-truth video of the delivered
size (PSNR of Y, U, V and all three, SSIM of Y; ``inf`` prints as ``Infinity``), ``--scores-log`` writes them per frame as CSV, and
``--scores-only`` evaluates without writing DST.
"""
from __future__ import annotations

import argparse
import json
import sys

MODELS = ("GShiftNet_S", "GShiftNet", "FCVSR_SNet", "FCVSRNet")
PIX_FMTS = ("yuv420p", "yuv420p10le", "nv12", "p010le")                   # harness.surfaces.PIX_FMTS (that module needs numpy)


def _size(text: str):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected WxH, got {text!r}")
    return w, h


def _cuts(text: str):
    return "auto" if text == "auto" else [int(v) for v in text.split(",") if v]


def _active(text: str):
    if text == "auto":
        return "auto"
    try:
        t, b, l, r = (int(v) for v in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected auto or T:B:L:R, got {text!r}")
    return t, b, l, r


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m fcvsr_amd.sr", description="4x video super-resolution of raw YUV 4:2:0, "
                                "streamed: SRC and DST are files, or - for stdin / stdout.")
    p.add_argument("--model", choices=MODELS, required=True)
    p.add_argument("--weights", required=True, metavar="W.pth", help="the model's state dict (torch.load, weights only)")
    p.add_argument("--size", type=_size, required=True, metavar="WxH", help="size of the source frames")
    p.add_argument("--pix-fmt", choices=PIX_FMTS, default="yuv420p")
    p.add_argument("--out-pix-fmt", choices=PIX_FMTS, default=None, help="default: --pix-fmt (same bit depth)")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--padding", default="replicate", choices=("replicate", "reflection", "reflection_circle", "circle"))
    p.add_argument("--quantise", default="truncate", choices=("truncate", "round"))
    p.add_argument("--ensemble", default=None, choices=("spatial", "spatial+temporal"))
    p.add_argument("--tile", type=_size, default=None, metavar="WxH", help="run the model on overlapping tiles of this size")
    p.add_argument("--tile-overlap", type=int, default=16)
    p.add_argument("--static-tiles", action="store_true", help="with --tile: do not run a tile window again whose frames did not "
                   "change since the previous frame of its group; the bytes written are the same")
    p.add_argument("--cuts", type=_cuts, default=None, metavar="auto|N,N,...", help="scene cuts: detect them, or frame numbers")
    p.add_argument("--cut-threshold", type=float, default=10.0)
    p.add_argument("--active", type=_active, default=None, metavar="auto|T:B:L:R", help="run the model on the picture only: detect "
                   "letterbox / pillarbox bars, or the box top:bottom:left:right in source samples (half-open)")
    p.add_argument("--active-limit", type=float, default=24.0, help="--active auto: a row or column is picture when its mean "
                   "sample lies above this (8-bit scale)")
    p.add_argument("--output-size", type=_size, default=None, metavar="WxH", help="deliver this size in place of 4x")
    p.add_argument("--matrix", default="bt709", choices=("bt601", "bt709"), help="RGB models: the stream's matrix")
    p.add_argument("--full-range", action="store_true", help="RGB models: full-range code values")
    p.add_argument("--chroma-loc", default="left", choices=("left", "center"), help="RGB models: chroma siting")
    p.add_argument("--max-frames", type=int, default=None)
    p.add_argument("--reference", default=None, metavar="PATH", help="ground-truth raw video of the delivered size (- is not taken: "
                   "stdin is SRC's): PSNR per plane and luma SSIM of the frames that are written go into the stats")
    p.add_argument("--reference-pix-fmt", choices=PIX_FMTS, default=None, help="default: the output format (same bit depth)")
    p.add_argument("--crop-border", type=int, default=4, help="--reference: luma border left out of the scores (even; chroma half)")
    p.add_argument("--baseline", default=None, choices=("bicubic",), help="--reference: also score the bicubic up-scale of the luma")
    p.add_argument("--tof", action="store_true", help="--reference: also score tOF, the Farneback-flow distance to the ground truth "
                   "(a restatement of the cv2 call; column tof of --scores-log)")
    p.add_argument("--scores-only", action="store_true", help="--reference: evaluate only; DST is neither opened nor written")
    p.add_argument("--scores-log", default=None, metavar="FILE", help="--reference: one CSV line per frame, "
                   "frame,psnr_y,psnr_u,psnr_v,psnr_yuv,ssim_y, written at the end")
    p.add_argument("--device", default="cuda")
    p.add_argument("src", metavar="SRC")
    p.add_argument("dst", metavar="DST")
    return p


def main(argv=None) -> int:
    p = parser()
    a = p.parse_args(argv)
    if a.reference is None and (a.scores_only or a.scores_log is not None or a.baseline is not None
                                or a.reference_pix_fmt is not None or a.tof):
        p.error("--scores-only, --scores-log, --baseline, --tof and --reference-pix-fmt need --reference")
    import torch

    from .arch import CVSR_freq, fcvsr_rgb
    from .harness.colour import ColourSpec
    from .harness.stream import stream_yuv420
    model = getattr(fcvsr_rgb if a.model.startswith("FCVSR") else CVSR_freq, a.model)()
    sd = torch.load(a.weights, map_location="cpu", weights_only=True)
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    model.load_state_dict({k[len("generator."):] if k.startswith("generator.") else k: v for k, v in sd.items()})
    model = model.to(a.device)
    bits = 10 if a.pix_fmt in ("yuv420p10le", "p010le") else 8
    active = a.active
    if active == "auto":
        from .harness.active import ActiveSpec
        active = ActiveSpec(limit=a.active_limit)
    dst = None if a.scores_only else sys.stdout.buffer if a.dst == "-" else a.dst
    stats = stream_yuv420(model, sys.stdin.buffer if a.src == "-" else a.src, dst, a.size[0], a.size[1], pix_fmt=a.pix_fmt, out_pix_fmt=a.out_pix_fmt,
                          colour=ColourSpec(a.matrix, a.full_range, a.chroma_loc, bits), batch=a.batch, padding=a.padding,
                          quantise=a.quantise, ensemble=a.ensemble, tile=None if a.tile is None else (a.tile[1], a.tile[0]),
                          tile_overlap=a.tile_overlap, cuts=a.cuts, cut_threshold=a.cut_threshold,
                          output_shape=None if a.output_size is None else (a.output_size[1], a.output_size[0]),
                          max_frames=a.max_frames, active=active, static_tiles=a.static_tiles, reference=a.reference,
                          reference_pix_fmt=a.reference_pix_fmt, crop_border=a.crop_border, baseline=a.baseline, tof=a.tof)
    if a.dst == "-" and dst is not None:
        sys.stdout.buffer.flush()
    if a.scores_log is not None:
        from .harness.reference import scores_csv
        with open(a.scores_log, "w") as f:
            f.write(scores_csv(stats))
    print(json.dumps({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in stats.items()}), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
