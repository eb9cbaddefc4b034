"""CPU: the contract of ``reference=`` (`harness.reference`): exact plane sums, PSNR bit-equal to `metrics.psnr`, the combined and
whole-sequence numbers, the prologue's errors (all before a file is opened), the command-line flags and the new C symbol."""
import math
import os
import re

import numpy as np
import pytest

from fcvsr_amd.harness import metrics
from fcvsr_amd.harness import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((72, 80), (54, 60), (36, 40), (27, 30))


def _planes(bits, P, h, w, seed=0):
    rs = np.random.RandomState(seed + bits + h)
    top = 256 if bits == 8 else 1536                                      # 10-bit containers reach above 1023
    dt = np.uint8 if bits == 8 else np.uint16
    a = rs.randint(0, top, (P, h, w)).astype(dt)
    b = np.clip(a.astype(np.int64) + rs.randint(-9, 10, (P, h, w)), 0, top - 1).astype(dt)
    return a, b


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("crop", [0, 2])
def test_plane_sse_host_is_the_plain_integer_loop(bits, crop):
    a, b = _planes(bits, 3, 7, 9)
    want = []
    for p in range(3):
        s = 0
        for i in range(crop, 7 - crop):
            for j in range(crop, 9 - crop):
                d = min(int(a[p, i, j]), 1023) - min(int(b[p, i, j]), 1023)
                s += d * d
        want.append(s)
    got = R.plane_sse_host(a, b, crop)
    assert got.dtype == np.int64 and got.tolist() == want
    assert R.plane_sse_host(a[:0], b[:0], crop).shape == (0,)
    assert R.plane_sse_host(a, a, crop).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        R.plane_sse_host(a, b, 4)                                         # 2 * 4 >= 7
    with pytest.raises(ValueError):
        R.plane_sse_host(a, b[:, :-1], 0)
    with pytest.raises(ValueError):
        R.plane_sse_host(a.astype(np.int32), b.astype(np.int32), 0)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_psnr_from_the_sums_is_bit_equal_to_metrics_psnr(bits, size):
    H, W = size
    crop, peak = 4, R.PEAKS[bits]
    y, gy = _planes(bits, 3, H, W, 1)
    u, gu = _planes(bits, 3, H // 2, W // 2, 2)
    v, gv = _planes(bits, 3, H // 2, W // 2, 3)
    gy[2], gu[2], gv[2] = y[2], u[2], v[2]                                # frame 2: equal planes
    sse = np.stack([R.plane_sse_host(y, gy, crop), R.plane_sse_host(u, gu, crop // 2), R.plane_sse_host(v, gv, crop // 2)], 1)
    sizes = R.plane_sizes(H, W, crop)
    assert sizes == ((H - 8) * (W - 8), (H // 2 - 4) * (W // 2 - 4), (H // 2 - 4) * (W // 2 - 4))
    got = R.scores_from_sse(sse, sizes, peak)
    rd = lambda a: np.minimum(a.astype(np.int64), 1023)                   # both sides read min(k, 1023)
    for k, (name, a, b, c) in enumerate((("psnr_y", y, gy, crop), ("psnr_u", u, gu, crop // 2), ("psnr_v", v, gv, crop // 2))):
        assert got[name].dtype == np.float64 and got[name].shape == (3,)
        for n in range(3):
            want = metrics.psnr(rd(a[n]), rd(b[n]), c, peak)
            assert got[name][n] == want and (n != 2 or math.isinf(want)), (name, n, got[name][n], want)
    for n in range(3):                                                    # the combined number, by the formula
        tot, cnt = int(sse[n].sum()), sum(sizes)
        want = float("inf") if tot == 0 else float(20.0 * np.log10(float(peak) / np.sqrt(np.float64(tot) / np.float64(cnt))))
        assert got["psnr_yuv"][n] == want
    assert np.isinf(got["psnr_yuv"][2]) and np.isfinite(got["psnr_yuv"][:2]).all()


def test_sequence_scores_means_and_globals():
    sse = np.array([[100, 10, 20], [0, 0, 0], [300, 30, 0]], dtype=np.int64)
    sizes, peak = (64, 16, 16), 255
    s = R.sequence_scores(sse, [0.5, 1.0, 0.25], sizes, peak)
    assert s["reference_frames"] == 3 and s["sse"].dtype == np.int64 and s["sse"].tolist() == sse.tolist()
    assert s["ssim_y"].tolist() == [0.5, 1.0, 0.25] and s["ssim_y_mean"] == float(np.mean([0.5, 1.0, 0.25]))
    assert math.isinf(s["psnr_y_mean"]) and math.isinf(s["psnr_yuv_mean"])          # frame 1 is inf
    f = lambda t, n: float(20.0 * np.log10(255.0 / np.sqrt(np.float64(t) / np.float64(n))))
    assert s["psnr_y_global"] == f(400, 3 * 64) and s["psnr_u_global"] == f(40, 3 * 16) and s["psnr_v_global"] == f(20, 3 * 16)
    assert s["psnr_yuv_global"] == f(460, 3 * 96)
    assert s["psnr_v"][2] == float("inf") and s["psnr_u"][0] == f(10, 16)
    one = R.sequence_scores(sse[:1], [0.5], sizes, peak)                  # one frame: global == per-frame == mean
    assert one["psnr_yuv_global"] == one["psnr_yuv"][0] == one["psnr_yuv_mean"]
    with pytest.raises(ValueError):
        R.scores_from_sse(sse, sizes, 1020)
    with pytest.raises(ValueError):
        R.scores_from_sse(sse.astype(np.float64), sizes, 255)
    csv = R.scores_csv(s).splitlines()
    assert csv[0] == "frame,psnr_y,psnr_u,psnr_v,psnr_yuv,ssim_y" and len(csv) == 4 and csv[2].startswith("1,inf,inf,inf,inf,1.0")


class _Model:
    """Enough of a model for the prologue; nothing of it runs."""

    def __init__(self, ch):
        self._img_ch = ch

    def parameters(self):
        raise AssertionError("the prologue must raise before the model is touched")


def _entry_points(tmp_path):
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    missing = str(tmp_path / "missing.yuv")                               # opening any of these would raise FileNotFoundError
    return ((lambda dst=missing, **kw: stream_yuv420(_Model(1), missing, dst, 20, 18, **kw)),
            (lambda dst=missing, **kw: super_resolve_yuv420(_Model(1), missing, dst, 20, 18, **kw)),
            (lambda dst=missing, **kw: super_resolve_yuv420_rgb(_Model(3), missing, dst, 20, 18, **kw)))


def test_the_prologue_raises_before_a_file_is_opened(tmp_path):
    gt = str(tmp_path / "missing_gt.yuv")
    for k, run in enumerate(_entry_points(tmp_path)):
        with pytest.raises(ValueError, match="crop_border"):
            run(reference=gt, crop_border=3)
        with pytest.raises(ValueError, match="crop_border"):
            run(reference=gt, crop_border=-2)
        with pytest.raises(ValueError, match="SSIM region"):
            run(reference=gt, crop_border=32)                             # 72 - 64 - 10 < 1
        with pytest.raises(ValueError, match="SSIM region"):
            run(reference=gt, output_shape=(18, 60))                      # 18 - 8 - 10 < 1
        if k != 1:                                                        # super_resolve_yuv420 takes no baseline= (test_upscale_cpu.py)
            with pytest.raises(ValueError, match="baseline"):
                run(baseline="bicubic")
            with pytest.raises(ValueError, match="baseline"):
                run(reference=gt, baseline="bilinear")
        with pytest.raises(ValueError, match="dst=None"):
            run(dst=None)
        if k == 0:
            with pytest.raises(ValueError, match="reference_pix_fmt"):
                run(reference=gt, reference_pix_fmt="yuv420p10le")        # an 8-bit run
            with pytest.raises(ValueError, match="reference_pix_fmt"):
                run(reference=gt, pix_fmt="p010le", reference_pix_fmt="nv12")
            with pytest.raises(ValueError, match="pix_fmt"):
                run(reference=gt, reference_pix_fmt="yuv422p")
            with pytest.raises(ValueError, match="reference_pix_fmt"):
                run(reference_pix_fmt="yuv420p")                          # without reference=
    assert os.listdir(tmp_path) == []                                     # and no destination was created
    assert R.check_crop(4, 27, 30) == 4 and R.check_crop(0, 11, 11) == 0
    with pytest.raises(ValueError):
        R.check_crop(0, 10, 30)
    with pytest.raises(ValueError):
        R.check_crop(4.0, 72, 80)


def test_the_command_line_flags():
    from fcvsr_amd.sr import main, parser
    base = ["--model", "GShiftNet_S", "--weights", "w.pth", "--size", "20x18"]
    a = parser().parse_args(base + ["in.yuv", "out.yuv"])
    assert (a.reference, a.reference_pix_fmt, a.crop_border, a.baseline, a.scores_only, a.scores_log) == (None, None, 4, None, False, None)
    a = parser().parse_args(base + ["--reference", "gt.yuv", "--reference-pix-fmt", "nv12", "--crop-border", "8", "--baseline",
                                    "bicubic", "--scores-only", "--scores-log", "s.csv", "in.yuv", "out.yuv"])
    assert (a.reference, a.reference_pix_fmt, a.crop_border, a.baseline, a.scores_only, a.scores_log) == \
        ("gt.yuv", "nv12", 8, "bicubic", True, "s.csv")
    text = parser().format_help()
    for flag in ("--reference", "--reference-pix-fmt", "--crop-border", "--baseline", "--scores-only", "--scores-log"):
        assert flag in text, flag
    for bad in (["--baseline", "lanczos"], ["--reference-pix-fmt", "yuv422p"]):
        with pytest.raises(SystemExit):
            parser().parse_args(base + bad + ["in.yuv", "out.yuv"])
    for needs in (["--scores-only"], ["--scores-log", "s.csv"], ["--baseline", "bicubic"]):
        with pytest.raises(SystemExit):                                   # they need --reference; nothing is loaded before that
            main(base + needs + ["in.yuv", "out.yuv"])


def test_the_symbol_is_declared_bound_and_exported_at_abi_version_2():
    import ctypes

    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"\bint fcvsr_plane_sse\s*\(", hdr) and re.search(r"#define FCVSR_ABI_VERSION 2\b", hdr)
    assert int(re.search(r"#define FCVSR_PLANE_SSE_SPAN_BYTES (\d+)", hdr).group(1)) == hip.PLANE_SSE_SPAN_BYTES
    assert int(re.search(r"#define FCVSR_PLANE_SSE_ROWS (\d+)", hdr).group(1)) == hip.PLANE_SSE_ROWS
    assert len(hip.SIGNATURES["fcvsr_plane_sse"]) == 13 and callable(hip.plane_sse)
    lib = ctypes.CDLL(build())
    assert hasattr(lib, "fcvsr_plane_sse") and hip.lib().fcvsr_abi_version() == 2
    fn = hip.lib().fcvsr_plane_sse                                        # argument errors come back before any device call
    assert fn(None, None, 1, 0, 4, 4, 16, 16, 0, None, 0, None, None) == 0             # P = 0: nothing to do
    for args in ((None, None, 3, 1, 4, 4, 16, 16, 0, None, 0, None, None),            # elem_size
                 (None, None, 1, 65536, 4, 4, 16, 16, 0, None, 0, None, None),        # too many planes
                 (None, None, 1, 1, 0, 4, 16, 16, 0, None, 0, None, None),            # h < 1
                 (None, None, 1, 1, 4, 4, 16, 16, 2, None, 0, None, None),            # 2 crop >= min(h, w)
                 (None, None, 1, 1, 4, 4, -1, 16, 0, None, 0, None, None),            # a negative stride
                 (None, None, 1, 1, 4, 4, 16, 16, 0, None, 0, None, None)):           # null pointers
        assert fn(*args) == -1, args
