"""GPU: ``reference=`` on the three file functions: the bytes written do not change, the scores are those of the bytes written
(checked on the host from the output file), the streamed run gives the whole-file run's numbers bit for bit, and the ground-truth
reader stops where it should.  The synthetic model and the sizes of tests/test_stream_gpu.py: 23 frames of 20x18, batch 2."""
import io
import os
import threading

import numpy as np
import pytest
import torch

from fcvsr_amd.harness import metrics
from fcvsr_amd.harness import reference as R
from fcvsr_amd.harness import surfaces as sf

pytestmark = pytest.mark.gpu

H, W, N, BATCH = 18, 20, 23, 2
TOL = 1e-9                                                                # tests/test_quality_gpu.py: device SSIM against metrics.ssim
SCORE_KEYS = ("sse", "psnr_", "ssim_", "reference_frames", "baseline_")    # what reference= / baseline= add to the stats
GLOBAL = ("psnr_y_global", "psnr_u_global", "psnr_v_global", "psnr_yuv_global")
_models, _cache = {}, {}


def _model(name="GShiftNet_S"):
    """A synthetic-weight model, built once."""
    if name not in _models:
        from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
        from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
        from fcvsr_amd.arch.schema import state_dict_shapes
        from fcvsr_amd.weights import synthetic_state_dict
        m = {"GShiftNet_S": GShiftNet_S, "FCVSR_SNet": FCVSR_SNet}[name]()
        m.load_state_dict(synthetic_state_dict(state_dict_shapes(name), gain=0.5), strict=True)
        m = m.cuda()
        m.precision = "bf16"
        _models[name] = m
    return _models[name]


def _frames(bits, n=N, h=H, w=W):
    """n I420 frames as bytes: smooth motion plus noise; 10-bit words reach above 1023."""
    rs = np.random.RandomState(bits + n)
    peak = 255 if bits == 8 else 1023
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        y = peak * (0.25 + 0.15 * np.sin((xx + 2 * i) / 3.0) * np.cos(yy / 4.0)) + rs.randint(0, 6, (h, w))
        if bits == 10 and i % 5 == 0:
            y[0, :3] = 1400
        c = peak * 0.5 + rs.randint(-20, 20, (2, h // 2, w // 2))
        out += [np.clip(y, 0, 1535 if bits == 10 else 255).reshape(-1), c.reshape(-1)]
    return np.concatenate(out).astype(np.uint8 if bits == 8 else "<u2").view(np.uint8).tobytes()


def _fmt(bits):
    return "yuv420p" if bits == 8 else "yuv420p10le"


def _noisy(out: bytes, bits, wo, ho, seed=1):
    """Ground-truth bytes (planar, `bits`) made from a run's own output: plus seeded integer noise, clipped to the peak; frame 1
    keeps its chroma planes (PSNR inf there)."""
    rs = np.random.RandomState(seed)
    peak = 255 if bits == 8 else 1023
    planes = [a.astype(np.int64) for a in sf.unpack_host(out, _fmt(bits), wo, ho)]
    noisy = [np.clip(a + rs.randint(-6, 7, a.shape), 0, peak) for a in planes]
    noisy[1][1], noisy[2][1] = planes[1][1], planes[2][1]
    return sf.pack_host(*(a.astype(np.uint8 if bits == 8 else np.uint16) for a in noisy), _fmt(bits))


class _Pipe:
    """The read end of an os.pipe() fed by a thread in pieces that do not align with frames."""

    def __init__(self, data: bytes, piece: int = 997):
        r, w = os.pipe()
        self.fh = os.fdopen(r, "rb", buffering=0)

        def feed():
            try:
                with os.fdopen(w, "wb", buffering=0) as out:
                    for s in range(0, len(data), piece):
                        out.write(data[s:s + piece])
            except BrokenPipeError:                                       # the reader stopped early and closed
                pass
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def close(self):
        rest = self.fh.read()                                             # drain, so that the feeder ends
        self.fh.close()
        self.thread.join()
        return rest


def _whole(tmp_path_factory, data, bits, model="GShiftNet_S", gt=None, write=True, **kw):
    """(output bytes or None, stats) of the whole-file function on the source bytes `data`, with `gt` bytes as ``reference=``."""
    from fcvsr_amd.harness.colour import ColourSpec
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    d = tmp_path_factory.mktemp("ref")
    src, dst, ref = str(d / "in.yuv"), str(d / "out.yuv") if write else None, None
    with open(src, "wb") as f:
        f.write(data)
    if gt is not None:
        ref = str(d / "gt.yuv")
        with open(ref, "wb") as f:
            f.write(gt)
        kw["reference"] = ref
    if model == "GShiftNet_S":
        stats = super_resolve_yuv420(_model(model), src, dst, W, H, bit_depth=bits, batch=BATCH, **kw)
    else:
        stats = super_resolve_yuv420_rgb(_model(model), src, dst, W, H, colour=ColourSpec(bit_depth=bits), batch=BATCH, **kw)
    if not write:
        assert sorted(os.listdir(d)) == (["in.yuv"] if gt is None else ["gt.yuv", "in.yuv"])
        return None, stats
    with open(dst, "rb") as f:
        return f.read(), stats


def _stream(data, bits, model="GShiftNet_S", gt=None, write=True, fmt=None, **kw):
    """(output bytes, stats, unread ground-truth bytes) of `stream_yuv420`, source and ground truth through pipes."""
    from fcvsr_amd.harness.colour import ColourSpec
    from fcvsr_amd.harness.stream import stream_yuv420
    pipe, out = _Pipe(data), io.BytesIO()
    gpipe = None if gt is None else _Pipe(gt, 1409)
    rest = None
    try:
        stats = stream_yuv420(_model(model), pipe.fh, out if write else None, W, H, pix_fmt=fmt or _fmt(bits), batch=BATCH,
                              colour=ColourSpec(bit_depth=bits), reference=None if gt is None else gpipe.fh, **kw)
    finally:
        pipe.close()
        if gpipe is not None:
            rest = gpipe.close()
    return out.getvalue(), stats, rest


def _case(tmp_path_factory, bits, model, n=N):
    """Per case, computed once: the source, the plain run, a noisy ground truth of it and the whole-file run scored against that."""
    key = (bits, model, n)
    if key not in _cache:
        data = _frames(bits, n)
        plain, pstats = _whole(tmp_path_factory, data, bits, model)
        gt = _noisy(plain, bits, 4 * W, 4 * H, seed=bits + n)
        out, stats = _whole(tmp_path_factory, data, bits, model, gt=gt)
        _cache[key] = (data, plain, pstats, gt, out, stats)
    return _cache[key]


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def _host_scores(out: bytes, gt: bytes, bits, wo, ho, crop=4, out_fmt=None, gt_fmt=None):
    """What the stats must hold, from the bytes alone: sums and PSNR on the host, SSIM by `frame_metrics` on the same planes."""
    from fcvsr_amd.harness.device_metrics import frame_metrics
    peak = R.PEAKS[bits]
    a, b = sf.unpack_host(out, out_fmt or _fmt(bits), wo, ho), sf.unpack_host(gt, gt_fmt or _fmt(bits), wo, ho)
    b = tuple(np.minimum(p, 1023) if bits == 10 else p for p in b)
    assert all(int(p.max()) <= peak for p in a)                           # what is written never exceeds the peak
    crops = (crop, crop // 2, crop // 2)
    sse = np.stack([R.plane_sse_host(p, q, c) for p, q, c in zip(a, b, crops)], 1)
    psnr = [np.array([metrics.psnr(p[n], q[n], c, peak) for n in range(p.shape[0])]) for p, q, c in zip(a, b, crops)]
    ssim = frame_metrics(_dev(a[0])[:, None], _dev(b[0])[:, None], crop_border=crop, quantise=None)[1].cpu().numpy()
    for n in (0, a[0].shape[0] - 1):                                      # and the device SSIM is the host's, as the metric tests pin it
        assert abs(ssim[n] - metrics.ssim(a[0][n], b[0][n], crop, peak=float(peak))) <= TOL
    return {"sse": sse, "psnr_y": psnr[0], "psnr_u": psnr[1], "psnr_v": psnr[2], "ssim_y": ssim}


def _same_scores(got, want):
    """Bit-equal stats of two runs: every key of ``reference=`` and of ``baseline=``."""
    mine = lambda d: sorted(k for k in d if k.startswith(SCORE_KEYS))
    assert mine(got) == mine(want) and len(mine(want)) >= 16, (mine(got), mine(want))
    for k in mine(want):
        a, b = got[k], want[k]
        assert type(a) == type(b) and np.array_equal(np.asarray(a), np.asarray(b)), (k, a, b)


CASES = [(8, "GShiftNet_S", N), (10, "GShiftNet_S", N), (8, "FCVSR_SNet", 9)]
IDS = ["y8", "y10", "rgb8"]


@pytest.mark.parametrize("bits,model,n", CASES, ids=IDS)
def test_the_bytes_do_not_change_and_the_scores_are_those_of_the_bytes(bits, model, n, tmp_path_factory):
    data, plain, pstats, gt, out, stats = _case(tmp_path_factory, bits, model, n)
    assert out == plain and len(out) == n * sf.frame_bytes(_fmt(bits), 4 * W, 4 * H)
    for k in pstats:                                                      # nothing of the plain stats moved, and nothing new without the keyword
        if k not in ("seconds", "fps"):
            assert np.array_equal(np.asarray(stats[k]), np.asarray(pstats[k])), k
    assert not any(k in pstats for k in ("sse", "psnr_y", "ssim_y", "reference_frames", "baseline_psnr_y"))
    want = _host_scores(out, gt, bits, 4 * W, 4 * H)
    assert stats["reference_frames"] == n and stats["sse"].dtype == np.int64 and stats["sse"].shape == (n, 3)
    assert stats["sse"].tolist() == want["sse"].tolist() and int(stats["sse"][:, 0].min()) > 0
    assert stats["sse"][1].tolist()[1:] == [0, 0] and np.isinf(stats["psnr_u"][1]) and np.isinf(stats["psnr_v"][1])
    for k in ("psnr_y", "psnr_u", "psnr_v", "ssim_y"):
        assert stats[k].dtype == np.float64 and stats[k].shape == (n,)
        assert np.array_equal(stats[k], want[k]), (k, stats[k], want[k])
        assert stats[k + "_mean"] == float(np.mean(want[k]))
    full = R.sequence_scores(want["sse"], want["ssim_y"], R.plane_sizes(4 * H, 4 * W, 4), R.PEAKS[bits])
    for k in ("psnr_yuv", "psnr_yuv_mean") + GLOBAL:
        assert np.array_equal(np.asarray(stats[k]), np.asarray(full[k])), k


@pytest.mark.parametrize("bits,model,n", CASES, ids=IDS)
def test_the_stream_gives_the_whole_file_scores_bit_for_bit(bits, model, n, tmp_path_factory):
    data, plain, _, gt, _, ref = _case(tmp_path_factory, bits, model, n)
    if bits == 8:
        out, stats, rest = _stream(data, bits, model, gt=gt)
        assert out == plain
    else:                                                                 # p010le out, scored against the planar 10-bit ground truth
        out, stats, rest = _stream(data, bits, model, gt=gt, out_pix_fmt="p010le", reference_pix_fmt="yuv420p10le")
        assert out == sf.pack_host(*sf.unpack_host(plain, _fmt(bits), 4 * W, 4 * H), "p010le")
    assert rest == b""
    _same_scores(stats, ref)
    assert stats["frames"] == n and stats["bytes_written"] == len(out) and stats["ring_frames"] <= 2 * BATCH + 12
    assert stats["h2d_bytes"] == len(data) + len(gt) and stats["d2h_bytes"] == len(out)


def test_semi_planar_ground_truth_and_a_longer_one_left_unread(tmp_path_factory):
    data, plain, _, gt, _, ref = _case(tmp_path_factory, 8, "GShiftNet_S", N)
    nv12 = sf.pack_host(*sf.unpack_host(gt, "yuv420p", 4 * W, 4 * H), "nv12")
    extra = nv12[:2 * sf.frame_bytes("nv12", 4 * W, 4 * H)]
    out, stats, rest = _stream(data, 8, gt=nv12 + extra, reference_pix_fmt="nv12")
    assert out == plain and rest == extra                                 # not a byte beyond the last frame needed was read
    _same_scores(stats, ref)


def test_ground_truth_equal_to_the_output(tmp_path_factory):
    """The sums are 0 and every PSNR is inf, exactly.  SSIM is 1 as `metrics.ssim` of a plane with itself is: the existing
    `frame_metrics` kernel gives 0.9999999999999999 for equal planes (its f64 map sum over the count), so this one comparison is
    with the host function, at the tolerance the device-metrics tests use for it."""
    data = _frames(8, 5)
    plain, _ = _whole(tmp_path_factory, data, 8)
    luma = sf.unpack_host(plain, "yuv420p", 4 * W, 4 * H)[0]
    want = np.array([metrics.ssim(p, p, 4) for p in luma])
    assert np.abs(want - 1.0).max() <= TOL
    for stats in (_whole(tmp_path_factory, data, 8, gt=plain)[1], _stream(data, 8, gt=plain)[1]):
        assert stats["sse"].tolist() == [[0, 0, 0]] * 5
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv"):
            assert np.isinf(stats[k]).all() and stats[k + "_mean"] == float("inf") and stats[k + "_global"] == float("inf")
        assert np.abs(stats["ssim_y"] - want).max() <= TOL and abs(stats["ssim_y_mean"] - 1.0) <= TOL, stats["ssim_y"]


@pytest.mark.parametrize("kw", [{"output_shape": (54, 60)}, {"ensemble": "spatial"}, {"tile": (16, 16), "tile_overlap": 4, "static_tiles": True},
                                {"active": (2, 16, 4, 20)}], ids=["output_shape", "ensemble", "static_tiles", "active"])
def test_the_scores_are_those_of_the_delivered_bytes(kw, tmp_path_factory):
    n = 5
    data = _frames(8, n)
    ho, wo = kw.get("output_shape", (4 * H, 4 * W))
    plain, _ = _whole(tmp_path_factory, data, 8, **dict(kw))
    gt = _noisy(plain, 8, wo, ho, seed=len(kw))
    out, stats = _whole(tmp_path_factory, data, 8, gt=gt, **dict(kw))
    assert out == plain and stats["out_size"] == (wo, ho)
    want = _host_scores(out, gt, 8, wo, ho)
    assert stats["sse"].tolist() == want["sse"].tolist() and stats["reference_frames"] == n
    for k in ("psnr_y", "psnr_u", "psnr_v", "ssim_y"):
        assert np.array_equal(stats[k], want[k]), (k, stats[k], want[k])
    sout, sstats, rest = _stream(data, 8, gt=gt, **dict(kw))
    assert sout == plain and rest == b""
    _same_scores(sstats, stats)
    if "static_tiles" in kw:
        assert stats["tiles_total"] > 0


def _baseline_want(data, gt, bits, shape, model):
    """`frame_metrics` of the contract up-scale of the LR centre frames against the ground-truth luma."""
    from fcvsr_amd.harness.colour import ColourSpec, i420_planes, rgb_to_i420, yuv420_to_rgb
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.resize import bicubic_upscale, imresize
    ho, wo = shape or (4 * H, 4 * W)
    y, u, v = (_dev(a) for a in sf.unpack_host(data, _fmt(bits), W, H))
    if model == "GShiftNet_S":
        up = (bicubic_upscale(y[:, None], 4, out="int") if shape is None else imresize(y[:, None], output_shape=shape, out="int"))[:, 0]
    else:
        spec = ColourSpec(bit_depth=bits)
        up = i420_planes(rgb_to_i420(imresize(yuv420_to_rgb(y, u, v, spec), output_shape=(ho, wo), out="int"), spec), ho, wo)[0]
    g = _dev(sf.unpack_host(gt, _fmt(bits), wo, ho)[0])
    p, s = frame_metrics(up[:, None], g[:, None], crop_border=4, quantise=None)
    return p.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("model,shape", [("GShiftNet_S", None), ("GShiftNet_S", (54, 60)), ("FCVSR_SNet", None)],
                         ids=["y", "y-output_shape", "rgb"])
def test_the_bicubic_baseline(model, shape, tmp_path_factory):
    n = 5
    data = _frames(8, n)
    kw = {} if shape is None else {"output_shape": shape}
    ho, wo = shape or (4 * H, 4 * W)
    plain, _ = _whole(tmp_path_factory, data, 8, model, **dict(kw))
    gt = _noisy(plain, 8, wo, ho, seed=3)
    without = _whole(tmp_path_factory, data, 8, model, gt=gt, **dict(kw))[1]
    if model == "GShiftNet_S":                                            # the whole-file Y function takes no baseline=: the stream does
        out, stats, _ = _stream(data, 8, model, gt=gt, baseline="bicubic", **dict(kw))
    else:
        out, stats = _whole(tmp_path_factory, data, 8, model, gt=gt, baseline="bicubic", **dict(kw))
        _same_scores(_stream(data, 8, model, gt=gt, baseline="bicubic", **dict(kw))[1], stats)
    assert out == plain and "baseline_psnr_y" not in without
    _same_scores({k: v for k, v in stats.items() if not k.startswith("baseline_")}, without)      # the other scores do not move
    p, s = _baseline_want(data, gt, 8, shape, model)
    assert np.array_equal(stats["baseline_psnr_y"], p) and np.array_equal(stats["baseline_ssim_y"], s)
    assert stats["baseline_psnr_y_mean"] == float(np.mean(p)) and stats["baseline_ssim_y_mean"] == float(np.mean(s))
    assert np.isfinite(p).all() and (s < 1).all()


def test_scores_only_writes_nothing(tmp_path_factory):
    data, plain, _, gt, _, ref = _case(tmp_path_factory, 8, "GShiftNet_S", N)
    _, stats = _whole(tmp_path_factory, data, 8, gt=gt, write=False)
    assert stats["bytes_written"] == 0 and stats["frames"] == N
    _same_scores(stats, ref)
    out, stats, rest = _stream(data, 8, gt=gt, write=False)
    assert out == b"" and rest == b"" and stats["bytes_written"] == 0 and stats["d2h_bytes"] == 0 and stats["frames"] == N
    _same_scores(stats, ref)


def test_a_short_ground_truth_raises_after_every_frame_was_written(tmp_path_factory):
    data, plain, _, gt, _, _ = _case(tmp_path_factory, 8, "GShiftNet_S", N)
    fb = sf.frame_bytes("yuv420p", 4 * W, 4 * H)
    from fcvsr_amd.harness.stream import stream_yuv420
    for short in (gt[:(N - 2) * fb], gt[:(N - 2) * fb + 11]):             # two frames short; and a broken frame after them
        pipe, gpipe, out = _Pipe(data), _Pipe(short, 1409), io.BytesIO()
        try:
            with pytest.raises(ValueError, match=rf"{N - 2} whole .*{N}"):
                stream_yuv420(_model(), pipe.fh, out, W, H, batch=BATCH, reference=gpipe.fh)
        finally:
            pipe.close()
            gpipe.close()
        assert out.getvalue() == plain                                    # all 23 frames
    with pytest.raises(ValueError, match=rf"{N - 2} whole .*{N}"):        # the whole-file function knows before it starts
        _whole(tmp_path_factory, data, 8, gt=gt[:(N - 2) * fb])


def test_max_frames_stops_both_readers(tmp_path_factory):
    data5 = _frames(8, 5)
    plain, _ = _whole(tmp_path_factory, data5, 8)
    fb = sf.frame_bytes("yuv420p", 4 * W, 4 * H)
    gt = _noisy(plain, 8, 4 * W, 4 * H, seed=9) + _case(tmp_path_factory, 8, "GShiftNet_S", N)[3][:4 * fb]      # nine frames
    _, ref = _whole(tmp_path_factory, data5, 8, gt=gt)                    # a longer file is fine: its first five frames count
    longer = data5 + _frames(8, 9)
    from fcvsr_amd.harness.stream import stream_yuv420
    pipe, gpipe, out = _Pipe(longer), _Pipe(gt, 1409), io.BytesIO()
    try:
        stats = stream_yuv420(_model(), pipe.fh, out, W, H, batch=BATCH, max_frames=5, reference=gpipe.fh)
    finally:
        rest, grest = pipe.close(), gpipe.close()
    assert out.getvalue() == plain and stats["frames"] == stats["reference_frames"] == 5
    assert len(rest) > 0 and longer.endswith(rest) and grest == gt[5 * fb:]
    _same_scores(stats, ref)
