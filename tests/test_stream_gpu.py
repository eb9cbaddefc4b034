"""GPU: `harness.stream.stream_yuv420` writes the bytes of the whole-file functions, from a pipe into a buffer, for every keyword, with
a frame ring that does not grow with the stream."""
import io
import os
import threading

import numpy as np
import pytest
import torch

from fcvsr_amd.harness import surfaces as sf

pytestmark = pytest.mark.gpu

H, W, N, BATCH = 18, 20, 23, 2                     # 18 rows are padded to 20; the ring of 2 * 2 + 12 = 16 slots wraps
SHARED = ("frames", "out_size", "cuts", "niqe", "niqe_mean", "brisque", "brisque_mean", "bytes_written")
_models, _refs = {}, {}


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


def _frames(bits, n=N, h=H, w=W, two_shots=False):
    """n I420 frames as bytes: smooth motion plus noise; 10-bit words reach above 1023 (they pass through, the kernels read
    min(k, 1023)); two_shots: the frames from n // 2 + 1 on lie at another mean level."""
    rs = np.random.RandomState(bits + n)
    peak = 255 if bits == 8 else 1023
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        level = 0.65 if two_shots and i > n // 2 else 0.25
        y = peak * (level + 0.15 * np.sin((xx + 2 * i) / 3.0) * np.cos(yy / 4.0)) + rs.randint(0, 6, (h, w))
        if bits == 10 and i % 5 == 0:
            y[0, :3] = 1400
        c = peak * 0.5 + rs.randint(-20, 20, (2, h // 2, w // 2))
        out += [np.clip(y, 0, 1535 if bits == 10 else 255).reshape(-1), c.reshape(-1)]
    return np.concatenate(out).astype(np.uint8 if bits == 8 else "<u2").view(np.uint8).tobytes()


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
            except BrokenPipeError:                                       # the reader stopped early (max_frames) and closed
                pass
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def close(self):
        rest = self.fh.read()                                             # drain, so that the feeder ends
        self.fh.close()
        self.thread.join()
        return rest


def _stream(data, fmt="yuv420p", model="GShiftNet_S", w=W, h=H, **kw):
    from fcvsr_amd.harness.stream import stream_yuv420
    pipe, out = _Pipe(data), io.BytesIO()
    try:
        stats = stream_yuv420(_model(model), pipe.fh, out, w, h, pix_fmt=fmt, batch=kw.pop("batch", BATCH), **kw)
    finally:
        pipe.close()
    return out.getvalue(), stats


def _whole(tmp_path_factory, bits, n=N, model="GShiftNet_S", w=W, h=H, two_shots=False, **kw):
    """(source bytes, output bytes, stats) of the whole-file function, computed once per case."""
    key = (bits, n, model, w, h, two_shots, repr(sorted(kw.items(), key=lambda t: t[0])))
    if key not in _refs:
        from fcvsr_amd.harness.colour import ColourSpec
        from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
        d = tmp_path_factory.mktemp("whole")
        src, dst = str(d / "in.yuv"), str(d / "out.yuv")
        data = _frames(bits, n, h, w, two_shots)
        with open(src, "wb") as f:
            f.write(data)
        if model == "GShiftNet_S":
            stats = super_resolve_yuv420(_model(model), src, dst, w, h, bit_depth=bits, batch=kw.pop("batch", BATCH), **kw)
        else:
            stats = super_resolve_yuv420_rgb(_model(model), src, dst, w, h, colour=ColourSpec(bit_depth=bits),
                                             batch=kw.pop("batch", BATCH), **kw)
        with open(dst, "rb") as f:
            _refs[key] = (data, f.read(), stats)
    return _refs[key]


def _same_stats(got, want):
    for k in SHARED:
        assert (k in got) == (k in want), k
        if k in want:
            a, b = got[k], want[k]
            assert np.array_equal(np.asarray(a), np.asarray(b)) and type(a) == type(b), (k, a, b)


def _fmt(bits):
    return "yuv420p" if bits == 8 else "yuv420p10le"


@pytest.mark.parametrize("bits,kw", [
    (8, {}), (10, {}), (8, {"padding": "reflection_circle"}), (10, {"quantise": "round"}), (8, {"ensemble": "spatial"}),
    (10, {"tile": (16, 16), "tile_overlap": 4}), (8, {"cuts": [9]}), (10, {"cuts": "auto"}), (8, {"output_shape": (54, 60)})],
    ids=lambda v: v if isinstance(v, int) else "-".join(v) or "plain")
def test_the_bytes_of_the_whole_file_path(bits, kw, tmp_path_factory):
    two_shots = kw.get("cuts") == "auto"
    data, want, ref = _whole(tmp_path_factory, bits, two_shots=two_shots, **kw)
    got, stats = _stream(data, _fmt(bits), **kw)
    assert len(got) == len(want) and got == want
    _same_stats(stats, ref)
    if two_shots:
        assert stats["cuts"] == [N // 2 + 1]
    assert stats["ring_frames"] <= 2 * BATCH + 12 and stats["frames_uploaded"] == stats["frames"] == N
    assert stats["h2d_bytes"] == len(data) and stats["d2h_bytes"] == len(want) and stats["seconds"] > 0 and stats["fps"] > 0


@pytest.mark.parametrize("fmt", ["nv12", "p010le"])
def test_semi_planar_in_and_out(fmt, tmp_path_factory):
    bits = sf.bit_depth(fmt)
    data, want, ref = _whole(tmp_path_factory, bits)
    if bits == 10:                                                        # P010 holds ten bits: the source of this case stays below 1024
        y, u, v = sf.unpack_host(data, _fmt(bits), W, H)
        data = sf.pack_host(*(np.minimum(a, 1023) for a in (y, u, v)), _fmt(bits))
    src = sf.pack_host(*sf.unpack_host(data, _fmt(bits), W, H), fmt)
    assert sf.unpack_host(src, fmt, W, H)[0].tolist() == sf.unpack_host(data, _fmt(bits), W, H)[0].tolist()
    got, stats = _stream(src, fmt)
    assert got == sf.pack_host(*sf.unpack_host(want, _fmt(bits), 4 * W, 4 * H), fmt)
    _same_stats(stats, ref)
    if fmt == "nv12":
        planar, _ = _stream(src, fmt, out_pix_fmt="yuv420p")
        assert planar == want


def test_mixing_bit_depths_and_unknown_formats_raise():
    from fcvsr_amd.harness.stream import stream_yuv420
    for kw in ({"pix_fmt": "nv12", "out_pix_fmt": "p010le"}, {"pix_fmt": "yuv420p10le", "out_pix_fmt": "yuv420p"},
               {"pix_fmt": "yuv422p"}, {"out_pix_fmt": "nv21"}):
        with pytest.raises(ValueError):
            stream_yuv420(_model(), io.BytesIO(b""), io.BytesIO(), W, H, **kw)
    with pytest.raises(ValueError):
        stream_yuv420(_model(), io.BytesIO(b""), io.BytesIO(), W, H)      # an empty stream


def test_the_rgb_twin(tmp_path_factory):
    from fcvsr_amd.harness.colour import ColourSpec
    data, want, ref = _whole(tmp_path_factory, 8, n=9, model="FCVSR_SNet")
    got, stats = _stream(data, "yuv420p", model="FCVSR_SNet", colour=ColourSpec())
    assert got == want
    _same_stats(stats, ref)
    src = sf.pack_host(*sf.unpack_host(data, "yuv420p", W, H), "nv12")
    got, _ = _stream(src, "nv12", model="FCVSR_SNet")
    assert got == sf.pack_host(*sf.unpack_host(want, "yuv420p", 4 * W, 4 * H), "nv12")


def test_the_ring_does_not_grow_with_the_stream(tmp_path_factory):
    data, want, _ = _whole(tmp_path_factory, 8, n=9)
    got, short = _stream(data)
    assert got == want and short["frames_uploaded"] == short["frames"] == 9
    _, long = _stream(_whole(tmp_path_factory, 8)[0])
    assert short["ring_frames"] == long["ring_frames"] <= 2 * BATCH + 12


def test_max_frames_leaves_the_rest_unread(tmp_path_factory):
    from fcvsr_amd.harness.stream import stream_yuv420
    data, want, _ = _whole(tmp_path_factory, 8, n=5)
    longer = data + _frames(8, 9)
    pipe, out = _Pipe(longer), io.BytesIO()
    try:
        stats = stream_yuv420(_model(), pipe.fh, out, W, H, batch=BATCH, max_frames=5)
    finally:
        rest = pipe.close()
    assert out.getvalue() == want and stats["frames"] == 5
    assert len(rest) > 0 and longer.endswith(rest)                        # bytes of the later frames were still in the pipe


def test_stray_bytes_are_reported_after_the_frames_are_written(tmp_path_factory):
    from fcvsr_amd.harness.stream import stream_yuv420
    data, want, _ = _whole(tmp_path_factory, 8, n=5)
    pipe, out = _Pipe(data + b"\x01" * 7), io.BytesIO()
    try:
        with pytest.raises(ValueError, match="7 stray bytes"):
            stream_yuv420(_model(), pipe.fh, out, W, H, batch=BATCH)
    finally:
        pipe.close()
    assert out.getvalue() == want


def test_a_cut_beyond_the_end_raises_after_the_frames_are_written(tmp_path_factory):
    from fcvsr_amd.harness.stream import stream_yuv420
    data, want, _ = _whole(tmp_path_factory, 8, n=5)
    out = io.BytesIO()
    with pytest.raises(ValueError):
        stream_yuv420(_model(), io.BytesIO(data), out, W, H, batch=BATCH, cuts=[5])
    assert out.getvalue() == want


def test_niqe_scores_equal_the_whole_file_ones(tmp_path_factory, golden_dir):
    from fcvsr_amd.harness.niqe import NiqeModel
    from fcvsr_amd.harness.yuv import _check_niqe
    niqe = NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    h, w = 24, 48                                                         # 96 x 192 SR frames: two blocks, the fewest NIQE takes
    _check_niqe(niqe, 8, w, h)
    for smaller in ((h - 2, w), (h, w - 2)):
        with pytest.raises(ValueError):
            _check_niqe(niqe, 8, smaller[1], smaller[0])
    data, want, ref = _whole(tmp_path_factory, 8, n=3, w=w, h=h, niqe=niqe)
    got, stats = _stream(data, w=w, h=h, niqe=niqe)
    assert got == want and stats["niqe"].shape == (3,)
    _same_stats(stats, ref)
