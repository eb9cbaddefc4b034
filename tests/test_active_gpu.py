"""GPU, end to end: with `active=` the resolver sees the active box only and the rest of the 4x frame is the bicubic up-scale of the
LR centre frame (`harness.active.compose_host`), in every entry point, and the stream writes the bytes of the whole-file functions."""
import io

import numpy as np
import pytest
import torch

import active_cases as ac
from fcvsr_amd.harness import active as A
from fcvsr_amd.harness import surfaces as sf
from fcvsr_amd.harness.shots import windows_for

pytestmark = pytest.mark.gpu

SPEC = A.ActiveSpec(min_side=8)
H, W, N, BATCH = 24, 32, 12, 4
SMALL, BIG = (8, 20, 4, 28), (4, 20, 4, 28)
_models = {}


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


def _growing(bits=8, n=N):
    """Letterboxed and pillarboxed frames whose picture grows upward at frame 5."""
    return ac.barred(bits, n, 1, H, W, lambda i: SMALL if i < 5 else BIG, seed=bits)


def _torch(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def _crop(a, box):
    t, b, l, r = box
    return np.ascontiguousarray(a[:, :, t:b, l:r])


@pytest.mark.parametrize("kw", [{}, {"ensemble": "spatial"}, {"tile": (16, 16), "tile_overlap": 4}], ids=["plain", "ensemble", "tile"])
@pytest.mark.parametrize("bits,box", [(8, BIG), (10, (3, 21, 5, 27))], ids=["u8-aligned", "u16-unaligned"])
def test_an_explicit_box_is_the_cropped_call_composed(bits, box, kw):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    lr = _growing(bits, 5)
    got = super_resolve_sequence(_model(), _torch(lr), batch=BATCH, active=box, **kw)
    inner = super_resolve_sequence(_model(), _torch(_crop(lr, box)), batch=BATCH, **kw)
    assert got.dtype == lr.dtype and got.shape == (5, 1, 4 * H, 4 * W)
    assert np.array_equal(got, A.compose_host(inner, lr, box))
    assert not np.array_equal(got, super_resolve_sequence(_model(), _torch(lr), batch=BATCH, **kw))


def test_float_frames_take_an_explicit_box():
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.niqe import bicubic_upscale
    lr = (_growing(8, 4).astype(np.float32) / 255).astype(np.float32)
    got = super_resolve_sequence(_model(), torch.from_numpy(lr), batch=BATCH, active=BIG)
    inner = super_resolve_sequence(_model(), torch.from_numpy(_crop(lr, BIG)), batch=BATCH)
    want = (np.clip(bicubic_upscale(lr, 4).astype(np.float32), 0, 1) * np.float32(255)).astype(np.uint8)     # quantised as SR frames are
    t, b, l, r = BIG
    want[..., 4 * t:4 * b, 4 * l:4 * r] = inner
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        super_resolve_sequence(_model(), torch.from_numpy(lr), active="auto")


@pytest.mark.parametrize("kw", [{}, {"tile": (16, 16), "tile_overlap": 4}], ids=["plain", "tile"])
def test_the_whole_frame_box_is_active_none(kw):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    lr = _torch(ac.barred(8, 4, 1, 18, 20, (0, 18, 0, 20), seed=2))       # 18 rows are padded to 20
    assert np.array_equal(super_resolve_sequence(_model(), lr, batch=BATCH, active=(0, 18, 0, 20), **kw),
                          super_resolve_sequence(_model(), lr, batch=BATCH, **kw))


def _assembled(model, lr, bits, batch, padding="replicate", **kw):
    """`active=SPEC` by its definition: per group the runs of one box (the brute-force window rule), each run the call on the cropped
    sequence with the run's centres, composed on the host.  Returns (frames, changes)."""
    from fcvsr_amd.harness.infer import super_resolve_sequence
    n = lr.shape[0]
    out, changes = [], []
    for s in range(0, n, batch):
        centres = list(range(s, min(n, s + batch)))
        boxes = [ac.brute_box(lr, bits, max(w), SPEC) for w in windows_for(centres, 7, n, padding, None)]
        for a, e, box in A.split_runs(boxes):
            inner = super_resolve_sequence(model, _torch(_crop(lr, box)), batch=batch, centres=centres[a:e], padding=padding, **kw)
            out.append(A.compose_host(inner, lr[centres[a:e]], box))
            if not changes or changes[-1][1] != box:
                changes.append((centres[a], box))
    return np.concatenate(out, 0), changes


@pytest.mark.parametrize("bits", [8, 10])
def test_auto_follows_a_box_that_changes_inside_a_group(bits):
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    lr = _growing(bits)
    want, changes = _assembled(_model(), lr, bits, BATCH)
    assert changes == [(0, SMALL), (2, BIG)]                              # centre 2 is the first whose window names frame 5
    got = super_resolve_sequence(_model(), _torch(lr), batch=BATCH, active=SPEC)
    assert np.array_equal(got, want)
    # evaluate_sequence scores, returns and reports the composed frames
    from fcvsr_amd.harness.device_metrics import frame_metrics
    hr = np.clip(want.astype(np.int32) + np.random.RandomState(1).randint(-9, 10, want.shape), 0, 255 if bits == 8 else 1023).astype(lr.dtype)
    scores = evaluate_sequence(_model(), _torch(lr), _torch(hr), batch=BATCH, active=SPEC, return_frames=True)
    assert np.array_equal(scores.frames, want) and scores.active == changes
    p, s = frame_metrics(_torch(want).cuda(), _torch(hr).cuda(), crop_border=4, quantise=None)
    assert np.array_equal(scores.psnr, p.cpu().numpy()) and np.array_equal(scores.ssim, s.cpu().numpy())
    assert evaluate_sequence(_model(), _torch(lr), _torch(hr), batch=BATCH).active is None
    # the default min_side does not believe boxes this small: the whole frame is used
    assert np.array_equal(super_resolve_sequence(_model(), _torch(lr[:4]), batch=BATCH, active="auto"),
                          super_resolve_sequence(_model(), _torch(lr[:4]), batch=BATCH))


def _i420(bits, n=N):
    """n I420 frames as bytes: the luma of `_growing`, flat chroma with noise."""
    rs = np.random.RandomState(bits)
    y = _growing(bits, n)
    peak = 255 if bits == 8 else 1023
    out = []
    for i in range(n):
        out += [y[i].reshape(-1), (peak // 2 + rs.randint(-20, 20, (2 * (H // 2) * (W // 2),))).astype(y.dtype)]
    return y, np.concatenate(out).astype(np.uint8 if bits == 8 else "<u2").view(np.uint8).tobytes()


def _whole(tmp_path, data, bits, model, **kw):
    from fcvsr_amd.harness.colour import ColourSpec
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "out.yuv")
    with open(src, "wb") as f:
        f.write(data)
    if model == "GShiftNet_S":
        stats = super_resolve_yuv420(_model(model), src, dst, W, H, bit_depth=bits, **kw)
    else:
        stats = super_resolve_yuv420_rgb(_model(model), src, dst, W, H, colour=ColourSpec(bit_depth=bits), **kw)
    with open(dst, "rb") as f:
        return f.read(), stats


@pytest.mark.parametrize("bits,model,batch", [(8, "GShiftNet_S", 2), (10, "GShiftNet_S", 4), (8, "FCVSR_SNet", 2)],
                         ids=["y-u8", "y-u16", "rgb-u8"])
def test_the_stream_writes_the_bytes_and_boxes_of_the_whole_file_functions(bits, model, batch, tmp_path):
    from fcvsr_amd.harness.stream import stream_yuv420
    n = N if model == "GShiftNet_S" else 9
    y, data = _i420(bits, n)
    fmt = "yuv420p" if bits == 8 else "yuv420p10le"
    want, ref = _whole(tmp_path, data, bits, model, batch=batch, active=SPEC)
    assert ref["active"] == [(0, SMALL), (2, BIG)]
    plain, none = _whole(tmp_path, data, bits, model, batch=batch)
    assert "active" not in none and plain != want
    if model == "GShiftNet_S":                                            # the luma plane is the sequence function's result
        sr, _ = _assembled(_model(), y, bits, batch)
        assert np.array_equal(sf.unpack_host(want, fmt, 4 * W, 4 * H)[0], sr[:, 0])
    for pix in (fmt, "nv12" if bits == 8 else "p010le"):
        src = data if pix == fmt else sf.pack_host(*sf.unpack_host(data, fmt, W, H), pix)
        out = io.BytesIO()
        stats = stream_yuv420(_model(model), io.BytesIO(src), out, W, H, pix_fmt=pix, batch=batch, active=SPEC)
        assert stats["active"] == ref["active"] and stats["frames"] == n
        assert out.getvalue() == (want if pix == fmt else sf.pack_host(*sf.unpack_host(want, fmt, 4 * W, 4 * H), pix))
    # an explicit box through the stream
    out = io.BytesIO()
    stats = stream_yuv420(_model(model), io.BytesIO(data), out, W, H, pix_fmt=fmt, batch=batch, active=BIG)
    assert stats["active"] == [(0, BIG)] and out.getvalue() == _whole(tmp_path, data, bits, model, batch=batch, active=BIG)[0]
