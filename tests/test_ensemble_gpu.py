"""GPU, end to end: the x8 / x16 self-ensemble (`harness.ensemble.SelfEnsemble`, the ``ensemble=`` keyword of the sequence and
YUV harnesses) equals its restatement with torch operators around the same model - eight (sixteen) forwards on flipped /
transposed / padded windows, cropped, restored and summed in the fixed order.  No tolerances: the transforms are exact data
movement, the sum order is fixed, and the forward is batch-invariant (tests/test_configs_gpu.py pins that)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(ctor_name="GShiftNet_S", precision="bf16"):
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    from helpers import get_ctor
    m = get_ctor(ctor_name)()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes(ctor_name), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = precision
    return m


def _variant(a, i):
    a = a.flip(-1) if i & 1 else a
    a = a.flip(-2) if i & 2 else a
    return (a.transpose(-1, -2) if i & 4 else a).contiguous()


def _restore(a, i):
    a = a.transpose(-1, -2) if i & 4 else a
    a = a.flip(-2) if i & 2 else a
    return (a.flip(-1) if i & 1 else a).contiguous()


def _mean8(m, win):
    """win: f32 (B,7,C,h,w) on the device, any h, w.  One forward per variant, padded at its own bottom / right."""
    acc = None
    with torch.no_grad():
        for i in range(8):
            v = _variant(win, i)
            vh, vw = v.shape[-2:]
            o = m(F.pad(v, (0, (-vw) % 4, 0, (-vh) % 4)))[..., :4 * vh, :4 * vw]
            o = _restore(o, i)
            acc = o if acc is None else acc + o
    return acc * 0.125


def _restate(m, win, temporal=False):
    out = _mean8(m, win)
    return (out + _mean8(m, win.flip(1))) * 0.5 if temporal else out


def _window(B, C, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).rand(B, 7, C, H, W).astype(np.float32)).cuda()


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("ctor,precision,B,C", [("GShiftNet_S", "bf16", 2, 1), ("GShiftNet_S", "f32", 2, 1), ("FCVSR_SNet", "bf16", 1, 3)])
def test_self_ensemble_equals_the_torch_restatement(ctor, precision, B, C, temporal):
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    m = _model(ctor, precision)
    win = _window(B, C, 16, 20, seed=3)
    got = SelfEnsemble(m, temporal=temporal)(win)
    ref = _restate(m, win, temporal)
    assert got.shape == (B, C, 64, 80) and got.dtype == torch.float32
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.numel()} values differ (max {float((got - ref).abs().max()):.3e})"
    with torch.no_grad():
        plain = m(win)
    assert not torch.equal(got, plain)                               # not a no-op
    if temporal:
        assert not torch.equal(got, _restate(m, win, False))


def test_self_ensemble_runs_without_autograd_and_takes_integer_windows():
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    from fcvsr_amd.harness.infer import _quantised
    m = _model()
    ens = SelfEnsemble(m)
    x8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (1, 7, 1, 14, 18)).astype(np.uint8))   # padded inside
    with torch.enable_grad():                                        # the training graph must not run
        ref = ens((x8.float() / 255).cuda())
    assert not ref.requires_grad and ref.shape == (1, 1, 56, 72)
    assert torch.equal(ens(x8.cuda()), ref)                          # uint8 samples enter as the floats of the table
    assert torch.equal(ref, _restate(m, (x8.float() / 255).cuda()))
    for mode in ("truncate", "round"):
        got = ens.super_resolve_u8(x8.cuda(), mode)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), _quantised(ref, mode))
    x16 = (x8.to(torch.int16) * 4 + 1).view(torch.uint16)
    ref16 = ens((x16.view(torch.int16).float() / 1023).cuda())
    got16 = ens.super_resolve_u16(x16.view(torch.int16).cuda().view(torch.uint16), "round")
    assert got16.dtype == torch.uint16
    assert np.array_equal(got16.view(torch.int16).cpu().numpy().view(np.uint16), _quantised(ref16, "round", 1023.0))
    with pytest.raises(ValueError, match="uint8"):
        ens.super_resolve_u8(x8.float().cuda())
    with pytest.raises(ValueError, match="quantise"):
        ens.super_resolve_u8(x8.cuda(), "nearest")


def test_use_graph_equals_eager():
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    m = _model()
    win = _window(2, 1, 16, 20, seed=5)
    eager = SelfEnsemble(m)(win)
    m.use_graph = True
    try:
        first = SelfEnsemble(m)(win)                                 # captures 8 x 16 x 20 and 8 x 20 x 16
        replay = SelfEnsemble(m)(win)
    finally:
        m.use_graph = False
        m.invalidate()
    assert torch.equal(first, eager) and torch.equal(replay, eager)


def _seq8(N, C, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, C, H, W)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _sequence_reference(quantise):
    """The hand restatement for the (6,1,18,20) sequence: every frame's window through the float model with the padding rule."""
    from fcvsr_amd.harness.infer import _quantised
    from fcvsr_amd.harness.windows import window_indices
    lr = (_seq8(6, 1, 18, 20, seed=1).float() / 255).cuda()
    win = torch.stack([lr[window_indices(i, 7, 6, "replicate")] for i in range(6)], 0)
    return _quantised(_restate(_model(), win), quantise)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_super_resolve_sequence_with_ensemble(quantise):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    m = _model()
    lr8 = _seq8(6, 1, 18, 20, seed=1)                               # 18 rows: every variant pads its own bottom / right
    got = super_resolve_sequence(m, lr8, batch=4, quantise=quantise, ensemble="spatial")
    flt = super_resolve_sequence(m, lr8.float() / 255, batch=4, quantise=quantise, ensemble="spatial")
    assert got.dtype == np.uint8 and got.shape == (6, 1, 72, 80)
    assert np.array_equal(got, flt)
    ref = _sequence_reference(quantise)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} bytes differ from the hand restatement"
    assert not np.array_equal(got, super_resolve_sequence(m, lr8, batch=4, quantise=quantise))
    sub = super_resolve_sequence(m, lr8.cuda(), batch=2, centres=[5, 0, 3], quantise=quantise, ensemble="spatial")
    assert np.array_equal(sub, ref[[5, 0, 3]])


def test_super_resolve_sequence_spatial_temporal():
    from fcvsr_amd.harness.infer import _quantised, super_resolve_sequence
    from fcvsr_amd.harness.windows import window_indices
    m = _model()
    lr8 = _seq8(6, 1, 18, 20, seed=1)
    got = super_resolve_sequence(m, lr8, batch=4, centres=[0, 4], ensemble="spatial+temporal")
    lr = (lr8.float() / 255).cuda()
    win = torch.stack([lr[window_indices(i, 7, 6, "replicate")] for i in (0, 4)], 0)
    assert np.array_equal(got, _quantised(_restate(m, win, temporal=True), "truncate"))


def test_evaluate_sequence_with_ensemble_scores_the_merged_frames():
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    m = _model()
    lr8 = _seq8(6, 1, 18, 20, seed=1)
    hr = _seq8(6, 1, 72, 80, seed=6)
    for lr in (lr8, lr8.float() / 255):
        res = evaluate_sequence(m, lr, hr, batch=4, ensemble="spatial", return_frames=True)
        frames = super_resolve_sequence(m, lr, batch=4, ensemble="spatial")
        assert np.array_equal(res.frames, frames)
        p, s = frame_metrics(torch.from_numpy(frames).cuda(), hr.cuda(), quantise=None)
        assert np.array_equal(res.psnr, p.cpu().numpy()) and np.array_equal(res.ssim, s.cpu().numpy())
        assert res.psnr_mean == float(np.mean(res.psnr)) and res.ssim_mean == float(np.mean(res.ssim))
    assert np.array_equal(frames, _sequence_reference("truncate"))


def test_evaluate_sequence_with_ensemble_10_bit():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import _quantised, evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.windows import window_indices
    m = _model()
    rs = np.random.RandomState(7)
    lr = rs.randint(0, 1024, (4, 1, 18, 20))
    lr[0, 0, 0, :4] = (2000, 1024, 65535, 1023)                     # out-of-range containers read as 1023
    lr16 = torch.from_numpy(lr.astype(np.uint16).view(np.int16)).view(torch.uint16)
    hr16 = torch.from_numpy(rs.randint(0, 1024, (4, 1, 72, 80)).astype(np.uint16).view(np.int16)).view(torch.uint16)
    res = evaluate_sequence(m, lr16, hr16, batch=4, quantise="round", ensemble="spatial", return_frames=True)
    frames = super_resolve_sequence(m, lr16, batch=4, quantise="round", ensemble="spatial")
    assert res.frames.dtype == np.uint16 and np.array_equal(res.frames, frames) and int(frames.max()) <= 1023
    lrf = (torch.from_numpy(np.minimum(lr, 1023)).float() / 1023).cuda()
    win = torch.stack([lrf[window_indices(i, 7, 4, "replicate")] for i in range(4)], 0)
    assert np.array_equal(frames, _quantised(_restate(m, win), "round", 1023.0))
    sr = torch.from_numpy(frames.view(np.int16)).cuda().view(torch.uint16)
    p, s = frame_metrics(sr, hip.bits16(hr16).cuda().view(torch.uint16), quantise=None)
    assert np.array_equal(res.psnr, p.cpu().numpy()) and np.array_equal(res.ssim, s.cpu().numpy())


def test_super_resolve_yuv420_with_ensemble(tmp_path):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import read_yuv420, super_resolve_yuv420, write_yuv420
    m = _model()
    N, H, W = 5, 18, 20
    rs = np.random.RandomState(8)
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
    src, dst, plain = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "ens.yuv", "plain.yuv"))
    write_yuv420(src, y, u, v)
    stats = super_resolve_yuv420(m, src, dst, W, H, batch=3, ensemble="spatial")
    super_resolve_yuv420(m, src, plain, W, H, batch=3)
    assert stats["frames"] == N and stats["out_size"] == (4 * W, 4 * H)
    oy, ou, ov = read_yuv420(dst, 4 * W, 4 * H)
    py, pu, pv = read_yuv420(plain, 4 * W, 4 * H)
    assert np.array_equal(oy, super_resolve_sequence(m, torch.from_numpy(y)[:, None], batch=3, ensemble="spatial")[:, 0])
    assert np.array_equal(ou, pu) and np.array_equal(ov, pv)        # chroma does not go through the ensemble
    assert not np.array_equal(oy, py)


def test_super_resolve_yuv420_rgb_with_ensemble(tmp_path):
    from fcvsr_amd.harness.colour import ColourSpec, rgb_to_yuv420_host, yuv420_to_rgb_host
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    m = _model("FCVSR_SNet", "bf16")
    spec = ColourSpec()
    N, H, W = 5, 18, 20
    rs = np.random.RandomState(9)
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
    src, dst = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv"), str(tmp_path / "out.yuv")
    write_yuv420(src, y, u, v)
    super_resolve_yuv420_rgb(m, src, dst, W, H, colour=spec, batch=3, ensemble="spatial")
    rgb = torch.from_numpy(yuv420_to_rgb_host(y, u, v, spec))
    sr = super_resolve_sequence(m, rgb, batch=3, ensemble="spatial")
    sy, su, sv = rgb_to_yuv420_host(sr, spec)
    ref = np.concatenate([p[i].ravel() for i in range(N) for p in (sy, su, sv)])
    got = np.fromfile(dst, dtype=np.uint8)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} samples differ"
    assert np.unique(got).size > 32
