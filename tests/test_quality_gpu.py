"""GPU: on-device PSNR / SSIM (fcvsr_frame_metrics, harness.device_metrics.frame_metrics) against the CPU functions of
harness/metrics.py, the sequence scorer harness.infer.evaluate_sequence, and validation inside train.step.fit."""
import re

import numpy as np
import pytest
import torch

from fcvsr_amd.harness.metrics import psnr, ssim, to_y_channel

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _structured(rs, N, C, H, W, noise=6):
    """uint8 HR = smooth pattern + noise, SR = HR +- small noise: SSIM far from 0."""
    yy, xx = np.mgrid[:H, :W]
    hr = np.empty((N, C, H, W), dtype=np.uint8)
    for n in range(N):
        for c in range(C):
            base = 128 + 70 * np.sin(xx / (5.0 + n + c)) * np.cos(yy / (7.0 + 2 * c)) + 20 * np.sin((xx + yy) / 11.0)
            hr[n, c] = np.clip(base + rs.randn(H, W) * 8, 0, 255).astype(np.uint8)
    sr = np.clip(hr.astype(np.int32) + rs.randint(-noise, noise + 1, hr.shape), 0, 255).astype(np.uint8)
    return sr, hr


def _cpu_metrics(sr, hr, crop, to_y):
    """Per-frame CPU PSNR / SSIM of (N,C,H,W) uint8 RGB frames, scored as HWC images (BGR-flipped for Y, as mmedit does)."""
    ps, ss = [], []
    for a, b in zip(sr, hr):
        if to_y:
            ab, bb = a[::-1].transpose(1, 2, 0), b[::-1].transpose(1, 2, 0)
            ps.append(psnr(to_y_channel(ab), to_y_channel(bb), crop))
            ss.append(ssim(ab, bb, crop, convert_to="Y"))
        else:
            ps.append(psnr(a.transpose(1, 2, 0), b.transpose(1, 2, 0), crop))
            ss.append(ssim(a.transpose(1, 2, 0), b.transpose(1, 2, 0), crop))
    return np.array(ps), np.array(ss)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fm(*a, **k):
    from fcvsr_amd.harness.device_metrics import frame_metrics
    p, s = frame_metrics(*a, **k)
    assert p.dtype == torch.float64 and s.dtype == torch.float64 and p.is_cuda and s.is_cuda
    return p.cpu().numpy(), s.cpu().numpy()


def test_known_answers_of_the_reference_on_the_device():
    """mmedit_train/tests/test_metrics/test_metrics.py:79-106: ones vs twos give SSIM 0.9130623 for every crop, 0.9987801 on Y."""
    ones, twos = np.ones((1, 1, 32, 32), np.uint8), np.full((1, 1, 32, 32), 2, np.uint8)
    for crop in range(5):
        _, s = _fm(_dev(ones), _dev(twos), crop_border=crop, quantise=None)
        np.testing.assert_almost_equal(s[0], 0.9130623)
    ones3, twos3 = np.ones((1, 3, 32, 32), np.uint8), np.full((1, 3, 32, 32), 2, np.uint8)
    _, s = _fm(_dev(ones3), _dev(twos3), crop_border=0, quantise=None)
    np.testing.assert_almost_equal(s[0], 0.9130623)
    _, s = _fm(_dev(ones3), _dev(twos3), crop_border=0, quantise=None, convert_to="Y")
    np.testing.assert_almost_equal(s[0], 0.9987801)


@pytest.mark.parametrize("H,W,N", [(72, 80, 3), (101, 37, 3), (720, 1280, 2)])
@pytest.mark.parametrize("C,to_y", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("crop", [0, 4])
def test_uint8_frames_match_the_cpu_functions(H, W, N, C, to_y, crop):
    sr, hr = _structured(np.random.RandomState(H * 7 + W + C + crop), N, C, H, W)
    p, s = _fm(_dev(sr), _dev(hr), crop_border=crop, quantise=None, convert_to="Y" if to_y else None)
    rp, rs_ = _cpu_metrics(sr, hr, crop, to_y)
    assert rs_.min() > 0.5                                      # structured inputs: SSIM far from 0
    assert np.abs(p - rp).max() <= TOL, (p, rp)
    assert np.abs(s - rs_).max() <= TOL, (s, rs_)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("C,to_y", [(1, False), (3, True), (3, False)])
def test_f32_frames_are_quantised_like_torch(quantise, C, to_y):
    """SR in [0,1] f32 with exact k/255 values, half steps, values below 0 and above 1, as a non-contiguous crop of a padded
    buffer: the kernel's quantisation equals torch's `(sr.clamp(0,1)*255).to(uint8)` (and `.round()` first)."""
    rs = np.random.RandomState(11 + C)
    N, H, W = 3, 45, 61
    _, hr = _structured(rs, N, C, H, W)
    v = hr.astype(np.float32) / 255.0 + rs.randn(N, C, H, W).astype(np.float32) * 0.01
    k = rs.randint(0, 256, v.shape)
    sel = rs.rand(*v.shape)
    v = np.where(sel < 0.15, (k / 255.0).astype(np.float32), v)
    v = np.where((sel >= 0.15) & (sel < 0.25), ((k + 0.5) / 255.0).astype(np.float32), v)
    v = np.where((sel >= 0.25) & (sel < 0.28), np.float32(-0.3), v)
    v = np.where((sel >= 0.28) & (sel < 0.31), np.float32(1.4), v)
    padded = torch.zeros((N, C, H + 3, W + 7), dtype=torch.float32, device="cuda")
    padded[:, :, :H, :W] = torch.from_numpy(v.astype(np.float32)).cuda()
    sr = padded[:, :, :H, :W]
    assert not sr.is_contiguous()
    q = sr.clamp(0, 1) * 255.0
    q = q.round() if quantise == "round" else q
    sr_u8 = q.to(torch.uint8).cpu().numpy()
    for crop in (0, 4):
        p, s = _fm(sr, _dev(hr), crop_border=crop, quantise=quantise, convert_to="Y" if to_y else None)
        rp, rs_ = _cpu_metrics(sr_u8, hr, crop, to_y)
        assert np.abs(p - rp).max() <= TOL and np.abs(s - rs_).max() <= TOL, (p, rp, s, rs_)
    # channels-last storage: strided channel axis
    sr_cl = sr.contiguous(memory_format=torch.channels_last)
    p, s = _fm(sr_cl, _dev(hr), crop_border=4, quantise=quantise, convert_to="Y" if to_y else None)
    rp, rs_ = _cpu_metrics(sr_u8, hr, 4, to_y)
    assert np.abs(p - rp).max() <= TOL and np.abs(s - rs_).max() <= TOL


def test_identical_frames_reproducibility_and_argument_errors():
    from fcvsr_amd.harness.device_metrics import frame_metrics
    sr, hr = _structured(np.random.RandomState(5), 4, 3, 90, 130)
    p, s = _fm(_dev(hr), _dev(hr), quantise=None)
    assert np.all(np.isinf(p)) and np.all(p > 0)
    assert np.abs(s - 1.0).max() <= 1e-12
    a = frame_metrics(_dev(sr), _dev(hr), quantise=None, convert_to="Y")
    b = frame_metrics(_dev(sr), _dev(hr), quantise=None, convert_to="Y")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):                              # shapes differ
        frame_metrics(_dev(sr), _dev(hr[:, :, :-1]), quantise=None)
    with pytest.raises(ValueError):                              # 18 - 2*4 - 10 = 0: empty SSIM region
        frame_metrics(_dev(sr[:, :, :18, :40]), _dev(hr[:, :, :18, :40]), quantise=None)
    with pytest.raises(ValueError):                              # f32 SR announced as uint8
        frame_metrics(_dev(sr).float() / 255, _dev(hr), quantise=None)
    with pytest.raises(ValueError):                              # Y needs 3 channels
        frame_metrics(_dev(sr[:, :1]), _dev(hr[:, :1]), quantise=None, convert_to="Y")
    with pytest.raises(RuntimeError):                            # no CPU fallback
        frame_metrics(torch.from_numpy(sr), torch.from_numpy(hr), quantise=None)


def _model(name):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    model = {"GShiftNet_S": GShiftNet_S, "FCVSR_SNet": FCVSR_SNet}[name]()
    model.load_state_dict(synthetic_state_dict(state_dict_shapes(name)))
    return model.cuda()


def _noisy_hr(sr_u8, seed):
    rs = np.random.RandomState(seed)
    return np.clip(sr_u8.astype(np.int32) + rs.randint(-5, 6, sr_u8.shape), 0, 255).astype(np.uint8)


def test_evaluate_sequence_equals_the_cpu_sequence_metrics():
    from fcvsr_amd.harness.infer import evaluate_sequence, sequence_psnr, sequence_ssim, super_resolve_sequence
    model = _model("GShiftNet_S")
    N, H, W = 5, 18, 20                                          # H is not a multiple of 4: padded, then cropped by view
    rs = np.random.RandomState(3)
    lr = torch.from_numpy((rs.randint(0, 256, (N, 1, H, W)) / 255.0).astype(np.float32))
    sr = super_resolve_sequence(model, lr, batch=2)
    hr = _noisy_hr(sr, 1)
    got = evaluate_sequence(model, lr, torch.from_numpy(hr), batch=2)
    assert got.frames is None and got.psnr.dtype == np.float64 and got.psnr.shape == (N,)
    for i in range(N):
        assert abs(got.psnr[i] - psnr(sr[i, 0], hr[i, 0], 4)) <= TOL
        assert abs(got.ssim[i] - ssim(sr[i, 0], hr[i, 0], 4)) <= TOL
    assert abs(got.psnr_mean - sequence_psnr(sr, hr)) <= TOL and abs(got.ssim_mean - sequence_ssim(sr, hr)) <= TOL
    again = evaluate_sequence(model, lr, torch.from_numpy(hr).cuda(), batch=2, return_frames=True)
    assert np.array_equal(again.frames, sr) and np.array_equal(again.psnr, got.psnr) and np.array_equal(again.ssim, got.ssim)


def test_evaluate_sequence_rgb_twin_round_and_y():
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    model = _model("FCVSR_SNet")
    N, H, W = 4, 14, 20
    rs = np.random.RandomState(4)
    lr = torch.from_numpy((rs.randint(0, 256, (N, 3, H, W)) / 255.0).astype(np.float32))
    sr = super_resolve_sequence(model, lr, batch=3, quantise="round")
    hr = _noisy_hr(sr, 2)
    got = evaluate_sequence(model, lr, torch.from_numpy(hr), batch=3, quantise="round", convert_to="Y", return_frames=True)
    assert np.array_equal(got.frames, sr)
    rp, rs_ = _cpu_metrics(sr, hr, 4, True)
    assert np.abs(got.psnr - rp).max() <= TOL and np.abs(got.ssim - rs_).max() <= TOL


def test_fit_validates_without_touching_the_training_state(monkeypatch):
    import fcvsr_amd.train.step as step_mod
    from fcvsr_amd.harness.infer import evaluate_sequence
    made = []

    class Recorded(step_mod.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(step_mod, "TrainStep", Recorded)
    model = _model("GShiftNet_S")
    rs = np.random.RandomState(9)
    h = w = 16

    def batches(epoch):
        for _ in range(2):
            hr = rs.randint(0, 256, (1, 1, 1, 4 * h, 4 * w)) / 255.0
            yield {"lr_imgs": torch.from_numpy((rs.randint(0, 256, (1, 1, 7, h, w)) / 255.0).astype(np.float32)),
                   "hr_imgs": torch.from_numpy(hr.astype(np.float32))}

    val = []
    for n, seed in ((4, 1), (3, 2)):
        lr = torch.from_numpy((np.random.RandomState(seed).randint(0, 256, (n, 1, 10, 12)) / 255.0).astype(np.float32))
        hr = torch.from_numpy(np.random.RandomState(seed + 10).randint(0, 256, (n, 1, 40, 48)).astype(np.uint8))
        val.append((lr, hr))
    snaps, logs, calls = [], [], []

    def snapshot():
        opt = made[0].optimizer
        return ([p.detach().clone() for p in model.parameters()],
                [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()],
                {k: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in st.items()} for k, st in opt.state_dict()["state"].items()})

    def log(msg):
        logs.append(msg)
        if msg.startswith("Epoch:"):
            snaps.append(snapshot())                         # after the epoch's training, before its validation

    def on_validate(epoch, p, s):
        calls.append((epoch, p, s))
        before, after = snaps[-1], snapshot()
        for a, b in zip(before[0], after[0]):
            assert torch.equal(a, b)
        for a, b in zip(before[1], after[1]):
            assert (a is None and b is None) or torch.equal(a, b)
        assert before[2].keys() == after[2].keys()
        for k in before[2]:
            for n in before[2][k]:
                x, y = before[2][k][n], after[2][k][n]
                assert torch.equal(x, y) if torch.is_tensor(x) else x == y

    step_mod.fit(model, batches, epochs=2, device="cuda", val_itv=1, log=log, val_sequences=val, on_validate=on_validate)
    assert [c[0] for c in calls] == [1, 2]
    lines = [m for m in logs if m.startswith("PSNR:")]
    assert len(lines) == 2
    assert all(re.fullmatch(r"PSNR:-?[0-9.]+, SSIM: -?[0-9.]+", m) for m in lines), lines
    assert lines[-1] == "PSNR:%f, SSIM: %f" % (calls[-1][1], calls[-1][2])
    scores = [evaluate_sequence(model, lr, hr) for lr, hr in val]
    assert calls[-1][1] == float(np.mean([s.psnr_mean for s in scores]))
    assert calls[-1][2] == float(np.mean([s.ssim_mean for s in scores]))


def test_fit_without_validation_is_unchanged():
    """val_sequences=None: no validation line, no callback, the same loss history as before."""
    import fcvsr_amd.train.step as step_mod
    model = _model("GShiftNet_S")
    rs = np.random.RandomState(2)
    data = [{"lr_imgs": torch.from_numpy((rs.randint(0, 256, (1, 1, 7, 16, 16)) / 255.0).astype(np.float32)),
             "hr_imgs": torch.from_numpy((rs.randint(0, 256, (1, 1, 1, 64, 64)) / 255.0).astype(np.float32))}]
    logs = []
    hist = step_mod.fit(model, lambda e: iter(data), epochs=1, device="cuda", log=logs.append)
    assert len(hist) == 1 and len(logs) == 1 and logs[0].startswith("Epoch: 1/1")
