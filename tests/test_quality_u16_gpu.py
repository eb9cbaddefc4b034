"""GPU: on-device PSNR / SSIM of 10-bit frames (fcvsr_frame_metrics_u16 through harness.device_metrics.frame_metrics with uint16
hr) against the CPU functions of harness/metrics.py with peak=1023."""
import math

import numpy as np
import pytest
import torch

from fcvsr_amd.harness.metrics import psnr, ssim

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _structured(rs, N, C, H, W, noise=24):
    """uint16 10-bit HR = smooth pattern + noise, SR = HR +- small noise: SSIM far from 0."""
    yy, xx = np.mgrid[:H, :W]
    hr = np.empty((N, C, H, W), dtype=np.uint16)
    for n in range(N):
        for c in range(C):
            base = 512 + 280 * np.sin(xx / (5.0 + n + c)) * np.cos(yy / (7.0 + 2 * c)) + 80 * np.sin((xx + yy) / 11.0)
            hr[n, c] = np.clip(base + rs.randn(H, W) * 32, 0, 1023).astype(np.uint16)
    sr = np.clip(hr.astype(np.int32) + rs.randint(-noise, noise + 1, hr.shape), 0, 1023).astype(np.uint16)
    return sr, hr


def _cpu_metrics(sr, hr, crop, peak=1023):
    ps = [psnr(a.transpose(1, 2, 0), b.transpose(1, 2, 0), crop, peak=peak) for a, b in zip(sr, hr)]
    ss = [ssim(a.transpose(1, 2, 0), b.transpose(1, 2, 0), crop, peak=peak) for a, b in zip(sr, hr)]
    return np.array(ps), np.array(ss)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _fm(*a, **k):
    from fcvsr_amd.harness.device_metrics import frame_metrics
    p, s = frame_metrics(*a, **k)
    assert p.dtype == torch.float64 and s.dtype == torch.float64 and p.is_cuda and s.is_cuda
    return p.cpu().numpy(), s.cpu().numpy()


# 32 x 40 with crop 4: a 14 x 22 map, one partial tile; 37 x 101 uncropped: a 27 x 91 map, 2 x 2 tiles with ragged edges;
# 25 x 21 with crop 2: an 11 x 7 map, a single partial tile
@pytest.mark.parametrize("H,W,crop", [(32, 40, 4), (37, 101, 0), (25, 21, 2)])
@pytest.mark.parametrize("C", [1, 3])
def test_uint16_frames_match_the_cpu_functions(H, W, crop, C):
    sr, hr = _structured(np.random.RandomState(H * 7 + W + C + crop), 3, C, H, W)
    p, s = _fm(_dev16(sr), _dev16(hr), crop_border=crop, quantise=None)
    rp, rs_ = _cpu_metrics(sr, hr, crop)
    assert rs_.min() > 0.5                                      # structured inputs: SSIM far from 0
    assert np.abs(p - rp).max() <= TOL, (p, rp)
    assert np.abs(s - rs_).max() <= TOL, (s, rs_)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("H,W,crop", [(32, 40, 4), (25, 21, 2)])
def test_f32_frames_are_quantised_with_the_1023_scale(quantise, H, W, crop):
    """SR in [0,1] f32 with exact k/1023 values, half steps, values below 0 and above 1, as a non-contiguous crop of a padded
    buffer: the kernel's quantisation equals torch's `(sr.clamp(0,1)*1023)` truncated (and `.round()` first)."""
    rs = np.random.RandomState(11 + H)
    N, C = 3, 1
    _, hr = _structured(rs, N, C, H, W)
    v = hr.astype(np.float32) / np.float32(1023) + rs.randn(N, C, H, W).astype(np.float32) * 0.01
    k = rs.randint(0, 1024, v.shape)
    sel = rs.rand(*v.shape)
    v = np.where(sel < 0.15, (k / 1023.0).astype(np.float32), v)
    v = np.where((sel >= 0.15) & (sel < 0.25), ((k + 0.5) / 1023.0).astype(np.float32), v)
    v = np.where((sel >= 0.25) & (sel < 0.28), np.float32(-0.3), v)
    v = np.where((sel >= 0.28) & (sel < 0.31), np.float32(1.4), v)
    padded = torch.zeros((N, C, H + 3, W + 7), dtype=torch.float32, device="cuda")
    padded[:, :, :H, :W] = torch.from_numpy(v.astype(np.float32)).cuda()
    sr = padded[:, :, :H, :W]
    assert not sr.is_contiguous()
    q = sr.clamp(0, 1) * 1023.0
    q = q.round() if quantise == "round" else q
    sr_u16 = q.to(torch.int32).cpu().numpy().astype(np.uint16)
    p, s = _fm(sr, _dev16(hr), crop_border=crop, quantise=quantise)
    rp, rs_ = _cpu_metrics(sr_u16, hr, crop)
    assert np.abs(p - rp).max() <= TOL and np.abs(s - rs_).max() <= TOL, (p, rp, s, rs_)
    # the same frames, already quantised
    p2, s2 = _fm(_dev16(sr_u16), _dev16(hr), crop_border=crop, quantise=None)
    assert np.array_equal(p, p2) and np.array_equal(s, s2)


def test_peak_1020_identical_frames_reproducibility_and_argument_errors():
    from fcvsr_amd.harness.device_metrics import frame_metrics
    sr, hr = _structured(np.random.RandomState(5), 4, 3, 45, 61)
    p, s = _fm(_dev16(sr), _dev16(hr), quantise=None)
    p20, s20 = _fm(_dev16(sr), _dev16(hr), quantise=None, peak=1020)
    assert np.abs((p20 - p) - 20.0 * math.log10(1020.0 / 1023.0)).max() <= TOL
    rp, rs_ = _cpu_metrics(sr, hr, 4, peak=1020)
    assert np.abs(p20 - rp).max() <= TOL and np.abs(s20 - rs_).max() <= TOL
    assert np.abs(s20 - s).max() > 0                             # the SSIM constants follow the peak
    p, s = _fm(_dev16(hr), _dev16(hr), quantise=None)
    assert np.all(np.isinf(p)) and np.all(p > 0)
    assert np.abs(s - 1.0).max() <= 1e-12
    a = frame_metrics(_dev16(sr), _dev16(hr), quantise=None)
    b = frame_metrics(_dev16(sr), _dev16(hr), quantise=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):                              # Y is not defined for 10-bit frames
        frame_metrics(_dev16(sr), _dev16(hr), quantise=None, convert_to="Y")
    with pytest.raises(ValueError):                              # uint8 SR against uint16 HR
        frame_metrics(torch.zeros(4, 3, 45, 61, dtype=torch.uint8, device="cuda"), _dev16(hr), quantise=None)
    with pytest.raises(ValueError):                              # uint8 frames are scored at 255
        frame_metrics(torch.zeros(4, 3, 45, 61, dtype=torch.uint8, device="cuda"),
                      torch.zeros(4, 3, 45, 61, dtype=torch.uint8, device="cuda"), quantise=None, peak=1020)
    with pytest.raises(ValueError):
        frame_metrics(_dev16(sr), _dev16(hr), quantise=None, peak=0)
    with pytest.raises(RuntimeError):                            # no CPU fallback
        frame_metrics(torch.from_numpy(sr), torch.from_numpy(hr), quantise=None)


def test_library_rejects_y_conversion_for_10_bit_frames():
    import ctypes as C
    from fcvsr_amd import hip
    from fcvsr_amd.harness.metrics import _gaussian_window
    L = hip.lib()
    fr = torch.zeros(1, 3, 32, 32, dtype=torch.int16, device="cuda")
    st = (C.c_int64 * 4)(*fr.stride())
    win = (C.c_double * 11)(*_gaussian_window())
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(64, dtype=torch.float64, device="cuda")
    args = lambda to_y, peak: (fr.data_ptr(), st, 0, fr.data_ptr(), st, 1, 3, 32, 32, 0, to_y, win, peak, out.data_ptr(),
                               scratch.data_ptr(), scratch.numel() * 8, hip.stream_ptr())
    assert L.fcvsr_frame_metrics_u16(*args(1, 1023.0)) == -1
    assert L.fcvsr_frame_metrics_u16(*args(0, 0.0)) == -1
    assert L.fcvsr_frame_metrics_u16(*args(0, 1023.0)) == 0
    torch.cuda.synchronize()
