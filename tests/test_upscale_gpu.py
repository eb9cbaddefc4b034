"""GPU: fcvsr_bicubic_upscale against the bits of the CPU contract (fcvsr_amd/harness/niqe.py bicubic_upscale, itself pinned to the
reference's recorded outputs by tests/test_upscale_cpu.py) on the smallest shapes at which the kernel can go wrong, the `baseline=`
keyword of the sequence scorer, and the file-to-file bicubic baseline of YUV 4:2:0 sequences."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (1,1,1,1): every tap reflects to the one sample; one-row and one-column planes; narrower than a store group, several planes, odd
# width; all stores aligned; ragged ends on both axes (and more than one workgroup per plane at 4x: 38 x 23 threads)
SHAPES = ((1, 1, 1, 1), (2, 1, 1, 9), (2, 1, 9, 1), (2, 3, 5, 7), (1, 1, 12, 16), (3, 1, 37, 23))


def _input(shape, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "u8":
        return rs.randint(0, 256, shape).astype(np.uint8)
    if kind == "u16":
        return rs.randint(0, 1024, shape).astype(np.uint16)
    return rs.random_sample(shape).astype(np.float32)


def _dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _host(t: torch.Tensor) -> np.ndarray:
    from fcvsr_amd.hip import frames_to_numpy
    return frames_to_numpy(t)


def _check(x: np.ndarray, factor: int, dev_in=None):
    """The device result of both output forms against the contract's bits."""
    from fcvsr_amd.harness.niqe import bicubic_upscale as contract
    from fcvsr_amd.harness.resize import bicubic_upscale
    dev_in = _dev(x) if dev_in is None else dev_in
    want_shape = tuple(x.shape[:-2]) + (factor * x.shape[-2], factor * x.shape[-1])
    got = bicubic_upscale(dev_in, factor)
    assert got.dtype == torch.float32 and tuple(got.shape) == want_shape and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(contract(x, factor).astype(np.float32)))
    if x.dtype != np.float32:
        goti = bicubic_upscale(dev_in, factor, out="int")
        assert goti.dtype == dev_in.dtype and tuple(goti.shape) == want_shape
        assert np.array_equal(_host(goti), contract(x, factor, out="int"))


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_device_bits_on_the_edge_shapes(kind, factor):
    for k, shape in enumerate(SHAPES):
        _check(_input(shape, kind, 40 + k), factor)


def test_device_matches_the_reference_goldens(golden_dir):
    """The recorded outputs of the reference's own function, straight against the device (no contract in between)."""
    from fcvsr_amd.harness.resize import bicubic_upscale
    cases = np.load(os.path.join(golden_dir, "upscale_cases.npz"))
    for name in ("37x23_u8", "37x23_u10", "37x23_f32", "2x3_u8", "const_5x7_u8"):
        for factor in (2, 4):
            got = bicubic_upscale(_dev(cases[f"in_{name}"]), factor)
            assert torch.equal(got.cpu(), torch.from_numpy(cases[f"out_{name}_x{factor}"])), (name, factor)


@pytest.mark.parametrize("factor", [2, 4])
def test_non_contiguous_view_of_a_larger_tensor(factor):
    big = _input((2, 2, 20, 30), "u8", 50)
    dev = _dev(big)[:, :, 3:16, 5:24]
    assert not dev.is_contiguous()
    _check(np.ascontiguousarray(big[:, :, 3:16, 5:24]), factor, dev)
    bigf = _input((2, 11, 14), "f32", 51)
    devf = _dev(bigf)[:, 1:10, 2:13]
    _check(np.ascontiguousarray(bigf[:, 1:10, 2:13]), factor, devf)
    big16 = _input((2, 11, 14), "u16", 52)
    dev16 = _dev(big16).view(torch.int16)[:, 1:10, 2:13].view(torch.uint16)
    _check(np.ascontiguousarray(big16[:, 1:10, 2:13]), factor, dev16)


@pytest.mark.parametrize("factor", [2, 4])
def test_checkerboard_clips_in_the_integer_form(factor):
    from fcvsr_amd.harness.niqe import bicubic_upscale as contract
    from fcvsr_amd.harness.resize import bicubic_upscale
    yy, xx = np.mgrid[0:8, 0:10]
    for dtype, peak in ((np.uint8, 255), (np.uint16, 1023)):
        chk = (((yy + xx) & 1) * peak).astype(dtype)[None]
        f32 = contract(chk, factor)
        assert (f32 < 0).any() and (f32 > peak).any()
        got = _host(bicubic_upscale(_dev(chk), factor, out="int"))
        assert got.min() == 0 and got.max() == peak
        _check(chk, factor)


@pytest.mark.parametrize("factor", [2, 4])
def test_uint16_samples_above_1023_read_as_1023(factor):
    x = _input((2, 9, 13), "u16", 53)
    wild = x.copy()
    at = np.random.RandomState(54).rand(*x.shape) < 0.2
    x[at] = 1023
    wild[at] = np.random.RandomState(55).randint(1024, 65536, int(at.sum())).astype(np.uint16)
    assert wild.max() > 32767                                 # the sign bit of the int16 view the tensor travels as
    from fcvsr_amd.harness.resize import bicubic_upscale
    for out in ("f32", "int"):
        a, b = bicubic_upscale(_dev(wild), factor, out=out), bicubic_upscale(_dev(x), factor, out=out)
        assert np.array_equal(_host(a), _host(b))
    _check(wild, factor)


def test_argument_errors_raise_before_any_launch():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.resize import bicubic_upscale
    x = torch.zeros(1, 1, 4, 4, dtype=torch.uint8).cuda()
    for bad in (1, 3, 8):
        with pytest.raises(ValueError, match="factor"):
            bicubic_upscale(x, bad)
    with pytest.raises(ValueError, match="int"):
        bicubic_upscale(x.float(), 4, out="int")
    with pytest.raises(ValueError, match="out"):
        bicubic_upscale(x, 4, out="u8")
    for dtype in (torch.float16, torch.int32, torch.float64):
        with pytest.raises(ValueError, match="uint8, uint16 or f32"):
            bicubic_upscale(x.to(dtype), 4)
    with pytest.raises(TypeError):
        bicubic_upscale(np.zeros((4, 4), dtype=np.uint8), 4)
    assert tuple(bicubic_upscale(torch.zeros(0, 1, 4, 4, dtype=torch.uint8).cuda(), 4).shape) == (0, 1, 16, 16)
    # the C entry point: FCVSR_E_ARG instead of a launch
    out = torch.zeros(64, dtype=torch.float32).cuda()
    fn, st = hip.lib().fcvsr_bicubic_upscale, hip.stream_ptr()
    assert fn(x.data_ptr(), hip.U8, 1, 4, 4, 4, None, hip.F32, st) == -1
    assert fn(x.data_ptr(), hip.U8, 1, 4, 4, 3, out.data_ptr(), hip.F32, st) == -1
    assert fn(x.data_ptr(), hip.U8, 1, 4, 4, 2, out.data_ptr(), hip.U16, st) == -1
    assert fn(x.data_ptr(), hip.U8, 0, 4, 4, 2, out.data_ptr(), hip.F32, st) == -1
    assert fn(x.data_ptr(), hip.U8, 1, 4, 4, 2, out.data_ptr() + 4, hip.F32, st) == -1      # f32 output: 16-byte aligned
    assert fn(x.data_ptr(), hip.U8, 1, 4, 4, 2, out.data_ptr(), hip.F32, st) == 0


def _model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    return m


@pytest.fixture(scope="module")
def s_model():
    return _model()


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_evaluate_sequence_baseline_keyword(s_model, kind):
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.harness.niqe import bicubic_upscale as contract
    lr_np, hr_np = _input((3, 1, 16, 20), kind, 60), _input((3, 1, 64, 80), kind, 61)
    lr, hr = (torch.from_numpy(a.view(np.int16)).view(torch.uint16) if kind == "u16" else torch.from_numpy(a) for a in (lr_np, hr_np))
    plain = evaluate_sequence(s_model, lr, hr, batch=2)
    assert plain.baseline_psnr is None and plain.baseline_ssim_mean is None
    got = evaluate_sequence(s_model, lr, hr, batch=2, baseline="bicubic")
    assert np.array_equal(got.psnr, plain.psnr) and np.array_equal(got.ssim, plain.ssim)
    p, q = frame_metrics(_dev(contract(lr_np, 4, out="int")), _dev(hr_np), crop_border=4, quantise=None)
    p, q = p.cpu().numpy(), q.cpu().numpy()
    assert got.baseline_psnr.dtype == np.float64 and got.baseline_psnr.shape == (3,) and got.baseline_ssim.shape == (3,)
    assert np.array_equal(got.baseline_psnr.view(np.int64), p.view(np.int64))
    assert np.array_equal(got.baseline_ssim.view(np.int64), q.view(np.int64))
    assert got.baseline_psnr_mean == float(np.mean(p)) and got.baseline_ssim_mean == float(np.mean(q))
    assert got.baseline_niqe is None and got.baseline_niqe_mean is None
    with pytest.raises(ValueError, match="baseline"):
        evaluate_sequence(s_model, lr, hr, baseline="bilinear")


def test_evaluate_sequence_baseline_float_frames_ensemble_and_niqe(s_model, golden_dir):
    """Float lr: the f32 baseline frames are quantised by the metric kernel as the SR frames are.  The baseline does not depend on
    ensemble=, and niqe= scores it too.  24 x 48 LR frames: the 96 x 192 SR frame holds the two blocks NIQE needs."""
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.harness.niqe import NiqeModel, frame_niqe
    from fcvsr_amd.harness.niqe import bicubic_upscale as contract
    niqe = NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    lr_np, hr_np = _input((2, 1, 24, 48), "u8", 62), _input((2, 1, 96, 192), "u8", 63)
    lr, hr = torch.from_numpy(lr_np), torch.from_numpy(hr_np)
    lrf = lr.float() / 255
    for quantise in ("truncate", "round"):
        got = evaluate_sequence(s_model, lrf, hr, batch=2, quantise=quantise, baseline="bicubic")
        up = _dev(contract(lrf.numpy(), 4).astype(np.float32))
        p, q = frame_metrics(up, _dev(hr_np), crop_border=4, quantise=quantise)
        assert np.array_equal(got.baseline_psnr, p.cpu().numpy()) and np.array_equal(got.baseline_ssim, q.cpu().numpy())
    a = evaluate_sequence(s_model, lr, hr, batch=2, baseline="bicubic", niqe=niqe)
    b = evaluate_sequence(s_model, lr, hr, batch=2, baseline="bicubic", ensemble="spatial")
    assert np.array_equal(a.baseline_psnr, b.baseline_psnr) and np.array_equal(a.baseline_ssim, b.baseline_ssim)
    assert b.baseline_niqe is None
    ref = frame_niqe(_dev(contract(lr_np, 4, out="int")), niqe)
    assert np.array_equal(a.baseline_niqe, ref, equal_nan=True) and a.baseline_niqe_mean == float(np.mean(a.baseline_niqe))


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_upscale_yuv420_writes_the_contract_of_the_three_planes(tmp_path, bit_depth):
    from fcvsr_amd.harness.niqe import bicubic_upscale as contract
    from fcvsr_amd.harness.yuv import read_yuv420, upscale_yuv420, write_yuv420
    N, H, W = 3, 12, 20
    kind = "u8" if bit_depth == 8 else "u16"
    y, u, v = _input((N, H, W), kind, 70), _input((N, H // 2, W // 2), kind, 71), _input((N, H // 2, W // 2), kind, 72)
    src = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv")
    write_yuv420(src, y, u, v)
    for factor in (4, 2):
        dst = str(tmp_path / f"bicubic_x{factor}.yuv")
        stats = upscale_yuv420(src, dst, W, H, factor=factor, bit_depth=bit_depth, batch=2)
        assert stats["frames"] == N and stats["out_size"] == (factor * W, factor * H)
        assert stats["bytes_written"] == os.path.getsize(dst) == N * factor * factor * W * H * 3 // 2 * (bit_depth // 8 + (bit_depth > 8))
        assert set(stats) == {"frames", "seconds", "fps", "bytes_read", "bytes_written", "out_size"}
        want = str(tmp_path / f"want_x{factor}.yuv")
        write_yuv420(want, *(contract(a, factor, out="int") for a in (y, u, v)))
        assert open(dst, "rb").read() == open(want, "rb").read()
        oy, ou, ov = read_yuv420(dst, factor * W, factor * H, bit_depth=bit_depth)
        assert oy.shape == (N, factor * H, factor * W) and ou.shape == ov.shape == (N, factor * H // 2, factor * W // 2)
