"""GPU: fcvsr_imresize against the bits of the CPU contract (fcvsr_amd/harness/resize.py imresize_host, itself pinned to the
reference's recorded outputs by tests/test_imresize_cpu.py) on the smallest shapes at which the kernel can go wrong, straight
against a handful of the reference's goldens, and the output_shape= keyword of the five harness entry points."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (leading dims, H, W), keywords.  Every tap reflects to the one sample; a one-row and a one-column plane (tap order in the class
# where the reference itself sums pairwise); more taps than 2n, so reflection wraps several times; columns first; ragged tiles and
# several workgroups on both axes (50 x 70 outputs: 7 x 3 tiles), rows first; 34 stored taps on both axes; the widest LDS tile of
# each order (rows first: 33 output columns at 1/8, a full tile of 32 spanning 280 source columns; columns first: 10 output rows at
# 10/72 over columns at 1/8, a full tile of 8 spanning 82 source rows); a tie at a scale that is no integer; shrinking by scale=
# with a ceil'd size
CASES = (((1, 1), 1, 1, dict(output_shape=(3, 3))),
         ((2,), 1, 9, dict(output_shape=(1, 7))),
         ((2,), 9, 1, dict(output_shape=(7, 1))),
         ((1,), 2, 3, dict(scale=0.3)),
         ((1, 1), 12, 16, dict(output_shape=(30, 9))),
         ((3,), 37, 23, dict(output_shape=(50, 70))),
         ((1,), 40, 48, dict(scale=1 / 8)),
         ((1,), 40, 264, dict(scale=1 / 8)),
         ((1,), 72, 64, dict(output_shape=(10, 8))),
         ((2, 1), 37, 23, dict(scale=1.25)),
         ((1,), 45, 80, dict(scale=2 / 3)))


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


def _check(x: np.ndarray, kw: dict, dev_in=None):
    """The device result of both output forms against the contract's bits."""
    from fcvsr_amd.harness.resize import imresize, imresize_host
    dev_in = _dev(x) if dev_in is None else dev_in
    want = imresize_host(x, **kw)
    got = imresize(dev_in, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32))), kw
    if x.dtype != np.float32:
        goti = imresize(dev_in, out="int", **kw)
        assert goti.dtype == dev_in.dtype and tuple(goti.shape) == want.shape
        assert np.array_equal(_host(goti), imresize_host(x, out="int", **kw)), kw


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_device_bits_on_the_edge_shapes(kind):
    for k, (lead, h, w, kw) in enumerate(CASES):
        _check(_input(lead + (h, w), kind, 140 + k), kw)


def test_device_matches_the_reference_goldens(golden_dir):
    """The recorded outputs of the reference's own class, straight against the device (no contract in between)."""
    from fcvsr_amd.harness.resize import imresize
    cases = np.load(os.path.join(golden_dir, "imresize_cases.npz"))
    scales = cases["scales"]
    picks = (("37x23_u8", "s0"), ("37x23_u10", "s2"), ("37x23_f32", "s5"), ("45x80_u8", "s1"), ("45x80_f32", "s4"), ("2x3_u8", "s3"),
             ("12x16_u10", "s6"), ("45x80_u8", "27x48"), ("12x16_f32", "24x8"), ("37x23_u10", "12x69"), ("5x7_u8", "6x8"),
             ("const_5x7_u8", "s2"), ("checker_8x10_u8", "s4"))
    for name, key in picks:
        ref = cases[f"out_{name}_{key}"]
        kw = dict(scale=float(scales[int(key[1:])])) if key.startswith("s") else dict(output_shape=ref.shape)
        got = imresize(_dev(cases[f"in_{name}"]), **kw)
        assert torch.equal(got.cpu(), torch.from_numpy(ref)), (name, key)


def test_non_contiguous_view_of_a_larger_tensor():
    kw = dict(output_shape=(17, 11))
    big = _input((2, 2, 20, 30), "u8", 150)
    dev = _dev(big)[:, :, 3:16, 5:24]
    assert not dev.is_contiguous()
    _check(np.ascontiguousarray(big[:, :, 3:16, 5:24]), kw, dev)
    bigf = _input((2, 11, 14), "f32", 151)
    _check(np.ascontiguousarray(bigf[:, 1:10, 2:13]), kw, _dev(bigf)[:, 1:10, 2:13])
    big16 = _input((2, 11, 14), "u16", 152)
    dev16 = _dev(big16).view(torch.int16)[:, 1:10, 2:13].view(torch.uint16)
    _check(np.ascontiguousarray(big16[:, 1:10, 2:13]), kw, dev16)


def test_checkerboard_clips_in_the_integer_form():
    from fcvsr_amd.harness.resize import imresize, imresize_host
    yy, xx = np.mgrid[0:8, 0:10]
    for dtype, peak in ((np.uint8, 255), (np.uint16, 1023)):
        chk = (((yy + xx) & 1) * peak).astype(dtype)[None]
        for kw in (dict(scale=1.5), dict(output_shape=(13, 17))):            # both axes up: the cubic overshoots on both sides
            f32 = imresize_host(chk, **kw)
            assert (f32 < 0).any() and (f32 > peak).any()
            got = _host(imresize(_dev(chk), out="int", **kw))
            assert got.min() == 0 and got.max() == peak
            _check(chk, kw)


def test_uint16_samples_above_1023_read_as_1023():
    from fcvsr_amd.harness.resize import imresize
    x = _input((2, 9, 13), "u16", 153)
    wild = x.copy()
    at = np.random.RandomState(154).rand(*x.shape) < 0.2
    x[at] = 1023
    wild[at] = np.random.RandomState(155).randint(1024, 65536, int(at.sum())).astype(np.uint16)
    assert wild.max() > 32767                                 # the sign bit of the int16 view the tensor travels as
    for kw in (dict(scale=0.75), dict(output_shape=(5, 30))):
        for out in ("f32", "int"):
            a, b = imresize(_dev(wild), out=out, **kw), imresize(_dev(x), out=out, **kw)
            assert np.array_equal(_host(a), _host(b))
        _check(wild, kw)


def test_argument_errors_raise_before_any_launch_and_tables_are_cached():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.resize import imresize
    x = torch.zeros(1, 1, 8, 8, dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="exactly one"):
        imresize(x)
    with pytest.raises(ValueError, match="exactly one"):
        imresize(x, scale=2, output_shape=(16, 16))
    with pytest.raises(ValueError, match="scale"):
        imresize(x, scale=0.1)
    with pytest.raises(ValueError, match="output_shape"):
        imresize(x, output_shape=(8, 65))
    with pytest.raises(ValueError, match="int"):
        imresize(x.float(), scale=2, out="int")
    with pytest.raises(ValueError, match="out"):
        imresize(x, scale=2, out="u8")
    for dtype in (torch.float16, torch.int32, torch.float64):
        with pytest.raises(ValueError, match="uint8, uint16 or f32"):
            imresize(x.to(dtype), scale=2)
    with pytest.raises(ValueError, match="non-empty"):
        imresize(torch.zeros(1, 0, 8, dtype=torch.uint8).cuda(), scale=2)
    with pytest.raises(TypeError):
        imresize(np.zeros((4, 4), dtype=np.uint8), scale=2)
    empty = imresize(torch.zeros(0, 1, 8, 8, dtype=torch.uint8).cuda(), output_shape=(12, 10), out="int")
    assert tuple(empty.shape) == (0, 1, 12, 10) and empty.dtype == torch.uint8
    imresize(x, output_shape=(12, 10))
    ty, tx = hip.resize_device_tables(8, 12, 12 / 8, x.device), hip.resize_device_tables(8, 10, 10 / 8, x.device)
    imresize(x, output_shape=(12, 10))
    assert hip.resize_device_tables(8, 12, 12 / 8, x.device)[0] is ty[0]      # uploaded once per size
    assert hip.resize_device_tables(8, 10, 10 / 8, x.device)[1] is tx[1]
    # the C entry point: FCVSR_E_ARG instead of a launch
    out = torch.zeros(12 * 10 + 1, dtype=torch.float32).cuda()
    fn, st = hip.lib().fcvsr_imresize, hip.stream_ptr()
    args = lambda **c: tuple({**dict(src=x.data_ptr(), sd=hip.U8, planes=1, H=8, W=8, Ho=12, Wo=10, wy=ty[0].data_ptr(), fy=ty[1].data_ptr(),
                                     Py=ty[2], wx=tx[0].data_ptr(), fx=tx[1].data_ptr(), Px=tx[2], rf=0, out=out.data_ptr(), od=hip.F32),
                              **c}.values()) + (st,)
    for change in (dict(out=None), dict(wy=None), dict(Py=35), dict(Px=0), dict(od=hip.U16), dict(planes=0), dict(Ho=65),
                   dict(out=out.data_ptr() + 2)):
        assert fn(*args(**change)) == -1, change
    assert fn(*args()) == 0
    assert torch.equal(out[:120].view(12, 10), imresize(x, output_shape=(12, 10))[0, 0])


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


def _torch16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


SHAPES = ((48, 60), (54, 70))          # 3x, and a size that is no multiple of the LR frame (16 x 20 LR, 64 x 80 at 4x)


@pytest.mark.parametrize("kind", ["u8", "u16", "float"])
def test_super_resolve_sequence_output_shape(s_model, kind):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.resize import imresize_host
    lr_np = _input((3, 1, 16, 20), "u8" if kind == "float" else kind, 160)
    lr = _torch16(lr_np).float() / 255 if kind == "float" else _torch16(lr_np)
    plain = super_resolve_sequence(s_model, lr, batch=2)
    assert np.array_equal(super_resolve_sequence(s_model, lr, batch=2, output_shape=None), plain)
    for shape in SHAPES:
        got = super_resolve_sequence(s_model, lr, batch=2, output_shape=shape)
        assert got.dtype == plain.dtype and got.shape == (3, 1) + shape
        assert np.array_equal(got, imresize_host(plain, output_shape=shape, out="int")), shape
    if kind == "u16":
        return
    for extra in (dict(ensemble="spatial"), dict(tile=(12, 16), tile_overlap=4), dict(quantise="round", cuts=[2])):
        plain = super_resolve_sequence(s_model, lr, batch=2, **extra)
        got = super_resolve_sequence(s_model, lr, batch=2, output_shape=SHAPES[1], **extra)
        assert np.array_equal(got, imresize_host(plain, output_shape=SHAPES[1], out="int")), extra


@pytest.mark.parametrize("kind", ["u8", "u16", "float"])
def test_evaluate_sequence_output_shape(s_model, kind):
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.resize import imresize_host
    ikind = "u8" if kind == "float" else kind
    shape = SHAPES[1]
    lr_np, hr_np, hr4_np = _input((3, 1, 16, 20), ikind, 161), _input((3, 1) + shape, ikind, 162), _input((3, 1, 64, 80), ikind, 163)
    lr, hr, hr4 = _torch16(lr_np), _torch16(hr_np), _torch16(hr4_np)
    if kind == "float":
        lr = lr.float() / 255
    a, b = evaluate_sequence(s_model, lr, hr4, batch=2), evaluate_sequence(s_model, lr, hr4, batch=2, output_shape=None)
    assert np.array_equal(a.psnr, b.psnr) and np.array_equal(a.ssim, b.ssim)
    got = evaluate_sequence(s_model, lr, hr, batch=2, output_shape=shape, return_frames=True, baseline="bicubic", quantise="round")
    frames = imresize_host(super_resolve_sequence(s_model, lr, batch=2, quantise="round"), output_shape=shape, out="int")
    assert np.array_equal(got.frames, frames)
    p, q = frame_metrics(_dev(frames), _dev(hr_np), crop_border=4, quantise=None)
    assert np.array_equal(got.psnr, p.cpu().numpy()) and np.array_equal(got.ssim, q.cpu().numpy())
    assert got.psnr_mean == float(np.mean(got.psnr))
    if kind == "float":                                       # f32 baseline frames, quantised by the metric kernel
        up = _dev(imresize_host(lr.numpy(), output_shape=shape).astype(np.float32))
        p, q = frame_metrics(up, _dev(hr_np), crop_border=4, quantise="round")
    else:
        p, q = frame_metrics(_dev(imresize_host(lr_np, output_shape=shape, out="int")), _dev(hr_np), crop_border=4, quantise=None)
    assert np.array_equal(got.baseline_psnr, p.cpu().numpy()) and np.array_equal(got.baseline_ssim, q.cpu().numpy())
    with pytest.raises(ValueError, match="hr must be"):
        evaluate_sequence(s_model, lr, hr4, batch=2, output_shape=shape)


def test_evaluate_sequence_output_shape_niqe_sees_the_resized_frames(s_model, golden_dir):
    """24 x 48 LR, delivered at 96 x 200: NIQE's size check and its features see the resized frames."""
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.harness.niqe import NiqeModel, frame_niqe
    niqe = NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    lr, hr = torch.from_numpy(_input((2, 1, 24, 48), "u8", 164)), torch.from_numpy(_input((2, 1, 96, 200), "u8", 165))
    got = evaluate_sequence(s_model, lr, hr, batch=2, output_shape=(96, 200), niqe=niqe, return_frames=True)
    assert np.array_equal(got.niqe, frame_niqe(_dev(got.frames), niqe), equal_nan=True)
    with pytest.raises(ValueError):                           # 90 rows hold no two 96 x 96 blocks: refused before any model pass
        evaluate_sequence(s_model, lr, hr[:, :, :90], batch=2, output_shape=(90, 200), niqe=niqe)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_yuv420_entry_points_write_the_contract_of_the_three_planes(s_model, tmp_path, bit_depth):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.resize import imresize_host
    from fcvsr_amd.harness.yuv import read_yuv420, super_resolve_yuv420, upscale_yuv420, write_yuv420
    N, H, W = 3, 16, 20
    kind = "u8" if bit_depth == 8 else "u16"
    y, u, v = _input((N, H, W), kind, 170), _input((N, H // 2, W // 2), kind, 171), _input((N, H // 2, W // 2), kind, 172)
    src = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv")
    write_yuv420(src, y, u, v)
    plain, none = str(tmp_path / "plain.yuv"), str(tmp_path / "none.yuv")
    super_resolve_yuv420(s_model, src, plain, W, H, bit_depth=bit_depth, batch=2)
    super_resolve_yuv420(s_model, src, none, W, H, bit_depth=bit_depth, batch=2, output_shape=None)
    assert open(plain, "rb").read() == open(none, "rb").read()
    ysr = super_resolve_sequence(s_model, _torch16(y)[:, None], batch=2)[:, 0]
    assert np.array_equal(read_yuv420(plain, 4 * W, 4 * H, bit_depth=bit_depth)[0], ysr)
    elem = 1 if bit_depth == 8 else 2
    for Ho, Wo in ((48, 60), (54, 70)):
        dst, want = str(tmp_path / f"sr_{Wo}x{Ho}.yuv"), str(tmp_path / f"want_{Wo}x{Ho}.yuv")
        stats = super_resolve_yuv420(s_model, src, dst, W, H, bit_depth=bit_depth, batch=2, output_shape=(Ho, Wo))
        assert stats["frames"] == N and stats["out_size"] == (Wo, Ho)
        assert stats["bytes_written"] == os.path.getsize(dst) == N * Ho * Wo * 3 // 2 * elem
        write_yuv420(want, imresize_host(ysr, output_shape=(Ho, Wo), out="int"),
                     *(imresize_host(c, output_shape=(Ho // 2, Wo // 2), out="int") for c in (u, v)))
        assert open(dst, "rb").read() == open(want, "rb").read()
        # the bicubic baseline of the same delivery size: all three planes straight from LR
        stats = upscale_yuv420(src, dst, W, H, bit_depth=bit_depth, batch=2, output_shape=(Ho, Wo))
        assert stats["out_size"] == (Wo, Ho) and stats["bytes_written"] == os.path.getsize(dst) == N * Ho * Wo * 3 // 2 * elem
        assert set(stats) == {"frames", "seconds", "fps", "bytes_read", "bytes_written", "out_size"}
        write_yuv420(want, imresize_host(y, output_shape=(Ho, Wo), out="int"),
                     *(imresize_host(c, output_shape=(Ho // 2, Wo // 2), out="int") for c in (u, v)))
        assert open(dst, "rb").read() == open(want, "rb").read()
    a, b = str(tmp_path / "up_a.yuv"), str(tmp_path / "up_b.yuv")
    upscale_yuv420(src, a, W, H, bit_depth=bit_depth, batch=2)
    upscale_yuv420(src, b, W, H, bit_depth=bit_depth, batch=2, output_shape=None)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_super_resolve_yuv420_rgb_output_shape(tmp_path):
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.colour import ColourSpec, rgb_to_yuv420_host, yuv420_to_rgb_host
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.resize import imresize_host
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    m = FCVSR_SNet()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("FCVSR_SNet"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    spec = ColourSpec()
    N, H, W = 3, 16, 20
    y, u, v = _input((N, H, W), "u8", 180), _input((N, H // 2, W // 2), "u8", 181), _input((N, H // 2, W // 2), "u8", 182)
    src, dst, plain, none = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "out.yuv", "plain.yuv", "none.yuv"))
    write_yuv420(src, y, u, v)
    stats = super_resolve_yuv420_rgb(m, src, dst, W, H, colour=spec, batch=2, output_shape=(54, 70))
    assert stats["out_size"] == (70, 54) and os.path.getsize(dst) == N * 54 * 70 * 3 // 2
    sr = super_resolve_sequence(m, torch.from_numpy(yuv420_to_rgb_host(y, u, v, spec)), batch=2)
    sy, su, sv = rgb_to_yuv420_host(imresize_host(sr, output_shape=(54, 70), out="int"), spec)
    ref = np.concatenate([p[i].ravel() for i in range(N) for p in (sy, su, sv)])
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8), ref)
    super_resolve_yuv420_rgb(m, src, plain, W, H, colour=spec, batch=2)
    super_resolve_yuv420_rgb(m, src, none, W, H, colour=spec, batch=2, output_shape=None)
    assert open(plain, "rb").read() == open(none, "rb").read()
