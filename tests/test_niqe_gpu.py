"""GPU: the NIQE block features of fcvsr_niqe_features against the CPU contract (fcvsr_amd/harness/niqe.py) and the reference's
recorded scores (tests/golden/niqe_cases.npz), every input form of the kernel, bit reproducibility, the device bicubic down-scale, and
the `niqe=` keyword of the sequence scorer and the YUV file-to-file path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9                                              # test_quality_gpu.py: f64 sums that differ only in summation order
SYNTHETIC = ("96x192", "192x288", "200x301", "bar_288x384", "corner_192x192")
ALPHA = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "niqe_cases.npz"))


@pytest.fixture(scope="module")
def model(golden_dir):
    from fcvsr_amd.harness.niqe import NiqeModel
    return NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))


def _sibling(seed):
    """A seeded 192 x 288 plane in the manner of the fixture's synthetic planes: sinusoids plus Gaussian noise, no flat region."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:192, 0:288].astype(np.float64)
    img = 120.0 + 40 * np.sin(rs.uniform(0.02, 0.2) * yy + rs.uniform(0.02, 0.2) * xx) + 25 * np.sin(rs.uniform(0.05, 0.3) * xx)
    return np.clip(np.round(img + rs.normal(0, 6.0, img.shape)), 0, 255).astype(np.uint8)


def _compare(got: np.ndarray, ref: np.ndarray, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[:, ALPHA], ref[:, ALPHA]), what
    err = float(np.max(np.abs(got[~nan] - ref[~nan]) / np.abs(ref[~nan])))
    print(f"{what}: max relative feature difference {err:.3e}")
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=TOL, atol=0, err_msg=str(what))


def _planes(cases):
    out = [(f"syn_{n}", cases[f"syn_{n}"], 0, float(cases[f"syn_{n}_score"])) for n in SYNTHETIC]
    out += [(f"baboon crop {c}", cases["baboon_b"], c, float(cases[f"baboon_score_{c}"])) for c in (0, 6)]
    return out


def test_features_and_scores_of_every_fixture_plane(cases, model):
    from fcvsr_amd.harness.niqe import frame_niqe, frame_niqe_features, niqe_features
    for what, img, crop, ref_score in _planes(cases):
        x = torch.from_numpy(img)[None, None].cuda()
        got = frame_niqe_features(x, model, crop_border=crop)
        again = frame_niqe_features(x, model, crop_border=crop)
        assert got.dtype == torch.float64 and got.is_cuda and got.shape[0] == 1 and got.shape[2] == 36
        assert torch.equal(got.view(torch.int64), again.view(torch.int64)), what      # bit-identical, NaN payloads included
        _compare(got[0].cpu().numpy(), niqe_features(img, model, crop), what)
        score = frame_niqe(x, model, crop_border=crop)
        assert score.shape == (1,) and score.dtype == np.float64
        print(f"{what}: device score {score[0]:.9f}, reference {ref_score:.9f}")
        assert abs(float(score[0]) - ref_score) <= 1.5e-5, what


def test_a_batch_of_three_frames(cases, model):
    from fcvsr_amd.harness.niqe import frame_niqe, frame_niqe_features, niqe_features
    imgs = [cases["syn_192x288"], _sibling(101), _sibling(102)]
    x = torch.from_numpy(np.stack(imgs))[:, None].cuda()
    got = frame_niqe_features(x, model).cpu().numpy()
    assert got.shape == (3, 6, 36)
    for i, img in enumerate(imgs):
        _compare(got[i], niqe_features(img, model), f"batch frame {i}")
    scores = frame_niqe(x, model)
    assert scores.shape == (3,) and abs(scores[0] - float(cases["syn_192x288_score"])) <= 1.5e-5


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_strided_f32_view_quantised_in_the_kernel(cases, model, quantise):
    from fcvsr_amd.harness.niqe import frame_niqe_features, niqe_features
    rs = np.random.RandomState(7)
    img = cases["syn_200x301"].astype(np.float32)
    f = np.clip((img + rs.uniform(0.05, 0.95, img.shape).astype(np.float32)) / np.float32(255.0), 0, 1).astype(np.float32)
    buf = torch.full((1, 1, 208, 304), 0.5, dtype=torch.float32).cuda()
    buf[:, :, :200, :301] = torch.from_numpy(f).cuda()
    view = buf[:, :, :200, :301]
    assert not view.is_contiguous()
    q = np.clip(f, 0, 1) * np.float32(255.0)                        # the kernel's quantisation, on the host
    q = np.rint(q) if quantise == "round" else np.trunc(q)
    assert not np.array_equal(np.rint(np.clip(f, 0, 1) * np.float32(255.0)), np.trunc(np.clip(f, 0, 1) * np.float32(255.0)))
    got = frame_niqe_features(view, model, quantise=quantise)[0].cpu().numpy()
    _compare(got, niqe_features(q.astype(np.uint8), model), f"f32 view, {quantise}")


def test_rgb_frame_scored_on_its_rounded_y(cases, model):
    from fcvsr_amd.harness.metrics import to_y_channel
    from fcvsr_amd.harness.niqe import frame_niqe_features, niqe_features
    rs = np.random.RandomState(8)
    base = cases["syn_192x288"].astype(np.int32)
    rgb = np.clip(np.stack([base + rs.randint(-20, 21, base.shape) for _ in range(3)]), 0, 255).astype(np.uint8)   # (3,H,W) RGB
    y = to_y_channel(rgb[::-1].transpose(1, 2, 0)).round()                                # BGR HWC in, as the reference
    got = frame_niqe_features(torch.from_numpy(rgb)[None].cuda(), model, convert_to="Y")[0].cpu().numpy()
    _compare(got, niqe_features(y, model), "RGB -> Y")
    with pytest.raises(ValueError, match="C must be 1"):
        frame_niqe_features(torch.from_numpy(rgb)[None].cuda(), model)
    with pytest.raises(ValueError, match="at least 2"):
        frame_niqe_features(torch.zeros(1, 1, 96, 191, dtype=torch.uint8).cuda(), model)


def test_device_bicubic_downscale(cases):
    from fcvsr_amd.harness.niqe import bicubic_downscale as contract
    from fcvsr_amd.harness.resize import bicubic_downscale
    for size in ("40x56", "16x16"):
        img = cases[f"rs_{size}"]
        for key, factor in (("half", 2), ("quarter", 4)):
            ref = cases[f"rs_{size}_{key}"]
            got = bicubic_downscale(torch.from_numpy(img)[None, None].cuda(), factor)
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1) + ref.shape
            g = got[0, 0].cpu().numpy().astype(np.float64)
            print(f"{size} 1/{factor}: vs reference {np.abs(g - ref).max():.3e}")
            assert np.abs(g - ref).max() <= 1e-3
            c32 = contract(img, factor).astype(np.float32).astype(np.float64)
            assert np.abs(g - c32).max() <= 2.0 ** -16                       # 1 ulp of f32 at 255
    # f32 planes, a batch with a channel axis, more than one tile in both directions, a partial last tile
    x = np.random.RandomState(9).rand(2, 3, 72, 136).astype(np.float32)
    for factor in (2, 4):
        got = bicubic_downscale(torch.from_numpy(x).cuda(), factor).cpu().numpy()
        assert got.shape == (2, 3, 72 // factor, 136 // factor)
        assert np.abs(got.astype(np.float64) - contract(x, factor)).max() <= 2.0 ** -24
    with pytest.raises(ValueError, match="multiples"):
        bicubic_downscale(torch.zeros(1, 1, 10, 8).cuda(), 4)


def _model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    return m


def test_evaluate_sequence_niqe_keyword(model):
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.harness.niqe import frame_niqe
    m = _model()
    rs = np.random.RandomState(10)
    lr = torch.from_numpy(rs.randint(0, 256, (10, 1, 24, 48)).astype(np.uint8))
    hr = torch.from_numpy(rs.randint(0, 256, (10, 1, 96, 192)).astype(np.uint8))
    plain = evaluate_sequence(m, lr, hr, batch=4)
    off = evaluate_sequence(m, lr, hr, batch=4, niqe=None)
    on = evaluate_sequence(m, lr, hr, batch=4, niqe=model, return_frames=True)
    assert off.niqe is None and off.niqe_mean is None and plain.niqe is None
    for r in (off, on):
        assert np.array_equal(r.psnr, plain.psnr) and np.array_equal(r.ssim, plain.ssim)
    assert on.niqe.shape == (10,) and on.niqe.dtype == np.float64
    ref = frame_niqe(torch.from_numpy(on.frames).cuda(), model)
    assert np.array_equal(on.niqe, ref, equal_nan=True)
    assert on.niqe_mean == float(np.mean(on.niqe))
    # the float path scores the frames it would write: quantised in the kernel
    onf = evaluate_sequence(m, lr.float() / 255, hr, batch=4, niqe=model, return_frames=True)
    assert np.array_equal(onf.niqe, frame_niqe(torch.from_numpy(onf.frames).cuda(), model), equal_nan=True)


def test_super_resolve_yuv420_niqe_keyword(model, tmp_path):
    from fcvsr_amd.harness.niqe import frame_niqe
    from fcvsr_amd.harness.yuv import read_yuv420, super_resolve_yuv420, write_yuv420
    m = _model()
    N, H, W = 6, 24, 48
    rs = np.random.RandomState(11)
    src, a, b = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "plain.yuv", "scored.yuv"))
    write_yuv420(src, rs.randint(0, 256, (N, H, W)).astype(np.uint8), rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8),
                 rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8))
    plain = super_resolve_yuv420(m, src, a, W, H, batch=4)
    scored = super_resolve_yuv420(m, src, b, W, H, batch=4, niqe=model)
    assert "niqe" not in plain and "niqe_mean" not in plain
    assert open(a, "rb").read() == open(b, "rb").read()
    assert scored["niqe"].shape == (N,) and scored["niqe_mean"] == float(np.mean(scored["niqe"]))
    y, _, _ = read_yuv420(b, 4 * W, 4 * H)
    assert np.array_equal(scored["niqe"], frame_niqe(torch.from_numpy(np.ascontiguousarray(y))[:, None].cuda(), model), equal_nan=True)
    with pytest.raises(ValueError, match="8-bit"):
        super_resolve_yuv420(m, src, b, W, H, bit_depth=10, niqe=model)


def test_super_resolve_yuv420_rgb_niqe_keyword(model, tmp_path):
    """The RGB twins' file-to-file path scores the rounded Y of its SR RGB frames before the encode; the written bytes are unchanged."""
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.colour import ColourSpec, i420_planes, yuv420_to_rgb
    from fcvsr_amd.harness.niqe import frame_niqe
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    m = FCVSR_SNet()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("FCVSR_SNet")))
    m = m.cuda()
    N, H, W = 3, 24, 48
    rs = np.random.RandomState(12)
    src, a, b = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "plain.yuv", "scored.yuv"))
    write_yuv420(src, rs.randint(16, 236, (N, H, W)).astype(np.uint8), rs.randint(16, 241, (N, H // 2, W // 2)).astype(np.uint8),
                 rs.randint(16, 241, (N, H // 2, W // 2)).astype(np.uint8))
    plain = super_resolve_yuv420_rgb(m, src, a, W, H, batch=2)
    scored = super_resolve_yuv420_rgb(m, src, b, W, H, batch=2, niqe=model)
    assert "niqe" not in plain and open(a, "rb").read() == open(b, "rb").read()
    assert scored["niqe"].shape == (N,) and scored["niqe_mean"] == float(np.mean(scored["niqe"]))
    frames = torch.from_numpy(np.fromfile(src, dtype=np.uint8).reshape(N, -1)).cuda()
    rgb = yuv420_to_rgb(*i420_planes(frames, H, W), ColourSpec())
    sr = torch.from_numpy(super_resolve_sequence(m, rgb, batch=2)).cuda()                  # the SR RGB frames of the same run
    assert np.array_equal(scored["niqe"], frame_niqe(sr, model, convert_to="Y"), equal_nan=True)
    with pytest.raises(ValueError, match="8-bit"):
        super_resolve_yuv420_rgb(m, src, b, W, H, colour=ColourSpec(bit_depth=10), niqe=model)
