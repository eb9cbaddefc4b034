"""GPU: the BRISQUE features of fcvsr_brisque_features against the CPU contract (fcvsr_amd/harness/brisque.py) and the reference's
recorded scores (tests/golden/brisque_cases.npz), every input form of the kernel, bit reproducibility, the wrap of the four products
over the whole plane, and the `brisque=` keyword of the sequence scorer and the YUV file-to-file paths.  The fixture's shapes are the
smallest that cross the kernels' tile edges (16 x 64 and 32 x 64) and wrap: 48x64, 74x102 (no multiple of a tile, odd halves),
192x288."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9                                              # test_niqe_gpu.TOL: f64 sums that differ only in summation order
PLANES = ("48x64", "74x102", "192x288", "const_48x64", "alt_48x64")
SCORED = ("48x64", "74x102", "192x288")                 # planes whose recorded reference score is a number of all 36 entries


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "brisque_cases.npz"))


@pytest.fixture(scope="module")
def model(cases):
    from fcvsr_amd.harness.brisque import BrisqueModel
    return BrisqueModel(cases["sv"], cases["sv_coef"])


def _compare(got: np.ndarray, ref: np.ndarray, what):
    from fcvsr_amd.harness.brisque import ALPHA
    assert got.shape == ref.shape == (36,) and got.dtype == np.float64, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[list(ALPHA)], ref[list(ALPHA)]), what
    err = float(np.max(np.abs(got[~nan] - ref[~nan]) / np.abs(ref[~nan])))
    print(f"{what}: max relative feature difference {err:.3e}")
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=TOL, atol=0, err_msg=str(what))


def test_features_and_scores_of_every_fixture_plane(cases, model):
    from fcvsr_amd.harness.brisque import brisque_features, frame_brisque, frame_brisque_features
    for name in PLANES:
        img = cases[f"plane_{name}"]
        x = torch.from_numpy(img)[None, None].cuda()
        got = frame_brisque_features(x)
        again = frame_brisque_features(x)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (1, 36)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64)), name      # bit-identical, NaN payloads included
        _compare(got[0].cpu().numpy(), brisque_features(img), name)
        if name in SCORED:
            ref_score = float(cases[f"score_{name}"])
            score = frame_brisque(x, model)
            assert score.shape == (1,) and score.dtype == np.float64
            print(f"{name}: device score {score[0]:.9f}, reference {ref_score:.9f}")
            bound = 4 * float(cases["max_score_diff"]) + float(np.spacing(np.float32(abs(ref_score))))   # test_brisque_cpu's
            assert abs(float(score[0]) - ref_score) <= bound, name
    assert np.isnan(frame_brisque_features(torch.from_numpy(cases["plane_alt_48x64"])[None, None].cuda())[0].cpu().numpy()).sum() == 8


def test_a_batch_of_three_different_planes(cases):
    from fcvsr_amd.harness.brisque import frame_brisque_features
    imgs = [cases["plane_48x64"], cases["plane_alt_48x64"], cases["plane_const_48x64"]]
    x = torch.from_numpy(np.stack(imgs))[:, None].cuda()
    got = frame_brisque_features(x)
    assert tuple(got.shape) == (3, 36)
    for i in range(3):
        single = frame_brisque_features(x[i:i + 1])
        assert torch.equal(got[i:i + 1].view(torch.int64), single.view(torch.int64)), i
    assert not torch.equal(got[0].view(torch.int64), got[1].view(torch.int64))


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_strided_f32_view_quantised_in_the_kernel(cases, quantise):
    from fcvsr_amd.harness.brisque import brisque_features, frame_brisque_features
    rs = np.random.RandomState(7)
    img = cases["plane_74x102"].astype(np.float32)
    f = np.clip((img + rs.uniform(0.05, 0.95, img.shape).astype(np.float32)) / np.float32(255.0), 0, 1).astype(np.float32)
    buf = torch.full((1, 1, 80, 112), 0.5, dtype=torch.float32).cuda()
    buf[:, :, :74, :102] = torch.from_numpy(f).cuda()
    view = buf[:, :, :74, :102]
    assert not view.is_contiguous()
    q = np.clip(f, 0, 1) * np.float32(255.0)                        # the kernel's quantisation, on the host
    assert not np.array_equal(np.rint(q), np.trunc(q))
    q = np.rint(q) if quantise == "round" else np.trunc(q)
    got = frame_brisque_features(view, quantise=quantise)[0].cpu().numpy()
    _compare(got, brisque_features(q.astype(np.uint8)), f"f32 view, {quantise}")


def test_rgb_frame_scored_on_its_integer_yiq_luma(cases, model):
    from fcvsr_amd.harness.brisque import brisque_features, frame_brisque, frame_brisque_features, yiq_luma
    rgb = cases["rgb_74x102"]
    x = torch.from_numpy(rgb)[None].cuda()
    got = frame_brisque_features(x, convert_to="Y")[0].cpu().numpy()
    y = yiq_luma(rgb)
    assert np.array_equal(y, cases["rgb_74x102_luma"])
    _compare(got, brisque_features(y), "RGB -> YIQ luma")
    ref_score = float(cases["score_rgb_74x102"])
    bound = 4 * float(cases["max_score_diff"]) + float(np.spacing(np.float32(abs(ref_score))))
    assert abs(float(frame_brisque(x, model, convert_to="Y")[0]) - ref_score) <= bound
    # rounding ties of the luma, half to even, in the kernel's integers: 28.5 -> 28, 221.5 -> 222
    tie = np.zeros((3, 16, 16), dtype=np.uint8)
    tie[:, :, 8:] = np.array([250, 250, 0], dtype=np.uint8)[:, None, None]
    tie[2, :, :8] = 250
    assert set(np.unique(yiq_luma(tie))) == {28, 222}
    _compare(frame_brisque_features(torch.from_numpy(tie)[None].cuda(), convert_to="Y")[0].cpu().numpy(), brisque_features(yiq_luma(tie)),
             "luma ties")
    with pytest.raises(ValueError, match="C must be 1"):
        frame_brisque_features(x)
    with pytest.raises(ValueError, match="even H and W of at least 16"):
        frame_brisque_features(torch.zeros(1, 1, 16, 15, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="even H and W of at least 16"):
        frame_brisque_features(torch.zeros(1, 1, 14, 16, dtype=torch.uint8).cuda())


def test_products_wrap_over_the_whole_plane(cases):
    """A ramp makes the last row and column differ strongly from the first ones; the four products read across that seam."""
    from fcvsr_amd.harness.brisque import brisque_features, frame_brisque_features
    yy, xx = np.mgrid[0:48, 0:64]
    img = np.clip(cases["plane_48x64"].astype(np.float64) * 0.4 + 2.0 * yy + 1.5 * xx, 0, 255).round().astype(np.uint8)
    assert abs(int(img[0].astype(int).mean()) - int(img[-1].astype(int).mean())) > 60
    ref = brisque_features(img)

    def replicated(m, shift):
        ys = np.clip(np.arange(m.shape[0]) - shift[0], 0, m.shape[0] - 1)
        xs = np.clip(np.arange(m.shape[1]) - shift[1], 0, m.shape[1] - 1)
        return m[np.ix_(ys, xs)]
    other = brisque_features(img, _shifted=replicated)
    rel = np.abs(other - ref) / np.abs(ref)
    print(f"edge-replicated instead of wrapped: max relative change {rel.max():.3e}")
    assert np.array_equal(other[:2], ref[:2]) and rel[2:18].max() > 1e3 * TOL and rel[20:].max() > 1e3 * TOL
    _compare(frame_brisque_features(torch.from_numpy(img)[None, None].cuda())[0].cpu().numpy(), ref, "ramp")


def _model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    return m


def test_evaluate_sequence_brisque_keyword(golden_dir, model):
    from fcvsr_amd.harness.brisque import frame_brisque
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.harness.niqe import NiqeModel
    niqe = NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    m = _model()
    rs = np.random.RandomState(10)
    lr = torch.from_numpy(rs.randint(0, 256, (6, 1, 24, 48)).astype(np.uint8))
    hr = torch.from_numpy(rs.randint(0, 256, (6, 1, 96, 192)).astype(np.uint8))
    plain = evaluate_sequence(m, lr, hr, batch=4, niqe=niqe, baseline="bicubic")
    on = evaluate_sequence(m, lr, hr, batch=4, niqe=niqe, baseline="bicubic", brisque=model, return_frames=True)
    assert plain.brisque is None and plain.brisque_mean is None and plain.baseline_brisque is None
    for k in ("psnr", "ssim", "niqe", "baseline_psnr", "baseline_ssim", "baseline_niqe"):
        assert np.array_equal(getattr(on, k), getattr(plain, k), equal_nan=True), k
    assert on.brisque.shape == (6,) and on.brisque.dtype == np.float64 and on.baseline_brisque.shape == (6,)
    assert np.array_equal(on.brisque, frame_brisque(torch.from_numpy(on.frames).cuda(), model), equal_nan=True)
    assert on.brisque_mean == float(np.mean(on.brisque)) and on.baseline_brisque_mean == float(np.mean(on.baseline_brisque))
    assert not np.array_equal(on.brisque, on.baseline_brisque)
    # the float path scores the frames it would write: quantised in the kernel
    onf = evaluate_sequence(m, lr.float() / 255, hr, batch=4, brisque=model, return_frames=True)
    assert np.array_equal(onf.brisque, frame_brisque(torch.from_numpy(onf.frames).cuda(), model), equal_nan=True)
    with pytest.raises(ValueError, match="8-bit"):
        evaluate_sequence(m, lr.to(torch.uint16), hr.to(torch.uint16), batch=4, brisque=model)
    with pytest.raises(ValueError, match="BrisqueModel"):
        evaluate_sequence(m, lr, hr, batch=4, brisque=niqe)


def test_super_resolve_yuv420_brisque_keyword(model, tmp_path):
    from fcvsr_amd.harness.brisque import frame_brisque
    from fcvsr_amd.harness.yuv import read_yuv420, super_resolve_yuv420, write_yuv420
    m = _model()
    N, H, W = 5, 24, 48
    rs = np.random.RandomState(11)
    src, a, b = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "plain.yuv", "scored.yuv"))
    write_yuv420(src, rs.randint(0, 256, (N, H, W)).astype(np.uint8), rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8),
                 rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8))
    plain = super_resolve_yuv420(m, src, a, W, H, batch=4)
    scored = super_resolve_yuv420(m, src, b, W, H, batch=4, brisque=model)
    assert "brisque" not in plain and "brisque_mean" not in plain and "niqe" not in scored
    assert open(a, "rb").read() == open(b, "rb").read()
    assert scored["brisque"].shape == (N,) and scored["brisque_mean"] == float(np.mean(scored["brisque"]))
    y, _, _ = read_yuv420(b, 4 * W, 4 * H)
    ref = frame_brisque(torch.from_numpy(np.ascontiguousarray(y))[:, None].cuda(), model)
    assert np.array_equal(scored["brisque"], ref, equal_nan=True)
    with pytest.raises(ValueError, match="8-bit"):
        super_resolve_yuv420(m, src, b, W, H, bit_depth=10, brisque=model)


def test_super_resolve_yuv420_rgb_brisque_keyword(model, tmp_path):
    """The RGB twins' file-to-file path scores the YIQ luma of its SR RGB frames before the encode; the written bytes are unchanged."""
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.brisque import frame_brisque
    from fcvsr_amd.harness.colour import ColourSpec, i420_planes, yuv420_to_rgb
    from fcvsr_amd.harness.infer import super_resolve_sequence
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
    scored = super_resolve_yuv420_rgb(m, src, b, W, H, batch=2, brisque=model)
    assert "brisque" not in plain and open(a, "rb").read() == open(b, "rb").read()
    assert scored["brisque"].shape == (N,) and scored["brisque_mean"] == float(np.mean(scored["brisque"]))
    frames = torch.from_numpy(np.fromfile(src, dtype=np.uint8).reshape(N, -1)).cuda()
    rgb = yuv420_to_rgb(*i420_planes(frames, H, W), ColourSpec())
    sr = torch.from_numpy(super_resolve_sequence(m, rgb, batch=2)).cuda()                  # the SR RGB frames of the same run
    assert np.array_equal(scored["brisque"], frame_brisque(sr, model, convert_to="Y"), equal_nan=True)
    with pytest.raises(ValueError, match="8-bit"):
        super_resolve_yuv420_rgb(m, src, b, W, H, colour=ColourSpec(bit_depth=10), brisque=model)
