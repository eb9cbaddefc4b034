"""Host: the NIQE contract (fcvsr_amd/harness/niqe.py) against the reference's published known answers and its recorded features and
scores (tests/golden/niqe_cases.npz, made by tests/golden/make_golden_niqe.py with the pristine model niqe_pris_params.npz), the
bicubic down-scale against the reference's recorded outputs, the error cases, and the C ABI / binding of the two new entry points."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("fcvsr_niqe_scratch_bytes", "fcvsr_niqe_features", "fcvsr_bicubic_downscale")
SYNTHETIC = ("96x192", "192x288", "200x301", "bar_288x384", "corner_192x192")
ALPHA = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]          # the alpha entries of the 36 features


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "niqe_cases.npz"))


@pytest.fixture(scope="module")
def model(golden_dir):
    from fcvsr_amd.harness.niqe import NiqeModel
    return NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))


def test_published_known_answers_on_the_baboon_plane(cases, model):
    """Reference tests/test_metrics/test_metrics.py:110-111, :129-130: 5.62525 and 5.82981 on the blue channel, crop_border 0 and 6.
    The reference's niqe() casts its input to float32 before anything else, and the published figures contain that path's f32
    roundings; the plane goes in as float32 here as it does there.  (The same plane as uint8 or f64 is scored in f64: next test.)"""
    from fcvsr_amd.harness.niqe import niqe
    plane = cases["baboon_b"].astype(np.float32)
    got0, got6 = niqe(plane, model), niqe(plane, model, crop_border=6)
    print(f"baboon: crop_border 0 -> {got0:.6f} (published 5.62525), crop_border 6 -> {got6:.6f} (published 5.82981)")
    np.testing.assert_almost_equal(got0, 5.62525, decimal=5)
    np.testing.assert_almost_equal(got6, 5.82981, decimal=5)


def test_baboon_plane_matches_the_reference_in_f64(cases, model):
    from fcvsr_amd.harness.niqe import niqe
    for crop in (0, 6):
        got, ref = niqe(cases["baboon_b"], model, crop_border=crop), float(cases[f"baboon_score_{crop}"])
        print(f"baboon crop_border={crop}: contract {got:.9f}, reference niqe_core on the f64 plane {ref:.9f}")
        assert abs(got - ref) <= 1.5e-5


@pytest.mark.parametrize("name", SYNTHETIC)
def test_synthetic_features_and_scores_match_the_reference(cases, model, name):
    from fcvsr_amd.harness.niqe import niqe_features, niqe_score
    img, ref, ref_score = cases[f"syn_{name}"], cases[f"syn_{name}_features"], float(cases[f"syn_{name}_score"])
    got = niqe_features(img, model)
    assert got.shape == ref.shape and got.dtype == np.float64
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    if name.startswith(("bar", "corner")):
        assert nan.any() and not nan[:, ALPHA].any()             # black blocks: NaN betas, alpha 0.2 from argmin over NaN
        assert (ref[nan.any(axis=1)][:, ALPHA] == 0.2).any()
    assert np.array_equal(got[:, ALPHA], ref[:, ALPHA])           # alpha on every block, the 0.2 of the NaN blocks included
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=1e-6, atol=0)
    score = niqe_score(got, model)
    print(f"{name}: contract {score:.9f}, reference {ref_score:.9f}")
    assert np.isfinite(score) and abs(score - ref_score) <= 1.5e-5


@pytest.mark.parametrize("size", ["40x56", "16x16"])
def test_bicubic_downscale_matches_the_reference(cases, size):
    """|d| <= 1e-3 on the 0..255 scale: two passes, each at most 17 f32 roundings of 2^-24 relative on terms bounded by
    sum|w| * 255 ~ 357, i.e. 7.2e-4.  (The contract mirrors the reference's f32 order, so the difference is in fact 0.)"""
    from fcvsr_amd.harness.niqe import bicubic_downscale
    img = cases[f"rs_{size}"]
    for key, factor in (("half", 2), ("quarter", 4)):
        got, ref = bicubic_downscale(img, factor), cases[f"rs_{size}_{key}"]
        assert got.shape == ref.shape == (img.shape[0] // factor, img.shape[1] // factor)
        err = float(np.abs(got - ref).max())
        print(f"{size} 1/{factor}: max-abs {err:.3e}")
        assert err <= 1e-3
    batch = np.stack([img, img[::-1]])                             # leading axes are batch axes
    assert np.array_equal(bicubic_downscale(batch, 2)[1], bicubic_downscale(img[::-1], 2))


def test_taps_are_the_normalised_antialiased_cubic():
    from fcvsr_amd.harness import niqe as nq

    def cubic(x):
        x = np.abs(x)
        return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x <= 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))

    for f, denom in ((2, 256), (4, 4096)):
        d = np.arange(2 * f - 0.5, -2 * f, -1.0)
        w = cubic(d / f) / f
        assert np.allclose(nq._TAPS[f], w / w.sum(), rtol=0, atol=1e-15)
        assert np.array_equal(nq._TAPS[f] * denom, np.round(nq._TAPS[f] * denom)) and nq._TAPS[f].sum() == 1.0
        assert np.array_equal(nq._TAPS[f].astype(np.float32).astype(np.float64), nq._TAPS[f])     # exact in f32


def test_error_cases(cases, model):
    from fcvsr_amd.harness.niqe import NiqeModel, bicubic_downscale, niqe, niqe_features, niqe_score
    img = cases["syn_96x192"]
    with pytest.raises(ValueError, match="at least 2"):
        niqe(img[:, :191], model)                                  # one block
    with pytest.raises(ValueError, match="at least 2"):
        niqe(img, model, crop_border=1)
    with pytest.raises(ValueError, match="8-bit"):
        niqe(img.astype(np.uint16), model)
    with pytest.raises(ValueError, match="8-bit"):
        niqe_features(img.astype(np.uint16), model)
    with pytest.raises(ValueError):
        niqe(img[None], model)
    with pytest.raises(ValueError, match="crop_border"):
        niqe(img, model, crop_border=-1)
    with pytest.raises(ValueError, match="NiqeModel"):
        niqe(img, (model.mu, model.cov, model.window))
    for bad in ((model.mu[:35], model.cov, model.window), (model.mu, model.cov[:35], model.window),
                (model.mu, model.cov, model.window[:5, :5]), (model.mu, model.cov.reshape(-1), model.window)):
        with pytest.raises(ValueError, match="shape"):
            NiqeModel(*bad)
    with pytest.raises(ValueError):
        niqe_score(np.zeros((1, 36)), model)
    with pytest.raises(ValueError):
        niqe_score(np.zeros((4, 18)), model)
    for bad_factor in (1, 3, 8, 2.5):
        with pytest.raises(ValueError, match="factor"):
            bicubic_downscale(np.zeros((8, 8)), bad_factor)
    with pytest.raises(ValueError, match="multiples"):
        bicubic_downscale(np.zeros((8, 6)), 4)


def test_model_load_round_trips_the_fixture(golden_dir, model, tmp_path):
    from fcvsr_amd.harness.niqe import NiqeModel
    raw = np.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    assert model.mu.shape == (36,) and model.cov.shape == (36, 36) and model.window.shape == (7, 7)
    assert np.array_equal(model.mu, raw["mu_pris_param"].reshape(36)) and np.array_equal(model.cov, raw["cov_pris_param"])
    assert np.array_equal(model.window, raw["gaussian_window"])
    path = str(tmp_path / "again.npz")
    np.savez(path, mu_pris_param=model.mu, cov_pris_param=model.cov, gaussian_window=model.window)
    again = NiqeModel.load(path)
    assert all(np.array_equal(getattr(again, k), getattr(model, k)) for k in ("mu", "cov", "window"))


def test_no_product_module_reads_the_tests_directory():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "fcvsr_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "niqe_pris_params" not in open(os.path.join(dirpath, f)).read().replace(
                    "mmedit/core/evaluation/niqe_pris_params.npz", ""), f


def test_new_symbols_are_declared_bound_and_exported_at_abi_version_2():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"#define\s+FCVSR_ABI_VERSION\s+2\b", hdr)
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
        assert name in hip.SIGNATURES, f"{name} has no row in hip.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES["fcvsr_niqe_scratch_bytes"]) == 4
    assert len(hip.SIGNATURES["fcvsr_niqe_features"]) == 15
    assert len(hip.SIGNATURES["fcvsr_bicubic_downscale"]) == 8
    assert hip.lib().fcvsr_abi_version() == 2
    assert callable(hip.niqe_features) and callable(hip.bicubic_downscale)
    # the scratch size is the 2.5 f64 planes of the scored region; 0 for nonsense
    assert hip.lib().fcvsr_niqe_scratch_bytes(3, 200, 301, 0) == 3 * 192 * 288 * 8 * 5 // 2
    assert hip.lib().fcvsr_niqe_scratch_bytes(1, 480, 500, 6) == 384 * 480 * 8 * 5 // 2
    assert hip.lib().fcvsr_niqe_scratch_bytes(0, 200, 301, 0) == 0


def test_harness_keywords_default_to_none_and_host_tensors_raise(model):
    import torch
    from fcvsr_amd.harness.infer import SequenceScores, evaluate_sequence
    from fcvsr_amd.harness.niqe import frame_niqe, frame_niqe_features
    from fcvsr_amd.harness.resize import bicubic_downscale
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    for fn in (evaluate_sequence, super_resolve_yuv420, super_resolve_yuv420_rgb):
        assert inspect.signature(fn).parameters["niqe"].default is None
    for fn in (frame_niqe, frame_niqe_features):
        p = inspect.signature(fn).parameters
        assert p["crop_border"].default == 0 and p["quantise"].default is None and p["convert_to"].default is None
    s = SequenceScores(np.zeros(1), np.zeros(1), 0.0, 0.0)
    assert s.frames is None and s.niqe is None and s.niqe_mean is None
    assert [f.name for f in SequenceScores.__dataclass_fields__.values()][-2:] == ["niqe", "niqe_mean"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frame_niqe(torch.zeros(1, 1, 96, 192, dtype=torch.uint8), model)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bicubic_downscale(torch.zeros(1, 1, 8, 8), 2)
    with pytest.raises(ValueError, match="8-bit"):
        frame_niqe(torch.zeros(1, 1, 96, 192, dtype=torch.uint16), model)
    with pytest.raises(ValueError, match="quantise"):
        frame_niqe(torch.zeros(1, 1, 96, 192, dtype=torch.uint8), model, quantise="floor")
    with pytest.raises(ValueError, match="8-bit"):                 # 10-bit runs with niqe= raise before anything is read
        super_resolve_yuv420(object(), "absent_48x24.yuv", "absent.out", 48, 24, bit_depth=10, niqe=model)
    with pytest.raises(ValueError, match="8-bit"):
        evaluate_sequence(object(), torch.zeros(2, 1, 24, 48), torch.zeros(2, 1, 96, 192, dtype=torch.uint16), niqe=model)
