"""CPU: the BRISQUE contract (fcvsr_amd/harness/brisque.py) against the reference's recorded features and scores
(tests/golden/brisque_cases.npz, written by tests/golden/make_golden_brisque.py), the regressor's file forms, the range scaling and
the argument checks.

The bounds come from the fixture: the generator measured the largest difference between contract (f64) and reference (f32 torch)
in scaled-feature units (`max_scaled_diff`) and in the score (`max_score_diff`); the reference's f32 sums change with torch's thread
count and version, hence the factor 4.  Features are compared in scaled units: relative error means nothing for eta, a difference of
near-equal numbers.

The constant-128 plane: the reference's f32 has no negative product there and NaN AGGD entries; in the contract's f64 the window's
f32 taps sum to 1 + 1.1e-8, the interior MSCN is -1.4e-6 and every entry is finite (make_golden_brisque.py has the figures).  Only
the entries the fixture lists as comparable (the two GGD fits) are held to the reference; the checkerboard plane `alt_48x64`, whose
empty sides are empty in exact arithmetic, pins the NaN pattern."""
import os

import numpy as np
import pytest

FULL = ("48x64", "74x102", "192x288", "alt_48x64")              # planes whose 36 entries are all comparable


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "brisque_cases.npz"))


@pytest.fixture(scope="module")
def model(cases):
    from fcvsr_amd.harness.brisque import BrisqueModel
    return BrisqueModel(cases["sv"], cases["sv_coef"])


def _plane(cases, name):
    from fcvsr_amd.harness.brisque import yiq_luma
    return yiq_luma(cases[name]) if name.startswith("rgb") else cases[f"plane_{name}"]


def _score_bound(cases, score):
    return 4 * float(cases["max_score_diff"]) + float(np.spacing(np.float32(abs(score))))


@pytest.mark.parametrize("name", FULL + ("rgb_74x102",))
def test_contract_against_the_reference(cases, model, name):
    from fcvsr_amd.harness.brisque import ALPHA, brisque_features, brisque_score, scale_features
    got, ref = brisque_features(_plane(cases, name)), cases[f"feat_{name}"]
    assert got.shape == (36,) and got.dtype == np.float64
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    a = list(ALPHA)
    assert np.array_equal(np.rint((got[a] - 0.2) / 0.001), np.rint((ref[a] - 0.2) / 0.001))      # ref holds f32(g)
    d = np.abs(scale_features(got)[~nan] - scale_features(ref)[~nan]).max()
    print(f"{name}: scaled-feature difference {d:.3e} (recorded maximum {float(cases['max_scaled_diff']):.3e})")
    assert d <= 4 * float(cases["max_scaled_diff"])
    ref_score = float(cases[f"score_{name}"])
    score = brisque_score(got, model)
    if np.isnan(ref_score):
        assert np.isnan(score) and nan.any()
    else:
        print(f"{name}: score {score:.9f}, reference {ref_score:.9f}")
        assert abs(score - ref_score) <= _score_bound(cases, ref_score)


def test_nan_pattern_of_the_checkerboard_plane(cases):
    """H and V products have no positive sample (eta, sigma_r^2 NaN), the diagonal ones no negative sample (eta, sigma_l^2 NaN);
    alpha is the grid's first entry; scale 2 is finite."""
    from fcvsr_amd.harness.brisque import brisque_features
    f = brisque_features(cases["plane_alt_48x64"])
    assert np.array_equal(np.flatnonzero(np.isnan(f)), [3, 5, 7, 9, 11, 12, 15, 16])
    assert np.array_equal(f[[2, 6, 10, 14]], [0.2] * 4)
    assert np.array_equal(np.isnan(f), np.isnan(cases["feat_alt_48x64"]))


def test_constant_plane_ggd_entries(cases):
    from fcvsr_amd.harness.brisque import brisque_features, scale_features
    got, ref = brisque_features(cases["plane_const_48x64"]), cases["feat_const_48x64"]
    keep = cases["const_48x64_comparable"]
    assert np.array_equal(keep, [0, 1, 18, 19])
    assert np.array_equal(np.rint((got[[0, 18]] - 0.2) / 0.001), np.rint((ref[[0, 18]] - 0.2) / 0.001))
    assert np.abs(scale_features(got)[keep] - scale_features(ref)[keep]).max() <= 4 * float(cases["max_scaled_diff"])


def test_rgb_luma_is_the_references(cases):
    from fcvsr_amd.harness.brisque import yiq_luma
    rgb = cases["rgb_74x102"]
    y = yiq_luma(rgb)
    assert y.dtype == np.uint8 and np.array_equal(y, cases["rgb_74x102_luma"])
    v = 299 * rgb[0].astype(np.int64) + 587 * rgb[1].astype(np.int64) + 114 * rgb[2].astype(np.int64)
    assert not (v % 1000 == 500).any()
    # ties round half to even: (0,0,250) -> 28500 / 1000 = 28.5 -> 28; (250,250,0) -> 221500 / 1000 = 221.5 -> 222
    px = lambda r, g, b: np.array([[[r]], [[g]], [[b]]], dtype=np.uint8)
    assert yiq_luma(px(0, 0, 250))[0, 0] == 28 and yiq_luma(px(250, 250, 0))[0, 0] == 222
    assert yiq_luma(px(1, 1, 1))[0, 0] == 1 and yiq_luma(px(255, 255, 255))[0, 0] == 255 and yiq_luma(px(0, 0, 5))[0, 0] == 1


def test_tables_and_window():
    import math
    from fcvsr_amd.harness.brisque import GAM, brisque_tables, gaussian_window
    t = brisque_tables()
    assert t.shape == (4, 9801) and t.dtype == np.float64 and not t.flags.writeable and brisque_tables() is t
    assert np.array_equal(t[3], GAM)
    for i in (0, 1800, 9800):
        g = GAM[i]
        l1, l2, l3 = math.lgamma(1 / g), math.lgamma(2 / g), math.lgamma(3 / g)
        assert t[0, i] == math.exp(l1 + l3 - 2 * l2) and t[1, i] == math.exp(2 * l2 - (l1 + l3))
        assert t[2, i] == math.exp(l2 - (l1 + l3) / 2)
    assert abs(t[0, 1800] - math.pi / 2) < 1e-9                                         # g = 2, a Gaussian: rho = pi / 2
    w = gaussian_window()
    assert w.shape == (7, 7) and np.array_equal(w, w.astype(np.float32).astype(np.float64))
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1]) and abs(w.sum() - 1) < 1e-6


def test_model_validates_and_loads_both_file_forms(tmp_path):
    import torch
    from fcvsr_amd.harness.brisque import BrisqueModel
    rs = np.random.RandomState(1)
    sv, coef = rs.uniform(-1, 1, (5, 36)), rs.normal(0, 1, 5)
    m = BrisqueModel(sv, coef)
    assert m.sv.shape == (5, 36) and m.sv_coef.shape == (5,) and m.sv.dtype == np.float64
    assert BrisqueModel(sv, coef[:, None]).sv_coef.shape == (5,)
    for bad_sv, bad_coef in ((sv.T, coef), (sv[:, :35], coef), (sv, coef[:4]), (sv[0], coef), (sv, np.zeros((5, 2)))):
        with pytest.raises(ValueError, match="BrisqueModel"):
            BrisqueModel(bad_sv, bad_coef)
    for k, arr in enumerate((sv, sv.T)):                                                 # (n,36) and (36,n)
        pth, npz = str(tmp_path / f"w{k}.pth"), str(tmp_path / f"w{k}.npz")
        torch.save((torch.from_numpy(coef), torch.from_numpy(np.ascontiguousarray(arr))), pth)
        np.savez(npz, sv_coef=coef, sv=arr)
        for path in (pth, npz):
            got = BrisqueModel.load(path)
            assert np.array_equal(got.sv, sv) and np.array_equal(got.sv_coef, coef)
    torch.save({"sv": 1}, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match="pair"):
        BrisqueModel.load(str(tmp_path / "bad.pth"))


def test_scaling_and_score_closed_form():
    from fcvsr_amd.harness.brisque import FEATURE_RANGES, BrisqueModel, brisque_score, scale_features
    assert FEATURE_RANGES.shape == (36, 2)
    assert np.array_equal(scale_features(FEATURE_RANGES[:, 0]), np.full(36, -1.0))
    assert np.array_equal(scale_features(FEATURE_RANGES[:, 1]), np.full(36, 1.0))
    mid = FEATURE_RANGES.mean(axis=1)
    np.testing.assert_allclose(scale_features(mid), 0.0, atol=1e-15)
    with pytest.raises(ValueError, match="36"):
        scale_features(np.zeros(35))
    # one support vector at the origin of the scaled space, scored at the upper bounds: ||1 - 0||^2 = 36
    one = BrisqueModel(np.zeros((1, 36)), np.array([2.5]))
    assert brisque_score(FEATURE_RANGES[:, 1], one) == pytest.approx(2.5 * np.exp(-0.05 * 36.0) + 153.591, rel=1e-15)
    assert brisque_score(mid, one) == pytest.approx(2.5 + 153.591, rel=1e-15)
    with pytest.raises(ValueError, match="BrisqueModel"):
        brisque_score(mid, (np.zeros((1, 36)), np.array([1.0])))
    with pytest.raises(ValueError, match=r"\(36,\)"):
        brisque_score(np.zeros((2, 36)), one)


def test_brisque_is_the_composition(cases, model):
    from fcvsr_amd.harness.brisque import brisque, brisque_features, brisque_score, scores_from_features
    y = cases["plane_48x64"]
    f = brisque_features(y)
    assert brisque(y, model) == brisque_score(f, model)
    assert np.array_equal(brisque_features(y.astype(np.float64)), f) and np.array_equal(brisque_features(y.astype(np.float32)), f)
    s = scores_from_features(np.stack([f, f]), model)
    assert s.shape == (2,) and s.dtype == np.float64 and s[0] == s[1] == brisque(y, model)


def test_errors(cases, model):
    from fcvsr_amd.harness.brisque import brisque_features, scores_from_features
    y = cases["plane_48x64"]
    for bad in (y[:47], y[:, :63], y[:14], y[:, :14]):
        with pytest.raises(ValueError, match="even H and W of at least 16"):
            brisque_features(bad)
    with pytest.raises(ValueError, match="8-bit"):
        brisque_features(y.astype(np.uint16))
    with pytest.raises(ValueError, match=r"\(H,W\) plane"):
        brisque_features(np.stack([y, y]))
    with pytest.raises(ValueError, match="non-zero variance"):
        brisque_features(np.zeros((16, 16), dtype=np.uint8))
    f = np.zeros((1, 36))
    with pytest.raises(ValueError, match="non-zero variance"):                         # the device path's host half
        scores_from_features(f, model)


def test_device_functions_refuse_host_tensors_and_bad_arguments():
    import torch
    from fcvsr_amd.harness.brisque import frame_brisque_features
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frame_brisque_features(torch.zeros(1, 1, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="8-bit"):
        frame_brisque_features(torch.zeros(1, 1, 16, 16, dtype=torch.uint16))
    with pytest.raises(ValueError, match="quantise"):
        frame_brisque_features(torch.zeros(1, 1, 16, 16, dtype=torch.uint8), quantise="floor")
    with pytest.raises(ValueError, match="color model"):
        frame_brisque_features(torch.zeros(1, 3, 16, 16, dtype=torch.uint8), convert_to="ycbcr")
    with pytest.raises(TypeError):
        frame_brisque_features(np.zeros((1, 1, 16, 16), dtype=np.uint8))


def test_keywords_are_off_by_default():
    import inspect
    from fcvsr_amd.harness.infer import SequenceScores, evaluate_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    for fn in (evaluate_sequence, super_resolve_yuv420, super_resolve_yuv420_rgb):
        assert inspect.signature(fn).parameters["brisque"].default is None
    s = SequenceScores(np.zeros(1), np.zeros(1), 0.0, 0.0)
    assert s.brisque is None and s.brisque_mean is None and s.baseline_brisque is None and s.baseline_brisque_mean is None
    s.brisque = np.ones(1)
    assert SequenceScores(np.zeros(1), np.zeros(1), 0.0, 0.0).brisque is None          # set per instance
