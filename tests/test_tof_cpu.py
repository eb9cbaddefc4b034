"""CPU: the host contract of tOF (`fcvsr_amd.harness.tof`): the Farneback restatement against answers that need no cv2 - the
polynomial expansion of an exact quadratic, the level counts, integer shifts of a smooth periodic texture - and the sequence rules."""
import numpy as np
import pytest

from fcvsr_amd.harness import tof as T


def texture(H, W, seed):
    """The smooth 8-bit texture: white noise, its spectrum times exp(-(fx^2 + fy^2) / (2 * 0.08^2)), normalised, rounded."""
    n = np.random.default_rng(seed).standard_normal((H, W))
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    t = np.real(np.fft.ifft2(np.fft.fft2(n) * np.exp(-(fx * fx + fy * fy) / (2 * 0.08 ** 2))))
    t = (t - t.min()) / (t.max() - t.min())
    return np.floor(255 * t + 0.5).astype(np.uint8)


def test_poly_exp_of_an_exact_quadratic_returns_its_local_coefficients():
    a, b, c, d, e, f = 3.0, 0.7, -1.3, 0.05, -0.02, 0.03
    h, w = 40, 48
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = a + b * x + c * y + d * x * x + e * y * y + f * x * y
    R = T.poly_exp_host(img)
    assert R.shape == (h, w, 5)
    # around (x0, y0): linear terms b + 2 d x0 + f y0 and c + 2 e y0 + f x0; the quadratic ones do not move
    want = np.stack([c + 2 * e * y + f * x, b + 2 * d * x + f * y, np.full_like(x, e), np.full_like(x, d), np.full_like(x, f)], -1)
    inner = (slice(5, h - 5), slice(5, w - 5))
    assert np.abs(R[inner] - want[inner]).max() <= 1e-9
    # the same quadratic written around pixel (5, 5): [c, b, e, d, f] there, which pins channel order and normalisation
    img0 = a + b * (x - 5) + c * (y - 5) + d * (x - 5) ** 2 + e * (y - 5) ** 2 + f * (x - 5) * (y - 5)
    assert np.abs(T.poly_exp_host(img0)[5, 5] - np.array([c, b, e, d, f])).max() <= 1e-9


@pytest.mark.parametrize("h,w,n", [(256, 272, 4), (128, 128, 3), (75, 101, 2), (40, 48, 1), (63, 64, 1), (720, 1280, 4)])
def test_level_counts(h, w, n):
    assert T.level_count(h, w) == n


def test_level_geometry_rounds_half_even_and_blur_taps():
    assert T.level_geometry(75, 101, 1) == (0.5, 3, (38, 50))           # 37.5 -> 38, 50.5 -> 50
    assert T.level_geometry(256, 272, 3) == (3.5, 19, (32, 34)) and T.level_geometry(256, 272, 2)[:2] == (1.5, 9)
    assert T.level_geometry(40, 48, 0) == (0.0, 3, (40, 48))
    assert T.gaussian_taps(3, 0.0).tolist() == [0.25, 0.5, 0.25]
    g = T.gaussian_taps(9, 1.5)
    assert abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1]) and g.argmax() == 4


@pytest.mark.parametrize("H,W,margin", [(256, 272, 24), (75, 101, 16)])
@pytest.mark.parametrize("shift", [(0, 1), (-2, 3), (5, -4)])
def test_integer_shifts_of_a_smooth_texture_are_recovered(H, W, margin, shift):
    dy, dx = shift
    t = texture(H, W, 1)
    flow = T.farneback_host(t, np.roll(t, (dy, dx), (0, 1)))
    assert flow.shape == (H, W, 2) and flow.dtype == np.float64
    inner = flow[margin:H - margin, margin:W - margin]
    err = max(np.abs(inner[..., 0] - dx).max(), np.abs(inner[..., 1] - dy).max())
    print(f"{H}x{W} shift {shift}: max interior error {err:.5f} px")
    assert err <= 0.02


def test_f32_evaluation_is_close_to_f64_and_inputs_are_read_by_their_type():
    t = texture(75, 101, 1)
    s = np.roll(t, (-2, 3), (0, 1))
    f64, f32 = T.farneback_host(t, s), T.farneback_host(t, s, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - f64).max() < 1e-3
    wide = t.astype(np.uint16) * 4
    big = wide.copy()
    big[wide > 1000] = 60000                                             # read as 1023
    want = T.farneback_host(np.minimum(big, 1023).astype(np.float64), (s.astype(np.uint16) * 4).astype(np.float64))
    assert np.array_equal(T.farneback_host(big, s.astype(np.uint16) * 4), want)
    assert np.array_equal(T.farneback_host(t.astype(np.float32), s.astype(np.float32)), f64)
    with pytest.raises(ValueError):
        T.farneback_host(t.astype(np.int32), s.astype(np.int32))
    with pytest.raises(ValueError):
        T.farneback_host(t, s[:, :-1])
    for kw in ({"levels": 2}, {"winsize": 13}, {"pyr_scale": 0.8}, {"iterations": 1}, {"poly_n": 7}, {"poly_sigma": 1.5}, {"flags": 256}):
        with pytest.raises(ValueError):
            T.farneback_host(t, s, **kw)


def test_matrices_take_both_branches_and_the_border_table():
    rng = np.random.default_rng(3)
    R0, R1 = rng.standard_normal((2, 20, 24, 5))
    flow = rng.standard_normal((20, 24, 2)) * 2
    M, inside = T.matrices_host(R0, R1, flow, return_mask=True)
    assert inside.any() and (~inside).any() and M.shape == (20, 24, 5)
    y, x = np.argwhere(~inside)[0]                                        # the out-of-range rule, by hand, at one pixel
    sc = T.border_scale(20, 24, np.float64)[y, x]
    dx, dy = flow[y, x]
    r4, r5, r6 = R0[y, x, 2], R0[y, x, 3], R0[y, x, 4] * 0.5
    r2, r3 = R0[y, x, 0] * 0.5 + r4 * dy + r6 * dx, R0[y, x, 1] * 0.5 + r6 * dy + r5 * dx
    r2, r3, r4, r5, r6 = (v * sc for v in (r2, r3, r4, r5, r6))
    assert np.allclose(M[y, x], [r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], rtol=1e-13)
    b = T.border_scale(20, 24, np.float64)
    assert b[10, 10] == 1.0 and b[0, 10] == 0.14 and b[2, 10] == 0.4472 and b[0, 0] == 0.14 * 0.14 and b[19, 23] == 0.14 * 0.14
    assert b[5, 5] == 1.0 and b[14, 18] == 1.0 and b[15, 10] == 0.4472


def test_tof_of_a_sequence_against_itself_is_zero_and_the_sequence_rules():
    t = [texture(40, 48, s) for s in (1, 2, 3, 4, 5)]
    assert T.tof_host(t[1], t[1], t[0], t[0]) == 0.0
    pred = np.stack([np.roll(t[0], (0, k), (0, 1)) for k in range(5)])
    true = np.stack([np.roll(t[0], (k % 2, k), (0, 1)) for k in range(5)])
    s = T.sequence_tof_host(pred, true)
    assert s["tof"].shape == (5,) and s["tof"][0] == 0.0 and (s["tof"][1:] > 0).all()
    assert s["tof_mean"] == float(s["tof"].mean()) and s["tof_pairs_mean"] == float(s["tof"][1:].mean())
    assert s["tof"][2] == T.tof_host(pred[2], true[2], pred[1], true[1])
    c = T.sequence_tof_host(pred, true, cuts=[3])
    assert c["tof"][3] == 0.0 and c["tof"][0] == 0.0 and np.array_equal(c["tof"][[1, 2, 4]], s["tof"][[1, 2, 4]])
    assert c["tof_mean"] == float(c["tof"].mean()) and c["tof_pairs_mean"] == float(c["tof"][[1, 2, 4]].mean())
    with pytest.raises(ValueError):
        T.sequence_tof_host(pred, true, cuts=[5])
    with pytest.raises(ValueError):
        T.sequence_tof_host(pred, true[:4])
    csv = T.tof_csv(s).splitlines()
    assert csv[0] == "frame,tof" and len(csv) == 6 and csv[1] == "0,0.0"


def test_epe_is_per_pixel_f32_then_an_f64_mean():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((2, 9, 11, 2)).astype(np.float32)
    d = a - b
    want = np.mean([float(np.sqrt(np.float32(d[i, j, 0] * d[i, j, 0] + d[i, j, 1] * d[i, j, 1]))) for i in range(9) for j in range(11)])
    assert abs(T.epe_host(a, b) - want) <= 1e-15 * want and T.epe_host(a, a) == 0.0


def test_rgb_luma_is_the_y_of_the_metrics():
    from fcvsr_amd.harness.metrics import to_y_channel
    rgb = np.random.default_rng(7).integers(0, 256, (3, 6, 7), dtype=np.uint8)
    want = to_y_channel(rgb[::-1].transpose(1, 2, 0))                      # to_y_channel takes BGR, HWC
    assert np.abs(T.rgb_to_y(rgb) - want).max() < 1e-12
    assert T.rgb_to_y(rgb, np.float32).dtype == np.float32


def test_the_library_declares_the_flow_entry_points():
    import os
    import re
    from fcvsr_amd import hip
    hdr = open(os.path.join(os.path.dirname(hip.__file__), "..", "include", "fcvsr_hip.h")).read()
    for name in ("fcvsr_farneback_scratch_bytes", "fcvsr_farneback_flow", "fcvsr_flow_epe_scratch_bytes", "fcvsr_flow_epe",
                 "fcvsr_flow_level_image", "fcvsr_flow_poly_exp", "fcvsr_flow_matrices", "fcvsr_flow_box_solve"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.SIGNATURES, name
    assert re.search(r"#define FCVSR_ABI_VERSION 2\b", hdr)
    for bad in ({"levels": 2}, {"winsize": 21}):
        with pytest.raises(ValueError):
            hip.farneback_flow(None, None, **bad)                          # the parameters are checked before anything else


def test_reference_runs_gain_the_column_only_with_the_keyword():
    from fcvsr_amd.harness import steps
    from fcvsr_amd.harness.reference import scores_csv
    kw = dict(crop_border=4, baseline=None, bit_depth=8, height=18, width=20)
    with pytest.raises(ValueError, match="needs reference="):
        steps.check_reference(None, "out.yuv", tof=True, **kw)
    assert steps.check_reference(None, "out.yuv", **kw) is None
    plain, with_tof = steps.check_reference("gt.yuv", "out.yuv", **kw), steps.check_reference("gt.yuv", "out.yuv", tof=True, **kw)
    assert (plain.words, with_tof.words) == (4, 5)
    assert steps.check_reference("gt.yuv", "out.yuv", tof=True, **{**kw, "baseline": "bicubic"}).words == 8
    rows = np.zeros((5, 3), dtype=np.int64)                                  # three frames as a group's packed host copy
    rows[:3] = 7
    rows[3] = np.array([0.5, 0.6, 0.7]).view(np.int64)
    rows[4] = np.array([0.0, 0.25, 0.75]).view(np.int64)
    with_tof.starts = [True, False, False]
    with_tof.add(rows.reshape(-1))
    plain.add(rows[:4].reshape(-1))
    s, p = with_tof.stats(), plain.stats()
    assert s["tof"].tolist() == [0.0, 0.25, 0.75] and s["tof_mean"] == 1.0 / 3 and s["tof_pairs_mean"] == 0.5
    assert "tof" not in p and np.array_equal(p["psnr_y"], s["psnr_y"])
    assert scores_csv(p).splitlines()[0] == "frame,psnr_y,psnr_u,psnr_v,psnr_yuv,ssim_y"
    assert scores_csv(s).splitlines()[0] == "frame,psnr_y,psnr_u,psnr_v,psnr_yuv,ssim_y,tof"
    assert scores_csv(s).splitlines()[2].endswith(",0.25") and len(scores_csv(s).splitlines()) == 4
