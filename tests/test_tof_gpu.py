"""GPU: the flow kernels of csrc/flow.hip against the host contract `fcvsr_amd.harness.tof`, stage by stage and as a whole, and tOF
through the harness.

One tolerance rule throughout (the polynomial expansion excepted, which has the per-element bound of tests/tolerance.py): with
``e32 = max|host(float32) - host(float64)|`` on the same inputs, computed here, a kernel passes with
``max|gpu - host64| <= 4 e32 + 2^-20 max|host64|`` over all pixels.  The kernels evaluate the host's f32 expression tree, so their
error is that of the f32 host evaluation; 4 covers another summation order of the same tree.

Measured on an MI355X (every case is printed by the test; the full table is in profiles/NOTES.md): in every case the kernel's
error EQUALS e32 to the digits printed, i.e. the kernels reproduce the host's f32 evaluation, and the factor 4 is not used up.
  max|gpu - host64| = e32, px (or samples)        level images 75x101: u8 0 / 1.9e-4 / 8.7e-5 / 5.6e-5 (levels 0..3),
  u16 0 / 7.6e-4 / 3.4e-4 / 2.2e-4, f32 1.9e-6 / 2.6e-5 / 1.0e-5 / 6.9e-6, RGB level 1 1.3e-4; matrices 1.7e-4 (max|M| 203);
  box_solve 3.0e-6; poly_exp worst ratio 2.1e-7 (bound 1.5e-5)
  whole flow (shift / texture 1 against 2 / shift): 256x272 7.0e-6 / 4.5e-4 / 4.9e-6; 75x101 u8 3.1e-6 / 2.3e-5 / 3.2e-6,
  u16 3.2e-6 / 2.0e-5 / 2.4e-6, f32 2.3e-6 / 7.0e-6 / 1.6e-6; 40x48 2.7e-6 / 4.1e-6 / 2.4e-6; 33x300 1.2e-5 / 2.3e-5 / 6.6e-6
  tOF values: frame_tof 1.0e-7, evaluate_sequence 7.7e-8 (4.4e-8 with cuts), streamed 7.5e-7 (8 bit) / 1.0e-7 (10 bit)
"""
import functools

import numpy as np
import pytest
import torch

from fcvsr_amd import hip
from fcvsr_amd.harness import tof as T
from tolerance import tau, worst_ratio

pytestmark = pytest.mark.gpu

SHIFT = (-2, 3)


def texture(H, W, seed):
    n = np.random.default_rng(seed).standard_normal((H, W))
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    t = np.real(np.fft.ifft2(np.fft.fft2(n) * np.exp(-(fx * fx + fy * fy) / (2 * 0.08 ** 2))))
    t = (t - t.min()) / (t.max() - t.min())
    return np.floor(255 * t + 0.5).astype(np.uint8)


def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def _as(kind, t8):
    """The 8-bit texture as the input type `kind`: uint16 is 4 x the samples with the brightest pushed beyond 1023."""
    if kind == "u8":
        return t8
    if kind == "u16":
        a = t8.astype(np.uint16) * 4
        a[t8 >= 250] = t8[t8 >= 250].astype(np.uint16) + 40000
        return a
    return (t8.astype(np.float32) - 100.5) / 7


def _check(what, got, h64, h32):
    """The rule: prints the figures, then asserts."""
    got, h64 = np.asarray(got, dtype=np.float64), np.asarray(h64, dtype=np.float64)
    e32 = float(np.abs(np.asarray(h32, dtype=np.float64) - h64).max())
    err = float(np.abs(got - h64).max())
    tol = 4 * e32 + 2.0 ** -20 * float(np.abs(h64).max())
    print(f"TOF {what}: gpu err {err:.3e}  e32 {e32:.3e}  tol {tol:.3e}  max|ref| {np.abs(h64).max():.3e}")
    assert got.shape == h64.shape and np.isfinite(got).all()
    assert err <= tol, (what, err, e32, tol)


@functools.lru_cache(maxsize=None)
def _stage_inputs():
    """75x101: the level-0 image of texture 1 and of its shift (f32), their host expansions and a random flow."""
    t = texture(75, 101, 1)
    imgs = [T.level_image_host(T.read_plane(p, np.float32), 75, 101, 0, np.float32) for p in (t, np.roll(t, SHIFT, (0, 1)))]
    R = [T.poly_exp_host(i) for i in imgs]
    flow = (np.random.default_rng(11).standard_normal((75, 101, 2)) * 2).astype(np.float32)
    return imgs, R, flow


def _pad8(R):
    return np.concatenate([R, np.zeros(R.shape[:-1] + (3,), R.dtype)], -1)


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_level_images(kind):
    src = _as(kind, texture(75, 101, 1))
    if kind == "u16":
        assert (src > 1023).any()
    planes = np.stack([src, np.roll(src, SHIFT, (0, 1))])
    for level in range(4):
        got = hip.flow_level_image(_dev(planes), level).cpu().numpy()
        h64 = np.stack([T.level_image_host(T.read_plane(p), 75, 101, level) for p in planes])
        h32 = np.stack([T.level_image_host(T.read_plane(p, np.float32), 75, 101, level, np.float32) for p in planes])
        assert got.shape == (2,) + T.level_geometry(75, 101, level)[2]
        _check(f"level_image {kind} level {level}", got, h64, h32)


def test_level_image_of_rgb_is_the_level_image_of_its_luma():
    rgb = np.stack([texture(75, 101, s) for s in (1, 2, 3)])
    got = hip.flow_level_image(_dev(rgb[None]), 1, rgb=True).cpu().numpy()[0]
    _check("level_image rgb level 1", got, T.level_image_host(T.rgb_to_y(rgb), 75, 101, 1),
           T.level_image_host(T.rgb_to_y(rgb, np.float32), 75, 101, 1, np.float32))


def test_poly_exp_per_element():
    imgs, _, _ = _stage_inputs()
    got = hip.flow_poly_exp(_dev(np.stack(imgs))).cpu()
    assert got.shape == (2, 75, 101, 8) and (got[..., 5:] == 0).all()
    ref = np.stack([T.poly_exp_host(i.astype(np.float64)) for i in imgs])
    S = np.stack([T.poly_exp_condition(i) for i in imgs])
    r = worst_ratio(got[..., :5], torch.from_numpy(ref), torch.from_numpy(S))
    print(f"TOF poly_exp: worst |err| / sum|tap products| {r:.3e}  bound {tau(121):.3e}")
    assert r <= tau(121)                                                   # 121 taps behind every element


def test_matrices_from_a_given_flow():
    _, R, flow = _stage_inputs()
    h64, inside = T.matrices_host(R[0].astype(np.float64), R[1].astype(np.float64), flow.astype(np.float64), return_mask=True)
    assert inside.any() and (~inside).any()                                # both branches; the border table covers 5 pixels a side
    h32 = T.matrices_host(R[0], R[1], flow)
    got = hip.flow_matrices(_dev(_pad8(R[0])[None]), _dev(_pad8(R[1])[None]), _dev(flow[None])).cpu().numpy()[0]
    _check("matrices", got.transpose(1, 2, 0), h64, h32)


def test_one_blur_and_solve_from_a_given_m():
    _, R, flow = _stage_inputs()
    M = T.matrices_host(R[0], R[1], flow)
    got = hip.flow_box_solve(_dev(np.ascontiguousarray(M.transpose(2, 0, 1))[None])).cpu().numpy()[0]
    _check("box_solve", got, T.box_solve_host(M.astype(np.float64)), T.box_solve_host(M))


@functools.lru_cache(maxsize=None)
def _flow_case(H, W, kind):
    """The 4-plane buffer [s, t1, t2, roll(t2)] with t1 = roll(s): pairs (shift, texture 1 against texture 2, shift), and the
    host flows of the three pairs in f64 and f32."""
    t1, t2 = texture(H, W, 1), texture(H, W, 2)
    buf = np.stack([_as(kind, p) for p in (np.roll(t1, (-SHIFT[0], -SHIFT[1]), (0, 1)), t1, t2, np.roll(t2, SHIFT, (0, 1)))])
    h64 = np.stack([T.farneback_host(buf[i], buf[i + 1]) for i in range(3)])
    h32 = np.stack([T.farneback_host(buf[i], buf[i + 1], dtype=np.float32) for i in range(3)])
    return buf, h64, h32


@pytest.mark.parametrize("H,W,kind", [(256, 272, "u8"), (75, 101, "u8"), (75, 101, "u16"), (75, 101, "f32"), (40, 48, "u8"),
                                      (33, 300, "u8")])
def test_whole_flow_in_a_batch_of_strided_views(H, W, kind):
    buf, h64, h32 = _flow_case(H, W, kind)
    d = _dev(buf)
    got = hip.farneback_flow(d[:-1], d[1:])
    assert got.shape == (3, H, W, 2) and got.dtype == torch.float32
    for i in range(3):
        alone = hip.farneback_flow(d[i:i + 1], d[i + 1:i + 2])
        assert torch.equal(alone[0], got[i]), f"pair {i} alone differs from pair {i} in the batch"
    g = got.cpu().numpy()
    for i, name in enumerate(("shift", "t1-t2", "shift2")):
        _check(f"flow {H}x{W} {kind} {name}", g[i], h64[i], h32[i])
    if kind == "u8":                                                       # the known answer, where the pyramid can follow it
        m = 24 if H >= 128 else 16
        if H > 2 * m + 1 and T.level_count(H, W) > 1:
            inner = g[0, m:H - m, m:W - m]
            assert np.abs(inner[..., 0] - SHIFT[1]).max() <= 0.02 and np.abs(inner[..., 1] - SHIFT[0]).max() <= 0.02


def test_flow_arguments():
    d = _dev(np.stack([texture(40, 48, 1)] * 2))
    for kw in ({"levels": 2}, {"winsize": 13}, {"pyr_scale": 0.8}, {"iterations": 2}, {"poly_n": 7}, {"poly_sigma": 1.1}, {"flags": 256}):
        with pytest.raises(ValueError):
            hip.farneback_flow(d[:1], d[1:], **kw)
    assert hip.farneback_flow(d[:1], d[1:], levels=3, winsize=15).shape == (1, 40, 48, 2)
    assert hip.farneback_flow(d[:0], d[:0]).shape == (0, 40, 48, 2)
    with pytest.raises(RuntimeError):
        hip.farneback_flow(d[:1].cpu(), d[1:].cpu())
    with pytest.raises(ValueError):
        hip.farneback_flow(d[:1], d[1:].float())
    with pytest.raises(ValueError):
        hip.farneback_flow(d[:1].to(torch.int32), d[1:].to(torch.int32))
    fn = hip.lib().fcvsr_farneback_flow                                    # argument errors come back before any device call
    out = torch.empty((1, 40, 48, 2), device="cuda")
    scratch = torch.empty((hip.lib().fcvsr_farneback_scratch_bytes(1, 40, 48) // 4,), device="cuda")
    ok = [d.data_ptr(), d[1:].data_ptr(), hip.FLOW_U8, 1, 40, 48, 0, 0, scratch.data_ptr(), scratch.numel() * 4, out.data_ptr()]
    for k, v in ((2, 4), (3, -1), (4, 1), (5, 20000), (6, -1), (8, 0), (9, scratch.numel() * 4 - 1), (10, 0)):
        bad = list(ok)
        bad[k] = v
        assert fn(*bad, hip.stream_ptr()) != 0, (k, v)
    assert hip.lib().fcvsr_farneback_scratch_bytes(1, 1, 48) == -1
    torch.cuda.synchronize()


def test_flow_epe():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((2, 3, 75, 101, 2)).astype(np.float32) * 3   # 7575 pixels: more than one workgroup per plane
    got = hip.flow_epe(_dev(a), _dev(b))
    assert got.dtype == torch.float64 and got.shape == (3,)
    for p in range(3):
        want = T.epe_host(a[p], b[p])
        assert abs(float(got[p]) - want) <= 1e-12 * want, (p, float(got[p]), want)
    assert hip.flow_epe(_dev(a), _dev(a)).cpu().tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(hip.flow_epe(_dev(a[1:2]), _dev(b[1:2]))[0], got[1])   # a plane's mean does not depend on the batch
    assert hip.flow_epe(_dev(a[:0]), _dev(b[:0])).shape == (0,)
    with pytest.raises(RuntimeError):
        hip.flow_epe(torch.from_numpy(a), torch.from_numpy(b))


def test_frame_tof_follows_the_sequence_rules():
    t = texture(40, 48, 1)
    pred = np.stack([np.roll(t, (0, k), (0, 1)) for k in range(5)])
    true = np.stack([np.roll(t, (k % 2, k), (0, 1)) for k in range(5)])
    got = T.frame_tof(_dev(pred), _dev(true)).cpu().numpy()
    host = T.sequence_tof_host(pred, true)["tof"]
    host32 = T.sequence_tof_host(pred, true, dtype=np.float32)["tof"]
    assert got[0] == 0.0
    _check("frame_tof", got, host, host32)
    cut = T.frame_tof(_dev(pred), _dev(true), cuts=[3]).cpu().numpy()
    assert cut[3] == 0.0 and np.array_equal(cut[[0, 1, 2, 4]], got[[0, 1, 2, 4]])
    tail = T.frame_tof(_dev(pred[2:]), _dev(true[2:]), first=(_dev(pred[1]), _dev(true[1]))).cpu().numpy()
    assert np.array_equal(tail, got[2:])                                   # the carried pair: the same bits as inside one batch
    assert T.frame_tof(_dev(pred[:1]), _dev(true[:1])).cpu().tolist() == [0.0]
    with pytest.raises(RuntimeError):
        T.frame_tof(torch.from_numpy(pred), torch.from_numpy(true))
    with pytest.raises(ValueError):
        T.frame_tof(_dev(pred), _dev(true[:4]))


# ---- through the harness ---------------------------------------------------------------------------------------------------------

_models = {}


def _model():
    """The synthetic-weight S model of the other harness tests, built once."""
    if "m" not in _models:
        from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
        from fcvsr_amd.arch.schema import state_dict_shapes
        from fcvsr_amd.weights import synthetic_state_dict
        m = GShiftNet_S()
        m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
        m = m.cuda()
        m.precision = "bf16"
        _models["m"] = m
    return _models["m"]


def _moving(n, h, w, peak):
    """n frames of one smooth texture drifting by a pixel a frame, plus a little noise, as integers up to `peak`."""
    t = texture(h + n, w + n, 3).astype(np.float64) / 255
    rs = np.random.RandomState(n + h)
    return np.stack([np.clip(np.floor(peak * t[i:i + h, 2 * (i // 2):2 * (i // 2) + w]) + rs.randint(0, 3, (h, w)), 0, peak)
                     for i in range(n)])


def test_evaluate_sequence_scores_tof_next_to_psnr_and_ssim():
    from fcvsr_amd.harness.infer import evaluate_sequence
    hr = _moving(7, 128, 128, 255).astype(np.uint8)[:, None]
    lr = torch.from_numpy(np.ascontiguousarray(hr[:, :, ::4, ::4]))
    hr_t = torch.from_numpy(hr)
    plain = evaluate_sequence(_model(), lr, hr_t, return_frames=True, batch=3)
    got = evaluate_sequence(_model(), lr, hr_t, tof=True, return_frames=True, batch=3)
    assert plain.tof is None and plain.tof_mean is None and plain.tof_pairs_mean is None
    assert np.array_equal(got.psnr, plain.psnr) and np.array_equal(got.ssim, plain.ssim) and np.array_equal(got.frames, plain.frames)
    assert got.tof.shape == (7,) and got.tof.dtype == np.float64 and got.tof[0] == 0.0 and (got.tof[1:] > 0).all()
    h64 = T.sequence_tof_host(got.frames[:, 0], hr[:, 0])
    h32 = T.sequence_tof_host(got.frames[:, 0], hr[:, 0], dtype=np.float32)
    _check("evaluate_sequence tof", got.tof, h64["tof"], h32["tof"])
    assert got.tof_mean == float(got.tof.mean()) and got.tof_pairs_mean == float(got.tof[1:].mean())
    cut = evaluate_sequence(_model(), lr, hr_t, tof=True, return_frames=True, batch=3, cuts=[4])
    assert cut.tof[4] == 0.0 and cut.tof[0] == 0.0 and cut.cuts == [4]
    c64 = T.sequence_tof_host(cut.frames[:, 0], hr[:, 0], cuts=[4])
    _check("evaluate_sequence tof, cuts=[4]", cut.tof, c64["tof"], T.sequence_tof_host(cut.frames[:, 0], hr[:, 0], [4], np.float32)["tof"])
    assert cut.tof_pairs_mean == float(cut.tof[[1, 2, 3, 5, 6]].mean())
    base = evaluate_sequence(_model(), lr, hr_t, tof=True, batch=3, baseline="bicubic")
    assert base.baseline_tof.shape == (7,) and base.baseline_tof[0] == 0.0 and np.array_equal(base.tof, got.tof)
    assert base.baseline_tof_mean == float(base.baseline_tof.mean())
    with pytest.raises(ValueError, match="tof=True scores one plane"):
        evaluate_sequence(_model(), lr.expand(-1, 3, -1, -1), hr_t.expand(-1, 3, -1, -1), tof=True)


SH, SW, SN = 18, 20, 10


def _i420(bits):
    """SN I420 frames of SH x SW as bytes, the luma drifting; and a ground truth for the 4x frames (a drifting texture as well)."""
    peak = 255 if bits == 8 else 1023
    dt = np.uint8 if bits == 8 else "<u2"
    rs = np.random.RandomState(bits)

    def pack(y, h, w):
        out = []
        for f in y:
            out += [f.reshape(-1), peak // 2 + rs.randint(-9, 9, 2 * (h // 2) * (w // 2))]
        return np.concatenate(out).astype(dt).view(np.uint8).tobytes()
    gt = _moving(SN, 4 * SH, 4 * SW, peak)
    return pack(gt[:, ::4, ::4], SH, SW), pack(gt, 4 * SH, 4 * SW), gt


@pytest.mark.parametrize("bits", [8, 10])
def test_streaming_carries_the_pair_across_groups(bits, tmp_path):
    from fcvsr_amd.harness.reference import scores_csv
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import super_resolve_yuv420
    src_b, gt_b, gt = _i420(bits)
    src, ref = str(tmp_path / "in.yuv"), str(tmp_path / "gt.yuv")
    for p, b in ((src, src_b), (ref, gt_b)):
        with open(p, "wb") as f:
            f.write(b)
    fmt = "yuv420p" if bits == 8 else "yuv420p10le"
    out = {k: str(tmp_path / (k + ".yuv")) for k in ("whole", "stream", "plain")}
    whole = super_resolve_yuv420(_model(), src, out["whole"], SW, SH, bit_depth=bits, batch=4, reference=ref, tof=True)
    stream = stream_yuv420(_model(), src, out["stream"], SW, SH, pix_fmt=fmt, batch=4, reference=ref, tof=True)
    plain = stream_yuv420(_model(), src, out["plain"], SW, SH, pix_fmt=fmt, batch=4, reference=ref)
    data = {k: open(p, "rb").read() for k, p in out.items()}
    assert data["whole"] == data["plain"] == data["stream"] and len(data["plain"]) == SN * 16 * SH * SW * 3 // 2 * (bits // 8 + (bits > 8))
    assert "tof" not in plain and "tof_mean" not in plain
    assert whole["tof"].shape == (SN,) and whole["tof"][0] == 0.0 and (whole["tof"][1:] > 0).all()
    assert np.array_equal(stream["tof"], whole["tof"])                     # bit for bit: the carry across the groups of 4
    assert stream["tof_mean"] == whole["tof_mean"] == float(whole["tof"].mean())
    assert whole["tof_pairs_mean"] == float(whole["tof"][1:].mean())
    for k in ("psnr_y", "ssim_y", "sse"):
        assert np.array_equal(stream[k], plain[k])
    ysr = np.frombuffer(data["whole"], dtype=np.uint8 if bits == 8 else "<u2").reshape(SN, -1)[:, :16 * SH * SW].reshape(SN, 4 * SH, 4 * SW)
    gty = gt.astype(np.uint8 if bits == 8 else np.uint16)
    _check(f"streamed tof, {bits} bit", whole["tof"], T.sequence_tof_host(ysr, gty)["tof"],
           T.sequence_tof_host(ysr, gty, dtype=np.float32)["tof"])
    head = scores_csv(stream).splitlines()[0]
    assert head.endswith(",ssim_y,tof") and not scores_csv(plain).splitlines()[0].endswith("tof")
    cut = stream_yuv420(_model(), src, None, SW, SH, pix_fmt=fmt, batch=4, reference=ref, tof=True, cuts=[4, 6])
    assert cut["tof"][4] == 0.0 and cut["tof"][6] == 0.0 and cut["tof"][5] > 0
    assert cut["tof_pairs_mean"] == float(cut["tof"][[1, 2, 3, 5, 7, 8, 9]].mean())
    base = [stream_yuv420(_model(), src, None, SW, SH, pix_fmt=fmt, batch=b, reference=ref, tof=True, baseline="bicubic") for b in (4, 3)]
    assert np.array_equal(base[0]["tof"], whole["tof"]) and np.array_equal(base[1]["tof"], whole["tof"])
    assert base[0]["baseline_tof"].shape == (SN,) and base[0]["baseline_tof"][0] == 0.0 and (base[0]["baseline_tof"][1:] > 0).all()
    assert np.array_equal(base[0]["baseline_tof"], base[1]["baseline_tof"])  # the baseline's carried plane, at two group sizes
    assert base[0]["baseline_tof_mean"] == float(base[0]["baseline_tof"].mean())
    for fn in (lambda: stream_yuv420(_model(), src, out["plain"], SW, SH, pix_fmt=fmt, tof=True),
               lambda: super_resolve_yuv420(_model(), src, out["plain"], SW, SH, bit_depth=bits, tof=True)):
        with pytest.raises(ValueError, match="needs reference="):
            fn()
