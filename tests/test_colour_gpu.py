"""GPU: the two colour kernels (csrc/colour.hip) equal the host specification of harness.colour sample for sample, their entry
points reject bad arguments before any launch, and the two paths built on them - YUV 4:2:0 files through an RGB model, and the clip
sampler fed from YUV files - are the compositions of host functions they are documented to be."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = list(itertools.product(("bt601", "bt709"), (False, True), ("left", "center"), (8, 10)))
# 2x2: every tap clamped; 4x6 and 18x22: scalar path, odd chroma width, a partial last run; 66x264: W % 8 == 0, the vector path,
# 3 * 33 * 33 lanes = 13 workgroups whose boundaries fall inside rows and frames
SHAPES = [(3, 2, 2), (3, 4, 6), (3, 18, 22), (3, 66, 264)]


def _spec(matrix, full_range, chroma_loc, bit_depth):
    from fcvsr_amd.harness.colour import ColourSpec
    return ColourSpec(matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, bit_depth=bit_depth)


def _dev(a):
    from fcvsr_amd import hip
    t = torch.from_numpy(np.ascontiguousarray(a))
    return hip.bits16(t).to(DEV).view(t.dtype)


def _host(t):
    from fcvsr_amd import hip
    return hip.frames_to_numpy(t)


def _inputs(d):
    """{(kind, shape): (y, u, v, rgb)} host arrays, made once per depth: seeded random planes, all-0 and all-P planes and, for
    uint16, planes with samples above 1023."""
    if d in _INPUTS:
        return _INPUTS[d]
    P, dt = (1 << d) - 1, (np.uint8 if d == 8 else np.uint16)
    rs = np.random.RandomState(40 + d)
    out = {}
    for N, H, W in SHAPES:
        shp = ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2), (N, 3, H, W))
        out["random", (N, H, W)] = tuple(rs.randint(0, P + 1, s).astype(dt) for s in shp)
        out["zeros", (N, H, W)] = tuple(np.zeros(s, dt) for s in shp)
        out["peak", (N, H, W)] = tuple(np.full(s, P, dt) for s in shp)
        if d == 10:
            hot = []
            for s in shp:
                a = rs.randint(0, P + 1, s).astype(dt)
                m = rs.rand(*s) < 0.25
                a[m] = rs.choice([1024, 2047, 0x8000, 0xFFFF], int(m.sum())).astype(dt)
                hot.append(a)
            out["above_1023", (N, H, W)] = tuple(hot)
    _INPUTS[d] = out
    return out


_INPUTS = {}


@pytest.mark.parametrize("matrix,full_range,chroma_loc,d", COMBOS)
def test_kernels_equal_the_host_specification(matrix, full_range, chroma_loc, d):
    from fcvsr_amd.harness.colour import rgb_to_yuv420, rgb_to_yuv420_host, yuv420_to_rgb, yuv420_to_rgb_host
    spec = _spec(matrix, full_range, chroma_loc, d)
    for (kind, shape), (y, u, v, rgb) in _inputs(d).items():
        got = yuv420_to_rgb(_dev(y), _dev(u), _dev(v), spec)
        assert got.dtype == spec.dtype and tuple(got.shape) == rgb.shape and got.is_contiguous()
        ref = yuv420_to_rgb_host(y, u, v, spec)
        bad = int((_host(got) != ref).sum())
        assert bad == 0, f"decode {kind} {shape}: {bad} of {ref.size} samples differ"
        planes = rgb_to_yuv420(_dev(rgb), spec)
        for name, g, r in zip("yuv", planes, rgb_to_yuv420_host(rgb, spec)):
            assert g.dtype == spec.dtype and tuple(g.shape) == r.shape
            bad = int((_host(g) != r).sum())
            assert bad == 0, f"encode {kind} {shape} plane {name}: {bad} of {r.size} samples differ"


@pytest.mark.parametrize("d", [8, 10])
@pytest.mark.parametrize("chroma_loc", ["left", "center"])
@pytest.mark.parametrize("shape", [(3, 18, 22), (2, 16, 40)])
def test_i420_batch_buffer_through_frame_strides(shape, chroma_loc, d):
    """Frames as a file holds them (Y | U | V per frame, one buffer): decoded from the buffer in place, encoded into one, in the
    scalar (18x22) and the vector (16x40) form."""
    from fcvsr_amd.harness.colour import i420_planes, rgb_to_i420, rgb_to_yuv420_host, yuv420_to_rgb, yuv420_to_rgb_host
    spec = _spec("bt709", False, chroma_loc, d)
    N, H, W = shape
    P, dt = spec.peak, (np.uint8 if d == 8 else np.uint16)
    rs = np.random.RandomState(H + d)
    fs = H * W * 3 // 2
    frames = rs.randint(0, P + 1, (N, fs)).astype(dt)
    y, u, v = frames[:, :H * W].reshape(N, H, W), frames[:, H * W:H * W * 5 // 4].reshape(N, H // 2, W // 2), \
        frames[:, H * W * 5 // 4:].reshape(N, H // 2, W // 2)
    fd = _dev(frames)
    py, pu, pv = i420_planes(fd, H, W)
    assert py.data_ptr() == fd.data_ptr() and pu.data_ptr() == fd.data_ptr() + H * W * fd.element_size()
    assert py.stride(0) == pu.stride(0) == pv.stride(0) == fs
    rgb = yuv420_to_rgb(py, pu, pv, spec)
    assert np.array_equal(_host(rgb), yuv420_to_rgb_host(y, u, v, spec))
    src = rs.randint(0, P + 1, (N, 3, H, W)).astype(dt)
    out = rgb_to_i420(_dev(src), spec)
    assert tuple(out.shape) == (N, fs) and out.is_contiguous()
    ry, ru, rv = rgb_to_yuv420_host(src, spec)
    assert np.array_equal(_host(out), np.concatenate([ry.reshape(N, -1), ru.reshape(N, -1), rv.reshape(N, -1)], 1))
    # a strided RGB source (a crop of larger frames) is taken through a dense copy
    big = rs.randint(0, P + 1, (N, 3, H + 2, W + 4)).astype(dt)
    out = rgb_to_i420(_dev(big)[:, :, :H, :W], spec)
    ry, ru, rv = rgb_to_yuv420_host(big[:, :, :H, :W], spec)
    assert np.array_equal(_host(out), np.concatenate([ry.reshape(N, -1), ru.reshape(N, -1), rv.reshape(N, -1)], 1))


def test_entry_points_reject_bad_arguments_and_launch_nothing():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.colour import ColourSpec, coefficients
    L = hip.lib()
    for d, dec, enc in ((8, L.fcvsr_yuv420_to_rgb, L.fcvsr_rgb_to_yuv420), (10, L.fcvsr_yuv420_to_rgb_u16, L.fcvsr_rgb_to_yuv420_u16)):
        dt = torch.uint8 if d == 8 else torch.int16
        N, H, W = 2, 4, 8
        y = torch.full((N, H, W), 7, dtype=dt, device=DEV)
        u = torch.full((N, H // 2, W // 2), 7, dtype=dt, device=DEV)
        v = torch.full((N, H // 2, W // 2), 7, dtype=dt, device=DEV)
        rgb = torch.full((N, 3, H, W), 7, dtype=dt, device=DEV)
        good = hip.Colour(**coefficients(ColourSpec(bit_depth=d)))
        shift13 = hip.Colour(**dict(coefficients(ColourSpec(bit_depth=d)), shift=13))
        siting = hip.Colour(**dict(coefficients(ColourSpec(bit_depth=d)), chroma_loc=2))
        st = hip.stream_ptr()

        def decode(y_=y.data_ptr(), u_=u.data_ptr(), v_=v.data_ptr(), n=N, h=H, w=W, sy=H * W, su=H * W // 4, sv=H * W // 4,
                   k=good, o=rgb.data_ptr()):
            return dec(y_, u_, v_, n, h, w, sy, su, sv, k, o, st)

        def encode(s=rgb.data_ptr(), n=N, h=H, w=W, k=good, sy=H * W, su=H * W // 4, sv=H * W // 4, y_=y.data_ptr(), u_=u.data_ptr(),
                   v_=v.data_ptr()):
            return enc(s, n, h, w, k, sy, su, sv, y_, u_, v_, st)

        for call in (decode, encode):
            bad = [dict(h=3), dict(w=7), dict(h=0), dict(w=-2), dict(n=0), dict(y_=None), dict(u_=None), dict(v_=None),
                   dict(k=None), dict(k=shift13), dict(k=siting), dict(sy=H * W - 1), dict(su=1), dict(sv=0)]
            bad.append(dict(o=None) if call is decode else dict(s=None))
            if d == 10:
                bad.append(dict(y_=y.data_ptr() + 1))
            for kw in bad:
                with pytest.raises(hip.HipError):
                    hip.check(call(**kw), "colour")
        assert decode(k=shift13) != 0 and b"shift" in L.fcvsr_last_error()
        assert encode(h=6, w=9) != 0 and b"even" in L.fcvsr_last_error()
        torch.cuda.synchronize()
        for t in (y, u, v, rgb):                                  # nothing was launched: every buffer still holds its fill
            assert bool((t == 7).all())
        assert decode() == 0 and encode() == 0
        torch.cuda.synchronize()


def _rgb_model(precision="bf16"):
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = FCVSR_SNet()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("FCVSR_SNet"), gain=0.5), strict=True)
    m = m.to(DEV)
    m.precision = precision
    return m


@pytest.fixture(scope="module")
def rgb_model():
    return _rgb_model()


def _composition(model, y, u, v, spec, batch, quantise):
    """Host decode, zero pad, window_indices, the model's integer path in the same batches, crop, host encode."""
    from fcvsr_amd.harness.colour import rgb_to_yuv420_host, yuv420_to_rgb_host
    from fcvsr_amd.harness.windows import window_indices
    N, H, W = y.shape
    rgb = yuv420_to_rgb_host(y, u, v, spec)
    x = np.zeros((N, 3, H + (-H) % 4, W + (-W) % 4), rgb.dtype)
    x[:, :, :H, :W] = rgb
    frames = []
    for s in range(0, N, batch):
        idx = [window_indices(i, 7, N, "replicate") for i in range(s, min(N, s + batch))]
        win = _dev(np.stack([x[j] for j in idx], 0))
        sr = model.super_resolve_u8(win, quantise) if spec.bit_depth == 8 else model.super_resolve_u16(win, quantise)
        sy, su, sv = rgb_to_yuv420_host(_host(sr)[:, :, :4 * H, :4 * W], spec)
        for i in range(sy.shape[0]):
            frames += [sy[i].ravel(), su[i].ravel(), sv[i].ravel()]
    return np.concatenate(frames)


@pytest.mark.parametrize("d,quantise", [(8, "truncate"), (8, "round"), (10, "truncate")])
def test_yuv420_file_through_an_rgb_model_equals_the_composition(tmp_path, rgb_model, d, quantise):
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    spec = _spec("bt709", False, "left", d)
    N, H, W = 9, 18, 22                                          # padded to 20 x 24 inside, cropped off again
    P, dt = spec.peak, (np.uint8 if d == 8 else np.uint16)
    rs = np.random.RandomState(50 + d)
    y, u, v = (rs.randint(0, P + 1, s).astype(dt) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
    src, dst = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv"), str(tmp_path / "out.yuv")
    write_yuv420(src, y, u, v)
    stats = super_resolve_yuv420_rgb(rgb_model, src, dst, W, H, colour=spec, batch=4, quantise=quantise)
    size = N * 16 * W * H * 3 // 2 * (1 if d == 8 else 2)
    assert os.path.getsize(dst) == size and stats["frames"] == N and stats["bytes_written"] == size
    assert stats["out_size"] == (4 * W, 4 * H) and stats["bytes_read"] == os.path.getsize(src)
    got = np.fromfile(dst, dtype=np.uint8 if d == 8 else "<u2")
    ref = _composition(rgb_model, y, u, v, spec, 4, quantise)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} samples differ"
    assert np.unique(got).size > 32                              # a real picture, not frames clamped to the ends


def test_sampler_from_yuv420_rgb_holds_the_host_decode(tmp_path):
    from fcvsr_amd.harness.colour import ColourSpec, yuv420_to_rgb_host
    from fcvsr_amd.harness.yuv import write_yuv420
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    rs = np.random.RandomState(60)
    pairs, host = [], []
    for i, (N, H, W) in enumerate([(8, 22, 26), (7, 20, 24)]):
        planes = []
        for k, name in ((1, "lr"), (4, "hr")):
            y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in
                       ((N, k * H, k * W), (N, k * H // 2, k * W // 2), (N, k * H // 2, k * W // 2)))
            path = str(tmp_path / f"s{i}{name}_{k * W}x{k * H}_{N}F.yuv")
            write_yuv420(path, y, u, v)
            planes.append((path, (y, u, v)))
        pairs.append((planes[0][0], planes[1][0]))
        host.append(tuple(yuv420_to_rgb_host(*p[1], ColourSpec()) for p in planes))
    sampler = DeviceClipSampler.from_yuv420_rgb(pairs, batch=2, crop=16, seed=3, device=DEV)
    assert sampler.channels == 3 and sampler.bit_depth == 8 and len(sampler) == 2
    for (lr, hr), (hlr, hhr) in zip(sampler.sequences, host):
        assert np.array_equal(_host(lr), hlr) and np.array_equal(_host(hr), hhr)
    bp = sampler.plan(0)[0]
    got, ref = sampler.build(bp), apply_plan_host(host, bp, 16)
    assert got["lr_imgs"].shape == (2, 3, 7, 16, 16)
    assert torch.equal(got["lr_imgs"].cpu(), ref["lr_imgs"]) and torch.equal(got["hr_imgs"].cpu(), ref["hr_imgs"])
    # another matrix, range and siting, 10-bit files: the depth comes from the spec
    spec = ColourSpec("bt601", True, "center", 10)
    y, u, v = (rs.randint(0, 1024, s).astype(np.uint16) for s in ((7, 20, 24), (7, 10, 12), (7, 10, 12)))
    Y, U, V = (rs.randint(0, 1024, s).astype(np.uint16) for s in ((7, 80, 96), (7, 40, 48), (7, 40, 48)))
    a, b = str(tmp_path / "t_24x20_7F_10bit.yuv"), str(tmp_path / "t_96x80_7F_10bit.yuv")
    write_yuv420(a, y, u, v)
    write_yuv420(b, Y, U, V)
    s10 = DeviceClipSampler.from_yuv420_rgb([(a, b)], colour=spec, batch=1, crop=16, seed=1, device=DEV)
    assert s10.bit_depth == 10 and s10.dtype == torch.uint16
    assert np.array_equal(_host(s10.sequences[0][0].view(torch.uint16)), yuv420_to_rgb_host(y, u, v, spec))
    assert np.array_equal(_host(s10.sequences[0][1].view(torch.uint16)), yuv420_to_rgb_host(Y, U, V, spec))
