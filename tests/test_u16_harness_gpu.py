"""GPU: the sequence harness with uint16 LR frames (10-bit samples in 16-bit containers) gives the results of the float frames
lr.float() / 1023, the streamed scheduler uploads half the bytes, the 10-bit chroma up-sampler follows its torch definition, and
the 10-bit YUV 4:2:0 path from file to file is the sequence path on Y plus the chroma kernel on U and V."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _model(precision="bf16"):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = precision
    return m


def _seq(N, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 1024, (N, 1, H, W)).astype(np.uint16))


def _float(t16):
    return torch.from_numpy(t16.numpy().astype(np.float32)) / 1023


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("hw", [(16, 20), (18, 20)])                 # 18 rows: padded to 20 as the reference pads 270 -> 272
def test_sequences_u16_equal_float_frames(hw, quantise):
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    m = _model()
    H, W = hw
    lr16 = _seq(9, H, W, seed=1 + H)
    hr = torch.from_numpy(np.random.RandomState(3).randint(0, 1024, (9, 1, 4 * H, 4 * W)).astype(np.uint16))
    got = super_resolve_sequence(m, lr16, batch=4, quantise=quantise)
    assert got.dtype == np.uint16 and got.shape == (9, 1, 4 * H, 4 * W) and int(got.max()) <= 1023
    assert np.unique(got).size > 32
    # device-resident uint16 input and a subset of centres
    sub = super_resolve_sequence(m, _dev16(lr16.numpy()), batch=2, centres=[8, 0, 3], quantise=quantise)
    assert np.array_equal(sub, got[[8, 0, 3]])
    a = evaluate_sequence(m, lr16, hr, batch=4, quantise=quantise, return_frames=True)
    b = evaluate_sequence(m, _float(lr16), hr, batch=4, quantise=quantise, return_frames=True)
    assert a.frames.dtype == np.uint16 and b.frames.dtype == np.uint16
    assert np.array_equal(a.frames, b.frames) and np.array_equal(a.frames, got)
    assert np.array_equal(a.psnr, b.psnr) and np.array_equal(a.ssim, b.ssim)
    assert a.psnr_mean == b.psnr_mean and a.ssim_mean == b.ssim_mean
    p, s = frame_metrics(_dev16(got), _dev16(hr.numpy()), crop_border=4, quantise=None)
    assert np.array_equal(a.psnr, p.cpu().numpy()) and np.array_equal(a.ssim, s.cpu().numpy())
    with pytest.raises(ValueError):                              # 8-bit lr against 10-bit hr
        evaluate_sequence(m, torch.zeros(9, 1, H, W, dtype=torch.uint8), hr)


def test_streamed_run_u16_equals_float_frames_with_half_of_the_upload():
    """The streamed uint16 run against the float frames.  A float streamed run has no bit depth to go by and quantises to 8 bits,
    so its frames cannot be compared with 10-bit ones: the keys, first centres, shapes, uploaded frame counts and the byte counts
    (half of the float run's) are compared with the float streamed run, and the frames themselves with `evaluate_sequence` on
    the float frames and a uint16 hr, which quantises the float path's output with the 1023 scale."""
    from fcvsr_amd.harness.infer import StreamedSuperResolver
    m = _model()
    seqs16 = [_seq(n, 18, 20, seed=10 + n) for n in (7, 5)]
    seqsf = [_float(s) for s in seqs16]
    for world in (1, 2):
        for rank in range(world):
            r16 = StreamedSuperResolver(m, batch=4)
            got = r16.run(seqs16, rank=rank, world=world)
            rf = StreamedSuperResolver(m, batch=4)
            ref = rf.run(seqsf, rank=rank, world=world)
            assert got.keys() == ref.keys()
            for s in ref:
                # the float run quantises to 8 bits: its 10-bit counterpart is the sequence path on the float frames
                assert got[s][0] == ref[s][0] and got[s][1].dtype == np.uint16 and got[s][1].shape == ref[s][1].shape
            assert r16.stats["frames_uploaded"] == rf.stats["frames_uploaded"]
            assert 2 * r16.stats["h2d_bytes"] == rf.stats["h2d_bytes"]
            assert r16._bufs["ring"].element_size() == 2 and r16._bufs["stage"][0].element_size() == 2
    # the frames: equal to the float frames' 10-bit results (evaluate_sequence quantises the float path with the 1023 scale)
    from fcvsr_amd.harness.infer import evaluate_sequence
    got = StreamedSuperResolver(m, batch=4).run(seqs16)
    for s, lr16 in enumerate(seqs16):
        hr = torch.zeros(lr16.shape[0], 1, 72, 80, dtype=torch.int16).view(torch.uint16)
        ref = evaluate_sequence(m, _float(lr16), hr, batch=4, return_frames=True).frames
        assert got[s][0] == 0 and np.array_equal(got[s][1], ref)
    with pytest.raises(ValueError, match="uint16"):
        StreamedSuperResolver(m, batch=4).run([seqs16[0], seqsf[1]])
    with pytest.raises(ValueError, match="uint16"):
        StreamedSuperResolver(m, batch=4).run([seqs16[0], torch.from_numpy((seqs16[1].numpy() >> 2).astype(np.uint8))])


def _chroma_ref(planes_u16):
    x = torch.from_numpy(planes_u16.numpy().astype(np.float32))[:, None] / 1023
    y = F.interpolate(x, scale_factor=4, mode="bicubic", align_corners=False)[:, 0]
    return (y.clamp(0, 1) * 1023).round().to(torch.int32)


def _chroma(planes_u16):
    from fcvsr_amd import hip
    out = hip.chroma_up4(_dev16(planes_u16.numpy()))
    assert out.dtype == torch.uint16
    return torch.from_numpy(_host16(out).astype(np.int32))


def test_chroma_kernel_u16_matches_torch_bicubic():
    rs = np.random.RandomState(4)
    planes = [torch.from_numpy(rs.randint(0, 1024, (3, 5, 7)).astype(np.uint16)),
              torch.from_numpy(rs.randint(0, 1024, (2, 33, 18)).astype(np.uint16))]
    yy, xx = np.mgrid[0:33, 0:18]
    planes.append(torch.from_numpy(np.clip(512 + 400 * np.sin(yy / 5.0) * np.cos(xx / 7.0), 0, 1023).astype(np.uint16))[None])
    edge = np.zeros((1, 8, 12), np.uint16)                       # 0 and 1023 side by side: the overshoot clamps, it does not wrap
    edge[:, :, 6:] = 1023
    edge[:, 4:, :] = 1023 - edge[:, 4:, :]
    planes.append(torch.from_numpy(edge))
    for p in planes:
        got, ref = _chroma(p), _chroma_ref(p)
        assert got.shape == ref.shape and int(got.max()) <= 1023 and int(got.min()) >= 0
        d = (got - ref).abs()
        assert int(d.max()) <= 1 and float(d.float().mean()) < 0.01, (int(d.max()), float(d.float().mean()))
    got = _chroma(planes[-1])
    assert int((got == 0).sum()) > 100 and int((got == 1023).sum()) > 100
    # exact on constant planes, every code value; samples above 1023 read as 1023
    const = torch.from_numpy(np.arange(1024, dtype=np.uint16))[:, None, None].expand(1024, 3, 4).contiguous()
    got = _chroma(const)
    assert torch.equal(got, torch.arange(1024, dtype=torch.int32)[:, None, None].expand(1024, 12, 16))
    assert torch.equal(got, _chroma_ref(const))
    over = torch.from_numpy(np.array([1024, 4095, 65535], np.uint16))[:, None, None].expand(3, 3, 4).contiguous()
    assert torch.equal(_chroma(over), torch.full((3, 12, 16), 1023, dtype=torch.int32))


def test_super_resolve_yuv420_10bit_file_to_file(tmp_path):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import parse_yuv_name, read_yuv420, super_resolve_yuv420, write_yuv420, yuv_bit_depth
    m = _model()
    N, H, W = 5, 16, 20
    rs = np.random.RandomState(5)
    y = rs.randint(0, 1024, (N, H, W)).astype(np.uint16)
    u = rs.randint(0, 1024, (N, H // 2, W // 2)).astype(np.uint16)
    v = rs.randint(0, 1024, (N, H // 2, W // 2)).astype(np.uint16)
    src = str(tmp_path / f"Seq_{W}x{H}_{N}F_10bit.yuv")
    dst = str(tmp_path / f"Seq_{4 * W}x{4 * H}_{N}F_10bit.yuv")
    write_yuv420(src, y, u, v)
    info = parse_yuv_name(src)
    assert yuv_bit_depth(src) == 10
    stats = super_resolve_yuv420(m, src, dst, info.width, info.height, batch=2, bit_depth=yuv_bit_depth(src))
    assert os.path.getsize(dst) == 5 * 80 * 64 * 3 // 2 * 2
    assert stats["frames"] == N and stats["bytes_written"] == os.path.getsize(dst) and stats["bytes_read"] == os.path.getsize(src)
    oy, ou, ov = read_yuv420(dst, 4 * W, 4 * H, bit_depth=10)
    assert oy.dtype == np.uint16 and max(int(oy.max()), int(ou.max()), int(ov.max())) <= 1023
    ref_y = super_resolve_sequence(m, torch.from_numpy(y)[:, None], batch=3)
    assert np.array_equal(oy, ref_y[:, 0])
    assert np.array_equal(ou, _chroma(torch.from_numpy(u)).numpy())
    assert np.array_equal(ov, _chroma(torch.from_numpy(v)).numpy())
