"""GPU: the sequence harness with uint8 LR frames (decoded 8-bit video) gives the results of the float frames lr.float() / 255,
the streamed scheduler uploads a quarter of the bytes, the chroma up-sampler follows its torch definition, and the YUV 4:2:0
path from file to file is the sequence path on Y plus the chroma kernel on U and V."""
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
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, 1, H, W)).astype(np.uint8))


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_super_resolve_sequence_u8_equals_float_frames(precision, quantise):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    m = _model(precision)
    lr8 = _seq(6, 18, 20, seed=1)                    # 18 rows: padded to 20 as the reference pads 270 -> 272
    got = super_resolve_sequence(m, lr8, batch=4, quantise=quantise)
    ref = super_resolve_sequence(m, lr8.float() / 255, batch=4, quantise=quantise)
    assert got.dtype == np.uint8 and got.shape == (6, 1, 72, 80)
    assert np.array_equal(got, ref)
    # device-resident uint8 input and a subset of centres
    sub = super_resolve_sequence(m, lr8.cuda(), batch=2, centres=[5, 0, 3], quantise=quantise)
    assert np.array_equal(sub, ref[[5, 0, 3]])


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_evaluate_sequence_u8_equals_float_frames(quantise):
    from fcvsr_amd.harness.infer import evaluate_sequence
    m = _model()
    lr8 = _seq(5, 18, 24, seed=2)
    hr = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (5, 1, 72, 96)).astype(np.uint8))
    a = evaluate_sequence(m, lr8, hr, batch=3, quantise=quantise, return_frames=True)
    b = evaluate_sequence(m, lr8.float() / 255, hr, batch=3, quantise=quantise, return_frames=True)
    assert np.array_equal(a.psnr, b.psnr) and np.array_equal(a.ssim, b.ssim)
    assert a.psnr_mean == b.psnr_mean and a.ssim_mean == b.ssim_mean
    assert np.array_equal(a.frames, b.frames)


def test_streamed_run_u8_equals_float_frames_with_a_quarter_of_the_upload():
    from fcvsr_amd.harness.infer import StreamedSuperResolver
    m = _model()
    seqs8 = [_seq(n, 18, 20, seed=10 + n) for n in (7, 5)]
    seqsf = [s.float() / 255 for s in seqs8]
    for world in (1, 2):
        for rank in range(world):
            r8 = StreamedSuperResolver(m, batch=4)
            got = r8.run(seqs8, rank=rank, world=world)
            rf = StreamedSuperResolver(m, batch=4)
            ref = rf.run(seqsf, rank=rank, world=world)
            assert got.keys() == ref.keys()
            for s in ref:
                assert got[s][0] == ref[s][0] and np.array_equal(got[s][1], ref[s][1])
            assert r8.stats["frames_uploaded"] == rf.stats["frames_uploaded"]
            assert 4 * r8.stats["h2d_bytes"] == rf.stats["h2d_bytes"]
            assert r8._bufs["ring"].dtype == torch.uint8 and r8._bufs["stage"][0].dtype == torch.uint8
    with pytest.raises(ValueError, match="uint8"):
        StreamedSuperResolver(m, batch=4).run([seqs8[0], seqsf[1]])


def _chroma_ref(planes_u8):
    y = F.interpolate(planes_u8.float()[:, None] / 255, scale_factor=4, mode="bicubic", align_corners=False)[:, 0]
    return (y.clamp(0, 1) * 255).round().to(torch.uint8)


def test_chroma_kernel_matches_torch_bicubic():
    from fcvsr_amd import hip
    rs = np.random.RandomState(4)
    # random planes, smooth planes and an odd-sized plane
    planes = [torch.from_numpy(rs.randint(0, 256, (3, 9, 11)).astype(np.uint8))]
    yy, xx = np.mgrid[0:24, 0:40]
    planes.append(torch.from_numpy(np.clip(128 + 100 * np.sin(yy / 5.0) * np.cos(xx / 7.0), 0, 255).astype(np.uint8))[None])
    planes.append(torch.from_numpy(rs.randint(0, 256, (1, 1, 5)).astype(np.uint8)))
    for p in planes:
        got = hip.chroma_up4(p.cuda()).cpu()
        ref = _chroma_ref(p)
        assert got.shape == ref.shape
        d = (got.int() - ref.int()).abs()
        assert int(d.max()) <= 1 and float(d.float().mean()) < 0.01, (int(d.max()), float(d.float().mean()))
    # exact on constant planes, every code value
    const = torch.arange(256, dtype=torch.uint8)[:, None, None].expand(256, 6, 8).contiguous()
    got = hip.chroma_up4(const.cuda()).cpu()
    assert torch.equal(got, const[:, :1, :1].expand(256, 24, 32))
    assert torch.equal(got, _chroma_ref(const))


def test_super_resolve_yuv420_file_to_file(tmp_path):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import parse_yuv_name, read_yuv420, super_resolve_yuv420, write_yuv420
    m = _model()
    N, H, W = 5, 18, 20                              # H padded to 20 inside
    rs = np.random.RandomState(5)
    y = rs.randint(0, 256, (N, H, W)).astype(np.uint8)
    u = rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8)
    v = rs.randint(0, 256, (N, H // 2, W // 2)).astype(np.uint8)
    src = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv")
    dst = str(tmp_path / f"Seq_{4 * W}x{4 * H}_{N}F.yuv")
    write_yuv420(src, y, u, v)
    info = parse_yuv_name(src)
    stats = super_resolve_yuv420(m, src, dst, info.width, info.height, batch=2)
    assert os.path.getsize(dst) == N * 16 * W * H * 3 // 2
    assert stats["frames"] == N and stats["bytes_written"] == os.path.getsize(dst)
    oy, ou, ov = read_yuv420(dst, 4 * W, 4 * H)
    ref_y = super_resolve_sequence(m, torch.from_numpy(y)[:, None], batch=3)
    assert np.array_equal(oy, ref_y[:, 0])
    assert np.array_equal(ou, hip.chroma_up4(torch.from_numpy(u).cuda()).cpu().numpy())
    assert np.array_equal(ov, hip.chroma_up4(torch.from_numpy(v).cuda()).cpu().numpy())
    # round mode follows the sequence path's round mode
    super_resolve_yuv420(m, src, dst, W, H, batch=4, quantise="round")
    ry, _, _ = read_yuv420(dst, 4 * W, 4 * H)
    assert np.array_equal(ry, super_resolve_sequence(m, torch.from_numpy(y)[:, None], batch=4, quantise="round")[:, 0])
