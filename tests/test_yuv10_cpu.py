"""No GPU: 10-bit YUV 4:2:0 files (two bytes per sample, little-endian), the `_10bit` file-name token, and the `peak` keyword of
the CPU metrics."""
import numpy as np
import pytest
import torch


def _planes10(n, h, w, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 1024, (n, h, w)).astype(np.uint16), rs.randint(0, 1024, (n, h // 2, w // 2)).astype(np.uint16),
            rs.randint(0, 1024, (n, h // 2, w // 2)).astype(np.uint16))


def test_10bit_round_trip_and_byte_order(tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420, write_yuv420
    y, u, v = _planes10(3, 4, 6)
    y[0, 0, 0], y[0, 0, 1], u[0, 0, 0], v[2, -1, -1] = 1023, 0x0102, 0x0301, 1023
    p = str(tmp_path / "a_6x4_3F_10bit.yuv")
    write_yuv420(p, y, u, v)
    raw = open(p, "rb").read()
    assert len(raw) == 3 * (6 * 4 * 3 // 2) * 2
    assert raw[:4] == b"\xff\x03\x02\x01"                        # 1023, then 0x0102: low byte first
    assert raw[48:50] == b"\x01\x03" and raw[-2:] == b"\xff\x03"
    ry, ru, rv = read_yuv420(p, 6, 4, bit_depth=10)
    assert ry.dtype == np.dtype("<u2") and ry.shape == (3, 4, 6) and ru.shape == (3, 2, 3)
    assert np.array_equal(ry, y) and np.array_equal(ru, u) and np.array_equal(rv, v)
    assert isinstance(ry.base, np.memmap) or isinstance(ry, np.memmap) or isinstance(getattr(ry.base, "base", None), np.memmap)
    y2, _, _ = read_yuv420(p, 6, 4, frames=2, bit_depth=10)
    assert y2.shape == (2, 4, 6) and np.array_equal(y2, y[:2])
    # a hand-built file: one 2x2 frame with Y = 1, 2, 3, 1023 and U = 512, V = 4
    q = str(tmp_path / "b.yuv")
    with open(q, "wb") as f:
        f.write(bytes([1, 0, 2, 0, 3, 0, 0xFF, 0x03, 0x00, 0x02, 4, 0]))
    hy, hu, hv = read_yuv420(q, 2, 2, bit_depth=10)
    assert hy.tolist() == [[[1, 2], [3, 1023]]] and hu.tolist() == [[[512]]] and hv.tolist() == [[[4]]]
    # single frames are accepted as for 8-bit
    write_yuv420(q, y[0], u[0], v[0])
    sy, _, _ = read_yuv420(q, 6, 4, bit_depth=10)
    assert np.array_equal(sy[0], y[0])
    # the same bytes read as 8-bit are twice as many frames
    assert read_yuv420(p, 6, 4)[0].shape == (6, 4, 6)


def test_10bit_reader_and_writer_errors(tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420, write_yuv420
    y, u, v = _planes10(1, 4, 6)
    p = str(tmp_path / "c.yuv")
    write_yuv420(p, (y >> 2).astype(np.uint8), (u >> 2).astype(np.uint8), (v >> 2).astype(np.uint8))      # 36 bytes
    with pytest.raises(ValueError, match="whole number"):
        read_yuv420(p, 6, 4, bit_depth=10)                       # 72-byte frames
    with pytest.raises(ValueError, match="bit_depth"):
        read_yuv420(p, 6, 4, bit_depth=12)
    write_yuv420(p, y, u, v)
    with pytest.raises(ValueError, match="holds 1"):
        read_yuv420(p, 6, 4, frames=2, bit_depth=10)
    for planes in ((y, u.astype(np.uint8), v), (y.astype(np.uint8), u, v), (y, u, v.astype(np.uint8))):
        with pytest.raises(ValueError, match="uint8"):
            write_yuv420(p, *planes)
    with pytest.raises(ValueError, match="uint8"):
        write_yuv420(p, y.astype(np.int16), u.astype(np.int16), v.astype(np.int16))


def test_yuv_bit_depth_from_the_file_name():
    from fcvsr_amd.harness.yuv import parse_yuv_name, yuv_bit_depth
    assert yuv_bit_depth("MarketPlace_1920x1080_60fps_10bit_420.yuv") == 10
    assert yuv_bit_depth("/data/x/Tango2_3840x2160_60fps_10BIT.yuv") == 10
    assert yuv_bit_depth("a_10Bit.yuv") == 10
    assert yuv_bit_depth("Traffic_640x400_300F.yuv") == 8
    assert yuv_bit_depth("/clips_10bit/Traffic_640x400_300F.yuv") == 8          # the directory does not count
    assert yuv_bit_depth("Seq_110bit_640x400.yuv") == 8 and yuv_bit_depth("Seq_10bits_640x400.yuv") == 8
    r = parse_yuv_name("MarketPlace_1920x1080_60fps_10bit_420.yuv")             # the 4-tuple is what it was
    assert tuple(r) == ("MarketPlace", 1920, 1080, None)


def test_super_resolve_yuv420_rejects_other_bit_depths(tmp_path):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_ETC, GShiftNet_S
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    p = str(tmp_path / "d_6x4_1F.yuv")
    write_yuv420(p, *_planes10(1, 4, 6))
    with pytest.raises(ValueError, match="bit_depth"):
        super_resolve_yuv420(GShiftNet_S(), p, str(tmp_path / "o.yuv"), 6, 4, bit_depth=12)
    m = GShiftNet_S()
    x16 = torch.zeros(1, 7, 1, 8, 8, dtype=torch.int16).view(torch.uint16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.super_resolve_u16(x16)
    with pytest.raises(ValueError, match="uint16"):
        m.super_resolve_u16(x16.view(torch.int16))
    with pytest.raises(ValueError, match="quantise"):
        m.super_resolve_u16(x16, quantise="floor")
    with pytest.raises(NotImplementedError):
        GShiftNet_ETC().super_resolve_u16(torch.zeros(1, 13, 1, 8, 8, dtype=torch.int16).view(torch.uint16))


def test_metrics_peak_keyword():
    from fcvsr_amd.harness.metrics import psnr, ssim
    rs = np.random.RandomState(1)
    a = rs.randint(0, 256, (40, 48)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + rs.randint(-6, 7, a.shape), 0, 255).astype(np.uint8)
    a4, b4 = a.astype(np.uint16) * 4, b.astype(np.uint16) * 4
    # scaling both images and the peak by 4 changes nothing: (4a, 4b) at 1020 is (a, b) at 255
    assert abs(psnr(a4, b4, peak=1020) - psnr(a, b)) <= 1e-12
    assert abs(ssim(a4, b4, peak=1020) - ssim(a, b)) <= 1e-12
    # full scale 1023 moves PSNR by 20 log10(1023 / 1020) and changes the SSIM constants
    assert abs(psnr(a4, b4, peak=1023) - psnr(a4, b4, peak=1020) - 20 * np.log10(1023 / 1020)) <= 1e-12
    assert ssim(a4, b4, peak=1023) != ssim(a4, b4, peak=1020)
    assert abs(ssim(a4, b4, peak=1023) - ssim(a4, b4, peak=1020)) < 1e-3
    # defaults are unchanged
    assert psnr(a, b) == psnr(a, b, 4, 255.0) == float(20.0 * np.log10(255.0 / np.sqrt(np.mean((a[4:-4, 4:-4].astype(np.float64)
                                                                                               - b[4:-4, 4:-4]) ** 2))))
    assert ssim(a, b) == ssim(a, b, 4, "HWC", None, 255.0)
    assert psnr(a, a, peak=1023) == float("inf")
    with pytest.raises(ValueError):
        ssim(np.stack([a4] * 3, -1), np.stack([b4] * 3, -1), convert_to="Y", peak=1023)


def test_10bit_table_values_round_trip_and_stay_distinct_in_f16():
    """What the 1023 divisor rests on: k -> k / 1023 -> * 1023 -> truncate (or round) returns k for all 1024 values in f32, and the
    values stay distinct in f16, the type the dedicated first layer builds its im2col tile in."""
    from fcvsr_amd import hip
    assert hip.PEAK10 == 1023 and hip.U16 == 4 and hip._DT[torch.uint16] == hip.U16
    k = torch.arange(1024, dtype=torch.int32)
    t = k.float() / 1023
    assert t.dtype == torch.float32 and float(t[0]) == 0.0 and float(t[-1]) == 1.0
    q = t.clamp(0, 1) * 1023.0
    assert torch.equal(q.to(torch.int32), k) and torch.equal(q.round().to(torch.int32), k)
    h = t.to(torch.float16)
    assert torch.unique(h).numel() == 1024 and bool((h[1:] > h[:-1]).all())
