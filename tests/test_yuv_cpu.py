"""CPU: the I420 reader / writer, the reference's Name_WxH_NF.yuv naming, and the argument errors of the uint8 and YUV entry
points that are raised before any device work."""
import os

import numpy as np
import pytest
import torch


def _planes(n, h, w, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 256, (n, h, w)).astype(np.uint8), rs.randint(0, 256, (n, h // 2, w // 2)).astype(np.uint8),
            rs.randint(0, 256, (n, h // 2, w // 2)).astype(np.uint8))


def test_write_read_round_trip(tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420, write_yuv420
    y, u, v = _planes(3, 6, 10)
    p = str(tmp_path / "seq_10x6_3F.yuv")
    write_yuv420(p, y, u, v)
    assert os.path.getsize(p) == 3 * 10 * 6 * 3 // 2
    ry, ru, rv = read_yuv420(p, 10, 6)
    assert ry.dtype == np.uint8 and ry.shape == (3, 6, 10) and ru.shape == (3, 3, 5) and rv.shape == (3, 3, 5)
    assert np.array_equal(ry, y) and np.array_equal(ru, u) and np.array_equal(rv, v)
    # frame order on disk: Y, U, V of frame 0, then frame 1, ...
    raw = np.fromfile(p, dtype=np.uint8)
    assert np.array_equal(raw[:60], y[0].ravel()) and np.array_equal(raw[60:75], u[0].ravel())
    assert np.array_equal(raw[75:90], v[0].ravel()) and np.array_equal(raw[90:150], y[1].ravel())
    fy, fu, fv = read_yuv420(p, 10, 6, frames=2)
    assert fy.shape == (2, 6, 10) and np.array_equal(fv, v[:2])
    # a single frame (H,W) is written as one frame
    write_yuv420(p, y[1], u[1], v[1])
    sy, su, sv = read_yuv420(p, 10, 6)
    assert sy.shape == (1, 6, 10) and np.array_equal(sy[0], y[1]) and np.array_equal(su[0], u[1])


def test_reader_does_not_copy(tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420, write_yuv420
    p = str(tmp_path / "a.yuv")
    write_yuv420(p, *_planes(2, 4, 4))
    y, u, v = read_yuv420(p, 4, 4)
    # views into one read-only mapping of the file, at the file's offsets: Y0 (16 bytes), U0 (4), V0 (4), Y1, ...
    assert u.ctypes.data == y.ctypes.data + 16 and v.ctypes.data == u.ctypes.data + 4
    assert y.strides == (24, 4, 1) and u.strides == (24, 2, 1)
    for a in (y, u, v):
        assert not a.flags.writeable and not a.flags.owndata


@pytest.mark.parametrize("name,expect", [
    ("Traffic_640x400_300F.yuv", ("Traffic", 640, 400, 300)),
    ("BasketballDrive_fps50_480x272_500F.yuv", ("BasketballDrive_fps50", 480, 272, 500)),
    ("Kimono1_fps24_480x272_240F.yuv", ("Kimono1_fps24", 480, 272, 240)),
    ("Traffic_2560x1600_30.yuv", ("Traffic", 2560, 1600, None)),
    ("BasketballDrive_1920x1080_50_500F.yuv", ("BasketballDrive", 1920, 1080, 500)),
    ("/data/test/KristenAndSara_320x184_600F.yuv", ("KristenAndSara", 320, 184, 600)),
])
def test_parse_reference_names(name, expect):
    from fcvsr_amd.harness.yuv import parse_yuv_name
    r = parse_yuv_name(name)
    assert (r.name, r.width, r.height, r.frames) == expect


def test_parse_rejects_names_without_a_size():
    from fcvsr_amd.harness.yuv import parse_yuv_name
    with pytest.raises(ValueError, match="WxH"):
        parse_yuv_name("Traffic_300F.yuv")


def test_reader_and_writer_errors(tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420, write_yuv420
    p = str(tmp_path / "b.yuv")
    write_yuv420(p, *_planes(2, 4, 6))
    with pytest.raises(ValueError, match="even"):
        read_yuv420(p, 5, 4)
    with pytest.raises(ValueError, match="even"):
        read_yuv420(p, 6, 3)
    with pytest.raises(ValueError, match="whole number"):
        read_yuv420(p, 8, 4)                       # 72 bytes, 48-byte frames
    with pytest.raises(ValueError, match="holds 2"):
        read_yuv420(p, 6, 4, frames=5)
    with open(p, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="whole number"):
        read_yuv420(p, 6, 4)
    y, u, v = _planes(1, 4, 6)
    with pytest.raises(ValueError, match="uint8"):
        write_yuv420(p, y.astype(np.uint16), u, v)
    with pytest.raises(ValueError, match="chroma"):
        write_yuv420(p, y, u[:, :1], v[:, :1])
    with pytest.raises(ValueError, match="even"):
        write_yuv420(p, y[:, :3], u, v)


def test_super_resolve_yuv420_rejects_colour_models_and_bad_files(tmp_path):
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    p = str(tmp_path / "c_6x4_2F.yuv")
    write_yuv420(p, *_planes(2, 4, 6))
    with pytest.raises(ValueError, match="C=3"):
        super_resolve_yuv420(FCVSR_SNet(), p, str(tmp_path / "o.yuv"), 6, 4)
    with pytest.raises(ValueError, match="even"):
        super_resolve_yuv420(GShiftNet_S(), p, str(tmp_path / "o.yuv"), 5, 4)
    with pytest.raises(ValueError, match="whole number"):
        super_resolve_yuv420(GShiftNet_S(), p, str(tmp_path / "o.yuv"), 8, 4)
    with pytest.raises(ValueError, match="quantise"):
        super_resolve_yuv420(GShiftNet_S(), p, str(tmp_path / "o.yuv"), 6, 4, quantise="nearest")


def test_super_resolve_u8_argument_errors_without_a_device():
    """The same errors as forward for host tensors; ValueError for a wrong dtype or quantise mode; ETC is out of scope."""
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_ETC, GShiftNet_S
    m = GShiftNet_S()
    x8 = torch.zeros(1, 7, 1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.super_resolve_u8(x8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x8.float())
    with pytest.raises(ValueError, match="uint8"):
        m.super_resolve_u8(x8.float())
    with pytest.raises(ValueError, match="quantise"):
        m.super_resolve_u8(x8, quantise="floor")
    with pytest.raises(ValueError, match="quantise"):
        m.super_resolve_u8(x8, quantise=None)
    with pytest.raises(NotImplementedError):
        GShiftNet_ETC().super_resolve_u8(torch.zeros(1, 13, 1, 8, 8, dtype=torch.uint8))
