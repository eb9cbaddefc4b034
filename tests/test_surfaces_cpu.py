"""CPU: the host contract of the raw 4:2:0 surface formats (`harness.surfaces`), the specification of csrc/surface.hip."""
import numpy as np
import pytest

from fcvsr_amd.harness import surfaces as sf


def _raw(fmt, n, w, h, seed):
    """n random frames of `fmt` as bytes: every bit of every byte is used, the low six bits of P010 words included."""
    return np.random.RandomState(seed).randint(0, 256, n * sf.frame_bytes(fmt, w, h)).astype(np.uint8)


def test_the_format_list_and_frame_bytes():
    assert sf.PIX_FMTS == ("yuv420p", "yuv420p10le", "nv12", "p010le")
    assert [sf.bit_depth(f) for f in sf.PIX_FMTS] == [8, 10, 8, 10]
    assert sf.frame_bytes("yuv420p", 18, 10) == 270 and sf.frame_bytes("nv12", 18, 10) == 270
    assert sf.frame_bytes("yuv420p10le", 18, 10) == 540 and sf.frame_bytes("p010le", 18, 10) == 540
    assert sf.frame_bytes("nv12", 1920, 1080) == 3110400 and sf.frame_bytes("p010le", 2, 2) == 12


@pytest.mark.parametrize("fmt", sf.PIX_FMTS)
@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (3, 10, 18), (2, 36, 72)])
def test_pack_of_unpack_gives_the_bytes_back(fmt, n, h, w):
    raw = _raw(fmt, n, w, h, seed=n + w)
    y, u, v = sf.unpack_host(raw, fmt, w, h)
    dt = np.uint8 if sf.bit_depth(fmt) == 8 else np.uint16
    assert y.dtype == dt and u.dtype == dt and v.dtype == dt
    assert y.shape == (n, h, w) and u.shape == (n, h // 2, w // 2) and v.shape == (n, h // 2, w // 2)
    want = raw
    if fmt == "p010le":                                                   # the low six bits are dropped on the way in
        want = (raw.view("<u2") & 0xffc0).astype("<u2").view(np.uint8)
        assert int(max(y.max(), u.max(), v.max())) <= 1023
    back = sf.pack_host(y, u, v, fmt)
    assert isinstance(back, bytes) and back == want.tobytes()
    assert sf.unpack_host(back, fmt, w, h)[1].tolist() == u.tolist()      # bytes are taken as well as arrays


def test_nv12_by_hand():
    # 4x2: Y rows 0..3, 4..7; one chroma row U0 V0 U1 V1
    raw = np.array([0, 1, 2, 3, 4, 5, 6, 7, 100, 200, 101, 201], dtype=np.uint8)
    y, u, v = sf.unpack_host(raw, "nv12", 4, 2)
    assert y.tolist() == [[[0, 1, 2, 3], [4, 5, 6, 7]]] and u.tolist() == [[[100, 101]]] and v.tolist() == [[[200, 201]]]
    assert sf.pack_host(y, u, v, "nv12") == raw.tobytes()
    assert sf.pack_host(y, u, v, "yuv420p") == bytes([0, 1, 2, 3, 4, 5, 6, 7, 100, 101, 200, 201])
    # 2x2, two frames
    raw = np.array([9, 8, 7, 6, 50, 60, 1, 2, 3, 4, 70, 80], dtype=np.uint8)
    y, u, v = sf.unpack_host(raw, "nv12", 2, 2)
    assert y.tolist() == [[[9, 8], [7, 6]], [[1, 2], [3, 4]]] and u.tolist() == [[[50]], [[70]]] and v.tolist() == [[[60]], [[80]]]


def test_p010_by_hand():
    # 2x2: the value sits in the high ten bits, little-endian; the second Y word carries junk in its low six bits
    words = [1023 << 6, (513 << 6) | 0x2a, 0 << 6, 1 << 6, 512 << 6, (64 << 6) | 0x3f]
    raw = np.array(words, dtype="<u2").view(np.uint8)
    assert raw[:4].tolist() == [0xc0, 0xff, 0x6a, 0x80]
    y, u, v = sf.unpack_host(raw, "p010le", 2, 2)
    assert y.dtype == np.uint16 and y.tolist() == [[[1023, 513], [0, 1]]] and u.tolist() == [[[512]]] and v.tolist() == [[[64]]]
    back = np.frombuffer(sf.pack_host(y, u, v, "p010le"), dtype="<u2")
    assert back.tolist() == [1023 << 6, 513 << 6, 0, 1 << 6, 512 << 6, 64 << 6]
    # 4x2: chroma U0 V0 U1 V1 in words
    words = [w << 6 for w in (1, 2, 3, 4, 5, 6, 7, 8)] + [(300 << 6) | 1, 400 << 6, 301 << 6, (401 << 6) | 0x20]
    y, u, v = sf.unpack_host(np.array(words, dtype="<u2").view(np.uint8), "p010le", 4, 2)
    assert y.tolist() == [[[1, 2, 3, 4], [5, 6, 7, 8]]] and u.tolist() == [[[300, 301]]] and v.tolist() == [[[400, 401]]]
    assert np.frombuffer(sf.pack_host(y, u, v, "yuv420p10le"), dtype="<u2").tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 300, 301, 400, 401]


@pytest.mark.parametrize("fmt,bits", [("yuv420p", 8), ("yuv420p10le", 10)])
def test_planar_unpacking_is_read_yuv420(fmt, bits, tmp_path):
    from fcvsr_amd.harness.yuv import read_yuv420
    raw = _raw(fmt, 3, 18, 10, seed=bits)                                 # 10-bit: words up to 65535 pass through unchanged
    path = str(tmp_path / "a.yuv")
    raw.tofile(path)
    got, want = sf.unpack_host(raw, fmt, 18, 10), read_yuv420(path, 18, 10, bit_depth=bits)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype.newbyteorder("=") and a.tolist() == np.asarray(b).tolist()
    if bits == 10:
        assert int(got[0].max()) > 1023


def test_bad_sizes_formats_and_planes_raise():
    for w, h in [(3, 2), (2, 3), (0, 2), (2, -2)]:
        with pytest.raises(ValueError):
            sf.frame_bytes("nv12", w, h)
    for fn in (lambda: sf.frame_bytes("yuv422p", 2, 2), lambda: sf.bit_depth("NV12"),
               lambda: sf.unpack_host(np.zeros(6, np.uint8), "i420", 2, 2),
               lambda: sf.pack_host(*(np.zeros((1, 2, 2), np.uint8),) + (np.zeros((1, 1, 1), np.uint8),) * 2, "nv21")):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        sf.unpack_host(np.zeros(7, np.uint8), "nv12", 2, 2)               # no whole number of frames
    with pytest.raises(ValueError):
        sf.pack_host(np.zeros((1, 2, 2), np.uint16), np.zeros((1, 1, 1), np.uint16), np.zeros((1, 1, 1), np.uint16), "nv12")
    with pytest.raises(ValueError):
        sf.pack_host(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 2, 1), np.uint8), np.zeros((1, 2, 1), np.uint8), "nv12")
