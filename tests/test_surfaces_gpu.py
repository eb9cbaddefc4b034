"""GPU: `fcvsr_surface_unpack` / `fcvsr_surface_pack` equal the host contract (`harness.surfaces`) bit for bit, for every format,
at row and frame sizes that put rows on every phase of the 16-byte grid, and never write outside a frame."""
import numpy as np
import pytest
import torch

from fcvsr_amd.harness import surfaces as sf

pytestmark = pytest.mark.gpu

# (n, H, W, Hp, Wp): 2x2, nothing but scalar tails; 18x10, 270-byte frames on odd phases and a 9-sample chroma row, ring rows padded
# to 12 x 20; 20x18 with Hp = 20, several 16-byte chunks per row; 72x36, whole chunks, heads and tails in one row, unpadded
SHAPES = [(2, 2, 2, 4, 4), (3, 10, 18, 12, 20), (5, 18, 20, 20, 20), (2, 36, 72, 36, 72)]
SLOTS = [5, 0, 3, 6, 1]
R = 7


def _dev(a: np.ndarray) -> torch.Tensor:
    """Host samples on the device in their dtype (uint16 travels as int16 bits)."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _host(t: torch.Tensor) -> np.ndarray:
    from fcvsr_amd import hip
    return hip.frames_to_numpy(t)


def _raw(fmt, n, w, h, seed):
    """Random frames as bytes.  8-bit: every byte value.  Planar 10-bit: words up to 1535, a third above 1023.  P010: every bit of
    every word, the low six included."""
    rs = np.random.RandomState(seed)
    if fmt == "yuv420p10le":
        return rs.randint(0, 1536, n * w * h * 3 // 2).astype("<u2").view(np.uint8)
    return rs.randint(0, 256, n * sf.frame_bytes(fmt, w, h)).astype(np.uint8)


def _rings(fmt, Hp, Wp, h, w, fill):
    dt = np.uint8 if sf.bit_depth(fmt) == 8 else np.uint16
    return [_dev(np.full(s, fill, dtype=dt)) for s in ((R, 1, Hp, Wp), (R, h // 2, w // 2), (R, h // 2, w // 2))]


@pytest.mark.parametrize("fmt", sf.PIX_FMTS)
@pytest.mark.parametrize("n,h,w,Hp,Wp", SHAPES)
def test_unpack_equals_the_host_contract(fmt, n, h, w, Hp, Wp):
    from fcvsr_amd import hip
    raw = _raw(fmt, n, w, h, seed=h + w)
    y, u, v = sf.unpack_host(raw, fmt, w, h)
    if fmt == "yuv420p10le":
        assert int(y.max()) > 1023                                        # passes through unchanged
    slots = SLOTS[:n]
    ry, ru, rv = _rings(fmt, Hp, Wp, h, w, 0)
    hip.surface_unpack(torch.from_numpy(raw).cuda(), fmt, w, h, torch.tensor(slots, dtype=torch.int32).cuda(), ry, ru, rv)
    gy, gu, gv = _host(ry), _host(ru), _host(rv)
    want_y, want_u, want_v = np.zeros_like(gy), np.zeros_like(gu), np.zeros_like(gv)
    for i, s in enumerate(slots):
        want_y[s, 0, :h, :w], want_u[s], want_v[s] = y[i], u[i], v[i]
    assert np.array_equal(gy, want_y) and np.array_equal(gu, want_u) and np.array_equal(gv, want_v)
    # a second pass of all-ones frames into the same slots: the padding stays zero, the other slots stay as they are
    ones = sf.pack_host(*(np.ones_like(a) for a in (y, u, v)), fmt)
    hip.surface_unpack(torch.from_numpy(np.frombuffer(ones, dtype=np.uint8).copy()).cuda(), fmt, w, h,
                       torch.tensor(slots, dtype=torch.int32).cuda(), ry, ru, rv)
    gy, gu, gv = _host(ry), _host(ru), _host(rv)
    for s in range(R):
        inside = 1 if s in slots else 0
        assert (gy[s, 0, :h, :w] == inside).all() and (gu[s] == inside).all() and (gv[s] == inside).all()
        assert not gy[s, 0, h:].any() and not gy[s, 0, :, w:].any()


@pytest.mark.parametrize("fmt", sf.PIX_FMTS)
@pytest.mark.parametrize("n,h,w,Hp,Wp", SHAPES)
def test_pack_equals_the_host_contract(fmt, n, h, w, Hp, Wp):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.colour import i420_planes
    dt = np.uint8 if sf.bit_depth(fmt) == 8 else np.uint16
    rs = np.random.RandomState(h * w)
    y, u, v = (rs.randint(0, 256 if dt == np.uint8 else 1024, s).astype(dt) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)))
    want = np.frombuffer(sf.pack_host(y, u, v, fmt), dtype=np.uint8).reshape(n, -1)
    uv = _dev(np.concatenate([u, v], 0))                                  # as chroma_up4 / imresize return them: b U planes, then b V
    got = hip.surface_pack(_dev(y), uv[:n], uv[n:], fmt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, sf.frame_bytes(fmt, w, h)) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    if fmt == "p010le":
        assert not (got.cpu().numpy().view("<u2") & 0x3f).any()
    # the planes of a batch of I420 frames (what colour.rgb_to_i420 returns), read where they lie
    frames = _dev(np.concatenate([a.reshape(n, -1) for a in (y, u, v)], 1))
    assert np.array_equal(hip.surface_pack(*i420_planes(frames, h, w), fmt).cpu().numpy(), want)
    # and a luma crop whose frames are not dense
    pad = _dev(np.pad(y, ((0, 0), (0, 2), (0, 4))))
    assert np.array_equal(hip.surface_pack(pad[:, :h, :w], uv[:n], uv[n:], fmt).cpu().numpy(), want)


def test_bad_input_raises():
    from fcvsr_amd import hip
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    z16 = lambda *s: torch.zeros(s, dtype=torch.int16, device="cuda").view(torch.uint16)
    slots = torch.zeros(1, dtype=torch.int32, device="cuda")
    rings = (z8(R, 1, 4, 4), z8(R, 1, 1), z8(R, 1, 1))
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(6), "i420", 2, 2, slots, *rings)
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(6), "nv12", 3, 2, slots, *rings)
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(7), "nv12", 2, 2, slots, *rings)            # no whole frame per slot
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(12), "p010le", 2, 2, slots, *rings)         # uint8 rings for a 10-bit format
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(6), "nv12", 2, 2, slots.long(), *rings)
    with pytest.raises(ValueError):
        hip.surface_unpack(z8(6), "nv12", 2, 2, slots, z8(R, 1, 1, 4), rings[1], rings[2])    # a ring smaller than the frame
    with pytest.raises(RuntimeError):
        hip.surface_unpack(z8(6).cpu(), "nv12", 2, 2, slots, *rings)
    with pytest.raises(RuntimeError):
        hip.surface_unpack(z8(6), "nv12", 2, 2, slots, rings[0].cpu(), rings[1], rings[2])
    with pytest.raises(ValueError):
        hip.surface_pack(z8(1, 2, 2), z8(1, 1, 1), z8(1, 1, 1), "yuv444p")
    with pytest.raises(ValueError):
        hip.surface_pack(z16(1, 2, 2), z16(1, 1, 1), z16(1, 1, 1), "nv12")
    with pytest.raises(ValueError):
        hip.surface_pack(z8(1, 2, 2), z8(1, 1, 1), z8(1, 1, 1), "p010le")
    with pytest.raises(ValueError):
        hip.surface_pack(z8(1, 2, 2), z8(1, 2, 1), z8(1, 2, 1), "nv12")
    with pytest.raises(ValueError):
        hip.surface_pack(torch.zeros(1, 2, 2, device="cuda"), z8(1, 1, 1), z8(1, 1, 1), "nv12")
    with pytest.raises(RuntimeError):
        hip.surface_pack(z8(1, 2, 2).cpu(), z8(1, 1, 1), z8(1, 1, 1), "nv12")
    # a slot number outside the ring writes nothing
    out = (z8(R, 1, 2, 2), z8(R, 1, 1), z8(R, 1, 1))
    hip.surface_unpack(z8(6) + 9, "nv12", 2, 2, torch.tensor([R], dtype=torch.int32, device="cuda"), *out)
    assert not any(t.any().item() for t in out)
