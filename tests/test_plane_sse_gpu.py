"""GPU: `hip.plane_sse` (fcvsr_plane_sse, csrc/plane_sse.hip) equals `harness.reference.plane_sse_host`, compared as integers, on
the smallest shapes that can break it: single samples, rows shorter than a 16-byte chunk, rows that end in a partial chunk, rows
off the 16-byte grid, several row tiles and several spans per plane, planes read in place inside an I420 batch buffer."""
import numpy as np
import pytest
import torch

from fcvsr_amd import hip
from fcvsr_amd.harness.reference import plane_sse_host

pytestmark = pytest.mark.gpu


def _pair(shape, dt, seed, top):
    rs = np.random.RandomState(seed)
    return rs.randint(0, top, shape).astype(dt), rs.randint(0, top, shape).astype(dt)


def _dev(a):
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def _check(a, b, crop):
    got = hip.plane_sse(_dev(a), _dev(b), crop)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (a.shape[0],)
    assert got.cpu().tolist() == plane_sse_host(a, b, crop).tolist(), (a.shape, a.dtype, crop)


@pytest.mark.parametrize("shape,dt,crop", [
    ((1, 1, 1), np.uint8, 0), ((1, 1, 1), np.uint16, 0),
    ((3, 18, 20), np.uint8, 0), ((3, 18, 20), np.uint8, 2),               # rows of 20 and 16 bytes that start off the 16-byte grid
    ((2, 9, 10), np.uint16, 0), ((2, 9, 10), np.uint16, 1),               # one chunk and a tail of 4 bytes; crop 1: exactly one chunk
    ((3, 6, 11), np.uint8, 0), ((2, 7, 7), np.uint16, 1),                 # rows shorter than a chunk: read sample by sample
    ((5, 37, 101), np.uint8, 4), ((5, 37, 101), np.uint16, 4),            # more than one row tile, a 13-byte / 10-byte tail
    ((2, 70, 300), np.uint8, 0), ((2, 70, 300), np.uint16, 0),            # several workgroups per plane (three row tiles)
    ((2, 33, 64), np.uint8, 0), ((2, 33, 32), np.uint16, 0),              # whole chunks only, everything on the 16-byte grid
    ((1, 3, 1100), np.uint8, 0), ((1, 3, 530), np.uint16, 1),             # two spans per row, the second one short
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_equals_the_host_contract(shape, dt, crop):
    top = 256 if dt == np.uint8 else 1536                                 # uint16 samples up to 1535 read as min(k, 1023)
    a, b = _pair(shape, dt, sum(shape) + crop, top)
    if dt == np.uint16:
        a.flat[0], b.flat[0] = 65535, 0                                   # the largest container value, the largest difference
    _check(a, b, crop)


def test_the_extremes_do_not_overflow_the_partial_sums():
    for dt, hi in ((np.uint8, 255), (np.uint16, 1023)):                   # every squared difference at its maximum, whole tiles
        a = np.full((1, 64, 1024 // np.dtype(dt).itemsize), hi, dtype=dt)
        got = hip.plane_sse(_dev(a), _dev(np.zeros_like(a)), 0)
        assert got.cpu().tolist() == [a.size * hi * hi]


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_the_planes_of_an_i420_batch_buffer_are_read_where_they_lie(dt):
    from fcvsr_amd.harness.colour import i420_planes
    N, H, W = 5, 18, 30                                                   # 810 samples per frame: every second uint8 frame lies
    fs = H * W * 3 // 2                                                   # off the 16-byte grid, and the frame stride exceeds a plane
    a, b = _pair((N, fs), dt, 7, 256 if dt == np.uint8 else 1536)
    ta, tb = _dev(a), _dev(b)
    hw, cw = H * W, (H // 2) * (W // 2)
    host = lambda x: (x[:, :hw].reshape(N, H, W), x[:, hw:hw + cw].reshape(N, H // 2, W // 2), x[:, hw + cw:].reshape(N, H // 2, W // 2))
    for k, (pa, pb) in enumerate(zip(i420_planes(ta, H, W), i420_planes(tb, H, W))):
        assert pa.data_ptr() == ta.data_ptr() + (0, hw, hw + cw)[k] * ta.element_size() and not pa.is_contiguous()
        for crop in (0, 2):
            got = hip.plane_sse(pa, pb, crop)
            assert got.cpu().tolist() == plane_sse_host(host(a)[k], host(b)[k], crop).tolist(), (k, crop)
    # a view against a separate dense tensor, a slice of a ring, and an odd start address
    y = i420_planes(ta, H, W)[0]
    dense = _dev(np.ascontiguousarray(host(b)[0]))
    assert hip.plane_sse(y, dense, 4).cpu().tolist() == plane_sse_host(host(a)[0], host(b)[0], 4).tolist()
    assert hip.plane_sse(y[1:4], dense[2:5], 0).cpu().tolist() == plane_sse_host(host(a)[0][1:4], host(b)[0][2:5], 0).tolist()
    flat_a, flat_b = a.reshape(-1), b.reshape(-1)
    oa, ob = hip.bits16(ta).reshape(-1)[1:1 + 2 * 7 * 23].reshape(2, 7, 23), hip.bits16(tb).reshape(-1)[3:3 + 2 * 7 * 23].reshape(2, 7, 23)
    want = plane_sse_host(flat_a[1:1 + 322].reshape(2, 7, 23), flat_b[3:3 + 322].reshape(2, 7, 23), 1)
    assert hip.plane_sse(oa, ob, 1).cpu().tolist() == want.tolist()


def test_int16_views_equal_planes_and_no_planes():
    a, b = _pair((3, 12, 21), np.uint16, 3, 1536)
    want = plane_sse_host(a, b, 2).tolist()
    ta, tb = _dev(a), _dev(b)
    assert hip.plane_sse(ta.view(torch.int16), tb.view(torch.int16), 2).cpu().tolist() == want
    assert hip.plane_sse(ta.view(torch.int16), tb, 2).cpu().tolist() == want
    assert hip.plane_sse(ta, ta.clone(), 0).cpu().tolist() == [0, 0, 0]
    c = np.minimum(a, 1023)                                               # equal once read as min(k, 1023)
    assert (c != a).any() and hip.plane_sse(ta, _dev(c), 0).cpu().tolist() == [0, 0, 0]
    u8 = _dev(_pair((2, 5, 5), np.uint8, 1, 256)[0])
    assert hip.plane_sse(u8, u8, 1).cpu().tolist() == [0, 0]
    empty = hip.plane_sse(u8[:0], u8[:0], 1)
    assert empty.dtype == torch.int64 and tuple(empty.shape) == (0,) and empty.is_cuda
    rows = u8[:, :, 1:4]                                                  # rows that are not dense: copied, then scored
    assert hip.plane_sse(rows, rows.flip(0), 0).cpu().tolist() == plane_sse_host(rows.cpu().numpy(), rows.flip(0).cpu().numpy(), 0).tolist()


def test_argument_errors():
    u8 = torch.zeros((2, 6, 8), dtype=torch.uint8, device="cuda")
    u16 = torch.zeros((2, 6, 8), dtype=torch.uint16, device="cuda")
    for a, b, crop in ((u8, u16, 0), (u8, u8[:, :5], 0), (u8, u8[:1], 0), (u8, u8, 3), (u8, u8, -1), (u8[0], u8[0], 0),
                       (u8.float(), u8.float(), 0), (u8.to(torch.int32), u8.to(torch.int32), 0)):
        with pytest.raises(ValueError):
            hip.plane_sse(a, b, crop)
    with pytest.raises(RuntimeError):
        hip.plane_sse(u8.cpu(), u8.cpu(), 0)
    out = torch.zeros((2,), dtype=torch.int64, device="cuda")
    scratch = torch.zeros((2,), dtype=torch.int64, device="cuda")
    call = lambda *v: hip.lib().fcvsr_plane_sse(*v, hip.stream_ptr())
    ok = (u8.data_ptr(), u8.data_ptr(), 1, 2, 6, 8, 48, 48, 0, scratch.data_ptr(), 16, out.data_ptr())
    assert call(*ok) == 0
    for k, bad in ((2, 4), (3, -1), (3, 65536), (4, 0), (5, (1 << 20) + 1), (6, -48), (8, 3), (8, -1), (9, 0), (9, scratch.data_ptr() + 4),
                   (10, 8), (11, 0), (11, out.data_ptr() + 4), (0, 0)):
        args = list(ok)
        args[k] = bad
        assert call(*args) == -1, (k, bad)                                # FCVSR_E_ARG, before any launch
    assert call(u16.data_ptr() + 1, u16.data_ptr(), 2, 2, 6, 8, 48, 48, 0, scratch.data_ptr(), 16, out.data_ptr()) == -1
    with pytest.raises(hip.HipError):
        hip.check(call(*ok[:2], 4, *ok[3:]), "fcvsr_plane_sse")
    torch.cuda.synchronize()
