"""GPU: `hip.frame_line_sums` and `hip.active_compose` equal their host contracts (`harness.active.line_sums_host`,
`compose_host`) exactly."""
import numpy as np
import pytest
import torch

from fcvsr_amd import hip
from fcvsr_amd.harness import active as A

pytestmark = pytest.mark.gpu


def _dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _frames(dtype, shape, seed=0, over=False):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rs.randint(0, 256, shape).astype(np.uint8)
    f = rs.randint(0, 1024, shape)
    if over:                                                              # a third of the samples lie above 1023: read as 1023
        f = np.where(rs.rand(*shape) < 1 / 3, rs.randint(1024, 65536, shape), f)
    return f.astype(np.uint16)


def _check_sums(t: torch.Tensor, host: np.ndarray):
    rows, cols = hip.frame_line_sums(t)
    want_r, want_c = A.line_sums_host(host)
    assert rows.dtype == torch.int64 and cols.dtype == torch.int64
    assert tuple(rows.shape) == want_r.shape and tuple(cols.shape) == want_c.shape
    assert np.array_equal(rows.cpu().numpy().astype(np.uint64), want_r)
    assert np.array_equal(cols.cpu().numpy().astype(np.uint64), want_c)


def _tile_shape(dtype):
    """H = two row tiles + 1, W = one workgroup's column span + 1."""
    return 2, 2, 2 * hip.LINE_SUMS_ROWS + 1, hip.LINE_SUMS_SPAN_BYTES // np.dtype(dtype).itemsize + 1


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 1, 6, 10), (2, 3, 9, 37), (2, 1, 20, 130), "tiles"], ids=str)
def test_line_sums_equal_the_host_sums(dtype, shape):
    shape = _tile_shape(dtype) if shape == "tiles" else shape
    f = _frames(dtype, shape, seed=sum(shape), over=shape == (2, 1, 20, 130))
    if dtype == np.uint16 and shape == (2, 1, 20, 130):
        assert 0.25 < (f > 1023).mean() < 0.42
    _check_sums(_dev(f), f)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_line_sums_off_the_16_byte_grid_and_of_the_int16_view(dtype):
    shape = (2, 2, 35, 70)
    f = _frames(dtype, shape, seed=7, over=True)
    flat = _dev(np.concatenate([np.zeros((1,), dtype), f.reshape(-1)]))
    x = hip.bits16(flat)[1:].view(flat.dtype).view(shape)                  # starts one sample after an aligned address
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    _check_sums(x, f)
    if dtype == np.uint16:
        _check_sums(hip.bits16(_dev(f)), f)
    saturated = np.full((1, 2, 33, 70), 255 if dtype == np.uint8 else 65535, dtype)      # the largest sums
    _check_sums(_dev(saturated), saturated)
    many = np.full((1, 70, 33, 21), 255 if dtype == np.uint8 else 1023, dtype)            # more channels than one flush of the byte sums
    _check_sums(_dev(many), many)


CASES = {                                                                 # (true H, W), resident (h, w), box
    "middle": ((12, 16), (12, 16), (4, 8, 4, 12)),
    "corner": ((12, 16), (12, 16), (0, 8, 0, 16)),
    "whole": ((12, 16), (12, 16), (0, 12, 0, 16)),
    "resident": ((10, 14), (12, 16), (2, 10, 3, 11)),
}


def _compose_case(dtype, case, seed):
    (H, W), (h, w), box = CASES[case]
    rs = np.random.RandomState(seed)
    N, C, centres = 5, 2, [3, 0, 4]
    t, b, l, r = box
    if dtype == np.float32:
        lr = rs.rand(N, C, h, w).astype(np.float32)
        sr = (rs.rand(3, C, 4 * (b - t) + 3, 4 * (r - l) + 8) * 1.2 - 0.1).astype(np.float32)
    else:
        lr = _frames(dtype, (N, C, h, w), seed, over=True)
        sr = _frames(dtype, (3, C, 4 * (b - t) + 3, 4 * (r - l) + 8), seed + 1)
    return lr, sr, centres, box, H, W


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_compose_equals_the_host_composition(dtype, case):
    lr, sr, centres, box, H, W = _compose_case(dtype, case, 11 + len(case))
    t, b, l, r = box
    hb, wb = 4 * (b - t), 4 * (r - l)
    lr_d, sr_d = _dev(lr), _dev(sr)
    want_lr = lr[centres][:, :, :H, :W]
    # a dense sr_box, and views of a larger tensor: two whose rows stay aligned to four samples, one that starts off that grid
    for oy, ox, dense in ((0, 0, True), (0, 0, False), (3, 5, False), (1, 4, False)):
        host = np.ascontiguousarray(sr[:, :, oy:oy + hb, ox:ox + wb])
        view = hip.bits16(sr_d)[:, :, oy:oy + hb, ox:ox + wb]
        view = (view.contiguous() if dense else view).view(sr_d.dtype)
        assert view.is_contiguous() == dense
        got = hip.active_compose(view, lr_d, centres, box, H, W)
        want = A.compose_host(host, want_lr, box)
        assert tuple(got.shape) == (3, 2, 4 * H, 4 * W) and got.dtype == lr_d.dtype
        got = hip.frames_to_numpy(got)
        assert got.dtype == want.dtype and np.array_equal(got, want), (case, oy, ox, dense)
    if case == "whole":
        assert np.array_equal(got, host)


def test_compose_validates_before_it_launches():
    lr, sr, centres, box, H, W = _compose_case(np.uint8, "middle", 1)
    lr_d, sr_d = _dev(lr), _dev(np.ascontiguousarray(sr[:, :, :16, :32]))
    for kw in ({"centres": [3, 0, 5]}, {"centres": [3, 0]}, {"box": (4, 8, 4, 13)}, {"box": (4, 4, 4, 12)}, {"H": 13}):
        args = dict(centres=centres, box=box, H=H, W=W)
        args.update(kw)
        with pytest.raises(ValueError):
            hip.active_compose(sr_d, lr_d, args["centres"], args["box"], args["H"], args["W"])
    with pytest.raises(ValueError):
        hip.active_compose(sr_d.float(), lr_d, centres, box, H, W)
    with pytest.raises(RuntimeError):
        hip.active_compose(sr_d.cpu(), lr_d.cpu(), centres, box, H, W)
    with pytest.raises(RuntimeError):
        hip.frame_line_sums(lr_d.cpu())
    with pytest.raises(ValueError):
        hip.frame_line_sums(lr_d.float())
