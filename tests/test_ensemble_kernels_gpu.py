"""GPU, kernel level (no model): the self-ensemble's window gather and merge kernels (csrc/ensemble.hip) against their host
specification (fcvsr_amd/harness/ensemble.py).  Everything is exact data movement or a fixed-order f32 sum: no tolerances."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N,C,h,w), index rows (b,T): repeated and out-of-order frame numbers, as edge padding and `centres` give
CASES = {
    # odd frame size: frames start at 2 mod 4 bytes (uint8) and at odd samples; both sides need padding; a single tile
    "18x21": ((5, 3, 18, 21), [[0, 0, 0, 1, 2, 3, 4], [4, 3, 1, 1, 0, 2, 2]]),
    # crosses the 64-wide tile with a ragged tail; the transposed variants cross it by rows
    "36x70": ((3, 1, 36, 70), [[0, 0, 0, 0, 1, 2, 2], [2, 1, 0, 2, 1, 0, 1]]),
}
DTYPES = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}


def _ceil4(v):
    return (v + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _source(case, kind):
    """The sequence (host, its own dtype) and the floats the kernels must read from it (host f32)."""
    from fcvsr_amd import hip
    shape, _ = CASES[case]
    rs = np.random.RandomState(len(case) + 7 * len(kind))
    if kind == "f32":
        src = torch.from_numpy(rs.rand(*shape).astype(np.float32))
        return src, src
    if kind == "u8":
        src = torch.from_numpy(rs.randint(0, 256, shape).astype(np.uint8))
        return src, hip.u8_table("cuda").cpu()[src.long()]
    a = rs.randint(0, 1024, shape)
    a.reshape(-1)[::5] = rs.randint(1024, 65536, a.reshape(-1)[::5].shape)          # samples above 1023 read as 1023
    src = torch.from_numpy(a.astype(np.uint16).view(np.int16)).view(torch.uint16)
    return src, hip.u16_table("cuda").cpu()[torch.from_numpy(np.minimum(a, 1023))]


@functools.lru_cache(maxsize=None)
def _expected_windows(case, kind, reverse):
    from fcvsr_amd.harness.ensemble import variant_host
    _, rows = CASES[case]
    _, vals = _source(case, kind)
    win = vals[torch.tensor(rows)]                                                  # (b,T,C,h,w)
    win = win.flip(1) if reverse else win
    out = []
    for i in range(8):
        v = variant_host(win, i)
        out.append(F.pad(v, (0, (-v.shape[-1]) % 4, 0, (-v.shape[-2]) % 4)))
    return torch.stack(out[:4]), torch.stack(out[4:])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("case", list(CASES))
def test_window_gather_equals_host_variants(case, kind, reverse):
    from fcvsr_amd import hip
    (N, C, h, w), rows = CASES[case]
    src, _ = _source(case, kind)
    exp_a, exp_t = _expected_windows(case, kind, reverse)
    dev_src = hip.bits16(src).cuda().view(src.dtype)
    idx = torch.tensor(rows, dtype=torch.int32).cuda()
    b, T = idx.shape
    got_a, got_t = hip.ensemble_windows(dev_src, idx, reverse=reverse)
    assert got_a.shape == (4, b, T, C, _ceil4(h), _ceil4(w)) and got_t.shape == (4, b, T, C, _ceil4(w), _ceil4(h))
    assert torch.equal(got_a.cpu(), exp_a) and torch.equal(got_t.cpu(), exp_t)
    # every element is stored, the zero padding included: poisoned buffers come back fully overwritten
    pa, pt = torch.full_like(got_a, float("nan")), torch.full_like(got_t, float("nan"))
    tail = (N, C, h, w, idx.data_ptr(), b, T, int(reverse), pa.data_ptr(), pt.data_ptr(), hip.stream_ptr())
    L = hip.lib()
    if kind == "f32":
        rc = L.fcvsr_ensemble_windows(dev_src.data_ptr(), *tail)
    elif kind == "u8":
        rc = L.fcvsr_ensemble_windows_u8(dev_src.data_ptr(), hip.u8_table("cuda").data_ptr(), *tail)
    else:
        rc = L.fcvsr_ensemble_windows_u16(dev_src.data_ptr(), hip.u16_table("cuda").data_ptr(), *tail)
    assert rc == 0
    assert not bool(torch.isnan(pa).any()) and not bool(torch.isnan(pt).any())
    assert torch.equal(pa.cpu(), exp_a) and torch.equal(pt.cpu(), exp_t)


# merge: the model outputs the two gather cases imply; b = 2
MERGE = {"18x21": (2, 3, 18, 21),        # 72 x 84 cropped out of 80 x 96
         "36x70": (2, 1, 36, 70)}        # 144 x 280 cropped out of 144 x 288


@functools.lru_cache(maxsize=None)
def _merge_inputs(case):
    b, C, h, w = MERGE[case]
    g = torch.Generator().manual_seed(11 + h)
    sa, st = (4, b, C, 4 * _ceil4(h), 4 * _ceil4(w)), (4, b, C, 4 * _ceil4(w), 4 * _ceil4(h))
    ts = [torch.randn(s, generator=g) * 0.6 + 0.5 for s in (sa, st, sa, st)]       # values below 0 and above 1
    assert all(float(t.min()) < 0 and float(t.max()) > 1 for t in ts)
    return ts


def _mean8(a, at, h, w):
    from fcvsr_amd.harness.ensemble import restore_host
    acc = None
    for i in range(8):
        o = a[i][..., :4 * h, :4 * w] if i < 4 else at[i - 4][..., :4 * w, :4 * h]
        o = restore_host(o, i)
        acc = o if acc is None else acc + o
    return acc * 0.125


@functools.lru_cache(maxsize=None)
def _merge_expected(case, temporal):
    _, _, h, w = MERGE[case]
    a, at, ra, rat = _merge_inputs(case)
    out = _mean8(a, at, h, w)
    return (out + _mean8(ra, rat, h, w)) * 0.5 if temporal else out


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("case", list(MERGE))
def test_merge_equals_sequential_restatement(case, temporal):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.infer import _quantised
    b, C, h, w = MERGE[case]
    a, at, ra, rat = [t.cuda() for t in _merge_inputs(case)]
    kw = dict(ra=ra, rat=rat) if temporal else {}
    exp = _merge_expected(case, temporal)
    got = hip.ensemble_merge(a, at, h, w, **kw)
    assert got.shape == (b, C, 4 * h, 4 * w) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), exp)
    assert not torch.equal(exp, _merge_expected(case, not temporal))                # the second pair matters
    for mode in ("truncate", "round"):
        got8 = hip.ensemble_merge(a, at, h, w, dtype=torch.uint8, quantise=mode, **kw)
        assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), _quantised(exp, mode))
        got16 = hip.ensemble_merge(a, at, h, w, dtype=torch.uint16, quantise=mode, **kw)
        assert got16.dtype == torch.uint16 and np.array_equal(hip.frames_to_numpy(got16), _quantised(exp, mode, 1023.0))
    assert not np.array_equal(_quantised(exp, "truncate"), _quantised(exp, "round"))


def test_library_rejects_bad_ensemble_arguments():
    """The C entry points return FCVSR_E_ARG (-1) instead of launching: null pointers, misaligned f32 tensors, zero sizes, a
    quantise mode that does not fit the output format; the wrappers raise on wrong shapes and dtypes."""
    from fcvsr_amd import hip
    L = hip.lib()
    st = hip.stream_ptr()
    src = torch.zeros(3, 1, 6, 10, device="cuda")
    src8 = torch.zeros(3, 1, 6, 10, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(1, 7, dtype=torch.int32, device="cuda")
    oa, ot = torch.zeros(4 * 7 * 8 * 12 + 4, device="cuda"), torch.zeros(4 * 7 * 12 * 8 + 4, device="cuda")
    tab = hip.u8_table("cuda")
    ok = (3, 1, 6, 10, idx.data_ptr(), 1, 7, 0)
    assert L.fcvsr_ensemble_windows(src.data_ptr(), *ok, oa.data_ptr(), ot.data_ptr(), st) == 0
    assert L.fcvsr_ensemble_windows(None, *ok, oa.data_ptr(), ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), 3, 1, 6, 10, None, 1, 7, 0, oa.data_ptr(), ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), *ok, None, ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), *ok, oa.data_ptr() + 4, ot.data_ptr(), st) == -1     # misaligned
    assert L.fcvsr_ensemble_windows(src.data_ptr(), *ok, oa.data_ptr(), ot.data_ptr() + 8, st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), 3, 1, 0, 10, idx.data_ptr(), 1, 7, 0, oa.data_ptr(), ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), 3, 1, 6, 10, idx.data_ptr(), 0, 7, 0, oa.data_ptr(), ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows(src.data_ptr(), 3, 1, 6, 10, idx.data_ptr(), 1, 7, 2, oa.data_ptr(), ot.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_windows_u8(src8.data_ptr(), None, *ok, oa.data_ptr(), ot.data_ptr(), st) == -1   # no table
    assert L.fcvsr_ensemble_windows_u8(src8.data_ptr(), tab.data_ptr(), *ok, oa.data_ptr(), ot.data_ptr(), st) == 0
    assert L.fcvsr_ensemble_windows_u16(src8.data_ptr() + 1, hip.u16_table("cuda").data_ptr(), *ok, oa.data_ptr(), ot.data_ptr(),
                                        st) == -1                                                          # odd address
    a, at = torch.zeros(4 * 32 * 48 + 4, device="cuda"), torch.zeros(4 * 48 * 32 + 4, device="cuda")
    out = torch.zeros(24 * 40 + 4, device="cuda")
    F32, U8, U16 = hip.F32, hip.U8, hip.U16
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, F32, 0, out.data_ptr(), st) == 0
    assert L.fcvsr_ensemble_merge(None, at.data_ptr(), None, None, 1, 1, 6, 10, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, F32, 0, None, st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), a.data_ptr(), None, 1, 1, 6, 10, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr() + 4, at.data_ptr(), None, None, 1, 1, 6, 10, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr() + 8, None, None, 1, 1, 6, 10, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, F32, 0, out.data_ptr() + 4, st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, U8, 1, out.data_ptr() + 2, st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 0, 1, 6, 10, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 0, F32, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, F32, 1, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, U8, 0, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, U16, 3, out.data_ptr(), st) == -1
    assert L.fcvsr_ensemble_merge(a.data_ptr(), at.data_ptr(), None, None, 1, 1, 6, 10, hip.BF16, 0, out.data_ptr(), st) == -1
    torch.cuda.synchronize()
    good_a, good_t = torch.zeros(4, 1, 1, 32, 48, device="cuda"), torch.zeros(4, 1, 1, 48, 32, device="cuda")
    with pytest.raises(ValueError):
        hip.ensemble_merge(good_a, good_a, 6, 10)                                   # at has a's shape
    with pytest.raises(ValueError):
        hip.ensemble_merge(good_a, good_t, 6, 10, ra=good_a)                        # half a temporal pair
    with pytest.raises(ValueError):
        hip.ensemble_merge(good_a, good_t, 6, 10, dtype=torch.uint8)                # no quantise mode
    with pytest.raises(ValueError):
        hip.ensemble_merge(good_a, good_t, 6, 10, quantise="round")                 # f32 result is not quantised
    with pytest.raises(ValueError):
        hip.ensemble_windows(src, idx.long())
    with pytest.raises(ValueError):
        hip.ensemble_windows(src.double(), idx)
