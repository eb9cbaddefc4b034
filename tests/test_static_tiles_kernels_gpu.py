"""GPU: the three kernels of ``static_tiles`` (csrc/tiles.hip), bit for bit: `hip.tile_pairs_equal` against a numpy comparison of
the stored bytes per tile rectangle, `hip.tile_windows(sel=)` against indexing the full result, `hip.tile_merge(src=)` against
`hip.tile_merge` on the expanded tensor.  The shapes are those of tests/test_tiles_gpu.py that stress the tile kernels."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, h, w), tile, overlap
CASES = {
    "13x21": ((1, 13, 21), (8, 12), (4, 4)),          # 3 x 3 tiles; rows start at every byte offset; padded both ways
    "26x42": ((3, 26, 42), (16, 20), (8, 6)),         # 3 x 3 tiles, three planes
    "26x42c1": ((1, 26, 42), (16, 20), (8, 6)),
    "70x90": ((1, 70, 90), (68, 72), (4, 8)),         # 2 x 2 tiles; an f32 tile takes two segments (two workgroups)
}
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
TORCH = {"u8": torch.uint8, "u16": torch.uint16, "f32": torch.float32}


def _plan(case):
    from fcvsr_amd.harness.tiles import tile_plan
    (C, h, w), tile, ov = CASES[case]
    return tile_plan(h, w, tile, ov)


def _noise(shape, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "f32":
        return rs.rand(*shape).astype(np.float32)
    return rs.randint(0, 256 if kind == "u8" else 1024, shape).astype(NP[kind])


def _to_device(a: np.ndarray, offset: int = 1) -> torch.Tensor:
    """The frames on the device, `offset` samples into their allocation: the sequence starts at an address that is a multiple of
    the sample size only."""
    flat = a.reshape(-1)
    host = torch.from_numpy(flat.view(np.int16) if a.dtype == np.uint16 else flat)
    buf = torch.zeros(flat.size + offset, dtype=host.dtype, device="cuda")
    buf[offset:] = host.cuda()
    t = buf[offset:].view(a.shape)
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def _equal_host(a: np.ndarray, pairs, plan) -> np.ndarray:
    """The numpy statement: the stored bytes of both frames agree on the tile's rectangle clipped to the frame, all channels."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(*a.shape, a.dtype.itemsize)
    E = np.zeros((len(pairs), plan.ny, plan.nx), dtype=np.uint8)
    for p, (fa, fb) in enumerate(pairs):
        for ky, ay in enumerate(plan.ys):
            for kx, ax in enumerate(plan.xs):
                y1, x1 = min(ay + plan.th, plan.h), min(ax + plan.tw, plan.w)
                E[p, ky, kx] = np.array_equal(raw[fa, :, ay:y1, ax:x1], raw[fb, :, ay:y1, ax:x1])
    return E


def _flip(a, f, c, y, x):
    """One sample of frame f changes in its lowest stored bit."""
    v = a[f, c, y:y + 1, x:x + 1].view(np.uint8 if a.dtype.itemsize == 1 else np.uint16 if a.dtype.itemsize == 2 else np.uint32)
    v ^= 1


def _run(a, pairs, plan, offset=1):
    from fcvsr_amd import hip
    got = hip.tile_pairs_equal(_to_device(a, offset), torch.tensor(pairs, dtype=torch.int32).cuda(), plan)
    assert got.shape == (len(pairs), plan.ny, plan.nx) and got.dtype == torch.uint8
    return got.cpu().numpy()


@pytest.mark.parametrize("kind", list(NP))
@pytest.mark.parametrize("case", list(CASES))
def test_tile_pairs_equal_single_samples(case, kind):
    """Frame 0 is the image; frames 1.. differ from it in one sample each: the first valid sample of the last tile, the last valid
    sample of tile (0,0), the last element of the last plane, a sample in the overlap of four tiles; frame 5 is identical."""
    (C, h, w), _, _ = CASES[case]
    plan = _plan(case)
    a = np.repeat(_noise((1, C, h, w), kind, seed=len(case)), 6, 0)
    ky, kx = plan.ny - 1, plan.nx - 1
    _flip(a, 1, 0, plan.ys[ky], plan.xs[kx])
    _flip(a, 2, 0, min(plan.th, h) - 1, min(plan.tw, w) - 1)
    _flip(a, 3, C - 1, h - 1, w - 1)
    oy, ox = plan.ys[1], plan.xs[1]                                                 # inside tiles (0,0), (0,1), (1,0), (1,1)
    assert oy < plan.th and ox < plan.tw
    _flip(a, 4, C // 2, oy, ox)
    pairs = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (5, 0), (3, 3), (2, 4)]
    exp = _equal_host(a, pairs, plan)
    assert exp[4].all() and exp[6].all() and exp[7].all()                           # identical frames
    assert exp[0].sum() < exp[0].size and exp[0][ky, kx] == 0
    assert exp[1][0, 0] == 0 and exp[2][ky, kx] == 0 and int(exp[2].sum()) == exp[2].size - 1
    assert (exp[3][:2, :2] == 0).all()
    got = _run(a, pairs, plan)
    assert np.array_equal(got, exp), f"differs at {np.argwhere(got != exp).tolist()}"
    assert np.array_equal(_run(a, pairs, plan, offset=0), exp)                      # and from the start of an allocation


@pytest.mark.parametrize("kind", list(NP))
def test_tile_pairs_equal_never_reads_outside_the_clipped_rectangle(kind):
    """The multiple-of-4 padding is not in memory: where it would be lie the next row, plane or frame.  Two frames agree on the
    clipped rectangle of one tile and differ in every other sample - that tile, and no other, is equal."""
    for case in ("13x21", "26x42"):
        (C, h, w), _, _ = CASES[case]
        plan = _plan(case)
        for ky, kx in ((plan.ny - 1, plan.nx - 1), (0, plan.nx - 1), (1, 1)):
            ay, ax = plan.ys[ky], plan.xs[kx]
            y1, x1 = min(ay + plan.th, h), min(ax + plan.tw, w)
            a = _noise((3, C, h, w), kind, seed=3)
            b = a[0].copy()
            b.view(np.uint8)[...] ^= 0x01                                           # every sample of frame 1 differs from frame 0
            b[:, ay:y1, ax:x1] = a[0, :, ay:y1, ax:x1]
            a[1] = b
            exp = _equal_host(a, [(0, 1), (1, 2)], plan)
            assert int(exp[0].sum()) == 1 and exp[0][ky, kx] == 1 and not exp[1].any()
            assert np.array_equal(_run(a, [(0, 1), (1, 2)], plan), exp), (case, ky, kx)


def test_tile_pairs_equal_compares_raw_bits():
    plan = _plan("26x42c1")
    # uint16: words that differ only above 1023 are different, though the model reads both as 1023
    a = np.repeat(_noise((1, 1, 26, 42), "u16", seed=5), 3, 0)
    a[0, 0, 25, 41], a[1, 0, 25, 41], a[2, 0, 25, 41] = 1500, 2000, 1500
    exp = _equal_host(a, [(0, 1), (0, 2)], plan)
    assert exp[0][2, 2] == 0 and int(exp[0].sum()) == 8 and exp[1].all()
    assert np.array_equal(_run(a, [(0, 1), (0, 2)], plan), exp)
    # f32: +0.0 and -0.0 differ; equal NaN patterns agree; different NaN patterns differ
    f = np.repeat(_noise((1, 1, 26, 42), "f32", seed=6), 4, 0)
    f[:, 0, 0, 0] = 0.0
    f[1, 0, 0, 0] = -0.0
    f[:, 0, 13, 30] = np.nan
    f[3, 0, 13, 30:31].view(np.uint32)[0] ^= 1                                      # another NaN
    assert np.isnan(f[3, 0, 13, 30])
    pairs = [(0, 1), (0, 2), (0, 3)]
    exp = _equal_host(f, pairs, plan)
    assert exp[0][0, 0] == 0 and int(exp[0].sum()) == 8 and exp[1].all() and not exp[2].all()
    assert np.array_equal(_run(f, pairs, plan), exp)


@pytest.mark.parametrize("kind", list(NP))
@pytest.mark.parametrize("case", ["13x21", "26x42", "70x90"])
def test_tile_windows_sel_equals_indexing_the_full_result(case, kind):
    from fcvsr_amd import hip
    (C, h, w), _, _ = CASES[case]
    plan = _plan(case)
    a = _noise((5, C, h, w), kind, seed=11)
    if kind == "u16":
        a.reshape(-1)[::5] = 40000                                                   # samples above 1023 read as 1023
    dev = _to_device(a)
    rows = [[0, 0, 0, 1, 2, 3, 4], [4, 3, 1, 1, 0, 2, 2], [2, 2, 3, 3, 4, 4, 0]]
    idx = torch.tensor(rows, dtype=torch.int32).cuda()
    full = hip.tile_windows(dev, idx, plan)
    rs = np.random.RandomState(2)
    sel = np.stack([rs.randint(0, 3, 11), rs.randint(0, plan.ny, 11), rs.randint(0, plan.nx, 11)], 1).astype(np.int32)
    sel[3] = sel[0]                                                                 # a repeated row
    sel[10] = (2, plan.ny - 1, plan.nx - 1)
    got = hip.tile_windows(dev, idx, plan, sel=torch.from_numpy(sel).cuda())
    assert got.shape == (11, 7, C, plan.th, plan.tw) and got.dtype == torch.float32
    exp = full[sel[:, 0].tolist(), sel[:, 1].tolist(), sel[:, 2].tolist()]
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
    one = hip.tile_windows(dev, idx, plan, sel=torch.tensor([[1, 0, plan.nx - 1]], dtype=torch.int32).cuda())
    assert torch.equal(one[0], full[1, 0, plan.nx - 1])


MERGE = {"26x42": ((3, 2, 26, 42), (16, 20), (8, 6)), "70x90": ((2, 1, 70, 90), (68, 72), (4, 8)), "20x20": ((4, 1, 20, 20), 8, 4)}


@pytest.mark.parametrize("case", list(MERGE))
def test_tile_merge_src_equals_the_merge_of_the_expanded_tensor(case):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    (b, C, h, w), tile, ov = MERGE[case]
    plan = tile_plan(h, w, tile, ov)
    n = 5
    g = torch.Generator().manual_seed(17)
    pool = (torch.randn((n, C, 4 * plan.th, 4 * plan.tw), generator=g) * 0.6 + 0.5).cuda()     # values below 0 and above 1
    src = torch.from_numpy(np.random.RandomState(4).randint(0, n, (b, plan.ny, plan.nx)).astype(np.int32)).cuda()
    src[0, 0, 0], src[b - 1, plan.ny - 1, plan.nx - 1] = n - 1, 0
    expanded = pool[src.long()]                                                     # (b,ny,nx,C,4th,4tw)
    got = hip.tile_merge(pool, plan, h, w, src=src)
    assert got.shape == (b, C, 4 * h, 4 * w)
    assert torch.equal(got.view(torch.int32), hip.tile_merge(expanded, plan, h, w).view(torch.int32))
    for dt in (torch.uint8, torch.uint16):
        for mode in ("truncate", "round"):
            q = hip.tile_merge(pool, plan, h, w, dtype=dt, quantise=mode, src=src)
            ref = hip.tile_merge(expanded, plan, h, w, dtype=dt, quantise=mode)
            assert q.dtype == dt and torch.equal(hip.bits16(q), hip.bits16(ref)), (dt, mode)
    assert not torch.equal(hip.tile_merge(pool, plan, h, w, dtype=torch.uint8, quantise="truncate", src=src),
                           hip.tile_merge(pool, plan, h, w, dtype=torch.uint8, quantise="round", src=src))


def test_library_rejects_bad_static_tile_arguments():
    """The C entry points return FCVSR_E_ARG (-1) instead of launching; the bindings raise ValueError for tables of the wrong shape."""
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    L, st = hip.lib(), hip.stream_ptr()
    plan = tile_plan(6, 10, 4, 2)                                                    # 8 x 12 padded: 3 x 5 tiles of 4 x 4
    ys, xs, wy, wx = plan.device_tables("cuda")
    ny, nx = plan.ny, plan.nx
    src = torch.zeros(3, 1, 6, 10, device="cuda")
    src8 = torch.zeros(3, 1, 6, 10, dtype=torch.uint8, device="cuda")
    pairs = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32, device="cuda")
    scratch = torch.zeros(2 * ny * nx, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2 * ny * nx, dtype=torch.uint8, device="cuda")

    def eq(src_p=src.data_ptr(), pairs_p=pairs.data_ptr(), P=2, ys_p=ys.data_ptr(), scratch_p=scratch.data_ptr(),
           nbytes=scratch.numel(), out_p=out.data_ptr(), th=4, h=6):
        return L.fcvsr_tile_pairs_equal(src_p, 3, 1, h, 10, pairs_p, P, ys_p, ny, xs.data_ptr(), nx, th, 4, scratch_p, nbytes, out_p, st)
    assert eq() == 0
    assert eq(src_p=None) == -1 and eq(pairs_p=None) == -1 and eq(ys_p=None) == -1 and eq(scratch_p=None) == -1 and eq(out_p=None) == -1
    assert eq(P=0) == -1 and eq(h=0) == -1 and eq(th=6) == -1 and eq(th=12) == -1
    assert eq(nbytes=2 * ny * nx - 1) == -1                                           # scratch too small
    assert eq(src_p=src.data_ptr() + 2) == -1 and eq(pairs_p=pairs.data_ptr() + 2) == -1
    args8 = (3, 1, 6, 10, pairs.data_ptr(), 2, ys.data_ptr(), ny, xs.data_ptr(), nx, 4, 4, scratch.data_ptr(), scratch.numel(),
             out.data_ptr(), st)
    assert L.fcvsr_tile_pairs_equal_u8(src8.data_ptr(), *args8) == 0
    assert L.fcvsr_tile_pairs_equal_u16(src8.data_ptr() + 1, *args8) == -1          # odd address
    assert L.fcvsr_tile_pairs_equal_u8(None, *args8) == -1

    idx = torch.zeros(1, 7, dtype=torch.int32, device="cuda")
    sel = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    wout = torch.zeros(2 * 7 * 16 + 4, device="cuda")

    def win(src_p=src.data_ptr(), idx_p=idx.data_ptr(), sel_p=sel.data_ptr(), n=2, out_p=wout.data_ptr(), b=1):
        return L.fcvsr_tile_windows_sel(src_p, 3, 1, 6, 10, idx_p, b, 7, ys.data_ptr(), ny, xs.data_ptr(), nx, 4, 4, sel_p, n, out_p, st)
    assert win() == 0
    assert win(src_p=None) == -1 and win(idx_p=None) == -1 and win(sel_p=None) == -1 and win(out_p=None) == -1
    assert win(n=0) == -1 and win(n=-1) == -1 and win(b=0) == -1 and win(out_p=wout.data_ptr() + 4) == -1
    assert L.fcvsr_tile_windows_sel_u8(src8.data_ptr(), None, 3, 1, 6, 10, idx.data_ptr(), 1, 7, ys.data_ptr(), ny, xs.data_ptr(), nx,
                                       4, 4, sel.data_ptr(), 2, wout.data_ptr(), st) == -1       # no table
    assert L.fcvsr_tile_windows_sel_u8(src8.data_ptr(), hip.u8_table("cuda").data_ptr(), 3, 1, 6, 10, idx.data_ptr(), 1, 7,
                                       ys.data_ptr(), ny, xs.data_ptr(), nx, 4, 4, sel.data_ptr(), 2, wout.data_ptr(), st) == 0

    pool = torch.zeros(2 * 256 + 4, device="cuda")
    slots = torch.zeros(ny * nx, dtype=torch.int32, device="cuda")
    res = torch.zeros(24 * 40 + 4, device="cuda")

    def merge(pool_p=pool.data_ptr(), n=2, slots_p=slots.data_ptr(), wy_p=wy.data_ptr(), out_p=res.data_ptr(), b=1, dt=hip.F32, q=0):
        return L.fcvsr_tile_merge_sel(pool_p, n, slots_p, ys.data_ptr(), ny, xs.data_ptr(), nx, 4, 4, wy_p, wx.data_ptr(), b, 1, 6, 10,
                                      dt, q, out_p, st)
    assert merge() == 0
    assert merge(pool_p=None) == -1 and merge(slots_p=None) == -1 and merge(wy_p=None) == -1 and merge(out_p=None) == -1
    assert merge(n=0) == -1 and merge(b=0) == -1 and merge(q=1) == -1 and merge(dt=hip.U8, q=0) == -1
    assert merge(pool_p=pool.data_ptr() + 4) == -1 and merge(slots_p=slots.data_ptr() + 2) == -1
    assert merge(dt=hip.U8, q=1) == 0 and merge(dt=hip.U16, q=2) == 0
    torch.cuda.synchronize()
    # the bindings: tables of the wrong shape or type
    good_pool = torch.zeros(2, 1, 16, 16, device="cuda")
    with pytest.raises(ValueError):
        hip.tile_merge(good_pool, plan, 6, 10, src=slots.view(1, nx, ny))
    with pytest.raises(ValueError):
        hip.tile_merge(good_pool, plan, 6, 10, src=slots.view(1, ny, nx).long())
    with pytest.raises(ValueError):
        hip.tile_merge(good_pool[:, :, :8], plan, 6, 10, src=slots.view(1, ny, nx))
    with pytest.raises(ValueError):
        hip.tile_windows(src, idx, plan, sel=sel[:, :2])
    with pytest.raises(ValueError):
        hip.tile_windows(src, idx, plan, sel=sel[:0])
    with pytest.raises(ValueError):
        hip.tile_windows(src, idx, plan, sel=sel.long())
    with pytest.raises(ValueError):
        hip.tile_pairs_equal(src, pairs[:, :1], plan)
    with pytest.raises(ValueError):
        hip.tile_pairs_equal(src, pairs[:0], plan)
    with pytest.raises(ValueError):
        hip.tile_pairs_equal(src[..., :8], pairs, plan)
