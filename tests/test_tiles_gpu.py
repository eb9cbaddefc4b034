"""GPU: tiled inference (`harness.tiles`, the ``tile=`` / ``tile_overlap=`` keywords of the sequence and YUV harnesses).  Kernel
level: the tile-window gather and the feathered merge of csrc/tiles.hip equal host slicing and the torch restatement of the blend.
End to end: `TiledSuperResolver` equals the same model on every tile window, blended by that restatement.  No tolerances: the gather
is exact data movement, the blend's order and roundings are fixed, and the forward is batch-invariant (tests/test_configs_gpu.py
pins that)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(ctor_name="GShiftNet_S", precision="bf16"):
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    from helpers import get_ctor
    m = get_ctor(ctor_name)()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes(ctor_name), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = precision
    return m


def _blend(tiles, plan):
    """The torch restatement of the blend on the host: tiles (b,ny,nx,C,4th,4tw) f32 -> (b,C,4h,4w); ky, then kx ascending, the
    weight product, the product with the value and the sum each one f32 operation."""
    tiles = tiles.cpu()
    b, ny, nx, C, TH, TW = tiles.shape
    wy, wx = torch.from_numpy(plan.wy), torch.from_numpy(plan.wx)
    out = torch.zeros(b, C, 4 * plan.Hp, 4 * plan.Wp)
    for ky in range(ny):
        for kx in range(nx):
            Y, X = 4 * plan.ys[ky], 4 * plan.xs[kx]
            g = wy[ky, Y:Y + TH].reshape(-1, 1) * wx[kx, X:X + TW].reshape(1, -1)
            term = g * tiles[:, ky, kx]
            out[:, :, Y:Y + TH, X:X + TW] += term
    return out[:, :, :4 * plan.h, :4 * plan.w].contiguous()


def _tile_stack(winp, plan, fn=lambda t: t):
    """fn on every tile window of the padded windows winp (B,T,C,Hp,Wp), stacked to (B,ny,nx,...)."""
    return torch.stack([torch.stack([fn(winp[..., ay:ay + plan.th, ax:ax + plan.tw].contiguous()) for ax in plan.xs], 1)
                        for ay in plan.ys], 1)


def _restate(fn, win, plan):
    """win: f32 (B,7,C,h,w) on the device.  One call of fn per tile, blended on the host."""
    with torch.no_grad():
        return _blend(_tile_stack(F.pad(win, (0, plan.Wp - plan.w, 0, plan.Hp - plan.h)), plan, fn), plan)


# (N,C,h,w), tile, overlap, index rows (b,T) with repeated and out-of-order frame numbers
CASES = {
    "26x42": ((5, 3, 26, 42), (16, 20), (8, 6), [[0, 0, 0, 1, 2, 3, 4], [4, 3, 1, 1, 0, 2, 2]]),   # 3 x 3 tiles, padded both ways
    "26x42c1": ((4, 1, 26, 42), (16, 20), (8, 6), [[0, 0, 1, 1, 2, 3, 3], [3, 2, 1, 0, 0, 1, 2]]),
    "12x18": ((3, 3, 12, 18), 32, 16, [[0, 0, 0, 1, 2, 2, 2]]),                                      # one tile, padded inside
    "12x18c1": ((3, 1, 12, 18), 32, 16, [[2, 1, 0, 1, 2, 2, 0]]),
    "13x21": ((3, 1, 13, 21), (8, 12), (4, 4), [[0, 1, 2, 2, 1, 0, 0]]),                             # rows start at every byte offset
    "70x90": ((2, 1, 70, 90), (68, 72), (4, 8), [[0, 1, 1, 0, 0, 1, 0]]),                            # tile planes of 2 x 2 blocks
}
DTYPES = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.uint16}


@functools.lru_cache(maxsize=None)
def _source(case, kind):
    """The sequence (host, its own dtype) and the floats the kernels must read from it (host f32)."""
    from fcvsr_amd import hip
    shape = CASES[case][0]
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


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("case", list(CASES))
def test_tile_windows_equal_host_slicing(case, kind):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    (N, C, h, w), tile, ov, rows = CASES[case]
    plan = tile_plan(h, w, tile, ov)
    src, vals = _source(case, kind)
    winp = F.pad(vals, (0, plan.Wp - w, 0, plan.Hp - h))[torch.tensor(rows)]         # (b,T,C,Hp,Wp)
    exp = _tile_stack(winp, plan)
    dev_src = hip.bits16(src).cuda().view(src.dtype)
    idx = torch.tensor(rows, dtype=torch.int32).cuda()
    b, T = idx.shape
    got = hip.tile_windows(dev_src, idx, plan)
    assert got.shape == exp.shape == (b, plan.ny, plan.nx, T, C, plan.th, plan.tw) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), exp)
    # every element is stored, the zero padding included: a poisoned buffer comes back fully overwritten
    poison = torch.full_like(got, float("nan"))
    ys, xs, _, _ = plan.device_tables("cuda")
    tail = (N, C, h, w, idx.data_ptr(), b, T, ys.data_ptr(), plan.ny, xs.data_ptr(), plan.nx, plan.th, plan.tw, poison.data_ptr(),
            hip.stream_ptr())
    L = hip.lib()
    if kind == "f32":
        rc = L.fcvsr_tile_windows(dev_src.data_ptr(), *tail)
    elif kind == "u8":
        rc = L.fcvsr_tile_windows_u8(dev_src.data_ptr(), hip.u8_table("cuda").data_ptr(), *tail)
    else:
        rc = L.fcvsr_tile_windows_u16(dev_src.data_ptr(), hip.u16_table("cuda").data_ptr(), *tail)
    assert rc == 0
    assert torch.equal(poison.cpu(), exp)


# merge: (b, C, h, w), tile, overlap
MERGE = {"26x42": ((2, 2, 26, 42), (16, 20), (8, 6)),        # 104 x 168 cropped out of 112 x 176: 2 x 3 blocks, up to 3 x 2 tiles a pixel
         "12x18": ((2, 3, 12, 18), 32, 16),                   # one tile: a crop
         "70x90": ((1, 1, 70, 90), (68, 72), (4, 8)),         # tiles larger than a block
         "20x20": ((1, 1, 20, 20), 8, 4)}                     # 4 x 4 tiles of 32 x 32 SR pixels: several tiles inside one block


@functools.lru_cache(maxsize=None)
def _merge_case(case):
    from fcvsr_amd.harness.tiles import tile_plan
    (b, C, h, w), tile, ov = MERGE[case]
    plan = tile_plan(h, w, tile, ov)
    g = torch.Generator().manual_seed(13 + h)
    tiles = torch.randn((b, plan.ny, plan.nx, C, 4 * plan.th, 4 * plan.tw), generator=g) * 0.6 + 0.5   # values below 0 and above 1
    assert float(tiles.min()) < 0 and float(tiles.max()) > 1
    return plan, tiles, _blend(tiles, plan)


@pytest.mark.parametrize("case", list(MERGE))
def test_tile_merge_equals_the_torch_restatement(case):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.infer import _quantised
    from fcvsr_amd.harness.tiles import blend_host
    (b, C, h, w), _, _ = MERGE[case]
    plan, tiles, exp = _merge_case(case)
    assert torch.equal(blend_host(tiles, plan), exp)                                 # the package's specification says the same
    dev = tiles.cuda()
    got = hip.tile_merge(dev, plan, h, w)
    assert got.shape == (b, C, 4 * h, 4 * w) and got.dtype == torch.float32
    bad = int((got.cpu() != exp).sum())
    assert bad == 0, f"{bad} of {exp.numel()} values differ (max {float((got.cpu() - exp).abs().max()):.3e})"
    for mode in ("truncate", "round"):
        got8 = hip.tile_merge(dev, plan, h, w, dtype=torch.uint8, quantise=mode)
        assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), _quantised(exp, mode))
        got16 = hip.tile_merge(dev, plan, h, w, dtype=torch.uint16, quantise=mode)
        assert got16.dtype == torch.uint16 and np.array_equal(hip.frames_to_numpy(got16), _quantised(exp, mode, 1023.0))
    assert not np.array_equal(_quantised(exp, "truncate"), _quantised(exp, "round"))


def test_library_rejects_bad_tile_arguments():
    """The C entry points return FCVSR_E_ARG (-1) instead of launching: null pointers, misaligned tensors, zero sizes, tiles that are
    no multiple of 4 or larger than the padded frame, a quantise mode that does not fit the output format."""
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    L, st = hip.lib(), hip.stream_ptr()
    plan = tile_plan(6, 10, 4, 2)                                                    # 8 x 12 padded: 3 x 5 tiles of 4 x 4
    ys, xs, wy, wx = plan.device_tables("cuda")
    ny, nx = plan.ny, plan.nx
    assert (ny, nx) == (3, 5)
    src = torch.zeros(3, 1, 6, 10, device="cuda")
    src8 = torch.zeros(3, 1, 6, 10, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(1, 7, dtype=torch.int32, device="cuda")
    out = torch.zeros(ny * nx * 7 * 16 + 4, device="cuda")
    tab = hip.u8_table("cuda")

    def win(src_p=src.data_ptr(), idx_p=idx.data_ptr(), ys_p=ys.data_ptr(), xs_p=xs.data_ptr(), out_p=out.data_ptr(), h=6, b=1,
            th=4, tw=4, ny_=ny):
        return L.fcvsr_tile_windows(src_p, 3, 1, h, 10, idx_p, b, 7, ys_p, ny_, xs_p, nx, th, tw, out_p, st)
    assert win() == 0
    assert win(src_p=None) == -1 and win(idx_p=None) == -1 and win(ys_p=None) == -1 and win(xs_p=None) == -1 and win(out_p=None) == -1
    assert win(out_p=out.data_ptr() + 4) == -1                                       # misaligned
    assert win(h=0) == -1 and win(b=0) == -1 and win(ny_=0) == -1
    assert win(th=6) == -1 and win(th=0) == -1 and win(th=12) == -1 and win(tw=16) == -1     # not a multiple of 4; too large
    assert L.fcvsr_tile_windows_u8(src8.data_ptr(), None, 3, 1, 6, 10, idx.data_ptr(), 1, 7, ys.data_ptr(), ny, xs.data_ptr(), nx, 4,
                                   4, out.data_ptr(), st) == -1                      # no table
    assert L.fcvsr_tile_windows_u8(src8.data_ptr(), tab.data_ptr(), 3, 1, 6, 10, idx.data_ptr(), 1, 7, ys.data_ptr(), ny,
                                   xs.data_ptr(), nx, 4, 4, out.data_ptr(), st) == 0
    assert L.fcvsr_tile_windows_u16(src8.data_ptr() + 1, hip.u16_table("cuda").data_ptr(), 3, 1, 6, 10, idx.data_ptr(), 1, 7,
                                    ys.data_ptr(), ny, xs.data_ptr(), nx, 4, 4, out.data_ptr(), st) == -1    # odd address
    tiles = torch.zeros(ny * nx * 256 + 4, device="cuda")
    res = torch.zeros(24 * 40 + 4, device="cuda")
    F32, U8, U16 = hip.F32, hip.U8, hip.U16

    def merge(tiles_p=tiles.data_ptr(), ys_p=ys.data_ptr(), wy_p=wy.data_ptr(), wx_p=wx.data_ptr(), out_p=res.data_ptr(), b=1, w=10,
              th=4, dt=F32, q=0):
        return L.fcvsr_tile_merge(tiles_p, ys_p, ny, xs.data_ptr(), nx, th, 4, wy_p, wx_p, b, 1, 6, w, dt, q, out_p, st)
    assert merge() == 0
    assert merge(tiles_p=None) == -1 and merge(ys_p=None) == -1 and merge(wy_p=None) == -1 and merge(wx_p=None) == -1
    assert merge(out_p=None) == -1
    assert merge(tiles_p=tiles.data_ptr() + 4) == -1 and merge(wx_p=wx.data_ptr() + 8) == -1 and merge(out_p=res.data_ptr() + 4) == -1
    assert merge(out_p=res.data_ptr() + 2, dt=U8, q=1) == -1
    assert merge(b=0) == -1 and merge(w=0) == -1 and merge(th=6) == -1 and merge(th=12) == -1
    assert merge(q=1) == -1 and merge(dt=U8, q=0) == -1 and merge(dt=U16, q=3) == -1 and merge(dt=hip.BF16) == -1
    assert merge(dt=U8, q=1) == 0 and merge(dt=U16, q=2) == 0
    torch.cuda.synchronize()
    good = torch.zeros(1, ny, nx, 1, 16, 16, device="cuda")
    with pytest.raises(ValueError):
        hip.tile_merge(good[:, :2], plan, 6, 10)                                    # a tile row is missing
    with pytest.raises(ValueError):
        hip.tile_merge(good, plan, 6, 14)                                           # not the plan's frame
    with pytest.raises(ValueError):
        hip.tile_merge(good, plan, 6, 10, dtype=torch.uint8)                        # no quantise mode
    with pytest.raises(ValueError):
        hip.tile_merge(good, plan, 6, 10, quantise="round")                         # an f32 result is not quantised
    with pytest.raises(ValueError):
        hip.tile_windows(src, idx.long(), plan)
    with pytest.raises(ValueError):
        hip.tile_windows(src[..., :8], idx, plan)


def _window(B, C, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).rand(B, 7, C, H, W).astype(np.float32)).cuda()


@pytest.mark.parametrize("ctor,precision,B,C", [("GShiftNet_S", "bf16", 2, 1), ("GShiftNet_S", "f32", 2, 1), ("FCVSR_SNet", "bf16", 1, 3)])
def test_tiled_super_resolver_equals_the_restatement(ctor, precision, B, C):
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    m = _model(ctor, precision)
    win = _window(B, C, 26, 42, seed=3)
    tsr = TiledSuperResolver(m, (16, 20), (8, 6))
    plan = tsr.plan(26, 42)
    got = tsr(win)
    ref = _restate(m, win, plan)
    assert got.shape == (B, C, 104, 168) and got.dtype == torch.float32
    bad = int((got.cpu() != ref).sum())
    assert bad == 0, f"{bad} of {ref.numel()} values differ (max {float((got.cpu() - ref).abs().max()):.3e})"
    assert torch.equal(tsr(win, batch=5), got)                       # the chunking of the model passes does not show
    with torch.no_grad():
        plain = m(F.pad(win, (0, 2, 0, 2)))[..., :104, :168]
    assert not torch.equal(got, plain)                               # a different estimator, not a no-op


def test_a_frame_that_fits_one_tile_equals_the_plain_path():
    from fcvsr_amd.harness.infer import _quantised
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    m = _model()
    tsr = TiledSuperResolver(m, 32)
    x8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (2, 7, 1, 14, 18)).astype(np.uint8))   # padded inside
    winf = (x8.float() / 255).cuda()
    with torch.enable_grad():                                        # the training graph must not run
        got = tsr(winf)
    with torch.no_grad():
        plain = m(F.pad(winf, (0, 2, 0, 2)))[..., :56, :72]
    assert not got.requires_grad and got.shape == (2, 1, 56, 72)
    assert torch.equal(got, plain)
    assert torch.equal(tsr(x8.cuda()), got)                          # uint8 samples enter as the floats of the table
    for mode in ("truncate", "round"):
        got8 = tsr.super_resolve_u8(x8.cuda(), mode)
        assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), _quantised(plain, mode))
        assert torch.equal(got8, m.super_resolve_u8(F.pad(x8, (0, 2, 0, 2)).cuda(), mode)[..., :56, :72])
    x16 = (x8.to(torch.int16) * 4 + 1).view(torch.uint16)
    with torch.no_grad():
        plain16 = m(F.pad(x16.view(torch.int16).float() / 1023, (0, 2, 0, 2)).cuda())[..., :56, :72]
    got16 = tsr.super_resolve_u16(x16.view(torch.int16).cuda().view(torch.uint16), "round")
    assert got16.dtype == torch.uint16
    assert np.array_equal(got16.view(torch.int16).cpu().numpy().view(np.uint16), _quantised(plain16, "round", 1023.0))
    with pytest.raises(ValueError, match="uint8"):
        tsr.super_resolve_u8(winf)
    with pytest.raises(ValueError, match="quantise"):
        tsr.super_resolve_u8(x8.cuda(), "nearest")


def test_tiles_with_spatial_ensemble_equal_the_restatement():
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    m = _model()
    win = _window(1, 1, 26, 42, seed=5)
    tsr = TiledSuperResolver(m, (16, 20), (8, 6), ensemble="spatial")
    got = tsr(win, batch=4)
    ref = _restate(SelfEnsemble(m), win, tsr.plan(26, 42))
    bad = int((got.cpu() != ref).sum())
    assert bad == 0, f"{bad} of {ref.numel()} values differ (max {float((got.cpu() - ref).abs().max()):.3e})"
    assert not torch.equal(got, TiledSuperResolver(m, (16, 20), (8, 6))(win))


def _graph_window_shapes(m):
    return {key[0][1:] for key in m._get_engine()._graphs}


def test_use_graph_equals_eager_and_captures_one_window_shape():
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    m = _model()
    tsr = TiledSuperResolver(m, (16, 20), (8, 6))
    win, other = _window(2, 1, 26, 42, seed=6), _window(1, 1, 18, 44, seed=7)       # two frame sizes, one tile shape
    eager, eager_other = tsr(win), tsr(other)
    m.invalidate()
    m.use_graph = True
    try:
        first = tsr(win)                                             # 18 tile windows: chunks of 8, 8, 2
        replay = tsr(win)
        third = tsr(other)                                           # 6 tile windows of the same shape
        shapes = _graph_window_shapes(m)
    finally:
        m.use_graph = False
        m.invalidate()
    assert torch.equal(first, eager) and torch.equal(replay, eager) and torch.equal(third, eager_other)
    assert shapes == {(7, 1, 16, 20)}, shapes


def _seq8(N, C, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, C, H, W)).astype(np.uint8))


SEQ_TILE = dict(tile=(16, 12), tile_overlap=4)                       # 18 x 20 frames: 2 x 2 tiles of 16 x 12 on the 20 x 20 padded frame


@functools.lru_cache(maxsize=None)
def _sequence_blend():
    """The hand restatement for the (6,1,18,20) sequence, f32: every frame's window, every tile through the float model."""
    from fcvsr_amd.harness.tiles import tile_plan
    from fcvsr_amd.harness.windows import window_indices
    lr = (_seq8(6, 1, 18, 20, seed=1).float() / 255).cuda()
    win = torch.stack([lr[window_indices(i, 7, 6, "replicate")] for i in range(6)], 0)
    plan = tile_plan(18, 20, (16, 12), 4)
    assert (plan.ys, plan.xs, plan.th, plan.tw) == ([0, 4], [0, 8], 16, 12)
    return _restate(_model(), win, plan)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_super_resolve_sequence_with_tiles(quantise):
    from fcvsr_amd.harness.infer import _quantised, super_resolve_sequence
    m = _model()
    lr8 = _seq8(6, 1, 18, 20, seed=1)
    got = super_resolve_sequence(m, lr8, batch=4, quantise=quantise, **SEQ_TILE)
    flt = super_resolve_sequence(m, lr8.float() / 255, batch=4, quantise=quantise, **SEQ_TILE)
    assert got.dtype == np.uint8 and got.shape == (6, 1, 72, 80)
    assert np.array_equal(got, flt)
    ref = _quantised(_sequence_blend(), quantise)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} bytes differ from the hand restatement"
    plain = super_resolve_sequence(m, lr8, batch=4, quantise=quantise)
    assert not np.array_equal(got, plain)
    sub = super_resolve_sequence(m, lr8.cuda(), batch=2, centres=[5, 0, 3], quantise=quantise, **SEQ_TILE)
    assert np.array_equal(sub, ref[[5, 0, 3]])
    # a frame that fits the tile: the untiled bytes
    assert np.array_equal(super_resolve_sequence(m, lr8, batch=4, quantise=quantise, tile=64), plain)
    assert np.array_equal(super_resolve_sequence(m, lr8.float() / 255, batch=4, quantise=quantise, tile=64),
                          super_resolve_sequence(m, lr8.float() / 255, batch=4, quantise=quantise))


def test_super_resolve_sequence_with_tiles_10_bit_and_cuts():
    from fcvsr_amd.harness.infer import _quantised, super_resolve_sequence
    from fcvsr_amd.harness.shots import shot_window_indices
    from fcvsr_amd.harness.tiles import tile_plan
    m = _model()
    rs = np.random.RandomState(7)
    lr = rs.randint(0, 1024, (4, 1, 18, 20))
    lr[0, 0, 0, :4] = (2000, 1024, 65535, 1023)                     # out-of-range containers read as 1023
    lr16 = torch.from_numpy(lr.astype(np.uint16).view(np.int16)).view(torch.uint16)
    got = super_resolve_sequence(m, lr16, batch=4, quantise="round", cuts=[2], **SEQ_TILE)
    assert got.dtype == np.uint16 and got.shape == (4, 1, 72, 80) and int(got.max()) <= 1023
    lrf = (torch.from_numpy(np.minimum(lr, 1023)).float() / 1023).cuda()
    win = torch.stack([lrf[shot_window_indices(i, 7, 4, [2], "replicate")] for i in range(4)], 0)
    ref = _quantised(_restate(m, win, tile_plan(18, 20, (16, 12), 4)), "round", 1023.0)
    assert np.array_equal(got, ref)
    assert np.array_equal(super_resolve_sequence(m, lr16, batch=4, quantise="round", tile=64),
                          super_resolve_sequence(m, lr16, batch=4, quantise="round"))


def test_evaluate_sequence_with_tiles_scores_the_blended_frames():
    from fcvsr_amd.harness.device_metrics import frame_metrics
    from fcvsr_amd.harness.infer import _quantised, evaluate_sequence, super_resolve_sequence
    m = _model()
    lr8 = _seq8(6, 1, 18, 20, seed=1)
    hr = _seq8(6, 1, 72, 80, seed=6)
    for lr in (lr8, lr8.float() / 255):
        res = evaluate_sequence(m, lr, hr, batch=4, return_frames=True, baseline="bicubic", **SEQ_TILE)
        frames = super_resolve_sequence(m, lr, batch=4, **SEQ_TILE)
        assert np.array_equal(res.frames, frames)
        p, s = frame_metrics(torch.from_numpy(frames).cuda(), hr.cuda(), quantise=None)
        assert np.array_equal(res.psnr, p.cpu().numpy()) and np.array_equal(res.ssim, s.cpu().numpy())
        assert res.psnr_mean == float(np.mean(res.psnr)) and res.ssim_mean == float(np.mean(res.ssim))
        plain = evaluate_sequence(m, lr, hr, batch=4, baseline="bicubic")
        assert np.array_equal(res.baseline_psnr, plain.baseline_psnr)               # the baseline does not depend on the tiles
        assert not np.array_equal(res.psnr, plain.psnr)
        whole = evaluate_sequence(m, lr, hr, batch=4, tile=64)
        assert np.array_equal(whole.psnr, plain.psnr) and np.array_equal(whole.ssim, plain.ssim)
    assert np.array_equal(frames, _quantised(_sequence_blend(), "truncate"))


def test_super_resolve_yuv420_with_tiles(tmp_path):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import read_yuv420, super_resolve_yuv420, write_yuv420
    m = _model()
    N, H, W = 5, 18, 20
    rs = np.random.RandomState(8)
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
    src, dst, plain = (str(tmp_path / n) for n in (f"Seq_{W}x{H}_{N}F.yuv", "tiled.yuv", "plain.yuv"))
    write_yuv420(src, y, u, v)
    stats = super_resolve_yuv420(m, src, dst, W, H, batch=3, **SEQ_TILE)
    super_resolve_yuv420(m, src, plain, W, H, batch=3)
    assert stats["frames"] == N and stats["out_size"] == (4 * W, 4 * H)
    oy, ou, ov = read_yuv420(dst, 4 * W, 4 * H)
    py, pu, pv = read_yuv420(plain, 4 * W, 4 * H)
    assert np.array_equal(oy, super_resolve_sequence(m, torch.from_numpy(y)[:, None], batch=3, **SEQ_TILE)[:, 0])
    assert np.array_equal(ou, pu) and np.array_equal(ov, pv)        # chroma does not go through the tiles
    assert not np.array_equal(oy, py)


def test_super_resolve_yuv420_rgb_with_tiles(tmp_path):
    from fcvsr_amd.harness.colour import ColourSpec, rgb_to_yuv420_host, yuv420_to_rgb_host
    from fcvsr_amd.harness.infer import super_resolve_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    m = _model("FCVSR_SNet", "bf16")
    spec = ColourSpec()
    N, H, W = 4, 18, 20
    rs = np.random.RandomState(9)
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2)))
    src, dst = str(tmp_path / f"Seq_{W}x{H}_{N}F.yuv"), str(tmp_path / "out.yuv")
    write_yuv420(src, y, u, v)
    super_resolve_yuv420_rgb(m, src, dst, W, H, colour=spec, batch=3, **SEQ_TILE)
    rgb = torch.from_numpy(yuv420_to_rgb_host(y, u, v, spec))
    sr = super_resolve_sequence(m, rgb, batch=3, **SEQ_TILE)
    sy, su, sv = rgb_to_yuv420_host(sr, spec)
    ref = np.concatenate([p[i].ravel() for i in range(N) for p in (sy, su, sv)])
    got = np.fromfile(dst, dtype=np.uint8)
    bad = int((got != ref).sum())
    assert bad == 0, f"{bad} of {ref.size} samples differ"
