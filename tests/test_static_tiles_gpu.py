"""GPU, end to end: ``static_tiles=True`` delivers the bytes of ``static_tiles=False`` on every entry point that takes ``tile=``, and
runs exactly the tile windows the CPU specification (`harness.tiles.static_map_host`) says have to run.  No tolerances: a reused tile
output is the output of the same window, and the forward does not depend on the batch a window sits in.

The content: (10,1,18,20) frames on the plan of tests/test_tiles_gpu.py's SEQ_TILE (tile (16,12), overlap 4: tiles at ys [0,4],
xs [0,8]).  The background is one noise image; only rows 0-3 x columns 0-7 change from frame to frame, and they belong to tile (0,0)
alone."""
import functools
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEQ_TILE = dict(tile=(16, 12), tile_overlap=4)
N, H, W, BATCH = 10, 18, 20, 5


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


def _content(peak=255, C=1, n=N, seed=3):
    rs = np.random.RandomState(seed)
    a = np.repeat(rs.randint(0, peak + 1, (1, C, H, W)), n, 0)
    a[:, :, :4, :8] = rs.randint(0, peak + 1, (n, C, 4, 8))
    return a.astype(np.uint8 if peak == 255 else np.uint16)


def _torch(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def _plan(h=H, w=W):
    from fcvsr_amd.harness.tiles import tile_plan
    plan = tile_plan(h, w, (16, 12), 4)
    return plan


def _expected(a, batch=BATCH, cuts=None, plan=None):
    """(tiles_total, tiles_run) of the run by the CPU specification alone."""
    from fcvsr_amd.harness.shots import windows_for
    from fcvsr_amd.harness.tiles import static_map_host
    plan = _plan() if plan is None else plan
    total = run = 0
    for s in range(0, len(a), batch):
        src = static_map_host(a, windows_for(range(s, min(len(a), s + batch)), 7, len(a), "replicate", cuts), plan)
        total += src.size
        run += int((src == np.arange(src.shape[0])[:, None, None]).sum())
    return total, run


@pytest.fixture
def made(monkeypatch):
    """The tiled resolvers the entry points make during the test, each with the windows its per-window function was given."""
    from fcvsr_amd.harness import tiles
    made, real = [], tiles.resolver_for

    def recording(*args, **kw):
        r = real(*args, **kw)
        if isinstance(r, tiles.TiledSuperResolver):
            fn, r.windows_seen = r._fn, 0

            def counted(win):
                r.windows_seen += win.shape[0]
                return fn(win)
            r._fn = counted
            made.append(r)
        return r
    monkeypatch.setattr(tiles, "resolver_for", recording)
    return made


def test_the_specification_alone_reuses_at_least_half_of_the_tiles():
    plan = _plan()
    assert (plan.ys, plan.xs, plan.th, plan.tw) == ([0, 4], [0, 8], 16, 12)
    for a in (_content(), _content(1023), _content().astype(np.float32) / 255):
        total, run = _expected(a)
        assert total == N * 4 and run == 2 * (4 + 4) and total - run >= total // 2
    assert _expected(_content(1023), cuts=[5]) == (40, 16)


def _both(made, fn, *args, **kw):
    """fn with static_tiles False and True: (plain result, static result, the static run's resolver)."""
    plain = fn(*args, **kw)
    assert made[-1].tiles_run == made[-1].tiles_total > 0 and not made[-1].static_tiles
    static = fn(*args, static_tiles=True, **kw)
    assert made[-1].static_tiles
    return plain, static, made[-1]


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_super_resolve_sequence_bytes_and_counts(made, quantise):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    a = _content()
    total, run = _expected(a)
    plain, static, r = _both(made, super_resolve_sequence, _model(), _torch(a), batch=BATCH, quantise=quantise, **SEQ_TILE)
    assert plain.dtype == np.uint8 and plain.shape == (N, 1, 72, 80)
    assert np.array_equal(static, plain), f"{int((static != plain).sum())} bytes differ"
    assert (r.tiles_total, r.tiles_run) == (total, run) and r.tiles_run < r.tiles_total
    assert r.windows_seen == r.tiles_run
    assert len({plain[i].tobytes() for i in range(N)}) == N                          # the frames do change


def test_float_frames(made):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    a = _content().astype(np.float32) / 255
    plain, static, r = _both(made, super_resolve_sequence, _model(), torch.from_numpy(a), batch=BATCH, **SEQ_TILE)
    assert np.array_equal(static, plain)
    assert (r.tiles_total, r.tiles_run) == _expected(a) and r.windows_seen == r.tiles_run < r.tiles_total


def test_10_bit_frames_with_cuts(made):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    a = _content(1023)
    a[:, 0, 17, 19] = 1023 + np.arange(N) * 100                                      # container words above 1023: all read as 1023,
    total, run = _expected(a, cuts=[5])                                              # but the raw words differ: tile (1,1) is dirty
    assert run > 16
    plain, static, r = _both(made, super_resolve_sequence, _model(), _torch(a), batch=BATCH, quantise="round", cuts=[5], **SEQ_TILE)
    assert plain.dtype == np.uint16 and np.array_equal(static, plain)
    assert (r.tiles_total, r.tiles_run) == (total, run) and r.windows_seen == run < total


def test_spatial_ensemble(made):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    a = _content()[:6]
    plain, static, r = _both(made, super_resolve_sequence, _model(), _torch(a), batch=3, ensemble="spatial", **SEQ_TILE)
    assert np.array_equal(static, plain)
    assert (r.tiles_total, r.tiles_run) == _expected(a, batch=3) and r.windows_seen == r.tiles_run < r.tiles_total


def test_inside_an_active_box(made):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    a = _content()
    box = (0, 18, 0, 16)                                                             # the model sees 18 x 16: tiles at xs [0, 4]
    plain, static, r = _both(made, super_resolve_sequence, _model(), _torch(a), batch=BATCH, active=box, **SEQ_TILE)
    assert np.array_equal(static, plain)
    crop = np.ascontiguousarray(a[:, :, :, :16])
    assert (r.tiles_total, r.tiles_run) == _expected(crop, plan=_plan(18, 16)) and r.windows_seen == r.tiles_run < r.tiles_total


def test_evaluate_sequence_scores(made):
    from fcvsr_amd.harness.infer import evaluate_sequence
    a = _content()
    hr = torch.from_numpy(np.random.RandomState(6).randint(0, 256, (N, 1, 72, 80)).astype(np.uint8))
    plain, static, r = _both(made, evaluate_sequence, _model(), _torch(a), hr, batch=BATCH, return_frames=True, **SEQ_TILE)
    assert np.array_equal(static.frames, plain.frames)
    assert np.array_equal(static.psnr, plain.psnr) and np.array_equal(static.ssim, plain.ssim)
    assert r.windows_seen == r.tiles_run < r.tiles_total


def _i420(a):
    """The frames `a` (n,1,H,W) as an I420 file's bytes with one fixed chroma image."""
    rs = np.random.RandomState(9)
    u, v = (np.repeat(rs.randint(0, 256, (1, H // 2, W // 2)).astype(np.uint8), len(a), 0) for _ in range(2))
    return b"".join(a[i, 0].tobytes() + u[i].tobytes() + v[i].tobytes() for i in range(len(a)))


@pytest.mark.parametrize("ctor", ["GShiftNet_S", "FCVSR_SNet"])
def test_the_file_functions_write_the_same_bytes_and_count(made, ctor, tmp_path):
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    m = _model(ctor)
    data = _i420(_content(n=7))
    src = str(tmp_path / f"Seq_{W}x{H}_7F.yuv")
    with open(src, "wb") as fh:
        fh.write(data)
    whole = super_resolve_yuv420 if ctor == "GShiftNet_S" else super_resolve_yuv420_rgb
    outs = {}
    for flag in (False, True):
        dst = str(tmp_path / f"out{int(flag)}.yuv")
        stats = whole(m, src, dst, W, H, batch=4, static_tiles=flag, **SEQ_TILE)
        outs[flag] = open(dst, "rb").read()
        assert ("tiles_total" in stats) == ("tiles_run" in stats) == flag
    assert outs[True] == outs[False] and len(outs[True]) == 7 * 72 * 80 * 3 // 2
    r = made[-1]
    assert (stats["tiles_total"], stats["tiles_run"]) == (r.tiles_total, r.tiles_run) == (28, r.windows_seen)
    assert r.tiles_run < r.tiles_total
    if ctor == "GShiftNet_S":
        assert r.tiles_run == (4 + 3) + (4 + 2)
    for flag in (False, True):
        out = io.BytesIO()
        sstats = stream_yuv420(m, io.BytesIO(data), out, W, H, batch=4, static_tiles=flag, **SEQ_TILE)
        assert out.getvalue() == outs[False]
        assert ("tiles_total" in sstats) == ("tiles_run" in sstats) == flag
    assert sstats["tiles_total"] == 28 and sstats["tiles_run"] == made[-1].windows_seen < 28


def _graph_batches(m):
    return {key[0][0] for key in m._get_engine()._graphs}


@pytest.mark.parametrize("rows,batch", [(6, 6), (4, 8)])
def test_use_graph_keeps_the_pass_sizes_bounded(rows, batch):
    from fcvsr_amd.harness.shots import windows_for
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    m = _model()
    x = _torch(_content()).cuda()
    idx = windows_for(range(2, 2 + rows), 7, N, "replicate", None)
    tsr = TiledSuperResolver(m, batch=batch, static_tiles=True, **SEQ_TILE)
    eager = tsr.sequence(x, idx, dtype=torch.uint8, quantise="round")
    run = tsr.tiles_run
    assert run == 4 + (rows - 1) and run % batch not in (0, 1, 2, 4)                 # a last chunk that has to be padded
    assert torch.equal(eager, TiledSuperResolver(m, batch=batch, **SEQ_TILE).sequence(x, idx, dtype=torch.uint8, quantise="round"))
    m.invalidate()
    m.use_graph = True
    try:
        first = tsr.sequence(x, idx, dtype=torch.uint8, quantise="round")
        replay = tsr.sequence(x, idx, dtype=torch.uint8, quantise="round")
        sizes = _graph_batches(m)
    finally:
        m.use_graph = False
        m.invalidate()
    assert torch.equal(first, eager) and torch.equal(replay, eager)
    assert tsr.tiles_run == 3 * run                                                 # the padding windows are not counted
    assert sizes and all(s == batch or s & (s - 1) == 0 for s in sizes), sizes
    assert all(s <= batch for s in sizes)
