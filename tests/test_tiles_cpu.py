"""Host: the specification of tiled inference (fcvsr_amd/harness/tiles.py) - the grid, the integer and normalised weights, the blend
on CPU tensors - the refusals of the ``tile=`` / ``tile_overlap=`` keywords (raised before anything touches a device), and the C ABI /
binding of the two kernels of csrc/tiles.hip."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("fcvsr_tile_windows", "fcvsr_tile_windows_u8", "fcvsr_tile_windows_u16", "fcvsr_tile_merge")


def nearest4_centre(win: torch.Tensor) -> torch.Tensor:
    """(B,T,C,H,W) -> (B,C,4H,4W): nearest x4 of the centre frame; commutes with cutting tiles at multiples of 1 LR pixel."""
    return win[:, win.shape[1] // 2].repeat_interleave(4, -2).repeat_interleave(4, -1)


def test_grid_examples():
    from fcvsr_amd.harness.tiles import axis_starts, axis_weights
    assert axis_starts(28, 16, 8) == [0, 8, 12]
    assert axis_starts(32, 16, 4) == [0, 12, 16]
    assert axis_starts(12, 16, 4) == [0]
    assert axis_weights(12, 16, 4)[1] == 12                              # one tile, as long as the axis
    assert axis_starts(16, 16, 8) == [0] and axis_starts(20, 16, 0) == [0, 4]


def test_grid_sweep_covers_contiguously_with_at_most_three_tiles():
    from fcvsr_amd.harness.tiles import axis_starts
    for t in (8, 16, 20, 32):
        for o in range(0, t // 2 + 1):
            for L in range(4, 101, 4):
                starts = axis_starts(L, t, o)
                tt = min(t, L)
                assert starts == sorted(set(starts)) and starts[0] == 0, (L, t, o)
                assert all(0 <= a and a + tt <= L for a in starts), (L, t, o)           # every tile inside [0, L)
                cover = np.array([[a <= p < a + tt for p in range(L)] for a in starts])
                n = cover.sum(0)
                assert n.min() >= 1 and n.max() <= 3, (L, t, o, n.min(), n.max())
                for p in range(L):                                                     # the covering indices are one range
                    ks = np.flatnonzero(cover[:, p])
                    assert ks[-1] - ks[0] + 1 == len(ks), (L, t, o, p)


def _formula(L, t, o, scale=4):
    """The integer weights, written out per coordinate from the issue's formula."""
    from fcvsr_amd.harness.tiles import axis_starts
    starts, tt = axis_starts(L, t, o), min(t, L)
    w = np.zeros((len(starts), scale * L), dtype=np.int64)
    for k, a in enumerate(starts):
        for q in range(scale * tt):
            left = q + 1 if a > 0 else float("inf")
            right = scale * tt - q if a + tt < L else float("inf")
            w[k, scale * a + q] = min(left, right, max(scale * o, 1))
    return w


def test_integer_weights_equal_the_formula_on_hand_written_cases():
    from fcvsr_amd.harness.tiles import axis_weights
    # L = 3, t = 2, o = 1 at scale 2: tiles [0, 2) and [1, 3), SR coordinates 0..5, cap 2
    starts, tt, wi, wn = axis_weights(3, 2, 1, scale=2)
    assert starts == [0, 1] and tt == 2
    assert wi.tolist() == [[2, 2, 2, 1, 0, 0],        # no left neighbour: flat, then the ramp 2, 1 toward the right edge
                           [0, 0, 1, 2, 2, 2]]
    assert wn.dtype == np.float32
    assert wn.tolist() == [[1.0, 1.0, np.float32(2 / 3), np.float32(1 / 3), 0.0, 0.0],
                           [0.0, 0.0, np.float32(1 / 3), np.float32(2 / 3), 1.0, 1.0]]
    # L = 5, t = 2, o = 1 at scale 1: starts 0, 1, 2, 3; cap 1, so every weight is 1 and the interior is a plain average of 2
    starts, tt, wi, wn = axis_weights(5, 2, 1, scale=1)
    assert starts == [0, 1, 2, 3]
    assert wi.tolist() == [[1, 1, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 1, 1]]
    assert wn[:, 0].tolist() == [1.0, 0.0, 0.0, 0.0] and wn[:, 2].tolist() == [0.0, 0.5, 0.5, 0.0]
    for L, t, o in ((28, 16, 8), (32, 16, 4), (44, 20, 6), (12, 16, 4)):
        assert np.array_equal(axis_weights(L, t, o)[2], _formula(L, t, o)), (L, t, o)


def test_normalised_weights():
    from fcvsr_amd.harness.tiles import axis_weights
    for L, t, o in ((28, 16, 8), (32, 16, 4), (44, 20, 6), (100, 32, 16), (12, 16, 4)):
        starts, tt, wi, wn = axis_weights(L, t, o)
        assert wn.shape == (len(starts), 4 * L) and wn.dtype == np.float32
        assert np.array_equal(wn, (wi.astype(np.float64) / wi.sum(0).astype(np.float64)).astype(np.float32))
        single = (wi > 0).sum(0) == 1
        assert single.any() and np.array_equal(wn.sum(0)[single], np.ones(single.sum(), np.float32))
        assert set(np.unique(wn[:, single]).tolist()) <= {0.0, 1.0}          # exactly 1.0f where one tile covers, 0 for the rest
        assert np.abs(wn.astype(np.float64).sum(0) - 1).max() <= 4.5e-8
        assert np.array_equal(wn == 0, wi == 0)


def test_zero_overlap_gives_unit_weights_and_a_plain_average_under_the_shifted_tile():
    from fcvsr_amd.harness.tiles import axis_weights
    starts, tt, wi, wn = axis_weights(20, 8, 0)                              # starts 0, 8, 12: the last tile is shifted by 4
    assert starts == [0, 8, 12]
    assert set(np.unique(wi)) == {0, 1}
    assert np.array_equal(wn[:, 4 * 12:4 * 16], np.array([[0.0], [0.5], [0.5]], np.float32).repeat(16, 1))
    assert np.array_equal(wn[:, :4 * 12].sum(0), np.ones(48, np.float32)) and set(np.unique(wn[:, :4 * 12]).tolist()) == {0.0, 1.0}


def test_tile_plan():
    from fcvsr_amd.harness.tiles import tile_plan
    p = tile_plan(26, 42, (16, 20), (8, 6))
    assert (p.Hp, p.Wp, p.th, p.tw) == (28, 44, 16, 20)
    assert p.ys == [0, 8, 12] and p.xs == [0, 14, 24] and (p.ny, p.nx) == (3, 3)
    assert p.wy.shape == (3, 112) and p.wx.shape == (3, 176) and p.wy.dtype == p.wx.dtype == np.float32
    assert ((p.wy > 0).sum(0).max(), (p.wx > 0).sum(0).max()) == (3, 2)      # rows 12..15 lie in all three tile rows
    assert tile_plan(26, 42, (16, 20), (8, 6)) is p                          # cached: one set of device tables per plan
    q = tile_plan(12, 18, 32)                                                # fits one tile: the tile is the padded frame
    assert (q.th, q.tw, q.ys, q.xs) == (12, 20, [0], [0]) and float(q.wy.min()) == float(q.wx.min()) == 1.0
    with pytest.raises(ValueError):
        tile_plan(12, 18, None)


def test_tiled_host_of_a_frame_that_fits_one_tile_is_fn_on_the_padded_frame():
    from fcvsr_amd.harness.tiles import tile_plan, tiled_host

    def fn(win):                                                             # not equivariant, depends on every frame
        o = nearest4_centre(win) * 0.7 + win.mean(1).repeat_interleave(4, -2).repeat_interleave(4, -1) * 0.3
        return o * torch.linspace(0.5, 1.5, o.shape[-1])
    win = torch.from_numpy(np.random.RandomState(0).rand(2, 7, 3, 10, 18).astype(np.float32))
    got = tiled_host(win, fn, tile_plan(10, 18, 32, 16))
    ref = fn(torch.nn.functional.pad(win, (0, 2, 0, 2)))[..., :40, :72]
    assert got.shape == (2, 3, 40, 72) and got.dtype == torch.float32 and torch.equal(got, ref)
    seq = win.reshape(14, 3, 10, 18)                                         # the sequence form: frames and index rows
    assert torch.equal(tiled_host(seq, fn, tile_plan(10, 18, 32, 16), idx=np.arange(14).reshape(2, 7).tolist()), ref)


def test_tiled_host_reproduces_a_tile_commuting_function_within_the_rounding_bound():
    from fcvsr_amd.harness.tiles import tile_plan, tiled_host
    plan = tile_plan(26, 42, (16, 20), (8, 6))                               # 3 x 3 tiles, up to 3 x 2 of them on a pixel
    win = torch.from_numpy(np.random.RandomState(1).rand(1, 7, 1, 26, 42).astype(np.float32))
    calls = []

    def fn(w):
        calls.append(tuple(w.shape))
        return nearest4_centre(w)
    got = tiled_host(win, fn, plan)
    assert calls == [(1, 7, 1, 16, 20)] * 9                                  # one shape for every pass
    ref = nearest4_centre(win)
    assert got.shape == ref.shape == (1, 1, 104, 168)
    err = float((got - ref).abs().max())
    assert err <= 2e-6, err                                                  # <= 9 terms x 3 roundings x 2^-24 on values in [0, 1]
    one = tiled_host(torch.ones_like(win), fn, plan)
    assert float((one - 1).abs().max()) <= 2e-6
    # single-cover pixels (the frame's corners) are copied exactly
    assert torch.equal(got[..., :4, :4], ref[..., :4, :4]) and torch.equal(got[..., -4:, -4:], ref[..., -4:, -4:])


def test_refusals():
    from fcvsr_amd.harness.tiles import TiledSuperResolver, check_tile, tile_plan
    assert check_tile(None) is None and check_tile(None, "nonsense") is None
    assert check_tile(32) == ((32, 32), (16, 16)) and check_tile((16, 20), (8, 6)) == ((16, 20), (8, 6))
    assert check_tile(np.int64(32), 0) == ((32, 32), (0, 0)) and check_tile([8, 8], 4) == ((8, 8), (4, 4))
    for tile, ov in ((30, 8), ((16, 18), 4), (0, 0), (-16, 0), (16.0, 4), ("16", 4), (True, 0),      # not a positive multiple of 4
                     (16, 9), ((16, 32), (8, 17)), (32, 20),                                           # o > t // 2
                     (16, -1), (16, (4, -4)),                                                          # negative overlap
                     ((16, 16, 16), 4), ((16,), 4), (16, (4, 4, 4)), (16, ()), (16, 2.5), (16, None)):  # wrong length / type
        with pytest.raises(ValueError):
            check_tile(tile, ov)
        with pytest.raises(ValueError):
            tile_plan(64, 64, tile, ov)
        with pytest.raises(ValueError):
            TiledSuperResolver(object(), tile, ov)
    with pytest.raises(ValueError):
        TiledSuperResolver(object(), None)
    with pytest.raises(ValueError):
        TiledSuperResolver(object(), 16, 4, ensemble="x8")


def test_entry_points_take_the_keywords_and_refuse_before_any_device_work(tmp_path):
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    for fn in (super_resolve_sequence, evaluate_sequence, super_resolve_yuv420, super_resolve_yuv420_rgb):
        p = inspect.signature(fn).parameters
        assert p["tile"].default is None and p["tile_overlap"].default == 16, fn.__name__
        assert p["tile"].kind is p["tile_overlap"].kind is inspect.Parameter.KEYWORD_ONLY

    class NoDevice:                                                          # any device work would need its parameters
        _img_ch = 1

        def parameters(self):
            raise AssertionError("the model was touched before the keywords were validated")
    lr = torch.zeros(3, 1, 8, 8, dtype=torch.uint8)
    hr = torch.zeros(3, 1, 32, 32, dtype=torch.uint8)
    for kw in (dict(tile=30), dict(tile=16, tile_overlap=9), dict(tile=16, tile_overlap=-1), dict(tile=(16, 16, 16))):
        with pytest.raises(ValueError, match="tile"):
            super_resolve_sequence(NoDevice(), lr, **kw)
        with pytest.raises(ValueError, match="tile"):
            evaluate_sequence(NoDevice(), lr, hr, **kw)
        with pytest.raises(ValueError, match="tile"):
            super_resolve_yuv420(NoDevice(), str(tmp_path / "absent_8x8.yuv"), str(tmp_path / "o.yuv"), 8, 8, **kw)
    rgb = NoDevice()
    rgb._img_ch = 3
    with pytest.raises(ValueError, match="tile"):
        super_resolve_yuv420_rgb(rgb, str(tmp_path / "absent_8x8.yuv"), str(tmp_path / "o.yuv"), 8, 8, tile=30)
    assert not os.path.exists(tmp_path / "o.yuv")
    # the arguments that were validated first still are
    with pytest.raises(ValueError, match="ensemble"):
        super_resolve_sequence(NoDevice(), lr, ensemble="x8", tile=30)
    with pytest.raises(ValueError, match="quantise"):
        evaluate_sequence(NoDevice(), lr, hr, quantise="nearest", tile=30)
    with pytest.raises(ValueError, match="one-channel"):
        super_resolve_yuv420(rgb, "absent_8x8.yuv", "o.yuv", 8, 8, tile=30)


def test_new_symbols_are_declared_bound_and_exported_at_abi_version_2():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"#define\s+FCVSR_ABI_VERSION\s+2\b", hdr)
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
        assert name in hip.SIGNATURES, f"{name} has no row in hip.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES["fcvsr_tile_windows"]) == 16
    assert len(hip.SIGNATURES["fcvsr_tile_windows_u8"]) == len(hip.SIGNATURES["fcvsr_tile_windows_u16"]) == 17
    assert len(hip.SIGNATURES["fcvsr_tile_merge"]) == 17
    assert hip.lib().fcvsr_abi_version() == 2
    assert callable(hip.tile_windows) and callable(hip.tile_merge)


def test_wrappers_reject_host_tensors_without_a_fallback():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import TiledSuperResolver, tile_plan
    plan = tile_plan(6, 10, 4, 2)
    idx = torch.zeros(1, 7, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.tile_windows(torch.zeros(3, 1, 6, 10), idx, plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.tile_merge(torch.zeros(1, plan.ny, plan.nx, 1, 16, 16), plan, 6, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TiledSuperResolver(object(), 4, 2)(torch.zeros(1, 7, 1, 8, 8))
    with pytest.raises(ValueError):
        hip.tile_windows(torch.zeros(3, 1, 6, 10, dtype=torch.float64), idx, plan)
    with pytest.raises(ValueError):
        hip.tile_windows(torch.zeros(3, 1, 6, 10), idx.long(), plan)
    with pytest.raises(ValueError):
        hip.tile_merge(torch.zeros(1, 1, 1, 16, 16), plan, 6, 10)
