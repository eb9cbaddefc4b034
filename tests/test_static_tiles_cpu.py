"""CPU: the specification of ``static_tiles`` (`harness.tiles`: `static_pairs`, `static_sources`, `static_map_host`) and the
keyword's interface (`check_keywords`, the CLI, the header and the binding table).  No device is touched."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS7 = [[0, 0, 0, 0, 1, 2, 3], [0, 0, 0, 1, 2, 3, 4], [0, 0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]]    # replicate padding at the start


def _computed(src):
    return src == np.arange(src.shape[0])[:, None, None]


def test_static_pairs_are_the_unique_unordered_pairs_of_neighbouring_rows():
    from fcvsr_amd.harness.tiles import static_pairs
    assert static_pairs([[3, 4, 5]]) == []                                          # one row: nothing to compare
    assert static_pairs([[0, 0, 1], [0, 1, 2]]) == [(0, 1), (1, 2)]                 # (0,0) is the same frame
    assert static_pairs([[5, 4, 3], [4, 5, 3], [5, 4, 3]]) == [(4, 5)]              # unordered, once
    assert static_pairs(ROWS7) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert static_pairs([[2, 2], [2, 2]]) == []
    with pytest.raises(ValueError):
        static_pairs([[0, 1], [0]])
    with pytest.raises(ValueError):
        static_pairs([])


def test_static_sources_chains_resolve_to_the_computed_row():
    from fcvsr_amd.harness.tiles import static_pairs, static_sources
    rows = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]]
    pairs = static_pairs(rows)
    assert pairs == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    E = np.ones((5, 1, 2), dtype=np.uint8)
    E[3, 0, 0] = 0                                                                  # frames 3 / 4 differ on tile (0,0)
    src = static_sources(E, pairs, rows)
    assert src.shape == (5, 1, 2) and src.dtype == np.int32
    # tile (0,1): one chain over all five rows.  tile (0,0): rows 1, 2 reuse row 0; row 3 compares (2,3),(3,4) and row 4 (3,4),(4,5)
    assert src[:, 0, 1].tolist() == [0, 0, 0, 0, 0]
    assert src[:, 0, 0].tolist() == [0, 0, 0, 3, 4]
    E[:] = 1
    E[4, 0, 0] = 0                                                                  # only the last row sees (4,5)
    assert static_sources(E, pairs, rows)[:, 0, 0].tolist() == [0, 0, 0, 0, 4]
    with pytest.raises(ValueError):
        static_sources(E[:3], pairs, rows)


def _frames(N, C, h, w, seed=0, dtype=np.uint8):
    """N copies of one noise image."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (1, C, h, w)).astype(dtype)
    return np.repeat(img, N, 0)


def test_a_fully_static_sequence_computes_row_0_only_and_one_row_computes_everything():
    from fcvsr_amd.harness.tiles import static_map_host, tile_plan
    plan = tile_plan(26, 42, (16, 20), (8, 6))
    f = _frames(7, 3, 26, 42)
    src = static_map_host(f, ROWS7, plan)
    assert src.shape == (4, plan.ny, plan.nx) and not src.any()
    assert int(_computed(src).sum()) == plan.ny * plan.nx
    one = static_map_host(f, ROWS7[2:3], plan)                                       # b == 1
    assert one.shape == (1, plan.ny, plan.nx) and _computed(one).all()
    # a torch tensor is read the same way
    assert np.array_equal(static_map_host(torch.from_numpy(f), ROWS7, plan), src)


def _covering(plan, y, x):
    return {(ky, kx) for ky, ay in enumerate(plan.ys) for kx, ax in enumerate(plan.xs)
            if ay <= y < ay + plan.th and ax <= x < ax + plan.tw}


@pytest.mark.parametrize("y,x,count", [(9, 3, 2), (9, 15, 4), (3, 3, 1)])
def test_one_changed_sample_dirties_exactly_the_covering_tiles(y, x, count):
    from fcvsr_amd.harness.tiles import static_map_host, tile_plan
    plan = tile_plan(26, 42, (16, 20), (8, 6))                                       # ys [0, 8, 12], xs [0, 14, 24]
    assert (plan.ys, plan.xs) == ([0, 8, 12], [0, 14, 24])
    cover = _covering(plan, y, x)
    assert len(cover) == count
    f = _frames(3, 1, 26, 42)
    f[1, 0, y, x] ^= 1
    src = static_map_host(f, [[0, 0], [0, 1], [0, 2]], plan)                         # row 1 sees (0,1), row 2 sees (1,2)
    dirty = {(ky, kx) for ky in range(plan.ny) for kx in range(plan.nx) if src[1, ky, kx] == 1}
    assert dirty == cover
    assert {(ky, kx) for ky in range(plan.ny) for kx in range(plan.nx) if src[2, ky, kx] == 2} == cover
    assert all(src[2, ky, kx] == 0 for ky in range(plan.ny) for kx in range(plan.nx) if (ky, kx) not in cover)


def test_the_last_sample_of_an_unpadded_frame_dirties_only_its_tiles():
    from fcvsr_amd.harness.tiles import static_map_host, tile_plan
    h, w = 13, 21                                                                   # padded to 16 x 24
    plan = tile_plan(h, w, (8, 12), 4)
    f = _frames(2, 1, h, w)
    f[1, 0, h - 1, w - 1] ^= 0x80
    src = static_map_host(f, [[0], [1]], plan)
    cover = _covering(plan, h - 1, w - 1)
    assert cover == {(plan.ny - 1, plan.nx - 1)}
    assert {(ky, kx) for ky in range(plan.ny) for kx in range(plan.nx) if src[1, ky, kx] == 1} == cover


def test_repeated_frame_numbers_are_static_without_being_compared():
    from fcvsr_amd.harness.tiles import static_map_host, static_pairs, static_sources, tile_plan
    plan = tile_plan(18, 20, (16, 12), 4)
    rows = [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert static_pairs(rows) == []
    src = static_sources(np.zeros((0, 2, 2), dtype=np.uint8), [], rows)
    assert not src.any()
    f = np.random.RandomState(1).randint(0, 256, (3, 1, 18, 20)).astype(np.uint8)   # all frames differ
    assert not static_map_host(f, rows, plan).any()
    mixed = static_map_host(f, [[0, 0, 1], [0, 0, 2]], plan)                        # (0,0) twice, then a differing pair
    assert _computed(mixed).all()


def test_out_of_order_rows_and_raw_bit_comparison():
    from fcvsr_amd.harness.tiles import static_map_host, tile_plan
    plan = tile_plan(18, 20, (16, 12), 4)
    f = _frames(4, 1, 18, 20)
    f[2, 0, 1, 1] ^= 1                                                              # frame 2 differs in tile (0,0) only
    src = static_map_host(f, [[3, 1], [1, 3], [2, 0], [0, 3]], plan)
    assert not src[:2].any()                                                        # (1,3) both ways: equal frames
    assert src[2].tolist() == [[2, 0], [0, 0]]                                      # (1,2) differs on tile (0,0)
    assert src[3].tolist() == [[3, 0], [0, 0]]                                      # (0,2) too
    # uint16: the raw word counts, not min(k, 1023)
    g = np.full((2, 1, 18, 20), 1023, dtype=np.uint16)
    g[1, 0, 17, 19] = 2000
    assert static_map_host(g, [[0], [1]], plan)[1].tolist() == [[0, 0], [0, 1]]
    # f32: +0.0 and -0.0 differ, equal NaN patterns agree
    z = np.zeros((2, 1, 18, 20), dtype=np.float32)
    z[:, 0, 0, 0] = np.nan
    assert not static_map_host(z, [[0], [1]], plan).any()
    z[1, 0, 17, 0] = -0.0
    assert static_map_host(torch.from_numpy(z), [[0], [1]], plan)[1].tolist() == [[0, 0], [1, 0]]


def test_a_reuse_chain_over_four_rows_in_the_map():
    from fcvsr_amd.harness.tiles import static_map_host, tile_plan
    plan = tile_plan(18, 20, (16, 12), 4)
    f = _frames(10, 1, 18, 20)
    f[8, 0, 0, 0] ^= 1                                                              # the last row's newest frame changes tile (0,0)
    rows = [[i + j for j in range(7)] for i in range(3)]                            # frames 0..6, 1..7, 2..8
    src = static_map_host(f, rows + [rows[2]], plan)
    assert src[:, 1, 1].tolist() == [0, 0, 0, 0]
    assert src[:, 0, 0].tolist() == [0, 0, 2, 2]                                    # the fourth row reuses the third, which was computed


def test_static_tiles_needs_a_tile_size():
    from fcvsr_amd.harness.steps import check_keywords
    from fcvsr_amd.harness.tiles import TiledSuperResolver, tile_counts

    class M:
        _img_ch = 1
    good = dict(ensemble=None, tile_overlap=16, batch=8, quantise="truncate", cuts=None, frame_dtype=torch.uint8)
    with pytest.raises(ValueError, match="static_tiles"):
        check_keywords(M(), tile=None, static_tiles=True, **good)
    with pytest.raises(ValueError, match="static_tiles"):
        check_keywords(M(), tile=32, static_tiles=1, **good)
    r = check_keywords(M(), tile=32, static_tiles=True, **good)
    assert isinstance(r, TiledSuperResolver) and r.static_tiles and (r.tiles_total, r.tiles_run) == (0, 0)
    assert tile_counts(r) == {"tiles_total": 0, "tiles_run": 0}
    plain = check_keywords(M(), tile=32, **good)
    assert isinstance(plain, TiledSuperResolver) and not plain.static_tiles and tile_counts(plain) == {}
    assert tile_counts(check_keywords(M(), tile=None, static_tiles=False, **good)) == {}


def test_entry_points_reject_static_tiles_without_tile_before_any_work(tmp_path):
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.stream import stream_yuv420
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb

    class M:                                                                         # never asked for parameters: the error comes first
        _img_ch = 1
    lr = torch.zeros(2, 1, 8, 8, dtype=torch.uint8)
    missing = str(tmp_path / "missing_8x8_2F.yuv")
    with pytest.raises(ValueError, match="static_tiles"):
        super_resolve_sequence(M(), lr, static_tiles=True)
    with pytest.raises(ValueError, match="static_tiles"):
        evaluate_sequence(M(), lr, torch.zeros(2, 1, 32, 32, dtype=torch.uint8), static_tiles=True)
    with pytest.raises(ValueError, match="static_tiles"):
        super_resolve_yuv420(M(), missing, str(tmp_path / "o.yuv"), 8, 8, static_tiles=True)
    M._img_ch = 3
    with pytest.raises(ValueError, match="static_tiles"):
        super_resolve_yuv420_rgb(M(), missing, str(tmp_path / "o.yuv"), 8, 8, static_tiles=True)
    with pytest.raises(ValueError, match="static_tiles"):
        stream_yuv420(M(), missing, str(tmp_path / "o.yuv"), 8, 8, static_tiles=True)
    assert not os.path.exists(str(tmp_path / "o.yuv"))


def test_cli_parses_static_tiles():
    from fcvsr_amd.sr import parser
    base = ["--model", "GShiftNet_S", "--weights", "w.pth", "--size", "320x180", "in.yuv", "out.yuv"]
    assert parser().parse_args(base).static_tiles is False
    a = parser().parse_args(["--tile", "128x128", "--static-tiles"] + base)
    assert a.static_tiles is True and a.tile == (128, 128)


def test_run_stats_adds_the_tile_counts_only_with_static_tiles():
    from fcvsr_amd.harness.steps import run_stats
    from fcvsr_amd.harness.tiles import TiledSuperResolver
    on, off = TiledSuperResolver(None, 32, static_tiles=True), TiledSuperResolver(None, 32)
    on.tiles_total, on.tiles_run = 40, 13
    off.tiles_total, off.tiles_run = 40, 40
    base = run_stats(9, 0.5, 100, 1600, (80, 72))
    assert run_stats(9, 0.5, 100, 1600, (80, 72), tiles=off) == base
    assert run_stats(9, 0.5, 100, 1600, (80, 72), tiles=on) == {**base, "tiles_total": 40, "tiles_run": 13}


def test_static_tile_entry_points_are_declared_and_bound():
    from fcvsr_amd import hip
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    for name, n in (("fcvsr_tile_pairs_equal", 17), ("fcvsr_tile_pairs_equal_u8", 17), ("fcvsr_tile_pairs_equal_u16", 17),
                    ("fcvsr_tile_windows_sel", 18), ("fcvsr_tile_windows_sel_u8", 19), ("fcvsr_tile_windows_sel_u16", 19),
                    ("fcvsr_tile_merge_sel", 19)):
        assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
        assert len(hip.SIGNATURES[name]) == n
    assert int(re.search(r"#define FCVSR_TILE_EQ_SEG_CHUNKS (\d+)", hdr).group(1)) == hip.TILE_EQ_SEG_CHUNKS
    assert hip.tile_eq_segments(1, 128, 128, 1) == 1 and hip.tile_eq_segments(3, 128, 128, 4) == 12
    assert hip.tile_eq_segments(1, 8, 12, 1) == 1 and hip.tile_eq_segments(1, 68, 72, 4) == 2
