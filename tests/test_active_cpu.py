"""CPU: the host contract of `active=` (`harness.active`): line sums, the box of a frame, the growing union, alignment and the
min_side fallback, the causal window rule, run splitting, keyword validation and the command line."""
import numpy as np
import pytest

import active_cases as ac
from fcvsr_amd.harness import active as A
from fcvsr_amd.harness.shots import windows_for

SMALL = A.ActiveSpec(min_side=8)


@pytest.mark.parametrize("bits", [8, 10])
def test_planted_bars_under_noise_give_the_planted_box(bits):
    f = ac.barred(bits, 3, 1, 40, 64, (7, 33, 9, 50), seed=bits)
    if bits == 10:
        f[0, 0, 20, 20] = 60000                                           # read as 1023
    rows, cols = A.line_sums_host(f)
    assert rows.dtype == np.uint64 and cols.dtype == np.uint64 and rows.shape == (3, 40) and cols.shape == (3, 64)
    g = np.minimum(f.astype(np.int64), 1023) if bits == 10 else f.astype(np.int64)
    assert np.array_equal(rows, g.sum((1, 3))) and np.array_equal(cols, g.sum((1, 2)))
    for i in range(3):
        assert A.frame_box(rows[i], cols[i], 1, 40, 64, bits) == (7, 33, 9, 50)
    # three channels: the sums run over all of them
    f3 = ac.barred(bits, 1, 3, 24, 36, (4, 20, 0, 36), seed=1)
    rows, cols = A.line_sums_host(f3)
    assert A.frame_box(rows[0], cols[0], 3, 24, 36, bits) == (4, 20, 0, 36)


def test_the_limit_is_strict_and_on_the_8_bit_scale():
    H, W = 6, 8
    f = np.zeros((1, 1, H, W), np.uint8)
    f[0, 0, 2] = 24                                                       # a row whose mean is exactly the limit is not picture
    f[0, 0, 3] = 25
    rows, cols = A.line_sums_host(f)
    assert A.frame_box(rows[0], cols[0], 1, H, W, 8, A.ActiveSpec(limit=24.0)) is None     # no column reaches a mean of 24
    assert A.frame_box(rows[0], cols[0], 1, H, W, 8, A.ActiveSpec(limit=8.0)) == (2, 4, 0, W)
    f10 = f.astype(np.uint16) * 4
    rows, cols = A.line_sums_host(f10)
    assert A.frame_box(rows[0], cols[0], 1, H, W, 10, A.ActiveSpec(limit=8.0)) == (2, 4, 0, W)


def test_an_all_black_frame_gives_none_and_the_whole_frame_is_used():
    f = ac.barred(8, 2, 1, 16, 20, (0, 0, 0, 0))
    rows, cols = A.line_sums_host(f)
    assert A.frame_box(rows[0], cols[0], 1, 16, 20, 8) is None
    b = A.ActiveBoxes(1, 16, 20, 8)
    b.push(rows, cols)
    assert b.upto(1) is None and A.used_box(b.upto(1), 16, 20) == (0, 16, 0, 20)


def test_a_bright_line_in_a_bar_grows_the_union_for_good():
    f = ac.barred(8, 6, 1, 40, 48, (8, 32, 0, 48))
    f[2, 0, 36, :] = 200                                                  # a subtitle line in the lower bar of frame 2 only
    rows, cols = A.line_sums_host(f)
    b = A.ActiveBoxes(1, 40, 48, 8)
    b.push(rows, cols)
    assert [b.upto(i) for i in range(6)] == [(8, 32, 0, 48)] * 2 + [(8, 37, 0, 48)] * 4
    with pytest.raises(ValueError):
        b.upto(6)


def test_alignment_is_outward_and_clipped():
    spec = A.ActiveSpec(align=4, min_side=8)
    assert A.used_box((5, 21, 6, 30), 30, 40, spec) == (4, 24, 4, 32)
    assert A.used_box((4, 24, 8, 32), 30, 40, spec) == (4, 24, 8, 32)
    assert A.used_box((3, 29, 1, 39), 30, 38, spec) == (0, 30, 0, 38)     # H = 30, W = 38 are no multiples of 4: clipped to the frame
    assert A.used_box((9, 29, 2, 37), 30, 38, A.ActiveSpec(align=8, min_side=8)) == (8, 30, 0, 38)


def test_min_side_falls_back_to_the_whole_frame():
    assert A.used_box((8, 36, 0, 64), 48, 64) == (0, 48, 0, 64)           # 28 rows < 32
    assert A.used_box((8, 40, 0, 64), 48, 64) == (8, 40, 0, 64)
    assert A.used_box((8, 40, 20, 44), 48, 64) == (0, 48, 0, 64)          # 24 columns
    assert A.used_box((8, 36, 0, 64), 48, 64, A.ActiveSpec(min_side=28)) == (8, 36, 0, 64)
    assert A.used_box(None, 48, 64) == (0, 48, 0, 64)


def _growing(bits=8, n=12):
    return ac.barred(bits, n, 1, 24, 32, lambda i: (8, 16, 4, 28) if i < 5 else (4, 20, 4, 28), seed=3)


@pytest.mark.parametrize("cuts", [None, [6]])
@pytest.mark.parametrize("padding", ["replicate", "reflection", "reflection_circle", "circle"])
def test_the_window_rule_is_causal(padding, cuts):
    f = _growing()
    n, C, H, W = f.shape
    plan = A.ActivePlan(SMALL, C, H, W, 8)
    plan.push(*A.line_sums_host(f))
    windows = windows_for(range(n), 7, n, padding, cuts)
    got = plan.group(range(n), windows, n)
    for c, (w, box) in enumerate(zip(windows, got)):
        last = max(w)
        assert box == ac.brute_box(f, 8, last, SMALL), (c, w)
        short = A.ActiveBoxes(C, H, W, 8, SMALL)                          # frames after the last one of the window do not exist yet
        short.push(*A.line_sums_host(f[:last + 1]))
        assert A.window_box(short, w, n) == box
    small = {(8, 16, 4, 28)} if min(max(w) for w in windows) < 5 else set()    # "circle" modes reach frame 6 from centre 0
    assert set(got) == small | {(4, 20, 4, 28)}
    first_big = min(c for c, w in enumerate(windows) if max(w) >= 5)
    assert plan.changes == ([(0, (8, 16, 4, 28))] if first_big else []) + [(first_big, (4, 20, 4, 28))]


def test_a_window_of_a_short_sequence_counts_from_the_end():
    f = _growing(n=3)
    b = A.ActiveBoxes(1, 24, 32, 8, SMALL)
    b.push(*A.line_sums_host(f))
    assert A.window_box(b, [0, 0, 1, 2, -1, -2, -3], 3) == (8, 16, 4, 28)


def test_a_group_is_split_into_runs_of_one_box():
    a, b = (8, 16, 4, 28), (4, 20, 4, 28)
    assert A.split_runs([a, a, b, b, b]) == [(0, 2, a), (2, 5, b)]
    assert A.split_runs([a]) == [(0, 1, a)]
    assert A.split_runs([a, b, a]) == [(0, 1, a), (1, 2, b), (2, 3, a)]
    assert A.split_runs([]) == []


def test_the_explicit_box_is_validated():
    assert A.check_active(None, "float32", 24, 32) is None
    assert A.check_active((4, 20, 0, 32), "float32", 24, 32) == (4, 20, 0, 32)
    assert A.check_active([np.int64(0), 24, 0, 32], "uint8", 24, 32) == (0, 24, 0, 32)
    for bad in ((4, 4, 0, 32), (-1, 20, 0, 32), (4, 25, 0, 32), (4, 20, 8, 8), (4, 20, 0, 33), (4, 20, 0), (4.0, 20, 0, 32),
                (True, 20, 0, 32), "box", 7):
        with pytest.raises(ValueError):
            A.check_active(bad, "uint8", 24, 32)
    assert A.check_active("auto", "uint8", 24, 32) == A.ActiveSpec()
    assert A.check_active(SMALL, "uint16", 24, 32) is SMALL
    for auto in ("auto", SMALL):
        with pytest.raises(ValueError):
            A.check_active(auto, "float32", 24, 32)
    for kw in ({"limit": -1.0}, {"align": 0}, {"min_side": 2.5}):
        with pytest.raises(ValueError):
            A.ActiveSpec(**kw)


def test_the_entry_points_refuse_in_the_prologue():
    import torch

    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    lr, hr = torch.zeros((3, 1, 24, 32)), torch.zeros((3, 1, 96, 128), dtype=torch.uint8)
    for bad in ("auto", SMALL, (4, 4, 0, 32), (0, 25, 0, 32), "letterbox"):       # the model (None here) is never reached
        with pytest.raises(ValueError):
            super_resolve_sequence(None, lr, active=bad)
        with pytest.raises(ValueError):
            evaluate_sequence(None, lr, hr, active=bad)


def test_chunks_equal_one_push():
    f = _growing()
    f[7, 0, 22, :] = 255
    rows, cols = A.line_sums_host(f)
    one = A.ActiveBoxes(1, 24, 32, 8, SMALL)
    one.push(rows, cols)
    for chunk in (1, 5, 12):
        parts = A.ActiveBoxes(1, 24, 32, 8, SMALL)
        for s in range(0, 12, chunk):
            parts.push(rows[s:s + chunk], cols[s:s + chunk])
        assert parts.frames == 12 and [parts.upto(i) for i in range(12)] == [one.upto(i) for i in range(12)]


def test_compose_host_puts_the_box_into_the_bicubic_frame():
    from fcvsr_amd.harness.niqe import bicubic_upscale
    rs = np.random.RandomState(0)
    lr = rs.randint(0, 256, (2, 1, 10, 14)).astype(np.uint8)
    sr = rs.randint(0, 256, (2, 1, 16, 24)).astype(np.uint8)
    out = A.compose_host(sr, lr, (2, 6, 4, 10))
    want = bicubic_upscale(lr, 4, out="int")
    assert out.dtype == np.uint8 and np.array_equal(out[..., 8:24, 16:40], sr)
    want[..., 8:24, 16:40] = sr
    assert np.array_equal(out, want)
    f = A.compose_host(sr.astype(np.float32), lr.astype(np.float32), (2, 6, 4, 10))
    assert f.dtype == np.float32 and np.array_equal(f[..., :8, :], bicubic_upscale(lr.astype(np.float32), 4)[..., :8, :].astype(np.float32))
    with pytest.raises(ValueError):
        A.compose_host(sr, lr, (2, 6, 4, 11))


def test_the_command_line():
    from fcvsr_amd import sr
    base = ["--model", "GShiftNet_S", "--weights", "w.pth", "--size", "480x270", "a", "b"]
    a = sr.parser().parse_args(base)
    assert a.active is None and a.active_limit == 24.0
    assert sr.parser().parse_args(["--active", "auto", "--active-limit", "16"] + base).active == "auto"
    assert sr.parser().parse_args(["--active", "auto", "--active-limit", "16"] + base).active_limit == 16.0
    assert sr.parser().parse_args(["--active", "34:236:0:480"] + base).active == (34, 236, 0, 480)
    for bad in ("34:236:0", "a:b:c:d", "letterbox"):
        with pytest.raises(SystemExit):
            sr.parser().parse_args(["--active", bad] + base)
