"""CPU: the scheduler of the streamed YUV path (`harness.stream.StreamPlan`, `AutoCuts`) makes the windows of the finished stream
without knowing its length, never ahead of the frames, inside the ring bound."""
import numpy as np
import pytest

from fcvsr_amd.harness.shots import cuts_from_sad, windows_for
from fcvsr_amd.harness.stream import FAR, AutoCuts, StreamPlan

PADDINGS = ["replicate", "reflection", "reflection_circle", "circle"]
T = 7


def _run(N, padding, batch, chunk, cuts, eof_with_last):
    """Feed N frames in chunks; returns the rows in the order they were handed out."""
    plan = StreamPlan(T, padding, batch, cuts)
    bound = 2 * batch + 2 * (T - 1)
    rows, left, floors = [], N, []
    while not plan.eof:
        n = min(chunk, left)
        assert plan.frames - plan.keep_from() + n <= bound, (N, padding, batch, chunk, cuts, plan.frames, plan.keep_from())
        left -= n
        plan.arrived(n, eof=(left == 0 and eof_with_last) or n == 0)
        groups = plan.ready()
        for centres, grows in groups:
            assert len(centres) == len(grows) and centres == list(range(len(rows), len(rows) + len(centres)))
            assert len(centres) == batch or (plan.eof and centres[-1] == N - 1), "only the last group may be short"
            if not plan.eof:
                assert all(0 <= f < plan.frames for r in grows for f in r), "a window names a frame that has not arrived"
                assert centres[-1] + T // 2 < plan.frames
            if N >= T:                    # in a sequence shorter than the window `window_indices` itself leaves the sequence
                assert all(f >= k for r in grows for f in r for k in floors), "a window names a frame keep_from() had given up"
            rows += grows
        floors = [plan.keep_from()]
    assert plan.keep_from() == N and plan.ready() == []
    assert plan.finish() == (None if cuts is None else list(cuts))
    return rows


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("batch", [1, 2, 8])
def test_the_windows_of_the_finished_stream(padding, batch):
    for N in range(1, 41):
        all_cuts = [None] + ([[1], [N - 1]] if N >= 2 else []) + ([[5, 6]] if N >= 7 else [])
        for cuts in all_cuts:
            want = windows_for(range(N), T, N, padding, cuts)
            for chunk in sorted({1, 3, batch}):
                got = _run(N, padding, batch, chunk, cuts, eof_with_last=bool((N + chunk) % 2))
                assert got == want, (N, padding, batch, chunk, cuts)


def test_nothing_runs_before_the_look_ahead_has_arrived():
    plan = StreamPlan(T, "replicate", 2, None)
    plan.arrived(4)
    assert plan.ready() == []                                             # centre 1 wants frame 4, centre 0 has no partner yet
    plan.arrived(1)
    assert [c for c, _ in plan.ready()] == [[0, 1]] and plan.keep_from() == 0
    plan.arrived(20)
    assert [c for c, _ in plan.ready()][-1] == [20, 21] and plan.keep_from() == 22 - 6
    circle = StreamPlan(T, "circle", 1, None)
    circle.arrived(6)
    assert circle.ready() == []                                           # the window of frame 0 names frames 4, 5, 6
    circle.arrived(1)
    assert circle.ready()[0][1] == [windows_for([0], T, 100, "circle", None)[0]]


def test_a_cut_at_or_beyond_the_end_raises_at_the_end():
    for cut in (9, 12):
        plan = StreamPlan(T, "replicate", 4, [3, cut])
        plan.arrived(9, eof=True)
        rows = [r for _, g in plan.ready() for r in g]
        assert rows == windows_for(range(9), T, 9, "replicate", [3])      # every frame before it is served
        with pytest.raises(ValueError):
            plan.finish()
    for bad in ([0], [4, 4], [5, 3], [1.5], "scdet"):
        with pytest.raises(ValueError):
            StreamPlan(T, "replicate", 4, bad)
    with pytest.raises(ValueError):
        StreamPlan(T, "mirror", 4, None)
    with pytest.raises(ValueError):
        StreamPlan(6, "replicate", 4, None)


def _sads(n_pairs, spikes, seed):
    rs = np.random.RandomState(seed)
    sad = rs.randint(1000, 3000, n_pairs).astype(np.uint64)
    for i in spikes:
        if i < n_pairs:
            sad[i] = rs.randint(40000, 60000)
    return sad


@pytest.mark.parametrize("n_pairs,spikes", [(1, [0]), (1, []), (2, [0]), (2, [1]), (3, [0, 2]), (30, [0, 9, 10, 17, 29]),
                                            (30, [1, 2, 28]), (64, [5, 33, 34, 35, 60])])
def test_incremental_cuts_equal_the_whole_list(n_pairs, spikes):
    count, bits, thr = 20 * 18, 8, 10.0
    sad = _sads(n_pairs, spikes, seed=n_pairs + len(spikes))
    want = cuts_from_sad(sad, count, bits, thr)
    if n_pairs >= 2:
        assert want, "the case has cuts to find"
    auto, told = AutoCuts(count, bits, thr), []
    assert auto.known_upto == 0
    for i, s in enumerate(sad):                                           # pair i: frame i + 1 has arrived
        new = auto.push([s])
        assert all(max(k, 2) <= i + 1 for k in new), "a cut was announced before frame max(k, 2) arrived"
        told += new
        assert auto.known_upto == (i + 1 if i + 1 >= 2 else 0)
        assert told == [k for k in want if k <= auto.known_upto]
    told += auto.end()
    assert told == want and auto.cuts == want and auto.known_upto == FAR
    # in chunks, and a threshold every score reaches: the lone pair of a two-frame stream scores 0.0
    chunked = AutoCuts(count, bits, thr)
    assert sum((chunked.push(sad[i:i + 5]) for i in range(0, n_pairs, 5)), []) + chunked.end() == want
    zero = AutoCuts(count, bits, 0.0)
    assert zero.push(sad) + zero.end() == cuts_from_sad(sad, count, bits, 0.0)


@pytest.mark.parametrize("padding", PADDINGS)
def test_auto_cuts_feed_the_plan(padding):
    count, bits, N, batch = 20 * 18, 8, 31, 4
    sad = _sads(N - 1, [0, 11, 12, 25], seed=3)
    cuts = cuts_from_sad(sad, count, bits)
    assert len(cuts) >= 3
    want = windows_for(range(N), T, N, padding, cuts)
    for chunk in (1, 3, 4):
        plan, auto, rows = StreamPlan(T, padding, batch, "auto"), AutoCuts(count, bits), []
        for s in range(0, N, chunk):
            e = min(N, s + chunk)
            assert plan.frames - plan.keep_from() + (e - s) <= 2 * batch + 12
            plan.cuts_known(auto.push(sad[max(s - 1, 0):e - 1]), auto.known_upto)
            if e == N:
                plan.cuts_known(auto.end(), FAR)
            plan.arrived(e - s, eof=e == N)
            for centres, g in plan.ready():
                assert plan.eof or all(f < plan.frames for r in g for f in r)
                rows += g
        assert rows == want and plan.finish() == cuts
