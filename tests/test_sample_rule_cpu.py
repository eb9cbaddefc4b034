"""CPU: the reference side of tests/test_sample_rule_gpu.py.  The table of tests/sample_rule_cases.py holds what it claims (conditions,
not measurements), its numpy `rule` is the harness's torch spelling and the test reference's on every finite entry, every wrong
spelling changes samples of the table, and the up-scale planes put exact ties into the host contracts of the second spelling."""
import numpy as np
import pytest
import torch

import infer_kernel_refs as R
import sample_rule_cases as S

PEAKS = pytest.mark.parametrize("peak", S.PEAKS)


@PEAKS
def test_table_holds_a_tie_for_every_k_inexact_products_and_carried_integers(peak):
    t = S.table(peak)
    v, P = t.values, np.float32(peak)
    count = {n: int((t.kind == i).sum()) for n, i in S.KIND.items()}
    print(f"[table {peak}] {v.size} entries: {count}")
    assert v.dtype == np.float32 and v.size % 256 != 0
    tie = S.of_kind(t, "tie", "tie_lo", "tie_hi")
    assert np.array_equal(v[tie] * P, (t.k[tie] + 0.5).astype(np.float32))                       # f32 product == k + 0.5, exactly
    assert np.array_equal(np.unique(t.k[S.of_kind(t, "tie")]), np.arange(peak))                  # 255 of 255, 1023 of 1023
    exact = v.astype(np.float64) * float(peak)                                                   # 24 x 10 bits: exact in f64
    lo, hi = S.of_kind(t, "tie_lo"), S.of_kind(t, "tie_hi")
    assert bool((exact[lo] < t.k[lo] + 0.5).all()) and bool((exact[hi] > t.k[hi] + 0.5).all())
    assert np.unique(t.k[np.concatenate([lo, hi])]).size >= peak - 1                             # 254 and 1022
    assert min(lo.size, hi.size) >= peak // 4
    carry = S.of_kind(t, "carry")
    if peak == 1023:
        assert carry.size >= 500
        assert np.array_equal(v[carry] * P, (t.k[carry] + 1).astype(np.float32)) and bool((exact[carry] < t.k[carry] + 1).all())
    else:
        assert carry.size == 0
    nb = S.of_kind(t, "tie_nb")
    assert nb.size == 2 * peak and not bool(np.isin(v[nb] * P, np.arange(peak) + np.float32(0.5)).all())
    entry = S.of_kind(t, "entry")
    assert np.array_equal(np.sort(v[entry]), (torch.arange(peak + 1, dtype=torch.int32).float() / peak).numpy())
    assert S.of_kind(t, "entry_nb").size == 2 * (peak + 1) and S.of_kind(t, "edge").size == len(S.EDGES) == 13
    assert S.of_kind(t, "nan").size == 1 and int(np.isnan(v).sum()) == 1
    half = S.of_kind(t, "half")
    below = np.nextafter(np.float32(0.5), np.float32(0))
    if peak == 255:
        assert half.size == 1 and v[half[0]] * P == below
    else:                                                    # the products of consecutive floats step over it: none exists
        c = np.sort(S._around(0.5 / peak, -64, 64)) * P      # consecutive floats: monotone products that straddle it
        assert half.size == 0 and bool((np.diff(c) >= 0).all()) and c.min() < below < c.max() and below not in c


@PEAKS
def test_table_is_shuffled_over_the_lanes_of_a_four_sample_store(peak):
    t = S.table(peak)
    again = S.table.__wrapped__(peak)
    assert S.same_bits(t.values, again.values) and np.array_equal(t.kind, again.kind)              # deterministic
    tie = S.of_kind(t, "tie")
    for parity in (0, 1):
        lanes = np.bincount(tie[t.k[tie] % 2 == parity] % 4, minlength=4)
        assert int(lanes.min()) >= peak // 16, (parity, lanes)
    for s in (S.side(peak), S.side(peak, 4), S.side(peak, 16)):
        p = S.plane(peak, s, s)
        assert s * s >= t.values.size > (s - 1) * (s - 1) * (s == S.side(peak)) and S.same_bits(p.reshape(-1)[:t.values.size], t.values)


@pytest.mark.parametrize("mode", S.MODES)
@PEAKS
def test_three_spellings_one_rule_on_every_finite_entry(peak, mode):
    """numpy `rule` == tests/infer_kernel_refs.quantise == harness.infer._quantised (torch on the host)."""
    from fcvsr_amd.harness.infer import _quantised
    t = S.table(peak)
    v = t.values[S.finite(t)]
    assert v.size == t.values.size - 3                                                           # +inf, -inf, NaN
    want = S.rule(v, peak, mode)
    assert int(want.min()) == 0 and int(want.max()) == peak
    tv = torch.from_numpy(v.copy())
    assert np.array_equal(R.quantise(tv, peak, mode).numpy().astype(np.int64), want)
    assert np.array_equal(_quantised(tv, mode, float(peak)).astype(np.int64), want)


@PEAKS
def test_every_wrong_rule_changes_samples_of_the_table(peak):
    t = S.table(peak)
    for name in S.MUTANTS:
        modes = S.concerns(name, peak)
        assert modes, name
        for mode in modes:
            n = S.changed(t, name, mode).size
            print(f"[mutant {peak} {mode}] {name}: {n} of {t.values.size} samples change")
            assert n > 0, (name, mode)
    # which entries catch which: half-away and floor(q + 0.5f) at ties (the latter also at `half`), the exact product at inexact
    # ties and carried integers, the clamps at the edges and at NaN
    kinds = lambda name, mode: {S.KINDS[i] for i in np.unique(t.kind[S.changed(t, name, mode)])}
    ties = {"tie", "tie_lo", "tie_hi", "tie_nb"}             # a tie's neighbour can be a second preimage of the same tie
    assert {"tie"} <= kinds("roundf", "round") <= ties
    assert {"tie_lo", "tie_hi"} <= kinds("exact_product", "round") <= ties
    assert kinds("other_clamp_order", "round") == kinds("other_clamp_order", "truncate") == {"nan"}
    assert kinds("no_lower_clamp", "truncate") == {"edge", "nan"} and kinds("no_upper_clamp", "truncate") == {"edge"}
    if peak == 255:
        assert "half" in kinds("floor_half", "round") and kinds("exact_product", "truncate") == set()
    else:
        assert kinds("exact_product", "truncate") >= {"carry"}
    for mode in S.MODES:
        k = S.killers(peak)[mode]
        assert 0 < k.size <= 64
        for name in S.MUTANTS:
            if mode in S.concerns(name, peak):
                assert np.intersect1d(k, S.changed(t, name, mode)).size > 0, (name, mode)


@PEAKS
def test_nan_gives_sample_0_and_the_other_clamp_order_gives_peak(peak):
    nan = np.array([np.nan], dtype=np.float32)
    for mode in S.MODES:
        assert S.rule(nan, peak, mode)[0] == 0
        assert S.MUTANTS["other_clamp_order"][0](nan, peak, mode)[0] == peak
        assert S.MUTANTS["no_lower_clamp"][0](nan, peak, mode)[0] == peak


@pytest.mark.parametrize("mode", S.MODES)
@PEAKS
def test_round_trip_of_both_sample_tables(peak, mode):
    """rule(tab[k]) == k for the tables of hip.u8_table / hip.u16_table (their host expression), and every product is exact."""
    from fcvsr_amd import hip
    tab = hip._INT_FORMATS[torch.uint8 if peak == 255 else torch.uint16][2]().numpy()
    assert S.same_bits(tab, S.sample_entries(peak)) and tab.size == peak + 1
    assert np.array_equal(S.rule(tab, peak, mode), np.arange(peak + 1))
    assert np.array_equal(tab * np.float32(peak), np.arange(peak + 1, dtype=np.float32))


@PEAKS
def test_short_list_and_what_survives_the_mean_of_eight_equal_passes(peak):
    t = S.table(peak)
    sl = S.short_list(peak)
    assert set(sl) == {"tie_even", "tie_odd", "tie_inexact_lo", "tie_inexact_hi", "one", "above_one", "negative", "nan"} | \
        ({"carry"} if peak == 1023 else set())
    assert t.k[sl["tie_even"]] % 2 == 0 and t.k[sl["tie_odd"]] % 2 == 1 and np.isnan(t.values[sl["nan"]])
    m = S.mean8(t.values)
    same = m.view(np.int32) == t.values.view(np.int32)
    print(f"[mean8 {peak}] {int(same.sum())} of {same.size} entries come back bit for bit")
    assert not bool(same.all())                              # 3v, 5v, 6v, 7v round: the sum of eight equal f32 is not 8v
    for kinds, parity in ((("tie",), 0), (("tie",), 1), (("tie_lo",), None), (("tie_hi",), None)) + \
            (((("carry",), None),) if peak == 1023 else ()):
        pos = S.of_kind(t, *kinds)
        if parity is not None:
            pos = pos[t.k[pos] % 2 == parity]
        assert int(same[pos].sum()) >= pos.size // 4, (kinds, parity, int(same[pos].sum()))
    with np.errstate(over="ignore"):
        pow2 = np.float32(8) * t.values                      # 8v is exact (a power of two) unless it overflows: +-3.4e38
    back = pow2 * np.float32(0.125)
    off = np.flatnonzero(back.view(np.int32) != t.values.view(np.int32))
    assert set(np.abs(t.values[off]).tolist()) == {float(np.float32(3.4e38))}


# ---- the up-scale family ---------------------------------------------------------------------------------------------------------------

UP = pytest.mark.parametrize("factor,peak", [(f, p) for f in (2, 4) for p in S.PEAKS])


def _planted(u):
    """(rows, cols) of the planted pixels of the up-scaled plane and their k."""
    cols = np.flatnonzero(u.tie)
    rows = np.arange(S.UP_ROWS * u.factor)
    return rows, cols, u.k[cols]


@UP
def test_upscale_planes_put_exact_ties_into_both_host_contracts(factor, peak):
    from fcvsr_amd.harness.niqe import UPSCALE_TAPS, bicubic_upscale
    from fcvsr_amd.harness.resize import imresize_host
    taps, den = S.UP_TAPS[factor]
    assert np.array_equal(UPSCALE_TAPS[factor] * den, taps)                                      # the contract's taps, as integers
    u = S.upscale_plane(factor, peak)
    rows, cols, k = _planted(u)
    assert u.plane.dtype == (np.uint8 if peak == 255 else np.uint16) and int(u.plane.max()) == peak and bool((u.plane == u.plane[0]).all())
    n_even, n_odd = int((k % 2 == 0).sum()) * rows.size, int((k % 2 == 1).sum()) * rows.size
    print(f"[upscale x{factor} peak {peak}] plane {u.plane.shape}, planted pixels: {n_even} on even k, {n_odd} on odd k; "
          f"range {u.num.min() / u.den} .. {u.num.max() / u.den}")
    assert n_even >= 4 and n_odd >= 4 and n_even + n_odd >= 8
    assert u.num.min() < 0 and u.num.max() > peak * u.den                                        # overshoot on both sides
    want = u.num.astype(np.float64) / u.den                                                      # exact: dyadic
    for f32 in (bicubic_upscale(u.plane, factor, out="f32"), imresize_host(u.plane, scale=factor, out="f32")):
        assert f32.shape == (S.UP_ROWS * factor, u.plane.shape[1] * factor)
        assert np.array_equal(f32, np.repeat(want[None], f32.shape[0], axis=0))                  # identical rows, exact sums
        assert np.array_equal(f32[np.ix_(rows, cols)], np.repeat((k + 0.5)[None], rows.size, axis=0))
    even = S.up_half_even(want, peak)
    for got in (bicubic_upscale(u.plane, factor, out="int"), imresize_host(u.plane, scale=factor, out="int")):
        assert got.dtype == u.plane.dtype and np.array_equal(got.astype(np.int64), np.repeat(even[None], got.shape[0], axis=0))
    assert np.array_equal(even[cols], k + (k % 2)) and int(even.min()) == 0 and int(even.max()) == peak
    away = S.up_half_away(want, peak)
    assert np.array_equal(np.flatnonzero(away != even), cols[k % 2 == 0])                        # a half-away contract differs there
