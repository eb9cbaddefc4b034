"""The integer sample rule (csrc/u8.h `quantised<PEAK>`, csrc/bicubic_up.h `up_result`) as a numpy f32 reference, the table of f32
inputs at which wrong spellings of it show, and those wrong spellings.  CPU only: numpy alone, no torch, nothing of fcvsr_amd.
tests/test_sample_rule_cpu.py shows that the table does what is said here; tests/test_sample_rule_gpu.py feeds it to every kernel
that ends in the rule.

The rule: sample = int(r(clamp(v, 0, 1) * PEAK)), the product ONE f32 multiply, r = trunc ("truncate") or round half to even
("round"), the clamp fmin(fmax(v, 0), 1) - so a NaN, which fmax drops in favour of the 0, gives sample 0.

Random floats never test it: v * PEAK lands on k + 0.5 with probability ~2^-24 * PEAK, so rintf, roundf and floorf(q + 0.5f) agree on
them, and so do one f32 multiply, an fma and an f64 multiply.  `table(peak)` holds, for peak 255 and 1023:
  tie        for every k in 0 .. peak-1 one f32 v with fl32(v * peak) == k + 0.5 (one whose exact product is the tie where there is one);
  tie_lo/hi  a v with fl32(v * peak) == k + 0.5 whose exact product lies below / above the tie: an exact (f64, fused) product rounds
             it to the other side;
  tie_nb     the two f32 neighbours of every `tie` entry;
  carry      (1023 only; 255 has none) v with fl32(v * 1023) == k + 1 and an exact product below k + 1: truncation gives k + 1 from
             the f32 product and k from an exact one;
  entry      the sample table's entries k / peak (the f32 division of hip.u8_table / hip.u16_table) - quantise(tab[k]) == k;
  entry_nb   their two neighbours;
  edge       -0.0, 0.0, the smallest subnormal, the largest f32 below 0, nextafter(1, 0), 1, nextafter(1, 2), 2, -1, +-3.4e38, +-inf;
  half       the preimage of the largest f32 below 0.5, where floorf(q + 0.5f) gives 1 (255 only: no f32 v has fl32(v * 1023) there,
             the products step over it);
  nan        one quiet NaN.
The positions are shuffled with a fixed seed: ties of even and odd k meet every lane of a 4-sample store.

`upscale_plane(factor, peak)` is the same idea for the second spelling (`up_result`, which clamps in sample units): the taps of
the x2 / x4 bicubic up-scale are k/128 and k/1024, so an integer plane of identical rows has exact sums, and columns found by search
give sums of exactly k + 0.5."""
import functools
from collections import namedtuple

import numpy as np

F32 = np.float32
PEAKS = (255, 1023)
MODES = ("truncate", "round")
KINDS = ("tie", "tie_lo", "tie_hi", "tie_nb", "carry", "entry", "entry_nb", "edge", "half", "nan")
KIND = {n: i for i, n in enumerate(KINDS)}
SEED = 20240607


def _clamp01(v):
    return np.fmin(np.fmax(v, F32(0)), F32(1))               # fmaxf / fminf: a NaN operand loses, so NaN -> 0


def _r(q, mode):
    if mode not in MODES:
        raise ValueError(f"mode: one of {MODES}, got {mode!r}")
    return np.trunc(q) if mode == "truncate" else np.rint(q)


def rule(v, peak, mode):
    """The samples of the f32 values `v` (any shape) at `peak` in `mode`, int64."""
    v = np.asarray(v, dtype=F32)
    q = _clamp01(v) * F32(peak)
    assert q.dtype == F32
    return _r(q, mode).astype(np.int64)


# ---- the wrong rules ------------------------------------------------------------------------------------------------------------------
# Each takes (v, peak, mode) as `rule` and returns int64 without wrapping to the container, so a value outside 0 .. peak shows as
# what it is.  MUTANTS maps a name to (function, the modes it concerns).

def _q(v, peak):
    return _clamp01(np.asarray(v, dtype=F32)) * F32(peak)


def _roundf(v, peak, mode):                                  # round half away from zero (q >= 0: floor(q + 0.5), exactly, in f64)
    q = _q(v, peak)
    return (np.trunc(q) if mode == "truncate" else np.floor(q.astype(np.float64) + 0.5)).astype(np.int64)


def _floor_half(v, peak, mode):                              # floorf(q + 0.5f): the sum is an f32
    q = _q(v, peak)
    return (np.trunc(q) if mode == "truncate" else np.floor(q + F32(0.5))).astype(np.int64)


def _exact_product(v, peak, mode):                           # f64 multiply (24 x 10 bits: exact), rounded to the integer once
    q = _clamp01(np.asarray(v, dtype=F32)).astype(np.float64) * float(peak)
    return _r(q, mode).astype(np.int64)


def _swapped(v, peak, mode):
    return rule(v, peak, "round" if mode == "truncate" else "truncate")


def _peak_plus_1(v, peak, mode):
    return rule(v, peak + 1, mode)


def _no_lower_clamp(v, peak, mode):                          # fminf(v, 1) alone: negative samples, and NaN -> PEAK
    q = np.fmin(np.asarray(v, dtype=F32), F32(1)) * F32(peak)
    return _r(np.maximum(q, F32(-2.0 ** 40)), mode).astype(np.int64)


def _no_upper_clamp(v, peak, mode):
    q = np.fmax(np.asarray(v, dtype=F32), F32(0)) * F32(peak)
    return _r(np.minimum(q, F32(2.0 ** 40)), mode).astype(np.int64)


def _other_clamp_order(v, peak, mode):                       # fmaxf(fminf(v, 1), 0): NaN -> PEAK
    q = np.fmax(np.fmin(np.asarray(v, dtype=F32), F32(1)), F32(0)) * F32(peak)
    return _r(q, mode).astype(np.int64)


MUTANTS = {
    "roundf": (_roundf, ("round",)),
    "floor_half": (_floor_half, ("round",)),
    "exact_product": (_exact_product, MODES),
    "modes_swapped": (_swapped, MODES),
    "peak_plus_1": (_peak_plus_1, MODES),
    "no_lower_clamp": (_no_lower_clamp, MODES),
    "no_upper_clamp": (_no_upper_clamp, MODES),
    "other_clamp_order": (_other_clamp_order, MODES),
}


def concerns(name, peak):
    """The modes in which mutant `name` can change a sample at `peak`.  An exact product never changes a truncated 8-bit sample: no
    f32 v has fl32(v * 255) on an integer with an exact product below it (24 + 8 bits round to 24 without crossing one)."""
    modes = MUTANTS[name][1]
    return ("round",) if (name, peak) == ("exact_product", 255) else modes


# ---- the table ------------------------------------------------------------------------------------------------------------------------

Table = namedtuple("Table", "peak values kind k")           # values f32 (n,), kind int (n,) index into KINDS, k int (n,) or -1


def _bits(v):
    return np.asarray(v, dtype=F32).view(np.int32)


def _around(centre, lo, hi):
    """The positive normal f32 values centre's bits + lo .. + hi (consecutive floats), centre first, then by distance."""
    offs = sorted(range(lo, hi + 1), key=lambda o: (abs(o), o))
    return (_bits(F32(centre)) + np.array(offs, dtype=np.int32)).view(F32)


def _nb(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))]


def sample_entries(peak):
    """The sample table of the integer entry points: entry k is the f32 division k / peak (what torch's `.float() / peak` gives)."""
    return np.arange(peak + 1, dtype=np.int32).astype(F32) / F32(peak)


EDGES = [F32(-0.0), F32(0.0), np.nextafter(F32(0), F32(1)), np.nextafter(F32(0), F32(-1)), np.nextafter(F32(1), F32(0)), F32(1),
         np.nextafter(F32(1), F32(2)), F32(2), F32(-1), F32(3.4e38), F32(-3.4e38), F32(np.inf), F32(-np.inf)]


@functools.lru_cache(maxsize=None)
def table(peak):
    """The `Table` of `peak` (255 or 1023), shuffled; deterministic."""
    if peak not in PEAKS:
        raise ValueError(f"peak: one of {PEAKS}, got {peak!r}")
    P, P64 = F32(peak), float(peak)
    rows = []                                                # (value, kind, k)
    for k in range(peak):
        tie = k + 0.5
        c = _around(tie / P64, -8, 8)
        c = c[(c * P) == F32(tie)]
        if c.size == 0:
            continue                                         # the CPU test demands a tie for every k
        exact = c.astype(np.float64) * P64
        on, lo, hi = c[exact == tie], c[exact < tie], c[exact > tie]
        first = on[0] if on.size else c[0]
        rows.append((first, "tie", k))
        rows += [(n, "tie_nb", k) for n in _nb(first)]
        if lo.size:
            rows.append((lo[0], "tie_lo", k))
        if hi.size:
            rows.append((hi[0], "tie_hi", k))
    for k1 in range(1, peak + 1):
        c = _around(k1 / P64, -8, 0)
        c = c[((c * P) == F32(k1)) & (c.astype(np.float64) * P64 < k1)]
        if c.size:
            rows.append((c[0], "carry", k1 - 1))
    for k, e in enumerate(sample_entries(peak)):
        rows.append((e, "entry", k))
        rows += [(n, "entry_nb", k) for n in _nb(e)]
    rows += [(e, "edge", -1) for e in EDGES]
    below_half = np.nextafter(F32(0.5), F32(0))
    c = _around(0.5 / P64, -8, 8)
    c = c[(c * P) == below_half]
    rows += [(c[0], "half", 0)] if c.size else []
    rows.append((F32(np.nan), "nan", -1))
    order = np.random.RandomState(SEED + peak).permutation(len(rows))
    values = np.array([rows[i][0] for i in order], dtype=F32)
    kind = np.array([KIND[rows[i][1]] for i in order], dtype=np.int64)
    ks = np.array([rows[i][2] for i in order], dtype=np.int64)
    for a in (values, kind, ks):
        a.setflags(write=False)
    return Table(peak, values, kind, ks)


def of_kind(t, *names):
    """Positions of the entries of the named kinds."""
    return np.flatnonzero(np.isin(t.kind, [KIND[n] for n in names]))


def finite(t):
    return np.flatnonzero(np.isfinite(t.values))


def changed(t, name, mode):
    """Positions of `t` at which mutant `name` gives another sample than the rule in `mode`."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.flatnonzero(MUTANTS[name][0](t.values, t.peak, mode) != rule(t.values, t.peak, mode))


@functools.lru_cache(maxsize=None)
def killers(peak, per=2):
    """{mode: positions}: for every mutant that concerns `mode`, the first `per` entries of every kind at which it changes a
    sample - the entries the one-sample launches repeat."""
    t = table(peak)
    out = {}
    for mode in MODES:
        pos = set()
        for name in MUTANTS:
            if mode not in concerns(name, peak):
                continue
            ch = changed(t, name, mode)
            for kd in np.unique(t.kind[ch]):
                pos.update(int(i) for i in ch[t.kind[ch] == kd][:per])
        out[mode] = np.array(sorted(pos), dtype=np.int64)
    return out


def short_list(peak):
    """Positions of the entries every site that takes one value per launch runs: {name: position}.  An even-k tie, an odd-k tie, a
    tie with an inexact product, a carried integer (1023 only), 1, nextafter(1, 2), a negative value, NaN."""
    t = table(peak)
    tie = of_kind(t, "tie")
    out = {"tie_even": int(tie[t.k[tie] % 2 == 0][0]), "tie_odd": int(tie[t.k[tie] % 2 == 1][0]),
           "tie_inexact_lo": int(of_kind(t, "tie_lo")[0]), "tie_inexact_hi": int(of_kind(t, "tie_hi")[0])}
    if peak == 1023:
        out["carry"] = int(of_kind(t, "carry")[0])
    bits = _bits(t.values)
    for name, v in (("one", F32(1)), ("above_one", np.nextafter(F32(1), F32(2))), ("negative", F32(-1))):
        out[name] = int(np.flatnonzero(bits == _bits(v))[0])
    out["nan"] = int(of_kind(t, "nan")[0])
    return out


def plane(peak, h, w, channels=1):
    """The table tiled (wrapping round) into an f32 (channels, h, w) array that holds every entry at least once."""
    t = table(peak)
    n = channels * h * w
    if n < t.values.size:
        raise ValueError(f"{channels} x {h} x {w} does not hold the {t.values.size} entries of the table")
    return np.resize(t.values, n).reshape(channels, h, w).copy()


def side(peak, multiple=1, channels=1):
    """The least side s, a multiple of `multiple`, with channels * s * s >= the table's length."""
    n = table(peak).values.size
    s = multiple
    while channels * s * s < n:
        s += multiple
    return s


def same_bits(a, b):
    """f32 arrays equal bit for bit (a NaN equals the same NaN, -0.0 differs from 0.0)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


def mean8(v):
    """harness.ensemble's merge of eight passes that all hold `v`: the fixed-order f32 sum, then * 0.125.  NOT v in general: 2v, 4v
    and 8v are exact, but the partial sums 3v, 5v, 6v and 7v need up to three more bits and are rounded, so about a third of the
    table comes out one ulp off (and +-3.4e38 overflows).  The entries with mean8(v) == v, bit for bit, still hold ties of both
    parities, inexact products and carried integers (tests/test_sample_rule_cpu.py counts them)."""
    v = np.asarray(v, dtype=F32)
    acc = v
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(7):
            acc = acc + v
        return acc * F32(0.125)


# ---- the up-scale family: planes whose contract value is an exact tie ---------------------------------------------------------------

UP_TAPS = {2: (np.array([[-3, 29, 111, -9], [-9, 111, 29, -3]], dtype=np.int64), 128),
           4: (np.array([[-45, 399, 745, -75], [-7, 93, 987, -49], [-49, 987, 93, -7], [-75, 745, 399, -45]], dtype=np.int64), 1024)}
UP_ROWS = 3

UpPlane = namedtuple("UpPlane", "factor peak plane num den tie k")   # plane uint (UP_ROWS, W); the rest per output column


def _reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def up_row_sums(row, factor):
    """The x`factor` up-scale of the integer row `row` in exact integers: numerators over the common denominator (128 / 1024)."""
    taps, den = UP_TAPS[factor]
    row = np.asarray(row, dtype=np.int64)
    o = np.arange(row.size * factor)
    first = (o - factor // 2) // factor - 1
    num = np.zeros(o.size, dtype=np.int64)
    for j in range(4):
        num += taps[o % factor, j] * row[_reflect(first + j, row.size)]
    return num, den


@functools.lru_cache(maxsize=None)
def upscale_plane(factor, peak):
    """An integer plane of UP_ROWS identical rows for the x`factor` bicubic up-scale at `peak`: for every phase of the taps and both
    parities of k, four columns found by brute-force search whose tap sum is exactly k + 0.5 with 0 <= k < peak; then a 0 / peak
    edge that overshoots below 0 and above peak.  `tie` marks the output columns whose value is a tie inside [0, peak], `k` its
    integer part (valid where `tie`)."""
    taps, den = UP_TAPS[factor]
    rs = np.random.RandomState(SEED + 7 * factor + peak)
    cols = []
    for phase in range(factor):
        for parity in (0, 1):
            while True:
                c = rs.randint(0, peak + 1, size=(4096, 4))
                s = c @ taps[phase]
                ok = (np.mod(s, den) == den // 2) & (s > 0) & (s < peak * den) & ((s // den) % 2 == parity)
                if ok.any():
                    cols += [int(x) for x in c[np.flatnonzero(ok)[0]]]
                    break
    cols += [0, 0, 0, peak, peak, peak, 0, 0, 0]
    row = np.array(cols, dtype=np.int64)
    num, den = up_row_sums(row, factor)
    tie = (np.mod(num, den) == den // 2) & (num > 0) & (num < peak * den)
    dt = np.uint8 if peak == 255 else np.uint16
    pl = np.repeat(row[None, :], UP_ROWS, axis=0).astype(dt)
    return UpPlane(factor, peak, pl, num, den, tie, num // den)


def up_half_even(v, peak):
    """np.around(np.clip(v, 0, peak)): the contract's (and `up_result`'s) rounding of the f32 sums v."""
    return np.rint(np.clip(np.asarray(v, dtype=F32), 0, peak)).astype(np.int64)


def up_half_away(v, peak):
    """The wrong contract: half away from zero."""
    return np.floor(np.clip(np.asarray(v, dtype=F32), 0, peak).astype(np.float64) + 0.5).astype(np.int64)
