"""CPU: the stage references of tests/engine_stage_refs.py are pinned to the oracle, a correct 16-bit evaluation fits under K = 4 with room
to spare, and the bound rejects named wiring errors - which the whole-model output checks do not.

Why stage by stage.  test_matrix_core_modes_against_reference asserts 68 dB / 3e-3 (bf16) and 86 dB / 5e-4 (f16) on the final output only.
Mutating the f64 oracle with the golden weights and comparing each mutant with the unmutated oracle gives (PSNR, max-abs of the output):

    wiring mutant                                                        S_16x20            full_20x24
    all warp offsets = 0 (the whole rfft2 -> ... -> irfft2 branch dead)  131 dB, 1.3e-6     125 dB, 2.8e-6
    offsets x/y swapped, or negated                                      131-133 dB         126-130 dB
    CorrBlock lookup = 0, or (i, j) transposed                           135-140 dB         137 dB
    every iteration uses MConvB.0                                        110 dB             101 dB
    every LeakyReLU 0.2 -> 0.1                                           77 dB, 5.4e-4      65.5 dB, 2.3e-3
    ContextBlock = identity                                              73 dB, 7.6e-4      67 dB, 1.7e-3

The first four rows pass even the f32 output tolerance of 1e-4 and the last two pass the bf16 limits on the S case: the final output does not
reject them (test_whole_output_is_blind measures it again on this file's own mutants), and that is the point of this file.

Weight sets: the golden weights ("gold"), whose warp offsets are 0.003-0.07 px rms and never leave a pixel cell, and the same weights with
MGAA.MConvB.{i}.conv2.weight multiplied by 20 ("x20"): mgaa1.offsets_f is then 1.5 px rms with 22 % of its entries beyond one pixel on
S_16x20 (1.65 px, 17 % on full_20x24), so the warp crosses cells and image borders.  mgaa2's offsets stay small at this scale (0.05 px;
its inputs are the aligned features), and so do the RGB twin's (0.06 px).

Mutants are judged under the bf16 bound with the f32 trunk, Mode("bf16", trunk16=False).  Findings (profiles/NOTES.md has the table):
  * no_mean cannot be separated at all: band 0 of the l2h list is the highest band, whose mask nearly vanishes at DC.  Its spatial mean
    is below a tenth of its rms, and the term the mean enters, 0.2 a mean f, is then of the size of the f32 rounding of mffr.out:
    0.0-0.3x the bound (test_mean_removal_is_below_f32_rounding asserts that this is the reason).
  * ctx_identity, rcb_slope_01 and offs_f_for_b are rejected (beyond the bound) but by 1.7-3.1x, not 4x, in bf16: a BlockRCB output is
    x + 2R + ..., and the ContextBlock / slope share of R is a few times the bf16 operand error of the block's four 3x3 layers.  They are
    rejected by >= 4x under the f16 bound, which is what the test asserts for them.
  * with bf16 trunk storage (trunk16) the 2^-9 store of al, mffr.out and the block outputs is larger than the warp's whole contribution to
    al and than the 0.2 a t f term of DivEnh: offs_*, factor_02, ctx_identity, rcb_slope_01 then sit at 0.2-1.5x the bound."""
import math

import pytest
import torch

import engine_stage_refs as R
from helpers import load_case, weights_for
from oracle import fcvsr_oracle as O

CPU_CASES = ["S_16x20", "full_20x24", "rgbS_16x20"]
SETS = {"gold": 1.0, "x20": 20.0}
WEAK = {"ctx_identity", "rcb_slope_01", "offs_f_for_b"}      # rejected by >= 4x under the f16 bound only (docstring)
NOOP = {"no_mean"}
_cache = {}


def scaled_weights(meta, scale):
    p = weights_for(meta)
    if scale != 1.0:
        for k in p:
            if k.startswith("MGAA.MConvB.") and k.endswith(".conv2.weight"):
                p[k] = p[k] * scale
    return p


def setup(case, wset):
    """(p32, p64, x, the oracle's f64 taps, their f64 replay): computed once and shared, never modified."""
    if (case, wset) not in _cache:
        x, _, meta = load_case(case)
        p = scaled_weights(meta, SETS[wset])
        p64 = R.params64(p)
        taps = {}
        with torch.no_grad():
            O.forward(p64, x.double(), taps)
        _cache[case, wset] = (p, p64, x, taps, R.replay(p64, x, taps))
    return _cache[case, wset]


@pytest.mark.parametrize("wset", list(SETS))
@pytest.mark.parametrize("case", CPU_CASES)
def test_replay_reproduces_oracle(case, wset):
    _, _, _, taps, rep = setup(case, wset)
    assert set(rep) == set(taps)
    bad = {k: float((rep[k] - v).abs().max()) / max(1.0, float(v.abs().max())) for k, v in taps.items()}
    bad = {k: v for k, v in bad.items() if not v <= 1e-12}
    assert not bad, bad


@pytest.mark.parametrize("case", ["S_16x20", "full_20x24"])
def test_x20_offsets_cross_pixel_cells(case):
    taps = setup(case, "x20")[3]
    o = taps["mgaa1.offsets_f"]
    assert float((o.abs() > 1).double().mean()) >= 0.15
    assert R.rms(taps["mgaa2.offsets_f"]) < 0.2
    assert float(setup(case, "gold")[3]["mgaa1.offsets_f"].abs().max()) < 1.0


@pytest.mark.parametrize("wset", list(SETS))
@pytest.mark.parametrize("case", CPU_CASES)
def test_f32_oracle_passes(case, wset):
    p, p64, x, _, _ = setup(case, wset)
    t32 = {}
    with torch.no_grad():
        O.forward(p, x, t32)
    res = R.judge(p64, x, t32, R.Mode("f32"))
    k, v = R.worst(res)
    assert v <= R.K, (k, res[k])


@pytest.mark.parametrize("trunk16", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("wset", list(SETS))
@pytest.mark.parametrize("case", CPU_CASES)
def test_standin_engine_within_2(case, wset, prec, trunk16):
    """The stand-in: the emulation evaluated in f32 (every convolution accumulated in f32, every stage fed from the stand-in's own taps)
    with each stage output rounded to its stored dtype."""
    _, p64, x, _, _ = setup(case, wset)
    st = R.replay(p64, x, {}, R.Mode(prec, trunk16, cd=torch.float32), chain=True)
    res = R.judge(p64, x, st, R.Mode(prec, trunk16))
    k, v = R.worst(res)
    assert v <= 2.0, (k, res[k])


def rejection(case, wset, name, mode):
    """How far beyond the bound the mutant's stage sits: max over its taps of max(rms ratio, max ratio) / K."""
    _, p64, x, taps, rep = setup(case, wset)
    stage = R.MUTANTS[name][0]
    key = (case, wset, mode.prec, mode.T, stage)
    if key not in _cache:
        _cache[key] = R.replay(p64, x, taps, mode, stages=[stage])
    mt = R.replay(p64, x, taps, mut=name, stages=[stage])
    return R.worst(R.ratios(mt, {k: rep[k] for k in mt}, _cache[key]))[1] / R.K


def test_at_least_25_mutants():
    assert len(set(R.MUTANTS) - WEAK - NOOP) >= 25


@pytest.mark.parametrize("name", sorted(set(R.MUTANTS) - NOOP))
def test_mutant_rejected_at_its_stage(name):
    mode = R.Mode("f16" if name in WEAK else "bf16", False)
    sets = ["x20"] if R.MUTANTS[name][1] else list(SETS)
    got = {(c, s): rejection(c, s, name, mode) for c in CPU_CASES for s in sets}
    print(name, {k: round(v, 1) for k, v in got.items()})
    if name in WEAK:                                         # still beyond the bf16 bound itself
        assert all(rejection(c, "x20", name, R.Mode("bf16", False)) > 1.0 for c in CPU_CASES)
    assert min(got.values()) >= 4.0, got


def test_mean_removal_is_below_f32_rounding():
    """Why `no_mean` is no mutant: the band DivEnh centres has next to no mean to remove."""
    for case in CPU_CASES:
        f0 = setup(case, "gold")[3]["mffr.bands"][:, 0]
        assert float(f0.mean(dim=(2, 3)).abs().max()) <= 0.1 * R.rms(f0)
        assert rejection(case, "gold", "no_mean", R.Mode("bf16", False)) < 1.0


@pytest.mark.parametrize("name", ["lookup_zero", "lookup_transposed", "mconvb0", "offs_xy_swapped", "offs_negated"])
def test_whole_output_is_blind(name):
    """A whole forward of the f64 oracle with the mutant wired in passes the f32 output tolerance of the parity tests (1e-4), and with it the
    16-bit limits, on the golden weights - while its own stage rejects it by >= 4x the bound (on the x20 set for the warp mutants)."""
    _, p64, x, taps, _ = setup("S_16x20", "gold")
    out = R.replay(p64, x, {}, mut=name, chain=True)["out"]
    d = out - taps["out"]
    psnr = 20 * math.log10(255 / (255 * R.rms(d)))
    print(name, round(psnr, 1), float(d.abs().max()))
    assert float(d.abs().max()) <= 1e-4 and psnr >= 100.0
