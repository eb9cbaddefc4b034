"""GPU: the composition of the kernels in fcvsr_amd/engine.py, stage by stage, against f64 replays of the engine's own taps
(tests/engine_stage_refs.py: what a stage is, what the emulation E holds, why K = 4), in every shipped configuration - and the same
forwards once more with every scratch and intermediate tensor filled with NaN, then with the largest finite value, before the kernels write
it: a kernel that leaves an element unwritten (a pad channel times a zero weight, the strip outside x < 8) then shows in the result.

Stage replay, measured on an MI355X (profiles/NOTES.md has the table per stage, mode and case): worst max(rms(e) / rms(E), max|e| / max|E|)
over all taps 1.77 in the 16-bit modes (stage 3, f32 in every mode; 1.00 wherever a 16-bit rounding dominates) and 2.44 in f32 (stage 2, on
the four DC values of a 4-channel tap; 1.5 without the DC pixel); the bound is K = 4.  Two rounding points came out of the first runs and
are in the emulation since: the f32 convolutions are one fmaf chain (2.0-2.7 rms, up to 5.3 max against torch's blocked f32 sum), and the
convolution epilogue adds its residuals one at a time, (acc + x?f) - x2f (5.02 on mgaa1.off_b of full_20x24 before).  Poisoned scratch: all
64 configurations bit-equal."""
import numpy as np
import pytest
import torch

import engine_stage_refs as R
from helpers import get_ctor, load_case, shapes_for, weights_for
from fcvsr_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

GPU_CASES = ["S_16x20", "S_b2_72x36", "full_20x24", "rgbS_16x20"]
SETS = {"gold": 1.0, "x20": 20.0}
EDGE_SHAPES = [(3, 7, 1, 4, 4), (1, 7, 1, 8, 36), (5, 7, 1, 12, 8), (2, 7, 1, 36, 68)]   # test_edge_shapes_fused_path_against_oracle
_cache = {}


def case_weights(case, wset):
    """(x, f32 weights, f64 weights); the x20 set multiplies MGAA.MConvB.{i}.conv2.weight by 20 (the warp then crosses pixel cells)."""
    if (case, wset) not in _cache:
        x, _, meta = load_case(case)
        p = weights_for(meta)
        if wset == "x20":
            for k in p:
                if k.startswith("MGAA.MConvB.") and k.endswith(".conv2.weight"):
                    p[k] = p[k] * SETS[wset]
        _cache[case, wset] = (x, meta, p, R.params64(p))
    return _cache[case, wset]


def build(meta, p, prec, trunk16, fused=True, streams=1):
    model = get_ctor(meta["ctor"])(**meta["kwargs"])
    model.load_state_dict(p, strict=True)
    model = model.to("cuda")
    model.precision, model.trunk16, model.streams, model.use_graph = prec, trunk16, streams, False
    model.fold_f1 = model.fuse_tail = model.fuse_rcb_l0 = fused
    return model


def run_with_taps(model, call):
    eng = model._get_engine()
    eng.taps = {}
    try:
        with torch.no_grad():
            y = call()
        torch.cuda.synchronize()
        return y.cpu(), {k: v.cpu() for k, v in eng.taps.items()}
    finally:
        eng.taps = None


def replay_check(case, wset, prec, trunk16, fused=True):
    x, meta, p, p64 = case_weights(case, wset)
    model = build(meta, p, prec, trunk16, fused)
    xd = x.cuda()
    y, taps = run_with_taps(model, lambda: model(xd))
    assert torch.equal(taps["out"], y)
    # precision "f32" ignores trunk16: where the taps are the same bits, the replay (its fmaf-chain emulation takes seconds) is shared
    hit = _cache.get((case, wset, prec, fused))
    if prec == "f32" and hit is not None and all(torch.equal(taps[k], v) for k, v in hit[0].items()):
        res = hit[1]
    else:
        res = R.judge(p64, x, taps, R.Mode(prec, trunk16))
        _cache[case, wset, prec, fused] = (taps, res)
    by = {}
    for k, v in res.items():
        s = R.stage_of(k)
        if s not in by or max(v) > max(res[by[s]]):
            by[s] = k
    print(f"RATIOS {case} {wset} {prec} trunk16={int(trunk16)} fused={int(fused)} "
          + " ".join(f"{s}:{res[by[s]][0]:.2f}/{res[by[s]][1]:.2f}" for s in sorted(by)))
    bad = {k: v for k, v in res.items() if not max(v) <= R.K}
    k, v = R.worst(res)
    assert not bad, f"worst: stage {R.stage_of(k)} {k} {v:.2f} of {len(bad)} taps beyond K = {R.K}: " \
                    f"{ {k: tuple(round(q, 2) for q in v) for k, v in sorted(bad.items())[:12]} }"


@pytest.mark.parametrize("wset", list(SETS))
@pytest.mark.parametrize("trunk16", [False, True])
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", GPU_CASES)
def test_stage_replay(case, prec, trunk16, wset):
    replay_check(case, wset, prec, trunk16)


@pytest.mark.parametrize("wset", list(SETS))
@pytest.mark.parametrize("trunk16", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_stage_replay_unfused(prec, trunk16, wset):
    """fold_f1, fuse_tail and fuse_rcb_l0 switched off: the launch sequences the fused kernels replace."""
    replay_check("S_16x20", wset, prec, trunk16, fused=False)


# ---- poisoned scratch ---------------------------------------------------------------------------------------------------------------

def poison(monkeypatch, fill):
    """Every tensor of Engine._new (all of the forward's scratch and intermediates) is filled before it is handed out: float tensors with
    NaN (fill = "nan") or the largest finite value ("max": 3e38 in f32) - max / ReLU / clamp instructions swallow a NaN operand -, integer
    tensors with 0xA5 bytes."""
    from fcvsr_amd.engine import Engine
    orig = Engine._new

    def new(dev, *shape, dtype=torch.float32):
        t = orig(dev, *shape, dtype=dtype)
        if t.is_floating_point():
            t.fill_(float("nan") if fill == "nan" else 3e38 if dtype == torch.float32 else torch.finfo(dtype).max)
        else:
            t.view(torch.uint8).fill_(0xA5)
        return t
    monkeypatch.setattr(Engine, "_new", staticmethod(new))


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def poison_check(monkeypatch, model, call):
    with torch.no_grad():
        call()                                               # first call of a configuration: caches, single-stream warm-up
    y0, t0 = run_with_taps(model, call)
    assert t0 and (t0["out"].shape != y0.shape or torch.equal(bits(t0["out"]), bits(y0)))   # (streams: a sub-batch)
    for fill in ("nan", "max"):
        with monkeypatch.context() as mp:
            poison(mp, fill)
            y1, t1 = run_with_taps(model, call)
        assert set(t1) == set(t0)
        bad = [k for k in t0 if not torch.equal(bits(t0[k]), bits(t1[k]))]
        assert not bad, (fill, sorted(bad, key=R.stage_of)[:8])
        assert torch.equal(bits(y0), bits(y1)), fill


@pytest.mark.parametrize("prec,trunk16", [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)])
@pytest.mark.parametrize("case", GPU_CASES)
def test_poisoned_scratch(monkeypatch, case, prec, trunk16):
    x, meta, p, _ = case_weights(case, "gold")
    model = build(meta, p, prec, trunk16)
    xd = x.cuda()
    poison_check(monkeypatch, model, lambda: model(xd))


@pytest.mark.parametrize("trunk16", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_poisoned_scratch_unfused(monkeypatch, prec, trunk16):
    x, meta, p, _ = case_weights("S_16x20", "gold")
    model = build(meta, p, prec, trunk16, fused=False)
    xd = x.cuda()
    poison_check(monkeypatch, model, lambda: model(xd))


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("word", ["u8", "u16"])
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", ["S_16x20", "rgbS_16x20"])
def test_poisoned_scratch_integer_frames(monkeypatch, case, prec, word, quantise):
    x, meta, p, _ = case_weights(case, "gold")
    model = build(meta, p, prec, True)
    full = 255 if word == "u8" else 1023
    xi = torch.from_numpy((x.numpy() * full).round().astype(np.uint8 if word == "u8" else np.uint16)).cuda()
    fwd = model.super_resolve_u8 if word == "u8" else model.super_resolve_u16
    poison_check(monkeypatch, model, lambda: fwd(xi, quantise))


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_poisoned_scratch_edge_shapes(monkeypatch, shape, prec, streams):
    """Images smaller than one tile of any kernel, partial tiles everywhere, batches that do not divide over the streams."""
    meta = dict(ctor="GShiftNet_S", kwargs={}, gain=0.5)
    model = build(meta, synthetic_state_dict(shapes_for(meta), gain=0.5), prec, True, streams=streams)
    xd = torch.from_numpy(np.random.RandomState(sum(shape)).rand(*shape).astype(np.float32)).cuda()
    poison_check(monkeypatch, model, lambda: model(xd))
