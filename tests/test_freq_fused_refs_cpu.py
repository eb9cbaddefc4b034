"""CPU: the float64 references of tests/freq_fused_refs.py (fcvsr_freq_mlp3, fcvsr_freq_head, fcvsr_convcorr_strip) are, at every case
of tests/test_freq_fused_gpu.py, (1) equal to plain torch conv2d / relu on the same rounded operands in f64, (2) wide enough for a
correct f32 evaluation that walks the channels in another order (worst |got - ref| / bound < 1) and (3) tight enough to reject every
wrong kernel of `WRONG_*` wherever its `*_cannot_differ` does not say why it cannot show.  Also here: the `spectrum` inputs leave the
f16 range, the `w4zero` bound is the residual and store terms alone, and the argument the engine's strip decomposition rests on - the
CorrBlock lookup is exactly zero at every column >= 8 - holds for the f64 lookup at full width."""
import math

import pytest
import torch
import torch.nn.functional as F

import freq_fused_refs as R
from freq_kernel_refs import corr_lookup
from infer_kernel_refs import BF16, D, F32

ids = lambda c: "-".join(str(v) for v in c)


def bf(t):
    return t.to(BF16).double()


def conv(x, w):
    """1x1 convolution, no bias: x (N, cin, H, W) f64, w (cout, cin) f32 rounded to bf16."""
    return F.conv2d(x, bf(w)[:, :, None, None])


def nchw(t):
    """(P, C) -> (1, C, P, 1)."""
    return t.double().t()[None, :, :, None]


def nhwc(t):
    return t[0, :, :, 0].t()


def close(tag, v, want):
    assert float((v - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), f"{tag}: not the plain torch formulation"


def inside(tag, v, ref, bound):
    d = (v.double() - ref).abs()
    worst = float(torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0)).max())
    assert worst < 1.0, f"{tag}: a correct f32 evaluation reaches {worst:.3f} of the bound"


def leaves(tag, v, ref, bound):
    d = torch.nan_to_num((v.double() - ref).abs(), nan=math.inf)
    assert bool((d > bound).any()), f"{tag}: the bound admits this wrong variant"


def reject(kernel, wrongs, cannot, evaluate, ref, bound):
    for w in wrongs:
        if not cannot(w):
            leaves(f"{kernel} {w}", evaluate(w), ref, bound)


# ---- mlp3 -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.MLP3_CASES, ids=ids)
def test_mlp3_reference(case):
    B, H, Wf, nd, _, _, name = case
    p = R.mlp3_inputs(*case)
    ref, bound = R.mlp3_ref(p, nd)
    assert ref.dtype == D and bound.dtype == D and ref.shape == bound.shape == (nd, B * H * Wf, 128)
    xa, xb = R.mlp3_operands(p, nd)
    for d in range(nd):
        a, b = nchw(xa[d]), nchw(xb[d])
        t = bf(F.relu(conv(bf(torch.cat([a, b], 1)), p["W0"])))
        t = bf(F.relu(conv(t, p["W2"])))
        close(f"mlp3 direction {d}", ref[d], nhwc((conv(t, p["W4"]) + a) - b))
    f32 = R.mlp3_ref(p, nd, cd=F32)[0]
    inside("mlp3", f32, ref, bound)
    inside("mlp3 stored as bf16", bf(f32), ref, bound)
    reject("mlp3", R.WRONG_MLP3, lambda w: R.mlp3_cannot_differ(w, case), lambda w: R.mlp3_ref(p, nd, wrong=w)[0], ref, bound)
    if name == "spectrum":
        assert float(xa.abs().max()) > R.F16_MAX and float(xb.abs().max()) > R.F16_MAX
    if name == "w4zero":                                     # sharp: nothing but the two residual roundings and the store is admitted
        a, d = xa.double().abs(), (xa.double() - xb.double()).abs()
        assert bool((bound < 2.0 ** -7 * d + 2.0 ** -22 * a).all())
        assert float((d / a.clamp_min(1e-30)).median()) < 2.0 ** -8          # ... on a residual that cancels


def test_mlp3_cases_cover_the_issue():
    cs = R.MLP3_CASES
    assert {c[:3] for c in cs} == {(1, 1, 1), (1, 1, 127), (1, 1, 128), (1, 1, 129), (2, 9, 23), (1, 25, 41)}
    assert {(c[:3], c[3]) for c in cs} == {(s, nd) for s in R.MLP3_SHAPES for nd in (1, 2)}
    assert {(c[4], c[5]) for c in cs} == {(l, s) for l in ("separate", "record") for s in (128, 136)}
    for s in [(2, 9, 23), (1, 25, 41)]:
        assert {c[6] for c in cs if c[:4] == s + (2,)} == set(R.SETS)
        assert {c[4] for c in cs if c[:4] == s + (2,)} == {"separate", "record"}
    assert max(c[0] * c[1] * c[2] for c in cs) <= 1100


# ---- head -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_tag)
def test_head_reference(case):
    dt, nhid, npix, stride, name = case
    p = R.head_inputs(*case)
    ref, bound = R.head_ref(p)
    assert ref.dtype == D and bound.dtype == D and ref.shape == bound.shape == (npix, 4)
    x = p["rec"][:, p["off"]:p["off"] + 128]
    t = bf(F.relu(conv(bf(nchw(x)), p["W0"])))
    if nhid == 2:
        t = bf(F.relu(conv(t, p["Wmid"])))
    close("head", ref, nhwc(conv(t, p["Wl"])))
    inside("head", R.head_ref(p, cd=F32)[0], ref, bound)
    reject("head", R.WRONG_HEAD, lambda w: R.head_cannot_differ(w, case), lambda w: R.head_ref(p, wrong=w)[0], ref, bound)
    if name == "spectrum":
        assert float(x.abs().max()) > R.F16_MAX


def test_head_cases_cover_the_issue():
    cs = R.HEAD_CASES
    for dt, strides in ((F32, {128, 384}), (BF16, {128, 256})):
        for nhid in (1, 2):
            assert {(c[2], c[3]) for c in cs if c[:2] == (dt, nhid)} >= {(n, s) for n in (1, 127, 128, 129, 414) for s in strides}
    assert {c[:2] for c in cs if c[4] == "spectrum"} == {(F32, 1), (F32, 2)}


# ---- strip ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.STRIP_CASES, ids=ids)
def test_strip_reference(case):
    B, H, Wf, xs = case
    p = R.strip_inputs(*case)
    ref, bound = R.strip_ref(p, case)
    assert ref.dtype == D and bound.dtype == D and ref.shape == bound.shape == (2 * B, H, Wf, 4)
    own = ~torch.isnan(ref)
    assert bool(own[:, :, :xs].all()) and not bool(own[:, :, xs:].any()) and not bool(bound[:, :, xs:].any())
    assert bool((p["corr"][..., 81:] != 0).all()) and bool(torch.isfinite(p["corr"]).all())
    assert R.pack(p["W0"]).shape == (128, 256) and not bool(R.pack(p["W0"])[:, 209:].any())
    for d in range(2):
        for b in range(B):
            x = torch.cat([p["off"][d * B + b, :, :xs].double(), bf(p["corr"][b, :, :, :81])], -1).permute(2, 0, 1)[None]
            t = bf(F.relu(conv(x, p["W0"])))
            t = bf(F.relu(conv(t, p["W2"])))
            close(f"strip {d} {b}", ref[d * B + b, :, :xs], conv(t, p["W4"])[0].permute(1, 2, 0))
    inside("strip", R.strip_ref(p, case, cd=F32)[0][own], ref[own], bound[own])
    reject("strip", R.WRONG_STRIP, lambda w: R.strip_cannot_differ(w, case), lambda w: R.strip_ref(p, case, wrong=w)[0][own], ref[own],
           bound[own])


def test_strip_cases_cover_the_issue():
    assert set(R.STRIP_CASES) == {(B, H, Wf, xs) for B in (1, 3) for H in (1, 5) for (Wf, xs) in [(5, 5), (8, 8), (19, 8), (19, 3)]}


# ---- every wrong variant shows somewhere ----------------------------------------------------------------------------------------------

def test_each_wrong_variant_can_differ_somewhere():
    for kernel, wrongs, cases, cannot in (("mlp3", R.WRONG_MLP3, R.MLP3_CASES, R.mlp3_cannot_differ),
                                          ("head", R.WRONG_HEAD, R.HEAD_CASES, R.head_cannot_differ),
                                          ("strip", R.WRONG_STRIP, R.STRIP_CASES, R.strip_cannot_differ)):
        for w in wrongs:
            assert any(not cannot(w, c) for c in cases), f"{kernel} {w}: no case can show it"
    assert "unrounded" not in "".join(R.WRONG_MLP3 + R.WRONG_HEAD + R.WRONG_STRIP)


# ---- the engine's strip decomposition ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.COMPOSE_CASES, ids=ids)
def test_lookup_is_zero_beyond_the_strip_and_the_decomposition_is_the_full_operation(case):
    B, H, Wf = case
    assert (B, H) == (2, 5) and Wf in (5, 8, 19)
    p = R.compose_inputs(*case)
    look, lb = corr_lookup(p["x1f"], p["x2f"], 128, Wf)
    assert float(look.abs().max()) > 0.0
    assert torch.equal(look[:, :, 8:], torch.zeros_like(look[:, :, 8:])) and not bool(lb[:, :, 8:].any())
    ref, bound = R.convcorr_full(p)
    assert ref.shape == bound.shape == (2 * B, H, Wf, 4)
    inside("convcorr", R.convcorr_full(p, cd=F32)[0], ref, bound)
    # head on `off` alone over the grid, the strip x < min(Wf, 8) recomputed with the lookup over it: the same function in f64
    xs = min(Wf, 8)
    parts = R.head(p["off"], p["W0"][:, :128], p["W2"], p["W4"])[0]
    s = R.strip(p["off"], look[:, :, :xs].float(), p["W0"], p["W2"], p["W4"], B, H, Wf, xs)[0]
    parts[:, :, :xs] = s[:, :, :xs]
    close("decomposition", parts, ref)
