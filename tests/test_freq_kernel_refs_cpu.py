"""CPU: the float64 references of tests/freq_kernel_refs.py are (1) pinned to the oracle / a plain torch formulation of the same operation,
(2) wide enough for a correct f32 evaluation at every input of tests/test_freq_kernels_gpu.py, and (3) tight enough to reject the wrong
kernels listed per kernel in the references (`*_WRONG`) at those very inputs: a derived bound must be left by every variant, a measured
entry's rejection figure (the smallest worst |wrong - ref| / scale over the variants) must be finite, positive and at least 8 x above
what a correct f32 evaluation shows.  Where a variant cannot differ at a shape, the references' `*_cannot_differ` say why, and the test
asserts that it indeed does not."""
import math
import unittest.mock as mock

import pytest
import torch
import torch.nn.functional as F

import freq_kernel_refs as R
from freq_kernel_refs import BF16, D, F16, F32

ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def inside(tag, v, ref, bound):
    bad = (v.double() - ref).abs() > bound
    assert not bool(bad.any()), f"{tag}: a correct f32 evaluation leaves the bound at {int(bad.sum())} of {bad.numel()} elements"


def leaves(tag, v, ref, bound):
    d = torch.nan_to_num((v.double() - ref).abs(), nan=math.inf)
    assert bool((d > bound).any()), f"{tag}: the bound admits this wrong variant"


def same(tag, v, ref):
    assert torch.equal(torch.nan_to_num(v.double(), nan=-1.0), torch.nan_to_num(ref, nan=-1.0)), f"{tag}: said not to differ, but it does"


# ---- corr_lookup ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CORR_CASES, ids=ids)
def test_corr_lookup_reference(case):
    from oracle import fcvsr_oracle as O
    B, Cn, H, Wf, ps = case
    a, b = R.corr_inputs(*case)
    ref, bound = R.corr_lookup(a, b, Cn, Wf)
    # the oracle on NCHW f64 (its divisor is the f32 sqrt(C) too: torch.sqrt of an f32 tensor)
    want = O.corr_lookup(a[..., :Cn].permute(0, 3, 1, 2).double(), b[..., :Cn].permute(0, 3, 1, 2).double())
    assert float((ref[..., :81].permute(0, 3, 1, 2) - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
    assert torch.equal(ref[..., 81:], torch.zeros_like(ref[..., 81:]))
    xs = min(Wf, 8)
    strip, _ = R.corr_lookup(a, b, Cn, xs)
    assert torch.equal(strip, ref[:, :, :xs])
    inside("corr_lookup", R.corr_lookup(a, b, Cn, Wf, cd=F32)[0], ref, bound)
    for w in R.CORR_WRONG:
        v = R.corr_lookup(a, b, Cn, Wf, wrong=w)[0]
        if R.corr_cannot_differ(w, B, Cn, H, Wf):
            same(f"corr_lookup {w}", v, ref)
        else:
            leaves(f"corr_lookup {w}", v, ref, bound)


def test_corr_cases_cover_the_issue():
    assert {c[1] for c in R.CORR_CASES} == {128, 64} and {c[2] for c in R.CORR_CASES} == {1, 63, 64, 65, 72}
    assert {c[3] for c in R.CORR_CASES} == {1, 2, 5, 6, 9} and {c[0] for c in R.CORR_CASES} == {1, 3}
    assert any(c[4] > c[1] for c in R.CORR_CASES)


# ---- channel_sum ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.SUM_CASES, ids=ids)
def test_channel_sum_reference(case):
    B, Cn, H, W = case
    x = R.sum_inputs(*case)
    ref, bound = R.channel_sum(x)
    assert torch.allclose(ref, x.double().sum(dim=(1, 2)), rtol=0, atol=1e-9)
    inside("channel_sum", R.channel_sum(x, cd=F32)[0], ref, bound)
    for w in R.SUM_WRONG:
        v = R.channel_sum(x, wrong=w)[0]
        if R.sum_cannot_differ(w, Cn, H * W):
            same(f"channel_sum {w}", v, ref)
        else:
            leaves(f"channel_sum {w}", v, ref, bound)


# ---- ca_gate --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GATE_CASES, ids=ids)
def test_ca_gate_reference(case):
    c, cr, B, neg = case
    p = R.gate_inputs(*case)
    ref, scale = R.ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"])
    mean = (p["sum"].double() * R.f32(p["inv_hw"])).view(B, c, 1, 1)
    want = torch.sigmoid(F.conv2d(F.relu(F.conv2d(mean, p["w1"].double().view(cr, c, 1, 1))), p["w2"].double().view(c, cr, 1, 1)))
    assert float((ref - want.view(B, c)).abs().max()) <= 1e-15
    if neg:
        assert torch.equal(ref, torch.full_like(ref, 0.5))
    assert bool((scale >= ref).all())
    fig = R.gate_rejection(*case)
    own = R._ratio(R.ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"], cd=F32)[0] - ref, scale)
    assert 0 < fig < math.inf and 8 * own < fig, (own, fig)
    for w in R.GATE_WRONG:
        if R.gate_cannot_differ(w, neg):
            same(f"ca_gate {w}", R.ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"], wrong=w)[0], ref)


# ---- convblk_tail ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.TAIL_CASES, ids=ids)
def test_convblk_tail_reference(case):
    ndir, B, H, W = case
    p = R.tail_inputs(*case)
    for A in (3, 6):
        for g0 in range(A):
            ref, bound, own = R.convblk_tail(p["u"], p["gate"], p["sim"], B, ndir, A, g0)
            assert int(own.sum()) == 4 * ndir * B * H * W
            # plain formulation: CA(u) + u times sim, channels (2p, 2p+1) of the re block and of the im block
            o = (p["u"].double() * p["gate"].double()[:, None, None, :] + p["u"].double()) * p["sim"].double().repeat(ndir, 1, 1, 1)
            for d in range(ndir):
                pr = g0 + d * A
                assert torch.equal(ref[..., 2 * pr:2 * pr + 2], o[d * B:(d + 1) * B, ..., :2])
                assert torch.equal(ref[..., 4 * A + 2 * pr:4 * A + 2 * pr + 2], o[d * B:(d + 1) * B, ..., 2:])
            v32 = R.convblk_tail(p["u"], p["gate"], p["sim"], B, ndir, A, g0, cd=F32)[0]
            inside("convblk_tail", v32[own], ref[own], bound[own])
            for w in R.TAIL_WRONG:
                v, _, vown = R.convblk_tail(p["u"], p["gate"], p["sim"], B, ndir, A, g0, wrong=w)
                if R.tail_cannot_differ(w, ndir, g0):
                    same(f"convblk_tail {w}", v, ref)
                else:                                        # a float the call owns is wrong, or one it does not own is written
                    moved = bool((vown != own).any())
                    both = own & vown
                    assert moved or bool(((v[both] - ref[both]).abs() > bound[both]).any()), f"convblk_tail {w}: admitted"


# ---- convblk --------------------------------------------------------------------------------------------------------------------------

def _oracle_conv_blk(p):
    from oracle import fcvsr_oracle as O
    prm = {"h.conv1.weight": p["w1"].double(), "h.conv2.weight": p["w2"].double(), "h.relu.weight": p["slope"].double(),
           "h.CA.conv_du.0.weight": p["cw1"].double().view(4, 4, 1, 1), "h.CA.conv_du.2.weight": p["cw2"].double().view(4, 4, 1, 1)}
    return O.conv_blk(prm, "h", p["x"].double().permute(0, 3, 1, 2))


@pytest.mark.parametrize("shape", R.CONVBLK_SHAPES, ids=ids)
@pytest.mark.parametrize("K", R.CONVBLK_K)
def test_convblk_reference(K, shape):
    H, W, B, slope = shape
    p = R.convblk_inputs(K, H, W, B, slope)
    (u, ub), (ref, scale, own) = R.convblk(p, B)
    A, g0 = R.CONVBLK_A, p["g0"]
    want = _oracle_conv_blk(p).permute(0, 2, 3, 1) * p["sim"].double().repeat(2, 1, 1, 1)           # (:1494-1498) times sim
    for d in range(2):
        pr = g0 + d * A
        got = torch.cat([ref[..., 2 * pr:2 * pr + 2], ref[..., 4 * A + 2 * pr:4 * A + 2 * pr + 2]], -1)
        w = want[d * B:(d + 1) * B]
        # the reference takes 1/HW and the slope as the f32 values the kernel receives: 2^-24 relative on the mean, at most
        assert float((got - w).abs().max()) <= 2e-7 * max(1.0, float(w.abs().max()))
    assert int(own.sum()) == 8 * B * H * W and bool((scale[own] >= ref[own].abs() * (1 - 1e-12)).all())
    (u32, _), (r32, _, _) = R.convblk(p, B, cd=F32)
    inside("convblk u", u32, u, ub)
    own_fig = R._ratio((r32.double() - ref)[own], scale[own])
    fig = R.convblk_rejection(K, H, W, B, slope)
    assert 0 < fig and 8 * own_fig < fig, (own_fig, fig)
    for w in R.CONVBLK_WRONG:
        (uw, _), (rw, _, _) = R.convblk(p, B, wrong=w)
        if R.convblk_cannot_differ(w, K, H, W):
            same(f"convblk {w}", rw, ref)
        elif w in ("clamp", "nozero"):                       # the padding variants already leave u's derived bound
            leaves(f"convblk u {w}", uw, u, ub)


def test_convblk_rejection_figures_are_finite_somewhere():
    """A single tile dropped leaves the gate at 0.5 exactly - a finite figure; no figure of the set is zero."""
    figs = [R.convblk_rejection(K, *s) for K in (1, 5) for s in R.CONVBLK_SHAPES]
    assert all(f > 0 for f in figs) and any(f < math.inf for f in figs)


# ---- DivEnh ---------------------------------------------------------------------------------------------------------------------------

def test_divenh_chain_is_the_oracle_s_divenh_loop():
    """oracle.mffr (band split, the DivEnh loop, the final CALayer) == the chain on the oracle's own bands with the gates of the
    ca_gate reference: pins the chain (carry = None: unrounded) and, once more, the gate."""
    from oracle import fcvsr_oracle as O
    g = R.gen(90)
    B, Cn, H, W, Q = 2, 16, 8, 12, R.DIVENH_Q
    x = torch.randn(B, Cn, H, W, generator=g, dtype=D)
    prm = {}
    for i in range(Q):
        prm[f"m.DivEnh_block.{i}.a"], prm[f"m.DivEnh_block.{i}.b"] = torch.randn(Cn, generator=g, dtype=D), torch.randn(Cn, generator=g, dtype=D)
        prm[f"m.DivEnh_block.{i}.ca.conv_du.0.weight"] = torch.randn(4, Cn, 1, 1, generator=g, dtype=D)
        prm[f"m.DivEnh_block.{i}.ca.conv_du.2.weight"] = torch.randn(Cn, 4, 1, 1, generator=g, dtype=D)
    prm["m.ca.conv_du.0.weight"], prm["m.ca.conv_du.2.weight"] = torch.randn(4, Cn, 1, 1, generator=g, dtype=D), torch.randn(Cn, 4, 1, 1, generator=g, dtype=D)
    taps = {}
    want = O.mffr(prm, "m", x, Q, taps)
    bands = [taps["mffr.bands"][:, i].permute(0, 2, 3, 1).contiguous() for i in range(Q)]
    p = dict(f=bands, a=[prm[f"m.DivEnh_block.{i}.a"] for i in range(Q)], b=[prm[f"m.DivEnh_block.{i}.b"] for i in range(Q)],
             g1=[torch.zeros(B, Cn, dtype=D) for _ in range(Q)], g2=[torch.zeros(B, Cn, dtype=D) for _ in range(Q)],
             mean_sum=bands[0].sum(dim=(1, 2)), inv_hw=1.0 / (H * W))
    # the gates of band i depend on the sums of its e1, e2, which depend on the state the earlier gates gave: band by band (the
    # gates not known yet are zero and reach nothing before their band), with the exact 1/HW and 0.2 of the oracle
    with mock.patch.object(R, "f32", float):
        for i in range(Q):
            res, _ = R.divenh_chain(p, carry=None)
            w1, w2 = prm[f"m.DivEnh_block.{i}.ca.conv_du.0.weight"].view(4, Cn), prm[f"m.DivEnh_block.{i}.ca.conv_du.2.weight"].view(Cn, 4)
            p["g1"][i] = R.ca_gate(res[f"e{i}"][0][0], 1.0 / (H * W), w1, w2)[0]
            p["g2"][i] = R.ca_gate(res[f"e{i}"][0][1], 1.0 / (H * W), w1, w2)[0]
        res, _ = R.divenh_chain(p, carry=None)
        so = res[f"so{Q - 1}"][0]
        assert torch.allclose(res[f"nx{Q - 1}"][0][0], so.sum(dim=(1, 2)), rtol=1e-13, atol=1e-12)
        gate = R.ca_gate(res[f"nx{Q - 1}"][0][0], 1.0 / (H * W), prm["m.ca.conv_du.0.weight"].view(4, Cn), prm["m.ca.conv_du.2.weight"].view(Cn, 4))[0]
    got = (so * gate[:, None, None, :]).permute(0, 3, 1, 2) + x
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("case", sorted({c[:4] for c in R.DIVENH_CASES}), ids=ids)
def test_divenh_reference(case):
    Cn, H, W, B = case
    p = R.divenh_inputs(*case)
    res, states = R.divenh_chain(p)
    r32, _ = R.divenh_chain(p, cd=F32, given=states)
    for name, (ref, bound) in res.items():
        inside(f"divenh {name}", r32[name][0], ref, bound)
    # nx{i} of the new state is e{i+1} of the stored one up to the rounding of the store
    for i in range(R.DIVENH_Q - 1):
        assert bool(((res[f"nx{i}"][0] - res[f"e{i + 1}"][0]).abs() <= res[f"nx{i}"][1] + res[f"e{i + 1}"][1]).all())
    assert torch.equal(res["e0"][0][1], torch.zeros_like(res["e0"][0][1])) and torch.equal(res["e0"][1][1], torch.zeros_like(res["e0"][1][1]))
    for w in R.DIVENH_WRONG:
        wr, _ = R.divenh_chain(p, wrong=w)
        for group, kinds in R.DIVENH_GROUPS.items():
            names = [n for n in res if n[:2] in kinds or n[:1] in kinds]
            out = any(bool(((wr[n][0] - res[n][0]).abs() > res[n][1]).any()) for n in names)
            if R.divenh_cannot_differ(w, group, H * W):
                assert not out, f"divenh {w} {group}: said not to differ"
            else:
                assert out, f"divenh {w}: every bound of {group} admits it"


# ---- ContextBlock pooling -------------------------------------------------------------------------------------------------------------

def _oracle_context(p):
    from oracle import fcvsr_oracle as O
    r = p["r"].double().permute(0, 3, 1, 2)
    Cn = r.shape[1]
    prm = {"g.conv_mask.weight": p["wmask"].double().view(1, Cn, 1, 1), "g.channel_add_conv.0.weight": p["w1"].double().view(Cn, Cn, 1, 1),
           "g.channel_add_conv.2.weight": p["w2"].double().view(Cn, Cn, 1, 1)}
    return (O.context_block(prm, "g", r) - r)[:, :, 0, 0]


def _gc_check(p, part, stress):
    ref, scale = R.gc_context(p, part)
    want = _oracle_context(p)                                # the oracle's slope is the f64 0.2, the kernel's the f32 one: 1.5e-8 apart
    assert float((ref - want).abs().max()) <= 2e-8 * float(scale.max())
    own = R._ratio(R.gc_context(p, part, cd=F32)[0] - ref, scale)
    fig = R.gc_rejection(p, part, stress)
    assert fig > 0 and 8 * own < fig, (own, fig)
    bid, pad = part(p["r"].shape[1], p["r"].shape[2])
    for w in R.GC_WRONG:
        if R.gc_cannot_differ(w, stress, bid, pad):
            v = R.gc_context(p, part, wrong=w)[0]
            assert float((v - ref).abs().max()) <= 1e-9 * float(scale.max()), f"gc {w}: said not to differ"
    if stress == "span":
        assert not bool(torch.isfinite(R.gc_context(p, part, F32, "nomax")[0]).all()), "exp without the maximum must overflow here"
    return fig


@pytest.mark.parametrize("case", R.GC_CASES, ids=ids)
def test_gc_context_reference(case):
    B, Cn, H, W, stress = case
    _gc_check(R.gc_inputs(B, Cn, H, W, stress, R.block_partition), R.block_partition, stress)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(R.GC_TILE_SETS))
def test_gc_tile_reference(name, dt):
    for (B, H, W, stress), p in zip(R.GC_TILE_SETS[name], R.gc_tile_inputs(name, dt)):
        if H * W > 4096 and dt == F16:
            continue                                         # the 270-tile level once is enough here (the GPU test runs both)
        assert p["r"].dtype == dt
        _gc_check(p, R.tile_partition, stress)


def test_tile_partition_counts():
    bid, pad = R.tile_partition(36, 929)
    assert int(bid.max()) + 1 == 270 and int(pad.sum()) == 270 * 128 - 36 * 929
    bid, pad = R.block_partition(257, 256)
    assert int(bid.max()) + 1 == 257 and int(pad.sum()) == 0


# ---- stage 2 at the largest admitted nparts ----------------------------------------------------------------------------------------------

def test_stage2_reference_and_limit():
    Cn = 64
    n = R.stage2_max_nparts(Cn)
    assert (2 * Cn + n) * 4 == R.STAGE2_DYNAMIC_LIMIT and (2 * Cn + n + 1) * 4 > R.STAGE2_DYNAMIC_LIMIT
    p = R.stage2_inputs(Cn, 300)
    ref, scale = R.stage2_reference(p)
    # one pixel per tile: gc_context on r with wmask chosen so that the logits are the given ones is the same thing; plain torch
    m = torch.softmax(p["logit"].double(), 1)
    t = (m[:, :, None] * p["r"].double()).sum(1) @ p["w1"].double().t()
    want = F.leaky_relu(t, R.f32(0.2)) @ p["w2"].double().t()
    assert float((ref - want).abs().max()) <= 1e-14
    own = R._ratio(R.stage2_reference(p, cd=F32)[0] - ref, scale)
    pm = R.stage2_inputs(Cn, n)
    rm, sm = R.stage2_reference(pm)
    fig = R._ratio(R.stage2_reference(pm, drop_last=True)[0] - rm, sm)
    assert fig > 0 and 8 * own < fig, (own, fig)
    assert pm["parts"].numel() * 4 < 5 * 2 ** 20
