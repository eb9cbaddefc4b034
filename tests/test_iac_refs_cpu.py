"""CPU: the float64 references of tests/iac_refs.py.
(a) On offsets that are finite and in range each one equals oracle.fcvsr_oracle (warp_bilinear, sac_kernel1_twice, one iteration of
    iac) evaluated in f64, to 1e-12 of the tensor's largest entry; the tile-by-tile evaluation equals the plain one.
(b) At the inputs and shapes of tests/test_iac_kernels_gpu.py the bounds tell a wrong kernel from a right one: every deliberately wrong
    f64 variant leaves `bound` at one element or more at every shape where it can differ, and the true formula evaluated in f32 (and
    stored in the test's dtype) stays inside it everywhere, at every planted offset class - which is where the k of every bound is
    checked without a GPU.
(c) The offset fields hold every planted class, in x only, in y only and in both."""
import pytest
import torch

import iac_refs as R
from iac_refs import BF16, F16, F32, D

TOL = 1e-12
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
sid = lambda s: "x".join(map(str, s))


def close(name, got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert err <= TOL * max(float(ref.abs().max()), 1e-300), f"{name}: {err:.3e}"


def nchw(t):
    return t.permute(0, 3, 1, 2)


def offending(wrong, ref, bound):
    return int(((wrong.double() - ref).abs() > bound).sum())


def accepts(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{name}: a correct f32 evaluation leaves the bound, worst err / bound {worst:.3f}"
    return worst


# ---- (a) the references against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES, ids=sid)
def test_references_are_the_oracle_on_finite_offsets_in_range(shape):
    """Offsets randn * 3 clamped so that every position stays inside (-2, W+1) x (-2, H+1): the guard is silent, the oracle's f64
    position equals the reference's f32 one (the offsets are multiples of 1/64, the sums exact)."""
    from oracle import fcvsr_oracle as O
    B, H, W = shape
    Cn = 4
    g = R.gen(200, B, H, W)
    prev, fin = torch.randn(B, H, W, Cn, generator=g), torch.randn(B, H, W, Cn, generator=g)
    K = torch.randn(B, H, W, 3 * Cn, generator=g)
    off = (torch.randn(B, H, W, 2, generator=g) * 3.0 * 64).round() / 64
    gx, gy = torch.arange(W).view(1, 1, W), torch.arange(H).view(1, H, 1)
    off[..., 0] = torch.minimum(torch.maximum(off[..., 0], -1.5 - gx), W + 0.5 - gx)
    off[..., 1] = torch.minimum(torch.maximum(off[..., 1], -1.5 - gy), H + 0.5 - gy)
    p64, o64, k64, f64 = nchw(prev).double(), nchw(off).double(), nchw(K).double(), nchw(fin).double()
    s_o = O.warp_bilinear(p64, o64)
    s, bs = R.warp(prev, off)
    close("warp", nchw(s), s_o)
    v, bv = R.sac_v(prev, K)
    kk = k64.reshape(B, Cn, 3, H, W)
    sp = torch.nn.functional.pad(p64, (0, 0, 1, 1), mode="replicate")
    close("sac_v", nchw(v), sum(sp[:, :, t:t + H] * kk[:, :, t] for t in range(3)))
    for slope in R.SLOPES:
        want = O.sac_kernel1_twice(s_o, k64) + f64
        want = torch.where(want >= 0, want, want * R.f32(slope))
        ref, bound = R.iac_step(prev, off, K, fin, slope)
        close("iac_step", nchw(ref), want)
        close("tiled 16", R.iac_step_tiled(prev, off, K, fin, slope, 16), ref)
        close("tiled 14", R.iac_step_tiled(prev, off, K, fin, slope, 14), ref)
        assert bool((bound >= 0).all()) and bool((bs >= 0).all()) and bool((bv >= 0).all())
    # one iteration of the oracle's iac (slope 0.1, K in its A * 6C layout, prev = feat_in)
    Kfull = torch.cat([k64, torch.zeros_like(k64)], 1)
    ref, _ = R.iac_step(prev, off, K, prev, 0.1)
    want = O.iac(p64, Kfull, [o64], 1)
    assert float((nchw(ref) - want).abs().max()) <= 1e-7 * max(float(want.abs().max()), 1.0)      # the oracle's slope is the f64 0.1
    h, _ = R.sac_h(prev, K, fin, 0.1)
    vp = torch.nn.functional.pad(p64, (1, 1, 0, 0), mode="replicate")
    hw = sum(vp[..., t:t + W] * kk[:, :, t] for t in range(3)) + f64
    close("sac_h", nchw(h), torch.where(hw >= 0, hw, hw * R.f32(0.1)))


# ---- (b) the bounds accept an f32 evaluation and reject wrong kernels ----------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES, ids=sid)
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: IDS[d])
def test_f32_evaluation_stays_inside_the_bounds(shape, dt):
    B, H, W = shape
    for Cn in (4, 32):
        p = R.step_inputs(B, H, W, Cn, dt, dt)
        if dt == F32:
            ref, bound = R.warp(p["prev"], p["off"])
            accepts("warp", R.warp(p["prev"], p["off"], cd=F32)[0], ref, bound)
            ref, bound = R.sac_v(p["prev"], p["K"])
            accepts("sac_v", R.sac_v(p["prev"], p["K"], cd=F32)[0], ref, bound)
            ref, bound = R.sac_h(p["prev"], p["K"], p["fin"], 0.1)
            accepts("sac_h", R.sac_h(p["prev"], p["K"], p["fin"], 0.1, cd=F32)[0], ref, bound)
        for slope in R.SLOPES:
            ref, bound = R.iac_step(p["prev"], p["off"], p["K"], p["fin"], slope, dt)
            got = R.iac_step(p["prev"], p["off"], p["K"], p["fin"], slope, dt, cd=F32)[0]
            assert got.dtype == F32 and bool(torch.isfinite(got).all())
            accepts(f"iac_step {IDS[dt]} C={Cn} slope {slope}", got.to(dt), ref, bound)


def _variants(p, slope, dt, shape):
    """(name, wrong f64 output, can it differ at this shape)."""
    B, H, W = shape
    a = (p["prev"], p["off"], p["K"], p["fin"], slope, dt)
    out = [("warp pad=clamp", R.iac_step(*a, pad="clamp")[0], True),
           ("x/y swapped", R.iac_step(*a, swap=True)[0], True),
           ("sac_v zero padding", R.iac_step(*a, pad_v="zeros")[0], True),
           ("sac_h zero padding", R.iac_step(*a, pad_h="zeros")[0], True),
           ("taps reversed", R.iac_step(*a, taps="reversed")[0], True),
           ("halo K 16", R.iac_step(*a, halo=16)[0], W > 16),
           ("halo K 14", R.iac_step(*a, halo=14)[0], W > 14),
           ("stale offsets 16", R.iac_step_tiled(*a[:5], 16, stale=True), B * ((H + 3) // 4) * ((W + 15) // 16) > 1),
           ("stale offsets 14", R.iac_step_tiled(*a[:5], 14, stale=True), B * ((H + 3) // 4) * ((W + 13) // 14) > 1)]
    return out


@pytest.mark.parametrize("shape", R.SHAPES, ids=sid)
@pytest.mark.parametrize("dt", [F32, BF16], ids=lambda d: IDS[d])
def test_bounds_reject_every_wrong_variant(shape, dt):
    """At the GPU tests' own inputs.  A 1 x 1 image cannot tell padding modes or the offset channels apart through random offsets (its
    position classes can), so there the variant only has to differ where the reference says it may."""
    B, H, W = shape
    p = R.step_inputs(B, H, W, 32, dt, dt)
    ref, bound = R.iac_step(p["prev"], p["off"], p["K"], p["fin"], 0.1, dt)
    for name, wrong, can in _variants(p, 0.1, dt, shape):
        n = offending(wrong, ref, bound)
        if can and (H > 1 or W > 1):
            assert n > 0, f"{name} at {shape}: stays inside the bound at every element"
    # the stand-alone passes
    if dt == F32:
        s, bs = R.warp(p["prev"], p["off"])
        assert offending(R.warp(p["prev"], p["off"], pad="clamp")[0], s, bs) > 0 or H * W == 1
        assert offending(R.warp(p["prev"], p["off"], swap=True)[0], s, bs) > 0 or H * W == 1
        v, bv = R.sac_v(p["prev"], p["K"])
        assert offending(R.sac_v(p["prev"], p["K"], pad="zeros")[0], v, bv) > 0
        assert offending(R.sac_v(p["prev"], p["K"], taps="reversed")[0], v, bv) > 0 or H == 1      # one row: the three taps read the same s
        h, bh = R.sac_h(p["prev"], p["K"], p["fin"], 0.1)
        assert offending(R.sac_h(p["prev"], p["K"], p["fin"], 0.1, pad="zeros")[0], h, bh) > 0
        assert offending(R.sac_h(p["prev"], p["K"], p["fin"], 0.1, taps="reversed")[0], h, bh) > 0 or W == 1
    # direction 1 with direction 0's offsets
    q = R.step_inputs(B, H, W, 32, dt, dt, key=1)
    args = ([p["prev"], q["prev"]], [p["off"], q["off"]], p["K"], [p["fin"], q["fin"]], 0.1, dt)
    right, wrong = R.iac_step2(*args), R.iac_step2(*args, same_off=True)
    assert offending(wrong[0][0], *right[0]) == 0
    assert offending(wrong[1][0], *right[1]) > 0 or H * W == 1


def test_clamp_sampling_is_rejected_at_the_planted_positions_alone():
    """pad = "clamp" differs from zero padding at the planted positions -0.5, W-0.5, the largest f32 below W (x only: y is randn) in a
    field whose other offsets are zero."""
    B, H, W = 1, 6, 9
    p = R.step_inputs(B, H, W, 4, F32, F32)
    for pos in (-0.5, W - 0.5, R.below(W)):
        off = torch.zeros(B, H, W, 2)
        off[0, 2, 3, 0] = pos - 3
        ref, bound = R.warp(p["prev"], off)
        wrong = R.warp(p["prev"], off, pad="clamp")[0]
        bad = (wrong - ref).abs() > bound
        assert bool(bad[0, 2, 3].any()) and int(bad.sum()) == int(bad[0, 2, 3].sum()), pos


# ---- (c) the planted classes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES + [(12, 5, 17)], ids=sid)
def test_every_planted_class_is_present(shape):
    B, H, W = shape
    counts = R.class_counts(R.offsets(B, H, W))
    assert len(counts) == 3 * len(R.CLASSES) == 72
    if R.full_coverage(B, H, W):
        empty = [k for k, n in counts.items() if n == 0]
        assert not empty, empty
    else:                                                       # smaller fields hold as many classes as they have room for
        room = min(B * H * W, 72)
        feasible = sum(1 for (c, ax), n in counts.items() if n > 0)
        assert feasible >= min(room, 1), counts
    # the union over the shapes of the GPU tests is complete as well
    total = {}
    for s in R.SHAPES:
        for k, n in R.class_counts(R.offsets(*s)).items():
            total[k] = total.get(k, 0) + n
    assert all(n > 0 for n in total.values())
