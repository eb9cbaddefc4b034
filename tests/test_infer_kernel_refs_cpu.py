"""CPU: the float64 references of tests/infer_kernel_refs.py.
(a) With rounding switched off (dt = None) each one equals an independent f64 statement of the same operation - F.interpolate,
    F.conv2d / F.pixel_shuffle / F.prelu, the lines of oracle.fcvsr_oracle (block_rcb, the tail of forward) - to 1e-12 of the tensor's
    largest entry.
(b) At the inputs and shapes of tests/test_infer_kernels_gpu.py the bounds tell a wrong kernel from a right one: every deliberately
    wrong f64 variant leaves `bound` at one element or more, and the true reference evaluated in f32 (and stored in the test's dtype)
    stays inside it everywhere - which is where the k of every bound is checked without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import infer_kernel_refs as R
from infer_kernel_refs import BF16, F16, F32, D

TOL = 1e-12
DT16 = [BF16, F16]


def close(name, got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert err <= TOL * max(float(ref.abs().max()), 1e-300), f"{name}: {err:.3e}"


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def rejects(name, wrong, ref, bound):
    bad = (wrong.double() - ref).abs() > bound
    assert bool(bad.any()), f"{name}: the wrong variant stays inside the bound at every element"


def accepts(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{name}: a correct f32 evaluation leaves the bound, worst err / bound {worst:.3f}"
    return worst


# ---- (a) the references against torch / the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.BILINEAR_SHAPES + [(1, 2, 3, 1)])
def test_bilinear_up4_reference_is_interpolate(shape):
    x = torch.randn(*shape, generator=R.gen(100, *shape), dtype=D)
    ref, bound = R.bilinear_up4(x)
    close("up4", ref, F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False))
    assert bool((bound >= 0).all())


@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 3, 5)])
@pytest.mark.parametrize("slope", [0.25, 0.0, 1.5])
def test_tail_reference_is_conv_shuffle_prelu_conv(B, H, W, slope):
    """The tail of oracle.forward from upconv2 on: conv 1x1 -> pixel_shuffle -> PReLU -> conv 3x3 + base, natural channel order; the
    reference is handed the same weights in the kernel's packing (rows (2i+j)*64 + c, the [16][64] tap table)."""
    from oracle import fcvsr_oracle as O
    g = R.gen(101, B, H, W)
    u1 = torch.randn(B, 64, 2 * H, 2 * W, generator=g, dtype=D)
    w2, b2 = torch.randn(256, 64, 1, 1, generator=g, dtype=D) / 8, torch.randn(256, generator=g, dtype=D)
    wl, bl = torch.randn(1, 64, 3, 3, generator=g, dtype=D) / 24, torch.randn(1, generator=g, dtype=D)
    base = torch.randn(B, 1, 4 * H, 4 * W, generator=g, dtype=D)
    a = torch.tensor([slope], dtype=D)
    for name, want in (("torch", F.conv2d(F.prelu(F.pixel_shuffle(F.conv2d(u1, w2, b2), 2), a), wl, bl, padding=1) + base),
                       ("oracle", F.conv2d(O._prelu(O.pixel_shuffle2(F.conv2d(u1, w2, b2)), a), wl, bl, padding=1) + base)):
        order = torch.tensor([4 * c + sp for sp in range(4) for c in range(64)])
        tab = torch.zeros(16, 64, dtype=D)
        tab[:9] = wl[0].permute(1, 2, 0).reshape(9, 64)
        ref, _ = R.tail_fused(nhwc(u1), w2[order, :, 0, 0], b2[order], slope, tab, bl, base[:, 0], None)
        close(f"tail vs {name}", ref, want[:, 0])


def test_gc_apply_and_xscale_references_are_the_oracle_lines():
    """block_rcb's second half: R = lrelu(r + add, 0.2) + z (oracle.rcb / context_block's broadcast add) and its three output lines
    with the identity for up.0 / down.0 (F.interpolate x0.5 bilinear of an even-sized tensor is the 2x2 mean)."""
    from oracle import fcvsr_oracle as O
    g = R.gen(102)
    B, Cn, H, W = 2, 8, 8, 12
    s = R.f32(0.2)
    Rs, xs = [], []
    for l in range(3):
        h, w = H >> l, W >> l
        r, z, x = (torch.randn(B, Cn, h, w, generator=g, dtype=D) for _ in range(3))
        add = torch.randn(B, Cn, generator=g, dtype=D)
        want = O._lrelu(r + add[:, :, None, None], s) + z
        ref, _ = R.gc_apply(nhwc(r), add, nhwc(z), 0.2, None)
        close(f"gc_apply level {l}", ref, nhwc(want))
        if h % 2 == 0 and w % 2 == 0:
            pooled, _ = R.gc_apply(nhwc(r), add, nhwc(z), 0.2, None, pool=True)
            close(f"gc_apply pool level {l}", pooled, nhwc(F.avg_pool2d(want, 2)))
            close(f"gc_apply pool level {l} vs interpolate", pooled,
                  nhwc(F.interpolate(want, scale_factor=0.5, mode="bilinear", align_corners=False)))
        Rs.append(want)
        xs.append(x)
    dn = lambda t: F.interpolate(t, scale_factor=0.5, mode="bilinear", align_corners=False)
    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False)
    want = [xs[0] + Rs[0] + Rs[0] + up(Rs[1]), xs[1] + Rs[1] + dn(Rs[0]) + up(Rs[2]), xs[2] + Rs[2] + dn(Rs[1]) + Rs[2]]
    got0, _ = R.xscale(nhwc(xs[0]), nhwc(Rs[0]), 2.0, None, 0, nhwc(Rs[1]), None)
    got1p, _ = R.xscale(nhwc(xs[1]), nhwc(Rs[1]), 1.0, nhwc(dn(Rs[0])), 1, nhwc(Rs[2]), None)
    got1f, _ = R.xscale(nhwc(xs[1]), nhwc(Rs[1]), 1.0, nhwc(Rs[0]), 0, nhwc(Rs[2]), None)
    got2, _ = R.xscale(nhwc(xs[2]), nhwc(Rs[2]), 2.0, nhwc(Rs[1]), 0, None, None)
    for name, got, w in (("out0", got0, want[0]), ("out1 pooled dn", got1p, want[1]), ("out1 full dn", got1f, want[1]), ("out2", got2, want[2])):
        close(name, got, nhwc(w))


def test_gc_apply_and_xscale_references_against_block_rcb_itself():
    """oracle.block_rcb called as it stands.  Its 3x3 layers get delta kernels and its inputs are positive, so both bodies pass z through
    (their LeakyReLUs see positive values) and r = z; the ContextBlock keeps random weights, large enough that r + add goes negative;
    up.0 / down.0 are identities.  Then R = lrelu(z + add, 0.2) + z is gc_apply's line and the three returned tensors are xscale's,
    with the oracle's own `add` (context_block(r) - r) handed to the reference."""
    from oracle import fcvsr_oracle as O
    g = R.gen(106)
    B, Cn, H, W = 2, 8, 8, 12
    delta = torch.zeros(Cn, Cn, 3, 3, dtype=D)
    delta[torch.arange(Cn), torch.arange(Cn), 1, 1] = 1.0
    eye = torch.eye(Cn, dtype=D)[:, :, None, None]
    p = {f"k.{n}.weight": delta for n in ("body.0", "body.2", "RCB.body.0", "RCB.body.2")}
    p.update({"k.up.0.weight": eye, "k.down.0.weight": eye,
              "k.RCB.gcnet.conv_mask.weight": torch.randn(1, Cn, 1, 1, generator=g, dtype=D),
              "k.RCB.gcnet.channel_add_conv.0.weight": torch.randn(Cn, Cn, 1, 1, generator=g, dtype=D),
              "k.RCB.gcnet.channel_add_conv.2.weight": torch.randn(Cn, Cn, 1, 1, generator=g, dtype=D)})
    xs = [torch.rand(B, Cn, H >> l, W >> l, generator=g, dtype=D) + 0.05 for l in range(3)]
    want = O.block_rcb(p, "k", xs)
    adds = [(O.context_block(p, "k.RCB.gcnet", z) - z)[:, :, 0, 0] for z in xs]
    assert any(bool(((z + a[:, :, None, None]) < 0).any()) for z, a in zip(xs, adds))          # the slope side is really taken
    Rs = [R.gc_apply(nhwc(z), a, nhwc(z), 0.2, None, slope32=False)[0] for z, a in zip(xs, adds)]     # the oracle's f64 0.2
    got = [R.xscale(nhwc(xs[0]), Rs[0], 2.0, None, 0, Rs[1], None)[0],
           R.xscale(nhwc(xs[1]), Rs[1], 1.0, Rs[0], 0, Rs[2], None)[0],
           R.xscale(nhwc(xs[2]), Rs[2], 2.0, Rs[1], 0, None, None)[0]]
    for l in range(3):
        close(f"block_rcb out{l}", got[l], nhwc(want[l]))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (5, 1), (3, 4)])
def test_xscale_up2_is_interpolate(h, w):
    x = torch.randn(2, 4, h, w, generator=R.gen(103, h, w), dtype=D)
    close("up2", R.resample(x, 2, 2, 3), F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 5)])
def test_feat_extract_reference_is_conv2d(B, H, W):
    """On inputs and weights that are exact in f16 (so the reference's f16 rounding is the identity)."""
    g = R.gen(104, B, H, W)
    x = torch.randint(0, 256, (B, 7, H, W), generator=g).to(D) / 256
    w = torch.randn(128, 7, 3, 3, generator=g).to(F16).to(D)
    b = torch.randn(128, generator=g, dtype=D)
    for bias in (b, None):
        ref, _ = R.feat_extract(x, R.feat_matrix(w.float()), bias, None)
        close("feat_extract", ref, nhwc(F.conv2d(x, w, bias, padding=1)))


def test_scale_add_and_quantise():
    g = R.gen(105)
    z, x, gate = torch.randn(2, 3, 4, 8, generator=g, dtype=D), torch.randn(2, 3, 4, 8, generator=g, dtype=D), torch.rand(2, 8, generator=g, dtype=D)
    ref, _ = R.scale_add(z, gate, x, None)
    close("scale_add", ref, nhwc(nchw(z) * gate[:, :, None, None] + nchw(x)))        # oracle._ca's broadcast product, plus x
    v = torch.tensor([-0.5, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.999, 1.0, 7.0])
    assert R.quantise(v, 255, "truncate").tolist() == [0, 0, 0, 1, 2, 254, 255, 255]
    assert R.quantise(v, 255, "round").tolist() == [0, 0, 0, 2, 2, 255, 255, 255]              # halves go to the even neighbour
    assert R.quantise(torch.tensor([0.5, 1.5 / 1023]), 1023, "round").tolist() == [512, 2]


# ---- (b) the bounds at the GPU tests' inputs --------------------------------------------------------------------------------------------

def test_bounds_bilinear_up4():
    hit = {"early": 0, "none": 0}
    for shape in R.BILINEAR_SHAPES:
        x = R.bilinear_window(*shape)[:, 3]
        ref, bound = R.bilinear_up4(x)
        accepts(f"up4 {shape}", R.bilinear_up4(x, F32)[0], ref, bound)
        for upper in hit:
            hit[upper] += int(((R.bilinear_up4(x, D, upper)[0] - ref).abs() > bound).any())
    assert hit["none"] == len(R.BILINEAR_SHAPES), hit       # an unclamped neighbour shows at every shape (the last row / column)
    assert hit["early"] >= 3, hit                           # clamped one early: wherever an axis has two source pixels or more


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B,H,W", R.TAIL_SMALL)
def test_bounds_tail_fused(B, H, W, dt):
    for slope in R.TAIL_SLOPES:
        p = R.tail_inputs(B, H, W, dt, slope)
        ref, bound = R.tail_ref(p, dt)
        tag = f"tail {B}x{H}x{W} {dt} slope {slope}"
        accepts(tag, R.tail_ref(p, dt, F32)[0], ref, bound)
        u2, _ = R.tail_u2(p["u1"], p["w2"], p["b2"], slope)

        def last(u, **kw):
            return R.tail_last(R.rnd(u, dt), p["wl"], p["bl"], p["base"], **kw)

        blocks = p["w2"].view(4, 64, 64), p["b2"].view(4, 64)
        swapped = [t[[0, 2, 1, 3]].reshape(-1, *t.shape[2:]) for t in blocks]                # rows (2j+i)*64 + c
        natural = [t.transpose(0, 1).reshape(-1, *t.shape[2:]) for t in blocks]              # the kernel handed rows 4c + 2i + j
        rejects(tag + " (i, j) swapped", last(R.tail_u2(p["u1"], swapped[0], swapped[1], slope)[0]), ref, bound)
        rejects(tag + " natural row order", last(R.tail_u2(p["u1"], natural[0], natural[1], slope)[0]), ref, bound)
        rejects(tag + " clamp padding", last(u2, pad="replicate"), ref, bound)
        rejects(tag + " no rounding of u2" if dt == BF16 else tag + " u2 rounded to bf16",
                R.tail_last(u2 if dt == BF16 else R.rnd(u2, BF16), p["wl"], p["bl"], p["base"]), ref, bound)
        if slope != 1.0:
            rejects(tag + " slope on the wrong side", last(R.tail_u2(p["u1"], p["w2"], p["b2"], slope, side="pos")[0]), ref, bound)
        shifted = torch.roll(ref, 1, dims=2)                                                  # a tile written one pixel to the right
        rejects(tag + " shifted", shifted, ref, bound)


@pytest.mark.parametrize("dt", DT16)
def test_bounds_tail_fused_tile_runs_shape(dt):
    """36 x 68 at B = 5, the batch the GPU test derives on a 256-CU part."""
    H, W = R.TAIL_BIG_HW
    p = R.tail_inputs(5, H, W, dt, 0.25)
    ref, bound = R.tail_ref(p, dt)
    tag = f"tail 5x{H}x{W} {dt}"
    accepts(tag, R.tail_ref(p, dt, F32)[0], ref, bound)
    u2r = R.rnd(R.tail_u2(p["u1"], p["w2"], p["b2"], 0.25)[0], dt)
    rejects(tag + " clamp padding", R.tail_last(u2r, p["wl"], p["bl"], p["base"], pad="replicate"), ref, bound)
    wrong = ref.clone()
    wrong[1, :8, :32] = ref[0, :8, :32]                     # the first tile of image 1 computed from image 0: a run that did not
    rejects(tag + " tile of the previous image", wrong, ref, bound)                           # step to the next image


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_bounds_gc_apply(dt):
    for rdt in {F32, dt}:
        for (H, W, pooled) in R.GC_LEVELS:
            for Cn in (64, 36):
                p = R.gc_inputs(2, H, W, Cn, dt, rdt)
                tag = f"gc_apply {H}x{W} C{Cn} {dt} r {rdt}"
                ref, bound = R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt)
                accepts(tag, R.rnd(R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt, cd=F32)[0], dt), ref, bound)
                rejects(tag + " slope 0.1", R.gc_apply(p["r"], p["add"], p["z"], 0.1, dt)[0], ref, bound)
                rejects(tag + " add of the other image", R.gc_apply(p["r"], p["add"].flip(0), p["z"], 0.2, dt)[0], ref, bound)
                if not pooled:
                    continue
                pref, pbound = R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt, pool=True)
                accepts(tag + " pool", R.rnd(R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt, pool=True, cd=F32)[0], dt), pref, pbound)
                if dt != F32:
                    rejects(tag + " pool of the unrounded R", R.gc_apply(p["r"], p["add"], p["z"], 0.2, None, pool=True)[0], pref, pbound)
                rejects(tag + " pool of three", pref - 0.25 * ref[:, 1::2, 1::2], pref, pbound)


@pytest.mark.parametrize("Cn", [64, 36])
@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_bounds_xscale(dt, Cn):
    cases = R.XS_LEVELS + [((2, 2), None, True, 2.0), ((12, 10), "full", True, 1.0)]
    for (H, W), dn, up, rs in cases:
        p = R.xscale_inputs(2, H, W, Cn, dt, dn, up)
        tag = f"xscale {H}x{W} C{Cn} {dt} dn {dn} up {up}"
        args = (p["x"], p["r"], rs, p["dn"], p["dn_pooled"], p["up"], dt)
        ref, bound = R.xscale(*args)
        accepts(tag, R.rnd(R.xscale(*args, cd=F32)[0], dt), ref, bound)
        rejects(tag + " r_scale", R.xscale(p["x"], p["r"], 3.0 - rs, *args[3:])[0], ref, bound)
        if up:
            rejects(tag + " upper neighbour not clamped", R.xscale(*args, upper="none")[0], ref, bound)
            if H >= 4 or W >= 4:
                rejects(tag + " upper neighbour clamped early", R.xscale(*args, upper="early")[0], ref, bound)
        if dn == "full":                                    # dn_pooled ignored: the (2H, 2W) tensor read as if it were (H, W)
            flat = p["dn"].reshape(2, -1)[:, :H * W * Cn].reshape(2, H, W, Cn)
            rejects(tag + " dn_pooled ignored", R.xscale(p["x"], p["r"], rs, flat, 1, p["up"], dt)[0], ref, bound)
        if dn == "pooled":                                  # ... and the other way round: the pooled tensor averaged again
            again = p["dn"].repeat_interleave(2, 1).repeat_interleave(2, 2).roll(1, 2)
            rejects(tag + " dn_pooled ignored", R.xscale(p["x"], p["r"], rs, again, 0, p["up"], dt)[0], ref, bound)


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B,H,W", R.FEAT_SHAPES)
def test_bounds_feat_extract(B, H, W, dt):
    for with_bias in (True, False):
        p = R.feat_inputs(B, H, W, with_bias)
        tag = f"feat_extract {B}x{H}x{W} {dt} bias {with_bias}"
        ref, bound = R.feat_extract(p["x"], p["wmat"], p["bias"], dt)
        accepts(tag, R.rnd(R.feat_extract(p["x"], p["wmat"], p["bias"], dt, cd=F32)[0], dt), ref, bound)
        wrong = torch.zeros(448, 64)
        wrong[:, :63] = p["w"].reshape(448, 63)                                              # column c*9 + tap
        rejects(tag + " im2col order c*9 + tap", R.feat_extract(p["x"], wrong.to(F16), p["bias"], dt)[0], ref, bound)
        rejects(tag + " flat pixel index at the border", R.feat_extract(p["x"], p["wmat"], p["bias"], dt, wrap=True)[0], ref, bound)
        rejects(tag + " x not rounded to f16", (R.im2col(p["x"].double()) @ p["wmat"].double()[:, :63].t()
                                                + (0 if p["bias"] is None else p["bias"].double())), ref, bound)


@pytest.mark.parametrize("Cn", [64, 36])
def test_bounds_scale_add(Cn):
    for xdt, odt in ((F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)):
        p = R.scale_add_inputs(2, 5, 7, Cn, xdt)
        tag = f"scale_add C{Cn} {xdt} -> {odt}"
        ref, bound = R.scale_add(p["z"], p["gate"], p["x"], odt)
        # the kernel's one fma, emulated from the f32 inputs: the product of two f32 is exact in f64, the f64 sum is rounded to f32
        # once.  torch's f32 z * g + x rounds twice and is not what the kernel computes; so this check shows no more than that
        # EPS * S covers half an f32 unit in the last place of the result
        fma32 = (p["z"].double() * p["gate"].double()[:, None, None, :] + p["x"].double()).float()
        accepts(tag + " (emulated fma)", R.rnd(fma32, odt), ref, bound)
        rejects(tag + " gate of the other image", R.scale_add(p["z"], p["gate"].flip(0), p["x"], odt)[0], ref, bound)
        rejects(tag + " gate of the next channel", R.scale_add(p["z"], p["gate"].roll(1, 1), p["x"], odt)[0], ref, bound)
