"""GPU: the IAC forward kernels through the C ABI against the per-element float64 references of tests/iac_refs.py: fcvsr_warp /
fcvsr_sac_v / fcvsr_sac_h (warp_kernel, sac_kernel: the training and fall-back forward), fcvsr_iac_step (iac_step_kernel at C = 32 and
through views the 64-channel kernel cannot take, iac_step64_kernel<.., 1, false> at C = 64), fcvsr_iac_step2 (iac_step64_kernel<.., 2,
false>) and fcvsr_iac_step2_fused (iac_fused2_kernel, iac_step64_kernel<.., 2, true>).  Every f64 comparison asserts |got - ref| <=
bound for EVERY element (bounds: iac_refs' docstring; tests/test_iac_refs_cpu.py shows that they reject wrong kernels at these very
inputs); the fused-predictor launches are compared bit for bit with the stand-alone 1x1 convolution + fcvsr_iac_step2, which is itself
held to the reference with the K that convolution stored.  The offset fields carry the planted classes of iac_refs.offsets (integer
offsets, positions on -1, 0, W-1, W, the largest f32 below W, offsets that round away, +-1e4 ... +-inf, NaN).  Outputs are pre-filled
with NaN.  Each docstring records the worst |got - ref| / bound measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import iac_refs as R
from iac_refs import BF16, F16, F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL_PAIRS = [(a, k) for a in (F32, BF16, F16) for k in (F32, BF16, F16)]            # (activations, K)
pid = lambda p: IDS[p] if p in IDS else str(p)


def within(tag, got, ref, bound):
    """|got - ref| <= bound at every element; the message carries the worst ratio."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    assert not bool(torch.isnan(got).any()), f"{tag}: the output holds a NaN (an element the kernel never wrote, or a non-finite offset that got through)"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    print(f"[{tag}] worst |got - ref| / bound {worst:.3f}")
    bad = err > bound
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements leave the bound, worst |got - ref| / bound {worst:.3f} "
                                 f"at {tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape))}")
    return worst


def nans(shape, dt):
    return torch.full(tuple(shape), NAN, device="cuda", dtype=dt)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def step(prev, off, K, fin, slope, dst):
    from fcvsr_amd import hip
    B, H, W, _ = prev.shape
    pv, ov, kv, fv, dv = (hip.view(t) for t in (prev, off, K, fin, dst))
    hip.check(hip.lib().fcvsr_iac_step(C.byref(pv), C.byref(ov), C.byref(kv), C.byref(fv), slope, B, H, W, C.byref(dv), hip.stream_ptr()),
              "fcvsr_iac_step")
    torch.cuda.synchronize()


def step2(prevs, offs, K, fins, slope, dsts):
    from fcvsr_amd import hip
    B, H, W, _ = prevs[0].shape
    V2 = hip.View * 2
    kv = hip.view(K)
    hip.check(hip.lib().fcvsr_iac_step2(V2(*map(hip.view, prevs)), V2(*map(hip.view, offs)), C.byref(kv), V2(*map(hip.view, fins)), slope,
                                        B, H, W, V2(*map(hip.view, dsts)), hip.stream_ptr()), "fcvsr_iac_step2")
    torch.cuda.synchronize()


def dev(p):
    return {k: v.cuda() for k, v in p.items()}


# ---- the three-launch path ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [4, 64])
def test_warp_sac_v_sac_h_vs_f64_reference(Cn):
    """fcvsr_warp, fcvsr_sac_v, fcvsr_sac_h each on its own inputs, and chained as train/blocks.py chains them (held to iac_step's
    reference), f32, at every shape.  measured <= 0.49 (warp), 0.77 (sac_v), 0.64 (sac_h), 0.24 (chain)"""
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    for B, H, W in R.SHAPES:
        p = R.step_inputs(B, H, W, Cn, F32, F32)
        d = dev(p)
        pv, ov, kv, fv = (hip.view(d[k]) for k in ("prev", "off", "K", "fin"))
        tag = f"C={Cn} {B}x{H}x{W}"
        s = nans(d["prev"].shape, F32)
        sv = hip.view(s)
        hip.check(L.fcvsr_warp(C.byref(pv), C.byref(ov), B, H, W, C.byref(sv), st), "fcvsr_warp")
        within(f"warp {tag}", s, *R.warp(p["prev"], p["off"]))
        v = nans(s.shape, F32)
        vv = hip.view(v)
        hip.check(L.fcvsr_sac_v(C.byref(pv), C.byref(kv), B, H, W, C.byref(vv), st), "fcvsr_sac_v")
        within(f"sac_v {tag}", v, *R.sac_v(p["prev"], p["K"]))
        for slope in R.SLOPES:
            out = nans(s.shape, F32)
            outv = hip.view(out)
            hip.check(L.fcvsr_sac_h(C.byref(pv), C.byref(kv), C.byref(fv), slope, B, H, W, C.byref(outv), st), "fcvsr_sac_h")
            within(f"sac_h {tag} slope {slope}", out, *R.sac_h(p["prev"], p["K"], p["fin"], slope))
            v2, out2 = nans(s.shape, F32), nans(s.shape, F32)
            v2v, out2v = hip.view(v2), hip.view(out2)
            hip.check(L.fcvsr_sac_v(C.byref(sv), C.byref(kv), B, H, W, C.byref(v2v), st), "fcvsr_sac_v")
            hip.check(L.fcvsr_sac_h(C.byref(v2v), C.byref(kv), C.byref(fv), slope, B, H, W, C.byref(out2v), st), "fcvsr_sac_h")
            within(f"chain {tag} slope {slope}", out2, *R.iac_step(p["prev"], p["off"], p["K"], p["fin"], slope, F32))


# ---- fcvsr_iac_step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [32, 64])
@pytest.mark.parametrize("adt,kdt", ALL_PAIRS, ids=pid)
def test_iac_step_vs_f64_reference(adt, kdt, Cn):
    """Every shape, slopes 0.1 and 1.5; C = 32: iac_step_kernel<kdt, adt>, C = 64: iac_step64_kernel<kdt, adt, 1, false> (all nine
    storage pairs of each).  measured <= 0.25 (f32 output), 1.00 (16-bit output, 0.998: the store term - a rounding error of just under
    half a unit in the last place - is nearly all of the bound there)"""
    for B, H, W in R.SHAPES:
        p = R.step_inputs(B, H, W, Cn, adt, kdt)
        if R.full_coverage(B, H, W):
            assert all(n > 0 for n in R.class_counts(p["off"]).values())
        d = dev(p)
        for slope in R.SLOPES:
            out = nans(d["prev"].shape, adt)
            step(d["prev"], d["off"], d["K"], d["fin"], slope, out)
            within(f"iac_step {IDS[adt]}/{IDS[kdt]} C={Cn} {B}x{H}x{W} slope {slope}", out,
                   *R.iac_step(p["prev"], p["off"], p["K"], p["fin"], slope, adt))


@pytest.mark.parametrize("layout", ["slice 4..68 of 72", "slice 0..64 of 68"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=pid)
def test_iac_step_c64_through_views_vs_f64_reference(dt, layout):
    """C = 64 with prev, feat_in and dst channel slices of wider buffers.  bf16: channels [4, 68) of 72 start 8 bytes into a pixel (not
    16-byte aligned), channels [0, 64) of 68 have a pixel stride that is no multiple of 8 elements - either way the 64-channel kernel's
    16-byte accesses are out and iac_step_kernel runs with grid.y = 2.  f32: both layouts still satisfy the 64-channel kernel (16-byte
    aligned, strides multiples of 4 floats - for f32 its conditions are those of the entry point itself), which then runs on strided
    views.  The channels outside the slice keep their pre-fill.  measured <= 0.23 (f32), 1.00 (bf16, 0.996)"""
    total, lo = (72, 4) if layout.startswith("slice 4") else (68, 0)
    for B, H, W in R.PARTIAL + [(1, 4, 16)]:
        p = R.step_inputs(B, H, W, 64, dt, dt, key=2)
        d = dev(p)
        bufs = {}
        for k in ("prev", "fin"):
            bufs[k] = torch.full((B, H, W, total), 7.0, device="cuda", dtype=dt)
            bufs[k][..., lo:lo + 64] = d[k]
        keep = {k: t.clone() for k, t in bufs.items()}
        out = nans((B, H, W, total), dt)
        step(bufs["prev"][..., lo:lo + 64], d["off"], d["K"], bufs["fin"][..., lo:lo + 64], 0.1, out[..., lo:lo + 64])
        tag = f"iac_step {IDS[dt]} {layout} {B}x{H}x{W}"
        within(tag, out[..., lo:lo + 64], *R.iac_step(p["prev"], p["off"], p["K"], p["fin"], 0.1, dt))
        outside = torch.cat([out[..., :lo], out[..., lo + 64:]], -1)
        assert bool(torch.isnan(outside).all()), f"{tag}: a channel outside the slice was written"
        assert all(torch.equal(bits(bufs[k]), bits(keep[k])) for k in bufs), f"{tag}: an input was written"


# ---- fcvsr_iac_step2 ----------------------------------------------------------------------------------------------------------------

def _step2_inputs(B, H, W, adt, kdt, key=0):
    p = [R.step_inputs(B, H, W, 64, adt, kdt, key + 10 * d) for d in range(2)]
    return dict(prevs=[q["prev"] for q in p], offs=[q["off"] for q in p], fins=[q["fin"] for q in p], K=p[0]["K"])


def _step2_check(tag, B, H, W, adt, kdt, slope, key=0):
    """Direction 1's dst is the channel slice [64, 128) of a 128-channel buffer whose other half keeps its pre-fill."""
    p = _step2_inputs(B, H, W, adt, kdt, key)
    prevs, offs, fins = ([t.cuda() for t in p[k]] for k in ("prevs", "offs", "fins"))
    K = p["K"].cuda()
    wide = nans((B, H, W, 128), adt)
    dsts = [nans((B, H, W, 64), adt), wide[..., 64:]]
    step2(prevs, offs, K, fins, slope, dsts)
    refs = R.iac_step2(p["prevs"], p["offs"], p["K"], p["fins"], slope, adt)
    worst = max(within(f"{tag} dir {d}", dsts[d], *refs[d]) for d in range(2))
    assert bool(torch.isnan(wide[..., :64]).all()), f"{tag}: channels outside direction 1's slice were written"
    return worst


@pytest.mark.parametrize("adt,kdt", ALL_PAIRS, ids=pid)
def test_iac_step2_vs_f64_reference(adt, kdt):
    """Both directions with their own offsets and features, one K: iac_step64_kernel<kdt, adt, 2, false>, all nine storage pairs, the
    partial-tile shapes, slope 0.1 and (at 2 x 5 x 17) 1.5.  measured <= 0.26 (f32 output), 1.00 (16-bit output, 0.998)"""
    for B, H, W in R.PARTIAL:
        _step2_check(f"iac_step2 {IDS[adt]}/{IDS[kdt]} {B}x{H}x{W}", B, H, W, adt, kdt, 0.1)
    _step2_check(f"iac_step2 {IDS[adt]}/{IDS[kdt]} 2x5x17 slope 1.5", 2, 5, 17, adt, kdt, 1.5, key=3)


# ---- the fused kernel predictor -------------------------------------------------------------------------------------------------------

def _fused_vs_unfused(tag, B, H, W, adt, kdt, slope, strided=False, f64=True, key=0):
    """fcvsr_iac_step2_fused == the stand-alone 1x1 conv2d_mfma (16-bit K, the middle one of three iterations: non-zero weight-row and
    bias offsets) + fcvsr_iac_step2, bit for bit.  strided: direction 1's prev and dst are channel slices of 128-channel buffers, so
    the two directions' strides differ.  f64: the unfused result is also held to the reference with the K the convolution stored."""
    from fcvsr_amd import hip
    p = _step2_inputs(B, H, W, adt, kdt, key)
    prevs, offs, fins = ([t.cuda() for t in p[k]] for k in ("prevs", "offs", "fins"))
    g = R.gen(9, B, H, W, key)
    k0 = torch.randn(B, H, W, 64, generator=g).to(kdt).cuda()
    w = (torch.randn(3 * 192, 64, 1, 1, generator=g) / 8.0).cuda()
    bias = (torch.randn(3 * 192, generator=g) * 0.1).cuda()
    wp = hip.pack_conv_weight_mfma(w, kdt)
    Kall = torch.empty(B, H, W, 3 * 192, device="cuda", dtype=kdt)
    hip.conv2d_mfma([dict(srcs=[k0], dst=Kall)], wp, 1, 3 * 192, hip.BF16 if kdt == BF16 else hip.F16, bias=bias)
    it = 1
    K = Kall[..., it * 192:(it + 1) * 192]

    def outputs():
        if not strided:
            return [nans((B, H, W, 64), adt), nans((B, H, W, 64), adt)], None
        wide = nans((B, H, W, 128), adt)
        return [nans((B, H, W, 64), adt), wide[..., :64]], wide

    if strided:
        pw = torch.full((B, H, W, 128), 3.0, device="cuda", dtype=adt)
        pw[..., :64] = prevs[1]
        prevs[1] = pw[..., :64]
    ref, _ = outputs()
    step2(prevs, offs, K, fins, slope, ref)
    out, wide = outputs()
    V2 = hip.View * 2
    k0v = hip.view(k0)
    hip.check(hip.lib().fcvsr_iac_step2_fused(V2(*map(hip.view, prevs)), V2(*map(hip.view, offs)), C.byref(k0v), wp.data_ptr() + it * 192 * 64 * 2,
                                              bias.data_ptr() + it * 192 * 4, V2(*map(hip.view, fins)), slope, B, H, W,
                                              V2(*map(hip.view, out)), hip.stream_ptr()), "fcvsr_iac_step2_fused")
    torch.cuda.synchronize()
    for d in range(2):
        assert not bool(torch.isnan(out[d]).any()), f"{tag} dir {d}: the fused output holds a NaN"
        differ = bits(out[d]) != bits(ref[d])
        assert not bool(differ.any()), f"{tag} dir {d}: {int(differ.sum())} of {differ.numel()} elements differ from the unfused chain"
    if wide is not None:
        assert bool(torch.isnan(wide[..., 64:]).all()), f"{tag}: channels outside direction 1's slice were written"
    worst = 0.0
    if f64:
        refs = R.iac_step2(p["prevs"], p["offs"], K.cpu(), p["fins"], slope, adt)
        worst = max(within(f"{tag} unfused dir {d}", ref[d], *refs[d]) for d in range(2))
    return worst


def run_shape():
    """(B, 5, 17, workgroups of iac_step64_kernel FK, of iac_fused2_kernel): 2 x 2 tiles per image in either tiling (4 x 16 and 4 x 14,
    partial in x and in y) and enough images that every workgroup of both persistent kernels walks a run of five tiles or more.  The
    workgroup counts mirror the host code: two resp. three per CU, rounded down to a multiple of 8."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nwg64 = max(8, 2 * cus // 8 * 8)
    nwg2 = max(8, 2 * cus // 2 * 3 // 8 * 8)
    B = 5 * nwg2 // 4 + 1
    while (4 * B) % nwg2 == 0 or (4 * B) % nwg64 == 0:
        B += 1
    return B, 5, 17, nwg64, nwg2


def _assert_runs(B, H, W, nwg64, nwg2):
    for tw, nwg in ((16, nwg64), (14, nwg2)):
        per_image = ((H + 3) // 4) * ((W + tw - 1) // tw)
        ntiles = B * per_image
        assert ntiles > nwg, (ntiles, nwg)                                  # workgroups walk runs of tiles ...
        assert ntiles % nwg != 0                                            # ... of uneven length ...
        assert per_image < ntiles // nwg                                    # ... each longer than an image: every run crosses a boundary
        assert W % tw != 0 and W > tw                                       # with a partial tile in x
    assert B * H * W * 64 < 2 ** 24                                         # keeps the f64 reference and the transfers small


def test_iac_step2_at_the_tile_run_shape_vs_f64_reference():
    """The shape of the tile-run tests below (B x 5 x 17, B from the CU count: 961 on an MI355X), bf16: what the fused launches are
    compared with is itself inside the bound at every element there.  measured <= 1.00 (0.996)"""
    B, H, W, nwg64, nwg2 = run_shape()
    _assert_runs(B, H, W, nwg64, nwg2)
    _step2_check(f"iac_step2 bf16 {B}x{H}x{W}", B, H, W, BF16, BF16, 0.1, key=5)


@pytest.mark.parametrize("adt,kdt", [(BF16, BF16), (F16, F16), (F32, BF16)], ids=pid)
def test_iac_step2_fused_tile_runs_equal_unfused(adt, kdt):
    """More tiles than launched workgroups: every workgroup walks five tiles or more (the loop body runs again, off_next is reloaded),
    across image boundaries, through partial tiles, with the planted offset classes spread over the runs - a stale or shifted off_next
    would warp a tile with its predecessor's offsets.  16-bit activations: iac_fused2_kernel; f32 activations with a bf16 predictor:
    iac_step64_kernel<bf16, f32, 2, true>.  Bit for bit equal to the unfused chain, which the test above holds to the reference."""
    B, H, W, nwg64, nwg2 = run_shape()
    _assert_runs(B, H, W, nwg64, nwg2)
    counts = R.class_counts(R.offsets(B, H, W, 5))
    assert all(n > 0 for n in counts.values())
    _fused_vs_unfused(f"fused tile runs {IDS[adt]}/{IDS[kdt]} {B}x{H}x{W}", B, H, W, adt, kdt, 0.1, f64=False, key=5)


@pytest.mark.parametrize("shape", [(2, 18, 37), (3, 5, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("adt,kdt,slope,strided", [(BF16, BF16, 1.5, False), (F16, F16, 1.5, False), (BF16, BF16, 0.1, True), (F16, F16, 0.1, True),
                                                   (F32, F16, 0.1, False), (F32, BF16, 1.5, True), (BF16, F16, 0.1, False),
                                                   (F16, BF16, 0.1, False), (BF16, BF16, 0.1, False), (F16, F16, 0.1, False)], ids=pid)
def test_iac_step2_fused_routes_equal_unfused(adt, kdt, slope, strided, shape):
    """The routes of fcvsr_iac_step2_fused that leave iac_fused2_kernel for iac_step64_kernel<kdt, adt, 2, true>: a slope outside [0, 1]
    (the register kernel's max form of the LeakyReLU does not cover it), the two directions strided differently, f32 activations (f16
    and bf16 predictor), 16-bit activations whose dtype is not the predictor's - all six instantiations - and, last two rows, the
    register kernel itself at these shapes.  Every route is bit-equal to the unfused chain by design (the predicted K is rounded to the
    predictor's dtype exactly as the stand-alone convolution stores it); the chain is held to the f64 reference with that stored K.
    measured <= 0.25 (f32 output), 1.00 (16-bit output, 0.995)"""
    B, H, W = shape
    _fused_vs_unfused(f"fused {IDS[adt]}/{IDS[kdt]} slope {slope} strided {strided} {B}x{H}x{W}", B, H, W, adt, kdt, slope, strided, key=7)
