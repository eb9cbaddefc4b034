"""GPU: the kernels at the bottom of the 16-bit inference path's bit-equality chains, through the C ABI, against the per-element float64
references of tests/infer_kernel_refs.py: fcvsr_bilinear_up4 (+ _u8, _u16), fcvsr_tail_fused (+ _u8, _u16), fcvsr_gc_apply_levels /
fcvsr_gc_apply, fcvsr_xscale_levels / fcvsr_xscale, fcvsr_feat_extract (+ _u8, _u16), fcvsr_scale_add and fcvsr_pixel_shuffle.  Every
f64 comparison asserts |got - ref| <= bound for EVERY element (bounds: infer_kernel_refs' docstrings; tests/test_infer_kernel_refs_cpu.py
shows that they reject wrong kernels at these very inputs); the integer variants and the pixel shuffle are compared exactly.  Write-only
outputs are pre-filled with NaN (float) or 77 (integer).  Each docstring records the worst |got - ref| / bound measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_kernel_refs as R
from infer_kernel_refs import BF16, F16, F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
IO = [F32, BF16, F16]
DT16 = [BF16, F16]
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
dtid = lambda d: IDS[d]


def within(tag, got, ref, bound):
    """|got - ref| <= bound at every element; the message carries the worst ratio."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    assert not bool(torch.isnan(got).any()), f"{tag}: the output holds a NaN (an element the kernel never wrote)"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    print(f"[{tag}] worst |got - ref| / bound {worst:.3f}")
    bad = err > bound
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements leave the bound, worst |got - ref| / bound {worst:.3f} "
                                 f"at {tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape))}")
    return worst


def dev16(a):
    """numpy uint16 -> device uint16 (uploaded as int16 bits)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def i32(t):
    """device integer frame -> host int32 values."""
    if t.dtype == torch.uint16:
        return torch.from_numpy(t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int32))
    return t.cpu().to(torch.int32)


# ---- bilinear_up4 -------------------------------------------------------------------------------------------------------------------

def _up4(fn, window, tab=None):
    """The engine's call: source = the strided centre-frame view of the (B,7,C,H,W) window, destination = the NHWC view of an NCHW
    tensor."""
    from fcvsr_amd import hip
    B, _, Cn, H, W = window.shape
    out = torch.full((B, Cn, 4 * H, 4 * W), NAN, device="cuda")
    cv, ov = hip.view(window[:, 3].permute(0, 2, 3, 1)), hip.view(out.permute(0, 2, 3, 1))
    args = (C.byref(cv),) + (() if tab is None else (tab.data_ptr(),)) + (B, H, W, C.byref(ov), hip.stream_ptr())
    hip.check(getattr(hip.lib(), fn)(*args), fn)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", R.BILINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bilinear_up4_vs_f64_reference(shape):
    """One source pixel, one row / column pair, odd sizes, a row longer than a wavefront.  measured <= 0.66"""
    w = R.bilinear_window(*shape)
    ref, bound = R.bilinear_up4(w[:, 3])
    within(f"bilinear_up4 {shape}", _up4("fcvsr_bilinear_up4", w.cuda()), ref, bound)


def _u8_windows():
    """The four shapes (values drawn at random) and a 16 x 16 frame that holds every byte value once."""
    for i, (B, Cn, H, W) in enumerate(R.BILINEAR_SHAPES):
        yield torch.randint(0, 256, (B, 7, Cn, H, W), generator=R.gen(7, i), dtype=torch.uint8)
    w = torch.randint(0, 256, (1, 7, 1, 16, 16), generator=R.gen(7, 9), dtype=torch.uint8)
    w[0, 3, 0] = torch.randperm(256, generator=R.gen(7, 10)).to(torch.uint8).view(16, 16)
    yield w


def _u16_windows():
    """The four shapes over 0..1100 (container values above 1023 included) and a 32 x 34 frame with every value 0..1023 and 64
    container values above 1023 (1024, 1025, 4095, 65535 among them)."""
    rs = np.random.RandomState(11)
    for (B, Cn, H, W) in R.BILINEAR_SHAPES:
        yield rs.randint(0, 1100, (B, 7, Cn, H, W)).astype(np.uint16)
    w = rs.randint(0, 1100, (1, 7, 1, 32, 34)).astype(np.uint16)
    over = np.concatenate([np.array([1024, 1025, 4095, 65535]), rs.randint(1024, 65536, 60)])
    w[0, 3, 0] = rs.permutation(np.concatenate([np.arange(1024), over])).reshape(32, 34).astype(np.uint16)
    yield w


def test_bilinear_up4_u8_equals_f32_kernel_on_table_values():
    """fcvsr_bilinear_up4_u8 on bytes k == fcvsr_bilinear_up4 on tab[k], bit for bit; all 256 byte values occur."""
    from fcvsr_amd import hip
    tab = hip.u8_table("cuda")
    seen = set()
    for w8 in _u8_windows():
        seen |= set(w8[:, 3].flatten().tolist())
        d8 = w8.cuda()
        got, want = _up4("fcvsr_bilinear_up4_u8", d8, tab), _up4("fcvsr_bilinear_up4", tab[d8.long()])
        assert torch.equal(got, want), f"{tuple(w8.shape)}: {int((got != want).sum())} of {want.numel()} values differ"
    assert len(seen) == 256


def test_bilinear_up4_u16_equals_f32_kernel_on_table_values():
    """fcvsr_bilinear_up4_u16 on samples k == fcvsr_bilinear_up4 on tab[min(k, 1023)], bit for bit; every value 0..1023 occurs and
    container values above 1023 read as 1023."""
    from fcvsr_amd import hip
    tab = hip.u16_table("cuda")
    seen = set()
    for w16 in _u16_windows():
        seen |= set(w16[:, 3].flatten().tolist())
        idx = torch.from_numpy(np.minimum(w16.astype(np.int64), 1023)).cuda()
        got, want = _up4("fcvsr_bilinear_up4_u16", dev16(w16), tab), _up4("fcvsr_bilinear_up4", tab[idx])
        assert torch.equal(got, want), f"{w16.shape}: {int((got != want).sum())} of {want.numel()} values differ"
    assert set(range(1024)) <= seen and max(seen) == 65535 and sum(v > 1023 for v in seen) >= 8


# ---- samples_to_f32 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.uint8, torch.uint16], ids=["u8", "u16"])
def test_samples_to_f32_reads_every_sample_value_through_the_table_of_its_dtype(dt):
    """hip.samples_to_f32 == tab[min(k, peak)], bit for bit, on every sample value (uint16: 0..1023 and container values above 1023)
    at numel 1027 (more than one block, no multiple of it) and, value by value, at numel 1; nothing past numel is written."""
    from fcvsr_amd import hip
    if dt == torch.uint8:
        k = np.arange(1027) % 256
        src, tab, peak = torch.from_numpy(k.astype(np.uint8)).cuda(), hip.u8_table("cuda"), 255
    else:
        k = np.concatenate([np.arange(1024), [1024, 4095, 65535]])
        src, tab, peak = dev16(k.astype(np.uint16)), hip.u16_table("cuda"), 1023
    assert tab.numel() == peak + 1 and src.numel() == 1027 and src.dtype == dt
    want = tab[torch.from_numpy(np.minimum(k, peak)).cuda()]
    whole = torch.full((1027 + 5,), NAN, device="cuda")
    hip.samples_to_f32(src, whole[:1027])
    single = torch.full((1027, 2), NAN, device="cuda")
    for i in range(1027):
        hip.samples_to_f32(src[i:i + 1], single[i, :1])
    torch.cuda.synchronize()
    assert torch.equal(whole[:1027], want) and bool(torch.isnan(whole[1027:]).all())
    assert torch.equal(single[:, 0], want) and bool(torch.isnan(single[:, 1]).all())


# ---- the fused tail -------------------------------------------------------------------------------------------------------------------

def _tail_dev(p):
    d = {k: p[k].cuda() for k in ("u1", "w2", "b2", "wl", "bl")}
    d["slope"] = torch.tensor([p["slope"]]).cuda()
    return d


def _tail_args(d):
    return (d["w2"].data_ptr(), d["b2"].data_ptr(), d["slope"].data_ptr(), d["wl"].data_ptr(), d["bl"].data_ptr())


def _tail_f32(p, d):
    """fcvsr_tail_fused on out = base (read-modify-write), out being the NHWC view of an NCHW tensor as in the engine."""
    from fcvsr_amd import hip
    B, H2, W2, _ = p["u1"].shape
    out = p["base"][:, None].cuda().contiguous()
    u1v, ov = hip.view(d["u1"]), hip.view(out.permute(0, 2, 3, 1))
    hip.check(hip.lib().fcvsr_tail_fused(C.byref(u1v), *_tail_args(d), B, H2, W2, C.byref(ov), hip.stream_ptr()), "fcvsr_tail_fused")
    torch.cuda.synchronize()
    return out[:, 0]


def _tail_check(tag, B, H, W, dt, slope):
    p = R.tail_inputs(B, H, W, dt, slope)
    ref, bound = R.tail_ref(p, dt)
    return within(tag, _tail_f32(p, _tail_dev(p)), ref, bound)


@pytest.mark.parametrize("slope", R.TAIL_SLOPES)
@pytest.mark.parametrize("B,H,W", R.TAIL_SMALL)
@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_tail_fused_vs_f64_reference(dt, B, H, W, slope):
    """A result narrower than one 8 x 32 tile (4 x 4), whole tiles in y and a partial one in x (6 x 20), partial both ways with a
    workgroup count that is no multiple of 8 (5 x 9); slopes inside [0, 1] and the generic PReLU form (1.5).
    measured <= 0.22 (bf16), 0.04 (f16)"""
    _tail_check(f"tail_fused {IDS[dt]} {B}x{H}x{W} slope {slope}", B, H, W, dt, slope)


@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_tail_fused_tile_runs_vs_f64_reference(dt):
    """36 x 68 with more tiles than launched workgroups (three per CU): a workgroup walks a run of tiles, across an image boundary.
    measured <= 0.30 (bf16), 0.06 (f16)"""
    H, W = R.TAIL_BIG_HW
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (4 * H // 8) * ((4 * W + 31) // 32)
    assert tiles == 18 * 9
    B = 3 * cus // tiles + 1
    assert B * tiles > 3 * cus and B <= 8, (B, cus)
    _tail_check(f"tail_fused {IDS[dt]} {B}x{H}x{W} tile runs", B, H, W, dt, 0.25)


@pytest.mark.parametrize("mode", ["truncate", "round"])
@pytest.mark.parametrize("B,H,W", [(3, 5, 9), (1, 6, 20)])
@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_tail_fused_u8_u16_equal_quantised_f32_result(dt, B, H, W, mode):
    """fcvsr_tail_fused_u8 / _u16 (u1, base) == quantise(fcvsr_tail_fused(u1, out = base), 255 / 1023, mode), exactly: the anchor of the
    f32 result carries over to the integer variants."""
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    p = R.tail_inputs(B, H, W, dt, 0.25)
    p["base"] = p["base"] * 1.3 - 0.15                        # both clamps occur
    d = _tail_dev(p)
    f32_result = _tail_f32(p, d).cpu()
    base = p["base"][:, None].cuda().contiguous()
    u1v, bv = hip.view(d["u1"]), hip.view(base.permute(0, 2, 3, 1))
    q = hip.QUANTISE[mode]
    for fn, peak, odt in (("fcvsr_tail_fused_u8", 255, torch.uint8), ("fcvsr_tail_fused_u16", 1023, torch.int16)):
        out = torch.full((B, 1, 4 * H, 4 * W), 77, device="cuda", dtype=odt)
        if peak == 1023:
            out = out.view(torch.uint16)
        ov = hip.view(out.permute(0, 2, 3, 1))
        hip.check(getattr(L, fn)(C.byref(u1v), *_tail_args(d), B, 2 * H, 2 * W, C.byref(bv), C.byref(ov), q, st), fn)
        torch.cuda.synchronize()
        want = R.quantise(f32_result, peak, mode)
        got = i32(out)[:, 0]
        assert torch.equal(base[:, 0].cpu(), p["base"]), f"{fn}: the f32 base was written"
        assert torch.equal(got, want), f"{fn} {mode}: {int((got != want).sum())} of {want.numel()} samples differ"
        assert int(want.min()) == 0 and int(want.max()) == peak and torch.unique(want).numel() > 32


# ---- gc_apply ---------------------------------------------------------------------------------------------------------------------------

def _gc_levels(levels, Cn, dt, rdt):
    """One fcvsr_gc_apply_levels launch over `levels` [(H, W, pooled)], B = 2; returns [(tag, got, ref, bound)]."""
    from fcvsr_amd import hip
    B = 2
    al = (hip.GcApplyLevel * 3)()
    keep, res = [], []
    for l, (H, W, pooled) in enumerate(levels):
        p = R.gc_inputs(B, H, W, Cn, dt, rdt)
        d = {k: v.cuda() for k, v in p.items()}
        out = torch.full((B, H, W, Cn), NAN, device="cuda", dtype=dt)
        pool = torch.full((B, H // 2, W // 2, Cn), NAN, device="cuda", dtype=dt) if pooled else None
        al[l].r, al[l].add, al[l].z, al[l].out, al[l].pool = d["r"].data_ptr(), d["add"].data_ptr(), d["z"].data_ptr(), out.data_ptr(), hip.ptr(pool)
        al[l].B, al[l].H, al[l].W = B, H, W
        keep.append(d)
        res.append((p, out, pool))
    hip.check(hip.lib().fcvsr_gc_apply_levels(al, len(levels), R.DT_CODE[dt], R.DT_CODE[rdt], 0.2, Cn, hip.stream_ptr()), "fcvsr_gc_apply_levels")
    torch.cuda.synchronize()
    cmp = []
    for (H, W, pooled), (p, out, pool) in zip(levels, res):
        cmp.append((f"out {H}x{W}", out, *R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt)))
        if pooled:
            cmp.append((f"pool {H}x{W}", pool, *R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt, pool=True)))
    return cmp


@pytest.mark.parametrize("dt,r16", [(F32, False), (BF16, False), (BF16, True), (F16, False), (F16, True)],
                         ids=["f32-r_f32", "bf16-r_f32", "bf16-r_io", "f16-r_f32", "f16-r_io"])
def test_gc_apply_levels_vs_f64_reference(dt, r16):
    """Three levels in one launch ((6,10) pooled, (3,5) not, (22,18) pooled; C = 64) and one single-level launch with C = 36: `out` and
    `pool`, the latter averaged from the ROUNDED out.  measured <= 0.61 (out) and 0.37 (pool) in f32, 0.998 (out) and 0.999 (pool)
    in the 16-bit modes, where the store's half unit in the last place is nearly the whole bound and one element of thousands comes
    close to it"""
    rdt = dt if r16 else F32
    for levels, Cn in ((R.GC_LEVELS, 64), (R.GC_LEVELS[:1], 36)):
        for name, got, ref, bound in _gc_levels(levels, Cn, dt, rdt):
            within(f"gc_apply_levels {IDS[dt]} r {IDS[rdt]} C{Cn} {name}", got, ref, bound)


@pytest.mark.parametrize("H,W", [(3, 5), (22, 18)])
@pytest.mark.parametrize("dt", IO, ids=dtid)
def test_gc_apply_vs_f64_reference(dt, H, W):
    """The single-level entry point (f32 r).  measured <= 0.61 (f32), 0.998 (16-bit: the store's half unit)"""
    from fcvsr_amd import hip
    B, Cn = 2, 64
    p = R.gc_inputs(B, H, W, Cn, dt, F32)
    d = {k: v.cuda() for k, v in p.items()}
    out = torch.full((B, H, W, Cn), NAN, device="cuda", dtype=dt)
    hip.check(hip.lib().fcvsr_gc_apply(d["r"].data_ptr(), d["add"].data_ptr(), d["z"].data_ptr(), out.data_ptr(), R.DT_CODE[dt], 0.2, B, H, W, Cn,
                                       hip.stream_ptr()), "fcvsr_gc_apply")
    torch.cuda.synchronize()
    within(f"gc_apply {IDS[dt]} {H}x{W}", out, *R.gc_apply(p["r"], p["add"], p["z"], 0.2, dt))


# ---- xscale -----------------------------------------------------------------------------------------------------------------------------

def _xs_levels(levels, Cn, dt):
    from fcvsr_amd import hip
    B = 2
    xl = (hip.XscaleLevel * 3)()
    keep, res = [], []
    for l, ((H, W), dn, up, rs) in enumerate(levels):
        p = R.xscale_inputs(B, H, W, Cn, dt, dn, up)
        d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items()}
        out = torch.full((B, H, W, Cn), NAN, device="cuda", dtype=dt)
        xl[l].x, xl[l].r, xl[l].out = d["x"].data_ptr(), d["r"].data_ptr(), out.data_ptr()
        xl[l].dn, xl[l].up = hip.ptr(d["dn"]), hip.ptr(d["up"])
        xl[l].r_scale, xl[l].dn_pooled = rs, p["dn_pooled"]
        xl[l].B, xl[l].H, xl[l].W = B, H, W
        keep.append(d)
        res.append((p, out, rs))
    hip.check(hip.lib().fcvsr_xscale_levels(xl, len(levels), R.DT_CODE[dt], Cn, hip.stream_ptr()), "fcvsr_xscale_levels")
    torch.cuda.synchronize()
    return [(f"{H}x{W}", out, *R.xscale(p["x"], p["r"], rs, p["dn"], p["dn_pooled"], p["up"], dt))
            for ((H, W), _, _, _), (p, out, rs) in zip(levels, res)]


@pytest.mark.parametrize("Cn", [64, 36])
@pytest.mark.parametrize("dt", IO, ids=dtid)
def test_xscale_levels_vs_f64_reference(dt, Cn):
    """C = 64 (16-byte accesses in the 16-bit modes) and C = 36 (8-byte); three levels in one launch - (22,18) with up from (11,9),
    (12,10) with a pooled dn and up from (6,5), (3,5) with an unpooled dn at (6,10) - and (2,2) with up from a single pixel.
    measured <= 0.71 (f32), 0.999 (16-bit: the store's half unit)"""
    for levels in (R.XS_LEVELS, [((2, 2), None, True, 2.0)]):
        for name, got, ref, bound in _xs_levels(levels, Cn, dt):
            within(f"xscale_levels {IDS[dt]} C{Cn} {name}", got, ref, bound)


@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_xscale_vs_f64_reference(dt):
    """The single-level entry point in the 16-bit modes at (12,10) with an unpooled dn and up.  measured <= 0.997"""
    from fcvsr_amd import hip
    B, H, W, Cn = 2, 12, 10, 64
    p = R.xscale_inputs(B, H, W, Cn, dt, "full", True)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items()}
    out = torch.full((B, H, W, Cn), NAN, device="cuda", dtype=dt)
    hip.check(hip.lib().fcvsr_xscale(d["x"].data_ptr(), d["r"].data_ptr(), 1.0, d["dn"].data_ptr(), d["up"].data_ptr(), out.data_ptr(),
                                     R.DT_CODE[dt], B, H, W, Cn, hip.stream_ptr()), "fcvsr_xscale")
    torch.cuda.synchronize()
    within(f"xscale {IDS[dt]}", out, *R.xscale(p["x"], p["r"], 1.0, p["dn"], 0, p["up"], dt))


# ---- feat_extract ---------------------------------------------------------------------------------------------------------------------

def _feat(fn, xwin, p, B, H, W, dt, tab=None, stride=64, choff=0):
    """The engine's launch: 7 blocks of 64 channels to p13[k, :B] (k = 0..2), f2, p13[k, B:]; returns them as (B,H,W,448) and the
    whole destination buffers."""
    from fcvsr_amd import hip
    n = 64
    p13 = torch.full((3, 2 * B, H, W, stride), NAN, device="cuda", dtype=dt)
    f2 = torch.full((B, H, W, stride), NAN, device="cuda", dtype=dt)
    dst = [p13[k, :B] for k in range(3)] + [f2] + [p13[k, B:] for k in range(3)]
    wm = p["wmat"].cuda()
    bias = None if p["bias"] is None else p["bias"].cuda()
    xv = hip.view(xwin.view(B, 7, H, W).permute(0, 2, 3, 1))
    P = C.c_void_p * 7
    args = (C.byref(xv),) + (() if tab is None else (tab.data_ptr(),)) + (
        B, H, W, wm.data_ptr(), hip.ptr(bias), 7, P(*[t.data_ptr() for t in dst]), (C.c_int64 * 7)(*([stride] * 7)),
        (C.c_int32 * 7)(*([choff] * 7)), R.DT_CODE[dt], hip.stream_ptr())
    hip.check(getattr(hip.lib(), fn)(*args), fn)
    torch.cuda.synchronize()
    return torch.cat([t[..., choff:choff + n] for t in dst], dim=3), (p13, f2)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,H,W", R.FEAT_SHAPES)
@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_feat_extract_vs_f64_reference(dt, B, H, W, with_bias):
    """The dedicated K = 64 im2col kernel (cin = 7, n = 64): 16 pixels, 90 pixels (one partial 128-pixel workgroup spanning two
    images), 720 pixels (5.6 workgroups, rows wrap inside a workgroup); k / 255 inputs (window (B,7,1,H,W)).
    measured <= 0.985 (bf16), 0.945 (f16): the store's half unit"""
    p = R.feat_inputs(B, H, W, with_bias)
    got, _ = _feat("fcvsr_feat_extract", p["x"].view(B, 7, 1, H, W).cuda(), p, B, H, W, dt)
    within(f"feat_extract {IDS[dt]} {B}x{H}x{W}", got, *R.feat_extract(p["x"], p["wmat"], p["bias"], dt))


@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_feat_extract_pixel_stride_and_channel_offset(dt):
    """dsx = 96 > 64 and dch = 16: channels [16, 80) of every destination pixel are written, the others keep their pre-fill.
    measured <= 0.970 (bf16), 0.931 (f16)"""
    B, H, W = 2, 5, 9
    p = R.feat_inputs(B, H, W)
    got, (p13, f2) = _feat("fcvsr_feat_extract", p["x"].view(B, 7, 1, H, W).cuda(), p, B, H, W, dt, stride=96, choff=16)
    within(f"feat_extract {IDS[dt]} stride 96 offset 16", got, *R.feat_extract(p["x"], p["wmat"], p["bias"], dt))
    for t in (p13, f2):
        assert bool(torch.isnan(t[..., :16]).all()) and bool(torch.isnan(t[..., 80:]).all()), "channels outside [16, 80) were written"


@pytest.mark.parametrize("B,H,W", R.FEAT_SHAPES)
@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_feat_extract_u8_u16_equal_f32_entry_on_table_values(dt, B, H, W):
    """fcvsr_feat_extract_u8 / _u16 on samples k == fcvsr_feat_extract on tab[min(k, peak)], bit for bit."""
    from fcvsr_amd import hip
    p = R.feat_inputs(B, H, W)
    t8, t16 = hip.u8_table("cuda"), hip.u16_table("cuda")
    x8 = p["x8"].view(B, 7, 1, H, W).cuda()
    got, _ = _feat("fcvsr_feat_extract_u8", x8, p, B, H, W, dt, tab=t8)
    want, _ = _feat("fcvsr_feat_extract", t8[x8.long()], p, B, H, W, dt)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"u8: {int((got != want).sum())} values differ"
    a16 = np.random.RandomState(B * 100 + H).randint(0, 1100, (B, 7, 1, H, W)).astype(np.uint16)
    got, _ = _feat("fcvsr_feat_extract_u16", dev16(a16), p, B, H, W, dt, tab=t16)
    want, _ = _feat("fcvsr_feat_extract", t16[torch.from_numpy(np.minimum(a16.astype(np.int64), 1023)).cuda()], p, B, H, W, dt)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"u16: {int((got != want).sum())} values differ"
    assert int(a16.max()) > 1023


# ---- scale_add, pixel_shuffle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [64, 36])
@pytest.mark.parametrize("xdt,odt", [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)], ids=lambda d: IDS[d])
def test_scale_add_vs_f64_reference(xdt, odt, Cn):
    """(2,5,7,C): 2240 / 1260 quads, no multiple of 256.  measured <= 0.98 (f32: one fma, the bound is half a unit in the last
    place of the result's condition), 0.994 (16-bit stores)"""
    from fcvsr_amd import hip
    B, H, W = 2, 5, 7
    assert (B * H * W * Cn // 4) % 256
    p = R.scale_add_inputs(B, H, W, Cn, xdt)
    d = {k: v.cuda() for k, v in p.items()}
    out = torch.full((B, H, W, Cn), NAN, device="cuda", dtype=odt)
    hip.check(hip.lib().fcvsr_scale_add(d["z"].data_ptr(), d["gate"].data_ptr(), d["x"].data_ptr(), R.DT_CODE[xdt], out.data_ptr(),
                                        R.DT_CODE[odt], B, H, W, Cn, hip.stream_ptr()), "fcvsr_scale_add")
    torch.cuda.synchronize()
    within(f"scale_add C{Cn} {IDS[xdt]} -> {IDS[odt]}", out, *R.scale_add(p["z"], p["gate"], p["x"], odt))


@pytest.mark.parametrize("B,H,W,Cn", [(2, 3, 5, 16), (1, 7, 9, 256)])
def test_pixel_shuffle_equals_torch(B, H, W, Cn):
    """fcvsr_pixel_shuffle (dense NHWC f32) == F.pixel_shuffle, exactly."""
    from fcvsr_amd import hip
    src = torch.randn(B, H, W, Cn, generator=R.gen(8, B, H, W, Cn))
    s = src.cuda()
    dst = torch.full((B, 2 * H, 2 * W, Cn // 4), NAN, device="cuda")
    hip.check(hip.lib().fcvsr_pixel_shuffle(s.data_ptr(), dst.data_ptr(), B, H, W, Cn, hip.stream_ptr()), "fcvsr_pixel_shuffle")
    torch.cuda.synchronize()
    want = F.pixel_shuffle(src.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(dst.cpu(), want)
