"""GPU: every kernel that ends in the integer sample rule (csrc/u8.h `quantised<PEAK>`; csrc/bicubic_up.h `up_result`) is driven so
that the f32 value reaching the rule is an entry of tests/sample_rule_cases.py's table, bit for bit, and its samples are compared
with the numpy `rule` exactly, on the CPU.  The table holds what random floats never do: f32 products on k + 0.5 for every k (half to
even against roundf and floorf(q + 0.5f)), ties and carried integers whose exact product lies off them (one f32 multiply against an
fma or an f64 multiply), the clamp edges, and a NaN (sample 0: the clamp order).  tests/test_sample_rule_cpu.py shows that each wrong
spelling changes samples of this table.  Integer outputs that the caller allocates are pre-filled with 77 and the 64 guard words
behind them are checked.

How each site's value is dictated, and what ran there (u8: peak 255, 1803 entries; u16: peak 1023, 7698 entries):
  hip.quantise (_u8, _u16; both modes)        the input IS the value.  The whole table in one launch (1803 / 7698 samples: no
                                              multiple of 256), then the mutant-killing entries (`killers`) again at n = 1.
  hip.tail_fused -> _u8 / _u16 (bf16, f16;    wl = 0 and bl = 0 (asserted), u1 / w2 / b2 random and finite: every last-layer
  both modes)                                 product is an exact 0, the sum is base + 0.  base = the whole table as a 44 x 44
                                              (u8) / 88 x 88 (u16) plane.  The f32 form on the same inputs returns base bit for bit
                                              (-0.0 comes back as 0.0: -0 + 0): that proves the value was dictated.
  hip.conv_last -> _u8 / _u16 (C = 1, 3;      wl = 0, no bias, base = the whole table (43 x 43, 88 x 88; three channels: 25 x 25,
  bf16; both modes)                           51 x 51); the f32 form returns base likewise.
  hip.tail_fused(centre=) -> _base_u8 /       a zero centre frame gives an exact zero base, wl = 0: the value is bl.  One 4 x 4
  _base_u16 (both modes)                      launch per entry of `short_list`: an even-k tie, an odd-k tie, a tie with the exact
                                              product below and one above, a carried integer (u16), 1, nextafter(1, 2), -1, NaN;
                                              the f32 form returns bl in all 16 pixels.
  hip.ensemble_merge (8 and 16 passes;        (a) all passes are `variant_host` of one 48 x 48 / 96 x 96 table plane.  The fixed-
  both modes, both formats)                   order f32 sum of eight equal values is NOT 8v (3v, 5v, 6v, 7v are rounded): the f32
                                              form returns `mean8` of the table bit for bit - v itself for 965 / 4001 entries, ties
                                              of both parities, inexact products and carried integers among them (the CPU test
                                              counts them) - and the samples are rule(mean8).  (b) passes 0..3 hold 1, 1, 2, 4
                                              times the plane, passes 4..7 zeros: v, 2v, 4v, 8v are exact, the f32 form returns
                                              the table itself (+-3.4e38 -> +-inf, the same samples) and every entry reaches the rule.
  hip.tile_merge and its src= (_sel) form     one tile covers the frame: the host-made wy and wx are exactly 1.0 (asserted),
  (both modes, both formats)                  0 + (1 * 1) * v = v; the f32 form returns the 48 x 48 / 96 x 96 table plane.
  hip.frame_metric_sums (8-bit with and       f32 frames = the table tiled into the least plane (43 x 43, 88 x 88; RGB 25 x 25)
  without to_y, _u16), hip.niqe_features,     with quantise = truncate / round against the same call on the integer frames `rule`
  hip.brisque_features (with / without to_y)  makes, QUANT_NONE: equal bits of every f64 result (fixed-order reductions).  NIQE:
                                              96 x 192, the least it admits; BRISQUE: 44 x 44 and RGB 26 x 26.
  hip.bicubic_upscale (x2, x4; u8, u16),      the second spelling.  `upscale_plane`: integer planes of identical rows whose dyadic
  hip.imresize (scale 2, 4), hip.active_      tap sums are exactly k + 0.5 on even and odd k, with overshoot below 0 and above
  compose                                     the peak; against the host contract's bits, and the planted pixels carry k + (k & 1).
NaN: asserted as sample 0 at every site above that takes an f32 (all but the up-scale family, whose inputs are integers).

Left out, because their value cannot be dictated: fcvsr_chroma_up4 / fcvsr_chroma_up4_u16 (the bicubic taps of F.interpolate are
not dyadic f32: no input makes the sum an exact tie) and fcvsr_tail_fused_base_u8 / _u16 beyond the short list above (the base is
computed from the integer centre frame: only a zero frame gives an exact base, so one value per launch).

Measured, not asserted (torch's NaN-to-integer cast is not specified): harness.infer._quantised_dev of a NaN on an MI355X gives
sample 0 at both peaks in both modes, as the kernels do."""
import numpy as np
import pytest
import torch

import sample_rule_cases as S

pytestmark = pytest.mark.gpu

GUARD = 64
DT = {255: torch.uint8, 1023: torch.uint16}
FMT = pytest.mark.parametrize("peak", S.PEAKS, ids=["u8", "u16"])
MODE = pytest.mark.parametrize("mode", S.MODES)
DT16 = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def guarded(peak, *shape):
    """(buffer, out): an integer tensor of `shape` in the format of `peak` filled with 77, followed by GUARD samples of 77."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), 77, dtype=torch.uint8 if peak == 255 else torch.int16, device="cuda")
    return buf, buf[:n].view(*shape).view(DT[peak])


def samples(t):
    """Integer device tensor -> host int64."""
    from fcvsr_amd import hip
    return hip.frames_to_numpy(t).astype(np.int64)


def guard_intact(buf):
    return bool((buf[-GUARD:].cpu() == 77).all())


def dev(a):
    """numpy f32 / uint8 / uint16 -> device tensor."""
    a = np.array(a, order="C")                               # a writable copy: the table's arrays are read-only
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def same(tag, got, want, values=None):
    """Exact equality of integer samples; the message names the first entries that differ."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        rows = [(int(i), None if values is None else repr(np.asarray(values).reshape(-1)[i]), int(got[i]), int(want[i])) for i in bad[:6]]
        raise AssertionError(f"{tag}: {bad.size} of {want.size} samples differ; (position, value, got, want) {rows}")


def dictated(base):
    """What base + 0 is, bit for bit: base, with -0.0 as 0.0."""
    return np.where(base == 0, np.float32(0), base).astype(np.float32)


def wants(plane, peak, mode):
    w = S.rule(plane, peak, mode)
    assert w[np.isnan(plane)].size >= 1 and not w[np.isnan(plane)].any()                         # NaN -> sample 0
    assert int(w.min()) == 0 and int(w.max()) == peak
    return w


# ---- hip.quantise ----------------------------------------------------------------------------------------------------------------------

@MODE
@FMT
def test_quantise_on_the_whole_table_and_on_single_killing_entries(peak, mode):
    from fcvsr_amd import hip
    t = S.table(peak)
    n, q = t.values.size, hip.QUANTISE[mode]
    assert n % 256 != 0 and n > 256
    src = dev(t.values)
    buf, out = guarded(peak, n)
    hip.quantise(src, out, q)
    kill = S.killers(peak)[mode]
    single = torch.full((kill.size, 2), 77, dtype=buf.dtype, device="cuda")
    for j, i in enumerate(kill.tolist()):
        hip.quantise(src[i:i + 1], single[j, :1].view(DT[peak]), q)
    torch.cuda.synchronize()
    want = wants(t.values, peak, mode)
    same(f"quantise {peak} {mode}", samples(out), want, t.values)
    assert guard_intact(buf)
    one = samples(single.view(DT[peak]))
    same(f"quantise {peak} {mode} n = 1", one[:, 0], want[kill], t.values[kill])
    assert bool((one[:, 1] == 77).all())


# ---- the fused tail and conv_last: wl = 0, the base is the table ---------------------------------------------------------------------

def _tail_weights(dt, hw, seed):
    g = torch.Generator().manual_seed(seed)
    u1 = torch.randn(1, 2 * hw, 2 * hw, 64, generator=g).to(dt).cuda()
    w2 = (torch.randn(256, 64, generator=g) / 8).to(dt).cuda()
    b2 = (torch.randn(256, generator=g) * 0.1).cuda()
    wl = torch.zeros(16, 64, dtype=dt, device="cuda")
    assert bool(torch.isfinite(u1.float()).all()) and bool(torch.isfinite(w2.float()).all()) and not bool(wl.float().any())
    return u1, w2, b2, torch.tensor([0.25]).cuda(), wl


@MODE
@DT16
@FMT
def test_tail_fused_integer_forms_on_a_dictated_base(peak, dt, mode):
    from fcvsr_amd import hip
    s = S.side(peak, 4)
    hw = s // 4
    plane = S.plane(peak, s, s)
    u1, w2, b2, slope, wl = _tail_weights(dt, hw, 3 + peak)
    bl = torch.zeros(1, device="cuda")
    assert float(bl[0]) == 0.0
    base = dev(plane)[None]                                                                      # (1,1,4H,4W)
    f32 = base.clone()
    hip.tail_fused(u1, w2, b2, slope, wl, bl, 1, 2 * hw, 2 * hw, f32.permute(0, 2, 3, 1), base=f32.permute(0, 2, 3, 1))
    buf, out = guarded(peak, 1, 1, s, s)
    hip.tail_fused(u1, w2, b2, slope, wl, bl, 1, 2 * hw, 2 * hw, out.permute(0, 2, 3, 1), base=base.permute(0, 2, 3, 1),
                   quant=hip.QUANTISE[mode])
    torch.cuda.synchronize()
    assert S.same_bits(f32.cpu().numpy()[0], dictated(plane)), "the f32 form did not return base: the value is not dictated"
    assert S.same_bits(base.cpu().numpy()[0], plane), "the integer form wrote its f32 base"
    same(f"tail_fused {peak} {dt} {mode}", samples(out), wants(plane, peak, mode), plane)
    assert guard_intact(buf)


@MODE
@pytest.mark.parametrize("channels", [1, 3])
@FMT
def test_conv_last_integer_forms_on_a_dictated_base(peak, channels, mode):
    from fcvsr_amd import hip
    dt = torch.bfloat16
    s = S.side(peak, 1, channels)
    plane = S.plane(peak, s, s, channels)
    g = torch.Generator().manual_seed(5 + peak + channels)
    u2 = torch.randn(1, s, s, 64, generator=g).to(dt).cuda()
    wl = torch.zeros(16 if channels == 1 else 32, 64, dtype=dt, device="cuda")
    assert bool(torch.isfinite(u2.float()).all()) and not bool(wl.float().any())
    base = dev(plane)[None]                                                                      # (1,C,H,W)
    f32 = base.clone()
    hip.conv_last(u2, wl, None, 1, s, s, channels, f32.permute(0, 2, 3, 1), f32.permute(0, 2, 3, 1))
    buf, out = guarded(peak, 1, channels, s, s)
    hip.conv_last(u2, wl, None, 1, s, s, channels, base.permute(0, 2, 3, 1), out.permute(0, 2, 3, 1), hip.QUANTISE[mode])
    torch.cuda.synchronize()
    assert S.same_bits(f32.cpu().numpy()[0], dictated(plane)), "the f32 form did not return base: the value is not dictated"
    assert S.same_bits(base.cpu().numpy()[0], plane), "the integer form wrote its f32 base"
    same(f"conv_last {peak} C={channels} {mode}", samples(out), wants(plane, peak, mode), plane)
    assert guard_intact(buf)


@MODE
@FMT
def test_tail_fused_base_integer_forms_one_value_per_launch(peak, mode):
    """A zero centre frame and wl = 0: the value is the bias bl.  One 4 x 4 launch per entry of the short list."""
    from fcvsr_amd import hip
    t, sl = S.table(peak), S.short_list(peak)
    dt = torch.bfloat16
    u1, w2, b2, slope, wl = _tail_weights(dt, 1, 9 + peak)
    centre_i = torch.zeros(1, 1, 1, 1, dtype=torch.uint8 if peak == 255 else torch.int16, device="cuda").view(DT[peak])
    centre_f = torch.zeros(1, 1, 1, 1, device="cuda")
    hip.sample_table(DT[peak], "cuda")
    got, f32s, bufs = {}, {}, {}
    for name, i in sl.items():
        bl = dev(t.values[i:i + 1])
        f32s[name] = torch.full((1, 4, 4, 1), 7.0, device="cuda")
        hip.tail_fused(u1, w2, b2, slope, wl, bl, 1, 2, 2, f32s[name], centre=centre_f)
        bufs[name], got[name] = guarded(peak, 1, 4, 4, 1)
        hip.tail_fused(u1, w2, b2, slope, wl, bl, 1, 2, 2, got[name], centre=centre_i, quant=hip.QUANTISE[mode])
    torch.cuda.synchronize()
    for name, i in sl.items():
        v = t.values[i]
        assert S.same_bits(f32s[name].cpu().numpy().reshape(-1), np.full(16, v, dtype=np.float32)), (name, "the value is not dictated")
        want = S.rule(v, peak, mode)
        same(f"tail_fused_base {peak} {mode} {name} ({v!r})", samples(got[name]), np.full(16, want), np.full(16, v))
        assert guard_intact(bufs[name])
    assert S.rule(t.values[sl["nan"]], peak, mode) == 0


# ---- the merges ------------------------------------------------------------------------------------------------------------------------

def _passes(plane, scales):
    """(a, at) of hip.ensemble_merge for one square (s, s) plane: pass i holds `variant_host` of scales[i] * plane."""
    from fcvsr_amd.harness.ensemble import variant_host
    with np.errstate(over="ignore"):
        v = [variant_host(np.float32(scales[i]) * plane if scales[i] else np.zeros_like(plane), i) for i in range(8)]
    return dev(np.stack(v[:4])[:, None, None]), dev(np.stack(v[4:])[:, None, None])


@pytest.mark.parametrize("temporal", [False, True], ids=["x8", "x16"])
@FMT
def test_ensemble_merge_integer_output_on_dictated_means(peak, temporal):
    from fcvsr_amd import hip
    s = S.side(peak, 16)
    h = s // 4
    plane = S.plane(peak, s, s)[0]
    with np.errstate(over="ignore"):
        exact = (np.float32(8) * plane) * np.float32(0.125)                                      # the table; +-3.4e38 -> +-inf
    assert np.array_equal(np.flatnonzero(exact.view(np.int32) != plane.view(np.int32)), np.flatnonzero(np.abs(plane) == np.float32(3.4e38)))
    # (b): -0.0 comes back as 0.0 (the zero passes are +0.0)
    for tag, scales, value in (("equal passes", [1] * 8, S.mean8(plane)), ("1, 1, 2, 4, 0, 0, 0, 0", [1, 1, 2, 4, 0, 0, 0, 0], dictated(exact))):
        a, at = _passes(plane, scales)
        kw = dict(ra=a, rat=at) if temporal else {}
        f32 = hip.ensemble_merge(a, at, h, h, **kw)
        ints = {mode: hip.ensemble_merge(a, at, h, h, dtype=DT[peak], quantise=mode, **kw) for mode in S.MODES}
        torch.cuda.synchronize()
        assert S.same_bits(f32.cpu().numpy()[0, 0], value), f"{tag}: the f32 form did not return the dictated value"
        for mode in S.MODES:
            assert ints[mode].dtype == DT[peak] and tuple(ints[mode].shape) == (1, 1, s, s)
            same(f"ensemble_merge {peak} {mode} {tag}", samples(ints[mode]), wants(value, peak, mode), value)


@pytest.mark.parametrize("sel", [False, True], ids=["tile_merge", "tile_merge_sel"])
@FMT
def test_tile_merge_integer_output_on_one_tile_with_unit_weights(peak, sel):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.tiles import tile_plan
    s = S.side(peak, 16)
    h = s // 4
    plan = tile_plan(h, h, h, 0)
    assert (plan.ny, plan.nx, plan.th, plan.tw) == (1, 1, h, h)
    assert plan.wy.dtype == np.float32 and bool((plan.wy == 1).all()) and bool((plan.wx == 1).all()) and plan.wy.shape == (1, s)
    plane = S.plane(peak, s, s)
    if sel:
        tiles = torch.stack([torch.zeros(1, s, s), torch.from_numpy(plane)]).cuda()              # a pool of two, slot 1 is used
        kw = dict(src=torch.ones(1, 1, 1, dtype=torch.int32, device="cuda"))
    else:
        tiles, kw = dev(plane)[None, None, None], {}
    f32 = hip.tile_merge(tiles, plan, h, h, **kw)
    ints = {mode: hip.tile_merge(tiles, plan, h, h, dtype=DT[peak], quantise=mode, **kw) for mode in S.MODES}
    torch.cuda.synchronize()
    assert S.same_bits(f32.cpu().numpy()[0], dictated(plane)), "the f32 form did not return the tile: the value is not dictated"
    for mode in S.MODES:
        assert ints[mode].dtype == DT[peak] and tuple(ints[mode].shape) == (1, 1, s, s)
        same(f"tile_merge {peak} {mode} sel={sel}", samples(ints[mode]), wants(plane, peak, mode), plane)


# ---- the scorers: f32 frames quantised on the way in == the integer frames of the rule ---------------------------------------------

def _frames(peak, h, w, channels, mode):
    """(f32 device frames (1,C,h,w) holding the table, the integer device frames `rule` makes of them)."""
    plane = S.plane(peak, h, w, channels)
    q = wants(plane, peak, mode).astype(np.uint8 if peak == 255 else np.uint16)
    return dev(plane)[None], dev(q)[None]


def _bits64(t):
    return t.cpu().contiguous().view(torch.int64)


@MODE
@pytest.mark.parametrize("peak,to_y", [(255, False), (255, True), (1023, False)], ids=["u8", "u8-to_y", "u16"])
def test_frame_metric_sums_quantise_on_the_way_in(peak, to_y, mode):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.metrics import _gaussian_window
    channels = 3 if to_y else 1
    s = S.side(peak, 1, channels)
    f32, ints = _frames(peak, s, s, channels, mode)
    hr = dev(np.random.RandomState(peak + channels).randint(0, peak + 1, (1, channels, s, s)).astype(np.uint8 if peak == 255 else np.uint16))
    got = hip.frame_metric_sums(f32, hr, hip.QUANTISE[mode], 0, to_y, _gaussian_window())
    want = hip.frame_metric_sums(ints, hr, hip.QUANT_NONE, 0, to_y, _gaussian_window())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 2) and bool(torch.isfinite(want).all()) and float(want[0, 0]) > 0
    assert torch.equal(_bits64(got), _bits64(want)), (got.cpu().tolist(), want.cpu().tolist())


@MODE
@pytest.mark.parametrize("to_y", [False, True], ids=["plane", "to_y"])
def test_niqe_features_quantise_on_the_way_in(to_y, mode):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.brisque import gaussian_window
    from fcvsr_amd.harness.niqe import aggd_tables
    from fcvsr_amd.harness.nss import device_tables
    f32, ints = _frames(255, 96, 192, 3 if to_y else 1, mode)                                    # two 96 x 96 blocks: the least
    tables = device_tables("niqe", aggd_tables(), "cuda")
    got = hip.niqe_features(f32, hip.QUANTISE[mode], 0, to_y, gaussian_window(), tables)
    want = hip.niqe_features(ints, hip.QUANT_NONE, 0, to_y, gaussian_window(), tables)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 2, 36) and bool(torch.isfinite(want).any())
    assert torch.equal(_bits64(got), _bits64(want))


@MODE
@pytest.mark.parametrize("to_y", [False, True], ids=["plane", "to_y"])
def test_brisque_features_quantise_on_the_way_in(to_y, mode):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.brisque import brisque_tables, gaussian_window
    from fcvsr_amd.harness.nss import device_tables
    channels = 3 if to_y else 1
    s = S.side(255, 2, channels)
    f32, ints = _frames(255, s, s, channels, mode)
    tables = device_tables("brisque", brisque_tables(), "cuda")
    got = hip.brisque_features(f32, hip.QUANTISE[mode], to_y, gaussian_window(), tables)
    want = hip.brisque_features(ints, hip.QUANT_NONE, to_y, gaussian_window(), tables)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 36) and bool(torch.isfinite(want).any())
    assert torch.equal(_bits64(got), _bits64(want))


# ---- the up-scale family: the second spelling --------------------------------------------------------------------------------------------

def _planted(u, got):
    cols = np.flatnonzero(u.tie)
    k = u.k[cols]
    assert cols.size * got.shape[0] >= 8 and int((k % 2 == 0).sum()) >= 1 and int((k % 2 == 1).sum()) >= 1
    return cols, np.repeat((k + (k % 2))[None], got.shape[0], axis=0)


@pytest.mark.parametrize("op", ["bicubic_upscale", "imresize"])
@pytest.mark.parametrize("factor", [2, 4])
@FMT
def test_bicubic_upscale_and_imresize_integer_output_on_planted_ties(peak, factor, op):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.niqe import bicubic_upscale
    from fcvsr_amd.harness.resize import imresize_host
    u = S.upscale_plane(factor, peak)
    if op == "bicubic_upscale":
        got, want = hip.bicubic_upscale(dev(u.plane), factor, out="int"), bicubic_upscale(u.plane, factor, out="int")
    else:
        got, want = hip.imresize(dev(u.plane), scale=factor, out="int"), imresize_host(u.plane, scale=factor, out="int")
    torch.cuda.synchronize()
    assert got.dtype == DT[peak]
    got = samples(got)
    same(f"{op} x{factor} {peak}", got, want.astype(np.int64))
    cols, even = _planted(u, got)
    same(f"{op} x{factor} {peak}: the planted ties", got[:, cols], even)
    assert int(got.min()) == 0 and int(got.max()) == peak


@FMT
def test_active_compose_integer_output_on_planted_ties(peak):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.active import compose_host
    u = S.upscale_plane(4, peak)
    H, W = u.plane.shape
    box = (0, 1, W - 2, W)                                                                       # over the trailing zeros
    assert not u.tie[4 * (W - 2):].any()
    lr = u.plane[None, None]
    sr = np.full((1, 1, 4, 8), 5, dtype=u.plane.dtype)
    got = hip.active_compose(dev(sr), dev(lr), [0], box, H, W)
    torch.cuda.synchronize()
    assert got.dtype == DT[peak]
    got = samples(got)
    same(f"active_compose {peak}", got, compose_host(sr, lr, box).astype(np.int64))
    cols, even = _planted(u, got[0, 0])
    same(f"active_compose {peak}: the planted ties", got[0, 0][:, cols], even)


# ---- measured, not asserted ------------------------------------------------------------------------------------------------------------

def test_print_what_the_torch_spelling_gives_for_nan_on_the_device():
    from fcvsr_amd.harness.infer import _quantised, _quantised_dev
    nan = torch.full((4,), float("nan"), device="cuda")
    for peak in S.PEAKS:
        for mode in S.MODES:
            print(f"[_quantised_dev NaN] peak {peak} {mode}: {samples(_quantised_dev(nan, mode, float(peak))).tolist()}")
    # the finite entries, on the device: the harness's spelling is the rule there as on the host
    for peak in S.PEAKS:
        t = S.table(peak)
        v = t.values[S.finite(t)]
        for mode in S.MODES:
            same(f"_quantised_dev {peak} {mode}", _quantised(dev(v), mode, float(peak)).astype(np.int64), S.rule(v, peak, mode), v)
