"""GPU: the f32 kernels every bit-equality chain of the frequency branch ends on, and the ContextBlock pooling, through the C ABI against
the per-element float64 references of tests/freq_kernel_refs.py: fcvsr_corr_lookup, fcvsr_channel_sum, fcvsr_ca_gate, fcvsr_convblk_tail,
fcvsr_convblk, fcvsr_divenh (both modes), fcvsr_divenh_apply_next (16-byte and generic path), fcvsr_gc_context, fcvsr_gc_partial_levels
(bf16 and f16) with fcvsr_gc_finish_levels and fcvsr_gc_finish, and the stage-2 entry points at the largest nparts they admit.  Inputs come
from seeded CPU generators; every comparison is made on the CPU in f64; every output a call owns is pre-filled with NaN (records that a
call owns only part of: NaN there, a sentinel elsewhere) and must hold none afterwards.

Derived bounds (corr_lookup, channel_sum, convblk_tail, u of convblk, every DivEnh output): |got - ref| <= bound at EVERY element; each
docstring records the worst |got - ref| / bound measured on an MI355X (expected below 1).
Measured bounds (behind an expf: the gate, the ConvBlk record, the ContextBlock vector): the bound is 8 x the case's OWN worst
|got - ref| / scale, found on an MI355X against the f64 reference and kept in the table below (parsed into MEASURED, one figure per case
and quantity, units of 1e-9, rounded up; run with -s for the figures of a run).  For every entry the test also asserts
8 * MEASURED < the case's rejection figure: the smallest worst |wrong - ref| / scale over the kernel's wrong variants at the same inputs
(tests/test_freq_kernel_refs_cpu.py), so that a bound which would let a dropped block pass fails by construction.

  ca_gate                                          gate
    c4 cr4 B1                                     46.13
    c4 cr4 B5                                     94.57
    c64 cr4 B1                                    33.83
    c64 cr4 B5                                    80.29
    c64 cr16 B1                                   43.90
    c64 cr16 B5                                   43.02
    c128 cr8 B1                                   18.97
    c128 cr8 B5                                   72.41
    c64 cr4 B5 neg                                 0.00
    c4 cr4 B1 neg                                  0.00
  convblk                                           rec
    K1 1x1 B3                                     24.16
    K1 5x3 B1                                     41.86
    K1 16x16 B3                                   61.98
    K1 17x15 B1                                   69.58
    K1 16x33 B3                                   72.03
    K1 33x17 B1                                   50.41
    K3 1x1 B3                                     28.11
    K3 5x3 B1                                     11.20
    K3 16x16 B3                                   14.08
    K3 17x15 B1                                   14.28
    K3 16x33 B3                                    3.02
    K3 33x17 B1                                    8.60
    K5 1x1 B3                                     18.44
    K5 5x3 B1                                      3.92
    K5 16x16 B3                                    1.09
    K5 17x15 B1                                    0.94
    K5 16x33 B3                                    0.65
    K5 33x17 B1                                    1.22
    K7 1x1 B3                                     82.81
    K7 5x3 B1                                      3.90
    K7 16x16 B3                                    0.70
    K7 17x15 B1                                    0.24
    K7 16x33 B3                                    0.54
    K7 33x17 B1                                    0.70
    K9 1x1 B3                                     36.86
    K9 5x3 B1                                      2.99
    K9 16x16 B3                                    0.55
    K9 17x15 B1                                    0.45
    K9 16x33 B3                                    1.00
    K9 33x17 B1                                    0.24
    K11 1x1 B3                                    43.92
    K11 5x3 B1                                     9.58
    K11 16x16 B3                                   0.09
    K11 17x15 B1                                   0.11
    K11 16x33 B3                                   0.15
    K11 33x17 B1                                   0.09
  gc_context                                        add
    C64 1x1x1                                      0.80
    C64 3x15x17                                    1.04
    C64 1x16x16                                    0.46
    C64 3x1x257                                    0.55
    C8 1x257x256                                   1.86
    C32 3x1x257                                    1.29
    C8 1x1x257                                     6.52
    C64 1x20x30 span                               0.24
    C64 1x20x30 last                               1.35
    C64 1x20x30 dom                                1.52
    C32 1x3x100 last                               2.58
  gc_tiles                                       levels   finish
    bf16 small L0 2x1x1                            1.40     1.40
    bf16 small L1 2x4x32                           0.71     0.71
    bf16 small L2 2x5x33                           0.59     0.59
    f16 small L0 2x1x1                             1.05     1.05
    f16 small L1 2x4x32                            0.41     0.41
    f16 small L2 2x5x33                            0.42     0.42
    bf16 mixedB L0 2x3x31                             -     0.44
    bf16 mixedB L1 1x36x929                           -     0.28
    bf16 mixedB L2 3x5x33                             -     0.46
    f16 mixedB L0 2x3x31                              -     0.56
    f16 mixedB L1 1x36x929                            -     0.29
    f16 mixedB L2 3x5x33                              -     1.02
    bf16 stress L0 2x9x70                          0.16     0.16
    bf16 stress L1 2x5x33                          0.84     0.84
    bf16 stress L2 2x3x31                          0.70     0.70
    f16 stress L0 2x9x70                           0.18     0.18
    f16 stress L1 2x5x33                           0.60     0.60
    f16 stress L2 2x3x31                           1.28     1.28
  stage2                                         levels   finish
    C64 n15232                                     3.73     8.13
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import freq_kernel_refs as R
from freq_kernel_refs import BF16, F16, F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
FACTOR = 8.0
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
ids = lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def _measured():
    """The docstring's table: {"<group> <case>": {quantity: worst ratio}}."""
    out, grp, cols = {}, None, None
    for line in __doc__.splitlines():
        m = re.match(r"  (ca_gate|convblk|gc_context|gc_tiles|stage2) +(\S.*)$", line)
        if m:
            grp, cols = m.group(1), m.group(2).split()
            continue
        m = re.match(r"    (\S.*?)  +([\d. -]+)$", line)
        if m and grp:
            out[f"{grp} {m.group(1)}"] = {c: float(v) * 1e-9 for c, v in zip(cols, m.group(2).split()) if v != "-"}
    return out


MEASURED = _measured()


def within(tag, got, ref, bound):
    """|got - ref| <= bound at every element; prints and returns the worst ratio."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    assert not bool(torch.isnan(got).any()), f"{tag}: the output holds a NaN (an element the kernel never wrote)"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[{tag}] worst |got - ref| / bound {worst:.3f}")
    bad = err > bound
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} of {bad.numel()} elements leave the bound, worst |got - ref| / bound {worst:.3f} "
                                 f"at {tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape))}")
    return worst


class Measured:
    """Collects the measured comparisons of one test: every figure is printed before anything is asserted."""

    def __init__(self):
        self.problems = []

    def check(self, group, case, qty, got, ref, scale, rejection):
        got = got.detach().double().cpu()
        assert tuple(got.shape) == tuple(ref.shape), (group, case, qty, tuple(got.shape), tuple(ref.shape))
        w = R._ratio(got - ref, scale)
        held = MEASURED.get(f"{group} {case}", {}).get(qty)
        print(f"[measured] {group} | {case} | {qty} | {w:.4e} | rejection {rejection:.3e} | table {held}")
        if bool(torch.isnan(got).any()):
            self.problems.append(f"{group} {case} {qty}: the output holds a NaN")
        elif held is None:
            self.problems.append(f"{group} {case} {qty}: no entry in the MEASURED table (this run: {w:.3e})")
        elif not FACTOR * held < rejection:
            self.problems.append(f"{group} {case} {qty}: {FACTOR:g} x measured {held:.3e} does not stay below the rejection figure {rejection:.3e}")
        elif not w <= FACTOR * held:
            self.problems.append(f"{group} {case} {qty}: worst err/scale {w:.3e} > {FACTOR:g} x measured {held:.3e}")

    def finish(self):
        assert not self.problems, "\n".join(self.problems)


def _env():
    from fcvsr_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


# ---- 1. corr_lookup -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CORR_CASES, ids=ids)
def test_corr_lookup_vs_f64_reference(case):
    """The full map (x_count = Wf) into a dense 84-channel tensor and the strip (x_count = min(Wf, 8)) into channels [4, 88) of a
    96-channel one: 81 lookup channels, three exact zeros, nothing outside the view.  measured <= 0.85"""
    hip, L, st = _env()
    B, Cn, H, Wf, ps = case
    a, b = R.corr_inputs(*case)
    ad, bd = a.cuda(), b.cuda()
    for xw, wide in ((Wf, False), (min(Wf, 8), True)):
        buf = nans(B, H, xw, 96 if wide else 84)
        dst = buf[..., 4:88] if wide else buf
        dv = hip.view(dst)
        hip.check(L.fcvsr_corr_lookup(ad.data_ptr(), bd.data_ptr(), ps, B, H, Wf, Cn, 4, xw, C.byref(dv), st), "fcvsr_corr_lookup")
        torch.cuda.synchronize()
        ref, bound = R.corr_lookup(a, b, Cn, xw)
        within(f"corr_lookup {case} x_count {xw}", dst, ref, bound)
        assert torch.equal(dst[..., 81:].cpu(), torch.zeros(B, H, xw, 3)), "channels 81..83 must be exact zeros"
        if wide:
            assert bool(torch.isnan(buf[..., :4]).all()) and bool(torch.isnan(buf[..., 88:]).all()), "written outside the view"


# ---- 2. channel_sum -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.SUM_CASES, ids=ids)
def test_channel_sum_vs_f64_reference(case):
    """A dense source and channels [2, 2 + C) of a (C + 5)-channel tensor.  measured <= 0.009 (of tau(n) * S)"""
    hip, L, st = _env()
    B, Cn, H, W = case
    x = R.sum_inputs(*case)
    ref, bound = R.channel_sum(x)
    nblk = (H * W + 255) // 256
    for wide in (False, True):
        if wide:
            buf = torch.randn(B, H, W, Cn + 5, generator=R.gen(49, *case)).cuda()
            src = buf[..., 2:2 + Cn]
            src.copy_(x)
        else:
            src = x.cuda()
        out, scratch = nans(B, Cn), nans(B * nblk * Cn)
        sv = hip.view(src)
        hip.check(L.fcvsr_channel_sum(C.byref(sv), B, H, W, out.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "fcvsr_channel_sum")
        torch.cuda.synchronize()
        assert not bool(torch.isnan(scratch).any()), "a stage-1 partial was never written"
        within(f"channel_sum {case} {'slice' if wide else 'dense'}", out, ref, bound)


# ---- 3. ca_gate -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GATE_CASES, ids=ids)
def test_ca_gate_vs_f64_reference(case):
    """(c, cr) = (4,4), (64,4), (64,16), (128,8: above the 64-thread block); B = 1 and 5; `neg`: the hidden layer all negative, the gate
    exactly 0.5.  Measured bound (module docstring)."""
    hip, L, st = _env()
    c, cr, B, neg = case
    p = R.gate_inputs(*case)
    d = {k: p[k].cuda() for k in ("sum", "w1", "w2")}
    gate = nans(B, c)
    hip.check(L.fcvsr_ca_gate(d["sum"].data_ptr(), p["inv_hw"], d["w1"].data_ptr(), d["w2"].data_ptr(), B, c, cr, gate.data_ptr(), st), "fcvsr_ca_gate")
    torch.cuda.synchronize()
    ref, scale = R.ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"])
    if neg:
        assert torch.equal(gate.cpu(), torch.full((B, c), 0.5)), "ReLU all zero: the gate must be exactly 0.5"
    m = Measured()
    m.check("ca_gate", R.gate_tag(*case), "gate", gate, ref, scale, R.gate_rejection(*case))
    m.finish()


# ---- 4. convblk_tail ------------------------------------------------------------------------------------------------------------------

def _record_prefill(own):
    """NaN where the call owns the float, the sentinel elsewhere."""
    spec = torch.full(own.shape, R.SENTINEL)
    spec[own] = NAN
    return spec.cuda()


def _record_check(tag, spec, ref, bound, own):
    got = spec.cpu()
    assert bool((got[~own] == R.SENTINEL).all()), f"{tag}: a float of the record that the call does not own was written"
    return got[own]


@pytest.mark.parametrize("case", R.TAIL_CASES, ids=ids)
def test_convblk_tail_vs_f64_reference(case):
    """ndir = 1 and 2, B = 1 and 3, HW = 1 / 255 / 257; records of 8A floats, A = 3 and 6, every g0 in [0, A): the call's 4 * ndir floats
    per pixel within the bound, every other float of the record untouched.  measured <= 0.89"""
    hip, L, st = _env()
    ndir, B, H, W = case
    p = R.tail_inputs(*case)
    d = {k: v.cuda() for k, v in p.items()}
    worst = 0.0
    for A in (3, 6):
        for g0 in range(A):
            ref, bound, own = R.convblk_tail(p["u"], p["gate"], p["sim"], B, ndir, A, g0)
            spec = _record_prefill(own)
            hip.check(L.fcvsr_convblk_tail(d["u"].data_ptr(), d["gate"].data_ptr(), d["sim"].data_ptr(), B, ndir, H, W, spec.data_ptr(),
                                           8 * A, 0, 4 * A, A, g0, st), "fcvsr_convblk_tail")
            torch.cuda.synchronize()
            tag = f"convblk_tail {case} A{A} g0 {g0}"
            worst = max(worst, within(tag, _record_check(tag, spec, ref, bound, own), ref[own], bound[own]))
    print(f"[convblk_tail {case}] worst over the records {worst:.3f}")


# ---- 5. convblk -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.CONVBLK_SHAPES, ids=ids)
@pytest.mark.parametrize("K", R.CONVBLK_K)
def test_convblk_vs_f64_reference(K, shape):
    """K = 1 ... 11 at 1 x 1, 5 x 3 (smaller than the halo), 16 x 16, 17 x 15, 16 x 33 and 33 x 17; B = 1 / 3, slopes 0.25 / 0 / -0.1.
    u_scratch against the derived bound (measured <= 0.005 of it), the spectrum record against the measured one, every float of the
    record that the call does not own untouched."""
    hip, L, st = _env()
    H, W, B, slope = shape
    p = R.convblk_inputs(K, H, W, B, slope)
    (u_ref, u_bound), (ref, scale, own) = R.convblk(p, B)
    d = {k: p[k].cuda() for k in ("x", "sim", "slope", "cw1", "cw2")}
    p1, p2 = hip.pack_conv_weight(p["w1"].cuda()), hip.pack_conv_weight(p["w2"].cuda())
    A, g0 = R.CONVBLK_A, p["g0"]
    ntile = ((H + 15) // 16) * ((W + 15) // 16)
    u, part = nans(2 * B, H, W, 4), nans(2 * B * ntile * 4)
    spec = _record_prefill(own)
    hip.check(L.fcvsr_convblk(d["x"].data_ptr(), p1.data_ptr(), p2.data_ptr(), d["slope"].data_ptr(), K, d["cw1"].data_ptr(), d["cw2"].data_ptr(),
                              d["sim"].data_ptr(), B, 2, H, W, u.data_ptr(), part.data_ptr(), part.numel(), spec.data_ptr(), 8 * A, 0, 4 * A,
                              A, g0, st), "fcvsr_convblk")
    torch.cuda.synchronize()
    tag = R.convblk_tag(K, H, W, B)
    assert not bool(torch.isnan(part).any()), "a tile's partial sum was never written"
    within(f"convblk u {tag}", u, u_ref, u_bound)
    got = _record_check(tag, spec, ref, scale, own)
    m = Measured()
    m.check("convblk", tag, "rec", got, ref[own], scale[own], R.convblk_rejection(K, H, W, B, slope))
    m.finish()


# ---- 6. DivEnh ------------------------------------------------------------------------------------------------------------------------

def _off(t, offset):
    """t on the device, `offset` floats past a 16-byte boundary."""
    if not offset:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + offset, device="cuda")
    d = buf[offset:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 * offset
    return d


@pytest.mark.parametrize("case", R.DIVENH_CASES, ids=ids)
def test_divenh_chain_kernels_vs_f64_reference(case):
    """One Q = 3 chain per case (HW = 1 / 255 / 256 / 257 / 480, B = 1 / 3; gates given).  Every call starts from the reference's stored
    running sums: fcvsr_divenh mode 0 (the sums of e1, e2; first = 1 and 0), mode 1 (s_f, s_o after each band) and
    fcvsr_divenh_apply_next (s_f, s_o and what the next step needs: next_kind 0 after bands 0 and 1, 1 after band 2) - on its 16-byte
    path (C = 64, 32), on the generic one (C = 24) and on the generic one at C = 64 with the bands 4 bytes off a 16-byte boundary.
    measured <= 0.56 (s_o), 1.00 (s_f: one addition, the bound is its half unit in the last place), 0.009 (sums)"""
    hip, L, st = _env()
    Cn, H, W, B, offset = case
    Q = R.DIVENH_Q
    p = R.divenh_inputs(Cn, H, W, B)
    res, states = R.divenh_chain(p)
    f = [_off(t, offset) for t in p["f"]]
    a, b, g1, g2 = ([t.cuda() for t in p[k]] for k in ("a", "b", "g1", "g2"))
    ms = p["mean_sum"].cuda()
    nblk = (H * W + 255) // 256
    tag = f"divenh {case}"
    for i in range(Q):
        first = 1 if i == 0 else 0

        def state():
            """The running sums the call reads; the first band only writes them."""
            if first:
                return nans(B, H, W, Cn), nans(B, H, W, Cn)
            return states[i - 1][0].float().cuda(), states[i - 1][1].float().cuda()

        # mode 0
        s_f, s_o = state()
        sums, scratch = nans(2, B, Cn), nans(2 * B * nblk * Cn)
        hip.check(L.fcvsr_divenh(0, first, f[i].data_ptr(), s_f.data_ptr(), s_o.data_ptr(), a[i].data_ptr(), b[i].data_ptr(), ms.data_ptr(),
                                 p["inv_hw"], None, None, sums.data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W, Cn, st), "fcvsr_divenh(0)")
        torch.cuda.synchronize()
        assert not bool(torch.isnan(scratch).any()), "a stage-1 partial was never written"
        within(f"{tag} mode 0 band {i}", sums, *res[f"e{i}"])
        # mode 1
        s_f, s_o = state()
        hip.check(L.fcvsr_divenh(1, first, f[i].data_ptr(), s_f.data_ptr(), s_o.data_ptr(), a[i].data_ptr(), b[i].data_ptr(), ms.data_ptr(),
                                 p["inv_hw"], g1[i].data_ptr(), g2[i].data_ptr(), None, None, 0, B, H, W, Cn, st), "fcvsr_divenh(1)")
        torch.cuda.synchronize()
        within(f"{tag} mode 1 band {i} s_f", s_f, *res[f"sf{i}"])
        within(f"{tag} mode 1 band {i} s_o", s_o, *res[f"so{i}"])
        # apply_next
        s_f, s_o = state()
        sums, scratch = nans(2, B, Cn), nans(2 * B * nblk * Cn)
        nxt = i + 1 < Q
        hip.check(L.fcvsr_divenh_apply_next(first, f[i].data_ptr(), s_f.data_ptr(), s_o.data_ptr(), a[i].data_ptr(), b[i].data_ptr(),
                                            ms.data_ptr(), p["inv_hw"], g1[i].data_ptr(), g2[i].data_ptr(),
                                            f[i + 1].data_ptr() if nxt else None, a[i + 1].data_ptr() if nxt else None,
                                            b[i + 1].data_ptr() if nxt else None, sums.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                            B, H, W, Cn, st), "fcvsr_divenh_apply_next")
        torch.cuda.synchronize()
        assert not bool(torch.isnan(scratch).any()), "a stage-1 partial was never written"
        within(f"{tag} apply_next band {i} s_f", s_f, *res[f"sf{i}"])
        within(f"{tag} apply_next band {i} s_o", s_o, *res[f"so{i}"])
        within(f"{tag} apply_next band {i} sums", sums, *res[f"nx{i}"])


# ---- 7. ContextBlock pooling ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GC_CASES, ids=ids)
def test_gc_context_vs_f64_reference(case):
    """f32 r: HW = 1 / 255 / 256 / 257, 257 x 256 (nblk = 257 > the 256 threads of stage 2), C = 64 / 32 / 8, B = 1 / 3; the stress
    inputs (logits spanning 80 over the blocks; the maximum at the last live pixel of a partial block; one pixel dominating).
    Measured bound (module docstring)."""
    hip, L, st = _env()
    B, Cn, H, W, stress = case
    p = R.gc_inputs(B, Cn, H, W, stress, R.block_partition)
    d = {k: v.cuda() for k, v in p.items()}
    nblk = (H * W + 255) // 256
    add, scratch = nans(B, Cn), nans(B * nblk * (Cn + 2))
    hip.check(L.fcvsr_gc_context(d["r"].data_ptr(), d["wmask"].data_ptr(), d["w1"].data_ptr(), d["w2"].data_ptr(), B, H, W, Cn, add.data_ptr(),
                                 scratch.data_ptr(), scratch.numel(), st), "fcvsr_gc_context")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(scratch).any()), "a stage-1 partial was never written"
    ref, scale = R.gc_context(p, R.block_partition)
    m = Measured()
    m.check("gc_context", R.gc_tag(*case), "add", add, ref, scale, R.gc_rejection(p, R.block_partition, stress))
    m.finish()


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(R.GC_TILE_SETS))
def test_gc_tile_partials_vs_f64_reference(name, dt):
    """fcvsr_gc_partial_levels on a stored 16-bit r, three levels in one launch (1 x 1, 4 x 32, 5 x 33; 3 x 31, 36 x 929 = 270 tiles,
    5 x 33 with B = 2 / 1 / 3; the stress inputs), finished by fcvsr_gc_finish per level and, where the levels share B, by
    fcvsr_gc_finish_levels; the reference is evaluated on the stored 16-bit values.  Measured bound (module docstring)."""
    hip, L, st = _env()
    levels = R.GC_TILE_SETS[name]
    n = 64
    ps = R.gc_tile_inputs(name, dt)
    wm, w1, w2 = ps[0]["wmask"].cuda(), ps[0]["w1"].cuda(), ps[0]["w2"].cuda()           # shared by the levels, as in BlockRCB
    rs = [p["r"].cuda() for p in ps]
    nparts = [((H + 3) // 4) * ((W + 31) // 32) for _, H, W, _ in levels]
    parts = [nans(B, npt, n + 2) for (B, _, _, _), npt in zip(levels, nparts)]
    pl = (hip.GcPartialLevel * 3)()
    for l, (B, H, W, _) in enumerate(levels):
        pl[l].r, pl[l].partial, pl[l].B, pl[l].H, pl[l].W = rs[l].data_ptr(), parts[l].data_ptr(), B, H, W
    hip.check(L.fcvsr_gc_partial_levels(pl, 3, hip.BF16 if dt == BF16 else hip.F16, wm.data_ptr(), n, st), "fcvsr_gc_partial_levels")
    torch.cuda.synchronize()
    for l in range(3):
        assert not bool(torch.isnan(parts[l]).any()), f"level {l}: a tile's partial was never written"
    same_b = len({lv[0] for lv in levels}) == 1
    adds_lv = [nans(lv[0], n) for lv in levels]
    if same_b:
        fl = (hip.GcFinishLevel * 3)()
        for l in range(3):
            fl[l].partial, fl[l].add, fl[l].nparts = parts[l].data_ptr(), adds_lv[l].data_ptr(), nparts[l]
        hip.check(L.fcvsr_gc_finish_levels(fl, 3, w1.data_ptr(), w2.data_ptr(), levels[0][0], n, st), "fcvsr_gc_finish_levels")
    adds = [nans(lv[0], n) for lv in levels]
    for l, (B, _, _, _) in enumerate(levels):
        hip.check(L.fcvsr_gc_finish(parts[l].data_ptr(), nparts[l], w1.data_ptr(), w2.data_ptr(), B, n, adds[l].data_ptr(), st), "fcvsr_gc_finish")
    torch.cuda.synchronize()
    m = Measured()
    for l, (B, H, W, stress) in enumerate(levels):
        ref, scale = R.gc_context(ps[l], R.tile_partition)
        rej = R.gc_rejection(ps[l], R.tile_partition, stress)
        case = f"{IDS[dt]} {name} L{l} {B}x{H}x{W}"
        if same_b:
            m.check("gc_tiles", case, "levels", adds_lv[l], ref, scale, rej)
        m.check("gc_tiles", case, "finish", adds[l], ref, scale, rej)
    m.finish()


# ---- the stage-2 entry points at the largest nparts they admit -----------------------------------------------------------------------------

def test_gc_stage2_at_the_largest_admitted_nparts():
    """The entry points admit (2C + nparts) * 4 <= 60 KiB of dynamic shared memory; gc_stage2_levels_kernel adds 5 KiB of static arrays,
    gc_stage2_kernel 1 KiB: 65 KiB and 61 KiB per workgroup.  A gfx950 workgroup may hold all 160 KiB of a CU's LDS, and the device
    reports that as its per-block limit, so the largest admitted size launches; the test works the sum out against the reported limit
    BEFORE it launches, then runs C = 64, nparts = 15232 (4 MB of synthetic one-pixel partials) through both entry points.  One more
    partial is refused with -1."""
    hip, L, st = _env()
    Cn = 64
    n = R.stage2_max_nparts(Cn)
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    need = {k: R.STAGE2_DYNAMIC_LIMIT + v for k, v in R.STAGE2_STATIC.items()}
    print(f"[stage2] per-block shared memory limit {limit}, needed {need}")
    assert all(v <= limit for v in need.values()), f"the largest admitted nparts cannot launch: {need} > {limit}; the argument check must refuse it"
    p = R.stage2_inputs(Cn, n)
    parts, w1, w2 = p["parts"].cuda(), p["w1"].cuda(), p["w2"].cuda()
    add_l, add_f = nans(1, Cn), nans(1, Cn)
    fl = (hip.GcFinishLevel * 3)()
    fl[0].partial, fl[0].add, fl[0].nparts = parts.data_ptr(), add_l.data_ptr(), n
    hip.check(L.fcvsr_gc_finish_levels(fl, 1, w1.data_ptr(), w2.data_ptr(), 1, Cn, st), "fcvsr_gc_finish_levels")
    hip.check(L.fcvsr_gc_finish(parts.data_ptr(), n, w1.data_ptr(), w2.data_ptr(), 1, Cn, add_f.data_ptr(), st), "fcvsr_gc_finish")
    torch.cuda.synchronize()
    ref, scale = R.stage2_reference(p)
    rej = R._ratio(R.stage2_reference(p, drop_last=True)[0] - ref, scale)
    m = Measured()
    m.check("stage2", f"C{Cn} n{n}", "levels", add_l, ref, scale, rej)
    m.check("stage2", f"C{Cn} n{n}", "finish", add_f, ref, scale, rej)
    m.finish()
    fl[0].nparts = n + 1
    assert L.fcvsr_gc_finish_levels(fl, 1, w1.data_ptr(), w2.data_ptr(), 1, Cn, st) == -1
    assert L.fcvsr_gc_finish(parts.data_ptr(), n + 1, w1.data_ptr(), w2.data_ptr(), 1, Cn, add_f.data_ptr(), st) == -1
