"""GPU: fcvsr_freq_mlp3, fcvsr_freq_head (all four instantiations) and fcvsr_convcorr_strip against the rounded-operand f64 references of
tests/freq_fused_refs.py, per element, through the C ABI only.  Every output lies in a buffer filled with a quiet-NaN bit pattern no
kernel produces, 64 elements longer than the tensor: what the kernel owns must come back finite and within `bound` of `ref`; what it
does not own - the spare halfwords of a wide mlp3 destination, the columns >= xs of the strip's grid, the tail of the buffer - must
hold the pattern bit for bit.  The comparison runs on the CPU in f64.

  test_mlp3_*      six pixel counts around the 128-pixel tile and the group of 8 tiles, one and two directions, the engine's three
                   separate stride-128 spectra and slices of one stride-384 record, destination strides 128 and 136, the four input
                   sets of the references (values beyond the f16 range; xa ~ xb; the residual in isolation).
  test_head_*      <f32|bf16> x <NHID 1|2> at 1, 127, 128, 129, 414 pixels; f32 at stride 128 and at channel offset 128 of stride 384;
                   bf16 at strides 128 and 256; spectrum-sized values on the f32 source.
  test_strip_*     B x H x (Wf, xs) with a lookup tensor of its own whose pad channels are non-zero.
  test_engine_*    the engine's sequence - lookup on the strip, head on `off` over the grid, strip in place - against the f64 convcorr on
                   [off | full-width f64 lookup] over the whole grid.
  test_*_rejects_* the entry points refuse bad arguments on the host, launch nothing and leave the output as it was.

No tolerance here is taken from a kernel's output: tests/test_freq_fused_refs_cpu.py shows, without a GPU, that every bound accepts a
correct f32 evaluation and rejects the wrong kernels at these very shapes and inputs.  Run with -s for the figures of a run (RATIO
lines per case, WORST per kernel and input set at the end).  Worst |got - ref| / bound measured on an MI355X - records, not thresholds:

  kernel                      normal    spectrum  near      w4zero
  fcvsr_freq_mlp3             0.8540    0.7929    0.7739    0.9897
  fcvsr_freq_head f32 NHID=1  0.0893    0.0057    -         -
  fcvsr_freq_head f32 NHID=2  0.0009    0.0020    -         -
  fcvsr_freq_head bf16 NHID=1 0.0285    -         -         -
  fcvsr_freq_head bf16 NHID=2 0.0587    -         -         -
  fcvsr_convcorr_strip        0.2166    -         -         -
  engine decomposition        0.0019    -         -         -
mlp3's figures are those of its bf16 store (half a last place of the result is the bound's largest term; `w4zero` leaves nothing else).
"""
import ctypes as C

import pytest
import torch

import freq_fused_refs as R
from infer_kernel_refs import BF16, F32

pytestmark = pytest.mark.gpu

INT_OF = {F32: torch.int32, BF16: torch.int16}
SENTINEL = {F32: 0x7FC12345, BF16: 0x7FC1}                   # quiet NaNs with a payload no kernel produces
GUARD = 64
WORST = {}
P2 = C.c_void_p * 2
ids = lambda c: "-".join(str(v) for v in c)


def _filled(numel, dt):
    """(bits, values): `numel` + GUARD elements of dt, every one the sentinel; two views of one buffer."""
    bits = torch.full((numel + GUARD,), SENTINEL[dt], dtype=INT_OF[dt], device="cuda")
    return bits, bits.view(dt)


def _is_sentinel(bits, dt):
    return bool((bits.cpu() == SENTINEL[dt]).all())


def _check(kernel, name, what, got, ref, bound):
    got = got.double().cpu()
    assert not bool(torch.isnan(got).any()), f"{kernel} {what}: {int(torch.isnan(got).sum())} elements were never written"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    WORST[(kernel, name)] = max(WORST.get((kernel, name), 0.0), worst)
    print(f"RATIO\t{kernel}\t{name}\t{what}\t{worst:.4f}")
    assert bool((err <= bound).all()), f"{kernel} {what}: worst err / bound {worst:.3f}"


def _weights(*ws):
    return [None if w is None else R.pack(w).cuda() for w in ws]


# ---- fcvsr_freq_mlp3 --------------------------------------------------------------------------------------------------------------------

def _mlp3_sources(p, layout):
    """(x1, x2, x3, pixel stride): device tensors (npix, 128) f32 at that stride."""
    xs = [p[k].reshape(-1, 128) for k in ("x1", "x2", "x3")]
    if layout == "separate":
        return [x.contiguous().cuda() for x in xs] + [128]
    rec = torch.cat(xs, 1).contiguous().cuda()
    return [rec[:, :128], rec[:, 128:256], rec[:, 256:], 384]


@pytest.mark.parametrize("case", R.MLP3_CASES, ids=ids)
def test_mlp3_vs_f64_reference(case):
    from fcvsr_amd import hip
    B, H, Wf, nd, layout, dsx, name = case
    p = R.mlp3_inputs(*case)
    ref, bound = R.mlp3_ref(p, nd)
    npix = B * H * Wf
    x1, x2, x3, sx = _mlp3_sources(p, layout)
    w0, w2, w4 = _weights(p["W0"], p["W2"], p["W4"])
    bits, vals = _filled(nd * npix * dsx, BF16)
    out = vals[:nd * npix * dsx].view(nd, npix, dsx)
    hip.check(hip.lib().fcvsr_freq_mlp3(P2(x1.data_ptr(), x3.data_ptr()), P2(x2.data_ptr(), x2.data_ptr()), nd, sx, npix, w0.data_ptr(),
                                        w2.data_ptr(), w4.data_ptr(), P2(out[0].data_ptr(), out[nd - 1].data_ptr()), dsx,
                                        hip.stream_ptr()), "fcvsr_freq_mlp3")
    torch.cuda.synchronize()
    _check("fcvsr_freq_mlp3", name, ids(case), out[..., :128], ref, bound)
    spare = bits[:nd * npix * dsx].view(nd, npix, dsx)[..., 128:]
    assert _is_sentinel(spare, BF16) and _is_sentinel(bits[nd * npix * dsx:], BF16), "a write outside the 128 channels of a pixel"


# ---- fcvsr_freq_head --------------------------------------------------------------------------------------------------------------------

def _head_launch(hip, x_ptr, code, stride, npix, w0, wmid, wl, out_ptr):
    return hip.lib().fcvsr_freq_head(x_ptr, code, stride, npix, w0.data_ptr(), None if wmid is None else wmid.data_ptr(), wl.data_ptr(),
                                     out_ptr, hip.stream_ptr())


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_tag)
def test_head_vs_f64_reference(case):
    from fcvsr_amd import hip
    dt, nhid, npix, stride, name = case
    p = R.head_inputs(*case)
    ref, bound = R.head_ref(p)
    rec = p["rec"].contiguous().cuda()
    w0, wmid, wl = _weights(p["W0"], p["Wmid"], p["Wl"])
    bits, vals = _filled(npix * 4, F32)
    hip.check(_head_launch(hip, rec.data_ptr() + p["off"] * rec.element_size(), hip.F32 if dt == F32 else hip.BF16, stride, npix, w0, wmid,
                           wl, vals.data_ptr()), "fcvsr_freq_head")
    torch.cuda.synchronize()
    _check(f"fcvsr_freq_head {'f32' if dt == F32 else 'bf16'} NHID={nhid}", name, R.head_tag(case), vals[:npix * 4].view(npix, 4), ref, bound)
    assert _is_sentinel(bits[npix * 4:], F32), "a write past the last pixel"


# ---- fcvsr_convcorr_strip ---------------------------------------------------------------------------------------------------------------

def _strip_launch(hip, off, corr, B, H, Wf, xs, w0, w2, w4, out_ptr):
    return hip.lib().fcvsr_convcorr_strip(off.data_ptr(), corr.data_ptr(), B, H, Wf, xs, w0.data_ptr(), w2.data_ptr(), w4.data_ptr(), out_ptr,
                                          hip.stream_ptr())


@pytest.mark.parametrize("case", R.STRIP_CASES, ids=ids)
def test_strip_vs_f64_reference(case):
    from fcvsr_amd import hip
    B, H, Wf, xs = case
    p = R.strip_inputs(*case)
    ref, bound = R.strip_ref(p, case)
    n = 2 * B * H * Wf * 4
    bits, vals = _filled(n, F32)
    w0, w2, w4 = _weights(p["W0"], p["W2"], p["W4"])
    hip.check(_strip_launch(hip, p["off"].cuda(), p["corr"].cuda(), B, H, Wf, xs, w0, w2, w4, vals.data_ptr()), "fcvsr_convcorr_strip")
    torch.cuda.synchronize()
    out = vals[:n].view(2 * B, H, Wf, 4)
    _check("fcvsr_convcorr_strip", "normal", ids(case), out[:, :, :xs], ref[:, :, :xs], bound[:, :, :xs])
    assert _is_sentinel(bits[:n].view(2 * B, H, Wf, 4)[:, :, xs:], F32), "columns >= xs must be left untouched"
    assert _is_sentinel(bits[n:], F32)


# ---- the engine's decomposition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.COMPOSE_CASES, ids=ids)
def test_engine_strip_decomposition_vs_full_f64_convcorr(case):
    from fcvsr_amd import hip
    B, H, Wf = case
    xs = min(Wf, 8)
    p = R.compose_inputs(*case)
    ref, bound = R.convcorr_full(p)
    x1f, x2f, off = p["x1f"].cuda(), p["x2f"].cuda(), p["off"].cuda()
    w0, w0off, w2, w4 = _weights(p["W0"], p["W0"][:, :128], p["W2"], p["W4"])
    cbits, cvals = _filled(B * H * xs * 84, F32)
    corr = cvals[:B * H * xs * 84].view(B, H, xs, 84)
    cv = hip.view(corr)
    st = hip.stream_ptr()
    hip.check(hip.lib().fcvsr_corr_lookup(x1f.data_ptr(), x2f.data_ptr(), 128, B, H, Wf, 128, 4, xs, C.byref(cv), st), "fcvsr_corr_lookup")
    n = 2 * B * H * Wf * 4
    bits, vals = _filled(n, F32)
    hip.check(_head_launch(hip, off.data_ptr(), hip.BF16, 128, 2 * B * H * Wf, w0off, w2, w4, vals.data_ptr()), "fcvsr_freq_head")
    hip.check(_strip_launch(hip, off, corr, B, H, Wf, xs, w0, w2, w4, vals.data_ptr()), "fcvsr_convcorr_strip")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(corr).any()) and float(corr.abs().max()) > 0.0 and _is_sentinel(cbits[B * H * xs * 84:], F32)
    _check("engine decomposition", "normal", ids(case), vals[:n].view(2 * B, H, Wf, 4), ref, bound)
    assert _is_sentinel(bits[n:], F32)


# ---- argument rejection: refused on the host, nothing launched --------------------------------------------------------------------------

def test_mlp3_rejects_bad_arguments():
    from fcvsr_amd import hip
    L = hip.lib()
    npix = 129
    x = torch.zeros(3, npix, 136, device="cuda")
    w0, w2, w4 = _weights(torch.zeros(128, 256), torch.zeros(128, 128), torch.zeros(128, 128))
    bits, vals = _filled(2 * npix * 136, BF16)
    o0, o1 = vals.data_ptr(), vals.data_ptr() + npix * 136 * 2
    xa, xb, dst = (x[0].data_ptr(), x[2].data_ptr()), (x[1].data_ptr(), x[1].data_ptr()), (o0, o1)
    ok = dict(xa=xa, xb=xb, nd=2, sx=136, npix=npix, w0=w0.data_ptr(), w2=w2.data_ptr(), w4=w4.data_ptr(), dst=dst, dsx=136)
    # a SOURCE stride of 132 floats is legal (16-byte pixels: a multiple of 4 floats); 132 halfwords of destination are not (8)
    bad = [("null xa", dict(xa=None)), ("null xb", dict(xb=None)), ("null dst", dict(dst=None)), ("null w2", dict(w2=None)),
           ("null xa[1]", dict(xa=(xa[0], None))), ("null dst[0]", dict(dst=(None, o1))),
           ("n_dirs 3", dict(nd=3)), ("n_dirs 0", dict(nd=0)),
           ("src stride 100", dict(sx=100)), ("dst stride 100", dict(dsx=100)), ("dst stride 132", dict(dsx=132)),
           ("xa + 8 bytes", dict(xa=(xa[0] + 8, xa[1]))), ("xb + 8 bytes", dict(xb=(xb[0], xb[1] + 8))), ("dst + 8 bytes", dict(dst=(o0 + 8, o1))),
           ("w0 + 8 bytes", dict(w0=w0.data_ptr() + 8)), ("w4 + 8 bytes", dict(w4=w4.data_ptr() + 8)),
           ("npix 0", dict(npix=0)), ("2^32 bytes of source", dict(npix=1 << 23, sx=128, dsx=128))]
    assert (1 << 23) * 128 * 4 == 1 << 32
    for what, change in bad:
        a = dict(ok, **change)
        arr = lambda v: None if v is None else P2(*v)
        rc = L.fcvsr_freq_mlp3(arr(a["xa"]), arr(a["xb"]), a["nd"], a["sx"], a["npix"], a["w0"], a["w2"], a["w4"], arr(a["dst"]), a["dsx"],
                               hip.stream_ptr())
        assert rc != 0, f"fcvsr_freq_mlp3 accepted: {what}"
    torch.cuda.synchronize()
    assert _is_sentinel(bits, BF16)


def test_head_rejects_bad_arguments():
    from fcvsr_amd import hip
    L = hip.lib()
    npix = 129
    x = torch.zeros(npix, 136, device="cuda")                # wide enough for every stride tried, in either dtype
    w0, wm, wl = _weights(torch.zeros(64, 128), torch.zeros(64, 64), torch.zeros(4, 64))
    bits, vals = _filled(npix * 4 + 4, F32)
    ok = dict(x=x.data_ptr(), dt=hip.F32, sx=136, npix=npix, w0=w0.data_ptr(), wm=wm.data_ptr(), wl=wl.data_ptr(), out=vals.data_ptr())
    bad = [("null x", dict(x=None)), ("null w0", dict(w0=None)), ("null w_last", dict(wl=None)), ("null out", dict(out=None)),
           ("stride 100", dict(sx=100)), ("stride 132", dict(sx=132)), ("bf16 stride 100", dict(sx=100, dt=hip.BF16)),
           ("bf16 stride 132", dict(sx=132, dt=hip.BF16)), ("x + 8 bytes", dict(x=x.data_ptr() + 8)), ("out + 8 bytes", dict(out=vals.data_ptr() + 8)),
           ("w_mid + 8 bytes", dict(wm=wm.data_ptr() + 8)), ("x_dtype f16", dict(dt=hip.F16)), ("x_dtype u8", dict(dt=hip.U8)),
           ("npix 0", dict(npix=0)), ("npix 2^30", dict(npix=1 << 30))]
    for what, change in bad:
        a = dict(ok, **change)
        rc = L.fcvsr_freq_head(a["x"], a["dt"], a["sx"], a["npix"], a["w0"], a["wm"], a["wl"], a["out"], hip.stream_ptr())
        assert rc != 0, f"fcvsr_freq_head accepted: {what}"
    torch.cuda.synchronize()
    assert _is_sentinel(bits, F32)


def test_strip_rejects_bad_arguments():
    from fcvsr_amd import hip
    L = hip.lib()
    B, H, Wf, xs = 1, 5, 19, 8
    off = torch.zeros(2 * B, H, Wf, 128, dtype=BF16, device="cuda")
    corr = torch.zeros(B * H * Wf * 84 + 4, device="cuda")   # a lookup of the full width: whatever xs a call names
    w0, w2, w4 = _weights(torch.zeros(64, 209), torch.zeros(64, 64), torch.zeros(4, 64))
    bits, vals = _filled(2 * B * H * Wf * 4 + 4, F32)
    ok = dict(off=off.data_ptr(), corr=corr.data_ptr(), B=B, H=H, Wf=Wf, xs=xs, w0=w0.data_ptr(), w2=w2.data_ptr(), w4=w4.data_ptr(),
              out=vals.data_ptr())
    bad = [("null off", dict(off=None)), ("null corr", dict(corr=None)), ("null w_mid", dict(w2=None)), ("null off4", dict(out=None)),
           ("xs > Wf", dict(xs=Wf + 1)), ("xs 0", dict(xs=0)), ("B 0", dict(B=0)), ("H -1", dict(H=-1)),
           ("off + 8 bytes", dict(off=off.data_ptr() + 8)), ("corr + 8 bytes", dict(corr=corr.data_ptr() + 8)),
           ("off4 + 8 bytes", dict(out=vals.data_ptr() + 8)), ("w0 + 8 bytes", dict(w0=w0.data_ptr() + 8))]
    for what, change in bad:
        a = dict(ok, **change)
        rc = L.fcvsr_convcorr_strip(a["off"], a["corr"], a["B"], a["H"], a["Wf"], a["xs"], a["w0"], a["w2"], a["w4"], a["out"], hip.stream_ptr())
        assert rc != 0, f"fcvsr_convcorr_strip accepted: {what}"
    torch.cuda.synchronize()
    assert _is_sentinel(bits, F32)


@pytest.fixture(scope="module", autouse=True)
def worst_figures():
    """-s: the worst err / bound per kernel and input set of this run (the table of the module docstring), after the last test."""
    yield
    for (kernel, name), v in sorted(WORST.items()):
        print(f"WORST\t{kernel}\t{name}\t{v:.4f}")
