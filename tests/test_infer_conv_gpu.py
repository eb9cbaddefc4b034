"""GPU: every inference convolution path against the rounded-operand f64 reference of tests/infer_conv_refs.py, per element.

(a) + (b)  fcvsr_conv2d_mfma: every problem of tests/golden/conv_plan_table.json that is not rejected, once per distinct kernel string
           it reaches over the six policies, and the edge shapes the table does not have (infer_conv_refs.edge_cases / gc_cases).
           Every destination (and every ContextBlock partial) lives inside a larger NaN-filled buffer at the recorded strides and
           offset; the launch goes through hip.conv2d_mfma under the case's policy; fcvsr_last_conv_kernel() must EQUAL the declared
           string; every destination element must be within `bound`; every buffer element outside the view must still hold the
           sentinel's bits.  ContextBlock fusion: lse_T and mu_T per 4 x 32 tile, every partial written, and the `add` vector of
           fcvsr_gc_finish_levels against the f64 formula on the unrounded y.
(c)        the exact-f32 family (fcvsr_conv2d, fcvsr_conv2d_f32mfma) against the unrounded reference with tau(n) * S.
(d)        fcvsr_conv_last per element; its _u8 / _u16 forms equal the quantised f32 result exactly.
(e)        one eager forward of every model configuration under hip.PROFILE: each kernel string the engine launches is declared by a
           case of this module.

No tolerance here is taken from a kernel's output: tests/test_infer_conv_refs_cpu.py shows, without a GPU, that every bound accepts
an f32 evaluation and rejects the wrong variants at these very shapes and inputs.  Run with -s for the worst err / bound per kernel."""
import ctypes as C

import pytest
import torch

import infer_conv_refs as R
from infer_kernel_refs import BF16, F16, F32, quantise

pytestmark = pytest.mark.gpu

MFMA = R.mfma_cases()
F32C = R.f32_cases()
INT_OF = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
SENTINEL = {F32: 0x7FC12345, BF16: 0x7FC1, F16: 0x7E01}      # quiet NaNs with a payload no kernel produces
WORST = {}


def _buffer(spec, dt, sentinel):
    """(buffer, view): the tensor of `spec` inside a buffer 64 elements longer than its extent, sentinel- or zero-filled."""
    extent = spec["offset"] + 1 + sum((n - 1) * s for n, s in zip(spec["shape"], spec["strides"]))
    buf = torch.zeros(extent + 64, dtype=dt, device="cuda")
    if sentinel:
        buf.view(INT_OF[dt]).fill_(SENTINEL[dt])
    return buf, buf.as_strided(spec["shape"], spec["strides"], spec["offset"])


def _place(values, spec):
    buf, v = _buffer(spec, values.dtype, False)
    v.copy_(values)
    return v


def _untouched(buf, spec, dt):
    """Every element of the buffer outside the view still holds the sentinel, bit for bit."""
    idx = torch.full((1,), spec["offset"], dtype=torch.long)
    for n, s in zip(spec["shape"], spec["strides"]):
        idx = (idx[:, None] + torch.arange(n) * s).reshape(-1)
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    outside[idx] = False
    return bool((buf.view(INT_OF[dt]).cpu()[outside] == SENTINEL[dt]).all())


def _policy(monkeypatch, lean, res):
    for var, val in (("FCVSR_MFMA_LEAN", lean), ("FCVSR_MFMA_RES", res)):
        if val == "unset":
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def _check(kernel, what, got, ref, bound):
    err = (got.double().cpu() - ref.double()).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"RATIO\t{kernel}\t{what}\t{worst:.4f}")
    assert bool((err <= bound).all()), f"{kernel} {what}: worst err / bound {worst:.3f}"


@pytest.mark.parametrize("c", MFMA, ids=lambda c: c["id"])
def test_conv2d_mfma_vs_f64_reference(c, monkeypatch):
    from fcvsr_amd import hip
    p = c["problem"]
    inp = R.make_inputs(p)
    refs = (R.gc_ref if p["gc"] else R.conv_ref)(p, inp)
    dt = R.DT[p["mma"]]
    ps, cout = p["pixel_shuffle"], p["cout"]
    wp = hip.pack_conv_weight_mfma(inp["w"].cuda(), dt, ps=ps)
    bias = inp["bias"]
    if bias is not None:
        bias = (bias[hip.ps_order(cout)] if ps else bias).contiguous().cuda()
    slope_t = None if inp["slope_t"] is None else inp["slope_t"].cuda()
    wmask = inp["wmask"].contiguous().cuda() if p["gc"] else None
    groups, held = [], []
    for gs, gi in zip(p["groups"], inp["groups"]):
        dbuf, dst = _buffer(gs["dst"], R.DT[gs["dst"]["dtype"]], True)
        G = dict(srcs=[_place(v, s) for v, s in zip(gi["srcs"], gs["srcs"])], res=[_place(v, s) for v, s in zip(gi["res"], gs["res"])],
                 dst=dst, ps=ps)
        pbuf = None
        if p["gc"]:
            B, H, W, _ = gs["srcs"][0]["shape"]
            nparts = ((H + 3) // 4) * ((W + 31) // 32)
            pspec = R.T((B, nparts, 1, cout + 2), "f32", offset=32)
            pbuf, pv = _buffer(pspec, F32, True)
            G["gc_partial"] = pv
            held.append((pbuf, pspec, pv, nparts))
        groups.append(G)
        held.append((dbuf, gs["dst"]))
    _policy(monkeypatch, c["lean"], c["res"])
    hip.conv2d_mfma(groups, wp, p["ksize"], cout, hip.BF16 if dt == BF16 else hip.F16, stride=p["stride"], bias=bias, act=p["act"],
                    slope=p["slope"], slope_t=slope_t, res_scale=p["res_scale"], pixel_shuffle=ps, gc_wmask=wmask)
    torch.cuda.synchronize()
    kernel = hip.lib().fcvsr_last_conv_kernel().decode()
    assert kernel == c["kernel"]
    for l, (gs, G, r) in enumerate(zip(p["groups"], groups, refs)):
        _check(kernel, f"{c['id']} L{l}", G["dst"], r["ref"], r["bound"])
    for h in held:
        assert _untouched(h[0], h[1], F32 if len(h) == 4 else R.DT[h[1]["dtype"]]), f"{kernel}: a write outside the view"
    if p["gc"]:
        parts = [h for h in held if len(h) == 4]
        B = p["groups"][0]["srcs"][0]["shape"][0]
        adds = [torch.full((B, cout), float("nan"), device="cuda") for _ in parts]
        for l, ((_, _, pv, nparts), r) in enumerate(zip(parts, refs)):
            part = pv.reshape(B, nparts, cout + 2).double().cpu()
            assert bool(torch.isfinite(part).all()), f"{kernel}: a partial of level {l} was not written"
            acc, m, s = part[..., :cout], part[..., cout], part[..., cout + 1]
            t = r["tiles"]
            _check(kernel + " lse", f"{c['id']} L{l}", m + torch.log(s), t["lse"], t["b_lse"])
            _check(kernel + " mu", f"{c['id']} L{l}", acc / s[..., None], t["mu"], t["b_mu"])
        fl = (hip.GcFinishLevel * len(parts))()
        for l, (_, _, pv, nparts) in enumerate(parts):
            fl[l].partial, fl[l].add, fl[l].nparts = pv.data_ptr(), adds[l].data_ptr(), nparts
        w1, w2 = inp["w1"].contiguous().cuda(), inp["w2"].contiguous().cuda()
        hip.check(hip.lib().fcvsr_gc_finish_levels(fl, len(parts), w1.data_ptr(), w2.data_ptr(), B, cout, hip.stream_ptr()), "gc_finish_levels")
        torch.cuda.synchronize()
        for l, r in enumerate(refs):
            _check(kernel + " add", f"{c['id']} L{l}", adds[l], r["add"], r["b_add"])


# ---- (c) the exact-f32 family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", F32C, ids=lambda c: c["id"])
def test_exact_f32_family_vs_f64_reference(c):
    from fcvsr_amd import hip
    p = c["problem"]
    inp = R.make_inputs(p)
    ref = R.conv_ref(p, inp)[0]
    gs, gi = p["groups"][0], inp["groups"][0]
    k, cout, ps = p["ksize"], p["cout"], p["pixel_shuffle"]
    dbuf, dst = _buffer(gs["dst"], F32, True)
    srcs = [_place(v, s) for v, s in zip(gi["srcs"], gs["srcs"])]
    if p.get("res_is_dst"):
        dst.copy_(gi["res"][0])
        res = [dst]
    else:
        res = [_place(v, s) for v, s in zip(gi["res"], gs["res"])]
    w, bias = inp["w"].cuda(), inp["bias"].cuda()
    slope_t = None if inp["slope_t"] is None else inp["slope_t"].cuda()
    if c["entry"] == "direct":
        hip.conv2d(srcs, hip.pack_conv_weight(w), k, cout, dst, bias=bias, stride=p["stride"], act=p["act"], slope=p["slope"],
                   slope_t=slope_t, res=res, res_scale=p["res_scale"], pixel_shuffle=ps)
        kernel = "fcvsr_conv2d"
    else:
        wm = hip.pack_conv_weight_f32mfma(w, ps=ps)
        bm = bias[hip.ps_order(cout).cuda()].contiguous() if ps else bias
        d = hip.ConvDesc()
        hip._fill_desc(d, srcs, wm, k, cout, wm.shape[1], dst, bm, 1, p["act"], p["slope"], slope_t, res, p["res_scale"], ps)
        assert hip.lib().fcvsr_conv2d_f32mfma_eligible(C.byref(d)) == 1
        hip.check(hip.lib().fcvsr_conv2d_f32mfma(C.byref(d), hip.stream_ptr()), "fcvsr_conv2d_f32mfma")
        kernel = "fcvsr_conv2d_f32mfma " + ("ps" if ps else "generic" if p.get("res_is_dst") else "vector")
    torch.cuda.synchronize()
    _check(kernel, c["id"], dst, ref["ref"], ref["bound"])
    assert _untouched(dbuf, gs["dst"], F32), f"{kernel}: a write outside the view"


# ---- (d) fcvsr_conv_last ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CONV_LAST_CASES, ids=lambda c: f"c{c[0]}-{str(c[1])[6:]}-{c[3]}x{c[4]}")
def test_conv_last_vs_f64_reference_and_integer_forms(case):
    from fcvsr_amd import hip
    cimg, dt, B, H, W = case
    q = R.conv_last_inputs(cimg, dt, B, H, W)
    ref, bound = R.conv_last_ref(q, cimg)
    spec = R.nchw((B, H, W, cimg), "f32", offset=3)
    obuf, out = _buffer(spec, F32, True)
    out.copy_(q["base"])
    u, wl, bias = q["u"].cuda(), q["wl"].cuda(), q["bias"].cuda()
    hip.conv_last(u, wl, bias, B, H, W, cimg, out, out)
    torch.cuda.synchronize()
    _check("fcvsr_conv_last", f"c{cimg} {H}x{W}", out, ref, bound)
    assert _untouched(obuf, spec, F32)
    base = q["base"].cuda()
    for idt, peak in ((torch.uint8, 255), (torch.uint16, hip.PEAK10)):
        for mode in ("truncate", "round"):
            o = torch.zeros(B, cimg, H, W, dtype=idt, device="cuda").permute(0, 2, 3, 1)
            hip.conv_last(u, wl, bias, B, H, W, cimg, base, o, hip.QUANTISE[mode])
            torch.cuda.synchronize()
            assert torch.equal(o.cpu().to(torch.int32), quantise(out.cpu(), peak, mode)), (idt, mode)


# ---- (e) engine closure -----------------------------------------------------------------------------------------------------------------

ENGINE = [("GShiftNet_S", "bf16", True), ("GShiftNet_S", "f16", True), ("GShiftNet_S", "bf16", False), ("GShiftNet_S", "f16", False),
          ("GShiftNet", "bf16", True), ("FCVSR_SNet", "bf16", True), ("GShiftNet_ETC", "bf16", True)]


@pytest.mark.parametrize("res", ["unset", "1"])
@pytest.mark.parametrize("cfg", ENGINE, ids=lambda c: f"{c[0]}-{c[1]}-{'trunk16' if c[2] else 'trunk32'}")
def test_engine_launches_only_declared_kernels(cfg, res, monkeypatch):
    from fcvsr_amd import hip
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    from helpers import get_ctor
    name, precision, trunk16 = cfg
    m = get_ctor(name)()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes(name), gain=0.5), strict=True)
    m = m.cuda()
    m.precision, m.trunk16 = precision, trunk16
    frames = m._in_frames + getattr(m, "_windows", 1) - 1
    x = torch.rand(1, frames, m._img_ch, 16, 20, generator=torch.Generator().manual_seed(11)).cuda()
    _policy(monkeypatch, "unset", res)
    monkeypatch.setattr(hip, "PROFILE", [])
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    launched = {r[6] for r in hip.PROFILE if r[3] == "mfma"}
    assert launched
    print(f"ENGINE\t{name}-{precision}-{trunk16}-res{res}\t" + "\t".join(sorted(launched)))
    declared = {c["kernel"] for c in MFMA}
    assert launched <= declared, sorted(launched - declared)
