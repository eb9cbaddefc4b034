"""GPU: 10-bit frames in 16-bit containers in, 10-bit SR frames out (`super_resolve_u16`) give exactly the samples of the float path
fed x.clamp(max=1023).float() / 1023 (divided on the host) and quantised with the 1023 scale, in every configuration: the dedicated
uint16 kernels (16-bit S / full / RGB twin) and the conversion kernels around the generic layers (exact-f32 mode, 21-channel
first layer).  uint16 tensors are moved to the device as int16 views of the same bits and compared as int32."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(ctor_name, precision, **attrs):
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    from helpers import get_ctor
    m = get_ctor(ctor_name)()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes(ctor_name), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = precision
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _frames(B, C, H, W, seed, hi=1024):
    """(B,7,C,H,W) uint16 numpy samples, uniform in [0, hi)."""
    return np.random.RandomState(seed).randint(0, hi, (B, 7, C, H, W)).astype(np.uint16)


def _dev16(a):
    """numpy uint16 -> device uint16 (uploaded as int16 bits)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _i32(t):
    """device uint16 -> host int32 values."""
    return torch.from_numpy(t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int32))


def _host_float(a16):
    """The float frames a caller converting on the host feeds the float path: min(k, 1023) -> .float() / 1023."""
    return torch.from_numpy(np.minimum(a16, 1023).astype(np.float32)) / 1023


def _expected(model, a16, quantise):
    with torch.no_grad():
        y = model(_host_float(a16).cuda())
    y = y.clamp(0, 1) * 1023.0
    y = y.round() if quantise == "round" else y
    return y.to(torch.int32).cpu()


def _check(model, a16, quantise):
    got = model.super_resolve_u16(_dev16(a16), quantise)
    ref = _expected(model, a16, quantise)
    assert got.dtype == torch.uint16 and tuple(got.shape) == tuple(ref.shape) and got.is_cuda
    g = _i32(got)
    mism = int((g != ref).sum())
    assert mism == 0, f"{mism} of {ref.numel()} samples differ (max {int((g - ref).abs().max())})"
    assert int(g.max()) <= 1023
    assert torch.unique(g).numel() > 32            # a real image, not a frame clamped to 0 / 1023
    return g


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("precision", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("hw", [(16, 20), (72, 36)])
def test_s_model_u16_equals_float_path(precision, hw, quantise):
    m = _model("GShiftNet_S", precision)
    _check(m, _frames(2, 1, *hw, seed=hw[0] + len(precision)), quantise)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_full_model_bf16_u16_equals_float_path(quantise):
    m = _model("GShiftNet", "bf16")
    _check(m, _frames(1, 1, 20, 24, seed=11), quantise)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_rgb_s_twin_bf16_u16_equals_float_path(quantise):
    m = _model("FCVSR_SNet", "bf16")
    _check(m, _frames(1, 3, 16, 20, seed=12), quantise)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_samples_above_1023_are_read_as_1023(precision):
    """A 16-bit container can hold more than 10 bits: such samples, also in the first and last row and column (the base skip's
    edge taps, the first layer's border pixels), give the result of the clamped input and never index past the table."""
    m = _model("GShiftNet_S", precision)
    a = _frames(2, 1, 16, 20, seed=13)
    rs = np.random.RandomState(14)
    big = rs.randint(1024, 65536, a.shape).astype(np.uint16)
    sel = rs.rand(*a.shape) < 0.1
    sel[..., 0, ::3] = True
    sel[..., -1, 1::3] = True
    sel[..., ::2, 0] = True
    sel[..., 1::2, -1] = True
    a = np.where(sel, big, a)
    a[0, 3, 0, 0, 0], a[0, 3, 0, -1, -1], a[1, 0, 0, 0, -1] = 65535, 65535, 1024
    assert int((a > 1023).sum()) > 100
    g = _check(m, a, "round")
    clamped = m.super_resolve_u16(_dev16(np.minimum(a, 1023)), "round")
    assert torch.equal(g, _i32(clamped))


def test_graph_two_streams_batch4_and_no_crosstalk_between_f32_u8_and_u16():
    """hipGraph replay with two streams at B = 4; alternating float, uint8 and uint16 calls of one shape on one model never replay
    each other's graph (the input dtype is part of the key), twice round."""
    m = _model("GShiftNet_S", "bf16", use_graph=True, streams=2, graph_cache_size=8)
    a16 = _frames(4, 1, 16, 20, seed=21)
    a8 = torch.from_numpy(np.random.RandomState(22).randint(0, 256, (4, 7, 1, 16, 20)).astype(np.uint8))
    xf = _host_float(_frames(4, 1, 16, 20, seed=23))
    e = _model("GShiftNet_S", "bf16")                            # eager, one stream
    with torch.no_grad():
        ref_f = e(xf.cuda())
    ref_8 = e.super_resolve_u8(a8.cuda(), "truncate")
    ref_16 = _i32(e.super_resolve_u16(_dev16(a16), "truncate"))
    assert torch.equal(ref_16, _expected(e, a16, "truncate"))
    for it in range(2):
        with torch.no_grad():
            yf = m(xf.cuda())
        assert yf.dtype == torch.float32 and torch.equal(yf, ref_f), it
        y8 = m.super_resolve_u8(a8.cuda(), "truncate")
        assert y8.dtype == torch.uint8 and torch.equal(y8, ref_8), it
        y16 = m.super_resolve_u16(_dev16(a16), "truncate")
        assert y16.dtype == torch.uint16 and torch.equal(_i32(y16), ref_16), it
    keys = list(m._engine._graphs)
    for dt in (torch.float32, torch.uint8, torch.uint16):
        assert any(dt in k for k in keys), (dt, keys)


def test_non_contiguous_input_view():
    m = _model("GShiftNet_S", "bf16")
    a = np.random.RandomState(31).randint(0, 1024, (2, 7, 1, 16, 28)).astype(np.uint16)
    x = _dev16(a)[:, :, :, :, 4:24]                            # (2,7,1,16,20), non-contiguous
    assert not x.is_contiguous()
    got = m.super_resolve_u16(x, "round")
    assert torch.equal(_i32(got), _expected(m, np.ascontiguousarray(a[..., 4:24]), "round"))


def test_u16_argument_errors():
    m = _model("GShiftNet_S", "bf16")
    x = _dev16(_frames(1, 1, 16, 20, seed=41))
    with pytest.raises(ValueError, match="multiples of 4"):
        m.super_resolve_u16(x[..., :18])
    with pytest.raises(ValueError, match="uint16"):
        m.super_resolve_u16(x.view(torch.int16).float())
    with pytest.raises(ValueError, match="uint16"):
        m.super_resolve_u16(x.view(torch.int16))
    with pytest.raises(ValueError, match="uint16"):
        m.super_resolve_u16(torch.zeros(1, 7, 1, 16, 20, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):
        m.super_resolve_u8(x)
    with pytest.raises(ValueError, match="quantise"):
        m.super_resolve_u16(x, "nearest")
    with pytest.raises(ValueError, match="frames"):
        m.super_resolve_u16(x[:, :5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.super_resolve_u16(torch.zeros(1, 7, 1, 16, 20, dtype=torch.uint16))
    with pytest.raises(NotImplementedError):
        _model("GShiftNet_ETC", "bf16").super_resolve_u16(_dev16(np.zeros((1, 13, 1, 16, 20), np.uint16)))


def _tail_problem(B, H, W, dt, slope, seed):
    from fcvsr_amd import hip
    g = torch.Generator().manual_seed(seed)
    p = {}
    p["u1"] = torch.randn(B, 2 * H, 2 * W, 64, generator=g).to(dt).cuda()
    w2 = torch.randn(256, 64, 1, 1, generator=g) / 8
    b2 = torch.randn(256, generator=g) * 0.1
    wl = torch.randn(1, 64, 3, 3, generator=g) / 240
    p["w2"] = hip.pack_conv_weight_mfma(w2.cuda(), dt, ps=True)
    p["b2"] = b2[hip.ps_order(256)].contiguous().cuda()
    tab = torch.zeros(16, 64)
    tab[:9] = wl[0].permute(1, 2, 0).reshape(9, 64)
    p["wl"] = tab.to(dt).contiguous().cuda()
    p["bl"] = torch.tensor([0.03]).cuda()
    p["slope"] = torch.tensor([slope]).cuda()
    # the centre frame as the engine passes it: a strided (B,H,W,1) view into the (B,T,1,H,W) window; some samples above 1023
    f = np.random.RandomState(seed).randint(0, 1100, (B, 7, 1, H, W)).astype(np.uint16)
    p["frames16"] = _dev16(f)
    return p


def _tail_args(p):
    return (p["w2"].data_ptr(), p["b2"].data_ptr(), p["slope"].data_ptr(), p["wl"].data_ptr(), p["bl"].data_ptr())


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("hw", [(16, 20), (72, 36)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_u16_base_in_kernel_equals_bilinear_u16_then_tail_u16(dt, hw, quantise):
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    B, (H, W) = 2, hw
    q = hip.QUANTISE[quantise]
    p = _tail_problem(B, H, W, dt, 0.25, seed=7 + H)
    tab = hip.u16_table("cuda")
    centre = p["frames16"][:, 3].permute(0, 2, 3, 1)
    u1v, cv = hip.view(p["u1"]), hip.view(centre)
    assert cv.dtype == hip.U16
    base = torch.empty(B, 1, 4 * H, 4 * W, device="cuda")
    bv = hip.view(base.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_bilinear_up4_u16(C.byref(cv), tab.data_ptr(), B, H, W, C.byref(bv), st), "fcvsr_bilinear_up4_u16")
    ref = torch.empty(B, 1, 4 * H, 4 * W, device="cuda", dtype=torch.uint16)
    rv = hip.view(ref.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_tail_fused_u16(C.byref(u1v), *_tail_args(p), B, 2 * H, 2 * W, C.byref(bv), C.byref(rv), q, st),
              "fcvsr_tail_fused_u16")
    got = torch.empty(B, 1, 4 * H, 4 * W, device="cuda", dtype=torch.int16).fill_(77).view(torch.uint16)
    gv = hip.view(got.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_tail_fused_base_u16(C.byref(u1v), *_tail_args(p), C.byref(cv), tab.data_ptr(), B, 2 * H, 2 * W, C.byref(gv), q,
                                          st), "fcvsr_tail_fused_base_u16")
    r, g = _i32(ref), _i32(got)
    assert torch.unique(r).numel() > 32 and int(r.max()) <= 1023
    assert torch.equal(g, r), f"{int((g != r).sum())} of {r.numel()} samples differ"


def test_library_rejects_bad_u16_arguments():
    """The C entry points return FCVSR_E_ARG (-1) instead of launching: a FCVSR_U8 view handed to a _u16 entry point, bad quantise
    modes, null pointers, a misaligned chroma destination."""
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    tab = hip.u16_table("cuda")
    assert tab.numel() == 1024 and tab.dtype == torch.float32 and tab.data_ptr() % 16 == 0
    host = (torch.arange(1024, dtype=torch.int32).float() / 1023)
    assert torch.equal(tab.cpu(), host)
    p = _tail_problem(1, 4, 4, torch.bfloat16, 0.25, seed=1)
    u1v = hip.view(p["u1"])
    c16 = hip.view(p["frames16"][:, 3].permute(0, 2, 3, 1))
    c8 = hip.view(torch.zeros(1, 4, 4, 1, dtype=torch.uint8, device="cuda"))
    fb = torch.zeros(1, 16, 16, 1, device="cuda")
    o16 = torch.zeros(1, 16, 16, 1, dtype=torch.int16, device="cuda").view(torch.uint16)
    o8 = torch.zeros(1, 16, 16, 1, dtype=torch.uint8, device="cuda")
    fv, o16v, o8v = hip.view(fb), hip.view(o16), hip.view(o8)
    # a uint8 view where uint16 is expected
    assert L.fcvsr_bilinear_up4_u16(C.byref(c8), tab.data_ptr(), 1, 4, 4, C.byref(fv), st) == -1
    assert L.fcvsr_tail_fused_base_u16(C.byref(u1v), *_tail_args(p), C.byref(c8), tab.data_ptr(), 1, 8, 8, C.byref(o16v), 1, st) == -1
    assert L.fcvsr_tail_fused_base_u16(C.byref(u1v), *_tail_args(p), C.byref(c16), tab.data_ptr(), 1, 8, 8, C.byref(o8v), 1, st) == -1
    assert L.fcvsr_tail_fused_u16(C.byref(u1v), *_tail_args(p), 1, 8, 8, C.byref(fv), C.byref(o8v), 1, st) == -1
    u2 = torch.zeros(1, 16, 16, 64, dtype=torch.bfloat16, device="cuda")
    wl = torch.zeros(16, 64, dtype=torch.bfloat16, device="cuda")
    assert L.fcvsr_conv_last_u16(C.byref(hip.view(u2)), wl.data_ptr(), None, 1, 16, 16, 1, C.byref(fv), C.byref(o8v), 1, st) == -1
    x8 = hip.view(torch.zeros(1, 7, 4, 4, dtype=torch.uint8, device="cuda").permute(0, 2, 3, 1))
    wf = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    dst = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device="cuda")
    assert L.fcvsr_feat_extract_u16(C.byref(x8), tab.data_ptr(), 1, 4, 4, wf.data_ptr(), None, 1, (C.c_void_p * 1)(dst.data_ptr()),
                                    (C.c_int64 * 1)(64), (C.c_int32 * 1)(0), hip.BF16, st) == -1
    # bad quantise modes
    assert L.fcvsr_tail_fused_base_u16(C.byref(u1v), *_tail_args(p), C.byref(c16), tab.data_ptr(), 1, 8, 8, C.byref(o16v), 0, st) == -1
    assert L.fcvsr_tail_fused_u16(C.byref(u1v), *_tail_args(p), 1, 8, 8, C.byref(fv), C.byref(o16v), 3, st) == -1
    assert L.fcvsr_quantise_u16(fb.data_ptr(), fb.numel(), 0, o16.data_ptr(), st) == -1
    assert L.fcvsr_conv_last_u16(C.byref(hip.view(u2)), wl.data_ptr(), None, 1, 16, 16, 1, C.byref(fv), C.byref(o16v), 0, st) == -1
    # null pointers
    assert L.fcvsr_bilinear_up4_u16(C.byref(c16), None, 1, 4, 4, C.byref(fv), st) == -1
    assert L.fcvsr_tail_fused_base_u16(C.byref(u1v), *_tail_args(p), C.byref(c16), None, 1, 8, 8, C.byref(o16v), 1, st) == -1
    assert L.fcvsr_u16_to_f32(None, tab.data_ptr(), 16, fb.data_ptr(), st) == -1
    assert L.fcvsr_quantise_u16(None, 16, 1, o16.data_ptr(), st) == -1
    assert L.fcvsr_chroma_up4_u16(None, tab.data_ptr(), 1, 2, 2, None, st) == -1
    # the chroma kernel stores 8 bytes at a time
    src = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.zeros(1024, dtype=torch.int16, device="cuda")
    assert out.data_ptr() % 8 == 0
    for off in (2, 4, 6):
        assert L.fcvsr_chroma_up4_u16(src.data_ptr(), tab.data_ptr(), 1, 2, 2, out.data_ptr() + off, st) == -1
    assert L.fcvsr_chroma_up4_u16(src.data_ptr(), tab.data_ptr(), 1, 2, 2, out.data_ptr() + 8, st) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.chroma_up4(torch.zeros(2, 4, 4, device="cuda"))
