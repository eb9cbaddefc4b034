"""GPU: the fused up-sampler tail that evaluates the bilinear x4 base skip itself (fcvsr_tail_fused_base, and its uint8 form
fcvsr_tail_fused_base_u8) against the two launches it replaces (fcvsr_bilinear_up4 + fcvsr_tail_fused, and their _u8 forms):
the same bits, for both 16-bit dtypes, for slopes inside [0, 1] (PReLU as max(x, s*x)) and outside (the generic form), on
shapes with one partial tile, with border tiles only and with interior tiles."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (36, 68), (180, 320)]                      # centre LR frame; u1 is (2H, 2W), the result (4H, 4W)
SLOPES = [0.25, 0.0, 1.0, -0.1, 1.5]                         # the last two take the generic PReLU branch


def _problem(B, H, W, dt, slope, seed):
    from fcvsr_amd import hip
    g = torch.Generator().manual_seed(seed)
    H2, W2 = 2 * H, 2 * W
    p = {}
    p["u1"] = torch.randn(B, H2, W2, 64, generator=g).to(dt).cuda()
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
    # the centre frame as the engine passes it: a strided (B,H,W,1) view into the (B,T,1,H,W) window
    p["frames8"] = torch.randint(0, 256, (B, 7, 1, H, W), generator=g, dtype=torch.uint8).cuda()
    p["frames"] = (p["frames8"].float() / 255).contiguous()
    return p


def _args(p):
    return (p["w2"].data_ptr(), p["b2"].data_ptr(), p["slope"].data_ptr(), p["wl"].data_ptr(), p["bl"].data_ptr())


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_base_in_kernel_equals_bilinear_then_tail(dt, hw, slope):
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    B, (H, W) = 2, hw
    p = _problem(B, H, W, dt, slope, seed=H + int(slope * 100) % 97)
    centre = p["frames"][:, 3].permute(0, 2, 3, 1)
    u1v, cv = hip.view(p["u1"]), hip.view(centre)
    ref = torch.empty(B, 1, 4 * H, 4 * W, device="cuda")
    rv = hip.view(ref.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_bilinear_up4(C.byref(cv), B, H, W, C.byref(rv), st), "fcvsr_bilinear_up4")
    base = ref.clone()
    hip.check(L.fcvsr_tail_fused(C.byref(u1v), *_args(p), B, 2 * H, 2 * W, C.byref(rv), st), "fcvsr_tail_fused")
    got = torch.full_like(ref, float("nan"))                  # write-only: whatever it held must not matter
    gv = hip.view(got.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_tail_fused_base(C.byref(u1v), *_args(p), C.byref(cv), B, 2 * H, 2 * W, C.byref(gv), st),
              "fcvsr_tail_fused_base")
    assert torch.isfinite(ref).all() and float((ref - base).abs().max()) > 0.05     # the tail term is really there
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} values differ, max {float((got - ref).abs().max())}"


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("slope", [0.25, 1.5])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_u8_base_in_kernel_equals_bilinear_u8_then_tail_u8(dt, hw, slope, quantise):
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    B, (H, W) = 2, hw
    q = hip.QUANTISE[quantise]
    p = _problem(B, H, W, dt, slope, seed=7 + H)
    tab = hip.u8_table("cuda")
    centre8 = p["frames8"][:, 3].permute(0, 2, 3, 1)
    u1v, cv = hip.view(p["u1"]), hip.view(centre8)
    base = torch.empty(B, 1, 4 * H, 4 * W, device="cuda")
    bv = hip.view(base.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_bilinear_up4_u8(C.byref(cv), tab.data_ptr(), B, H, W, C.byref(bv), st), "fcvsr_bilinear_up4_u8")
    ref = torch.empty(B, 1, 4 * H, 4 * W, device="cuda", dtype=torch.uint8)
    rv = hip.view(ref.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_tail_fused_u8(C.byref(u1v), *_args(p), B, 2 * H, 2 * W, C.byref(bv), C.byref(rv), q, st), "fcvsr_tail_fused_u8")
    got = torch.full_like(ref, 77)
    gv = hip.view(got.permute(0, 2, 3, 1))
    hip.check(L.fcvsr_tail_fused_base_u8(C.byref(u1v), *_args(p), C.byref(cv), tab.data_ptr(), B, 2 * H, 2 * W, C.byref(gv), q, st),
              "fcvsr_tail_fused_base_u8")
    assert torch.unique(ref).numel() > 32                     # a real image, not a frame clamped to 0 / 255
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} bytes differ"


def test_library_rejects_bad_base_arguments():
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    p = _problem(1, 4, 4, torch.bfloat16, 0.25, seed=1)
    out = torch.empty(1, 1, 16, 16, device="cuda")
    u1v, ov = hip.view(p["u1"]), hip.view(out.permute(0, 2, 3, 1))
    c8 = hip.view(p["frames8"][:, 3].permute(0, 2, 3, 1))
    cf = hip.view(p["frames"][:, 3].permute(0, 2, 3, 1))
    assert L.fcvsr_tail_fused_base(C.byref(u1v), *_args(p), C.byref(c8), 1, 8, 8, C.byref(ov), st) == -1      # uint8 centre
    assert L.fcvsr_tail_fused_base(C.byref(u1v), *_args(p), None, 1, 8, 8, C.byref(ov), st) == -1
    odd = hip.view(p["u1"][:, :7])
    assert L.fcvsr_tail_fused_base(C.byref(odd), *_args(p), C.byref(cf), 1, 7, 8, C.byref(ov), st) == -1      # H2 odd
    o8 = torch.empty(1, 1, 16, 16, device="cuda", dtype=torch.uint8)
    o8v = hip.view(o8.permute(0, 2, 3, 1))
    tab = hip.u8_table("cuda")
    assert L.fcvsr_tail_fused_base_u8(C.byref(u1v), *_args(p), C.byref(cf), tab.data_ptr(), 1, 8, 8, C.byref(o8v), 1, st) == -1   # f32 centre
    assert L.fcvsr_tail_fused_base_u8(C.byref(u1v), *_args(p), C.byref(c8), None, 1, 8, 8, C.byref(o8v), 1, st) == -1            # no table
    assert L.fcvsr_tail_fused_base_u8(C.byref(u1v), *_args(p), C.byref(c8), tab.data_ptr(), 1, 8, 8, C.byref(ov), 1, st) == -1   # f32 out
    assert L.fcvsr_tail_fused_base_u8(C.byref(u1v), *_args(p), C.byref(c8), tab.data_ptr(), 1, 8, 8, C.byref(o8v), 0, st) == -1  # QUANT_NONE
