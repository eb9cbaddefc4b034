"""GPU: the pyramid-builder, pyramid-fuse and up-sampler convolution paths against the paths they replaced, bit for bit.

  * conv3s2_lean_kernel (stride-2 3x3, only the existing output pixels) == the generic kernel's sub2 mode (full-resolution
    evaluation, even outputs kept; FCVSR_MFMA_LEAN=0 selects it);
  * conv1ps_res_kernel (1x1 64 -> cout pixel-shuffle up-convolution, resident weights, input read once) == conv1_lean_kernel
    (FCVSR_MFMA_RES=0 selects it);
  * 16-bit storage of the pyramid-fuse tensors: a 16-bit destination holds exactly the f32 destination rounded to the MFMA
    dtype (round to nearest even, as the consumer's staging rounds an f32 source), for the SCNetbk group conv (conv3_res, two
    residuals) and the pixel-shuffled 1x1 upconv1_L2_2 (generic kernel, residual), and fcvsr_pixel_shuffle16 writes the rounded
    shuffle plus zero pad channels;
  * upconv_fuse on the 16-bit sources [o0 | l2p | l3_2 + 4 zero channels] == the generic kernel on the three f32 sources."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import infer_conv_refs as R

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _mma(hip, dt):
    return hip.BF16 if dt == torch.bfloat16 else hip.F16


def _run(monkeypatch, env, value, fn):
    monkeypatch.setenv(env, value)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv(env)


@pytest.mark.parametrize("mdt", ["bf16", "f16"])
@pytest.mark.parametrize("levels,B,io16", [([(180, 320)], 2, True), ([(90, 160)], 3, True), ([(37, 53)], 2, True),
                                           ([(37, 53)], 2, False), ([(21, 70), (11, 35)], 2, True)])
def test_stride2_path_matches_generic_sub2(mdt, levels, B, io16, monkeypatch):
    from fcvsr_amd import hip
    dt = DT[mdt]
    cin = cout = 64
    g0 = torch.Generator().manual_seed(B * 1000 + levels[0][0] + int(io16))
    w = torch.randn(cout, cin, 3, 3, generator=g0) / (3.0 * cin ** 0.5)
    bias = torch.randn(cout, generator=g0).cuda()
    wp = hip.pack_conv_weight_mfma(w.cuda(), dt)
    sdt = dt if io16 else torch.float32
    groups = []
    for (H, W) in levels:
        x = torch.randn(B, H, W, cin, generator=g0).cuda().to(sdt)
        y = torch.empty(B, (H + 1) // 2, (W + 1) // 2, cout, device="cuda", dtype=sdt)
        groups.append(dict(srcs=[x], dst=y))
    outs = []
    for mode in ("1", "0"):
        for g in groups:
            g["dst"].fill_(float("nan"))
        _run(monkeypatch, "FCVSR_MFMA_LEAN", mode,
             lambda: hip.conv2d_mfma(groups, wp, 3, cout, _mma(hip, dt), stride=2, bias=bias, act=hip.ACT_LEAKY, slope=0.1))
        outs.append([g["dst"].clone() for g in groups])
    for a, b in zip(*outs):
        assert not torch.isnan(a.float()).any() and not torch.isnan(b.float()).any()
        assert torch.equal(a, b)
    # and the pair is right: every element of level 0 within the derived bound of the rounded-operand f64 reference
    # (tests/infer_conv_refs.py; tests/test_infer_conv_gpu.py pins both kernels at the tile edges)
    p = R.problem("anchor", 3, [cin], cout, levels[:1], B, mdt, mdt if io16 else "f32", src=mdt if io16 else "f32", stride=2, act=2, slope=0.1)
    r = R.conv_ref(p, dict(w=w, bias=bias.cpu(), slope_t=None, groups=[dict(srcs=[groups[0]["srcs"][0].cpu()], res=[])]))[0]
    assert bool(((outs[0][0].double().cpu() - r["ref"]).abs() <= r["bound"]).all())


@pytest.mark.parametrize("mdt", ["bf16", "f16"])
@pytest.mark.parametrize("cout,B,H,W", [(256, 2, 180, 320), (256, 1, 37, 53), (128, 2, 45, 80), (32, 1, 9, 11)])
def test_upconv1_resident_matches_lean(mdt, cout, B, H, W, monkeypatch):
    from fcvsr_amd import hip
    dt = DT[mdt]
    cin = 64
    g0 = torch.Generator().manual_seed(cout + H)
    w = torch.randn(cout, cin, 1, 1, generator=g0) / cin ** 0.5
    bias = torch.randn(cout, generator=g0)
    wp = hip.pack_conv_weight_mfma(w.cuda(), dt, ps=True)
    bp = bias[hip.ps_order(cout)].contiguous().cuda()
    slope_t = torch.tensor([0.2], device="cuda")
    x = torch.randn(B, H, W, cin, generator=g0).cuda().to(dt)
    y = torch.empty(B, 2 * H, 2 * W, cout // 4, device="cuda", dtype=dt)
    outs = []
    for mode in ("1", "0"):
        y.fill_(float("nan"))
        _run(monkeypatch, "FCVSR_MFMA_RES", mode,
             lambda: hip.conv2d_mfma([dict(srcs=[x], dst=y)], wp, 1, cout, _mma(hip, dt), bias=bp, act=hip.ACT_PRELU,
                                     slope_t=slope_t, pixel_shuffle=True))
        outs.append(y.clone())
    assert not torch.isnan(outs[0].float()).any() and not torch.isnan(outs[1].float()).any()
    assert torch.equal(outs[0], outs[1])
    # every element within the derived bound of the rounded-operand f64 reference (tests/infer_conv_refs.py)
    p = R.problem("anchor", 1, [cin], cout, [(H, W)], B, mdt, mdt, ps=True, act=3, slope_v=0.2)
    r = R.conv_ref(p, dict(w=w, bias=bias, slope_t=slope_t.cpu(), groups=[dict(srcs=[x.cpu()], res=[])]))[0]
    assert bool(((outs[0].double().cpu() - r["ref"]).abs() <= r["bound"]).all())


@pytest.mark.parametrize("mdt", ["bf16", "f16"])
def test_16bit_destinations_round_like_staging(mdt, monkeypatch):
    """The producers of o0..o2 / l2p store what the f32 destination holds, rounded to the MFMA dtype."""
    from fcvsr_amd import hip
    dt = DT[mdt]
    g0 = torch.Generator().manual_seed(7)
    B, n = 2, 64
    levels = [(24, 70), (12, 35), (6, 18)]
    # SCNetbk's last group conv: 3 grouped levels, 16-bit source, two residuals (conv3_res_kernel MODE 0 vs MODE 1)
    w = torch.randn(n, n, 3, 3, generator=g0) / (3.0 * n ** 0.5)
    bias = torch.randn(n, generator=g0).cuda()
    wp = hip.pack_conv_weight_mfma(w.cuda(), dt)
    xs = [torch.randn(B, H, W, n, generator=g0).cuda().to(dt) for (H, W) in levels]
    rs = [[torch.randn(B, H, W, n, generator=g0).cuda().to(dt) for _ in range(2)] for (H, W) in levels]
    got = {}
    for odt in (torch.float32, dt):
        outs = [torch.full((B, H, W, n), float("nan"), device="cuda", dtype=odt) for (H, W) in levels]
        _run(monkeypatch, "FCVSR_MFMA_RES", "1",           # the resident-weight kernel at any size, as at full resolution
             lambda: hip.conv2d_mfma([dict(srcs=[xs[l]], dst=outs[l], res=rs[l]) for l in range(3)], wp, 3, n, _mma(hip, dt),
                                     bias=bias, res_scale=[1.0, 1.0]))
        got[odt] = outs
    for a, b in zip(got[torch.float32], got[dt]):
        assert not torch.isnan(a).any()
        assert torch.equal(a.to(dt), b)
    # upconv1_L2_2: 1x1 over [l2 (64) | l3_1 (16)] f32, residual l2, pixel shuffle (generic 1x1 kernel), into a channel slice
    H, W = 23, 41
    w2 = torch.randn(n, n + n // 4, 1, 1, generator=g0) / n ** 0.5
    b2 = torch.randn(n, generator=g0)
    wp2 = hip.pack_conv_weight_mfma(w2.cuda(), dt, ps=True)
    bp2 = b2[hip.ps_order(n)].contiguous().cuda()
    l2 = torch.randn(B, H, W, n, generator=g0).cuda()
    l31 = torch.randn(B, H, W, n // 4, generator=g0).cuda()
    ref = torch.full((B, 2 * H, 2 * W, n // 4), float("nan"), device="cuda")
    l2p = torch.full((B, 2 * H, 2 * W, n // 4), float("nan"), device="cuda", dtype=dt)
    for d in (ref, l2p):
        hip.conv2d_mfma([dict(srcs=[l2, l31], dst=d, res=[l2])], wp2, 1, n, _mma(hip, dt), bias=bp2, res_scale=[1.0],
                        pixel_shuffle=True)
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any()
    assert torch.equal(ref.to(dt), l2p)
    # fcvsr_pixel_shuffle16: channels [0, 4) the rounded shuffle of l3_1, the rest zeros; here into a channel slice (strided
    # pixels) whose neighbours stay untouched, and into a dense 8-channel tensor as the engine uses it
    buf = torch.full((B, 2 * H, 2 * W, 24), float("nan"), device="cuda", dtype=dt)
    l32 = torch.full((B, 2 * H, 2 * W, 8), float("nan"), device="cuda", dtype=dt)
    for d in (buf[..., 8:24], l32):
        v = hip.view(d)
        hip.check(hip.lib().fcvsr_pixel_shuffle16(l31.data_ptr(), C.byref(v), B, H, W, n // 4, hip.stream_ptr()), "pixel_shuffle16")
    torch.cuda.synchronize()
    ps = F.pixel_shuffle(l31.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(dt)
    assert torch.equal(buf[..., 8:12], ps) and torch.equal(l32[..., :4], ps)
    assert torch.equal(buf[..., 12:].float(), torch.zeros(B, 2 * H, 2 * W, 12, device="cuda"))
    assert torch.equal(l32[..., 4:].float(), torch.zeros(B, 2 * H, 2 * W, 4, device="cuda"))
    assert torch.isnan(buf[..., :8].float()).all()


@pytest.mark.parametrize("mdt", ["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", [(2, 180, 320), (1, 37, 52)])
def test_upconv_fuse_16bit_sources_match_three_f32_sources(mdt, B, H, W):
    from fcvsr_amd import hip
    dt = DT[mdt]
    n = 64
    g0 = torch.Generator().manual_seed(H + W)
    w = torch.randn(n, n + n // 4 + n // 16, 3, 3, generator=g0) / (3.0 * 84 ** 0.5)
    bias = torch.randn(n, generator=g0).cuda()
    wp = hip.pack_conv_weight_mfma(w.cuda(), dt)
    o0 = torch.randn(B, H, W, n, generator=g0).cuda()
    l2p = torch.randn(B, H, W, n // 4, generator=g0).cuda()
    l32 = torch.randn(B, H, W, n // 16, generator=g0).cuda()
    l32p = torch.cat([l32, torch.zeros(B, H, W, 4, device="cuda")], dim=3).to(dt)
    outs = []
    for srcs in ([o0, l2p, l32], [o0.to(dt), l2p.to(dt), l32p]):
        y = torch.full((B, H, W, n), float("nan"), device="cuda", dtype=dt)
        hip.conv2d_mfma([dict(srcs=srcs, dst=y)], wp, 3, n, _mma(hip, dt), bias=bias)
        torch.cuda.synchronize()
        outs.append(y)
    assert not torch.isnan(outs[0].float()).any()
    assert torch.equal(outs[0], outs[1])
