"""GPU: the 16-bit 3x3 matrix-core convolutions (conv3_res_kernel, conv3_lean_kernel, conv_mfma_kernel) against a float64 CPU
reference of the rounded operands, and conv3_res against the other two bit for bit where the existing tests do not reach.

conv3_res_kernel issues v_mfma_f32_16x16x32 (9 taps x 2 steps of 32 channels), the other two 32x32x16 (9 taps x 4 steps of 16);
in both the order is tap-major with ascending channels.  The reference rounds x, w and the 16-bit residuals to the operand dtype,
sums in f64 and applies bias, activation, residuals and pixel shuffle.  Every entry is bounded by
    |got - ref| <= tau(n) * S + u * |ref|,
S = the same operation on absolute values, n = the products summed into the entry, tau(n) as in test_train_conv_gpu.py, and u the
rounding of the destination (one unit in the last place: 2^-7 bf16, 2^-10 f16, 0 f32)."""
import pytest
import torch
import torch.nn.functional as F

from tolerance import tau

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 0.0}
RS = [1.0, -0.5]


def _problem(cin, cout, levels, B, dst16, nres, mdt, ps, seed):
    from fcvsr_amd import hip
    dt = DT[mdt]
    g0 = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, 3, 3, generator=g0) / (3.0 * cin ** 0.5)).to(dt).float()
    bias = torch.randn(cout, generator=g0)
    wp = hip.pack_conv_weight_mfma(w.cuda(), dt, ps=ps)
    bp = (bias[hip.ps_order(cout)] if ps else bias).contiguous().cuda()
    groups = []
    for (H, W) in levels:
        x = torch.randn(B, H, W, cin, generator=g0).to(dt)
        res = [torch.randn(B, H, W, cout, generator=g0).to(dt) for _ in range(nres)]
        shape = (B, 2 * H, 2 * W, cout // 4) if ps else (B, H, W, cout)
        y = torch.empty(shape, device="cuda", dtype=dt if dst16 else torch.float32)
        src = x.float() if cin % 8 else x              # a 16-bit source needs 8-channel granules: f32 of the same values
        groups.append(dict(srcs=[src.cuda()], dst=y, res=[r.cuda() for r in res], ps=ps, x=x, r=res))
    return w, bias, bp, wp, groups


def _run(groups, wp, bp, cout, mdt, act, ps, monkeypatch, res, lean=True):
    from fcvsr_amd import hip
    monkeypatch.setenv("FCVSR_MFMA_RES", "1" if res else "0")
    monkeypatch.setenv("FCVSR_MFMA_LEAN", "1" if lean else "0")
    slope_t = torch.tensor([0.25]).cuda()
    for g in groups:
        g["dst"].fill_(float("nan"))
    hip.conv2d_mfma([dict(srcs=g["srcs"], dst=g["dst"], res=g["res"], ps=ps) for g in groups], wp, 3, cout,
                    hip.BF16 if mdt == "bf16" else hip.F16, bias=bp, act=act, slope=0.1, slope_t=slope_t,
                    res_scale=RS[:len(groups[0]["res"])], pixel_shuffle=ps)
    torch.cuda.synchronize()
    kname = hip.lib().fcvsr_last_conv_kernel().decode()
    monkeypatch.delenv("FCVSR_MFMA_RES")
    monkeypatch.delenv("FCVSR_MFMA_LEAN")
    return kname, [g["dst"].float().cpu() for g in groups]


def _reference(g, w, bias, act, ps):
    """f64 result and its condition S of one level (NHWC; the pixel-shuffled layout for ps)."""
    x = g["x"].double().permute(0, 3, 1, 2)
    wd = w.double()
    y = F.conv2d(x, wd, bias.double(), padding=1)
    s = F.conv2d(x.abs(), wd.abs(), bias.double().abs(), padding=1)
    if act == 2:
        y = torch.where(y >= 0, y, 0.1 * y)
    elif act == 3:
        y = torch.where(y >= 0, y, 0.25 * y)
    for q, r in enumerate(g["r"]):
        rr = r.double().permute(0, 3, 1, 2)
        y = y + RS[q] * rr
        s = s + abs(RS[q]) * rr.abs()
    if ps:
        y, s = F.pixel_shuffle(y, 2), F.pixel_shuffle(s, 2)
    return y.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1)


# (kernel, cin, cout, levels, B, dst16, nres, mma, ps, act); act 2 = LeakyReLU(0.1), 3 = PReLU(0.25), 0 = none
CASES = [
    ("conv3_res", 64, 64, [(21, 37), (11, 19), (6, 10)], 2, True, 0, "bf16", False, 2),
    ("conv3_res", 64, 64, [(19, 70)], 3, False, 2, "bf16", False, 0),
    ("conv3_res", 64, 128, [(40, 70), (20, 35)], 1, True, 1, "bf16", False, 2),
    ("conv3_res", 64, 256, [(17, 33)], 1, True, 0, "f16", False, 3),
    ("conv3_res", 128, 64, [(23, 41), (12, 21), (6, 11)], 2, False, 1, "bf16", False, 3),
    ("conv3_res", 128, 128, [(17, 45)], 2, True, 2, "f16", False, 2),
    ("conv3_res", 64, 256, [(13, 37)], 2, True, 0, "bf16", True, 3),
    ("conv3_lean", 64, 64, [(21, 37), (11, 19)], 2, True, 1, "bf16", False, 2),
    ("conv3_lean", 128, 64, [(17, 35)], 2, False, 0, "f16", False, 3),
    ("conv3_lean", 64, 128, [(9, 40)], 2, True, 2, "bf16", False, 0),
    ("conv_mfma", 84, 64, [(15, 29), (8, 15)], 2, False, 0, "bf16", False, 2),
    ("conv_mfma", 64, 64, [(15, 29)], 2, True, 0, "f16", False, 3),
    ("conv_mfma", 64, 256, [(11, 21)], 2, True, 0, "bf16", True, 3),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}to{c[2]}-L{len(c[3])}-{'d16' if c[5] else 'f32'}-r{c[6]}-{c[7]}{'-ps' if c[8] else ''}")
def test_conv3_16bit_vs_f64_reference(case, monkeypatch):
    kernel, cin, cout, levels, B, dst16, nres, mdt, ps, act = case
    w, bias, bp, wp, groups = _problem(cin, cout, levels, B, dst16, nres, mdt, ps, seed=cin * 7 + cout + nres + len(levels))
    kname, outs = _run(groups, wp, bp, cout, mdt, act, ps, monkeypatch, res=kernel == "conv3_res", lean=kernel != "conv_mfma")
    assert kname.startswith(kernel), kname
    u = ULP[DT[mdt] if dst16 else torch.float32]
    t = tau(9 * cin)
    for g, got in zip(groups, outs):
        ref, s = _reference(g, w, bias, act, ps)
        assert not torch.isnan(got).any()
        err = (got.double() - ref).abs()
        bound = t * s + u * ref.abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{kname}: worst err / bound {worst:.3f}")
        assert bool((err <= bound).all()), f"{kname}: worst err / bound {worst:.3f}"


# conv3_res against conv3_lean (lean=True) and the generic kernel (lean=False, no residuals: its residuals are f32 only), bit for
# bit: the 128-input-channel layers with an f32 destination (NCH = 2, MODE 0), PReLU (NSU = 0) and f16 operands
BITWISE = [
    (128, 64, [(23, 41), (12, 21)], False, 1, "bf16", 3, True),
    (128, 128, [(17, 45)], False, 0, "f16", 2, True),
    (64, 64, [(21, 37), (11, 19), (6, 10)], True, 1, "f16", 3, True),
    (64, 128, [(19, 70)], False, 2, "f16", 3, True),
    (128, 64, [(23, 41)], False, 0, "bf16", 3, False),
    (64, 64, [(21, 37)], True, 0, "f16", 3, False),
]


@pytest.mark.parametrize("case", BITWISE, ids=lambda c: f"{c[0]}to{c[1]}-{'d16' if c[3] else 'f32'}-r{c[4]}-{c[5]}-act{c[6]}-{'lean' if c[7] else 'generic'}")
def test_conv3_res_bitwise_other_paths(case, monkeypatch):
    cin, cout, levels, dst16, nres, mdt, act, lean = case
    w, bias, bp, wp, groups = _problem(cin, cout, levels, 2, dst16, nres, mdt, False, seed=cin + 3 * cout + nres)
    k0, o0 = _run(groups, wp, bp, cout, mdt, act, False, monkeypatch, res=False, lean=lean)
    k1, o1 = _run(groups, wp, bp, cout, mdt, act, False, monkeypatch, res=True)
    assert k0.startswith("conv3_lean" if lean else "conv_mfma"), k0
    assert k1.startswith("conv3_res"), k1
    for a, b in zip(o0, o1):
        assert not torch.isnan(a).any()
        assert torch.equal(a, b)
