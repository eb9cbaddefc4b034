"""CPU: the hand-written float64 references of tests/train_block_refs.py against torch autograd in float64 on the plain operator
chains (the F.* expressions of tests/test_train_gpu.py and graph.py's unfused forms), to 1e-12 of each tensor's largest entry, at
tiny shapes.  Also: the input builders of tests/test_train_blocks_gpu.py converge for every seed that file uses."""
import pytest
import torch
import torch.nn.functional as F

import train_block_refs as R

D = torch.float64
TOL = 1e-12


def close(name, got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert err <= TOL * max(float(ref.abs().max()), 1e-300), f"{name}: {err:.3e}"


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=D) * scale


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 5), (3, 4, 2)])
def test_rcb_tail_reference_vs_autograd(B, H, W):
    g = torch.Generator().manual_seed(100 + B * H * W)
    C, slope = 64, 0.2
    r, z = rnd(g, B, C, H, W, scale=0.7).requires_grad_(), rnd(g, B, C, H, W).requires_grad_()
    wm, w1, w2 = (rnd(g, *s, scale=k).requires_grad_() for s, k in (((1, C, 1, 1), 0.3), ((C, C, 1, 1), 0.2), ((C, C, 1, 1), 0.2)))
    go = rnd(g, B, C, H, W)
    rm = r.permute(0, 2, 3, 1).reshape(B, H * W, C)
    m = torch.softmax(rm @ wm.reshape(C, 1), dim=1)
    ctx = (m.transpose(1, 2) @ rm).reshape(B, C)
    t = ctx @ w1.flatten(1).t()
    add = F.leaky_relu(t, slope) @ w2.flatten(1).t()
    for x in (ctx, t, add):
        x.retain_grad()
    out = F.leaky_relu(r + add[:, :, None, None], slope) + z
    out.backward(go)
    ref = R.rcb_tail_reference(r, z, wm, w1, w2, slope, go)
    close("out", ref["out"], out.detach())
    for name, x in (("ctx", ctx), ("t", t), ("add", add)):
        close(name, ref[name][0], x.detach())
    close("gadd", ref["gadd"][0], add.grad)
    close("gctx", ref["gctx"][0], ctx.grad)
    close("gr", ref["gr"], r.grad)
    close("gz", ref["gz"], z.grad)
    for name, p in (("dwmask", wm), ("dw1", w1), ("dw2", w2)):
        close(name, ref[name][0], p.grad)
        assert bool((ref[name][1] >= ref[name][0].abs() * (1 - 1e-12)).all()), name          # a condition bounds its value


@pytest.mark.parametrize("B,C,H,W", [(1, 32, 1, 1), (2, 64, 3, 5), (3, 32, 4, 3)])
def test_divenh_band_reference_vs_autograd(B, C, H, W):
    g = torch.Generator().manual_seed(200 + C + H)
    f, sf, so = (rnd(g, B, C, H, W).requires_grad_() for _ in range(3))
    a = (1.0 + 0.3 * rnd(g, 1, C, 1, 1)).requires_grad_()
    b = (0.5 + 0.3 * rnd(g, 1, C, 1, 1)).requires_grad_()
    w1, w2 = rnd(g, C // 16, C, 1, 1, scale=0.4).requires_grad_(), rnd(g, C, C // 16, 1, 1, scale=0.4).requires_grad_()
    g1, g2 = rnd(g, B, C, H, W), rnd(g, B, C, H, W)
    stats = []

    def ca(zz):
        y = zz.mean(dim=(2, 3))
        h = F.relu(y @ w1.flatten(1).t())
        s = torch.sigmoid(h @ w2.flatten(1).t())
        stats.append((y.detach(), h.detach(), s.detach()))
        return zz * s[:, :, None, None]

    t = f - sf + 0.2 * so
    o = ca(0.2 * a * t * f + b * f) + ca(0.2 * a * so * f + b * f)
    nsf, nso = sf + f, so + o
    ((nsf * g1).sum() + (nso * g2).sum()).backward()
    ref = R.divenh_band_reference(f, sf, so, a, b, w1, w2, g1, g2)
    close("Sf", ref["Sf"], nsf.detach())
    close("So", ref["So"], nso.detach())
    for k in range(2):
        close(f"mean{k}", ref["mean"][k], stats[k][0])
        close(f"z{k}", ref["z"][k], stats[k][1])
        close(f"gate{k}", ref["gate"][k], stats[k][2])
    for name, p in (("gf", f), ("gSf", sf), ("gSo", so)):
        close(name, ref[name], p.grad)
    close("ga", ref["ga"][0], a.grad.reshape(-1))
    close("gb", ref["gb"][0], b.grad.reshape(-1))
    close("dw1", ref["dw1"][0], w1.grad)
    close("dw2", ref["dw2"][0], w2.grad)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 32), (2, 1, 4, 32), (2, 4, 1, 64), (2, 3, 5, 32)])
def test_iac_bwd_sac_reference_vs_autograd(B, H, W, C):
    from fcvsr_amd.train import graph as G
    g = torch.Generator().manual_seed(300 + H * W)
    slope = 0.1
    s, fin = rnd(g, B, C, H, W).requires_grad_(), rnd(g, B, C, H, W).requires_grad_()
    k1 = rnd(g, B, 3 * C, H, W, scale=0.4).requires_grad_()
    gy = rnd(g, B, C, H, W)
    k = k1.reshape(B, C, 3, H, W)
    sp = F.pad(s, (0, 0, 1, 1), mode="replicate")
    v = sp[:, :, 0:H] * k[:, :, 0] + sp[:, :, 1:H + 1] * k[:, :, 1] + sp[:, :, 2:H + 2] * k[:, :, 2]
    v.retain_grad()
    vp = F.pad(v, (1, 1, 0, 0), mode="replicate")
    h = vp[..., 0:W] * k[:, :, 0] + vp[..., 1:W + 1] * k[:, :, 1] + vp[..., 2:W + 2] * k[:, :, 2]
    close("graph._sac is this chain", G._sac(s.detach(), k1.detach()), h.detach())
    slope32 = float(torch.tensor(slope, dtype=torch.float32))        # the kernel (and so the reference) multiplies by the f32 slope
    out = F.leaky_relu(h + fin, slope32)
    out.backward(gy)
    nhwc = lambda x: x.detach().permute(0, 2, 3, 1).contiguous()
    ref = R.iac_bwd_sac_reference(nhwc(gy), nhwc(out), nhwc(v), nhwc(s), nhwc(k1), slope)
    close("gfin", ref["gfin"][0], nhwc(fin.grad))
    close("gv", ref["gv"][0], nhwc(v.grad))
    close("gK", ref["gK"][0], nhwc(k1.grad))
    g0, k0 = rnd(g, B, H, W, C), rnd(g, B, H, W, 3 * C)
    acc = R.iac_bwd_sac_reference(nhwc(gy), nhwc(out), nhwc(v), nhwc(s), nhwc(k1), slope, gfin0=g0, gk0=k0)
    close("gfin +=", acc["gfin"][0], ref["gfin"][0] + g0)
    close("gK +=", acc["gK"][0], ref["gK"][0] + k0)
    close("S gK +=", acc["gK"][1], ref["gK"][1] + k0.abs())


@pytest.mark.parametrize("slope", [0.25, 0.0, -0.5])
def test_prelu_reference_vs_autograd(slope):
    g = torch.Generator().manual_seed(400)
    x = rnd(g, 2, 3, 4, 5)
    x.view(-1)[::7] = 0.0
    x.requires_grad_()
    a = torch.tensor([slope], dtype=D, requires_grad=True)
    go = rnd(g, 2, 3, 4, 5)
    y = F.prelu(x, a)
    y.backward(go)
    ref = R.prelu_reference(x, a, go)
    close("y", ref["y"], y.detach())
    close("gx", ref["gx"], x.grad)
    close("gslope", ref["gslope"][0], a.grad)


@pytest.mark.parametrize("B,C,h,w", [(1, 4, 1, 1), (2, 4, 1, 5), (1, 8, 5, 1), (2, 4, 3, 7)])
def test_xscale_references_vs_autograd(B, C, h, w):
    g = torch.Generator().manual_seed(500 + h * w)
    H, W = 2 * h, 2 * w
    x, Rr = rnd(g, B, C, H, W), rnd(g, B, C, H, W)
    dn, up = rnd(g, B, C, 2 * H, 2 * W).requires_grad_(), rnd(g, B, C, h, w).requires_grad_()
    go = rnd(g, B, C, H, W)
    pd = F.interpolate(dn, scale_factor=0.5, mode="bilinear", align_corners=False)
    pu = F.interpolate(up, scale_factor=2.0, mode="bilinear", align_corners=False)
    close("pool2", R.pool2_forward(dn), pd.detach())
    close("up2", R.up2_forward(up), pu.detach())
    (x + 2.0 * Rr + pd + pu).backward(go)
    close("pool2_adjoint", R.pool2_adjoint(go), dn.grad)
    ref, S, n = R.up2_adjoint(go)
    close("up2_adjoint", ref, up.grad)
    assert bool((S >= ref.abs() * (1 - 1e-12)).all()) and n == 16
    for d_, u_, rs in ((None, up, 2.0), (dn, up, 1.0), (dn, None, 2.0)):
        want = x + rs * Rr + (pd if d_ is not None else 0) + (pu if u_ is not None else 0)
        close("xscale", R.xscale_forward(x, Rr, rs, d_, u_)[0], want.detach())


@pytest.mark.parametrize("B,C,H,Wf", [(1, 8, 3, 1), (2, 8, 7, 2), (1, 12, 9, 6), (2, 4, 5, 5)])
def test_corr_lookup_reference_vs_autograd(B, C, H, Wf):
    from fcvsr_amd.train import graph as G
    g = torch.Generator().manual_seed(600 + H * Wf)
    a, b = rnd(g, B, C, H, Wf).requires_grad_(), rnd(g, B, C, H, Wf).requires_grad_()
    go = rnd(g, B, 81, H, Wf)
    y = G._corr_lookup(a, b)
    y.backward(go)
    ref = R.corr_lookup_reference(a, b, 4, go)
    close("corr", ref["corr"], y.detach())
    close("gx1", ref["gx1"], a.grad)
    close("gx2", ref["gx2"], b.grad)
    assert bool((ref["gx1"][:, ~ref["touched"]] == 0).all()) and bool((a.grad[:, ~ref["touched"]] == 0).all())


def test_gpu_test_inputs_converge_away_from_the_kinks():
    """Every (shape, seed) of tests/test_train_blocks_gpu.py: after at most R.ROUNDS resampling rounds no LeakyReLU argument r + add, no
    bottleneck t and no hidden pre-activation of the DivEnh gate is within R.MARGIN of zero in the f64 reference."""
    for s in R.RCB_SHAPES:
        assert R.rcb_inputs(*s)[1] == 0, s
    for stress in R.RCB_STRESS:
        for identity in (False, True):
            assert R.rcb_inputs(*R.RCB_STRESS_SHAPE, stress=stress, identity=identity)[1] == 0, (stress, identity)
    for c in R.DIVENH_CASES:
        assert R.divenh_inputs(*c)[1] == 0, c
