"""fcvsr_iac_bwd_warp_det (atomic-free backward of the IAC warp: source pass, stable sort, ordered gather) at operator level and
through `blocks.iac_both(..., deterministic=True)`: bit-equal g_off, bit-repeatable g_prev, values against an exact f64 reference with
the textbook bound of an n-term f32 sum, and against the scatter form."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                   # unit round-off of f32
SHAPES = [(2, 24, 20), (3, 17, 33), (1, 64, 64)]
FIELDS = ["smooth", "wild", "collapsed"]


def _offsets(kind, B, H, W, g):
    """(B,2,H,W) f32 offset field on the host (channel 0 = x, channel 1 = y)."""
    if kind == "smooth":
        return 0.7 * torch.randn(B, 2, H, W, generator=g)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    if kind == "collapsed":                      # every pixel of an image samples one interior fractional position
        off = torch.empty(B, 2, H, W)
        for b in range(B):
            off[b, 0] = (0.37 * W + 0.3 + b) - xs[b]
            off[b, 1] = (0.61 * H + 0.7 - b) - ys[b]
        return off
    assert kind == "wild"
    off = max(H, W) * torch.randn(B, 2, H, W, generator=g)
    flat = off.view(-1)
    n = flat.numel()
    pick = torch.randperm(n, generator=g)
    k = max(4, n // 16)
    flat[pick[:k]] = flat[pick[:k]].round()                                           # exact integers
    flat[pick[k:k + k // 4]] = 1e9
    flat[pick[k + k // 4:k + k // 2]] = -1e9
    # sampling positions exactly on -1, 0, W-1, W (x) and -1, 0, H-1, H (y)
    pp = torch.randperm(B * H * W, generator=g)[:max(8, B * H * W // 8)]
    for j, p in enumerate(pp.tolist()):
        b, y, x = p // (H * W), (p // W) % H, p % W
        off[b, 0, y, x] = float((-1, 0, W - 1, W)[j % 4] - x)
        if j % 3 == 0:
            off[b, 1, y, x] = float((-1, 0, H - 1, H)[(j // 4) % 4] - y)
        elif j % 3 == 1:
            off[b, 1, y, x] = 0.25 * (j % 7)
    return off


def _inputs(kind, B, H, W, C, seed, centre_tap=False):
    """Host tensors: gv, prev (B,H,W,C); Kbig (B,H,W,2*6C) whose channels [6C, 9C) are k1; offbig (B,4,H,W) whose planes 1:3 are off."""
    g = torch.Generator().manual_seed(seed)
    gv = torch.randn(B, H, W, C, generator=g) * torch.exp(3.0 * torch.randn(B, H, W, 1, generator=g))     # wide dynamic range
    prev = torch.randn(B, H, W, C, generator=g)
    Kbig = 0.5 * torch.randn(B, H, W, 12 * C, generator=g)
    if centre_tap:
        k1 = torch.zeros(B, H, W, C, 3)
        k1[..., 1] = 1.0
        Kbig[..., 6 * C:9 * C] = k1.reshape(B, H, W, 3 * C)
    offbig = torch.randn(B, 4, H, W, generator=g)
    offbig[:, 1:3] = _offsets(kind, B, H, W, g)
    return gv, prev, Kbig, offbig


def _views(Kbig, offbig, C):
    """k1 and off as the strided views `_IacFn` hands to the library."""
    return Kbig[..., 6 * C:9 * C], offbig[:, 1:3].permute(0, 2, 3, 1)


def _workspace(B, H, W, C, dev="cuda"):
    from fcvsr_amd import hip
    n = ctypes.c_size_t(0)
    hip.check(hip.lib().fcvsr_iac_bwd_warp_det_workspace(B, H, W, C, ctypes.byref(n)), "fcvsr_iac_bwd_warp_det_workspace")
    assert n.value >= B * H * W * (C * 4 + 16)                    # g_s, keys and ids twice
    return torch.empty(n.value, dtype=torch.uint8, device=dev)


def _run(det, gv, prev, Kbig, offbig, C, fill=None, ws=None):
    """One call of fcvsr_iac_bwd_warp_det (det) or of fcvsr_iac_bwd_warp on device copies of the inputs -> (gprev, goff)."""
    from fcvsr_amd import hip
    L = hip.lib()
    B, H, W, _ = gv.shape
    gv, prev, Kbig, offbig = (t.cuda() for t in (gv, prev, Kbig, offbig))
    k1, off = _views(Kbig, offbig, C)
    kv, ov = hip.view(k1), hip.view(off)
    goff = torch.empty(B, H, W, 2, device="cuda")
    if det:
        gprev = torch.full((B, H, W, C), float("nan") if fill is None else fill, device="cuda")
        ws = _workspace(B, H, W, C) if ws is None else ws
        hip.check(L.fcvsr_iac_bwd_warp_det(gv.data_ptr(), ctypes.byref(kv), prev.data_ptr(), ctypes.byref(ov), B, H, W, C, gprev.data_ptr(),
                                           goff.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()), "fcvsr_iac_bwd_warp_det")
    else:
        gprev = torch.zeros(B, H, W, C, device="cuda")
        hip.check(L.fcvsr_iac_bwd_warp(gv.data_ptr(), ctypes.byref(kv), prev.data_ptr(), ctypes.byref(ov), B, H, W, C, gprev.data_ptr(),
                                       goff.data_ptr(), hip.stream_ptr()), "fcvsr_iac_bwd_warp")
    torch.cuda.synchronize()
    return gprev, goff


def _gs_f64(gv, k1):
    """g_s = transposed vertical 3-tap pass of g_v with replicate padding, in f64 (k1: (B,H,W,3C), channel c's taps at 3c + t)."""
    B, H, W, C = gv.shape
    g = gv.double()
    k = k1.double().reshape(B, H, W, C, 3)
    gs = g * k[..., 1]
    gs[:, :-1] += g[:, 1:] * k[:, 1:, :, :, 0]
    gs[:, 1:] += g[:, :-1] * k[:, :-1, :, :, 2]
    gs[:, 0] += g[:, 0] * k[:, 0, :, :, 0]
    gs[:, -1] += g[:, -1] * k[:, -1, :, :, 2]
    return gs


def _reference(gs, off, f32_products):
    """Per destination element the f64 sum R of the bilinear contributions w * g_s, the f64 sum S of their magnitudes and the
    addend count n.  The four weights per source are computed in f32 with the kernel's expressions (fx = x + off; w1 = fx - floor(fx);
    w0 = 1 - w1; w = wy * wx); with f32_products the product w * g_s is rounded to f32 first, as the kernel adds it."""
    B, H, W, C = gs.shape
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    fx, fy = xs + off[..., 0].float(), ys + off[..., 1].float()
    x0f, y0f = torch.floor(fx), torch.floor(fy)
    wx1, wy1 = fx - x0f, fy - y0f
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    sane = (fx > -2.0) & (fx < W + 1.0) & (fy > -2.0) & (fy < H + 1.0)
    x0 = torch.where(sane, x0f, torch.full_like(x0f, -4.0)).long()
    y0 = torch.where(sane, y0f, torch.full_like(y0f, -4.0)).long()
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    R = torch.zeros(B * H * W, C, dtype=torch.float64)
    S = torch.zeros(B * H * W, C, dtype=torch.float64)
    n = torch.zeros(B * H * W, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            w = ((wy1 if dy else wy0) * (wx1 if dx else wx0))[ok]                     # f32 product, as the kernel
            idx = ((bi * H + yi) * W + xi)[ok]
            src = gs[ok]
            if f32_products:
                p = (w.unsqueeze(1) * src.float()).double()
            else:
                p = w.double().unsqueeze(1) * src.double()
            R.index_add_(0, idx, p)
            S.index_add_(0, idx, p.abs())
            n.index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    return R.view(B, H, W, C), S.view(B, H, W, C), n.view(B, H, W, 1)


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C", [32, 64])
def test_goff_bits_and_repeatable_gprev(C, B, H, W, kind):
    """g_off has the bits of the scatter form's; two calls - the second on freshly allocated inputs and workspace after unrelated work
    on the stream - give the same g_prev bits; a NaN-filled g_prev comes back without NaN, exactly 0 where no source lands."""
    inp = _inputs(kind, B, H, W, C, seed=100 + C + H)
    gp_a, goff_a = _run(False, *inp, C)
    gp1, goff1 = _run(True, *inp, C)
    assert torch.equal(goff1, goff_a)
    junk = torch.randn(512, 512, device="cuda")
    junk = (junk @ junk).relu_()                                                      # unrelated work, other allocations
    hold = [torch.empty(n, device="cuda") for n in (1000, 70000, 333)]               # shift what the allocator hands out next
    gp2, goff2 = _run(True, *(t.clone() for t in inp), C, fill=float("nan"))
    del hold
    assert torch.equal(gp1, gp2)
    assert torch.equal(goff1, goff2)
    assert not torch.isnan(gp1).any()
    _, _, n = _reference(inp[0], _views(inp[2], inp[3], C)[1], True)
    empty = (n == 0).expand(B, H, W, C)
    assert bool((gp1.cpu()[empty] == 0).all())
    if kind == "smooth":
        assert float(n.max()) >= 3 and int((n == 0).sum()) < B * H * W // 4          # the case is what it says
    if kind == "collapsed":
        assert int((n > 0).sum()) == 4 * B and float(n.max()) == H * W


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C", [32, 64])
def test_gprev_against_exact_reference(C, B, H, W, kind):
    """k1 = 1 on the centre tap, 0 elsewhere: g_s is g_v bit for bit, so the f32 products the kernel adds can be restated exactly.
    Required: |g_prev - R| <= n * 2^-24 * S element-wise (R, S: f64 sums of the products and of their magnitudes, n: their count) - the
    bound (n - 1) u S of adding n floats in any order, with one u S of room.  Derived, not tuned."""
    gv, prev, Kbig, offbig = _inputs(kind, B, H, W, C, seed=200 + C + W, centre_tap=True)
    gp, _ = _run(True, gv, prev, Kbig, offbig, C)
    R, S, n = _reference(gv, _views(Kbig, offbig, C)[1], True)
    err = (gp.cpu().double() - R).abs()
    bound = n * U * S
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"C={C} ({B},{H},{W}) {kind}: worst |g_prev - R| / (n u S) = {worst:.3f}, n up to {int(n.max())}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C", [32, 64])
def test_gprev_against_the_scatter_form(C, B, H, W, kind):
    """Random k1: both forms add the same f32 products, each is within n u S of the exact sum, so they are within 2 n u S of each
    other (S, n from an f64 restatement of g_s in the test, hence the factor 1 + 1e-3)."""
    gv, prev, Kbig, offbig = _inputs(kind, B, H, W, C, seed=300 + C + B)
    gp_d, _ = _run(True, gv, prev, Kbig, offbig, C)
    gp_a, _ = _run(False, gv, prev, Kbig, offbig, C)
    k1, off = _views(Kbig, offbig, C)
    _, S, n = _reference(_gs_f64(gv, k1), off, False)
    err = (gp_d.cpu().double() - gp_a.cpu().double()).abs()
    bound = 2 * n * U * S * (1 + 1e-3)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"C={C} ({B},{H},{W}) {kind}: worst |det - scatter| / (2 n u S) = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    assert float(gp_d.abs().max()) > 0


def test_argument_errors_launch_nothing():
    """Too small / null / misaligned workspace, C = 48, an offset view with one channel: negative code, a message, outputs untouched."""
    from fcvsr_amd import hip
    L = hip.lib()
    B, H, W, C = 1, 8, 12, 64
    gv, prev, Kbig, offbig = (t.cuda() for t in _inputs("smooth", B, H, W, C, seed=5))
    k1, off = _views(Kbig, offbig, C)
    ws = _workspace(B, H, W, C)
    gprev = torch.full((B, H, W, C), 7.0, device="cuda")
    goff = torch.full((B, H, W, 2), 7.0, device="cuda")

    def call(k1=k1, off=off, C=C, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), gv=gv):
        kv, ov = hip.view(k1), hip.view(off)
        return L.fcvsr_iac_bwd_warp_det(gv.data_ptr(), ctypes.byref(kv), prev.data_ptr(), ctypes.byref(ov), B, H, W, C, gprev.data_ptr(),
                                        goff.data_ptr(), ws_ptr, ws_bytes, hip.stream_ptr())

    K48 = torch.randn(B, H, W, 3 * 48, device="cuda")
    cases = {"small workspace": dict(ws_bytes=ws.numel() - 1), "null workspace": dict(ws_ptr=None),
             "misaligned workspace": dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4),
             "C = 48": dict(C=48, k1=K48, gv=torch.randn(B, H, W, 48, device="cuda")),
             "one offset channel": dict(off=offbig[:, 1:2].permute(0, 2, 3, 1))}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc < 0, (what, rc)
        msg = L.fcvsr_last_error().decode()
        assert "fcvsr_iac_bwd_warp_det" in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((gprev == 7.0).all()) and bool((goff == 7.0).all()), what
    n = ctypes.c_size_t(123)
    assert L.fcvsr_iac_bwd_warp_det_workspace(B, H, W, 48, ctypes.byref(n)) < 0 and n.value == 123
    assert L.fcvsr_iac_bwd_warp_det_workspace(1 << 12, 1 << 10, 1 << 10, 64, ctypes.byref(n)) < 0          # cells do not fit the key
    assert "fcvsr_iac_bwd_warp_det_workspace" in L.fcvsr_last_error().decode()
    assert call() == 0                                                                 # and the good call still runs
    torch.cuda.synchronize()
    assert not bool((gprev == 7.0).any())


def _iac_case(B, C, H, W, A, g):
    cl = dict(memory_format=torch.channels_last)
    x1 = torch.randn(B, C, H, W, generator=g).cuda().contiguous(**cl)
    x3 = torch.randn(B, C, H, W, generator=g).cuda().contiguous(**cl)
    K0 = (torch.randn(B, A * 6 * C, H, W, generator=g) * 0.4).cuda().contiguous(**cl)
    offs0 = [(torch.randn(B, 2, H, W, generator=g) * 2.5).cuda() for _ in range(2 * A)]
    go = [torch.randn(B, C, H, W, generator=g).cuda() for _ in range(2)]
    return x1, x3, K0, offs0, go


def _iac_grads(case, A, C, mode):
    """outputs and gradients of both IAC directions: mode "torch" = the operator chain of graph.py, else iac_both(deterministic=mode)"""
    from fcvsr_amd.train import graph as G
    from fcvsr_amd.train.blocks import iac_both
    x1, x3, K0, offs0, go = case
    a, b, K = (t.clone().requires_grad_(True) for t in (x1, x3, K0))
    offs = [o.clone().requires_grad_(True) for o in offs0]
    if mode == "torch":
        outs = []
        for feat_in, ofs in ((a, offs[:A]), (b, offs[A:])):
            feat = feat_in
            for i in range(A):
                k1 = K[:, i * 6 * C: i * 6 * C + 3 * C]
                feat = G._lrelu(G._sac(G._warp(feat, ofs[i]), k1) + feat_in, 0.1)
            outs.append(feat)
        yf, yb = outs
    else:
        yf, yb = iac_both(a, b, K, offs[:A], offs[A:], 0.1, deterministic=mode)
    (yf * go[0]).sum().backward(retain_graph=True)
    (yb * go[1]).sum().backward()
    torch.cuda.synchronize()
    return [yf.detach(), yb.detach(), a.grad, b.grad, K.grad] + [o.grad for o in offs]


def test_iac_both_deterministic_matches_torch_ops_and_repeats():
    """iac_both(..., deterministic=True) against the torch-operator chain of test_iac_fused_matches_torch_ops (same inputs, same metric,
    the same 5e-5), and two backward passes with bit-equal gradients for the features, the kernels and every offset field."""
    g = torch.Generator().manual_seed(21)
    for (B, C, H, W, A) in ((2, 64, 12, 20, 3), (1, 32, 9, 7, 2)):
        case = _iac_case(B, C, H, W, A, g)
        ref = _iac_grads(case, A, C, "torch")
        det1 = _iac_grads(case, A, C, True)
        det2 = _iac_grads(case, A, C, True)
        names = ["yf", "yb", "g_x1", "g_x3", "g_K"] + [f"g_off{i}" for i in range(2 * A)]
        for name, u, v, w in zip(names, ref, det1, det2):
            scale = max(float(u.abs().max()), 1e-12)
            err = float((u - v).abs().max()) / scale
            assert err <= 5e-5, f"{name} ({B},{C},{H},{W}): {err:.2e}"
            assert torch.equal(v, w), name


def test_above_one_million_pixels():
    """1032 x 1024 pixels: above 2^20 keys the library sort switches from its merge sort to its one-sweep radix sort, which must be
    stable and repeatable too - same g_off bits as the scatter form, two calls bit-equal, g_prev within 2 n u S of the scatter form."""
    B, H, W, C = 1, 1032, 1024, 32
    inp = _inputs("smooth", B, H, W, C, seed=77)
    gp1, goff1 = _run(True, *inp, C)
    gp2, _ = _run(True, *(t.clone() for t in inp), C)
    gpa, goffa = _run(False, *inp, C)
    assert torch.equal(gp1, gp2) and torch.equal(goff1, goffa) and not torch.isnan(gp1).any()
    k1, off = _views(inp[2], inp[3], C)
    _, S, n = _reference(_gs_f64(inp[0], k1), off, False)
    assert bool(((gp1.cpu().double() - gpa.cpu().double()).abs() <= 2 * n * U * S * (1 + 1e-3)).all())
