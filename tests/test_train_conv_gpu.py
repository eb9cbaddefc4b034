"""GPU: every branch of the training convolution (fcvsr_amd.train.conv2d / conv2d_levels) against a float64 CPU reference whose
operands are rounded exactly as each direction's kernel rounds them.

Rounding per direction (ops._run_conv / _Conv2dFn.backward / the kernels' conversions):
  forward         x and w in the mode's 16-bit dtype on the matrix-core path (1x1 / 3x3, stride 1, cin % 4 == 0, cout % 4 == 0 or < 4),
                  f32 otherwise;
  input gradient  gp and w in the mode's dtype when the transposed layer is matrix-core eligible, f32 otherwise;
  weight gradient x and gp in bf16 in BOTH 16-bit modes on the matrix-core path (3x3 / 1x1, stride 1, channels multiples of 64),
                  f32 otherwise (cout-1, 4-channel and exact slab kernels);
  bias gradient   f32.
gp (the gradient at the pre-activation) is computed as fcvsr_act_bwd does: f32 gy times 1 or the f32 slope, the mask taken from the
kernel's own saved output (y > 0), so near-zero pre-activations cannot flip between kernel and reference.

Every entry is bounded by its own condition:  |got - ref| <= tau(n) * S,  S = the same operation in f64 on the absolute values of the
rounded operands, n = the number of products summed into the entry, tau(n) = 2^-16 for n <= 4096 and 2^-22 sqrt(n) above.  The bound
allows f32 accumulation noise with margin, is far below bf16 rounding (2^-9), and is derived, not measured: at the small shapes one
missing or duplicated product exceeds it, at the large ones a missing tile does.  Each case prints its worst err / S per direction
next to tau(n) (run with -s)."""
import ctypes as C
import contextlib
import zlib

import pytest
import torch
import torch.nn.functional as F

from tolerance import tau, worst_ratio

pytestmark = pytest.mark.gpu

MMA = {"bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# which operands each direction rounds (mirrors the dispatch in fcvsr_amd/train/ops.py; a wrong guess fails the bound by ~2^7)

def fwd_dtype(prec, cin, cout, k, stride):
    ok = prec in MMA and k in (1, 3) and stride == 1 and cin % 4 == 0 and (cout % 4 == 0 or cout < 4)
    return MMA[prec] if ok else None


def dx_dtype(prec, cin, cout, k):
    # dL/dx is a stride-1 convolution of the (zero-inserted) gp with the transposed weight: the channel roles swap
    ok = prec in MMA and k in (1, 3) and cout % 4 == 0 and (cin % 4 == 0 or cin < 4)
    return MMA[prec] if ok else None


def dw_dtype(prec, cin, cout, k, stride):
    if cout == 1 and k == 3 and stride == 1 and cin in (16, 32, 64):
        return None                                        # fcvsr_wgrad_cout1: f32
    ok = prec in MMA and k in (1, 3) and stride == 1 and cin % 64 == 0 and cout % 64 == 0
    return torch.bfloat16 if ok else None                  # fcvsr_conv2d_wgrad_mfma rounds to bf16 whatever the mode


def rounded(t, dt):
    """f32 tensor -> f64 tensor of its values rounded to `dt` (round to nearest even), or exact when dt is None."""
    return (t if dt is None else t.to(dt)).double()


def act_f64(pre, act):
    if act is None:
        return pre
    return torch.where(pre > 0, pre, pre * (SLOPE if act == "lrelu" else 0.0))


def gp_like_kernel(gy, y_kernel, act):
    """fcvsr_act_bwd: f32 gy * (y > 0 ? 1 : slope) in f32, the mask from the kernel's saved output."""
    if act is None:
        return gy
    s = torch.tensor(SLOPE if act == "lrelu" else 0.0, dtype=torch.float32)
    return torch.where(y_kernel > 0, gy, gy * s)


def reference(prec, x, w, b, gy, y_kernel, stride, act):
    """f64 reference and condition of every direction: dict name -> (ref, S, n)."""
    cout, cin, k, _ = w.shape
    pad = k // 2
    B = x.shape[0]
    Ho, Wo = gy.shape[2], gy.shape[3]
    out = {}
    fd = fwd_dtype(prec, cin, cout, k, stride)
    xf, wf = rounded(x, fd), rounded(w, fd)
    bd = None if b is None else b.double()
    pre = F.conv2d(xf, wf, bd, stride, pad)
    S = F.conv2d(xf.abs(), wf.abs(), None if b is None else bd.abs(), stride, pad)
    out["y"] = (act_f64(pre, act), S, cin * k * k)
    gp = gp_like_kernel(gy, y_kernel, act)
    dd = dx_dtype(prec, cin, cout, k)
    gq, wq = rounded(gp, dd), rounded(w, dd)
    out["dx"] = (torch.nn.grad.conv2d_input(x.shape, wq, gq, stride, pad),
                 torch.nn.grad.conv2d_input(x.shape, wq.abs(), gq.abs(), stride, pad), cout * k * k)
    wd = dw_dtype(prec, cin, cout, k, stride)
    xq, gq = rounded(x, wd), rounded(gp, wd)
    out["dw"] = (torch.nn.grad.conv2d_weight(xq, w.shape, gq, stride, pad),
                 torch.nn.grad.conv2d_weight(xq.abs(), w.shape, gq.abs(), stride, pad), B * Ho * Wo)
    if b is not None:
        g64 = gp.double()
        out["db"] = (g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3)), B * Ho * Wo)
    return out


def check(tag, got: dict, refs: dict):
    """Every direction within its bound; prints the worst err / S of each next to its tau(n)."""
    ratios, bad = {}, {}
    for name, (ref, S, n) in refs.items():
        assert got[name] is not None, f"{tag}: no {name}"
        assert tuple(got[name].shape) == tuple(ref.shape), (tag, name, tuple(got[name].shape), tuple(ref.shape))
        ratios[name] = (worst_ratio(got[name], ref, S), tau(n))
        if not ratios[name][0] <= ratios[name][1]:
            bad[name] = ratios[name]
    print(f"[{tag}] worst err/S (tau): " + "  ".join(f"{k} {r:.2e} ({t:.1e})" for k, (r, t) in ratios.items()))
    assert not bad, f"{tag}: bound exceeded (worst err/S, tau) {bad}"


def make(seed, B, cin, cout, k, H, W, bias, wscale=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (wscale or (cin * k * k) ** 0.5)
    b = torch.randn(cout, generator=g) if bias else None
    return g, x, w, b


def run(prec, x, w, b, gy, stride, act, *, g0w=None, g0b=None, accumulate=False, x_grad=True):
    """fcvsr_amd.train.conv2d forward + backward on the GPU; returns y, dx, w.grad, b.grad (CPU) and the kernel's output."""
    from fcvsr_amd.train import conv2d
    from fcvsr_amd.train.ops import accumulate_into_grad
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(x_grad)
    wd = w.cuda().requires_grad_(True)
    bd = None if b is None else b.cuda().requires_grad_(True)
    if g0w is not None:
        wd.grad = g0w.cuda().clone()
    if g0b is not None:
        bd.grad = g0b.cuda().clone()
    y = conv2d(xd, wd, bd, stride, prec, act, SLOPE if act == "lrelu" else 0.0)
    preset = [t.grad for t in (wd, bd) if t is not None and t.grad is not None]
    with (accumulate_into_grad(*preset) if accumulate else contextlib.nullcontext()):
        y.backward(gy.cuda())
    torch.cuda.synchronize()
    yc = y.detach().float().cpu()
    got = dict(y=yc, dx=xd.grad.cpu() if x_grad else None, dw=wd.grad.cpu())
    if b is not None:
        got["db"] = bd.grad.cpu()
    return got, yc


def conv_case(prec, cin, cout, k, stride, B, H, W, bias, act, seed, tag):
    g, x, w, b = make(seed, B, cin, cout, k, H, W, bias)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gy = torch.randn(B, cout, Ho, Wo, generator=g)
    got, yk = run(prec, x, w, b, gy, stride, act)
    check(tag, got, reference(prec, x, w, b, gy, yk, stride, act))


# (cin, cout, k, stride, B, H, W, bias, act): together they run every branch of _run_conv and _Conv2dFn.backward
CASES = {
    "64-64-k3": (64, 64, 3, 1, 3, 13, 37, True, "lrelu"),          # matrix cores in every direction (16-bit modes)
    "64-64-k3-plain": (64, 64, 3, 1, 1, 6, 10, False, None),
    "64-128-k1": (64, 128, 1, 1, 3, 7, 19, True, "relu"),
    "128-128-k3": (128, 128, 3, 1, 1, 9, 35, True, "lrelu"),       # several cin and cout blocks
    "64-1": (64, 1, 3, 1, 3, 11, 13, True, None),                  # fcvsr_wgrad_cout1; 16-bit: the padded 4-channel forward
    "32-1": (32, 1, 3, 1, 1, 10, 6, True, "lrelu"),
    "16-1": (16, 1, 3, 1, 3, 7, 9, False, None),
    "64-1-relu-odd": (64, 1, 3, 1, 1, 3, 5, True, "relu"),          # act on an odd number of outputs
    "64-2-lrelu": (64, 2, 3, 1, 3, 5, 9, True, "lrelu"),            # 16-bit: strided view of the 4-channel output saved for act
    "64-3-relu": (64, 3, 3, 1, 1, 10, 6, False, "relu"),
    "64-5-lrelu-odd": (64, 5, 3, 1, 1, 3, 5, True, "lrelu"),        # B*H*W*cout = 75: not a multiple of 4
    "4-4-k1": (4, 4, 1, 1, 3, 11, 9, True, "lrelu"),               # wgrad_c4_kernel<1>, <3>, <5>
    "4-4-k3": (4, 4, 3, 1, 1, 13, 10, True, None),
    "4-4-k5": (4, 4, 5, 1, 3, 7, 6, False, "relu"),
    "7-24": (7, 24, 3, 1, 3, 10, 15, True, "lrelu"),               # cin % 4 != 0: f32 in every mode
    "96-64": (96, 64, 3, 1, 1, 14, 22, True, "relu"),              # matrix-core forward, f32 weight gradient
    "64-64-k5": (64, 64, 5, 1, 1, 9, 11, True, None),              # k = 5: f32 fallback
    "64-64-s2": (64, 64, 3, 2, 3, 13, 19, True, "lrelu"),          # stride 2 at odd sizes: f32 forward, zero-inserted input gradient
    "16-8-s2": (16, 8, 3, 2, 1, 13, 19, False, None),
    "tiny-2x5": (64, 64, 3, 1, 1, 2, 5, True, "lrelu"),
    "tiny-1x3": (4, 4, 3, 1, 3, 1, 3, True, "relu"),
    "tiny-3x1": (64, 128, 1, 1, 1, 3, 1, False, None),
    "1x1-spatial": (64, 64, 3, 1, 3, 1, 1, True, "relu"),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_conv_matches_rounded_f64_reference(prec, name):
    cin, cout, k, stride, B, H, W, bias, act = CASES[name]
    conv_case(prec, cin, cout, k, stride, B, H, W, bias, act, seed=zlib.crc32(name.encode()) % 10007 + len(prec), tag=f"{prec} {name}")


def _mfma_slab_layout(B, H, W, cin, cout, k):
    """(slabs, tiles, tiles per slab, slabs that get a tile) of fcvsr_conv2d_wgrad_mfma, derived from its scratch size and the 4 x 32
    pixel tile."""
    from fcvsr_amd import hip
    slabs = hip.lib().fcvsr_conv2d_wgrad_mfma_scratch_elems(B, H, W, cin, cout, k, k) // (k * k * cin * cout + cout)
    tiles = B * ((H + 3) // 4) * ((W + 31) // 32)
    per = (tiles + slabs - 1) // slabs
    return slabs, tiles, per, (tiles + per - 1) // per


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 128)])
def test_conv_large_multi_tile_slabs(prec, cin, cout):
    """B = 2 at 132 x 140: in the 16-bit modes the matrix-core weight gradient gives several tiles to a slab and leaves slabs without
    a tile (they must still write zero partials)."""
    B, H, W = 2, 132, 140
    slabs, tiles, per, used = _mfma_slab_layout(B, H, W, cin, cout, 3)
    print(f"{cin}->{cout}: {tiles} tiles over {slabs} slabs, {per} per slab, {slabs - used} empty")
    assert per >= 2 and used < slabs, (tiles, slabs, per, used)
    conv_case(prec, cin, cout, 3, 1, B, H, W, True, "lrelu" if cin == 64 else None, seed=cin + len(prec),
              tag=f"{prec} large {cin}-{cout}")


@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_conv_large_cout1_many_rows_per_block(prec):
    """fcvsr_wgrad_cout1 with B*H > 1024 rows: several rows per block."""
    from fcvsr_amd import hip
    B, H, W, cin = 3, 347, 40, 64
    assert hip.lib().fcvsr_wgrad_cout1_scratch_elems(B, H, cin) == 1024 * 9 * cin and B * H > 1024
    conv_case(prec, cin, 1, 3, 1, B, H, W, True, None, seed=347 + len(prec), tag=f"{prec} large 64-1")


def test_conv_large_f32_slab_cap():
    """fcvsr_conv2d_wgrad with more than 96 * 512 pixels: the slab count is capped at 96, slabs hold more than 512 pixels."""
    from fcvsr_amd import hip
    B, H, W, cin, cout = 1, 230, 220, 7, 24
    slabs = hip.lib().fcvsr_conv2d_wgrad_scratch_elems(B, H, W, cin, cout, 3, 3) // (9 * cin * cout)
    assert slabs == 96 and (B * H * W + 511) // 512 > 96
    conv_case("f32", cin, cout, 3, 1, B, H, W, True, "lrelu", seed=96, tag="f32 large 7-24")


# ---------------------------------------------------------------------------------------------------------------------------------
# conv2d_levels: one layer applied to three pyramid levels (grouped launches in the 16-bit modes)

LEVEL_SETS = {
    "64-64-k3": (64, 64, 3, 2, [(12, 20), (6, 10), (3, 5)]),
    "64-128-k1": (64, 128, 1, 1, [(9, 13), (5, 7), (3, 3)]),
    "64-64-k3-large": (64, 64, 3, 2, [(132, 140), (66, 70), (33, 35)]),
}


def levels_inputs(name, seed):
    cin, cout, k, B, sizes = LEVEL_SETS[name]
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, cin, h, w, generator=g) for h, w in sizes]
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    gys = [torch.randn(B, cout, h, w, generator=g) for h, w in sizes]
    return xs, w, b, gys


def run_levels(prec, xs, w, b, gys, *, g0w=None, g0b=None, accumulate=False, x_grad=True):
    from fcvsr_amd.train.ops import conv2d_levels
    from fcvsr_amd.train.ops import accumulate_into_grad
    xds = [x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(x_grad) for x in xs]
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    if g0w is not None:
        wd.grad = g0w.cuda().clone()
    if g0b is not None:
        bd.grad = g0b.cuda().clone()
    ys = conv2d_levels(xds, wd, bd, prec, "lrelu", SLOPE)
    if prec in MMA:
        assert type(ys[0].grad_fn).__name__ == "_ConvLevelsFnBackward", "expected the grouped launches"
    preset = [t.grad for t in (wd, bd) if t.grad is not None]
    with (accumulate_into_grad(*preset) if accumulate else contextlib.nullcontext()):
        torch.autograd.backward(ys, [gy.cuda() for gy in gys])
    torch.cuda.synchronize()
    yks = [y.detach().float().cpu() for y in ys]
    got = dict(dw=wd.grad.cpu(), db=bd.grad.cpu())
    for i, y in enumerate(yks):
        got[f"y{i}"] = y
        if x_grad:
            got[f"dx{i}"] = xds[i].grad.cpu()
    return got, yks


def levels_reference(prec, xs, w, b, gys, yks):
    """Per level y and dx; dw and db summed over the levels (S and n summed too)."""
    refs, dw, db = {}, None, None
    for i, (x, gy, yk) in enumerate(zip(xs, gys, yks)):
        r = reference(prec, x, w, b, gy, yk, 1, "lrelu")
        refs[f"y{i}"], refs[f"dx{i}"] = r["y"], r["dx"]
        dw = r["dw"] if dw is None else tuple(a + c for a, c in zip(dw, r["dw"]))
        db = r["db"] if db is None else tuple(a + c for a, c in zip(db, r["db"]))
    refs["dw"], refs["db"] = dw, db
    return refs


@pytest.mark.parametrize("name", list(LEVEL_SETS))
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16"])
def test_conv_levels_matches_rounded_f64_reference(prec, name):
    if name.endswith("large"):
        cin, cout, k, B, sizes = LEVEL_SETS[name]
        slabs, tiles, per, used = _mfma_slab_layout(B, sizes[0][0], sizes[0][1], cin, cout, k)
        assert per >= 2 and used < slabs, (tiles, slabs, per, used)
    xs, w, b, gys = levels_inputs(name, seed=len(name) + len(prec))
    got, yks = run_levels(prec, xs, w, b, gys)
    check(f"{prec} levels {name}", got, levels_reference(prec, xs, w, b, gys, yks))


# ---------------------------------------------------------------------------------------------------------------------------------
# accumulate mode (TrainStep): the reductions ADD into an existing .grad; a parameter without .grad still gets a plain gradient

def _accumulate_configs(w, b, g):
    g0w = torch.randn(w.shape, generator=g)
    g0b = None if b is None else torch.randn(b.shape, generator=g)
    yield "w+b", g0w, g0b
    yield "w", g0w, None
    if b is not None:
        yield "b", None, g0b


def _with_g0(refs, name, g0):
    ref, S, n = refs[name]
    return (ref + g0.double(), S + g0.double().abs(), n)


@pytest.mark.parametrize("prec,name", [("f32", "64-1"), ("f32", "7-24"), ("f32", "4-4-k3"), ("f32", "64-64-k3"), ("bf16", "64-64-k3"),
                                       ("bf16", "64-1"), ("f16", "128-128-k3"), ("bf16", "96-64")])
def test_conv_accumulate_mode_adds_into_existing_grad(prec, name):
    """fcvsr_wgrad_cout1, fcvsr_conv2d_wgrad (slab and 4-channel kernels), the matrix-core weight gradient with its fused bias, and
    fcvsr_colsum: .grad == G0 + ref, i.e. the kernel adds (not writes) and autograd does not add the result a second time."""
    cin, cout, k, stride, B, H, W, _, act = CASES[name]
    if name == "4-4-k3":
        act = "lrelu"
    g, x, w, b = make(zlib.crc32(name.encode()) % 997, B, cin, cout, k, H, W, True)
    gy = torch.randn(B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g)
    for cfg, g0w, g0b in _accumulate_configs(w, b, g):
        got, yk = run(prec, x, w, b, gy, stride, act, g0w=g0w, g0b=g0b, accumulate=True, x_grad=False)
        refs = reference(prec, x, w, b, gy, yk, stride, act)
        refs = {n_: refs[n_] for n_ in ("dw", "db")}
        if g0w is not None:
            refs["dw"] = _with_g0(refs, "dw", g0w)
        if g0b is not None:
            refs["db"] = _with_g0(refs, "db", g0b)
        check(f"{prec} accumulate {name} grad set on {cfg}", got, refs)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_conv_levels_accumulate_mode_adds_into_existing_grad(prec):
    """fcvsr_conv2d_wgrad_mfma_groups and its fused bias in accumulate mode."""
    xs, w, b, gys = levels_inputs("64-64-k3", seed=11)
    g = torch.Generator().manual_seed(12)
    for cfg, g0w, g0b in _accumulate_configs(w, b, g):
        got, yks = run_levels(prec, xs, w, b, gys, g0w=g0w, g0b=g0b, accumulate=True, x_grad=False)
        refs = levels_reference(prec, xs, w, b, gys, yks)
        refs = {n_: refs[n_] for n_ in ("dw", "db")}
        if g0w is not None:
            refs["dw"] = _with_g0(refs, "dw", g0w)
        if g0b is not None:
            refs["db"] = _with_g0(refs, "db", g0b)
        check(f"{prec} accumulate levels grad set on {cfg}", {k_: got[k_] for k_ in ("dw", "db")}, refs)


# ---------------------------------------------------------------------------------------------------------------------------------

def test_first_layer_f16_training_path():
    """feat_extract in the 16-bit training modes (graph.forward_train): inputs k/255 zero-padded from 7 to 64 channels, precision "f16":
    forward with f16 x and w, weight gradient with bf16 x and gp.  Pinned against the rounded-operand reference; the error against the
    UNROUNDED f64 result is printed to keep this layer's real precision on record."""
    from fcvsr_amd.train import conv2d
    g = torch.Generator().manual_seed(255)
    B, T, H, W, cout = 2, 7, 20, 36, 448
    x7 = torch.randint(0, 256, (B, T, H, W), generator=g).float() / 255
    w7 = torch.randn(cout, T, 3, 3, generator=g) / (T * 9) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    x = torch.cat([x7, torch.zeros(B, 64 - T, H, W)], 1)
    w = F.pad(w7, (0, 0, 0, 0, 0, 64 - T))
    gy = torch.randn(B, cout, H, W, generator=g)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = conv2d(x.cuda().contiguous(memory_format=torch.channels_last), wd, bd, 1, "f16")
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu())
    refs = reference("f16", x, w, b, gy, got["y"], 1, None)
    refs = {n_: refs[n_] for n_ in ("y", "dw", "db")}
    check("first layer f16", got, refs)
    exact_y = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    exact_dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), 1, 1)
    ey = float((got["y"].double() - exact_y).abs().max()) / float(exact_y.abs().max())
    edw = float((got["dw"].double() - exact_dw).abs().max()) / float(exact_dw.abs().max())
    print(f"[first layer f16] against the unrounded f64 result: forward max-abs / max {ey:.2e}, dw {edw:.2e}")


def test_rejected_wgrad_call_writes_neither_dw_nor_dbias():
    """The bias gradient of the matrix-core weight gradient is an argument of the call: a call that rejects its arguments (cin = 48)
    writes neither dw nor dbias, and the next call without a bias (dbias = NULL) leaves that buffer alone and gives the right dw."""
    from fcvsr_amd import hip
    L = hip.lib()
    st = hip.stream_ptr()
    sentinel = torch.full((256,), 7.0, device="cuda")
    B, H, W, cout = 1, 8, 32, 64
    x48 = torch.randn(B, H, W, 48, device="cuda")
    gy = torch.randn(B, H, W, cout, device="cuda")
    dw48 = torch.zeros(cout * 48 * 9, device="cuda")
    n48 = 4 * (9 * 64 * cout + cout)
    scratch48 = torch.zeros(n48, device="cuda")
    xv, gv = hip.view(x48), hip.view(gy)
    rc = L.fcvsr_conv2d_wgrad_mfma(C.addressof(xv), C.addressof(gv), B, H, W, 3, 3, 1, 1, dw48.data_ptr(), sentinel.data_ptr(),
                                   scratch48.data_ptr(), n48, 0, 0, st)
    assert rc != 0, "cin = 48 must be rejected"
    torch.cuda.synchronize()
    assert torch.equal(dw48, torch.zeros_like(dw48))        # nothing launched
    assert torch.equal(sentinel, torch.full_like(sentinel, 7.0))
    x64 = torch.randn(B, H, W, 64, device="cuda")
    dw = torch.empty(cout * 64 * 9, device="cuda")
    n = L.fcvsr_conv2d_wgrad_mfma_scratch_elems(B, H, W, 64, cout, 3, 3)
    scratch = torch.empty(n, device="cuda")
    xv = hip.view(x64)
    hip.check(L.fcvsr_conv2d_wgrad_mfma(C.addressof(xv), C.addressof(gv), B, H, W, 3, 3, 1, 1, dw.data_ptr(), None, scratch.data_ptr(), n,
                                        0, 0, st), "fcvsr_conv2d_wgrad_mfma")
    torch.cuda.synchronize()
    assert torch.equal(sentinel, torch.full_like(sentinel, 7.0)), "a call without a bias wrote into the earlier call's bias buffer"
    ref = torch.nn.grad.conv2d_weight(x64.cpu().permute(0, 3, 1, 2).to(torch.bfloat16).double(), (cout, 64, 3, 3),
                                      gy.cpu().permute(0, 3, 1, 2).to(torch.bfloat16).double(), 1, 1)
    S = torch.nn.grad.conv2d_weight(x64.cpu().permute(0, 3, 1, 2).to(torch.bfloat16).double().abs(), (cout, 64, 3, 3),
                                    gy.cpu().permute(0, 3, 1, 2).to(torch.bfloat16).double().abs(), 1, 1)
    check("bias request", {"dw": dw.cpu().view(cout, 64, 3, 3)}, {"dw": (ref, S, B * H * W)})
