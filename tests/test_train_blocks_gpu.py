"""GPU: the hand-written non-convolution training blocks (fcvsr_amd/train/blocks.py: rcb_tail, divenh_band, prelu, xscale,
corr_lookup through their autograd wrappers, fcvsr_iac_bwd_sac through the C ABI) against the per-element float64 references of
tests/train_block_refs.py, at the shapes where their kernels change branch: HW = 1 / 255 / 256 / 257 around the 256-pixel block,
B * nblk = 28 / 29 / 32 / 33 / 36 / 65 partial rows around the eight-loads-in-flight loop of the final row sums, and sizes past the grid
caps of the apply kernels (1024 blocks) and of PReLU (2048 backward, 4096 forward).  Inputs are f32 from a seeded CPU generator;
every comparison is made on the CPU in f64; outputs the test owns are pre-filled with NaN, the wrappers' outputs must hold none.

Bounds, per entry:
  a sum                       |got - ref| <= tau(n) * S, S and n from the reference's triple (train_block_refs: what S is made of);
  elementwise, no statistic   (gz, Sf', the resampling adjoints, PReLU y / gx, corr_lookup, gfin) exact, or 2^-22 * terms * S;
  elementwise, through a pooled statistic and a softmax or sigmoid (out, gr, So', gf, gSf, gSo):  no derivable bound.  MEASURED holds
  the worst  |got - ref| / scale  found on an MI355X against the f64 reference, scale = the entry's own condition: the absolute values
  of its direct terms (>= |ref|, and not small where they cancel) plus the statistic's share (train_block_refs: `*_scale`).  The bound
  is 8 x the case's OWN measured worst (the table below is parsed into MEASURED, one figure per case and quantity): room for another
  expf rounding and another order of the two-stage sums, two to three orders below what one dropped block or pixel does at these
  shapes.

Measured on an MI355X, worst |got - ref| / scale per case in units of 1e-9, rounded up (the stress rows: `out` only, the forward is
what they check; run with -s for the figures of a run):
  rcb_tail                                          out       gr
    1x1x1                                          1.05     0.31
    3x1x1                                          1.17     0.40
    1x15x17                                        1.24    65.77
    3x5x51                                         1.47    90.30
    1x8x32                                         1.05    67.00
    3x4x64                                         1.42    69.04
    1x1x257                                        1.21    56.84
    3x257x1                                        1.92    91.68
    4x35x51                                        1.74   103.20
    1x67x107                                       1.68   114.50
    4x23x89                                        1.96   129.20
    3x15x187                                       2.20   118.90
    3x9x313                                        1.58    86.02
    5x7x439                                        1.84   104.80
    1x27x607                                       2.21   124.10
    accumulate 3x5x51                              1.47    90.30
    accumulate 1x67x107                            1.68   114.50
    accumulate 5x7x439                             1.84   104.80
    stress span40                                  0.30        -
    stress span40 identity                        80.60        -
    stress last_pixel                              0.83        -
    stress last_pixel identity                    65.38        -
    stress levels                                  1.56        -
    stress levels identity                        68.10        -
  divenh_band                                        So       gf      gSf      gSo
    C64 1x1x1                                     47.17    53.73    56.12    61.60
    C64 3x1x1                                     78.66    74.58    59.89    87.17
    C64 1x15x17                                   76.85   110.00    84.42   108.70
    C64 3x5x51                                   101.90   132.50   136.70   111.20
    C64 1x8x32                                    59.86   111.30    61.70   106.30
    C64 3x4x64                                    55.31   136.51    57.66   104.80
    C64 1x1x257                                   65.96   135.30    71.42   106.30
    C64 3x257x1                                  108.40   137.60    76.65   112.30
    C64 4x35x51                                  150.50   183.30   148.40   117.30
    C64 1x67x107                                 153.90   180.00   152.60   114.80
    C64 4x23x89                                   81.16   140.20    79.31   113.10
    C64 3x15x187                                 102.20   157.20   130.20   111.30
    C64 3x9x313                                  136.40   152.01   142.70   115.70
    C64 5x7x439                                  130.20   154.20   168.20   113.60
    C64 1x27x607                                 168.70   160.40   170.90   114.60
    C32 1x1x1                                     43.82    52.75    55.13    53.68
    C32 3x1x1                                     75.68    87.81    52.44    90.68
    C32 1x15x17                                  146.30   132.70   127.20   110.00
    C32 3x5x51                                   165.50   154.30   175.80   111.20
    C32 1x8x32                                   104.10   134.30   168.60   113.10
    C32 3x4x64                                   108.00   135.11    95.11   112.60
    C32 1x1x257                                  137.40   142.00   103.80   114.90
    C32 3x257x1                                  132.40   136.80   165.20   119.10
    C32 4x35x51                                  173.30   152.20   154.60   113.60
    C32 1x67x107                                 182.30   148.40   176.30   109.00
    C32 4x23x89                                  200.00   183.30   171.60   116.90
    C32 3x15x187                                 177.30   169.60   160.20   148.00
    C32 3x9x313                                  214.30   156.90   151.80   114.70
    C32 5x7x439                                  251.50   193.80   193.30   121.30
    C32 1x75x437                                 188.10   187.80   183.90   114.70
    accumulate C64 3x5x51                        101.90   132.50   136.70   111.20
    accumulate C32 1x67x107                      182.30   148.40   176.30   109.00
    accumulate C64 5x7x439                       130.20   154.20   168.20   113.60
The derived bounds, for comparison (worst err / S over all cases as a fraction of the bound, same run): rcb_tail dwmask 0.002, dw1 0.010,
dw2 0.009; divenh_band ga 0.21, gb 0.23, dw1 0.006, dw2 0.031 (the largest at HW = 1); iac_bwd_sac gfin 0.24, gv 0.012, gK 0.014; prelu
gslope 0.004; xscale out 0.17, gup 0.052; corr_lookup 0.53; the adjoint identities hold to 1.2e-8 of sum |u| |A^T g| (signed data), up2's to 1.1e-8 of the product (positive data)."""
import contextlib
import ctypes as C
import re

import pytest
import torch

import train_block_refs as R
from tolerance import tau, worst_ratio

pytestmark = pytest.mark.gpu

CL = dict(memory_format=torch.channels_last)
EXACT = 2.0 ** -22
FACTOR = 8.0


def _measured():
    """The docstring's table: {"<block> <case>": {quantity: worst ratio}}."""
    out, blk, cols = {}, None, None
    for line in __doc__.splitlines():
        m = re.match(r"  (rcb_tail|divenh_band) +(\S.*)$", line)
        if m:
            blk, cols = m.group(1), m.group(2).split()
            continue
        m = re.match(r"    (\S.*?)  +([\d. -]+)$", line)
        if m and blk:
            out[f"{blk} {m.group(1)}"] = {c: float(v) * 1e-9 for c, v in zip(cols, m.group(2).split()) if v != "-"}
    return out


MEASURED = _measured()


def check_sum(tag, name, got, triple):
    ref, S, n = triple
    assert tuple(got.shape) == tuple(ref.shape), (tag, name, tuple(got.shape), tuple(ref.shape))
    w = worst_ratio(got, ref, S)
    print(f"[{tag}] {name}: worst err/S {w:.2e} (tau({n}) = {tau(n):.1e})")
    assert w <= tau(n), f"{tag} {name}: worst err/S {w:.3e} > tau({n}) = {tau(n):.3e}"


def check_elem(tag, name, got, ref, S=None, terms=1):
    """Elementwise, no pooled statistic: |got - ref| <= 2^-22 * terms * S (S = |ref| for a single product); terms = 0: exact."""
    assert tuple(got.shape) == tuple(ref.shape), (tag, name, tuple(got.shape), tuple(ref.shape))
    if terms == 0:
        assert torch.equal(got.double().cpu(), ref), f"{tag} {name}: not exact"
        return
    w = worst_ratio(got, ref, ref.abs() if S is None else S)
    print(f"[{tag}] {name}: worst err/S {w:.2e} (bound {EXACT * terms:.1e})")
    assert w <= EXACT * terms, f"{tag} {name}: worst err/S {w:.3e} > {EXACT * terms:.3e}"


def check_measured(tag, name, got, ref, scale):
    assert tuple(got.shape) == tuple(ref.shape), (tag, name, tuple(got.shape), tuple(ref.shape))
    w = worst_ratio(got, ref, scale)
    bound = FACTOR * MEASURED[tag][name]
    print(f"[{tag}] {name}: worst err/scale {w:.3e} (bound {bound:.3e})")
    assert w <= bound, f"{tag} {name}: worst err/scale {w:.3e} > {FACTOR:g} x measured {MEASURED[tag][name]:.3e}"


def no_nan(tag, **tensors):
    for k, t in tensors.items():
        assert t is not None and not bool(torch.isnan(t).any()), f"{tag}: {k} holds a NaN (an element the kernels never wrote)"


def with_g0(triple, g0):
    ref, S, n = triple
    return ref + g0.double(), S + g0.double().abs(), n + 1


# ---- rcb_tail -----------------------------------------------------------------------------------------------------------------------

def run_rcb(inp, g0=None):
    from fcvsr_amd.train.blocks import rcb_tail
    from fcvsr_amd.train.ops import accumulate_into_grad, grad_destinations
    r, z = (inp[k].cuda().contiguous(**CL).requires_grad_(True) for k in ("r", "z"))
    ps = [inp[k].cuda().requires_grad_(True) for k in ("wmask", "w1", "w2")]
    if g0 is not None:
        for p, g in zip(ps, g0):
            p.grad = g.cuda().clone()
    y = rcb_tail(r, z, *ps, 0.2)
    with (accumulate_into_grad(*[p.grad for p in ps]) if g0 is not None else contextlib.nullcontext()):
        if g0 is not None:
            assert grad_destinations(*ps)[1] == 1                  # the kernel itself adds into the three .grad tensors
        y.backward(inp["gout"].cuda())
    torch.cuda.synchronize()
    got = dict(out=y.detach().cpu(), gr=r.grad.cpu(), gz=z.grad.cpu(), dwmask=ps[0].grad.cpu(), dw1=ps[1].grad.cpu(), dw2=ps[2].grad.cpu())
    no_nan("rcb_tail", **got)
    return got


def rcb_check(tag, inp, got, g0=None):
    ref = R.rcb_tail_reference(inp["r"], inp["z"], inp["wmask"], inp["w1"], inp["w2"], 0.2, inp["gout"])
    check_elem(tag, "gz", got["gz"], ref["gz"], terms=0)
    check_measured(tag, "out", got["out"], ref["out"], ref["out_scale"])
    check_measured(tag, "gr", got["gr"], ref["gr"], ref["gr_scale"])
    for i, name in enumerate(("dwmask", "dw1", "dw2")):
        check_sum(tag, name, got[name], ref[name] if g0 is None else with_g0(ref[name], g0[i]))


@pytest.mark.parametrize("B,H,W", R.RCB_SHAPES)
def test_rcb_tail_vs_f64_reference(B, H, W):
    """Output, gr, gz and the three parameter gradients; every branch of the partial / apply / row-sum kernels (module docstring)."""
    inp, left = R.rcb_inputs(B, H, W)
    assert left == 0, f"{left} entries within {R.MARGIN} of a kink"
    rcb_check(f"rcb_tail {B}x{H}x{W}", inp, run_rcb(inp))


@pytest.mark.parametrize("B,H,W", [(3, 5, 51), (1, 67, 107), (5, 7, 439)])
def test_rcb_tail_accumulate_mode_adds_into_existing_grad(B, H, W):
    """accumulate = 1 of fcvsr_rcbt_backward (the row-sum kernel's `dwmask[o] + t` / `out[i] + s`): .grad == G0 + ref."""
    inp, left = R.rcb_inputs(B, H, W)
    assert left == 0
    g = torch.Generator().manual_seed(R.shape_seed(3, B, H, W))
    g0 = [torch.randn(inp[k].shape, generator=g) for k in ("wmask", "w1", "w2")]
    rcb_check(f"rcb_tail accumulate {B}x{H}x{W}", inp, run_rcb(inp, g0), g0)


@pytest.mark.parametrize("stress", R.RCB_STRESS)
def test_rcb_tail_softmax_pool_stress(stress):
    """Two blocks per image (299 pixels): logits spanning +-40, the largest logit in the last pixel of the partial block, images of
    one batch at logit levels -30 / 0 / +30.  The output against f64 softmax pooling; `add`, read back from out - z (every pixel
    gives it: lrelu^-1(out - z) - r), within its own condition plus the rounding of that read-back; and, with W1 = W2 = I, the
    pooled vector ctx itself (add = lrelu(ctx))."""
    B, H, W = R.RCB_STRESS_SHAPE
    for identity in (False, True):
        inp, left = R.rcb_inputs(B, H, W, stress=stress, identity=identity)
        assert left == 0
        tag = f"rcb_tail stress {stress}{' identity' if identity else ''}"
        ref = R.rcb_tail_forward(inp["r"], inp["z"], inp["wmask"], inp["w1"], inp["w2"], 0.2)
        got = run_rcb(inp)
        check_measured(tag, "out", got["out"], ref["out"], ref["out_scale"])
        q = got["out"].double() - inp["z"].double()
        u_back = torch.where(q > 0, q, q / 0.2)
        add_back = u_back - inp["r"].double()                                     # (B,C,H,W): the same add[b][c] at every pixel
        add, S_add, n = ref["add"]
        floor = EXACT * (ref["out"].abs() + inp["z"].double().abs() + ref["u"].abs()) / 0.2
        err = (add_back - add[:, :, None, None]).abs()
        bound = tau(n) * S_add[:, :, None, None] + floor
        print(f"[{tag}] add from out - z: worst err/bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), f"{tag}: add read back from out - z is off by up to {float((err / bound).max()):.3e} bounds"
        if identity:                                                              # add = lrelu(ctx), t = ctx
            ctx, S_ctx, n = ref["ctx"]
            a_back = add_back
            ctx_back = torch.where(a_back > 0, a_back, a_back / 0.2)
            err = (ctx_back - ctx[:, :, None, None]).abs()
            bound = tau(n) * S_ctx[:, :, None, None] + floor / 0.2
            print(f"[{tag}] ctx from out - z: worst err/bound {float((err / bound).max()):.3e}")
            assert bool((err <= bound).all()), f"{tag}: ctx is off by up to {float((err / bound).max()):.3e} bounds"


# ---- divenh_band --------------------------------------------------------------------------------------------------------------------

DV_PARAMS = ("a", "b", "w1", "w2")


def run_divenh(inp, g0=None):
    from fcvsr_amd.train.blocks import divenh_band
    from fcvsr_amd.train.ops import accumulate_into_grad, grad_destinations
    xs = [inp[k].cuda().contiguous(**CL).requires_grad_(True) for k in ("f", "sf", "so")]
    ps = [inp[k].cuda().requires_grad_(True) for k in DV_PARAMS]
    if g0 is not None:
        for p, g in zip(ps, g0):
            p.grad = g.cuda().clone()
    nsf, nso = divenh_band(*xs, *ps)
    with (accumulate_into_grad(*[p.grad for p in ps]) if g0 is not None else contextlib.nullcontext()):
        if g0 is not None:
            assert grad_destinations(*ps)[1] == 1
        torch.autograd.backward([nsf, nso], [inp["g1"].cuda(), inp["g2"].cuda()])
    torch.cuda.synchronize()
    got = dict(Sf=nsf.detach().cpu(), So=nso.detach().cpu(), gf=xs[0].grad.cpu(), gSf=xs[1].grad.cpu(), gSo=xs[2].grad.cpu(),
               ga=ps[0].grad.cpu().reshape(-1), gb=ps[1].grad.cpu().reshape(-1), dw1=ps[2].grad.cpu(), dw2=ps[3].grad.cpu())
    no_nan("divenh_band", **got)
    return got


def divenh_check(tag, inp, got, g0=None):
    ref = R.divenh_band_reference(*(inp[k] for k in ("f", "sf", "so", "a", "b", "w1", "w2", "g1", "g2")))
    check_elem(tag, "Sf", got["Sf"], ref["Sf"], inp["f"].double().abs() + inp["sf"].double().abs(), terms=1)
    check_measured(tag, "So", got["So"], ref["So"], ref["So_scale"])
    for name in ("gf", "gSf", "gSo"):
        check_measured(tag, name, got[name], ref[name], ref[name + "_scale"])
    for i, name in enumerate(("ga", "gb", "dw1", "dw2")):
        t = ref[name]
        if g0 is not None:
            t = with_g0(t, g0[i].reshape(t[0].shape))
        check_sum(tag, name, got[name], t)


@pytest.mark.parametrize("C_,B,H,W", R.DIVENH_CASES)
def test_divenh_band_vs_f64_reference(C_, B, H, W):
    """Both outputs, the three input gradients and ga, gb, dw1, dw2; every branch of the reduce / apply / row-sum kernels."""
    inp, left = R.divenh_inputs(C_, B, H, W)
    assert left == 0, f"{left} hidden units within {R.MARGIN} of the ReLU kink"
    divenh_check(f"divenh_band C{C_} {B}x{H}x{W}", inp, run_divenh(inp))


@pytest.mark.parametrize("C_,B,H,W", [(64, 3, 5, 51), (32, 1, 67, 107), (64, 5, 7, 439)])
def test_divenh_band_accumulate_mode_adds_into_existing_grad(C_, B, H, W):
    """accumulate = 1 of fcvsr_divenh_band_backward: .grad == G0 + ref for a, b and both gate weights."""
    inp, left = R.divenh_inputs(C_, B, H, W)
    assert left == 0
    g = torch.Generator().manual_seed(R.shape_seed(4, C_, B, H, W))
    g0 = [torch.randn(inp[k].shape, generator=g) for k in DV_PARAMS]
    divenh_check(f"divenh_band accumulate C{C_} {B}x{H}x{W}", inp, run_divenh(inp, g0), g0)


# ---- fcvsr_iac_bwd_sac (C ABI) ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [32, 64])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 1, 9), (2, 9, 1), (2, 5, 7), (1, 13, 21)])
def test_iac_bwd_sac_vs_f64_reference(B, H, W, Cn):
    """gfin, gv, gK for all four (fin_accumulate, k_accumulate): destinations hold NaN where the call assigns and known values where
    it adds; k1 and gk are the second iteration's channel slices of (B,H,W,6*C*A) tensors, A = 2 (pixel stride 12 C, not 3 C), and
    the bytes of gK outside the slice keep their NaN; yout holds exact zeros (the slope side, as `yout > 0` says)."""
    from fcvsr_amd import hip
    L = hip.lib()
    A, slope = 2, 0.1
    lo, hi = 6 * Cn, 9 * Cn
    for fa in (0, 1):
        for ka in (0, 1):
            g = torch.Generator().manual_seed(R.shape_seed(5, B, H, W, Cn, fa, ka))
            gy, yout, v, s = (torch.randn(B, H, W, Cn, generator=g) for _ in range(4))
            yout.view(-1)[::5] = 0.0
            Kbig = torch.randn(B, H, W, 6 * Cn * A, generator=g) * 0.4
            gfin0 = torch.randn(B, H, W, Cn, generator=g) if fa else None
            gk0 = torch.randn(B, H, W, 3 * Cn, generator=g) if ka else None
            nan = float("nan")
            gfin = gfin0.cuda() if fa else torch.full((B, H, W, Cn), nan, device="cuda")
            gv = torch.full((B, H, W, Cn), nan, device="cuda")
            gKbig = torch.full((B, H, W, 6 * Cn * A), nan, device="cuda")
            if ka:
                gKbig[..., lo:hi] = gk0.cuda()
            d = [t.cuda() for t in (gy, yout, v, s)]
            Kd = Kbig.cuda()
            k1v, gkv = hip.view(Kd[..., lo:hi]), hip.view(gKbig[..., lo:hi])
            assert k1v.sx == 12 * Cn and gkv.sx == 12 * Cn
            hip.check(L.fcvsr_iac_bwd_sac(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), C.byref(k1v), slope, B, H, W, Cn,
                                          gfin.data_ptr(), fa, gv.data_ptr(), C.byref(gkv), ka, hip.stream_ptr()), "fcvsr_iac_bwd_sac")
            torch.cuda.synchronize()
            tag = f"iac_bwd_sac C{Cn} {B}x{H}x{W} fin+={fa} k+={ka}"
            gKc = gKbig.cpu()
            got = dict(gfin=gfin.cpu(), gv=gv.cpu(), gK=gKc[..., lo:hi])
            no_nan(tag, **got)
            outside = torch.cat([gKc[..., :lo], gKc[..., hi:]], dim=-1)
            assert bool(torch.isnan(outside).all()), f"{tag}: gK was written outside the channel slice"
            ref = R.iac_bwd_sac_reference(gy, yout, v, s, Kbig[..., lo:hi], slope, gfin0=gfin0, gk0=gk0)
            rf, Sf, nf = ref["gfin"]
            check_elem(tag, "gfin", got["gfin"], rf, Sf, terms=nf)
            check_sum(tag, "gv", got["gv"], ref["gv"])
            check_sum(tag, "gK", got["gK"], ref["gK"])


# ---- prelu --------------------------------------------------------------------------------------------------------------------------

def prelu_case(tag, shape, x_cl, g_cl, slope):
    from fcvsr_amd.train.blocks import prelu
    g = torch.Generator().manual_seed(R.shape_seed(6, *shape, x_cl, g_cl))
    x = torch.randn(*shape, generator=g)
    x.view(-1)[::3] = 0.0                                           # exact zeros take the slope side
    go = torch.randn(*shape, generator=g) + 0.5                     # a non-zero mean: doubled or dropped terms do not average out
    a = torch.tensor([slope])
    xd = (x.cuda().contiguous(**CL) if x_cl else x.cuda()).requires_grad_(True)
    gd = go.cuda().contiguous(**CL) if g_cl else go.cuda()
    ad = a.cuda().requires_grad_(True)
    y = prelu(xd, ad)
    y.backward(gd)
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu(), gx=xd.grad.cpu(), gslope=ad.grad.cpu())
    no_nan(tag, **got)
    ref = R.prelu_reference(x, a, go)
    check_elem(tag, "y", got["y"], ref["y"])
    check_elem(tag, "gx", got["gx"], ref["gx"])
    check_sum(tag, "gslope", got["gslope"], ref["gslope"])


# numel / 4 = 1, 255, 257, 2048 * 256 + 300 (past the backward's grid cap) and 4096 * 256 + 300 (past the forward's)
PRELU_SHAPES = [(1, 4, 1, 1), (1, 4, 15, 17), (1, 4, 1, 257), (1, 4, 626, 838), (1, 4, 2, 524438)]


@pytest.mark.parametrize("shape", PRELU_SHAPES)
def test_prelu_vs_f64_reference(shape):
    """y, gx and gslope (by its condition sum |g x|) for contiguous and channels_last inputs, an incoming gradient whose strides differ
    from x's, slopes 0.25 / 0 / -0.5, x with exact zeros."""
    n4 = shape[0] * shape[1] * shape[2] * shape[3] // 4
    assert n4 in (1, 255, 257, 2048 * 256 + 300, 4096 * 256 + 300)
    slopes = (0.25, 0.0, -0.5)
    for i, (x_cl, g_cl) in enumerate(((False, False), (True, True), (False, True), (True, False))):
        for slope in (slopes if n4 < 4096 else slopes[i % 3:i % 3 + 1]):
            prelu_case(f"prelu n4={n4} x_cl={x_cl} g_cl={g_cl} slope={slope}", shape, x_cl, g_cl, slope)


def test_prelu_odd_numel_takes_the_torch_fallback_and_matches():
    """numel % 4 != 0: blocks.prelu hands the call to torch; the same reference, the same bounds."""
    for slope in (0.25, 0.0, -0.5):
        prelu_case(f"prelu fallback slope={slope}", (1, 3, 5, 7), False, False, slope)


# ---- xscale -------------------------------------------------------------------------------------------------------------------------

def adjoint_identity(tag, fwd_u, g, u, adj_g):
    """<A u, g> == <u, A^T g> in f64, A u from the reference and A^T g from the kernel, on the signed test data: to 1e-6 of
    sum |u| |A^T g| (the signed inner product cancels to a few units, and f32 rounding of A^T g alone exceeds 1e-6 of that)."""
    u64, a64 = u.double(), adj_g.detach().cpu().double()
    lhs, rhs = float((fwd_u * g.double()).sum()), float((u64 * a64).sum())
    scale = float((u64.abs() * a64.abs()).sum())
    print(f"[{tag}] <A u, g> = {lhs:.9e}, <u, A^T g> = {rhs:.9e}, difference / sum |u||A^T g| = {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs - rhs) <= 1e-6 * scale, (tag, lhs, rhs, scale)


@pytest.mark.parametrize("Cn", [4, 32, 64])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (5, 1), (3, 7)])
def test_xscale_vs_f64_reference(h, w, Cn):
    """The three dn / up combinations of graph._block_rcb at low-resolution sizes (h, w) (one row, one column, both edges in one
    pixel): forward, gx, gR and the two resampling adjoints; and for each adjoint <A u, g> == <u, A^T g> with the kernel's A^T g
    (`adjoint_identity` on the signed data; for up2 also on positive u and g to 1e-6 of the inner product itself)."""
    from fcvsr_amd.train.blocks import xscale
    B, H, W = 3, 2 * h, 2 * w
    g = torch.Generator().manual_seed(R.shape_seed(7, h, w, Cn))
    x, Rr, go = (torch.randn(B, Cn, H, W, generator=g) for _ in range(3))
    dn = torch.randn(B, Cn, 2 * H, 2 * W, generator=g)
    up = torch.randn(B, Cn, h, w, generator=g)
    assert (B * h * w * Cn // 4) % 256                              # up2_adjoint's last block is partial
    for use_dn, use_up, rs in ((False, True, 2.0), (True, True, 1.0), (True, False, 2.0)):
        tag = f"xscale C{Cn} low {h}x{w} dn={use_dn} up={use_up}"
        xd, Rd, dd, ud = (t.cuda().contiguous(**CL).requires_grad_(True) for t in (x, Rr, dn, up))
        y = xscale(xd, Rd, rs, dd if use_dn else None, ud if use_up else None)
        y.backward(go.cuda())
        torch.cuda.synchronize()
        ref, S, n = R.xscale_forward(x, Rr, rs, dn if use_dn else None, up if use_up else None)
        no_nan(tag, out=y.detach(), gx=xd.grad, gR=Rd.grad)
        check_elem(tag, "out", y.detach().cpu(), ref, S, terms=n)
        check_elem(tag, "gx", xd.grad.cpu(), go.double(), terms=0)
        check_elem(tag, "gR", Rd.grad.cpu(), rs * go.double(), terms=0)
        if use_dn:
            no_nan(tag, gdn=dd.grad)
            check_elem(tag, "gdn", dd.grad.cpu(), R.pool2_adjoint(go), terms=0)
            adjoint_identity(tag + " pool2", R.pool2_forward(dn), go, dn, dd.grad)
        else:
            assert dd.grad is None
        if use_up:
            no_nan(tag, gup=ud.grad)
            aref, aS, an = R.up2_adjoint(go)
            check_elem(tag, "gup", ud.grad.cpu(), aref, aS, terms=an)
            adjoint_identity(tag + " up2", R.up2_forward(up), go, up, ud.grad)
            # and on positive data, where nothing cancels: to 1e-6 of the inner product itself
            up_p, go_p = up.abs() + 0.1, go.abs() + 0.1
            u2 = up_p.cuda().contiguous(**CL).requires_grad_(True)
            xscale(xd.detach(), Rd.detach(), rs, None, u2).backward(go_p.cuda())
            lhs = float((R.up2_forward(up_p) * go_p.double()).sum())
            rhs = float((up_p.double() * u2.grad.cpu().double()).sum())
            print(f"[{tag}] positive data: <up(u), g> = {lhs:.9e}, <u, up^T g> = {rhs:.9e}, relative difference {abs(lhs - rhs) / abs(lhs):.2e}")
            assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (tag, lhs, rhs)
        else:
            assert ud.grad is None


# ---- corr_lookup --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [128, 64])
@pytest.mark.parametrize("H", [1, 64, 69])
def test_corr_lookup_vs_f64_reference(H, Cn):
    """Wf = 1, 2, 5 (x_count = Wf) and 6 (x_count = radius + 2); H below, at and past the row cut-off of the C/2 x 2 sampling image.
    One product and one division per entry; gradient entries that no (pixel, i, j) maps to are bit-zero."""
    from fcvsr_amd.train.blocks import corr_lookup
    for Wf in (1, 2, 5, 6):
        B = 2
        g = torch.Generator().manual_seed(R.shape_seed(8, H, Wf, Cn))
        a, b = torch.randn(B, Cn, H, Wf, generator=g), torch.randn(B, Cn, H, Wf, generator=g)
        go = torch.randn(B, 81, H, Wf, generator=g)
        ad, bd = (t.cuda().contiguous(**CL).requires_grad_(True) for t in (a, b))
        y = corr_lookup(ad, bd)
        y.backward(go.cuda())
        torch.cuda.synchronize()
        tag = f"corr_lookup C{Cn} {H}x{Wf}"
        got = dict(corr=y.detach().cpu(), gx1=ad.grad.cpu(), gx2=bd.grad.cpu())
        no_nan(tag, **got)
        ref = R.corr_lookup_reference(a, b, 4, go)
        for name in ("corr", "gx1", "gx2"):
            check_elem(tag, name, got[name], ref[name])              # (a * b) / sqrt(C): 2^-22 of the entry, zeros exact
        untouched = ~ref["touched"]
        for name in ("gx1", "gx2"):
            bits = got[name].contiguous().view(torch.int32)[:, untouched]
            assert bool((bits == 0).all()), f"{tag}: {name} has a non-zero bit pattern where no source maps"
