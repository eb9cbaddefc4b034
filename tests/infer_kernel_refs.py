"""Float64 CPU references of the 16-bit inference path's non-convolution kernels, written per element from the formulas in the kernel
file headers (tail.hip, bilinear.h, tail_fused.hip, scnet.hip, feat_extract.hip, mffr.hip, u8.h); nothing here calls fcvsr_amd.hip.
Each reference returns (ref, bound): f64 tensors of the output's shape, `bound` the error a correct kernel may show at that element.
tests/test_infer_kernel_refs_cpu.py pins the references to torch / the oracle and shows that the bounds reject wrong kernels;
tests/test_infer_kernels_gpu.py asserts |got - ref| <= bound for every element of every kernel output.

What a bound is made of (stated again next to each function):
  f32 arithmetic   k * 2^-24 * S.  S = the same expression on absolute values (>= every intermediate); k = the rounded f32 operations on
                   the longest path to one output, counted from the kernel source (an fma is one; a product by 0.5, 0.25 or by a
                   bilinear weight of a x2 / x4 grid - multiples of 1/8 resp. 1/16 formed exactly - is exact only where the comment
                   says so).  Parallel branches do not add to k: each one's error is weighted by its share of S.  Sums of n > 16
                   products in an order the kernel (its MFMA) chooses: tau(n) * S (tests/tolerance.py).
  final store      u * |ref|, u = 2^-8 (bf16) or 2^-11 (f16): half a unit in the last place, round to nearest even; never less than
                   half the spacing of f16's subnormals (2^-25), where the relative figure does not hold; zero for an f32 store.  `ref`
                   itself is NOT rounded to the store type: a rounded reference would pay the store rounding twice.
  rounded          the kernel rounds some intermediates to 16 bit before it uses them (u2 inside the fused tail, R before the 2x2
  intermediates    pool).  The reference rounds its f64 value the same way (.to(dtype), nearest even).  The kernel's f32 value x' lies
                   within e (its own f32 bound) of the f64 value x, so its rounding differs from the reference's only where
                   round(x - e) != round(x + e) (rounding is monotone), and then by at most |round(x + e) - round(x - e)| - one unit
                   in the last place unless e is large.  That spread, weighted by |w_i|, is added: sum |w_i| spread_i.  It is never
                   allowed to exceed u * sum |w_i| |v_i| (capped by it), and is zero for every operand that sits clear of a tie -
                   which is what lets the bound tell `pool of the rounded R` from `pool of the unrounded R`.

The `upper`, `pad`, `side` and `wrap` keywords select deliberately WRONG variants (an unclamped neighbour, clamp padding, the slope on
the wrong side, a flat pixel index without the column test); only tests/test_infer_kernel_refs_cpu.py passes them, to show that the
bounds reject them.  `cd` is the dtype the arithmetic runs in: float64, or float32 for that file's "a correct f32 evaluation stays
inside the bound" check."""
import torch
import torch.nn.functional as F

from tolerance import tau

D = torch.float64
EPS = 2.0 ** -24
U = {None: 0.0, torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {None: 0.0, torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def shape_seed(*key):
    s = 29
    for k in key:
        s = (s * 1000003 + int(k)) % 2147483647
    return s


def gen(*key):
    return torch.Generator().manual_seed(shape_seed(*key))


def f32(v):
    """A Python scalar as the f32 the kernel receives."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def rnd(t, dt):
    """Values of t rounded to the storage type dt (nearest even), in t's dtype; f32 / None: unchanged."""
    return t if dt in (None, torch.float32) else t.to(dt).to(t.dtype)


def store(ref, dt):
    """The final-store term."""
    return (U[dt] * ref.abs()).clamp_min(TINY[dt])


def spread(x, e, dt):
    """How far the kernel's rounding of its own x' (|x' - x| <= e) can sit from the reference's rounding of x."""
    if dt in (None, torch.float32):
        return torch.zeros_like(x)
    return (rnd(x + e, dt) - rnd(x - e, dt)).abs()


# ---- bilinear resampling (align_corners = False) ------------------------------------------------------------------------------------

def axis_taps(n_in, scale, cd=D, upper="clamp"):
    """Output index o of a x`scale` axis: source coordinate (o + 0.5) / scale - 0.5 clamped at 0, lower neighbour i0 = floor, weight
    l = coordinate - i0 of the upper neighbour i1 = i0 + 1 clamped at n_in - 1."""
    o = torch.arange(scale * n_in, dtype=cd)
    s = ((o + 0.5) / scale - 0.5).clamp_min(0.0)
    i0 = s.floor().long()
    l = s - i0.to(cd)
    if upper == "clamp":
        i1 = i0 + (i0 < n_in - 1).long()
    elif upper == "early":                                   # WRONG: clamped one early
        i1 = i0 + (i0 < n_in - 2).long()
    else:                                                    # WRONG ("none"): not clamped; the caller appends a zero row / column
        i1 = i0 + 1
    return i0, i1, l


def resample(x, scale, hd, wd, upper="clamp"):
    """x up-sampled by `scale` along dims hd (rows) and wd (columns), in the kernels' order: along x inside each row, then along y."""
    H, W = x.shape[hd], x.shape[wd]
    if upper == "none":
        x = torch.cat([x, torch.zeros_like(x.narrow(hd, 0, 1))], hd)
        x = torch.cat([x, torch.zeros_like(x.narrow(wd, 0, 1))], wd)
    y0, y1, ly = axis_taps(H, scale, x.dtype, upper)
    x0, x1, lx = axis_taps(W, scale, x.dtype, upper)
    sy, sx = [1] * x.dim(), [1] * x.dim()
    sy[hd], sx[wd] = -1, -1
    ly, lx = ly.view(sy), lx.view(sx)

    def row(yi):
        r = x.index_select(hd, yi)
        return (1.0 - lx) * r.index_select(wd, x0) + lx * r.index_select(wd, x1)

    return (1.0 - ly) * row(y0) + ly * row(y1)


def bilinear_up4(x, cd=D, upper="clamp"):
    """fcvsr_bilinear_up4 (bilinear.h): x (B,C,H,W) f32 -> (B,C,4H,4W) f32.
    f32 arithmetic, k = 4: the coordinates and both weights are multiples of 1/8 formed exactly (0.25 * (o + 0.5) - 0.5 on small
    integers), 1 - l is exact.  No fma (the library is built with -ffp-contract=off): the two products inside a row run in parallel
    [1], their sum [2], the product by (1-ly) or ly [3], the sum of the two rows [4].  No store term, no intermediates."""
    v = x.to(cd)
    return resample(v, 4, 2, 3, upper), 4 * EPS * resample(v.abs(), 4, 2, 3, upper)


# ---- fused up-sampler tail --------------------------------------------------------------------------------------------------------

def prelu(y, s, side="neg"):
    return torch.where(y >= 0, y, s * y) if side == "neg" else torch.where(y >= 0, s * y, y)       # "pos" is WRONG


def tail_u2(u1, w2, b2, slope, cd=D, side="neg"):
    """Steps 1-3 of tail_fused.hip before the rounding: u1 (B,H2,W2,64) 16-bit, w2 (256,64) 16-bit with rows sub-pixel-major
    ((2i+j)*64 + c), b2 (256,) f32 in the same order or None -> u2 (B,2*H2,2*W2,64) = PReLU(PixelShuffle2(W2 u1 + b2)) and e, the bound
    of the kernel's f32 value of it: tau(65) * S for the 64 MFMA products plus the bias, 2^-24 * S for the product by the slope, both
    times max(1, |slope|)."""
    x, w = u1.to(cd), w2.to(cd)
    B, H2, W2, _ = x.shape
    b = torch.zeros(256, dtype=cd) if b2 is None else b2.to(cd)
    y = x @ w.t() + b
    S = x.abs() @ w.abs().t() + b.abs()

    def shuffle(t):                                          # row (2i+j)*64 + c of pixel (h, w) -> channel c of pixel (2h+i, 2w+j)
        return t.view(B, H2, W2, 2, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, 64)

    s = f32(slope)
    return shuffle(prelu(y, s, side)), shuffle(S).double() * ((tau(65) + EPS) * max(1.0, abs(s)))


def tail_last(u2, wl, bl, base, pad="zeros"):
    """conv_last0 of tail_fused.hip: u2 (B,HH,WW,64), wl the [16][64] tap table (row ky*3+kx, rows 9..15 unused), bl (1,) or None, base
    (B,HH,WW) -> base + bl + the 3x3 64 -> 1 convolution with zero padding outside the image."""
    cd = u2.dtype
    w = wl.to(cd)[:9].view(3, 3, 64).permute(2, 0, 1)[None]
    x = u2.permute(0, 3, 1, 2)
    if pad == "zeros":
        y = F.conv2d(x, w, padding=1)
    else:                                                    # WRONG: clamp padding
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)
    return y[:, 0] + (0.0 if bl is None else bl.to(cd)[0]) + base.to(cd)


def tail_fused(u1, w2, b2, slope, wl, bl, base, dt, cd=D):
    """fcvsr_tail_fused: (B,4H,4W) f32 result, dt = the dtype of u1 / w2 / wl (None: u2 is not rounded).
    f32 arithmetic: 576 products in two chained MFMAs per tap, then base + bias and nine tap sums on the vector ALU: 578 terms in
    the kernel's order, tau(578) * S.  Store: f32, none.  Rounded intermediate: u2, weight |wl| (module docstring); unrounded (dt =
    None) its f32 error e itself passes through the convolution instead."""
    u2, e = tail_u2(u1, w2, b2, slope, cd)
    u2r = rnd(u2, dt)
    ref = tail_last(u2r, wl, bl, base)
    zero = torch.zeros_like(base, dtype=D)
    wa, ba = wl.double().abs(), None if bl is None else bl.double().abs()
    S = tail_last(u2r.double().abs(), wa, ba, base.double().abs())
    if dt is None:
        flip = tail_last(e, wa, None, zero)
    else:
        flip = torch.minimum(tail_last(spread(u2.double(), e, dt), wa, None, zero), U[dt] * tail_last(u2r.double().abs(), wa, None, zero))
    return ref, tau(578) * S + flip


# ---- BlockRCB's elementwise kernels (NHWC) --------------------------------------------------------------------------------------------

def mean2x2(t):
    B, H, W, C = t.shape
    t = t.view(B, H // 2, 2, W // 2, 2, C)
    top, bot = 0.5 * t[:, :, 0, :, 0] + 0.5 * t[:, :, 0, :, 1], 0.5 * t[:, :, 1, :, 0] + 0.5 * t[:, :, 1, :, 1]
    return 0.5 * top + 0.5 * bot


def gc_apply(r, add, z, slope, dt, pool=False, cd=D, slope32=True):
    """fcvsr_gc_apply / _levels (scnet.hip): r, z (B,H,W,C), add (B,C) f32, dt = the dtype of z / out / pool.
    pool = False: `out`, R = lrelu(r + add[b, c]) + z.  f32 arithmetic k = 3 (r + add, * slope, + z), S = |r| + |add| + |z|; store u |R|.
    pool = True: the pooled tensor, mean2x2 of R ROUNDED to dt.  f32 arithmetic on the rounded R: k = 2 (the products by 0.5 are exact:
    one sum inside each row, one across), S = mean2x2 |R|; rounded intermediates R with weight 1/4, e = R's f32 bound above; store
    u |pool|.  dt f32 / None rounds nothing: R's own error passes through, k = 3 + 2 on S = mean2x2(|r| + |add| + |z|).
    The slope is the f32 the kernel receives; slope32 = False keeps the f64 value (the oracle's literal 0.2, for the CPU pin)."""
    rr, zz, a = r.to(cd), z.to(cd), add.to(cd)[:, None, None, :]
    v = rr + a
    R = torch.where(v >= 0, v, v * (f32(slope) if slope32 else slope)) + zz
    S = (rr.abs() + a.abs() + zz.abs()).double()
    if not pool:
        return R, 3 * EPS * S + store(R.double(), dt)
    if dt in (None, torch.float32):
        return mean2x2(R), 5 * EPS * mean2x2(S)
    Rr = rnd(R, dt)
    P, A = mean2x2(Rr), mean2x2(Rr.double().abs())
    flip = torch.minimum(mean2x2(spread(R.double(), 3 * EPS * S, dt)), U[dt] * A)
    return P, 2 * EPS * A + flip + store(P.double(), dt)


def xscale(x, r, rs, dn, dn_pooled, up, dt, cd=D, upper="clamp"):
    """fcvsr_xscale / _levels (scnet.hip): round_dt(x + rs * r + D + bilinear_x2(up)), all (B,H,W,C) in dt; D = dn (dn_pooled) or the
    2x2 mean of the (B,2H,2W,C) tensor dn; up (B,H/2,W/2,C); either may be None.
    f32 arithmetic, S = |x| + |rs| |r| + |D|'s terms + the interpolation of |up|: fma(rs, r, x) [1]; pooled dn: one sum [+1]; unpooled:
    the row sums 0.5 a + 0.5 b (one rounding each) run in parallel with that first fma, then two fmas by 0.5 [+2]; up: the four
    weights are products of multiples of 1/4, exact; four fmas [+4].  The longest path is 3 (unpooled dn), 7 with up.  Store u |ref|."""
    v = x.to(cd) + f32(rs) * r.to(cd)
    S = x.double().abs() + abs(f32(rs)) * r.double().abs()
    k = 1
    if dn is not None:
        v = v + (dn.to(cd) if dn_pooled else mean2x2(dn.to(cd)))
        S = S + (dn.double().abs() if dn_pooled else mean2x2(dn.double().abs()))
        k += 1 if dn_pooled else 2
    if up is not None:
        v = v + resample(up.to(cd), 2, 1, 2, upper)
        S = S + resample(up.double().abs(), 2, 1, 2, upper)
        k += 4
    return v, k * EPS * S + store(v.double(), dt)


def scale_add(z, gate, x, dt, cd=D):
    """fcvsr_scale_add (mffr.hip): round_dt(z * gate[b, c] + x), z (B,H,W,C) f32, gate (B,C) f32, x f32 or dt.  One fma: k = 1 on
    S = |z gate| + |x|; store u |ref|."""
    g = gate.to(cd)[:, None, None, :]
    v = z.to(cd) * g + x.to(cd)
    return v, EPS * (z.double().abs() * g.double().abs() + x.double().abs()) + store(v.double(), dt)


# ---- feat_extract -------------------------------------------------------------------------------------------------------------------

def im2col(x, wrap=False):
    """x (B,cin,H,W) -> (B,H,W,9*cin), column tap*cin + c = x[b, c, y + ky - 1, x + kx - 1] (tap = ky*3 + kx), zero outside the image."""
    B, Cn, H, W = x.shape
    if not wrap:
        p = F.pad(x, (1, 1, 1, 1))
        taps = [p[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
    else:                                                    # WRONG: the neighbour of a border pixel comes from the flat pixel index
        p = F.pad(x.reshape(B, Cn, H * W), (W + 1, W + 1))
        taps = [p[:, :, W + 1 + (ky - 1) * W + kx - 1:][:, :, :H * W].view(B, Cn, H, W) for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 1).permute(0, 3, 4, 1, 2).reshape(B, H, W, 9 * Cn)


def feat_extract(x, wmat, bias, dt, cd=D, wrap=False):
    """fcvsr_feat_extract (feat_extract.hip): x (B,7,H,W) f32, wmat (n_blk*64, 64) f16 with column k = tap*7 + c (column 63 unused),
    bias f32 or None -> (B,H,W,n_blk*64) in dt.  The kernel builds an f16 im2col tile: x is ROUNDED TO F16 first (an input, rounded the
    same way by both sides: no spread).  f16 x f16 products are exact in f32; 63 of them and the bias, 64 terms in the MFMA's order:
    tau(64) * S.  Store u |ref|."""
    cols = im2col(x.to(torch.float16).to(cd), wrap)
    w = wmat.to(cd)[:, :63]
    b = torch.zeros(w.shape[0], dtype=cd) if bias is None else bias.to(cd)
    v = cols @ w.t() + b
    S = cols.double().abs() @ w.double().abs().t() + b.double().abs()
    return v, tau(64) * S + store(v.double(), dt)


def feat_matrix(w):
    """(cout, 7, 3, 3) -> the [cout][64] f16 matrix of the kernel, column tap*7 + c."""
    mat = torch.zeros(w.shape[0], 64)
    mat[:, :63] = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return mat.to(torch.float16)


# ---- integer output (u8.h), plain torch f32: exact comparisons, not a bound --------------------------------------------------------

def quantise(v, peak, mode):
    """clamp(v, 0, 1) * peak in f32, truncated ("truncate") or rounded half to even ("round"), as int32."""
    q = v.float().clamp(0.0, 1.0) * torch.tensor(float(peak), dtype=torch.float32)
    return (torch.trunc(q) if mode == "truncate" else torch.round(q)).to(torch.int32)


# ---- inputs shared by the GPU tests and the CPU discrimination test -----------------------------------------------------------------

BILINEAR_SHAPES = [(2, 1, 1, 1), (1, 3, 2, 3), (2, 1, 5, 7), (1, 1, 4, 36)]
TAIL_SLOPES = [0.25, 0.0, 1.5]
TAIL_SMALL = [(2, 4, 4), (1, 6, 20), (3, 5, 9)]              # (B, H, W) of the LR centre frame; u1 is (2H, 2W), the result (4H, 4W)
TAIL_BIG_HW = (36, 68)
GC_LEVELS = [(6, 10, True), (3, 5, False), (22, 18, True)]   # (H, W, pooled)
FEAT_SHAPES = [(1, 4, 4), (2, 5, 9), (3, 12, 20)]
DT_CODE = {F32: 0, BF16: 1, F16: 2}


def bilinear_window(B, C, H, W):
    """(B,7,C,H,W) f32 window; the kernels read its centre frame [:, 3]."""
    return torch.randn(B, 7, C, H, W, generator=gen(1, B, C, H, W))


def tail_inputs(B, H, W, dt, slope):
    g = gen(2, B, H, W, int(slope * 100), dt == BF16)
    wl = torch.zeros(16, 64)
    wl[:9] = torch.randn(9, 64, generator=g) / 200
    return dict(u1=torch.randn(B, 2 * H, 2 * W, 64, generator=g).to(dt), w2=(torch.randn(256, 64, generator=g) / 8).to(dt),
                b2=torch.randn(256, generator=g) * 0.1, slope=slope, wl=wl.to(dt), bl=torch.tensor([0.03]),
                base=0.1 + 0.8 * torch.rand(B, 4 * H, 4 * W, generator=g))


def tail_ref(p, dt, cd=D):
    return tail_fused(p["u1"], p["w2"], p["b2"], p["slope"], p["wl"], p["bl"], p["base"], dt, cd)


def gc_inputs(B, H, W, Cn, dt, rdt):
    g = gen(3, B, H, W, Cn, DT_CODE[dt], DT_CODE[rdt])
    return dict(r=torch.randn(B, H, W, Cn, generator=g).to(rdt), add=torch.randn(B, Cn, generator=g) * 0.5,
                z=torch.randn(B, H, W, Cn, generator=g).to(dt))


def xscale_inputs(B, H, W, Cn, dt, dn, up):
    """dn: None, "pooled" (B,H,W,C) or "full" (B,2H,2W,C); up: bool, (B,H/2,W/2,C)."""
    g = gen(4, B, H, W, Cn, DT_CODE[dt])
    t = lambda h, w: torch.randn(B, h, w, Cn, generator=g).to(dt)
    return dict(x=t(H, W), r=t(H, W), dn=None if dn is None else (t(H, W) if dn == "pooled" else t(2 * H, 2 * W)),
                dn_pooled=int(dn == "pooled"), up=t(H // 2, W // 2) if up else None)


XS_LEVELS = [((22, 18), None, True, 2.0), ((12, 10), "pooled", True, 1.0), ((3, 5), "full", False, 2.0)]   # (H, W), dn, up, rs


def feat_inputs(B, H, W, with_bias=True):
    g = gen(5, B, H, W)
    x8 = torch.randint(0, 256, (B, 7, H, W), generator=g, dtype=torch.uint8)
    w = torch.randn(448, 7, 3, 3, generator=g) / 8
    return dict(x8=x8, x=x8.float() / 255, w=w, wmat=feat_matrix(w), bias=torch.randn(448, generator=g) * 0.1 if with_bias else None)


def scale_add_inputs(B, H, W, Cn, xdt):
    g = gen(6, B, H, W, Cn, DT_CODE[xdt])
    return dict(z=torch.randn(B, H, W, Cn, generator=g), gate=torch.rand(B, Cn, generator=g), x=torch.randn(B, H, W, Cn, generator=g).to(xdt))
