"""Float64 CPU references of the fused frequency-head kernels - fcvsr_freq_mlp3 (freq_mlp.hip), fcvsr_freq_head and
fcvsr_convcorr_strip (freq_head.hip) - restated from the reference model (CVSR_freq.py:1371-1396, applied at :1472-1488) and the kernel
file headers; nothing here calls fcvsr_amd.hip.  tests/test_freq_fused_refs_cpu.py pins the references to plain torch conv2d / relu and
shows that the bounds accept a correct f32 evaluation in another summation order and reject the wrong kernels of `WRONG_*`;
tests/test_freq_fused_gpu.py asserts |got - ref| <= bound for every element the kernels write.  Conventions as in
tests/infer_kernel_refs.py: every reference returns (ref, bound), f64 tensors of the output's shape; `cd` is the dtype the arithmetic
runs in (float64, or float32 - then every product runs over a permuted channel order - for the CPU self-check); `wrong` selects a
deliberately WRONG variant.

The operations (1x1 convolutions without bias; every operand of a product is a bf16 number, the sums are f32):
  mlp3   out = (xa - xb) + W4 . relu(W2 . relu(W0 . [xa | xb])), 128 channels, per direction.  Layer 0 multiplies the f32 spectra
         ROUNDED to bf16 (nearest even); both hidden tensors are rounded to bf16 after the ReLU; the residual takes the UNROUNDED f32
         spectra, (acc + xa) - xb as two fmas; the result is stored as bf16.
  head   out (4 channels, f32) = Wl . relu([Wmid . relu](W0 . x)), x 128 channels - bf16 as stored, or f32 rounded to bf16 - hidden
         width 64, rounded to bf16 after each ReLU; f32 store.
  strip  head on [off (128, bf16) | corr (81 live of 84, f32 -> bf16)] for the 2 B H xs pixels x < xs of a (2B, H, Wf) grid; direction d
         of image b takes the lookup row (b, y, x) (both directions share the lookup); the result lands at pixel (d B + b, y, x) of a
         (2B, H, Wf, 4) tensor whose columns >= xs are not produced (NaN in `ref`, 0 in `bound`).

The bound, derived and not measured:
  one layer        its f32 pre-activation a' lies within e = tau(n) * S + |W| c of the reference's a: S = |W| |v| (the same product
                   on absolute values), n = the products per output (256, 212, 128 or 64; tests/tolerance.py), c = the error carried
                   by its input v (next paragraph; zero for layer 0, whose input both sides round from the same f32 numbers).
  hidden values    the reference rounds h = relu(a) to bf16 as the kernel rounds its own h' = relu(a'), which lies in
                   [relu(a - e), relu(a + e)] (the ReLU is monotone and 1-Lipschitz).  Rounding is monotone too, so the two rounded
                   values differ by at most the spread of that interval, rnd(relu(a + e)) - rnd(relu(a - e)) - `spread` of
                   infer_kernel_refs.py, taken after the ReLU: zero wherever h sits clear of a tie and for every unit that is dead
                   on both ends, one unit in the last place where a tie lies inside.  As in the "rounded intermediates" paragraph
                   there it is capped by one unit in the last place of |rnd h| (`ulp`).  The cap is where this stops being a worst
                   case: behind the first hidden layer e holds the flips of up to 128 inputs at their full weight and often exceeds
                   a last place, and a kernel whose flips all lined up could move a second-layer value by more than the cap admits.
                   They do not line up: the f32 evaluation of the CPU test, another summation order in every layer, stays at 0.27
                   of the bound or less before its store, and the kernels' own figures are in tests/test_freq_fused_gpu.py.
  mlp3 residual    2 * 2^-24 * (|acc| + |xa| + |xb|): one rounding per fma, each on a value below that sum.
  final store      store(ref, bf16) for mlp3, none for the f32 results.  `ref` is never rounded to the store type.
No "hidden tensor not rounded" variant is listed: a kernel that keeps its hidden values in f32 differs from this reference by up to
half a last place of every hidden value - the size of the flips the capped spread has to admit.  It leaves the bound by a factor of
2 to 5 at a few elements in 10^4 of the larger cases and nowhere at the small ones: too close to be required of every case, and by
its construction the bound need not tell the two apart.

Input sets (`SETS`; seeded CPU generators): `normal`; `spectrum` - scale 3000 and pixel 0 of every image 40 times larger, an
unnormalised spectrum with its DC bin: max |x| > 65504, outside f16; `near` - xa = xb + 2^-10 noise re-rounded to f32 (|noise| >= 1/4),
neighbouring frames: the residual cancels; `w4zero` - `near` with W4 = 0: the bound collapses to the residual and store terms."""
import torch

from freq_kernel_refs import corr_lookup
from infer_kernel_refs import BF16, D, EPS, F32, gen, rnd, spread, store
from tolerance import tau

NAN = float("nan")
SETS = ["normal", "spectrum", "near", "w4zero"]
F16_MAX = 65504.0


def pack(w):
    """(cout, cin) f32 -> the kernels' bf16 weight matrix [ceil128(cout)][ceil64(cin)], cin contiguous, zero padded."""
    cout, cin = w.shape
    out = torch.zeros((cout + 127) // 128 * 128, (cin + 63) // 64 * 64, dtype=BF16)
    out[:cout, :cin] = w.to(BF16)
    return out


def _layer(v, c, w, n, cd):
    """a = v . w^T and the bound e of the kernel's f32 value of it; v (.., cin) in cd, c its carried error (f64) or None, w (cout, cin).
    cd = float32 walks the channels in another (fixed) order."""
    if cd == F32:
        p = torch.randperm(w.shape[1], generator=gen(70, w.shape[1]))
        a = v[..., p] @ w[:, p].t()
    else:
        a = v @ w.t()
    wa = w.double().abs().t()
    e = tau(n) * (v.double().abs() @ wa)
    return a, e if c is None else e + c @ wa


def ulp(t):
    """One unit in the last place of the bf16 numbers t (8 significant bits); 0 for 0."""
    m, ex = torch.frexp(t.double().abs())
    return torch.where(m == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), ex - 8))


def _hidden(a, e, relu=True):
    """relu, bf16: the reference's hidden tensor and the error it carries (module docstring)."""
    act = torch.relu if relu else (lambda t: t)
    hr = rnd(act(a), BF16)
    lo, hi = act(a.double() - e), act(a.double() + e)        # h' lies in [lo, hi]
    return hr, torch.minimum(spread(0.5 * (hi + lo), 0.5 * (hi - lo), BF16), ulp(hr))


# ---- fcvsr_freq_mlp3 --------------------------------------------------------------------------------------------------------------------

WRONG_MLP3 = ["xbxa", "w24", "norelu2", "resadd", "resround", "dirswap", "droptile"]
MLP3_SHAPES = [(1, 1, 1), (1, 1, 127), (1, 1, 128), (1, 1, 129), (2, 9, 23), (1, 25, 41)]      # (1,25,41): 1025 pixels, 9 tiles = 8 + 1
MLP3_LAYOUTS = ["separate", "record"]                        # three stride-128 tensors (the engine) / slices of one stride-384 record
MLP3_DST = [128, 136]


def _mlp3_cases():
    """(B, H, Wf, n_dirs, layout, dst_pix_stride, set)."""
    cases = []
    for i, s in enumerate(MLP3_SHAPES):                      # every shape x direction count on `normal`; layouts and strides alternate
        for nd in (1, 2):
            cases.append(s + (nd, MLP3_LAYOUTS[(i + nd) % 2], MLP3_DST[(i // 2 + nd) % 2], "normal"))
    for s in MLP3_SHAPES[4:]:                                # every set, both layouts, both strides at the two larger shapes
        for k, name in enumerate(SETS):
            for j in range(2):
                c = s + (2, MLP3_LAYOUTS[j], MLP3_DST[(j + k) % 2], name)
                if c not in cases:
                    cases.append(c)
    return cases


MLP3_CASES = _mlp3_cases()


def mlp3_inputs(B, H, Wf, nd, layout, dsx, name):
    """x1, x2, x3 (B,H,Wf,128) f32: xa = x1 (direction 0), x3 (direction 1), xb = x2; W0 (128,256), W2, W4 (128,128) f32."""
    g = gen(71, B, H, Wf, SETS.index(name))
    r = lambda *s: torch.randn(*s, generator=g)
    if name in ("near", "w4zero"):
        x2 = r(B, H, Wf, 128)
        noise = [r(B, H, Wf, 128) for _ in range(2)]
        x1, x3 = [(x2 + 2.0 ** -10 * torch.where(n >= 0, 1.0, -1.0) * n.abs().clamp_min(0.25)).float() for n in noise]
    else:
        x1, x2, x3 = r(B, H, Wf, 128), r(B, H, Wf, 128), r(B, H, Wf, 128)
        if name == "spectrum":
            for x in (x1, x2, x3):
                x *= 3000.0
                x[:, 0, 0] *= 40.0
    W0, W2, W4 = r(128, 256) / 16, r(128, 128) / 11, r(128, 128) / 11
    if name == "w4zero":
        W4 = torch.zeros_like(W4)
    return dict(x1=x1, x2=x2, x3=x3, W0=W0, W2=W2, W4=W4)


def mlp3_operands(p, nd):
    """(xa, xb) as (n_dirs, npix, 128)."""
    f = lambda x: x.reshape(-1, 128)
    return torch.stack([f(p["x1"]), f(p["x3"])][:nd]), torch.stack([f(p["x2"])] * nd)


def mlp3_cannot_differ(wrong, case):
    """dirswap needs a second direction; droptile a ninth tile of a two-direction launch.  With W4 = 0 nothing of the MLP reaches the
    result: the swapped concat, the missing ReLU and W2 <-> W4 (a zero layer 2: relu(0) = 0 into layer 4) leave every bit as it is.
    A residual taken from the staged bf16 copies is off by up to 2^-9 (|xa| + |xb|): where the result carries xa - xb at the sources'
    own size (`normal`, `spectrum`) that is the size of its store rounding 2^-8 |ref|, which the bound has to admit; it has to show
    where the residual cancels (`near`) and where nothing else is left (`w4zero`: four orders of magnitude)."""
    B, H, Wf, nd, _, _, name = case
    if wrong == "dirswap":
        return nd == 1
    if wrong == "droptile":
        return nd == 1 or B * H * Wf <= 1024
    if wrong == "resround":
        return name in ("normal", "spectrum")
    if wrong in ("xbxa", "w24", "norelu2"):
        return name == "w4zero"
    return False


def mlp3(xa, xb, W0, W2, W4, cd=D, wrong=None):
    """xa, xb (n_dirs, npix, 128) f32, W0 (128,256), W2, W4 (128,128) -> (n_dirs, npix, 128), stored as bf16.
    tau(256) S0; hidden 0 carried through |W2| + tau(128) S2; hidden 1 carried through |W4| + tau(128) S4; the two residual fmas; the
    bf16 store."""
    a_, b_ = xa.to(cd), xb.to(cd)
    nd = a_.shape[0]
    if wrong == "dirswap" and nd == 2:                       # WRONG: direction 1 computed from direction 0's xa
        a_ = torch.stack([a_[0], a_[0]])
    w0, w2, w4 = (rnd(w.to(cd), BF16) for w in (W0, W2, W4))
    if wrong == "w24":                                       # WRONG: layers 2 and 4 swapped
        w2, w4 = w4, w2
    v0 = rnd(torch.cat((b_, a_) if wrong == "xbxa" else (a_, b_), -1), BF16)     # xbxa WRONG: the concat the other way round
    a0, e0 = _layer(v0, None, w0, 256, cd)
    h0, c0 = _hidden(a0, e0)
    a1, e1 = _layer(h0, c0, w2, 128, cd)
    h1, c1 = _hidden(a1, e1, relu=wrong != "norelu2")        # norelu2 WRONG
    acc, e2 = _layer(h1, c1, w4, 128, cd)
    ra, rb = (rnd(a_, BF16), rnd(b_, BF16)) if wrong == "resround" else (a_, b_)   # resround WRONG: the staged bf16 copies
    ref = (acc + ra) + rb if wrong == "resadd" else (acc + ra) - rb               # resadd WRONG
    bound = e2 + 2 * EPS * (acc.double().abs() + xa.double().abs() + xb.double().abs()) + store(ref.double(), BF16)
    if wrong == "droptile" and nd == 2:                      # WRONG: the ninth tile (the tail of the first group of 8) never runs
        ref = ref.clone()
        ref[:, 1024:1152] = NAN
    return ref, bound


def mlp3_ref(p, nd, cd=D, wrong=None):
    xa, xb = mlp3_operands(p, nd)
    return mlp3(xa, xb, p["W0"], p["W2"], p["W4"], cd, wrong)


# ---- fcvsr_freq_head --------------------------------------------------------------------------------------------------------------------

WRONG_HEAD = ["nomid", "norelu", "rowperm", "srcoff"]
HEAD_NPIX = [1, 127, 128, 129, 414]
HEAD_STRIDES = {F32: [128, 384], BF16: [128, 256]}           # f32 at stride 384: the slice at channel offset 128 of a 384-float record


def _head_cases():
    """(source dtype, NHID, npix, x_pix_stride, set): all four instantiations at every size and stride; `spectrum` on the f32 source."""
    cases = [(dt, nhid, n, s, "normal") for dt in (F32, BF16) for nhid in (1, 2) for n in HEAD_NPIX for s in HEAD_STRIDES[dt]]
    return cases + [(F32, nhid, n, s, "spectrum") for nhid in (1, 2) for n in (1, 129, 414) for s in HEAD_STRIDES[F32]]


HEAD_CASES = _head_cases()


def head_tag(c):
    return f"{str(c[0])[6:]}-nhid{c[1]}-{c[2]}px-s{c[3]}-{c[4]}"


def head_inputs(dt, nhid, npix, stride, name):
    """rec (npix, stride) in dt: the pixel records as they lie in memory; the kernel's x is channels [off, off + 128) of each."""
    g = gen(72, dt == BF16, nhid, npix, stride, SETS.index(name))
    rec = torch.randn(npix, stride, generator=g)
    if name == "spectrum":
        rec *= 3000.0
        rec[0] *= 40.0
    off = 128 if stride == 384 else 0
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(rec=rec.to(dt), off=off, W0=r(64, 128) / 11, Wmid=r(64, 64) / 8 if nhid == 2 else None, Wl=r(4, 64) / 8)


def head_cannot_differ(wrong, case):
    """NHID = 1 has no middle layer to leave out; only the stride-384 slice has an offset to forget."""
    return (wrong == "nomid" and case[1] == 1) or (wrong == "srcoff" and case[3] != 384)


def head(x, W0, Wmid, Wl, cd=D, wrong=None, n0=128, ex=None, x0=None):
    """x (.., cin) bf16 or f32, W0 (64, cin), Wmid (64,64) or None, Wl (4,64) -> (.., 4) f32.  n0: the products of layer 0 the bound
    counts (128; 212 on the strip), ex: the error x carries (a computed source: the composition), x0: what `srcoff` reads instead."""
    if wrong == "srcoff" and x0 is not None:                 # WRONG: the slice read at channel offset 0
        x = x0
    v = rnd(x.to(cd), BF16)
    w0, wl = rnd(W0.to(cd), BF16), rnd(Wl.to(cd), BF16)
    a, e = _layer(v, ex, w0, n0, cd)
    h, c = _hidden(a, e, relu=wrong != "norelu")             # norelu WRONG: layer 0's ReLU missing
    if Wmid is not None and wrong != "nomid":                # nomid WRONG
        a, e = _layer(h, c, rnd(Wmid.to(cd), BF16), 64, cd)
        h, c = _hidden(a, e)
    out, bound = _layer(h, c, wl, 64, cd)
    if wrong == "rowperm":                                   # WRONG: the four output rows in another order
        out = out[..., [1, 2, 3, 0]]
    return out, bound


def head_ref(p, cd=D, wrong=None):
    o = p["off"]
    return head(p["rec"][:, o:o + 128], p["W0"], p["Wmid"], p["Wl"], cd, wrong, x0=p["rec"][:, :128])


# ---- fcvsr_convcorr_strip ---------------------------------------------------------------------------------------------------------------

WRONG_STRIP = ["pitch", "noshare", "pad84", "nocorr"]
# B = 3, H = 5, xs = 8: 240 strip pixels, the direction boundary at pixel 120 inside the first tile, a partial second tile
STRIP_CASES = [(B, H, Wf, xs) for B in (1, 3) for H in (1, 5) for (Wf, xs) in [(5, 5), (8, 8), (19, 8), (19, 3)]]


def strip_inputs(B, H, Wf, xs):
    """off (2B,H,Wf,128) bf16; corr (B,H,xs,84) f32, a tensor of its own (not a lookup) whose three pad channels hold finite non-zero
    values; W0 (64, 209): the packed matrix has zero pad columns; Wpad (64, 3): the weights `pad84` gives them."""
    g = gen(73, B, H, Wf, xs)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(off=r(2 * B, H, Wf, 128).to(BF16), corr=r(B, H, xs, 84) * 0.5, W0=r(64, 209) / 14, W2=r(64, 64) / 8, W4=r(4, 64) / 8,
                Wpad=r(64, 3) / 14)


def strip_cannot_differ(wrong, case):
    """With xs = Wf the strip is the grid: both pitches agree."""
    return wrong == "pitch" and case[2] == case[3]


def strip(off, corr, W0, W2, W4, B, H, Wf, xs, cd=D, wrong=None, Wpad=None):
    """off (2B,H,Wf,128) bf16, corr (B,H,xs,84) f32, W0 (64,209), W2 (64,64), W4 (4,64) -> (2B,H,Wf,4) f32, NaN at columns >= xs.
    head's bound with n = 212 for layer 0 (128 + 84 staged channels)."""
    if wrong == "pitch":                                     # WRONG: strip pixel p read at grid pixel p (pitch xs, not Wf)
        o = off.reshape(-1, 128)[:2 * B * H * xs].reshape(2 * B, H, xs, 128)
    else:
        o = off[:, :, :xs]
    look, w0 = corr[..., :81], W0
    if wrong == "pad84":                                     # WRONG: the pad channels multiply weights of their own
        look, w0 = corr, torch.cat([W0, Wpad], 1)
    look = torch.cat([look, torch.zeros_like(look) if wrong == "noshare" else look])     # noshare WRONG: direction 1 without lookup
    if wrong == "nocorr":                                    # WRONG
        look = torch.zeros_like(look)
    v, b = head(torch.cat([o.float(), look], -1), w0, W2, W4, cd, n0=212)
    ref = torch.full((2 * B, H, Wf, 4), NAN, dtype=v.dtype)
    bound = torch.zeros(2 * B, H, Wf, 4, dtype=D)
    ref[:, :, :xs], bound[:, :, :xs] = v, b
    return ref, bound


def strip_ref(p, case, cd=D, wrong=None):
    return strip(p["off"], p["corr"], p["W0"], p["W2"], p["W4"], *case, cd=cd, wrong=wrong, Wpad=p["Wpad"])


# ---- the engine's decomposition: head on `off` over the grid, then the strip over the lookup columns ------------------------------------

COMPOSE_CASES = [(2, 5, 5), (2, 5, 8), (2, 5, 19)]          # (B, H, Wf); the engine's xs = min(Wf, 8)


def compose_inputs(B, H, Wf):
    g = gen(74, B, H, Wf)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x1f=r(B, H, Wf, 128), x2f=r(B, H, Wf, 128), off=r(2 * B, H, Wf, 128).to(BF16), W0=r(64, 209) / 14, W2=r(64, 64) / 8,
                W4=r(4, 64) / 8)


def convcorr_full(p, cd=D):
    """convcorr on [off | CorrBlock lookup] over the WHOLE (2B,H,Wf) grid, the lookup at full width in f64 (freq_kernel_refs.corr_lookup,
    both directions share it).  The device lookup is an f32 kernel result within its own derived bound of that; rounded to bf16 it
    carries spread(lookup, bound, bf16) (capped as a hidden value's) into layer 0 through |W0|."""
    look, lb = corr_lookup(p["x1f"], p["x2f"], 128, p["x1f"].shape[2])
    look, lb = look[..., :81], lb[..., :81]
    ex = torch.minimum(spread(look, lb, BF16), ulp(rnd(look, BF16)))
    off = p["off"]
    x = torch.cat([off.double(), torch.cat([look, look])], -1)
    ex = torch.cat([torch.zeros(off.shape, dtype=D), torch.cat([ex, ex])], -1)
    return head(x, p["W0"], p["W2"], p["W4"], cd, n0=212, ex=ex)
