"""Float64 CPU references of the IAC forward kernels, written per element from the formulas in the kernel file headers (iac.hip:1-10,
mgaa.hip:96-168); nothing here calls fcvsr_amd.hip.  Tensors are NHWC as the kernels see them: prev / feat_in / out (B,H,W,C), off
(B,H,W,2) f32 with channel 0 = x, K (B,H,W,3C) with channel c*3+t.  Each reference returns (ref, bound): f64 tensors of the output's
shape, `bound` the error a correct kernel may show at that element.  tests/test_iac_refs_cpu.py pins the references to the oracle and
shows that the bounds reject wrong kernels; tests/test_iac_kernels_gpu.py asserts |got - ref| <= bound for every element.

    out = LeakyReLU_slope( SAC_h( SAC_v( warp(prev, off), K ), K ) + feat_in )

What a bound is made of (the rules of infer_kernel_refs): k * 2^-24 * S, S = the same expression on absolute values, k = the rounded
f32 operations on the longest path to one output, counted from the kernel source; u * |ref| for a 16-bit store (`store`).
  warp     The sampling position is the F32 value the kernels form, fx = f32(gx) + off_x (one rounded add), and the reference forms it
           in f32 too: floor(fx), and with it the choice of the four taps, is then the kernels' own by construction, at every offset.
           Everything after it is f64.  wx1 = fx - floor(fx) is exact in f32 for fx >= 0; for -1 <= fx < 0 it is one rounding and the
           tap that would carry wx0 lies outside the image; wx0 = 1 - wx1 is one rounding.  So each 1-D weight of a tap INSIDE the image
           is within one rounding [1] (x and y in parallel [+1]), their product [3], then at most four chained fmas [7]: K_WARP = 7 on
           S = sum w |prev|.  (An evaluation without fma - product, then three sums that are not 0 + x - has the same count.)
           Outside (-2, W+1) x (-2, H+1), or not finite: zero, bound zero (the kernels' guard before the float-to-int conversion).
  SAC      three chained fmas per pass: K_SAC = 3 each.  The warp's error reaches the output through both passes weighted by |K|: with
           S_v = sum_t |K| S_s and S_h = sum_t |K| S_v (the halo column of v = v at the clamped column, with K of the clamped column)
           the error before the residual is (7 + 3 + 3) 2^-24 S_h.
  residual h + feat_in [+1]: k = 14 on S = S_h + |feat_in|; call it e.
  LeakyReLU the select form r >= 0 ? r : r * slope with the f32 slope the kernel receives: e passes with factor 1 (r > e), |slope|
           (r < -e), or - where |r| <= e and the kernel's r may sit on the other side of zero - max(1, |slope|, |slope| + |1 - slope|);
           the product is one more rounding, 2^-24 |ref|.
  store    u |ref| for a 16-bit output (never below half of f16's subnormal spacing), nothing for f32.
K and the features are used as stored: 16-bit inputs are exact in f32 and in f64.

The keywords `pad`, `swap`, `pad_v`, `pad_h`, `taps`, `halo`, `same_off` and iac_step_tiled's `stale` select deliberately WRONG variants;
only tests/test_iac_refs_cpu.py passes them.  `cd` is the dtype the arithmetic after the position runs in: float64, or float32 for that
file's "a correct f32 evaluation stays inside the bound" check."""
import numpy as np
import torch

from infer_kernel_refs import BF16, D, EPS, F16, F32, f32, gen, shape_seed, store  # noqa: F401  (re-exported for the two test files)

K_WARP, K_SAC = 7, 3
K_STEP = K_WARP + 2 * K_SAC + 1
DT_CODE = {F32: 0, BF16: 1, F16: 2}


# ---- warp ---------------------------------------------------------------------------------------------------------------------------

def positions(off, swap=False):
    """The f32 sampling positions (fx, fy), each (B,H,W): f32(gx) + off_x, one rounded f32 add.  swap = True is WRONG (x from channel 1)."""
    _, H, W, _ = off.shape
    ox, oy = (off[..., 1], off[..., 0]) if swap else (off[..., 0], off[..., 1])
    fx = torch.arange(W, dtype=F32).view(1, 1, W) + ox.float()
    fy = torch.arange(H, dtype=F32).view(1, H, 1) + oy.float()
    return fx, fy


def sample(prev, fx, fy, cd=D, pad="zeros"):
    """prev (B,H,W,C) sampled bilinearly at the f32 positions fx, fy (B,h,w) -> value (B,h,w,C) in cd and S (f64), the same sum on
    absolute values.  Taps outside the image contribute zero; a position outside (-2, W+1) x (-2, H+1) or not finite gives zero."""
    B, H, W, Cn = prev.shape
    h, w = fx.shape[1:]
    sane = (fx > -2.0) & (fx < float(W) + 1.0) & (fy > -2.0) & (fy < float(H) + 1.0)          # NaN compares false
    px = torch.where(sane, fx, torch.full_like(fx, -4.0)).to(cd)
    py = torch.where(sane, fy, torch.full_like(fy, -4.0)).to(cd)
    x0, y0 = px.floor(), py.floor()
    wx1, wy1 = px - x0, py - y0
    wx, wy = (1.0 - wx1, wx1), (1.0 - wy1, wy1)
    p, pa = prev.to(cd).reshape(B, H * W, Cn), prev.double().abs().reshape(B, H * W, Cn)
    val, S = torch.zeros(B, h, w, Cn, dtype=cd), torch.zeros(B, h, w, Cn, dtype=D)
    for dy in range(2):
        for dx in range(2):
            xi, yi = x0.long() + dx, y0.long() + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            if pad == "clamp":                                 # WRONG: the clamped sample keeps its weight
                ok = sane
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, h * w, 1).expand(B, h * w, Cn)
            wgt = wy[dy] * wx[dx] * ok.to(cd)
            val = val + p.gather(1, idx).view(B, h, w, Cn) * wgt[..., None]
            S = S + pa.gather(1, idx).view(B, h, w, Cn) * wgt.double().abs()[..., None]
    return val, S


def warp_parts(prev, off, cd=D, pad="zeros", swap=False):
    fx, fy = positions(off, swap)
    return sample(prev, fx, fy, cd, pad)


def warp(prev, off, cd=D, pad="zeros", swap=False):
    """fcvsr_warp / phase 1 of the fused kernels.  k = K_WARP = 7 (module docstring)."""
    val, S = warp_parts(prev, off, cd, pad, swap)
    return val, K_WARP * EPS * S


# ---- SAC passes ----------------------------------------------------------------------------------------------------------------------

def shift(t, d, axis, pad="replicate"):
    """t at index i + d along `axis`: clamped (replicate padding), or zero outside (pad = "zeros", WRONG for the SAC)."""
    n = t.shape[axis]
    idx = torch.arange(n) + d
    r = t.index_select(axis, idx.clamp(0, n - 1))
    if pad != "replicate":
        view = [1] * t.dim()
        view[axis] = n
        r = r * ((idx >= 0) & (idx < n)).to(t.dtype).view(view)
    return r


def ktap(K, t, taps="fwd"):
    """Tap t of every channel: K[..., c*3 + t].  taps = "reversed" is WRONG."""
    return K[..., (2 - t if taps == "reversed" else t)::3]


def sac(s, Ss, K, axis, cd=D, pad="replicate", taps="fwd"):
    """sum_t s[i + t - 1] * K[.., c*3+t] along `axis` (1 = vertical, 2 = horizontal), and the same sum of Ss (f64, >= |s|) with |K|."""
    acc, S = 0.0, 0.0
    for t in range(3):
        acc = acc + shift(s.to(cd), t - 1, axis, pad) * ktap(K, t, taps).to(cd)
        S = S + shift(Ss, t - 1, axis, pad) * ktap(K, t, taps).double().abs()
    return acc, S


def sac_v(s, K, cd=D, pad="replicate", taps="fwd"):
    """fcvsr_sac_v on a given s (B,H,W,C) f32: k = K_SAC = 3 on S = sum_t |s| |K|."""
    v, S = sac(s, s.double().abs(), K, 1, cd, pad, taps)
    return v, K_SAC * EPS * S


def lrelu(r, e, slope, cd, dt):
    """The select form with the f32 slope, and its bound from e = the bound of r (module docstring)."""
    s = f32(slope)
    out = torch.where(r >= 0, r, r * torch.tensor(s, dtype=cd))
    rd = r.double()
    m = torch.where(rd.abs() > e, torch.where(rd >= 0, torch.ones_like(rd), torch.full_like(rd, abs(s))),
                    torch.full_like(rd, max(1.0, abs(s), abs(s) + abs(1.0 - s))))
    return out, m * e + EPS * out.double().abs() + store(out.double(), dt)


def sac_h(v, K, fin, slope, cd=D, pad="replicate", taps="fwd"):
    """fcvsr_sac_h on a given v: three fmas, the residual, the slope: k = 4 on S = sum_t |v| |K| + |feat_in| before the LeakyReLU."""
    h, S = sac(v, v.double().abs(), K, 2, cd, pad, taps)
    r = h + fin.to(cd)
    return lrelu(r, (K_SAC + 1) * EPS * (S + fin.double().abs()), slope, cd, None)


def iac_tail(s, Ss, K, fin, slope, adt, cd=D, pad_v="replicate", pad_h="replicate", taps="fwd", halo=None):
    """Both SAC passes, residual and LeakyReLU on a warped s with majorant Ss.  halo = tw is WRONG: the column of v left of a tile's
    first column and right of its last one (tiles tw wide) is formed with the K of the tile's own edge column."""
    v, Sv = sac(s, Ss, K, 1, cd, pad_v, taps)
    if halo is None:
        h, Sh = sac(v, Sv, K, 2, cd, pad_h, taps)
    else:
        W = s.shape[2]
        x = torch.arange(W).view(1, 1, W, 1)
        vl = sac(shift(s, -1, 2), Ss, K, 1, cd, pad_v, taps)[0]
        vr = sac(shift(s, 1, 2), Ss, K, 1, cd, pad_v, taps)[0]
        cols = (torch.where(x % halo == 0, vl, shift(v, -1, 2)), v, torch.where(x % halo == halo - 1, vr, shift(v, 1, 2)))
        h = sum(cols[t] * ktap(K, t, taps).to(cd) for t in range(3))
        Sh = sac(v, Sv, K, 2, cd, pad_h, taps)[1]
    r = h + fin.to(cd)
    return lrelu(r, K_STEP * EPS * (Sh + fin.double().abs()), slope, cd, adt)


def iac_step(prev, off, K, fin, slope, adt=None, cd=D, pad="zeros", swap=False, **tail):
    """fcvsr_iac_step (one direction of fcvsr_iac_step2 / _fused): k = K_STEP = 14 before the LeakyReLU (module docstring); adt = the
    dtype the output is stored in."""
    s, Ss = warp_parts(prev, off, cd, pad, swap)
    return iac_tail(s, Ss, K, fin, slope, adt, cd, **tail)


def iac_step2(prevs, offs, K, fins, slope, adt=None, cd=D, same_off=False):
    """Both directions with one K.  same_off = True is WRONG: direction 1 warped with direction 0's offsets."""
    return [iac_step(prevs[d], offs[0 if same_off else d], K, fins[d], slope, adt, cd) for d in range(2)]


def iac_step_tiled(prev, off, K, fin, slope, tw, th=4, stale=False):
    """The step evaluated the way the fused kernels walk it: tiles of th x tw pixels in the order (image, tile row, tile column), each
    with its own warped halo tile of (th + 2) x (tw + 2) clamped pixels.  stale = False reproduces iac_step's reference.  stale = True
    is WRONG: every tile after the first is warped with the offsets that the PREVIOUS tile of the run loaded for the same halo slots."""
    B, H, W, Cn = prev.shape
    out = torch.zeros(B, H, W, Cn, dtype=D)
    Kd, find, s32 = K.double(), fin.double(), f32(slope)
    last = None
    for b in range(B):
        for ty0 in range(0, H, th):
            for tx0 in range(0, W, tw):
                gy = (torch.arange(th + 2) + ty0 - 1).clamp(0, H - 1)
                gx = (torch.arange(tw + 2) + tx0 - 1).clamp(0, W - 1)
                here = off[b][gy][:, gx]                                            # (th+2, tw+2, 2)
                o = last if stale and last is not None else here
                last = here
                fx = gx.to(F32).view(1, 1, -1) + o[..., 0].float()[None]
                fy = gy.to(F32).view(1, -1, 1) + o[..., 1].float()[None]
                s = sample(prev[b:b + 1], fx, fy)[0][0]                            # (th+2, tw+2, C)
                ky = (torch.arange(th) + ty0).clamp(0, H - 1)
                kh = Kd[b][ky][:, gx]                                               # K of the v domain's (clamped) pixels
                v = sum(s[t:t + th] * kh[..., t::3] for t in range(3))              # (th, tw+2, C)
                kc = kh[:, 1:tw + 1]
                r = sum(v[:, t:t + tw] * kc[..., t::3] for t in range(3))
                ny, nx = min(th, H - ty0), min(tw, W - tx0)
                r = r[:ny, :nx] + find[b, ty0:ty0 + ny, tx0:tx0 + nx]
                out[b, ty0:ty0 + ny, tx0:tx0 + nx] = torch.where(r >= 0, r, r * s32)
    return out


# ---- inputs shared by the GPU tests and the CPU discrimination test -----------------------------------------------------------------

SHAPES = [(1, 1, 1), (2, 1, 9), (2, 9, 1), (1, 4, 14), (1, 4, 16), (2, 5, 15), (2, 5, 17), (3, 5, 3), (2, 22, 37)]   # (B, H, W)
PARTIAL = [(2, 5, 15), (2, 5, 17), (3, 5, 3), (2, 22, 37)]
SLOPES = [0.1, 1.5]
AXES = ("x", "y", "xy")
MAX_PLANTS = 288


def below(n):
    """The largest f32 below n."""
    return float(np.nextafter(np.float32(n), np.float32(0)))


def plant_values(n):
    """(class, kind, value) of one axis of size n: kind "off" = the offset itself, "pos" = the sampling position (offset = value - g,
    exact in f32 for these values, so f32(g + offset) IS the position)."""
    big = [("1e4", 1e4), ("3e9", 3e9), ("3.4e38", 3.4e38), ("inf", float("inf"))]
    return ([("off+0", "off", 0.0), ("off-0", "off", -0.0), ("off+1", "off", 1.0), ("off-1", "off", -1.0), ("off+2", "off", 2.0),
             ("off-3", "off", -3.0), ("pos-1", "pos", -1.0), ("pos-0.5", "pos", -0.5), ("pos0", "pos", 0.0), ("posN-1", "pos", n - 1.0),
             ("posN-0.5", "pos", n - 0.5), ("posN", "pos", float(n)), ("belowN", "pos", below(n)), ("tiny+", "off", 1e-8),
             ("tiny-", "off", -1e-8)] + [(s + nm, "off", (1 if s == "+" else -1) * v) for nm, v in big for s in "+-"] + [("nan", "off", float("nan"))])


CLASSES = [c for c, _, _ in plant_values(4)]


def offsets(B, H, W, key=0):
    """(B,H,W,2) f32: randn * 3, and at up to MAX_PLANTS pixels (a quarter of the field at most: planted positions far outside the image
    leave zeros, and a field of zeros tells no SAC variant from another) taken from a fixed permutation of all pixels - so edge, corner
    and interior tiles all receive some - one planted class each, cycling through every
    (class, axis) pair: x only, y only (the other component stays randn * 3), or both.  tiny+- go to a coordinate > 0, where
    f32(g + off) rounds back onto g.  The corner pixels of the first and the last image carry +0 in both components (class off+0 / xy)
    whatever the permutation put there: a corner of s that is prev's own corner - not zero - is what lets the padding of either SAC
    pass show at every shape, the one-row and one-column ones included, where randn * 3 leaves most of s zero."""
    g = gen(7, B, H, W, key)
    off = torch.randn(B, H, W, 2, generator=g) * 3.0
    N = B * H * W
    order = torch.randperm(N, generator=g).tolist()
    variants = [(c, kind, ax) for ax in AXES for c, kind, _ in plant_values(4)]
    rot = shape_seed(B, H, W, key) % len(variants)
    used, ptr = set(), 0
    for i in range(min(max(1, N // 4), MAX_PLANTS)):
        cls, kind, ax = variants[(i + rot) % len(variants)]
        need = cls.startswith("tiny")
        j = ptr
        while j < N:
            p = order[j]
            y, x = (p // W) % H, p % W
            if p not in used and not (need and (("x" in ax and x == 0) or ("y" in ax and y == 0))):
                break
            j += 1
        if j == N:
            continue
        used.add(p)
        while ptr < N and order[ptr] in used:
            ptr += 1
        b = p // (H * W)
        for ch, coord, n in ((0, x, W), (1, y, H)):
            if AXES[2][ch] in ax:
                val = dict((c, v) for c, _, v in plant_values(n))[cls]
                off[b, y, x, ch] = val - coord if kind == "pos" else val
    for b in {0, B - 1}:                                      # see the docstring: the corners sample themselves
        for y in {0, H - 1}:
            for x in {0, W - 1}:
                off[b, y, x] = 0.0
    return off


def axis_classes(o, g, n):
    """Masks (B,H,W) of every class for one offset component o with coordinate grid g (f32) on an axis of size n."""
    f = g + o
    fin = torch.isfinite(o)
    m = {"off+0": (o == 0) & ~torch.signbit(o), "off-0": (o == 0) & torch.signbit(o)}
    for c, v in (("off+1", 1.0), ("off-1", -1.0), ("off+2", 2.0), ("off-3", -3.0)):
        m[c] = o == v
    for c, v in (("pos-1", -1.0), ("pos-0.5", -0.5), ("pos0", 0.0), ("posN-1", n - 1.0), ("posN-0.5", n - 0.5), ("posN", float(n)),
                 ("belowN", below(n))):
        m[c] = f == v
    for s, sg in (("+", 1.0), ("-", -1.0)):
        so = o * sg
        m["tiny" + s] = (so > 0) & (so < 1e-6) & (g > 0) & (f == g)
        m[s + "1e4"] = fin & (so >= 5e3) & (so <= 1e6)
        m[s + "3e9"] = fin & (so >= 1e9) & (so <= 1e10)
        m[s + "3.4e38"] = fin & (so >= 1e38)
        m[s + "inf"] = torch.isinf(o) & (so > 0)
    m["nan"] = torch.isnan(o)
    return m


def class_counts(off):
    """{(class, axis): pixels}: axis "x" / "y" = that component is of the class and the other one of no class at all, "xy" = both."""
    _, H, W, _ = off.shape
    mx = axis_classes(off[..., 0], torch.arange(W, dtype=F32).view(1, 1, W).expand(off.shape[:3]), W)
    my = axis_classes(off[..., 1], torch.arange(H, dtype=F32).view(1, H, 1).expand(off.shape[:3]), H)
    anyx, anyy = torch.stack(list(mx.values())).any(0), torch.stack(list(my.values())).any(0)
    out = {}
    for c in CLASSES:
        out[c, "x"], out[c, "y"], out[c, "xy"] = int((mx[c] & ~anyy).sum()), int((my[c] & ~anyx).sum()), int((mx[c] & my[c]).sum())
    return out


def full_coverage(B, H, W):
    """Shapes large enough that `offsets` plants every (class, axis) pair: room for all of them, and coordinates > 0 on both axes."""
    return B * H * W >= 12 * len(CLASSES) and H > 1 and W > 1


def step_inputs(B, H, W, Cn, adt, kdt, key=0):
    """prev, feat_in (B,H,W,Cn) in adt, K (B,H,W,3 Cn) in kdt: finite randn rounded to the storage dtype; off: `offsets`."""
    g = gen(8, B, H, W, Cn, DT_CODE[adt], DT_CODE[kdt], key)
    return dict(prev=torch.randn(B, H, W, Cn, generator=g).to(adt), fin=torch.randn(B, H, W, Cn, generator=g).to(adt),
                K=torch.randn(B, H, W, 3 * Cn, generator=g).to(kdt), off=offsets(B, H, W, key))
