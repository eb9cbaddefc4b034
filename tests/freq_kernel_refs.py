"""Float64 CPU references of the f32 kernels of the frequency branch and of the ContextBlock pooling, written per element from the
formulas in the kernel file headers (mgaa.hip, reduce.h, convblk.hip, mffr.hip, scnet.hip); nothing here calls fcvsr_amd.hip.  These are
the kernels every bit-equality chain of the suite ends on: fcvsr_corr_lookup, fcvsr_channel_sum, fcvsr_ca_gate, fcvsr_convblk_tail,
fcvsr_convblk, fcvsr_divenh / fcvsr_divenh_apply_next and fcvsr_gc_context / fcvsr_gc_partial_levels / fcvsr_gc_finish(_levels).
tests/test_freq_kernel_refs_cpu.py pins the references to torch / the oracle and shows that the bounds reject wrong kernels;
tests/test_freq_kernels_gpu.py compares the kernels with them through the C ABI.  Conventions as in tests/infer_kernel_refs.py.

Two kinds of result:
  derived   (ref, bound): |got - ref| <= bound per element.  f32 arithmetic k * 2^-24 * S, S = the same expression on absolute values,
            k = the rounded operations on the longest path, counted from the kernel source (the library is built with
            -ffp-contract=off: a*t*f + b*f is four roundings, only explicit fmaf calls fuse).  A sum of n terms in the kernel's order:
            tau(n) * S (tests/tolerance.py), plus k * 2^-24 * S for the k roundings inside each term.
  measured  (ref, scale): results behind an expf - the CALayer gate (sigmoid), the ConvBlk record, the ContextBlock vector (softmax).
            scale is the entry's own condition by the rules of tests/train_block_refs.py: absolute values of the direct terms, a
            product with a small matrix on absolute values, sigmoid g as g + g (1 - g) S(s), softmax m_p as
            Sm_p = m_p (1 + L_p + sum_q m_q L_q) with L_p = sum_c |wmask_c r_pc|.  The GPU test bounds |got - ref| / scale by 8 x the
            case's own measured worst and requires that to stay below `*_rejection`: the smallest worst-ratio over the kernel's wrong
            variants at the same inputs.

`cd` is the dtype the arithmetic runs in (float64, or float32 for the "a correct f32 evaluation stays inside the bound" check);
`wrong` selects a deliberately WRONG variant, listed per kernel in `*_WRONG`; only the CPU file and the rejection figures pass it."""
import math

import torch
import torch.nn.functional as F

from infer_kernel_refs import BF16, D, EPS, F16, F32, f32, gen
from tolerance import tau

INF = float("inf")


def _ratio(err, scale):
    """Worst |err| / scale; scale = 0 must be exact; a non-finite wrong value counts as infinitely far."""
    err = torch.nan_to_num(err.double().abs(), nan=INF, posinf=INF)
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ---- 1. fcvsr_corr_lookup (mgaa.hip) -------------------------------------------------------------------------------------------------

CORR_WRONG = ["rowcol", "cutC", "ppch", "divC"]
# (B, C, H, Wf, pix_stride): C = 128 and 64; H = 1, 63, 64, 65 around the 64-row image of C = 128, 72 beyond it; Wf = 1, 2, 5, 6, 9
CORR_CASES = [(1, 128, 1, 1, 128), (3, 128, 63, 2, 128), (1, 128, 64, 5, 160), (1, 128, 65, 6, 128), (3, 128, 72, 9, 160),
              (1, 64, 1, 2, 96), (3, 64, 63, 5, 64), (1, 64, 65, 9, 64), (1, 64, 72, 6, 80), (3, 64, 64, 1, 64)]


def corr_inputs(B, Cn, H, Wf, ps):
    g = gen(41, B, Cn, H, Wf, ps)
    return torch.randn(B, H, Wf, ps, generator=g), torch.randn(B, H, Wf, ps, generator=g)


def corr_cannot_differ(wrong, B, Cn, H, Wf):
    """cutC admits rows C/2 <= y + j - r < C: none exists while H + 3 < C/2.  ppch: with a single pixel both readings of the flat
    offset e agree (pp = 0, ch = e)."""
    return (wrong == "cutC" and H + 3 < Cn // 2) or (wrong == "ppch" and H * Wf == 1)


def corr_lookup(x1f, x2f, Cn, xw, radius=4, nch=84, cd=D, wrong=None):
    """x1f, x2f (B,H,Wf,ps) f32 NHWC (channels [0, C) used) -> (B,H,xw,nch): channel c = i*n + j (n = 2r+1) of pixel (y, x) is
    P[e] = x1f x2f / sqrt(C) at the flat NCHW offset e = (y*Wf + x)*C + row*2 + col of the batch item, row = y + j - r in [0, C/2),
    col = x + i - r in {0, 1}; e names channel e // HW of pixel e % HW.  Zero elsewhere and in channels >= n*n (exactly).
    f32 arithmetic: the product [1], the division by the f32 sqrt(C) [2] (correctly rounded): k = 2 on S = |ref|."""
    B, H, Wf, _ = x1f.shape
    n, HW = 2 * radius + 1, H * Wf
    c = torch.arange(nch).view(1, 1, nch)
    y = torch.arange(H).view(H, 1, 1)
    x = torch.arange(xw).view(1, xw, 1)
    i, j = c // n, c % n
    if wrong == "rowcol":                                    # WRONG: i moves the row, j the column
        i, j = j, i
    col, row = x + i - radius, y + j - radius
    ok = (c < n * n) & (col >= 0) & (col <= 1) & (row >= 0) & (row < (Cn if wrong == "cutC" else Cn // 2))   # cutC WRONG: cut-off at C
    e = ((y * Wf + x) * Cn + row * 2 + col).clamp(0, Cn * HW - 1)
    if wrong == "ppch":                                      # WRONG: the offset read as NHWC (pixel-major)
        pp, ch = e // Cn, e % Cn
    else:
        ch, pp = e // HW, e % HW
    a = x1f.to(cd).reshape(B, HW, -1)[:, pp, ch] * x2f.to(cd).reshape(B, HW, -1)[:, pp, ch]
    v = a / (float(Cn) if wrong == "divC" else f32(math.sqrt(Cn)))                                          # divC WRONG
    v = torch.where(ok, v, torch.zeros_like(v))
    return v, 2 * EPS * v.double().abs()


# ---- 2. fcvsr_channel_sum (mgaa.hip, reduce.h) ----------------------------------------------------------------------------------------

SUM_WRONG = ["lastpix", "lastblk", "sublane"]
# (B, C, H, W): HW = 1 / 255 / 256 / 257 / 289 at C = 4 (ConvBlk's use; R = 64 sub-lanes); nblk = 28 / 29 / 33 at C = 64 around
# stage 2's blk + 7R < nblk loop (R = 4); nblk = 449 at C = 4, where its unrolled loop runs (448 < nblk); C = 3 and 12 (256 % C != 0:
# idle sub-lanes), C = 256 (R = 1)
SUM_CASES = [(1, 4, 1, 1), (3, 4, 15, 17), (1, 4, 16, 16), (3, 4, 1, 257), (1, 4, 17, 17), (1, 64, 31, 223), (3, 64, 67, 107),
             (1, 64, 7, 1171), (1, 4, 1, 114721), (3, 3, 257, 1), (1, 12, 17, 17), (3, 256, 1, 257), (1, 256, 1, 1)]
assert [-(-h * w // 256) for _, _, h, w in SUM_CASES[5:9]] == [28, 29, 33, 449]


def sum_inputs(B, Cn, H, W):
    """randn; the last pixel carries +-max(1, HW/256) so that its loss shows against tau(n) * S at every size."""
    g = gen(42, B, Cn, H, W)
    x = torch.randn(B, H, W, Cn, generator=g)
    sign = 1.0 - 2.0 * (torch.arange(B * Cn).view(B, Cn) % 2)
    x[:, H - 1, W - 1] = sign * max(1.0, H * W / 256.0)
    return x


def sum_cannot_differ(wrong, Cn, HW):
    """Sub-lane R - 1 (R = 256 // C) owns the pixels q of a block with q % R == R - 1: none while HW < R."""
    return wrong == "sublane" and HW < 256 // Cn


def channel_sum(x, cd=D, wrong=None):
    """x (B,H,W,C) -> (B,C) sums over the pixels.  tau(HW) * S, S = the sum of |x|."""
    B, H, W, Cn = x.shape
    HW = H * W
    v = x.to(cd).reshape(B, HW, Cn)
    keep = torch.ones(HW, dtype=torch.bool)
    if wrong == "lastpix":
        keep[-1] = False
    elif wrong == "lastblk":
        keep[(HW - 1) // 256 * 256:] = False
    elif wrong == "sublane":
        R = 256 // Cn
        keep[(torch.arange(HW) % 256) % R == R - 1] = False
    return (v * keep.to(cd)[None, :, None]).sum(1), tau(HW) * v.double().abs().sum(1)


# ---- 3. fcvsr_ca_gate (mgaa.hip) ------------------------------------------------------------------------------------------------------

GATE_WRONG = ["w1t", "norelu", "invhw2"]
# (c, cr, B, neg); c = 128 is above the 64-thread block; neg: every hidden unit negative, ReLU all zero, the gate exactly 0.5
GATE_CASES = [(c, cr, B, False) for (c, cr) in [(4, 4), (64, 4), (64, 16), (128, 8)] for B in (1, 5)] + [(64, 4, 5, True), (4, 4, 1, True)]
GATE_HW = 399


def gate_tag(c, cr, B, neg):
    return f"c{c} cr{cr} B{B}" + (" neg" if neg else "")


def gate_inputs(c, cr, B, neg):
    g = gen(43, c, cr, B, neg)
    s = torch.randn(B, c, generator=g) * GATE_HW * 0.5
    w1, w2 = torch.randn(cr, c, generator=g) / math.sqrt(c), torch.randn(c, cr, generator=g)
    if neg:
        s, w1 = s.abs(), -w1.abs()
    return dict(sum=s, inv_hw=1.0 / GATE_HW, w1=w1, w2=w2)


def gate_cannot_differ(wrong, neg):
    """With positive sums and a negative W1 the hidden layer is negative whichever way W1 is read and however often 1/HW is
    applied: only the missing ReLU shows."""
    return neg and wrong in ("w1t", "invhw2")


def ca_gate(s, inv_hw, w1, w2, cd=D, wrong=None):
    """CALayer gate (:1812-1828): sum (B,c), w1 (cr,c), w2 (c,cr) -> sigmoid(W2 relu(W1 (sum * inv_hw))), and its scale."""
    cr, c = w1.shape
    inv = f32(inv_hw)
    mean = s.to(cd) * inv * (inv if wrong == "invhw2" else 1.0)
    W1 = w1.reshape(c, cr).t() if wrong == "w1t" else w1     # WRONG: the flat buffer read as [c][cr]
    pre = mean @ W1.to(cd).t()
    hid = pre if wrong == "norelu" else torch.relu(pre)
    sg = torch.sigmoid(hid @ w2.to(cd).t())
    S_pre = (s.double().abs() * inv) @ w1.double().abs().t()
    S_s = (S_pre * (pre.double() > 0)) @ w2.double().abs().t()
    return sg, sg.double() * (1.0 + (1.0 - sg.double()) * S_s)


def gate_rejection(c, cr, B, neg):
    p = gate_inputs(c, cr, B, neg)
    ref, scale = ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"])
    return min(_ratio(ca_gate(p["sum"], p["inv_hw"], p["w1"], p["w2"], wrong=w)[0] - ref, scale)
               for w in GATE_WRONG if not gate_cannot_differ(w, neg))


# ---- 4. fcvsr_convblk_tail (mgaa.hip) -------------------------------------------------------------------------------------------------

TAIL_WRONG = ["nogateplus", "reim", "dirhead"]
TAIL_CASES = [(ndir, B, H, W) for ndir in (1, 2) for B in (1, 3) for (H, W) in [(1, 1), (15, 17), (1, 257)]]
SENTINEL = -777.25


def tail_inputs(ndir, B, H, W):
    g = gen(44, ndir, B, H, W)
    return dict(u=torch.randn(ndir * B, H, W, 4, generator=g), gate=torch.rand(ndir * B, 4, generator=g),
                sim=torch.randn(B, H, W, 4, generator=g))


def tail_cannot_differ(wrong, ndir, g0):
    """A [head][dir] record has pair g0 * ndir + dir where the kernel's [dir][head] has g0 + dir * A: the same for one direction."""
    return wrong == "dirhead" and ndir == 1


def record(o, S, B, ndir, A, g0, ps, re_off, im_off, k, wrong=None):
    """o, S (ndir*B,H,W,4): (re0, re1, im0, im1) of pair g0 of each direction -> the (B,H,W,ps) record: ref (NaN where the call owns
    nothing), bound / scale (k * 2^-24 * S, or S itself for k = None) and the mask of the floats the call owns."""
    _, H, W, _ = o.shape
    ref = torch.full((B, H, W, ps), float("nan"), dtype=o.dtype)
    Sr = torch.zeros(B, H, W, ps, dtype=D)
    if wrong == "reim":
        re_off, im_off = im_off, re_off
    for d in range(ndir):
        gi = 2 * ((g0 * ndir + d) if wrong == "dirhead" else (g0 + d * A))
        od, Sd = o[d * B:(d + 1) * B], S[d * B:(d + 1) * B]
        ref[..., re_off + gi:re_off + gi + 2], ref[..., im_off + gi:im_off + gi + 2] = od[..., :2], od[..., 2:]
        Sr[..., re_off + gi:re_off + gi + 2], Sr[..., im_off + gi:im_off + gi + 2] = Sd[..., :2], Sd[..., 2:]
    return ref, (Sr if k is None else k * EPS * Sr), ~torch.isnan(ref)


def convblk_tail(u, gate, sim, B, ndir, A, g0, cd=D, wrong=None):
    """(:355-356, :1495-1498) o = (u * gate + u) * sim, bn = dir*B + b; floats (o0, o1) to re_off + gi, (o2, o3) to im_off + gi of
    the pixel's record, gi = 2 (g0 + dir * A), re_off = 0, im_off = 4A, pix_stride = 8A.  One fmaf [1] and one product [2]: k = 2 on
    S = (|u| |gate| + |u|) |sim|."""
    uu, gg = u.to(cd), gate.to(cd)[:, None, None, :]
    ss = sim.to(cd).repeat(ndir, 1, 1, 1)
    fma = (uu.double() * gg.double() + (0.0 if wrong == "nogateplus" else uu.double())).to(cd)    # one rounding, as fmaf
    o = fma * ss
    S = (u.double().abs() * gate.double().abs()[:, None, None, :] + u.double().abs()) * ss.double().abs()
    return record(o, S, B, ndir, A, g0, 8 * A, 0, 4 * A, 2, wrong)


# ---- 5. fcvsr_convblk (convblk.hip) ---------------------------------------------------------------------------------------------------

CONVBLK_WRONG = ["clamp", "nozero", "droptile", "tilemean"]
CONVBLK_K = [1, 3, 5, 7, 9, 11]
# (H, Wf, B, slope): one pixel; smaller than the halo; one whole tile; partial tiles both ways; 1 x 3 and 3 x 2 tiles
CONVBLK_SHAPES = [(1, 1, 3, 0.25), (5, 3, 1, 0.0), (16, 16, 3, -0.1), (17, 15, 1, 0.25), (16, 33, 3, 0.0), (33, 17, 1, -0.1)]
CONVBLK_A = 3


def convblk_tag(K, H, W, B):
    return f"K{K} {H}x{W} B{B}"


def convblk_inputs(K, H, W, B, slope):
    g = gen(45, K, H, W, B)
    r = lambda *s: torch.randn(*s, generator=g)
    half = r(2, 4)                                           # hidden units in +- pairs: two of the four are live for every mean
    return dict(x=r(2 * B, H, W, 4), sim=r(B, H, W, 4), w1=r(4, 4, K, K) / (2.0 * K), w2=r(4, 4, K, K) / (2.0 * K),
                slope=torch.tensor([slope]), cw1=torch.cat([half, -half]), cw2=r(4, 4), g0=(K // 2) % CONVBLK_A)


def convblk_cannot_differ(wrong, K, H, W):
    """K = 1 has no halo: nothing is padded.  One tile exactly: its padded area is HW."""
    return (K == 1 and wrong in ("clamp", "nozero")) or (wrong == "tilemean" and H % 16 == 0 and W % 16 == 0)


def _conv(x, w, pad):
    return F.conv2d(x, w, padding=pad)


def convblk(p, B, cd=D, wrong=None):
    """One ConvBlk head (:344-357, :1494-1498): x (2B,H,W,4) NHWC, w1 / w2 (4,4,K,K) -> u = conv2(PReLU(conv1(x))) with zero padding
    of BOTH convolutions, gate = CALayer 4-4-4 on mean_HW(u), record of (u * gate + u) * sim as in convblk_tail.  Returns
    (u, u_bound), (rec, rec_scale, own).
    u, derived: each conv is a chain of n = 4 K^2 fmaf: tau(n) * S.  t = PReLU(conv1) has tau(n) * S_t + 2^-24 |t| (the slope product),
    carried through conv2 by |w2| and PReLU's Lipschitz constant max(1, |slope|); u adds tau(n) * (|t| conv |w2|).
    record, measured: scale = S_u (1 + S_gate) |sim|, S_u = S_t conv |w2| (>= |u|, not small where u cancels), S_gate the sigmoid rule
    on the mean of S_u."""
    x, w1, w2 = p["x"].to(cd).permute(0, 3, 1, 2), p["w1"].to(cd), p["w2"].to(cd)
    N, _, H, W = x.shape
    K = w1.shape[-1]
    P, n = K // 2, 4 * K * K
    s = float(p["slope"][0])
    act = lambda v: torch.where(v >= 0, v, v * s)
    if wrong == "clamp":                                     # WRONG: the intermediate continued by its border values
        u = _conv(F.pad(act(_conv(x, w1, P)), (P, P, P, P), mode="replicate"), w2, 0) if P else _conv(act(_conv(x, w1, P)), w2, P)
    elif wrong == "nozero":                                  # WRONG: the intermediate evaluated outside the image too
        u = _conv(act(_conv(x, w1, 2 * P)), w2, 0)
    else:
        u = _conv(act(_conv(x, w1, P)), w2, P)
    lip = max(1.0, abs(s))
    xa, w1a, w2a = x.double().abs(), p["w1"].double().abs(), p["w2"].double().abs()
    t64 = act(_conv(x.double(), p["w1"].double(), P))
    S_t = _conv(xa, w1a, P) * lip
    S_u = _conv(S_t, w2a, P)
    u_bound = tau(n) * _conv(t64.abs(), w2a, P) + (tau(n) + EPS) * S_u
    tiles = (-(-H // 16)) * (-(-W // 16))
    usum = u.sum(dim=(2, 3))
    if wrong == "droptile":                                  # WRONG: the last 16 x 16 tile's partial sum left out
        usum = usum - u[:, :, (H - 1) // 16 * 16:, (W - 1) // 16 * 16:].sum(dim=(2, 3))
    inv = f32(1.0 / (256 * tiles)) if wrong == "tilemean" else f32(1.0 / (H * W))
    gate, _ = ca_gate(usum, inv, p["cw1"], p["cw2"], cd)
    gd = gate.double()
    pre = (u.double().sum(dim=(2, 3)) * inv) @ p["cw1"].double().t()
    S_s = (((S_u.sum(dim=(2, 3)) * inv) @ p["cw1"].double().abs().t()) * (pre > 0)) @ p["cw2"].double().abs().t()
    S_gate = gd * (1.0 + (1.0 - gd) * S_s)
    un = u.permute(0, 2, 3, 1)
    ss = p["sim"].to(cd).repeat(2, 1, 1, 1)
    o = (un * gate[:, None, None, :] + un) * ss
    S_o = S_u.permute(0, 2, 3, 1) * (1.0 + S_gate[:, None, None, :]) * ss.double().abs()
    A = CONVBLK_A
    return (un, u_bound.permute(0, 2, 3, 1)), record(o, S_o, B, 2, A, p["g0"], 8 * A, 0, 4 * A, None)


def convblk_rejection(K, H, W, B, slope):
    p = convblk_inputs(K, H, W, B, slope)
    _, (ref, scale, own) = convblk(p, B)
    fig = INF
    for w in CONVBLK_WRONG:
        if not convblk_cannot_differ(w, K, H, W):
            fig = min(fig, _ratio((convblk(p, B, wrong=w)[1][0] - ref)[own], scale[own]))
    return fig


# ---- 6. DivEnh (mffr.hip) -------------------------------------------------------------------------------------------------------------

DIVENH_WRONG = ["no02a", "no02so", "meannohw", "sfearly", "lastpix"]
DIVENH_Q = 3
# (C, H, W, B, offset): fcvsr_divenh_apply_next takes its 16-byte path at C = 64 and 32, the generic one at C = 24 (256 % 6 != 0) and
# at C = 64 with the band pointers 4 bytes off a 16-byte boundary (offset = 1 float)
DIVENH_CASES = [(64, 1, 1, 1, 0), (64, 15, 17, 3, 0), (64, 16, 16, 1, 0), (64, 1, 257, 3, 0), (64, 20, 24, 1, 0), (32, 1, 257, 3, 0),
                (32, 20, 24, 1, 0), (24, 1, 257, 3, 0), (24, 15, 17, 1, 0), (24, 16, 16, 1, 0), (24, 1, 1, 3, 0), (64, 1, 257, 1, 1),
                (64, 20, 24, 3, 1)]


def divenh_inputs(Cn, H, W, B):
    g = gen(46, Cn, H, W, B)
    Q = DIVENH_Q
    f = [torch.randn(B, H, W, Cn, generator=g) * (1.0 if i == 0 else 0.5) + (0.3 if i == 0 else 0.0) for i in range(Q)]
    return dict(f=f, a=[torch.randn(Cn, generator=g) for _ in range(Q)], b=[torch.randn(Cn, generator=g) for _ in range(Q)],
                g1=[torch.rand(B, Cn, generator=g) for _ in range(Q)], g2=[torch.rand(B, Cn, generator=g) for _ in range(Q)],
                mean_sum=f[0].sum(dim=(1, 2)), inv_hw=1.0 / (H * W))


def _psum(v, S, k, drop):
    """Sum over the pixels of (B,H,W,C): tau(HW) * S for the order of the sum, k * 2^-24 * S for the k roundings inside a term."""
    B, H, W, Cn = v.shape
    v, S = v.reshape(B, H * W, Cn), S.reshape(B, H * W, Cn)
    if drop:                                                 # WRONG: the last pixel of the last block left out
        v = v[:, :-1]
    return v.sum(1), (tau(H * W) + k * EPS) * S.sum(1)


def divenh_chain(p, cd=D, wrong=None, carry=F32, given=None):
    """The Q-band DivEnh chain (:2104-2133) with the gates g1, g2 given.  Band i: aa = 0.2 a, first band t = f - mean_sum * inv_hw,
    later t = f - s_f + 0.2 s_o;  e1 = aa t f + b f, e2 = aa s_o f + b f (0 in the first band);  o = e1 g1 + e2 g2;  s_f += f, s_o += o.
    Every kernel call reads the running sums from memory: the reference carries them in `carry` (f32, as stored; None: unrounded, for
    the pin to the oracle), so that each call is compared on inputs it was given; `given` (the states another evaluation returned)
    replaces the chain's own stored states: the f32 evaluation and the kernels start every band from the reference's.  Returns {name: (ref, bound)} and the carried states:
      e{i}      (2,B,C) sums of e1, e2 of band i from the stored state     [fcvsr_divenh mode 0]
      sf{i}, so{i}  the running sums after band i                           [mode 1 and fcvsr_divenh_apply_next]
      nx{i}     (2,B,C) what apply_next(band i) adds: the sums of e1, e2 of band i+1 from the NEW state, or (sum of s_o, 0) after
                the last band.
    Roundings (no contraction): first band mean [1], t [2], aa [1], aa t [3], (aa t) f [4], + b f [5]: e1 k = 5; later t = (f - s_f) +
    0.2 s_o [2] and again k = 5; e2 = (aa s_o) f + b f: k = 4; o = e1 g1 [6] (+ e2 g2 [7]); s_o + o: k = 8 (6 in the first band, a
    plain store), s_f + f: k = 1 (0).  nx carries the new state's roundings: k = 8 + 5."""
    Q = len(p["f"])
    fa = lambda t: t.double().abs()
    inv = f32(p["inv_hw"])
    c02 = f32(0.2)
    res, states = {}, []
    sf = so = None
    for i in range(Q):
        first = i == 0
        f = p["f"][i].to(cd)
        a, b = p["a"][i].to(cd), p["b"][i].to(cd)
        g1, g2 = p["g1"][i].to(cd)[:, None, None, :], p["g2"][i].to(cd)[:, None, None, :]

        def exprs(f, a, b, sf, so, S_sf, S_so, first):
            aa = a if wrong == "no02a" else c02 * a
            aaS = fa(aa)
            if first:
                mean = p["mean_sum"].to(cd)[:, None, None, :] * (1.0 if wrong == "meannohw" else inv)
                t, S_t = f - mean, fa(f) + fa(mean)
                e1, e2 = aa * t * f + b * f, torch.zeros_like(f)
                S1, S2 = aaS * S_t * fa(f) + fa(b) * fa(f), torch.zeros_like(fa(f))
            else:
                sfe = sf + f if wrong == "sfearly" else sf
                t = f - sfe + (0.0 if wrong == "no02so" else c02 * so)
                S_t = fa(f) + S_sf + c02 * S_so
                e1, e2 = aa * t * f + b * f, aa * so * f + b * f
                S1, S2 = aaS * S_t * fa(f) + fa(b) * fa(f), aaS * S_so * fa(f) + fa(b) * fa(f)
            return e1, e2, S1, S2

        e1, e2, S1, S2 = exprs(f, a, b, sf, so, None if first else fa(sf), None if first else fa(so), first)
        drop = wrong == "lastpix"
        s1, b1 = _psum(e1, S1, 5, drop)
        s2, b2 = _psum(e2, S2, 4, drop)
        res[f"e{i}"] = (torch.stack([s1, s2]), torch.stack([b1, b2]))
        if first:
            o, S_o = e1 * g1, S1 * fa(g1)
            nsf, nso, S_nsf, S_nso, k_f, k_o = f, o, fa(f), S_o, 0, 6
        else:
            o, S_o = e1 * g1 + e2 * g2, S1 * fa(g1) + S2 * fa(g2)
            nsf, nso, S_nsf, S_nso, k_f, k_o = sf + f, so + o, fa(sf) + fa(f), fa(so) + S_o, 1, 8
        res[f"sf{i}"], res[f"so{i}"] = (nsf, k_f * EPS * S_nsf), (nso, k_o * EPS * S_nso)
        if i + 1 < Q:
            n1, n2, T1, T2 = exprs(p["f"][i + 1].to(cd), p["a"][i + 1].to(cd), p["b"][i + 1].to(cd), nsf, nso, S_nsf, S_nso, False)
            s1, b1 = _psum(n1, T1, k_o + 5, drop)
            s2, b2 = _psum(n2, T2, k_o + 4, drop)
        else:
            s1, b1 = _psum(nso, S_nso, k_o, drop)
            s2, b2 = torch.zeros_like(s1), torch.zeros_like(b1)
        res[f"nx{i}"] = (torch.stack([s1, s2]), torch.stack([b1, b2]))
        sf, so = (nsf, nso) if carry is None else (nsf.to(carry).to(cd), nso.to(carry).to(cd))
        states.append((sf, so))
        if given is not None:
            sf, so = given[i][0].to(cd), given[i][1].to(cd)
    return res, states


DIVENH_GROUPS = {"mode0": ("e",), "mode1": ("so",), "apply_next": ("so", "nx")}   # the outputs an entry point is compared on


def divenh_cannot_differ(wrong, group, HW):
    """meannohw: 1/HW = 1 for a single pixel.  lastpix touches only sums, which mode 1 has none of.  (no02so and sfearly change t of
    the later bands only, meannohw the first band's: every group holds outputs of all three bands.)"""
    return (wrong == "meannohw" and HW == 1) or (wrong == "lastpix" and group == "mode1")


# ---- 7. ContextBlock pooling (scnet.hip) ----------------------------------------------------------------------------------------------

GC_WRONG = ["nomax", "blockmax", "padzero", "droptile", "lreluside"]
# fcvsr_gc_context: (B, C, H, W, stress); blocks of 256 pixels.  257 x 256 gives nblk = 257, above the 256 threads of stage 2
GC_CASES = [(1, 64, 1, 1, None), (3, 64, 15, 17, None), (1, 64, 16, 16, None), (3, 64, 1, 257, None), (1, 8, 257, 256, None),
            (3, 32, 1, 257, None), (1, 8, 1, 257, None), (1, 64, 20, 30, "span"), (1, 64, 20, 30, "last"), (1, 64, 20, 30, "dom"),
            (1, 32, 3, 100, "last")]
# the tile entry (4 x 32 tiles, C = 64, 16-bit r): name -> [(B, H, W, stress)] per level
GC_TILE_SETS = {"small": [(2, 1, 1, None), (2, 4, 32, None), (2, 5, 33, None)],
                "mixedB": [(2, 3, 31, None), (1, 36, 929, None), (3, 5, 33, None)],
                "stress": [(2, 9, 70, "span"), (2, 5, 33, "last"), (2, 3, 31, "dom")]}


def gc_tag(B, Cn, H, W, stress):
    return f"C{Cn} {B}x{H}x{W}" + (f" {stress}" if stress else "")


def block_partition(H, W):
    """fcvsr_gc_context: block id of every pixel and the number of padded slots per block."""
    HW = H * W
    bid = torch.arange(HW) // 256
    return bid, 256 - torch.bincount(bid)


def tile_partition(H, W):
    """The 4 x 32 tiles of fcvsr_gc_partial_levels / the conv epilogue."""
    tx = -(-W // 32)
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    bid = ((y // 4) * tx + x // 32).reshape(-1)
    return bid, 128 - torch.bincount(bid)


def gc_inputs(B, Cn, H, W, stress, part, dt=F32, shared=None):
    """r (B,H,W,C) stored in dt, wmask, w1, w2.  Stress (mirrors test_rcb_tail_softmax_pool_stress): the logits get an offset along
    wmask - `span`: +92 ... +12 falling over the blocks, whole blocks scale to (nearly) nothing and exp without the maximum overflows
    f32; `last`: -30 everywhere but at the last live pixel of the partial last block; `dom`: -60 everywhere but at pixel 1.
    `shared`: another level's inputs, whose wmask, w1, w2 this one takes (BlockRCB's levels share them)."""
    g = gen(47, B, Cn, H, W, {None: 0, "span": 1, "last": 2, "dom": 3}[stress], {F32: 0, BF16: 1, F16: 2}[dt])
    wm = torch.randn(Cn, generator=g) * 0.3
    w1, w2 = torch.randn(Cn, Cn, generator=g) / math.sqrt(Cn), torch.randn(Cn, Cn, generator=g) / math.sqrt(Cn)
    if shared is not None:
        wm, w1, w2 = shared["wmask"], shared["w1"], shared["w2"]
    r = torch.randn(B, H * W, Cn, generator=g)
    bid, _ = part(H, W)
    nb = int(bid.max()) + 1
    off = torch.zeros(H * W)
    if stress == "span":
        off = 92.0 - 80.0 * bid.double() / max(1, nb - 1)
    elif stress == "last":
        off = torch.full((H * W,), -30.0)
        off[-1] = 0.0
    elif stress == "dom":
        off = torch.full((H * W,), -60.0)
        off[1] = 0.0
    r = r + off.float()[None, :, None] * (wm / (wm * wm).sum())[None, None, :]
    return dict(r=r.reshape(B, H, W, Cn).to(dt), wmask=wm, w1=w1, w2=w2)


def gc_tile_inputs(name, dt):
    """The levels of GC_TILE_SETS[name]: C = 64, one wmask / w1 / w2 for all of them."""
    ps = []
    for B, H, W, stress in GC_TILE_SETS[name]:
        ps.append(gc_inputs(B, 64, H, W, stress, tile_partition, dt, shared=ps[0] if ps else None))
    return ps


def gc_cannot_differ(wrong, stress, bid, pad):
    """nomax is the same function until exp overflows (the span inputs); blockmax needs two blocks; padzero a padded slot, and logits
    that do not dwarf 0 (span: the maximum is +92, a slot weighs e^-92); the dropped tile is the first one, which weighs e^-30 of
    the last pixel in `last` (where it is the only tile it is everything: the result is non-finite, which counts)."""
    if wrong == "nomax":
        return stress != "span"
    if wrong == "blockmax":
        return int(bid.max()) == 0
    if wrong == "padzero":
        return int(pad.sum()) == 0 or stress == "span"
    if wrong == "droptile":
        return stress == "last" and int(bid.max()) > 0
    return False


def gc_context(p, part, cd=D, wrong=None):
    """ContextBlock (:657-701) on the STORED r: logits l_p = <r_p, wmask>, m = softmax over the pixels, ctx = sum_p m_p r_p,
    add = W2 lrelu_0.2(W1 ctx) -> (add (B,C), scale).  `part` (block_partition / tile_partition) only matters to the wrong variants."""
    r = p["r"].to(cd)
    B, H, W, Cn = r.shape
    rm = r.reshape(B, H * W, Cn)
    wm, W1, W2 = p["wmask"].to(cd), p["w1"].to(cd), p["w2"].to(cd)
    bid, pad = part(H, W)
    nb = int(bid.max()) + 1
    logit = rm @ wm
    if wrong == "droptile":                                  # WRONG: the first block / tile never arrives
        live = bid != 0
        rm, logit, bid, pad, nb = rm[:, live], logit[:, live], bid[live] - 1, pad[1:], nb - 1
    if wrong == "padzero":                                   # WRONG: the padded slots of partial blocks count as pixels r = 0, logit 0
        npad = int(pad.sum())
        rm, logit = torch.cat([rm, torch.zeros(B, npad, Cn, dtype=cd)], 1), torch.cat([logit, torch.zeros(B, npad, dtype=cd)], 1)
    if rm.shape[1] == 0:
        ctx = torch.full((B, Cn), float("nan"), dtype=cd)
    else:
        if wrong == "nomax":                                 # WRONG: exp of the raw logits
            e = torch.exp(logit)
        elif wrong == "blockmax":                            # WRONG: every block keeps its own maximum
            bm = torch.stack([logit[:, bid == k].max(1).values for k in range(nb)], 1)
            e = torch.exp(logit - bm[:, bid])
        else:
            e = torch.exp(logit - logit.max(1, keepdim=True).values)
        m = e / e.sum(1, keepdim=True)
        ctx = (m[:, :, None] * rm).sum(1)
    t = ctx @ W1.t()
    s = f32(0.2)
    a = torch.where(t >= 0, s * t, t) if wrong == "lreluside" else torch.where(t >= 0, t, s * t)
    add = a @ W2.t()
    # scale (train_block_refs' rules), always from the unmodified f64 evaluation
    r64 = p["r"].double().reshape(B, H * W, Cn)
    l64 = r64 @ p["wmask"].double()
    L = r64.abs() @ p["wmask"].double().abs()
    m64 = torch.softmax(l64, 1)
    Sm = m64 * (1.0 + L + (m64 * L).sum(1, keepdim=True))
    S_ctx = (Sm[:, :, None] * r64.abs()).sum(1)
    t64 = (m64[:, :, None] * r64).sum(1) @ p["w1"].double().t()
    S_a = (S_ctx @ p["w1"].double().abs().t()) * torch.where(t64 >= 0, 1.0, s)
    return add, S_a @ p["w2"].double().abs().t()


def gc_rejection(p, part, stress):
    ref, scale = gc_context(p, part)
    bid, pad = part(p["r"].shape[1], p["r"].shape[2])
    fig = INF
    for w in GC_WRONG:
        if not gc_cannot_differ(w, stress, bid, pad):
            cd = F32 if w == "nomax" else D
            fig = min(fig, _ratio(gc_context(p, part, cd, w)[0].double() - ref, scale))
    return fig


# ---- the stage-2 shared-memory limit ---------------------------------------------------------------------------------------------------

STAGE2_DYNAMIC_LIMIT = 60 * 1024                             # the three entry points admit (2C + nparts) * 4 <= 60 KiB
STAGE2_STATIC = {"fcvsr_gc_finish_levels": 5 * 1024, "fcvsr_gc_finish": 1024}    # red[256] (+ red4_s[1024]) floats


def stage2_max_nparts(Cn):
    return STAGE2_DYNAMIC_LIMIT // 4 - 2 * Cn


def stage2_inputs(Cn, nparts, B=1):
    """Synthetic partials of the stage-1 layout [B][nparts][C + 2]: per tile the weighted channel sums (sum_p e_p r_pc), the tile
    maximum m and sum_p e_p - here each tile is ONE pixel with logit m (e = 1, sums = r), so the reference is gc_context on those
    pixels with the given logits."""
    g = gen(48, Cn, nparts, B)
    r = torch.randn(B, nparts, Cn, generator=g)
    logit = torch.randn(B, nparts, generator=g) * 2.0
    parts = torch.cat([r, logit[:, :, None], torch.ones(B, nparts, 1)], 2).contiguous()
    return dict(parts=parts, r=r, logit=logit, w1=torch.randn(Cn, Cn, generator=g) / math.sqrt(Cn),
                w2=torch.randn(Cn, Cn, generator=g) / math.sqrt(Cn))


def stage2_reference(p, cd=D, drop_last=False):
    """add (B,C) and its scale for stage2_inputs: the logits are given (exact inputs, L = 0 in the softmax rule)."""
    r, l = p["r"].to(cd), p["logit"].to(cd)
    if drop_last:                                            # WRONG: the last partial never read
        r, l = r[:, :-1], l[:, :-1]
    m = torch.softmax(l, 1)
    t = (m[:, :, None] * r).sum(1) @ p["w1"].to(cd).t()
    s = f32(0.2)
    add = torch.where(t >= 0, t, s * t) @ p["w2"].to(cd).t()
    m64 = torch.softmax(p["logit"].double(), 1)
    S_ctx = (m64[:, :, None] * p["r"].double().abs()).sum(1)
    t64 = (m64[:, :, None] * p["r"].double()).sum(1) @ p["w1"].double().t()
    S_a = (S_ctx @ p["w1"].double().abs().t()) * torch.where(t64 >= 0, 1.0, s)
    return add, S_a @ p["w2"].double().abs().t()
