"""Float64 CPU references of the inference convolutions (fcvsr_conv2d_mfma's six kernels, fcvsr_conv2d, fcvsr_conv2d_f32mfma,
fcvsr_conv_last) and the list of cases the GPU test runs; nothing here calls fcvsr_amd.hip.  tests/test_infer_conv_refs_cpu.py pins
the reference to plain torch, shows that the bounds accept a correct f32 evaluation and reject wrong kernels at every case, and
checks the dispatch the cases declare; tests/test_infer_conv_gpu.py asserts |got - ref| <= bound for every element.

A *problem* is a dict in the format of scripts/record_conv_plan_table.py (ksize, stride, cout, mma, act, slope, slope_t, bias,
res_scale, pixel_shuffle, gc, groups of srcs / res / dst with shape, dtype, strides, offset), plus optional keys of this module:
slope_v (the PReLU scalar, default 0.25), seed (another seeded input set, where the first one has no element that tells a wrong
variant apart), values ("k255": sources are k / 255 of a byte k), zero_tail (the last 4 channels of the last
source are zero padding), gc_stress (the sources are freq_kernel_refs.gc_inputs' stress set and the weights the identity tap, so that
the layer output is that set exactly).  mma = None is the exact-f32 family.

conv_ref(p, inp) -> per group {"ref", "bound"} in the destination's (b, y, x, c) layout (pixel-shuffled where the problem is):
  operands   an f32 source is rounded to the MFMA dtype (nearest even, as staging does); a 16-bit source is taken as stored; weights are
             rounded to the MFMA dtype and passed in NATURAL row order (the sub-pixel-major packing is the kernel's business);
             bias, slope and res_scale are f32 values; residuals (f32 or 16-bit) are taken as stored.  mma = None rounds nothing.
  operation  sources concatenated in order; convolution of stride 1 or 2 with zero padding k // 2 (stride 2: the even output pixels);
             + bias; activation (none / ReLU / leaky(slope) / PReLU(slope tensor)); + rs[q] * res[q]; pixel shuffle.
  bound      L * tau(n) * S + u * |ref|:  tau from tests/tolerance.py, n = k * k * cin_total, S the same operation on absolute values
             (|x| * |w| + |bias| + sum |rs| |res|), L = max(1, |slope|) (the activation is L-Lipschitz, so a sign flip of a near-zero
             pre-activation stays inside), u one unit in the last place of the destination (2^-7 bf16, 2^-10 f16, 0 f32).  `ref` is
             not rounded to the destination.

ContextBlock fusion (gc): the conv epilogue pools the UNROUNDED f32 value, also where the store is 16-bit.  The partial of a 4 x 32
tile T is (acc_c, m, sum) with any maximum m the kernel likes; two quantities do not depend on that choice and are what is compared:
    lse_T = log sum_p exp(l_p) = m + log(sum),        mu_Tc = sum_p softmax(l)_p y_pc = acc_c / sum,        l_p = <y_p, wmask>.
With E_pc = L * tau(n) * S_pc (the element bound WITHOUT the store term u |ref|: nothing is stored on the way to the partial - with
the store term the bound could not tell the pooling of the rounded store from the pooling of the f32 value, which is the difference
this reference exists to see):
    delta_p  = sum_c |wm_c| E_pc + tau(C) sum_c |wm_c| |y_pc|          (logit: the inputs' error, then C products summed in f32)
    D_T      = max_p delta_p
    |d lse_T| <= D_T + 2^-16
    |d mu_Tc| <= max_p E_pc + (e^(2 D_T) - 1) max_p |y_pc - mu_Tc| + tau(128) sum_p w_p |y_pc|
(the logarithm and the sum of <= 128 positive terms are well conditioned: 2^-16 covers them; the rounding of m + log(sum) at a large
lse is inside D_T, whose second term is tau(C) times at least |l_p|).  The f32 evaluation of the CPU test stays inside both as stated.
A softmax weight moves by at most a factor e^(+-2 D) when every logit moves by at most D, and sum_p dw_p = 0, so the weights' error
moves mu by at most (e^(2D) - 1) times the spread of y around mu; the last term is the f32 summation of <= 128 weighted values.
The image-level vector `add` = W2 lrelu_0.2(W1 ctx) is freq_kernel_refs.gc_context on that y.  Its bound carries the same three terms
for ctx, with the softmax-weighted means in place of the maxima (d ctx_c = sum_p w_p dy_pc + sum_p dw_p (y_pc - ctx_c), |dw_p| <=
w_p (e^(2D) - 1): sum_p w_p E_pc + (e^(2D) - 1) sum_p w_p |y_pc - ctx_c| + tau(HW) sum_p w_p |y_pc|, D over the image), plus 2 tau(C) of
the two small products' own condition, all through |W1| and |W2| (lrelu is 1-Lipschitz).  It is a worst-case bound and a wide one:
D sums E = tau(n) S over the channels as if every element erred by its bound in the direction of wmask, and |W2| |W1| has none of
the cancellation of W2 W1, so at a level of several tiles it admits 10 to 25 % of |add| (a few % at the stress set, 0.2 % at a
one-pixel level).  That still rejects the finish kernel's gross errors - the slope on the wrong side at every level of every case,
a partial that never arrives wherever a tile is more than a twelfth of the image (the CPU test shows both) - and the sharp check
of the fused epilogue is lse_T / mu_T per tile; fcvsr_gc_finish_levels itself is pinned by tests/test_freq_kernels_gpu.py.

conv_last_ref: fcvsr_conv_last through infer_kernel_refs.tail_last, bound tau(9 * 64 + 2) * S (576 products, bias, base; f32 store).

`wrong` selects a deliberately WRONG variant (WRONG lists them); only the CPU test passes it.  `cd` is the dtype the arithmetic runs
in: float64, or float32 for "a correct f32 evaluation stays inside the bound"."""
import json
import math
import os
import zlib

import torch
import torch.nn.functional as F

from freq_kernel_refs import gc_context, gc_inputs, tile_partition
from infer_kernel_refs import BF16, D, F16, F32, f32, tail_last
from tolerance import tau

DT = {"f32": F32, "bf16": BF16, "f16": F16, None: None}
ULP = {F32: 0.0, BF16: 2.0 ** -7, F16: 2.0 ** -10}
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")
LEAN = {"unset": 1, "0": 0}
RES = {"unset": 2, "0": 0, "1": 1}
WRONG = ["clamp", "drop4", "srcorder", "noround", "otherdt", "odd", "pstranspose", "actafter", "nors", "biaslast", "preluside",
         "gcrounded", "gc8x32"]


# ---- problems ---------------------------------------------------------------------------------------------------------------------------

def T(shape, dtype, strides=None, offset=0):
    """One (b, y, x, c) tensor: dense NHWC unless `strides` (elements) says otherwise, `offset` elements into its buffer."""
    b, y, x, c = shape
    return dict(shape=list(shape), dtype=dtype, strides=list(strides or (y * x * c, x * c, c, 1)), offset=offset, align=0)


def nchw(shape, dtype, offset=0):
    b, y, x, c = shape
    return T(shape, dtype, strides=(c * y * x, x, 1, y * x), offset=offset)


def problem(name, k, cins, cout, levels, B, mma, dst, *, src=None, nres=0, res=None, act=0, slope=0.0, slope_v=None, bias=True,
            rs=(1.0, -0.5), ps=False, stride=1, gc=False, dst_layout="nhwc", src_layout="nhwc", **extra):
    """One problem: a source per entry of `cins` and per level (H, W), residuals shaped like the (pre-shuffle) output."""
    groups = []
    for (H, W) in levels:
        ho, wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
        oshape = (B, 2 * ho, 2 * wo, cout // 4) if ps else (B, ho, wo, cout)
        sdt = src or (mma if all(c % 8 == 0 for c in cins) and mma else "f32")
        mk = nchw if src_layout == "nchw" else T
        groups.append(dict(srcs=[mk((B, H, W, c), sdt) for c in cins],
                           res=[T((B, ho, wo, cout), res or mma or "f32") for _ in range(nres)],
                           dst=(nchw if dst_layout == "nchw" else T)(oshape, dst)))
    p = dict(name=name, ksize=k, stride=stride, cout=cout, mma=mma, act=act, slope=slope, slope_t=act == 3, bias=bias,
             res_scale=list(rs[:nres]), pixel_shuffle=ps, gc=gc, groups=groups)
    if slope_v is not None:
        p["slope_v"] = slope_v
    p.update(extra)
    return p


def cin_total(p):
    return sum(s["shape"][3] for s in p["groups"][0]["srcs"])


def make_inputs(p):
    """Seeded CPU operands of a problem: w (cout, cin, k, k) f32 in natural order, bias, slope_t, per group the stored values of every
    source and residual as (b, y, x, c) tensors of their dtype; for gc also wmask, w1, w2."""
    g = torch.Generator().manual_seed((zlib.crc32(p["name"].encode()) + p.get("seed", 0)) & 0x7FFFFFFF)
    k, cout, cin = p["ksize"], p["cout"], cin_total(p)
    out = dict(w=torch.randn(cout, cin, k, k, generator=g) / (k * math.sqrt(cin)),
               bias=torch.randn(cout, generator=g) * 0.5 if p["bias"] else None,
               slope_t=torch.tensor([float(p.get("slope_v", 0.25))]) if p["slope_t"] else None, groups=[])
    if p["gc"]:
        out.update(wmask=torch.randn(cout, generator=g) * 0.3, w1=torch.randn(cout, cout, generator=g) / math.sqrt(cout),
                   w2=torch.randn(cout, cout, generator=g) / math.sqrt(cout))
    shared = None
    for gr in p["groups"]:
        srcs = []
        for s in gr["srcs"]:
            if p.get("values") == "k255":
                v = torch.randint(0, 256, s["shape"], generator=g).float() / 255
            else:
                v = torch.randn(s["shape"], generator=g)
            srcs.append(v.to(DT[s["dtype"]]))
        if p.get("gc_stress"):
            B, H, W, c = gr["srcs"][0]["shape"]
            shared = gc_inputs(B, c, H, W, p["gc_stress"], tile_partition, DT[gr["srcs"][0]["dtype"]], shared=shared)
            srcs = [shared["r"]]
            out.update(wmask=shared["wmask"], w1=shared["w1"], w2=shared["w2"], bias=None)
            out["w"] = torch.zeros(cout, cin, k, k)
            out["w"][:, :, k // 2, k // 2] = torch.eye(cout, cin)
        if p.get("zero_tail"):
            srcs[-1][..., -4:] = 0
        out["groups"].append(dict(srcs=srcs, res=[torch.randn(r["shape"], generator=g).to(DT[r["dtype"]]) for r in gr["res"]]))
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def _rnd(t, dt, cd):
    return t.to(cd) if dt is None else t.to(dt).to(cd)


def neg_slope(p, inp):
    """(ns, L): the factor of the negative side as the f32 the kernel uses, and the activation's Lipschitz constant."""
    act = p["act"]
    ns = {0: 1.0, 1: 0.0, 2: f32(p["slope"]), 3: float(inp["slope_t"][0]) if inp["slope_t"] is not None else 0.0}[act]
    return ns, max(1.0, abs(ns))


def cannot_differ(p, wrong):
    """The wrong variants that are the same function at this problem."""
    k, cout, nres = p["ksize"], p["cout"], len(p["res_scale"])
    ns = {0: 1.0, 1: 0.0, 2: f32(p["slope"]), 3: float(p.get("slope_v", 0.25))}[p["act"]]
    gr = p["groups"]
    dst16 = gr[0]["dst"]["dtype"] != "f32"
    # an f16 store moves a value by 2^-11 |y|: averaged over a tile's pixels that is below E = tau(n) S; only a one-pixel tile shows it
    one_pixel_tile = any(g["srcs"][0]["shape"][1] % 4 == 1 and g["srcs"][0]["shape"][2] % 32 == 1 for g in gr)
    return {"clamp": k == 1 or bool(p.get("gc_stress")),         # the stress set's weights are the centre tap alone
            "drop4": bool(p.get("zero_tail")) or bool(p.get("gc_stress")),
            "srcorder": len(gr[0]["srcs"]) == 1,
            "noround": p["mma"] is None or bool(p.get("gc_stress")),
            "otherdt": p["mma"] is None or bool(p.get("gc_stress")),
            "odd": p["stride"] == 1,
            "pstranspose": not p["pixel_shuffle"],
            "actafter": ns == 1.0 or nres == 0,
            "nors": nres == 0,
            "biaslast": not p["bias"] or cout % 32 == 0 or bool(p.get("gc_stress")),
            "preluside": ns == 1.0,
            "gcrounded": not (p["gc"] and dst16) or bool(p.get("gc_stress")) or     # (the stress set is exact in 16 bits)
                         (gr[0]["dst"]["dtype"] == "f16" and not one_pixel_tile),
            "gc8x32": not p["gc"] or all(g["srcs"][0]["shape"][1] <= 4 for g in gr)}[wrong]


def conv_ref(p, inp, cd=D, wrong=None, rounding=True):
    """Module docstring.  Per group a dict: ref, bound, and E (the bound without the store term) in the destination's layout."""
    dt = DT[p["mma"]] if rounding and wrong != "noround" else None
    if wrong == "otherdt" and dt is not None:
        dt = F16 if dt == BF16 else BF16
    k, stride, cout = p["ksize"], p["stride"], p["cout"]
    w = _rnd(inp["w"], dt, cd)
    ns, L = neg_slope(p, inp)
    bias = torch.zeros(cout, dtype=cd) if inp["bias"] is None else inp["bias"].to(cd).clone()
    if wrong == "biaslast":
        bias[cout // 32 * 32:] = 0
    n = k * k * cin_total(p)
    outs = []
    for gs, gi in zip(p["groups"], inp["groups"]):
        srcs = [s.to(cd) if s.dtype != F32 else _rnd(s, dt, cd) for s in gi["srcs"]]
        if wrong == "srcorder":
            srcs = srcs[::-1]
        x = torch.cat(srcs, 3).permute(0, 3, 1, 2)
        if wrong == "drop4":                                 # WRONG: the last 4 input channels never arrive
            x = x.clone()
            x[:, -4:] = 0

        def conv(xx, wv):
            if wrong == "clamp" and k > 1:
                return F.conv2d(F.pad(xx, (k // 2,) * 4, mode="replicate"), wv, stride=stride)
            if wrong == "odd" and stride == 2:
                full = F.pad(F.conv2d(xx, wv, padding=k // 2), (0, 1, 0, 1))
                return full[:, :, 1::2, 1::2]
            return F.conv2d(xx, wv, stride=stride, padding=k // 2)

        y = conv(x, w) + bias.view(1, -1, 1, 1)
        S = conv(x.abs(), w.abs()).double() + bias.abs().double().view(1, -1, 1, 1)

        def act(v):
            if wrong == "preluside":
                return torch.where(v >= 0, ns * v, v)
            return torch.where(v >= 0, v, ns * v)

        if wrong != "actafter":
            y = act(y)
        for q, r in enumerate(gi["res"]):
            rs = f32(p["res_scale"][q])
            rr = r.to(cd).permute(0, 3, 1, 2)
            if wrong != "nors":
                y = y + rs * rr
            S = S + abs(rs) * rr.abs().double()
        if wrong == "actafter":
            y = act(y)
        if p["pixel_shuffle"]:
            if wrong == "pstranspose":                       # WRONG: channel 4c + 2i + j lands at (2h + j, 2w + i)
                perm = torch.tensor([4 * c + 2 * j + i for c in range(cout // 4) for i in range(2) for j in range(2)])
                y = y[:, perm]
            y = F.pixel_shuffle(y, 2)
            S = F.pixel_shuffle(S, 2)
        y, S = y.permute(0, 2, 3, 1), S.permute(0, 2, 3, 1)
        E = L * tau(n) * S
        outs.append(dict(ref=y, E=E, bound=E + ULP[DT[gs["dst"]["dtype"]]] * y.double().abs()))
    return outs


def _tiles(H, W, th):
    tx = -(-W // 32)
    return [(ty * tx + txi, slice(ty * th, min(H, ty * th + th)), slice(txi * 32, min(W, txi * 32 + 32)))
            for ty in range(-(-H // th)) for txi in range(tx)]


def gc_tiles(y, E, wmask, cd=D, th=4):
    """Per 4 x 32 tile of y (B,H,W,C): lse (B, nt), mu (B, nt, C) and their bounds (module docstring).  th = 8 is the WRONG 8 x 32
    partition, reported on the 4 x 32 tiles it covers."""
    B, H, W, Cn = y.shape
    yc, wm = y.to(cd), wmask.to(cd)
    y64, wa = y.double(), wmask.double().abs()
    delta = (E * wa).sum(3) + tau(Cn) * (y64.abs() * wa).sum(3)
    nt = len(_tiles(H, W, 4))
    lse, mu = torch.zeros(B, nt, dtype=cd), torch.zeros(B, nt, Cn, dtype=cd)
    b_lse, b_mu = torch.zeros(B, nt, dtype=D), torch.zeros(B, nt, Cn, dtype=D)
    tx = -(-W // 32)
    for t, ys, xs in _tiles(H, W, th):
        v = yc[:, ys, xs].reshape(B, -1, Cn)
        l = v @ wm
        m = l.max(1, keepdim=True).values
        e = torch.exp(l - m)
        s = e.sum(1)
        ls, mm = m[:, 0] + torch.log(s), (e[:, :, None] * v).sum(1) / s[:, None]
        v64 = y64[:, ys, xs].reshape(B, -1, Cn)
        w64 = torch.softmax(v64 @ wmask.double(), 1)
        mu64 = (w64[:, :, None] * v64).sum(1)
        Dt = delta[:, ys, xs].reshape(B, -1).max(1).values
        bl = Dt + 2.0 ** -16
        bm = (E[:, ys, xs].reshape(B, -1, Cn).max(1).values + torch.expm1(2 * Dt)[:, None] * (v64 - mu64[:, None]).abs().max(1).values
              + tau(128) * (w64[:, :, None] * v64.abs()).sum(1))
        if th == 4:
            ids = [t]
        else:                                                # the 8-row tile (ty, txi) covers the 4-row tiles (2 ty, txi), (2 ty + 1, txi)
            ty, txi = divmod(t, tx)
            ids = [i for i in ((2 * ty) * tx + txi, (2 * ty + 1) * tx + txi) if i < nt]
        for i in ids:
            lse[:, i], mu[:, i], b_lse[:, i], b_mu[:, i] = ls, mm, bl, bm
    return dict(lse=lse, mu=mu, b_lse=b_lse, b_mu=b_mu)


def gc_add(y, E, inp, cd=D):
    """The image-level ContextBlock vector add (B, C) of y through freq_kernel_refs.gc_context, and its bound (module docstring)."""
    B, H, W, Cn = y.shape
    p = dict(r=y, wmask=inp["wmask"], w1=inp["w1"], w2=inp["w2"])
    add, _ = gc_context(p, tile_partition, cd)
    y64, wm = y.double().reshape(B, H * W, Cn), inp["wmask"].double()
    delta = (E.reshape(B, H * W, Cn) * wm.abs()).sum(2) + tau(Cn) * (y64.abs() * wm.abs()).sum(2)
    Dm = delta.max(1).values + 2.0 ** -16
    w64 = torch.softmax(y64 @ wm, 1)
    ctx = (w64[:, :, None] * y64).sum(1)
    a_ctx = (w64[:, :, None] * y64.abs()).sum(1)
    d_ctx = ((w64[:, :, None] * E.reshape(B, H * W, Cn)).sum(1) + torch.expm1(2 * Dm)[:, None] * (w64[:, :, None] * (y64 - ctx[:, None]).abs()).sum(1)
             + tau(H * W) * a_ctx)
    W1, W2 = inp["w1"].double().abs(), inp["w2"].double().abs()
    return add, (d_ctx + 2 * tau(Cn) * a_ctx) @ W1.t() @ W2.t()


def gc_ref(p, inp, cd=D, wrong=None):
    """Per group: conv_ref's dict plus tiles (gc_tiles) and add, b_add (gc_add)."""
    outs = conv_ref(p, inp, cd, None if wrong in ("gcrounded", "gc8x32") else wrong)
    for o, gs in zip(outs, p["groups"]):
        y = o["ref"]
        if wrong == "gcrounded":                             # WRONG: the pooling reads the 16-bit store
            y = y.to(DT[gs["dst"]["dtype"]]).to(cd)
        o["tiles"] = gc_tiles(y, o["E"], inp["wmask"], cd, th=8 if wrong == "gc8x32" else 4)
        o["add"], o["b_add"] = gc_add(y, o["E"], inp, cd)
    return outs


def conv_last_inputs(cimg, dt, B, H, W):
    g = torch.Generator().manual_seed(9000 + 100 * cimg + 10 * (dt == BF16) + B + 7 * H + 13 * W)
    rows = 16 if cimg == 1 else 32
    wl = torch.zeros(rows, 64)
    wl[:9 * cimg] = torch.randn(9 * cimg, 64, generator=g) / 24
    return dict(u=torch.randn(B, H, W, 64, generator=g).to(dt), wl=wl.to(dt), bias=torch.randn(cimg, generator=g) * 0.1,
                base=torch.rand(B, H, W, cimg, generator=g))


def conv_last_ref(q, cimg, cd=D, pad="zeros"):
    """fcvsr_conv_last: out (B,H,W,cimg) = base + bias + conv3x3(u), the table row tap * cimg + c.  Channel c is tail_last on the rows
    c, cimg + c, ...; bound tau(578) * S."""
    u, refs, Ss = q["u"].to(cd), [], []
    for c in range(cimg):
        wl = torch.zeros(16, 64, dtype=cd)
        wl[:9] = q["wl"].to(cd)[c:9 * cimg:cimg]
        refs.append(tail_last(u, wl, q["bias"][c:c + 1], q["base"][..., c], pad))
        Ss.append(tail_last(u.double().abs(), wl.double().abs(), q["bias"][c:c + 1].double().abs(), q["base"][..., c].double().abs()))
    return torch.stack(refs, 3), tau(9 * 64 + 2) * torch.stack(Ss, 3)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

def case(kernel, p, lean="unset", res="unset"):
    return dict(id=f"{p['name']}[{lean},{res}]", kernel=kernel, lean=lean, res=res, problem=p)


SHRUNK = {"stride2_0": (37, 53), "upconv1_ps_256_90x160": (37, 53)}      # the two largest problems of the table at a smaller size
# problems the planner rejects under FCVSR_MFMA_LEAN=0 although the table records a kernel (tests/test_conv_plan_cpu.py: NOW_REJECTED)
MSG_RES16 = "16-bit residuals are only supported by the lean 3x3 path"
MSG_GC16 = "ContextBlock fusion with a 16-bit destination needs the lean 3x3 path, no residuals"
NOW_REJECTED = {
    "shape_case2_64to128": MSG_RES16, "shape_case5_128to128": MSG_RES16, "shape_case7_64to64": MSG_RES16, "shape_case9_64to128": MSG_RES16,
    "shape_case1_64to64": MSG_RES16, "shape_case4_128to64": MSG_RES16,
    "bitwise0_128to64": MSG_RES16, "bitwise2_64to64": MSG_RES16, "bitwise3_64to128": MSG_RES16,
    "groupconv_2res_dst_f32": MSG_RES16, "groupconv_2res_dst_bf16": MSG_RES16,
    "gc_fused_dst_bf16": MSG_GC16,
}


def _shrink(p, H, W):
    """The table problem with every (dense) tensor of its single group rebuilt at H x W."""
    g = p["groups"][0]
    B = g["srcs"][0]["shape"][0]
    s2, ps = p["stride"] == 2, p["pixel_shuffle"]
    ho, wo = ((H + 1) // 2, (W + 1) // 2) if s2 else (H, W)
    q = dict(p)
    q["groups"] = [dict(srcs=[T((B, H, W, s["shape"][3]), s["dtype"]) for s in g["srcs"]],
                        res=[T((B, ho, wo, r["shape"][3]), r["dtype"]) for r in g["res"]],
                        dst=T((B, 2 * ho, 2 * wo, p["cout"] // 4) if ps else (B, ho, wo, p["cout"]), g["dst"]["dtype"]))]
    return q


def table_cases():
    """Every problem of the recorded table that is not rejected, once per distinct kernel string it reaches over the six policies;
    the four size_rule_* problems (3 x 128 x 512 pixels) are left out."""
    with open(TABLE) as f:
        tab = json.load(f)
    cases = []
    for p in tab["problems"]:
        if p["name"].startswith("size_rule_"):
            continue
        seen = set()
        for policy in tab["policies"]:
            lean, res = policy.split(",")
            r = p["results"][policy]
            if "kernel" not in r or r["kernel"] in seen or (p["name"] in NOW_REJECTED and lean == "0"):
                continue
            seen.add(r["kernel"])
            q = {k: v for k, v in p.items() if k != "results"}
            if p["name"] in SHRUNK:
                q = _shrink(q, *SHRUNK[p["name"]])
            cases.append(case(r["kernel"], q, lean, res))
    return cases


def _k(name, bf, *rest):
    return f"{name}<" + ", ".join(str(r).lower() if isinstance(r, bool) else str(r) for r in (bf,) + rest) + ">"


def edge_cases():
    """The smallest shapes at which the kernels can still go wrong and the table does not have (B = 2 unless the name says otherwise)."""
    Cs = []
    small = [(1, 1), (3, 5), (4, 32), (5, 33)]
    for mma in ("bf16", "f16"):
        bf = mma == "bf16"
        # ---- 3x3 generic and lean ----
        for (H, W) in small:
            p = problem(f"e3_{mma}_{H}x{W}", 3, [64], 64, [(H, W)], 2, mma, mma, act=2, slope=0.1, nres=1)
            Cs.append(case(_k("conv3_lean_kernel", bf, 64, True, True), p))
            p = problem(f"e3g_{mma}_{H}x{W}", 3, [64], 64, [(H, W)], 2, mma, "f32", act=3, nres=1, res="f32")
            Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p, lean="0"))
            Cs.append(case(_k("conv3_lean_kernel", bf, 64, True, False), p))
        p = problem(f"e3_{mma}_cout1_nchw", 3, [64], 1, [(5, 33)], 2, mma, "f32", act=0, dst_layout="nchw")
        Cs.append(case(_k("conv_mfma_kernel", bf, 32, 3), p, lean="0"))
        Cs.append(case(_k("conv3_lean_kernel", bf, 32, True, False), p))
        p = problem(f"e3_{mma}_cin4", 3, [4], 64, [(5, 33)], 2, mma, "f32", act=1)
        Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p))
        p = problem(f"e3_{mma}_3src_f32", 3, [64, 16, 4], 64, [(5, 33)], 2, mma, mma, src="f32", act=2, slope=0.2)
        Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p))
        p = problem(f"e3_{mma}_3src_16", 3, [64, 16, 8], 64, [(5, 33)], 2, mma, mma, act=2, slope=0.2, zero_tail=True)
        Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p))
        p = problem(f"e3_{mma}_lean_ff", 3, [64], 64, [(5, 33)], 2, mma, "f32", src="f32", act=0)
        Cs.append(case(_k("conv3_lean_kernel", bf, 64, False, False), p))
        p = problem(f"e3_{mma}_lean_f16dst", 3, [128], 64, [(5, 33)], 2, mma, mma, src="f32", act=1)
        Cs.append(case(_k("conv3_lean_kernel", bf, 64, False, True), p))
        if mma == "f16":                                     # the force_f16 first layer: byte-valued planar frames
            for cin, cout in ((7, 192), (21, 64)):
                p = problem(f"e3_f16_planar{cin}to{cout}", 3, [cin], cout, [(5, 33)], 2, mma, mma, src="f32", src_layout="nchw", act=0, values="k255")
                Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p))
        p = problem(f"e3_{mma}_cout32", 3, [64], 32, [(5, 33)], 2, mma, mma, act=1)
        Cs.append(case(_k("conv3_lean_kernel", bf, 32, True, True), p))
        # ---- 1x1 ----
        for cins, cout in [([128, 84], 64), ([64, 16], 64), ([256], 128), ([64], 576), ([64], 1152), ([64], 4), ([4], 64), ([64], 1)]:
            tag = "+".join(map(str, cins))
            p = problem(f"e1_{mma}_{tag}to{cout}", 1, cins, cout, [(5, 7)], 3, mma, "f32", act=2, slope=0.2,
                        dst_layout="nchw" if cout == 1 else "nhwc")
            lean1 = all(c % 64 == 0 for c in cins) and cout % 8 == 0
            Cs.append(case(_k("conv1_lean_kernel", bf, 64, p["groups"][0]["srcs"][0]["dtype"] != "f32", False, False) if lean1
                           else _k("conv_mfma_kernel", bf, 64 if cout > 32 else 32, 1), p))
            if lean1:
                Cs.append(case(_k("conv_mfma_kernel", bf, 64, 1), p, lean="0"))
        for npix in (1, 127, 128, 129):
            p = problem(f"e1_{mma}_flat{npix}", 1, [64], 64, [(1, npix)], 1, mma, mma, act=1, nres=1, res="f32")
            Cs.append(case(_k("conv1_lean_kernel", bf, 64, True, True, False), p))
            Cs.append(case(_k("conv_mfma_kernel", bf, 64, 1), p, lean="0"))
        for s16 in (False, True):
            for d16 in (False, True):
                for ps in (False, True):
                    p = problem(f"e1_{mma}_s{int(s16)}d{int(d16)}ps{int(ps)}", 1, [64], 256 if ps else 64, [(5, 7)], 3, mma,
                                mma if d16 else "f32", src=mma if s16 else "f32", act=3, slope_v=-0.1, ps=ps)
                    Cs.append(case(_k("conv1_lean_kernel", bf, 64, s16, d16, ps), p, res="0"))
                    if ps and s16 and d16:
                        Cs.append(case(_k("conv1ps_res_kernel", bf), p))
        p = problem(f"e1_{mma}_f32res_d16", 1, [64, 64], 64, [(5, 7)], 3, mma, mma, src="f32", act=0, nres=2, res="f32")
        Cs.append(case(_k("conv1_lean_kernel", bf, 64, False, True, False), p))
        p = problem(f"e1_{mma}_cout32", 1, [64], 32, [(5, 7)], 3, mma, "f32", act=0)
        Cs.append(case(_k("conv1_lean_kernel", bf, 32, True, False, False), p))
        Cs.append(case(_k("conv_mfma_kernel", bf, 32, 1), p, lean="0"))
        # ---- stride 2 ----
        s2 = [(1, 1), (1, 2), (2, 1), (5, 7), (8, 64), (9, 65)]
        for (H, W) in s2:
            for io in ("f32", mma):
                p = problem(f"s2_{mma}_{io}_{H}x{W}", 3, [64], 64, [(H, W)], 2, mma, io, src=io, stride=2, act=2, slope=0.1)
                Cs.append(case(_k("conv3s2_lean_kernel", bf, io != "f32", io != "f32"), p))
                Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p, lean="0"))
        p = problem(f"s2_{mma}_3levels", 3, [64], 64, [(9, 65), (5, 33), (3, 17)], 2, mma, mma, stride=2, act=3)
        Cs.append(case(_k("conv3s2_lean_kernel", bf, True, True), p))
        Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p, lean="0"))
        p = problem(f"s2_{mma}_cout128", 3, [128], 128, [(9, 65)], 2, mma, "f32", src="f32", stride=2, act=0)
        Cs.append(case(_k("conv3s2_lean_kernel", bf, False, False), p))
        Cs.append(case(_k("conv_mfma_kernel", bf, 64, 3), p, lean="0"))
        p = problem(f"s2_{mma}_f32_to_16", 3, [64], 64, [(9, 65)], 2, mma, mma, src="f32", stride=2, act=1)
        Cs.append(case(_k("conv3s2_lean_kernel", bf, False, True), p))
        # ---- conv3_res_kernel ----
        for H in (1, 7, 8, 9):
            for W in (1, 31, 32, 33):
                p = problem(f"r3_{mma}_{H}x{W}", 3, [64], 64, [(H, W)], 2, mma, mma, act=2, slope=0.1, nres=1, seed=int(mma == "f16" and H * W == 1))
                Cs.append(case(_k("conv3_res_kernel", bf, 1, 1, 1), p, res="1"))
        for d16 in (False, True):
            for nres in (0, 2):
                p = problem(f"r3_{mma}_128_noact_d{int(d16)}_r{nres}", 3, [128], 64, [(9, 33)], 2, mma, mma if d16 else "f32", act=0, nres=nres)
                Cs.append(case(_k("conv3_res_kernel", bf, (2 if nres == 0 else 1) if d16 else 0, 2, 2), p, res="1"))
        p = problem(f"r3_{mma}_64_noact", 3, [64], 64, [(9, 33)], 2, mma, mma, act=0)
        Cs.append(case(_k("conv3_res_kernel", bf, 2, 1, 2), p, res="1"))
        # instantiations the engine launches at 64 channels (tests/test_infer_conv_gpu.py: the engine closure found them)
        for d16, nres, act, var in [(True, 1, 0, (1, 1, 2)), (True, 0, 2, (2, 1, 1)), (False, 0, 3, (0, 1, 0)), (True, 0, 3, (2, 1, 0))]:
            p = problem(f"r3_{mma}_64_d{int(d16)}_r{nres}_act{act}", 3, [64], 64, [(9, 33)], 2, mma, mma if d16 else "f32", act=act, slope=0.1, nres=nres)
            Cs.append(case(_k("conv3_res_kernel", bf, *var), p, res="1"))
        for slope in (0.0, 0.1, 1.0, 1.5):
            p = problem(f"r3_{mma}_leaky{slope}", 3, [64], 64, [(9, 33)], 2, mma, mma, act=2, slope=slope, nres=1)
            Cs.append(case(_k("conv3_res_kernel", bf, 1, 1, 1 if slope <= 1.0 else 0), p, res="1"))
        for sv in (0.25, -0.1, 1.5):
            p = problem(f"r3_{mma}_prelu{sv}", 3, [128], 128, [(9, 33)], 2, mma, "f32", act=3, slope_v=sv, nres=1)
            Cs.append(case(_k("conv3_res_kernel", bf, 0, 2, 0), p, res="1"))
    return Cs


def gc_cases():
    """ContextBlock fusion: two level sets x three destinations x cout 64 / 36, and the span stress set."""
    Cs = []
    for li, levels in enumerate([[(1, 1), (4, 32), (5, 33)], [(21, 37), (11, 19), (6, 10)]]):
        for dst in ("f32", "bf16", "f16"):
            for cout in (64, 36 if dst == "f32" else 40):    # a 16-bit destination needs cout % 8 == 0: 36 is rejected there
                mma = "f16" if dst == "f16" else "bf16"
                bf = mma == "bf16"
                p = problem(f"gc_L{li}_{dst}_c{cout}", 3, [64], cout, levels, 2, mma, dst, act=0, gc=True)
                Cs.append(case(_k("conv3_lean_kernel", bf, 64, True, False) + " +gc", p))
    for dst in ("f32", "bf16"):
        p = problem(f"gc_span_{dst}", 3, [64], 64, [(9, 70), (5, 33), (3, 31)], 2, "bf16", dst, act=0, bias=False, gc=True, gc_stress="span")
        Cs.append(case(_k("conv3_lean_kernel", True, 64, True, False) + " +gc", p))
    return Cs


def mfma_cases():
    return table_cases() + edge_cases() + gc_cases()


def f32_cases():
    """The exact-f32 family (mma = None): `entry` "direct" is fcvsr_conv2d, "f32mfma" fcvsr_conv2d_f32mfma.  res_is_dst: the single
    residual is the destination itself (the NCHW result that conv_last0 adds into)."""
    Cs = []

    def add(entry, p):
        Cs.append(dict(id=p["name"], entry=entry, problem=p))

    acts = [dict(act=0), dict(act=1), dict(act=2, slope=0.1), dict(act=3, slope_v=0.3)]
    for i, (k, stride, cin, cout) in enumerate([(1, 1, 8, 1), (3, 1, 7, 3), (5, 1, 4, 8), (7, 1, 4, 16), (3, 1, 7, 448), (3, 2, 64, 16),
                                                (5, 2, 4, 3), (1, 2, 8, 8), (7, 2, 4, 1), (3, 2, 7, 448)]):
        add("direct", problem(f"d_k{k}s{stride}_{cin}to{cout}", k, [cin], cout, [(5, 9)], 2, None, "f32", stride=stride, **acts[i % 4]))
    add("direct", problem("d_3src", 3, [8, 4, 4], 16, [(5, 9)], 2, None, "f32", act=2, slope=0.2))
    add("direct", problem("d_nchw", 3, [7], 3, [(5, 9)], 2, None, "f32", src_layout="nchw", dst_layout="nchw", act=1))
    add("direct", problem("d_ps", 3, [8], 16, [(5, 9)], 2, None, "f32", ps=True, act=3))
    add("direct", problem("d_ps_448", 1, [8], 448, [(5, 9)], 2, None, "f32", ps=True, act=0))
    add("direct", problem("d_2res", 3, [8], 8, [(5, 9)], 2, None, "f32", nres=2, act=2, slope=0.1))
    p = problem("d_misaligned", 3, [8], 8, [(5, 9)], 2, None, "f32", nres=1, act=1)
    for t in p["groups"][0]["srcs"] + p["groups"][0]["res"] + [p["groups"][0]["dst"]]:
        t["offset"] = 1                                      # 4 bytes past a 16-byte boundary: the non-vector path
    add("direct", p)
    for (H, W) in [(1, 1), (4, 32), (5, 33), (10, 37)]:
        for k in (1, 3):
            for cout in (8, 68):
                add("f32mfma", problem(f"m_vec_k{k}_{cout}_{H}x{W}", k, [32], cout, [(H, W)], 2, None, "f32", nres=2, act=2, slope=0.1))
            for cout in (16, 64):
                add("f32mfma", problem(f"m_ps_k{k}_{cout}_{H}x{W}", k, [64], cout, [(H, W)], 2, None, "f32", ps=True, act=3))
            for cimg in (1, 3):
                add("f32mfma", problem(f"m_gen_k{k}_{cimg}_{H}x{W}", k, [64], cimg, [(H, W)], 2, None, "f32", nres=1, rs=(1.0,), act=0,
                                       dst_layout="nchw", res_is_dst=True))
    return Cs


CONV_LAST_CASES = [(cimg, dt, 2, H, W) for cimg in (1, 3) for dt in (BF16, F16) for (H, W) in [(1, 1), (3, 5), (21, 45)]]
