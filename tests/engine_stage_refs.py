"""Float64 stage references of the engine's forward (fcvsr_amd/engine.py), written with the oracle's own helpers; nothing here imports
fcvsr_amd.hip.  The engine records a tap after every stage; a stage here is a pure function from upstream taps to one tap, so a wiring
error of the engine (a weight slice, the dir*B + b stacking, a pointer pair, a slope, a residual sign) shows at the tap it first moves,
at full size, and not diluted through the rest of the network.  tests/test_engine_stage_refs_cpu.py pins the stages to `O.forward` and
shows that the bound below rejects named wrong variants (32, four of them findings); tests/test_engine_stages_gpu.py replays the engine's own taps.

The yardstick is the reference, not the engine.  For the taps t of a candidate (the engine, or a stand-in):

    ref  = replay(p, x, t)                    every stage in f64, fed from the candidate's upstream taps
    emul = replay(p, x, t, Mode(prec, ...))   the same stage with the rounding points of that configuration (below)
    E = emul - ref,   e = candidate - ref,    pass:  rms(e) <= K rms(E)  and  max|e| <= K max|E|,   K = 4.

Rounding points of Mode(prec, trunk16) - each stage's docstring says which apply and the engine line that causes it:
  op    operands (activations and weights) of every convolution and 1x1 layer are rounded to the MFMA dtype (Engine._convg: bf16 or
        f16); products are exact in f32 and the f32 accumulator is one further f32 rounding of the f64 sum.
  fq    frequency-domain layers use bf16 in both 16-bit modes (Engine._convg `freq=True`, Engine._adt(freq=True)).
  fe    feat_extract multiplies in f16 in both 16-bit modes (`force_f16`, Engine._feat_weights).
  A     tensors read only by MFMA layers are stored in the MFMA dtype (Engine._adt).
  T     the trunk is stored in the MFMA dtype with trunk16, else f32 (Engine._tdt).
  f32   kernels that compute in f32 (FFTs, CorrBlock, ConvBlk, the IAC step, DivEnh, ContextBlock, pooling and resampling) are evaluated
        in f32 by torch: that is the f32-arithmetic error a correct f32 evaluation of the same formula shows.  Without it E would be
        identically zero for stages 3 and 6 (no 16-bit rounding anywhere) and no engine could pass.
  chain precision = "f32" only: every convolution is one fmaf chain over its K terms (`fma_chain_conv`).
The stored dtype of a tap is part of its emulation (the store is a rounding point of the engine).

Mode(prec, trunk16, cd=torch.float32) is the stand-in engine of the CPU test: the same rounding points with every convolution
accumulated in f32 as well.

`mut` selects deliberately WRONG stage variants (MUTANTS); only the CPU test passes it."""
import torch
import torch.nn.functional as F

from oracle import fcvsr_oracle as O

D = torch.float64
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
K = 4.0


def rnd(t, dt):
    """t rounded to dt (nearest even), in t's dtype; None: unchanged."""
    return t if dt is None else t.to(dt).to(t.dtype)


def fma_chain_conv(x, w, b, stride=1):
    """The f32 convolution kernels' arithmetic (conv_direct.hip `acc = fmaf(v, w, acc)`; conv_f32.hip: v_mfma_f32_32x32x2_f32, "bit-equal
    to an fmaf chain"): one chain over all taps and input channels per output, every link rounded to f32, then + bias, rounded.  x, w: f64
    tensors holding f32 values - a product of two f32 is exact in f64, so each link is fl32(acc + v w) up to double rounding.  A blocked or
    pairwise f32 sum (torch's) has a several times smaller error at K = 576..1152 terms: measured on the GPU, the engine sat at 2.0-2.7x
    (rms) and up to 5.3x (max) of a torch-f32 emulation on exactly the stages made of such layers, and at 1.0 on the others."""
    B, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    pad = kh // 2
    xp = F.pad(x, (pad, pad, pad, pad))
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    acc = torch.zeros(B, Cout, Ho, Wo, dtype=D)
    a32 = torch.zeros(B, Cout, Ho, Wo, dtype=F32)
    for ky in range(kh):
        for kx in range(kw):
            xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            wk = w[:, :, ky, kx].t().reshape(Cin, 1, Cout, 1, 1)
            for ci in range(Cin):
                torch.addcmul(acc, wk[ci], xs[:, ci:ci + 1], out=acc)
                a32.copy_(acc)
                acc.copy_(a32)
    if b is not None:
        acc = rnd(acc + b.view(1, -1, 1, 1), F32)
    return acc


class Mode:
    def __init__(self, prec=None, trunk16=False, cd=D):
        self.prec, self.cd, self.ref = prec, cd, prec is None
        if prec is None:
            self.op = self.fq = self.fe = self.A = self.T = None
        elif prec == "f32":
            self.op = self.fq = self.fe = self.A = self.T = F32
        else:
            self.op = self.A = {"bf16": BF16, "f16": F16}[prec]
            self.fq, self.fe = BF16, F16
            self.T = self.op if trunk16 else F32
        self._p32 = {}

    def r(self, t, dt):
        return t if self.ref else rnd(t, dt)

    def f32(self, t):
        """An f32 value (the result of an elementwise f32 step of a kernel)."""
        return t if self.ref else rnd(t, F32)

    def params32(self, p):
        if id(p) not in self._p32:
            self._p32[id(p)] = (p, {k: v.float() for k, v in p.items()})
        return self._p32[id(p)][1]

    def conv(self, p, key, x, dt, stride=1, w=None):
        """nn.Conv2d `key` ("same" padding) on x with operands in dt."""
        w = p[key + ".weight"] if w is None else w
        b = p.get(key + ".bias")
        pad = w.shape[-1] // 2
        if self.ref:
            return F.conv2d(x, w, b, stride=stride, padding=pad)
        if self.cd == F32:
            return F.conv2d(rnd(x, dt).float(), rnd(w, dt).float(), None if b is None else b.float(), stride=stride,
                            padding=pad).double()
        if dt == F32:
            return fma_chain_conv(rnd(x, F32), rnd(w, F32), b, stride)
        return rnd(F.conv2d(rnd(x, dt), rnd(w, dt), b, stride=stride, padding=pad), F32)

    def k32(self, fn, *args):
        """fn (an f32 kernel of the engine) on tensors and parameter dicts: in f64 for the reference, in f32 otherwise."""
        if self.ref:
            return fn(*args)
        a32 = [self.params32(a) if isinstance(a, dict) else (a.float() if torch.is_tensor(a) else a) for a in args]
        return fn(*a32).double()


REF = Mode()


# ---- stages -------------------------------------------------------------------------------------------------------------------------

def s1_feat(m, p, x):
    """x -> feat.  fe: both operands f16 (engine.py `hip.feat_extract` / `_conv(..., force_f16=True)` in _forward); T: the features are
    stored in the trunk dtype (`p13`, `f13`, `f2` allocated with dtype=adt)."""
    B, T, C, H, W = x.shape
    return m.r(m.conv(p, "feat_extract.0", x.reshape(B, T * C, H, W), m.fe), m.T)


def s2_heads(m, p, x1, x2, x3, mut=None):
    """three feature groups -> off_f, off_b, sim.  f32: rfft2 and the CorrBlock lookup (fcvsr_rfft2, fcvsr_corr_lookup); fq: every layer
    of convfuse, convcrt and convcorr takes bf16 operands, the lookup channels included (`fcvsr_freq_mlp3`, `fcvsr_freq_head`,
    `fcvsr_convcorr_strip`, or `_convg(..., freq=True)`); the offset spectra `off` are stored in bf16 (`off = self._new(..., dtype=fdt)`),
    the residuals x?f and - x2f are added in f32, one after the other, before that store."""
    x1f, x2f, x3f = (m.k32(O.spec_pack, t) for t in (x1, x2, x3))
    xa, xb = (x3f, x1f) if mut == "dirs_swapped" else (x1f, x3f)

    def chain(prefix, t, n, w0=None):
        for li in range(n):
            t = m.conv(p, f"MGAA.{prefix}.{2 * li}", t, m.fq, w=w0 if li == 0 else None)
            if li < n - 1:
                t = F.relu(t)
        return t

    def off(xd):
        # the epilogue adds the residuals one at a time, each sum rounded (conv_direct.hip `v += a.rs[r] * res[r]`, res = [x?f, x2f],
        # res_scale = [1, -1]): (acc + x?f) - x2f.  At the DC pixel, where both spectra are ~H W mean, that costs u |x?f|, not u |x?f - x2f|
        sg = -1.0 if mut == "res_sign" else 1.0
        return m.r(m.f32(m.f32(chain("convfuse", torch.cat([xd, x2f], 1), 3) + sg * xd) - sg * x2f), m.fq)

    sim = chain("convcrt", x1f if mut == "sim_from_x1f" else x2f, 2)
    corr = m.k32(O.corr_lookup, x1f, x2f)
    if mut == "lookup_zero":
        corr = torch.zeros_like(corr)
    if mut == "lookup_transposed":
        B, _, H, Wf = corr.shape
        corr = corr.reshape(B, 9, 9, H, Wf).transpose(1, 2).reshape(B, 81, H, Wf)
    w0 = None
    if mut == "convcorr_cols":                               # the offset spectra multiplied by the lookup's weight columns
        w0 = p["MGAA.convcorr.0.weight"].clone()
        c2 = x1f.shape[1]
        w0[:, :c2] = p["MGAA.convcorr.0.weight"][:, 81:81 + c2]
    zero = torch.zeros_like(corr[:, :2])
    off4 = [chain("convcorr", torch.cat([off(xd), corr, zero], 1), 3, w0) for xd in (xa, xb)]
    return off4[0], off4[1], sim


def s3_offsets(m, p, off4, sim, A, H, W, mut=None):
    """off_f or off_b, sim -> offsets (B,A,2,H,W).  f32 throughout in every mode: ConvBlk with f32 "direct" weights, . * sim and the plane
    split (`fcvsr_convblk_heads` / `fcvsr_convblk`), `fcvsr_irfft2`."""
    def fn(p, off4, sim):
        outs = []
        for i in range(A):
            o = O.conv_blk(p, f"MGAA.MConvB.{0 if mut == 'mconvb0' else i}", off4)
            if mut != "no_sim":
                o = o * sim
            re, im = (o[:, 2:], o[:, :2]) if mut == "re_im_swapped" else (o[:, :2], o[:, 2:])
            outs.append(torch.fft.irfft2(torch.complex(re, im), s=(H, W), norm="backward"))
        return torch.stack(outs, 1)
    return m.k32(fn, p, off4, sim)


def s4_align(m, p, feat_in, x2, offsets, A, mut=None):
    """x1 or x3, x2, the engine's own offsets -> al.  op + A: conv_KP, F.0 and F.1 take MFMA operands and their outputs kp, k0, K are stored
    in the MFMA dtype (`kp`, `k0`, `K` allocated with dtype=self._adt(); the folded F.1 of `fcvsr_iac_step2_fused` rounds its kernels the
    same way, iac.hip "result rounded to the MFMA dtype"); f32: the IAC step itself (warp, SAC, + feat_in, LeakyReLU); T: every iteration's
    output is stored in the trunk dtype (`ping`, `ping2`, `al` allocated with dtype=fdt_act)."""
    C = feat_in.shape[1]
    kp = m.r(m.conv(p, "MGAA.conv_KP", x2, m.op), m.A)
    k0 = m.r(m.conv(p, "MGAA.F.0", kp, m.op), m.A)
    Kk = m.r(m.conv(p, "MGAA.F.1", k0, m.op), m.A)

    def step(s, o, k1, fin):
        s = O.warp_bilinear(s, o)
        if mut == "sac_once":                                # the vertical pass only
            k = k1.reshape(s.shape[0], C, 3, *s.shape[2:])
            sp = F.pad(s, (0, 0, 1, 1), mode="replicate")
            h = sum(sp[:, :, t:t + s.shape[2], :] * k[:, :, t] for t in range(3))
        else:
            h = O.sac_kernel1_twice(s, k1)
        return O._lrelu(h if mut == "no_feat_in" else h + fin, 0.2 if mut == "iac_slope_02" else 0.1)

    feat = feat_in
    for i in range(A):
        base = i * 6 * C + (3 * C if mut == "f2_half" else 0)
        o = offsets[:, (i - 1) % A if mut == "offs_prev_iter" else i]
        if mut == "offs_xy_swapped":
            o = o.flip(1)
        if mut == "offs_negated":
            o = -o
        feat = m.r(m.k32(step, feat, o, Kk[:, base:base + 3 * C], feat_in), m.T)
    return feat


def s5_out(m, p, al_f, al_b, x2, mut=None):
    """al_f, al_b, x2 -> mgaa.out.  op: conv3's operands; the residual x2 is added in f32; T: `out` is stored in the trunk dtype."""
    if mut == "al_swapped":
        al_f, al_b = al_b, al_f
    y = m.conv(p, "MGAA.conv3", torch.cat([al_f, al_b], 1), m.op)
    return m.r(m.f32(y if mut == "no_x2" else y + x2), m.T)


def s6_bands(m, x, Q, mut=None):
    """mgaa2.out -> mffr.bands (B,Q,n,H,W), low to high reversed.  f32 throughout (`fcvsr_rfft2`, `fcvsr_irfft2_bands`, f32 masks)."""
    def fn(x):
        fr = O.split_bands(x, Q)
        return torch.stack(fr if mut == "band_order" else fr[::-1], 1)
    return m.k32(fn, x)


def s7_mffr(m, p, bands, x, Q, mut=None):
    """mffr.bands, mgaa2.out -> mffr.out.  f32 throughout (`fcvsr_divenh*`, `fcvsr_ca_gate`, `fcvsr_scale_add`); T: `out` is stored in the
    trunk dtype (`_mffr(a2, out_dtype=tdt)`)."""
    c = 1.0 if mut == "factor_02" else 0.2

    def fn(p, bands, x):
        key = "MFFRblock"
        s_f, s_o = torch.zeros_like(x), torch.zeros_like(x)
        for i in range(Q):
            a = p[f"{key}.DivEnh_block.{i}.a"].reshape(1, -1, 1, 1)
            b = p[f"{key}.DivEnh_block.{i}.b"].reshape(1, -1, 1, 1)
            ca = f"{key}.DivEnh_block.{i}.ca"
            f = bands[:, i]
            if i == 0:
                t = f if mut == "no_mean" else f - f.mean(dim=(2, 3), keepdim=True)
                o = O._ca(p, ca, c * a * t * f + b * f)
            else:
                t = f - s_f + c * s_o
                o = O._ca(p, ca, c * a * t * f + b * f)
                if mut != "no_s_o":
                    o = o + O._ca(p, ca, c * a * s_o * f + b * f)
            s_f, s_o = s_f + f, s_o + o
        return O._ca(p, key + ".ca", s_o) + x
    return m.r(m.k32(fn, p, bands, x), m.T)


def s8_down(m, p, key, d):
    """mffr.out -> d1, d1 -> d2.  op: the stride-2 layer's operands; T: stored in the trunk dtype (`d1`, `d2` with dtype=tdt)."""
    return m.r(m.conv(p, key, d, m.op, stride=2), m.T)


def s9_block(m, p, key, xs, mut=None):
    """block inputs (3 levels) -> BlockRCB outputs.  op: the four 3x3 layers and up.0 / down.0; A: t1 and r1 are stored in the MFMA dtype
    (`_block_rcb`: `t1`, `r1` with self._adt()); T: t2, r (with trunk16: `rr = like(x, n, tdt if r16 else f32)`), R before the pool
    (`fcvsr_gc_apply_levels` stores R and its 2x2 pool P in the trunk dtype, `fcvsr_rcb_tail` rounds them where that sequence stores them),
    down.0's and up.0's outputs (`dn`, `up` = _new_like(P / R)) and the block outputs; f32: ContextBlock on the stored r, the pool, the
    bilinear x2 and the cross-scale sum (`fcvsr_gc_*`, `fcvsr_xscale*`).  down.0 runs on the pooled R as in the engine
    (conv1x1(avgpool2) = avgpool2(conv1x1))."""
    sl = 0.1 if mut == "rcb_slope_01" else 0.2

    def gc(p, r, z):
        c = r if mut == "ctx_identity" else O.context_block(p, key + ".RCB.gcnet", r)
        return O._lrelu(c, sl) + z

    R = []
    for z in xs:
        t1 = m.r(O._lrelu(m.conv(p, key + ".body.0", z, m.op), 0.1), m.A)
        t2 = m.r(m.conv(p, key + ".body.2", t1, m.op), m.T)
        r1 = m.r(O._lrelu(m.conv(p, key + ".RCB.body.0", t2, m.op), sl), m.A)
        r = m.r(m.conv(p, key + ".RCB.body.2", r1, m.op), m.T)
        R.append(m.r(m.k32(gc, p, r, t2), m.T))
    kd, ku = (".up.0", ".down.0") if mut == "updown_swapped" else (".down.0", ".up.0")

    def dn(z):
        P = m.r(m.k32(lambda t: F.avg_pool2d(t, 2), z), m.T)
        return m.r(m.conv(p, key + kd, P, m.op), m.T)

    def up(z):
        return m.r(m.conv(p, key + ku, z, m.op), m.T)

    def comb(x, r, rs, d, u):
        y = x + rs * r
        if d is not None:
            y = y + d
        if u is not None:
            y = y + F.interpolate(u, scale_factor=2.0, mode="bilinear", align_corners=False)
        return y

    rs0 = 1.0 if mut == "r0_once" else 2.0
    return [m.r(m.k32(comb, xs[0], R[0], rs0, None, up(R[1])), m.T),
            m.r(m.k32(comb, xs[1], R[1], 1.0, dn(R[0]), up(R[2])), m.T),
            m.r(m.k32(comb, xs[2], R[2], 2.0, dn(R[1]), None), m.T)]


def s10_group(m, p, key, t, cur, xs, last, mut=None):
    """BlockRCB outputs, the group's input, SCNetbk's input -> group outputs.  op: the group conv's operands; both skips are added in f32 in
    its epilogue (`res=[cur, xs]`); stored in T, the last group's (o0..o2) in A (`_scnet(..., self._adt() if fuse16 ...)`)."""
    outs = []
    for l in range(3):
        y = m.conv(p, key + ".conv", t[l], m.op)
        if mut != "no_group_skip":
            y = m.f32(y + cur[l])
        if last and mut != "no_outer_skip":
            y = m.f32(y + xs[l])
        outs.append(m.r(y, m.A if last else m.T))
    return outs


def _ps_wrong(x):
    """WRONG pixel shuffle: sub-pixel-major channel order, out[c, 2h+i, 2w+j] = in[(2i+j) C/4 + c]."""
    B, C, H, W = x.shape
    return x.reshape(B, 2, 2, C // 4, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, C // 4, 2 * H, 2 * W)


def s11_fz(m, p, o0, o1, o2):
    """o0..o2 -> fz.  op: every layer's operands; A (fuse16 sources, `_forward`): l3_2, l2p, fz0 and fz are stored in the MFMA dtype; l3_1
    and l2 stay f32."""
    a = p["lrelu.weight"]
    l3_1 = O.pixel_shuffle2(m.f32(O._prelu(m.conv(p, "upconv1_L3", o2, m.op), a)))
    l3_2 = m.r(O.pixel_shuffle2(l3_1), m.A)
    l2 = m.f32(O._prelu(m.conv(p, "upconv1_L2", o1, m.op), a))
    l2p = m.r(O.pixel_shuffle2(m.f32(l2 + m.conv(p, "upconv1_L2_2", torch.cat([l2, l3_1], 1), m.op))), m.A)
    fz0 = m.r(m.conv(p, "upconv_fuse", torch.cat([o0, l2p, l3_2], 1), m.op), m.A)
    return m.r(m.conv(p, "recorb0", fz0, m.op), m.A)


def s12_out(m, p, fz, x, mut=None):
    """fz, x -> out.  op: upconv1, upconv2, conv_last0; A: u1 and u2 are stored in the MFMA dtype (`u1`, `u2` with self._adt(); the fused
    tail rounds u2 to it in LDS, tail_fused.hip); f32: the bilinear x4 base and its sum."""
    T = x.shape[1]
    a = p["lrelu.weight"] * (0.5 if mut == "prelu_slope" else 1.0)
    ps = _ps_wrong if mut == "ps_order" else O.pixel_shuffle2
    u1 = m.r(m.f32(O._prelu(ps(m.conv(p, "upconv1", fz, m.op)), a)), m.A)
    u2 = m.r(m.f32(O._prelu(ps(m.conv(p, "upconv2", u1, m.op)), a)), m.A)
    y = m.conv(p, "conv_last0", u2, m.op)
    base = m.k32(lambda t: F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=False), x[:, T // 2])
    return m.f32(y if mut == "no_base" else y + base)


# name -> (stage, needs warp offsets beyond a pixel cell: only the x20 weight set separates it)
MUTANTS = {
    "dirs_swapped": (2, False), "res_sign": (2, False), "lookup_zero": (2, False), "lookup_transposed": (2, False),
    "sim_from_x1f": (2, False), "convcorr_cols": (2, False),
    "mconvb0": (3, False), "no_sim": (3, False), "re_im_swapped": (3, False),
    "offs_xy_swapped": (4, True), "offs_negated": (4, True), "offs_prev_iter": (4, True), "f2_half": (4, False),
    "sac_once": (4, False), "no_feat_in": (4, False), "iac_slope_02": (4, False), "offs_f_for_b": (4, True),
    "no_x2": (5, False), "al_swapped": (5, False),
    "band_order": (6, False), "factor_02": (7, False), "no_s_o": (7, False), "no_mean": (7, False),
    "updown_swapped": (9, False), "r0_once": (9, False), "ctx_identity": (9, False), "rcb_slope_01": (9, False),
    "no_group_skip": (10, False), "no_outer_skip": (10, False),
    "prelu_slope": (12, False), "ps_order": (12, False), "no_base": (12, False),
}


def stage_of(tap):
    """The stage that produces a tap."""
    if tap == "feat":
        return 1
    if tap.startswith("mgaa"):
        s = tap.split(".")[1]
        return 2 if s in ("off_f", "off_b", "sim") else 3 if s.startswith("offsets") else 4 if s.startswith("al_") else 5
    if tap in ("d1", "d2"):
        return 8
    if tap.startswith("sc.g"):
        return 9 if ".k" in tap else 10
    return {"mffr.bands": 6, "mffr.out": 7, "sc.o0": 10, "sc.o1": 10, "sc.o2": 10, "fz": 11, "out": 12}[tap]


def replay(p, x, taps, mode=None, mut=None, stages=None, chain=False):
    """{tap: value} (f64) with every stage fed from `taps`, never from its own outputs.  p: f64 parameter dict keyed like the state_dict;
    x: the input clip; mode: None / REF for the reference, Mode(...) for an emulation; stages: restrict to these stage numbers.
    chain=True is the opposite: a whole forward under `mode`, every stage fed from the stages before it (`taps` may be empty) - the
    stand-in engine of the CPU test."""
    m = mode or REF
    cfg = O.infer_config(p)
    n, A, Q, G = cfg["n"], cfg["A"], cfg["Q"], cfg["G"]
    x = x.to(D)
    B, T, C, H, W = x.shape
    t = {k: v.to(D) for k, v in taps.items()}


    class Out(dict):
        def __setitem__(self, k, v):
            dict.__setitem__(self, k, v)
            if chain:
                t[k] = v
    out = Out()

    def want(s):
        return stages is None or s in stages

    def mu(s, only=None):
        return mut if mut is not None and MUTANTS[mut][0] == s and (only is None or mut in only) else None

    with torch.no_grad():
        if want(1):
            out["feat"] = s1_feat(m, p, x)
        grp = lambda i: t["feat"][:, i * n:(i + 1) * n]
        if want(2) or want(3) or want(4) or want(5):
            for tag in "132":
                x1, x2, x3 = {"1": lambda: (grp(0), grp(1), grp(2)), "3": lambda: (grp(4), grp(5), grp(6)),
                              "2": lambda: (t["mgaa1.out"], grp(3), t["mgaa3.out"])}[tag]()
                pre = f"mgaa{tag}."
                if want(2):
                    for k, v in zip(("off_f", "off_b", "sim"), s2_heads(m, p, x1, x2, x3, mu(2))):
                        out[pre + k] = v
                if want(3):
                    for d in "fb":
                        out[pre + "offsets_" + d] = s3_offsets(m, p, t[pre + "off_" + d], t[pre + "sim"], A, H, W, mu(3))
                if want(4):
                    m4 = mu(4)
                    out[pre + "al_f"] = s4_align(m, p, x1, x2, t[pre + "offsets_f"], A, None if m4 == "offs_f_for_b" else m4)
                    out[pre + "al_b"] = s4_align(m, p, x3, x2, t[pre + ("offsets_f" if m4 == "offs_f_for_b" else "offsets_b")], A,
                                                 None if m4 == "offs_f_for_b" else m4)
                if want(5):
                    out[pre + "out"] = s5_out(m, p, t[pre + "al_f"], t[pre + "al_b"], x2, mu(5))
        if want(6):
            out["mffr.bands"] = s6_bands(m, t["mgaa2.out"], Q, mu(6))
        if want(7):
            out["mffr.out"] = s7_mffr(m, p, t["mffr.bands"], t["mgaa2.out"], Q, mu(7))
        if want(8):
            out["d1"] = s8_down(m, p, "rconcat1", t["mffr.out"])
            out["d2"] = s8_down(m, p, "rconcat2", t["d1"])
        if want(9) or want(10):
            xs = [t["mffr.out"], t["d1"], t["d2"]]
            cur = xs
            for g in range(G):
                tt = cur
                for k in range(3):
                    if want(9):
                        for l, v in enumerate(s9_block(m, p, f"recorb1.body.{g}.body.{k}", tt, mu(9))):
                            out[f"sc.g{g}.k{k}.l{l}"] = v
                    tt = [t[f"sc.g{g}.k{k}.l{l}"] for l in range(3)]
                last = g == G - 1
                if want(10):
                    for l, v in enumerate(s10_group(m, p, f"recorb1.body.{g}", tt, cur, xs, last, mu(10))):
                        out[f"sc.g{g}.l{l}"] = v
                        if last:
                            out[f"sc.o{l}"] = v
                cur = [t[f"sc.g{g}.l{l}"] for l in range(3)]
        if want(11):
            out["fz"] = s11_fz(m, p, t["sc.o0"], t["sc.o1"], t["sc.o2"])
        if want(12):
            out["out"] = s12_out(m, p, t["fz"], x, mu(12))
    return out


# ---- the criterion ------------------------------------------------------------------------------------------------------------------

def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def ratios(cand, ref, emul):
    """{tap: (rms(e) / rms(E), max|e| / max|E|)} over the taps of `ref`; a tap with E = 0 passes only with e = 0."""
    res = {}
    for k, r in ref.items():
        e, E = cand[k].to(D) - r, emul[k] - r
        assert e.shape == E.shape, (k, e.shape, E.shape)
        q = []
        for a, b in ((rms(e), rms(E)), (float(e.abs().max()), float(E.abs().max()))):
            q.append(0.0 if a == 0 else float("inf") if b == 0 or a != a else a / b)
        res[k] = tuple(q)
    return res


def judge(p, x, taps, mode, stages=None):
    """Replay `taps` (a candidate's) in f64 and under `mode`: {tap: (rms ratio, max ratio)}.  The candidate passes a tap when both are <= K."""
    return ratios(taps, replay(p, x, taps, REF, stages=stages), replay(p, x, taps, mode, stages=stages))


def worst(res):
    k = max(res, key=lambda k: max(res[k]))
    return k, max(res[k])


def params64(p):
    """The f32 weights as f64 (exact)."""
    return {k: v.to(D) for k, v in p.items()}
