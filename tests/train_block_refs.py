"""Float64 CPU references of the fused training blocks (fcvsr_amd/train/blocks.py; kernels in csrc/train_rcb.hip, train_mffr.hip,
train_iac.hip and train_ops.hip), written per element from the formulas in the kernel file headers.  Nothing here calls the code under
test and nothing is derived by autograd; tests/test_train_block_refs_cpu.py pins every function to torch autograd in float64 on the
plain operator chain, tests/test_train_blocks_gpu.py compares the kernels with them.

Every summed quantity is a triple (ref, S, n): S is the same sum over the absolute values of its terms, n the number of terms.
A term is a product of exact f64 operands; three rules say what stands in for an operand that was itself computed:
  pooled    a sum over the pixels of an image (ctx, gadd, the means, gg) that is an operand of a parameter gradient enters with its
            own S (the gradient is then the double sum over images and pixels, n = B * HW); elsewhere with its absolute value;
  dense     a product with one of the small matrices (W1, W2, the gate's two layers) is taken on absolute values (|W| |x|);
  softmax   m_p = exp(l_p - M) / sum_q exp(l_q - M):  a perturbation d of the logits changes m_p by m_p (d_p - sum_q m_q d_q), and the
            logit l_p = wmask . r_p has the condition L_p = sum_c |wmask_c r_pc|, so m_p enters as Sm_p = m_p (1 + L_p + sum_q m_q L_q)
            in the forward quantities (ctx, add and the scales), which the stress inputs with logits up to +-40 check.  The backward
            sums (dwmask, dw1) take m_p itself: they run at L_p of about 9, where eight roundings of a logit (8 * 2^-24 * L_p) stay a
            factor of three below tau(n) >= 2^-16, and a looser S would hide one dropped block of 64;
  sigmoid   g = 1 / (1 + exp(-s)) enters as g + g (1 - g) S(s).
LeakyReLU / ReLU scale by the slope of the side the f64 value is on (the tests keep every such value away from the kink).
Elementwise results that depend on a pooled statistic carry `*_scale`: the entry's own condition, i.e. the absolute values of its
direct terms (|lrelu(u)| + |z| for out, |gSf'| for gf, ...: at least |ref|, and not small where those terms cancel) plus the same
rules applied to the part that comes through the statistic.

Layouts: NCHW tensors as blocks.py takes them, except iac_bwd_sac (dense NHWC, the C ABI's layout)."""
import math

import torch

D = torch.float64


def _d(t):
    return t.detach().to(D).cpu()


def _lrelu(x, s):
    return torch.where(x > 0, x, x * s)


def _dl(x, s):
    """LeakyReLU'(x) as a tensor of 1 / slope."""
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, s))


# -------------------------------------------------------------------------------------------------------------------------------------
# RCB tail (train_rcb.hip):  R = lrelu(r + add) + z,  add = W2 lrelu(W1 ctx),  ctx[c] = sum_p m_p r[p][c],  m = softmax_p(wmask . r[p])

def rcb_tail_forward(r, z, wmask, w1, w2, slope):
    r, z = _d(r), _d(z)
    B, C, H, W = r.shape
    wm, W1, W2 = _d(wmask).reshape(C), _d(w1).reshape(C, C), _d(w2).reshape(C, C)
    rm = r.reshape(B, C, H * W)
    logit = torch.einsum("c,bcp->bp", wm, rm)
    L = torch.einsum("c,bcp->bp", wm.abs(), rm.abs())
    e = torch.exp(logit - logit.max(dim=1, keepdim=True).values)
    m = e / e.sum(dim=1, keepdim=True)
    Sm = m * (1.0 + L + (m * L).sum(dim=1, keepdim=True))
    ctx = torch.einsum("bp,bcp->bc", m, rm)
    S_ctx = torch.einsum("bp,bcp->bc", Sm, rm.abs())
    t = ctx @ W1.t()
    S_t = S_ctx @ W1.abs().t()
    a = _lrelu(t, slope)
    S_a = S_t * _dl(t, slope)
    add = a @ W2.t()
    S_add = S_a @ W2.abs().t()
    u = r + add[:, :, None, None]
    out = _lrelu(u, slope) + z
    return dict(out=out, out_scale=_lrelu(u, slope).abs() + z.abs() + S_add[:, :, None, None] * _dl(u, slope), u=u, m=m, Sm=Sm, logit=logit,
                ctx=(ctx, S_ctx, H * W), t=(t, S_t, H * W), a=(a, S_a, H * W), add=(add, S_add, H * W))


def rcb_tail_reference(r, z, wmask, w1, w2, slope, g):
    """out, gr, gz (elementwise; out_scale / gr_scale: the statistic's share of their condition) and the triples ctx, t, add, gadd,
    gctx, dwmask, dw1, dw2."""
    f = rcb_tail_forward(r, z, wmask, w1, w2, slope)
    r, g = _d(r), _d(g)
    B, C, H, W = r.shape
    HW = H * W
    wm, W1, W2 = _d(wmask).reshape(C), _d(w1).reshape(C, C), _d(w2).reshape(C, C)
    rm = r.reshape(B, C, HW)
    m, Sm = f["m"], f["Sm"]
    (ctx, S_ctx, _), (t, S_t, _), (a, S_a, _) = f["ctx"], f["t"], f["a"]
    gu = g * _dl(f["u"], slope)
    gadd, S_gadd = gu.sum(dim=(2, 3)), gu.abs().sum(dim=(2, 3))
    ga, A_ga = gadd @ W2, gadd.abs() @ W2.abs()                   # ga[c] = sum_k W2[k][c] gadd[k]
    gt, A_gt = ga * _dl(t, slope), A_ga * _dl(t, slope)
    gctx, A_gctx = gt @ W1, A_gt @ W1.abs()
    A_a = (ctx.abs() @ W1.abs().t()) * _dl(t, slope)
    dw2 = torch.einsum("bc,bk->ck", gadd, a)
    S_dw2 = torch.einsum("bc,bk->ck", S_gadd, A_a)
    dw1 = torch.einsum("bc,bk->ck", gt, ctx)
    S_dw1 = torch.einsum("bc,bk->ck", A_gt, torch.einsum("bp,bcp->bc", m, rm.abs()))
    gm = torch.einsum("bc,bcp->bp", gctx, rm)
    A_gm = torch.einsum("bc,bcp->bp", A_gctx, rm.abs())
    gdot = (gctx * ctx).sum(dim=1, keepdim=True)
    A_gdot = (A_gctx * ctx.abs()).sum(dim=1, keepdim=True)
    gl = m * (gm - gdot)
    gr = gu + (m[:, None, :] * gctx[:, :, None] + wm[None, :, None] * gl[:, None, :]).reshape(B, C, H, W)
    gr_scale = gu.abs() + (Sm[:, None, :] * A_gctx[:, :, None] + wm.abs()[None, :, None] * (Sm * (A_gm + A_gdot))[:, None, :]).reshape(B, C, H, W)
    dwm = torch.einsum("bp,bcp->c", gl, rm)
    # gl_p = m_p (gm_p - gdot) cancels (exactly, for a single pixel): its terms are those of the two 64-term products
    G = torch.einsum("bc,bcp->bp", gctx.abs(), rm.abs()) + (gctx * ctx).abs().sum(dim=1, keepdim=True)
    S_dwm = torch.einsum("bp,bcp->c", m * G, rm.abs())
    S_gctx = A_gctx
    f.update(gr=gr, gr_scale=gr_scale, gz=g, gadd=(gadd, S_gadd, HW), gctx=(gctx, S_gctx, HW),
             dwmask=(dwm.reshape(1, C, 1, 1), S_dwm.reshape(1, C, 1, 1), B * HW),
             dw1=(dw1.reshape(C, C, 1, 1), S_dw1.reshape(C, C, 1, 1), B * HW),
             dw2=(dw2.reshape(C, C, 1, 1), S_dw2.reshape(C, C, 1, 1), B * HW))
    return f


# -------------------------------------------------------------------------------------------------------------------------------------
# DivEnh band (train_mffr.hip):  t = f - Sf + 0.2 So;  e1 = (0.2 a t + b) f;  e2 = (0.2 a So + b) f;  Sf' = Sf + f;
#   So' = So + e1 CA(e1) + e2 CA(e2),  CA(e) = sigmoid(W2 relu(W1 mean_HW(e)))

def divenh_band_forward(f, sf, so, a, b, w1, w2):
    f, sf, so = _d(f), _d(sf), _d(so)
    B, C, H, W = f.shape
    CR = C // 16
    av, bv = _d(a).reshape(1, C, 1, 1), _d(b).reshape(1, C, 1, 1)
    W1, W2 = _d(w1).reshape(CR, C), _d(w2).reshape(C, CR)
    t = f - sf + 0.2 * so
    S_tt = f.abs() + sf.abs() + 0.2 * so.abs()
    c1, c2 = 0.2 * av * t + bv, 0.2 * av * so + bv
    S_c1, S_c2 = 0.2 * av.abs() * S_tt + bv.abs(), 0.2 * av.abs() * so.abs() + bv.abs()
    e = [c1 * f, c2 * f]
    S_e = [S_c1 * f.abs(), S_c2 * f.abs()]
    mean, S_mean, pre, S_pre, z, S_z, A_z, gate, S_gate, S_s = [], [], [], [], [], [], [], [], [], []
    for k in range(2):
        mean.append(e[k].mean(dim=(2, 3)))
        S_mean.append(S_e[k].mean(dim=(2, 3)))
        pre.append(mean[k] @ W1.t())
        S_pre.append(S_mean[k] @ W1.abs().t())
        z.append(torch.relu(pre[k]))
        S_z.append(S_pre[k] * (pre[k] > 0))
        A_z.append((mean[k].abs() @ W1.abs().t()) * (pre[k] > 0))
        s = z[k] @ W2.t()
        S_s.append(S_z[k] @ W2.abs().t())
        gate.append(torch.sigmoid(s))
        S_gate.append(gate[k] + gate[k] * (1 - gate[k]) * S_s[k])
    g1, g2 = gate[0][:, :, None, None], gate[1][:, :, None, None]
    nsf = sf + f
    nso = so + e[0] * g1 + e[1] * g2
    nso_scale = so.abs() + S_e[0] * S_gate[0][:, :, None, None] + S_e[1] * S_gate[1][:, :, None, None]
    return dict(Sf=nsf, So=nso, So_scale=nso_scale, t=t, S_tt=S_tt, c=[c1, c2], S_c=[S_c1, S_c2], e=e, S_e=S_e, mean=mean,
                S_mean=S_mean, pre=pre, S_pre=S_pre, z=z, S_z=S_z, A_z=A_z, gate=gate, S_gate=S_gate, S_s=S_s, HW=H * W)


def divenh_band_reference(f, sf, so, a, b, w1, w2, gsf, gso):
    """Sf', So', gf, gSf, gSo (elementwise, with *_scale) and the triples ga, gb, dw1, dw2."""
    o = divenh_band_forward(f, sf, so, a, b, w1, w2)
    f, so, gsf, gso = _d(f), _d(so), _d(gsf), _d(gso)
    B, C, H, W = f.shape
    HW, CR = H * W, C // 16
    av = _d(a).reshape(1, C, 1, 1)
    W1, W2 = _d(w1).reshape(CR, C), _d(w2).reshape(C, CR)
    ge, S_ge, gu, S_gu, gz, S_gz = [], [], [], [], [], []
    for k in range(2):
        g, S_g, S_s = o["gate"][k], o["S_gate"][k], o["S_s"][k]
        gg = (gso * o["e"][k]).sum(dim=(2, 3))
        S_gg = (gso.abs() * o["S_e"][k]).sum(dim=(2, 3))
        gu.append(gg * g * (1 - g))
        S_gu.append(S_gg * g * (1 - g))
        on = (o["pre"][k] > 0).to(D)
        gz.append((gu[k] @ W2) * on)                               # gz[h] = sum_c W2[c][h] gu[c]
        S_gz.append((gu[k].abs() @ W2.abs()) * on)
        gm = gz[k] @ W1 / HW                                       # gm[c] = sum_h W1[h][c] gz[h]
        S_gm = S_gz[k] @ W1.abs() / HW
        ge.append(gso * g[:, :, None, None] + gm[:, :, None, None])
        S_ge.append(gso.abs() * S_g[:, :, None, None] + S_gm[:, :, None, None])
    gt = 0.2 * av * f * ge[0]
    S_gt = 0.2 * av.abs() * f.abs() * S_ge[0]
    gf = gsf + o["c"][0] * ge[0] + o["c"][1] * ge[1] + gt
    gf_scale = gsf.abs() + o["S_c"][0] * S_ge[0] + o["S_c"][1] * S_ge[1] + S_gt
    gSf = gsf - gt
    gSo = gso + 0.2 * gt + 0.2 * av * f * ge[1]
    gSo_scale = gso.abs() + 0.2 * S_gt + 0.2 * av.abs() * f.abs() * S_ge[1]
    ga = (0.2 * f * (o["t"] * ge[0] + so * ge[1])).sum(dim=(0, 2, 3))
    S_ga = (0.2 * f.abs() * (o["t"].abs() * ge[0].abs() + so.abs() * ge[1].abs())).sum(dim=(0, 2, 3))
    gb = (f * (ge[0] + ge[1])).sum(dim=(0, 2, 3))
    S_gb = (f.abs() * (ge[0].abs() + ge[1].abs())).sum(dim=(0, 2, 3))
    dw2 = sum(torch.einsum("bc,bh->ch", gu[k], o["z"][k]) for k in range(2))
    S_dw2 = sum(torch.einsum("bc,bh->ch", S_gu[k], o["A_z"][k]) for k in range(2))
    dw1 = sum(torch.einsum("bh,bc->hc", gz[k], o["mean"][k]) for k in range(2))
    S_dw1 = sum(torch.einsum("bh,bc->hc", S_gz[k], o["S_mean"][k]) for k in range(2))
    n = B * HW
    o.update(gf=gf, gf_scale=gf_scale, gSf=gSf, gSf_scale=gsf.abs() + S_gt, gSo=gSo, gSo_scale=gSo_scale,
             ga=(ga, S_ga, n), gb=(gb, S_gb, n), dw1=(dw1.reshape(CR, C, 1, 1), S_dw1.reshape(CR, C, 1, 1), n),
             dw2=(dw2.reshape(C, CR, 1, 1), S_dw2.reshape(C, CR, 1, 1), n))
    return o


# -------------------------------------------------------------------------------------------------------------------------------------
# backward of the SAC half of one IAC iteration (train_iac.hip), dense NHWC:
#   v[y][x] = sum_t s[clamp(y+t-1)][x] K[c*3+t][y][x];  h[y][x] = sum_t v[y][clamp(x+t-1)] K[c*3+t][y][x];  out = lrelu(h + feat_in)

def iac_bwd_sac_reference(gy, yout, v, s, k1, slope, gfin0=None, gk0=None):
    """gy, yout, v, s: (B,H,W,C); k1: (B,H,W,3C), channel c*3+t.  gfin0 / gk0: what the destinations hold when the call accumulates.
    Returns the triples gfin, gv, gK; the activation mask is yout > 0, exactly as the kernel takes it."""
    gy, yout, v, s, k1 = _d(gy), _d(yout), _d(v), _d(s), _d(k1)
    B, H, W, C = gy.shape
    K = k1.reshape(B, H, W, C, 3)
    # the kernel multiplies by the f32 slope
    gh = torch.where(yout > 0, gy, gy * float(torch.tensor(slope, dtype=torch.float32)))
    gfin, S_gfin, n_fin = gh.clone(), gh.abs(), 1
    if gfin0 is not None:
        gfin, S_gfin, n_fin = gfin + _d(gfin0), S_gfin + _d(gfin0).abs(), 2
    gv, S_gv = torch.zeros_like(gh), torch.zeros_like(gh)
    for t in range(3):                                            # position clamp(x'+t-1) receives gh[x'] K[t][x']
        xs = (torch.arange(W) + t - 1).clamp(0, W - 1)
        gv.index_add_(2, xs, gh * K[..., t])
        S_gv.index_add_(2, xs, (gh * K[..., t]).abs())
    gK, S_gK = torch.empty_like(K), torch.empty_like(K)
    for t in range(3):
        xs = (torch.arange(W) + t - 1).clamp(0, W - 1)
        ys = (torch.arange(H) + t - 1).clamp(0, H - 1)
        gK[..., t] = gh * v[:, :, xs] + gv * s[:, ys]
        S_gK[..., t] = (gh * v[:, :, xs]).abs() + S_gv * s[:, ys].abs()
    gK, S_gK, n_k = gK.reshape(B, H, W, 3 * C), S_gK.reshape(B, H, W, 3 * C), 6
    if gk0 is not None:
        gK, S_gK, n_k = gK + _d(gk0), S_gK + _d(gk0).abs(), 7
    return dict(gfin=(gfin, S_gfin, n_fin), gv=(gv, S_gv, 4), gK=(gK, S_gK, n_k))


# -------------------------------------------------------------------------------------------------------------------------------------
# PReLU with one slope (train_ops.hip)

def prelu_reference(x, slope, g):
    """y, gx (elementwise: one product each) and the triple gslope = sum over x <= 0 of g x."""
    x, g = _d(x), _d(g)
    a = float(_d(slope).reshape(-1)[0])
    pos = x > 0
    y = torch.where(pos, x, a * x)
    gx = torch.where(pos, g, a * g)
    terms = torch.where(pos, torch.zeros_like(x), g * x)
    return dict(y=y, gx=gx, gslope=(terms.sum().reshape(_d(slope).shape), terms.abs().sum().reshape(_d(slope).shape), x.numel()))


# -------------------------------------------------------------------------------------------------------------------------------------
# cross-scale sum (fcvsr_xscale forward; up2_adjoint / pool2_adjoint in train_rcb.hip)

def pool2_forward(d):
    """2x2 mean: (B,C,2H,2W) -> (B,C,H,W)."""
    d = _d(d)
    return 0.25 * (d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2] + d[:, :, 1::2, 0::2] + d[:, :, 1::2, 1::2])


def pool2_adjoint(g):
    """out[i][j] = 0.25 g[i / 2][j / 2]: exact in f32."""
    g = _d(g)
    return 0.25 * g.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _up2_taps(n):
    """x2 bilinear, align_corners = False, source index clamped: output i reads low-resolution lo[i], hi[i] with weights 1 - w, w."""
    i = torch.arange(2 * n, dtype=D)
    src = ((i + 0.5) / 2 - 0.5).clamp_min(0.0)
    lo = src.floor().long().clamp_max(n - 1)
    hi = (lo + 1).clamp_max(n - 1)
    w = src - lo.to(D)
    return lo, hi, w


def up2_forward(u):
    """(B,C,h,w) -> (B,C,2h,2w)."""
    u = _d(u)
    lo, hi, w = _up2_taps(u.shape[2])
    r = u[:, :, lo] * (1 - w)[None, None, :, None] + u[:, :, hi] * w[None, None, :, None]
    lo, hi, w = _up2_taps(u.shape[3])
    return r[:, :, :, lo] * (1 - w) + r[:, :, :, hi] * w


def up2_adjoint(g):
    """(B,C,2h,2w) -> the triple of (B,C,h,w): transposed up2_forward, at most 16 terms per entry."""
    g = _d(g)

    def one(x):
        h = x.shape[2] // 2
        lo, hi, w = _up2_taps(h)
        r = torch.zeros(x.shape[0], x.shape[1], h, x.shape[3], dtype=D)
        r.index_add_(2, lo, x * (1 - w)[None, None, :, None])
        r.index_add_(2, hi, x * w[None, None, :, None])
        r = r.transpose(2, 3)
        wd = r.shape[2] // 2
        lo, hi, w = _up2_taps(wd)
        q = torch.zeros(r.shape[0], r.shape[1], wd, r.shape[3], dtype=D)
        q.index_add_(2, lo, r * (1 - w)[None, None, :, None])
        q.index_add_(2, hi, r * w[None, None, :, None])
        return q.transpose(2, 3).contiguous()

    return one(g), one(g.abs()), 16


def xscale_forward(x, R, r_scale, dn, up):
    """x + r_scale R + pool2(dn) + up2(up): value, S and the largest number of terms of an entry."""
    out, S, n = _d(x) + r_scale * _d(R), _d(x).abs() + abs(r_scale) * _d(R).abs(), 2
    if dn is not None:
        out, S, n = out + pool2_forward(dn), S + pool2_forward(_d(dn).abs()), n + 4
    if up is not None:
        out, S, n = out + up2_forward(up), S + up2_forward(_d(up).abs()), n + 4
    return out, S, n


# -------------------------------------------------------------------------------------------------------------------------------------
# CorrBlock lookup (mgaa.hip / train_ops.hip):  corr[c = i*n + j][y][x] = P[e],  e = (y*Wf + x)*C + (y+j-r)*2 + (x+i-r)  inside the
# NCHW-contiguous product buffer P = x1f * x2f / sqrt(C) of one batch item, zero unless 0 <= x+i-r <= 1 and 0 <= y+j-r < C/2

def corr_lookup_reference(x1f, x2f, radius, g):
    """corr (B,n*n,H,Wf), gx1, gx2 (B,C,H,Wf): one product and one division per entry; gradient entries no (i, j) maps to are 0.0."""
    a, b, g = _d(x1f).contiguous(), _d(x2f).contiguous(), _d(g)
    B, C, H, Wf = a.shape
    n = 2 * radius + 1
    af, bf = a.reshape(B, -1), b.reshape(B, -1)
    norm = math.sqrt(float(C))
    corr = torch.zeros(B, n * n, H, Wf, dtype=D)
    ga, gb = torch.zeros_like(af), torch.zeros_like(bf)
    hit = torch.zeros(C * H * Wf, dtype=torch.long)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(Wf), indexing="ij")
    for i in range(n):
        for j in range(n):
            col, row = xs + i - radius, ys + j - radius
            ok = (col >= 0) & (col <= 1) & (row >= 0) & (row < C // 2)
            if not bool(ok.any()):
                continue
            e = ((ys * Wf + xs) * C + row * 2 + col)[ok]
            yy, xx = ys[ok], xs[ok]
            corr[:, i * n + j, yy, xx] = af[:, e] * bf[:, e] / norm
            gg = g[:, i * n + j, yy, xx] / norm
            ga[:, e] = gg * bf[:, e]
            gb[:, e] = gg * af[:, e]
            hit[e] += 1
    assert int(hit.max()) <= 1                                     # every source element is read by at most one (pixel, i, j)
    return dict(corr=corr, gx1=ga.reshape(B, C, H, Wf), gx2=gb.reshape(B, C, H, Wf), touched=(hit > 0).reshape(C, H, Wf))


# -------------------------------------------------------------------------------------------------------------------------------------
# Inputs of tests/test_train_blocks_gpu.py (f32, seeded CPU generator).  Three quantities must not sit near a kink in the f64
# reference - LeakyReLU at r + add, the bottleneck's t, divenh's hidden pre-activation - so that the kernel's f32 value is on the same
# side: entries within MARGIN are resampled, at most ROUNDS times; the builders return how many are left (the tests assert 0).

MARGIN, ROUNDS = 1e-3, 5

# (B, H, W): HW = 1, 255, 256, 257 with B = 1 and 3; B * ceil(HW / 256) = 28, 29, 32, 33, 36, 65 partial rows; HW = 16389 is past the
# 1024-block cap of the C = 64 apply kernels (16 float4 per pixel), HW = 32775 past that of C = 32 (8 per pixel)
EDGE_SHAPES = [(1, 1, 1), (3, 1, 1), (1, 15, 17), (3, 5, 51), (1, 8, 32), (3, 4, 64), (1, 1, 257), (3, 257, 1)]
ROW_SHAPES = [(4, 35, 51), (1, 67, 107), (4, 23, 89), (3, 15, 187), (3, 9, 313), (5, 7, 439)]
CAP64_SHAPE, CAP32_SHAPE = (1, 27, 607), (1, 75, 437)
RCB_SHAPES = EDGE_SHAPES + ROW_SHAPES + [CAP64_SHAPE]
DIVENH_CASES = [(64,) + s for s in RCB_SHAPES] + [(32,) + s for s in EDGE_SHAPES + ROW_SHAPES + [CAP32_SHAPE]]
RCB_STRESS_SHAPE = (3, 13, 23)                                     # 299 pixels: one full block and a partial one
RCB_STRESS = ("span40", "last_pixel", "levels")


def shape_seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % 2147483647
    return s


def rcb_inputs(B, H, W, stress=None, identity=False):
    """r, z, wmask, w1, w2, gout (f32) and the number of entries left inside the kink margin.
    stress: "span40" scales wmask until the logits span about +-40; "last_pixel" puts the largest logit of every image into the last
    pixel (the partial last block); "levels" shifts the logits of the images of the batch to -30, 0, +30.  identity: W1 = W2 = I, so
    that add = lrelu(ctx) and the pooled vector itself can be read back from the output."""
    C = 64
    g = torch.Generator().manual_seed(shape_seed(1, B, H, W, 0 if stress is None else 1 + RCB_STRESS.index(stress), identity))
    r = torch.randn(B, C, H, W, generator=g) * 0.7
    z = torch.randn(B, C, H, W, generator=g)
    wm = torch.randn(1, C, 1, 1, generator=g) * 0.3
    w1 = torch.eye(C).reshape(C, C, 1, 1) if identity else torch.randn(C, C, 1, 1, generator=g) * 0.2
    w2 = torch.eye(C).reshape(C, C, 1, 1) if identity else torch.randn(C, C, 1, 1, generator=g) * 0.2
    gout = torch.randn(B, C, H, W, generator=g)
    unit = (wm / (wm.double() ** 2).sum().float()).reshape(1, C, 1, 1)           # wmask . unit = 1
    if stress == "span40":
        lg = torch.einsum("c,bchw->bhw", wm.reshape(C).double(), r.double())
        wm = wm * float(40.0 / lg.abs().max())
    elif stress == "last_pixel":
        lg = torch.einsum("c,bchw->bhw", wm.reshape(C).double(), r.double())
        want = lg.reshape(B, -1).max(dim=1).values + 10.0
        r[:, :, H - 1, W - 1] += unit.reshape(1, C) * (want - lg[:, H - 1, W - 1]).float().reshape(B, 1)
    elif stress == "levels":
        r += unit * torch.linspace(-30.0, 30.0, B).reshape(B, 1, 1, 1)
    left = -1
    for rnd in range(ROUNDS + 1):
        f = rcb_tail_forward(r, z, wm, w1, w2, 0.2)
        bad_u = f["u"].abs() < MARGIN
        bad_t = f["t"][0].abs() < MARGIN
        left = int(bad_u.sum()) + int(bad_t.sum())
        if left == 0 or rnd == ROUNDS:
            break
        if bool(bad_t.any()):                                       # first the bottleneck (a new W1 row moves add everywhere)
            if identity:                                            # t = ctx: move the pooled vector by moving r itself
                r += torch.randn(B, C, 1, 1, generator=g) * 0.05 * bad_t.reshape(B, C, 1, 1)
            else:
                rows = bad_t.any(dim=0)
                w1[rows] = torch.randn(int(rows.sum()), C, 1, 1, generator=g) * 0.2
            continue
        # a new draw for r = u - add with |u| in [10, 20] margins: a small move, so that the pooled vector (and with it add and every
        # other entry's u) moves by far less than the margin; entries within two margins are redrawn for the same reason
        fix = f["u"].abs() < 2 * MARGIN
        k = int(fix.sum())
        sign = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        unew = (sign * MARGIN * (10.0 + 10.0 * torch.rand(k, generator=g))).double()
        r[fix] = (unew - f["add"][0][:, :, None, None].expand(B, C, H, W)[fix]).float()
    return dict(r=r, z=z, wmask=wm, w1=w1, w2=w2, gout=gout), left


def divenh_inputs(C, B, H, W):
    """f, sf, so, a, b, w1, w2, g1, g2 (f32) and the number of hidden pre-activations left inside the kink margin."""
    g = torch.Generator().manual_seed(shape_seed(2, C, B, H, W))
    f, sf, so = (torch.randn(B, C, H, W, generator=g) for _ in range(3))
    a = 1.0 + 0.3 * torch.randn(1, C, 1, 1, generator=g)
    b = 0.5 + 0.3 * torch.randn(1, C, 1, 1, generator=g)
    w1 = torch.randn(C // 16, C, 1, 1, generator=g) * 0.4
    w2 = torch.randn(C, C // 16, 1, 1, generator=g) * 0.4
    g1, g2 = (torch.randn(B, C, H, W, generator=g) for _ in range(2))
    left = -1
    for rnd in range(ROUNDS + 1):
        o = divenh_band_forward(f, sf, so, a, b, w1, w2)
        bad = (o["pre"][0].abs() < MARGIN) | (o["pre"][1].abs() < MARGIN)          # (B, C/16)
        left = int(bad.sum())
        if left == 0 or rnd == ROUNDS:
            break
        rows = bad.any(dim=0)
        w1[rows] = torch.randn(int(rows.sum()), C, 1, 1, generator=g) * 0.4
    return dict(f=f, sf=sf, so=so, a=a, b=b, w1=w1, w2=w2, g1=g1, g2=g2), left
