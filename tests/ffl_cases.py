"""Shared by tests/test_ffl_cpu.py and tests/test_ffl_gpu.py: the half-spectrum form of the focal frequency loss that csrc/ffl.hip
computes, written in torch f64, the test shapes, and the error bounds of the device path.

Half-spectrum form.  Per plane (batch x patch x channel) with d = pred - target, N = h w, U = rfft2(d) unnormalised on (h, Wf = w//2+1),
cw = 1 on the columns kx = 0 and kx = w/2 (even w only) and 2 elsewhere, u = |U| / sqrt(N):
    wgt = u^alpha / max_k u^alpha  (0 where the max is 0)
    loss = loss_weight / (P N) * sum_planes sum_k cw_k wgt_k u_k^2
    grad_pred = 2 loss_weight / (P N) * c2r(wgt * U),  c2r = irfft2 with its 1/N;   grad_target = -grad_pred

Bounds (eps = 3e-6 is the per-entry bound tests/test_fft_paths_gpu.py holds every real or imaginary part of a spectrum to, relative to
the tensor's max; M_U = max |U| over the call, in f64):
  loss: |dL| <= sum_k (|dL/dRe U_k| + |dL/dIm U_k|) * eps M_U to first order, with the derivative of the form whose weights and plane max
        are ATTACHED (the computed weights move with the computed spectrum); a factor 2 for the second-order terms and the f32 rounding
        of pred - target; plus tau(P h Wf) * L for the f32 sum of P h Wf non-negative terms (tests/tolerance.py).
  gradient: every entry of wgt * U is off by at most (1 + 2 alpha) eps M_U (U itself by eps M_U, the weight u^alpha / max by a relative
        2 alpha eps M_U / |U| at worst, times |U| <= M_U); the inverse transform sums N of them with weight 1/N, coherently at worst, and
        adds its own eps * max|c2r(wgt * U)|; times the scale 2 loss_weight / (P N) and the same factor 2."""
import math

import torch

from tolerance import tau

EPS_FFT = 3e-6

# (B, C, H, W); the last one gets sample 1's prediction set equal to its target (a plane with zero difference)
SHAPES = [(1, 1, 8, 6), (2, 1, 12, 10), (1, 3, 9, 7), (2, 3, 16, 20), (3, 1, 32, 32)]
ALPHAS = [1.0, 2.0, 0.5]


def make_pair(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(1000 + seed + sum(shape))
    pred = torch.rand(shape, generator=g, dtype=torch.float64)
    target = torch.rand(shape, generator=g, dtype=torch.float64)
    if shape == (3, 1, 32, 32):
        pred[1] = target[1]
    # values that are exact in f32, so that every precision starts from the same numbers
    return pred.float().to(dtype), target.float().to(dtype)


def patches(x, f):
    h, w = x.shape[2] // f, x.shape[3] // f
    return torch.stack([x[:, :, i * h:(i + 1) * h, j * w:(j + 1) * w] for i in range(f) for j in range(f)], 1)


def col_weights(w, dtype=torch.float64):
    cw = torch.full((w // 2 + 1,), 2.0, dtype=dtype)
    cw[0] = 1.0
    if w % 2 == 0:
        cw[-1] = 1.0
    return cw


def spectrum(pred, target, f=1):
    """U (B, f*f, C, h, Wf) complex128, unnormalised."""
    return torch.fft.rfft2(patches(pred.double() - target.double(), f))


def weights_of(U, h, w, alpha):
    u = U.abs() / math.sqrt(h * w)
    m = u ** alpha
    mx = m.amax(dim=(-2, -1), keepdim=True)
    return torch.where(mx > 0, m / torch.where(mx > 0, mx, torch.ones_like(mx)), torch.zeros_like(m))


def halfspec_loss(pred, target, alpha=1.0, loss_weight=1.0, f=1):
    h, w = pred.shape[2] // f, pred.shape[3] // f
    U = spectrum(pred, target, f)
    P, N = U[..., 0, 0].numel(), h * w
    u2 = (U.real ** 2 + U.imag ** 2) / N
    return loss_weight / (P * N) * (col_weights(w) * weights_of(U, h, w, alpha) * u2).sum()


def unpatch(y, f):
    """(B, f*f, C, h, w) -> (B, C, f*h, f*w)"""
    B, _, C, h, w = y.shape
    return y.reshape(B, f, f, C, h, w).permute(0, 3, 1, 4, 2, 5).reshape(B, C, f * h, f * w)


def halfspec_grad(pred, target, alpha=1.0, loss_weight=1.0, f=1):
    """grad_pred of the formula above (no autograd)."""
    h, w = pred.shape[2] // f, pred.shape[3] // f
    U = spectrum(pred, target, f)
    P, N = U[..., 0, 0].numel(), h * w
    r = torch.fft.irfft2(weights_of(U, h, w, alpha) * U, s=(h, w))
    return unpatch(2.0 * loss_weight / (P * N) * r, f)


def attached_loss_of_spectrum(U, h, w, alpha, loss_weight):
    """The half-spectrum loss as a function of U with weight and plane max attached: c * sum cw * u^(2 + alpha) / max u^alpha, written
    through s = |U|^2 with exponents whose derivatives are finite at s = 0."""
    P, N = U[..., 0, 0].numel(), h * w
    s = (U.real ** 2 + U.imag ** 2) / N
    smax = s.amax(dim=(-2, -1), keepdim=True)
    ok = smax > 0
    mx = torch.where(ok, smax, torch.ones_like(smax)) ** (alpha / 2)
    terms = torch.where(ok, s ** (1.0 + alpha / 2) / mx, torch.zeros_like(s))
    return loss_weight / (P * N) * (col_weights(w) * terms).sum()


def bounds(pred, target, alpha=1.0, loss_weight=1.0, f=1):
    """(loss bound, gradient bound per element) of the device path for these f64 inputs."""
    h, w = pred.shape[2] // f, pred.shape[3] // f
    U = spectrum(pred, target, f).detach().requires_grad_(True)
    P, N = U[..., 0, 0].numel(), h * w
    L = attached_loss_of_spectrum(U, h, w, alpha, loss_weight)
    (g,) = torch.autograd.grad(L, U)
    norm1 = float(g.real.abs().sum() + g.imag.abs().sum())
    Ud = U.detach()
    M_U = float(Ud.abs().max())
    loss_bound = 2.0 * EPS_FFT * M_U * norm1 + tau(P * h * (w // 2 + 1)) * float(L.detach())
    r = torch.fft.irfft2(weights_of(Ud, h, w, alpha) * Ud, s=(h, w))
    grad_bound = 2.0 * (2.0 * loss_weight / (P * N)) * EPS_FFT * ((1.0 + 2.0 * alpha) * M_U + float(r.abs().max()))
    return loss_bound, grad_bound


def reference_loss_and_grad(ffl_reference, pred, target, alpha=1.0, loss_weight=1.0, f=1):
    """f64 restatement and its autograd gradients (pred, target)."""
    p = pred.double().detach().requires_grad_(True)
    t = target.double().detach().requires_grad_(True)
    L = ffl_reference(p, t, alpha, loss_weight, f)
    gp, gt = torch.autograd.grad(L, (p, t))
    return L.detach(), gp, gt
