"""Losses of the reference's two training loops."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable


def charbonnier_loss(x: torch.Tensor, y: torch.Tensor, mean_res: bool = False, eps: float = 1e-4) -> torch.Tensor:
    """sum(sqrt((x - y)^2 + eps)), eps = 1e-4 (reference CVSR_train/opt/loss.py:20-31; `mean_res` averages the difference
    per sample first).  A SUM over all elements: gradients scale with the batch, so data-parallel ranks all-reduce with SUM."""
    diff = x - y
    if mean_res:
        diff = diff.reshape(x.shape[0], -1).mean(1, keepdim=True)
    return torch.sum(torch.sqrt(diff * diff + eps))


def charbonnier_loss_mmedit(pred: torch.Tensor, target: torch.Tensor, loss_weight: float = 1.0, eps: float = 1e-12,
                            reduction: str = "mean") -> torch.Tensor:
    """mmedit's CharbonnierLoss (reference mmedit_train/mmedit/models/losses/pixelwise_loss.py:41-51, :120-160):
    sqrt((pred - target)^2 + eps), eps = 1e-12, mean by default (data-parallel ranks average)."""
    v = torch.sqrt((pred - target) ** 2 + eps)
    if reduction == "mean":
        v = v.mean()
    elif reduction == "sum":
        v = v.sum()
    elif reduction != "none":
        raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['none', 'mean', 'sum']")
    return loss_weight * v


def _check_ffl_args(pred: torch.Tensor, target: torch.Tensor, alpha: float, patch_factor: int) -> None:
    if pred.dim() != 4 or target.dim() != 4:
        raise ValueError(f"focal frequency loss takes (B,C,H,W) tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if not alpha > 0:
        raise ValueError(f"alpha must be positive, got {alpha}")
    f = patch_factor
    if int(f) != f or f < 1 or pred.shape[2] % f or pred.shape[3] % f:
        raise ValueError(f"patch_factor {patch_factor} does not divide H = {pred.shape[2]} and W = {pred.shape[3]}")


def ffl_reference(pred: torch.Tensor, target: torch.Tensor, alpha: float = 1.0, loss_weight: float = 1.0,
                  patch_factor: int = 1) -> torch.Tensor:
    """The focal frequency loss (Jiang et al., ICCV 2021) with its default options, restated in plain torch ops from the published
    algorithm; the reference's `FFL(loss_weight=1.0, alpha=1.0)` (CVSR_train/opt/deep_learning.py:192-220) is the
    `FocalFrequencyLoss` of the `focal_frequency_loss` package, which this project does not vendor or import: that this restatement
    agrees with the package was established by reading it, not by running it.  Any device, any float dtype (16-bit inputs are
    transformed in f32).

        y(x) = the f x f patch crops of x stacked on a new axis 1: (B, f*f, C, h, w)
        D    = fft2(y(pred), norm="ortho") - fft2(y(target), norm="ortho")
        wgt  = |D|^alpha / (its max over each (h, w) plane), NaN -> 0, clamped to [0, 1], detached
        loss = loss_weight * mean(wgt * |D|^2)

    The package's log_matrix, batch_matrix, ave_spectrum and external `matrix` options are not parameters here."""
    _check_ffl_args(pred, target, alpha, patch_factor)
    f = int(patch_factor)
    h, w = pred.shape[2] // f, pred.shape[3] // f

    def spectrum(x):
        if x.dtype not in (torch.float32, torch.float64):            # torch.fft has no 16-bit transforms on every device: f32 then
            x = x.float()
        y = torch.stack([x[:, :, i * h:(i + 1) * h, j * w:(j + 1) * w] for i in range(f) for j in range(f)], 1)
        return torch.fft.fft2(y, norm="ortho")

    D = spectrum(pred) - spectrum(target)
    d2 = D.real ** 2 + D.imag ** 2
    m = torch.sqrt(d2) ** alpha
    wgt = m / m.amax(dim=(-2, -1), keepdim=True)
    wgt = torch.where(torch.isnan(wgt), torch.zeros_like(wgt), wgt).clamp(0.0, 1.0).detach()
    return loss_weight * torch.mean(wgt * d2)


class _FocalFrequencyFn(torch.autograd.Function):
    """The loss on the library's kernels (csrc/ffl.hip has the formulas): pred - target as ONE NHWC image whose channels are the
    B*f*f*C planes -> fcvsr_rfft2 (half spectrum) -> per-plane max, weights and the fixed-order sum; backward: fcvsr_irfft2 of the
    weighted spectrum the forward left, scaled and scattered back to NCHW.  No host synchronisation: safe under stream capture."""

    @staticmethod
    def forward(ctx, pred, target, alpha, loss_weight, f):
        from .. import hip
        from .fft import _rfft2
        B, Cn, H, W = pred.shape
        h, w = H // f, W // f
        P = B * f * f * Cn
        Pp = P + (P & 1)                                 # an even channel count keeps the FFT kernels on their pair / vector paths
        p, t = pred.float().contiguous(), target.float().contiguous()
        dev = p.device
        lib, st = hip.lib(), hip.stream_ptr()
        d = torch.empty((1, h, w, Pp), dtype=torch.float32, device=dev)
        hip.check(lib.fcvsr_ffl_diff(p.data_ptr(), t.data_ptr(), B, Cn, H, W, f, d.data_ptr(), Pp, st), "fcvsr_ffl_diff")
        try:
            spec = _rfft2(d, Pp, 0, Pp)                  # (1, h, Wf, 2 Pp): imaginary parts at 0.., real parts at Pp..
        except hip.HipError as e:
            if "too long for LDS" in str(e) or "too many factors" in str(e):
                raise ValueError(str(e)) from e
            raise
        n_ws = lib.fcvsr_ffl_workspace_elems(h, w, P)
        ws = torch.empty((n_ws,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        hip.check(lib.fcvsr_ffl_weight(spec.data_ptr(), 2 * Pp, 0, Pp, h, w, P, float(alpha), float(loss_weight), ws.data_ptr(), n_ws,
                                       loss.data_ptr(), st), "fcvsr_ffl_weight")
        ctx.save_for_backward(spec)
        ctx.dims = (B, Cn, H, W, f, Pp, float(loss_weight), pred.dtype, target.dtype)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .. import hip
        from .fft import _irfft2
        (spec,) = ctx.saved_tensors
        B, Cn, H, W, f, Pp, loss_weight, pdt, tdt = ctx.dims
        r = _irfft2(spec, Pp, 0, Pp, H // f, W // f)     # out of place: the saved spectrum stays intact
        gup = g.float().contiguous()
        gp = torch.empty((B, Cn, H, W), dtype=torch.float32, device=spec.device) if ctx.needs_input_grad[0] else None
        gt = torch.empty((B, Cn, H, W), dtype=torch.float32, device=spec.device) if ctx.needs_input_grad[1] else None
        hip.check(hip.lib().fcvsr_ffl_grad(r.data_ptr(), Pp, gup.data_ptr(), loss_weight, B, Cn, H, W, f, hip.ptr(gp), hip.ptr(gt),
                                           hip.stream_ptr()), "fcvsr_ffl_grad")
        return (None if gp is None else gp.to(pdt)), (None if gt is None else gt.to(tdt)), None, None, None


def focal_frequency_loss(pred: torch.Tensor, target: torch.Tensor, alpha: float = 1.0, loss_weight: float = 1.0,
                         patch_factor: int = 1) -> torch.Tensor:
    """`ffl_reference` on the HIP kernels for device tensors (f32 arithmetic, a f32 device scalar; sums in a fixed order, so two calls
    agree bit for bit; no host synchronisation, so it can be captured in a hipGraph after one eager call of the shape), and
    `ffl_reference` itself for CPU tensors.  A mean-type loss: a batch's value is the mean of its samples' values.
    ValueError: inputs that are not 4-D or differ in shape, alpha <= 0, a patch_factor that does not divide H and W, or a patch row /
    column too long for the FFT kernels (the library's message is passed on)."""
    _check_ffl_args(pred, target, alpha, patch_factor)
    if not pred.is_cuda:
        return ffl_reference(pred, target, alpha, loss_weight, patch_factor)
    if target.device != pred.device:
        raise ValueError(f"pred is on {pred.device}, target on {target.device}")
    return _FocalFrequencyFn.apply(pred, target, float(alpha), float(loss_weight), int(patch_factor))


def charbonnier_ffl_loss(pred: torch.Tensor, target: torch.Tensor, eps: float = 1e-6, ffl_weight: float = 1.0,
                         alpha: float = 1.0) -> torch.Tensor:
    """The reference's Charbonnier_FFL_Loss (CVSR_train/opt/deep_learning.py:206-220): mean(sqrt((pred - target)^2 + eps)), eps = 1e-6,
    plus FFL(loss_weight=ffl_weight, alpha=alpha).  Both terms are means: data-parallel ranks average their gradients
    (`reduce_op="mean"`, as with `charbonnier_loss_mmedit`)."""
    _check_ffl_args(pred, target, alpha, 1)
    diff = pred - target
    return torch.mean(torch.sqrt(diff * diff + eps)) + focal_frequency_loss(pred, target, alpha=alpha, loss_weight=ffl_weight)
