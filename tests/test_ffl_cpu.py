"""Focal frequency loss, host side: the torch restatement `ffl_reference` against a dense-DFT evaluation of the published formula, the
half-spectrum form the kernels compute (tests/ffl_cases.py) against the restatement and its autograd gradient, the identities the
device layout relies on (a batch is the mean of its samples, patch_factor the mean over the crops), the edge cases (zero-difference
plane, NaN), the argument errors, `charbonnier_ffl_loss` against the reference class's arithmetic, `fit`'s new keywords, and the error
bounds of tests/test_ffl_gpu.py applied to the restatement run in f32 (a bound the f32 restatement itself misses would be a wrong
derivation)."""
import inspect
import math

import pytest
import torch

import ffl_cases as K
from fcvsr_amd.train import charbonnier_ffl_loss, charbonnier_loss, ffl_reference, focal_frequency_loss
from fcvsr_amd.train.step import fit


def _dft(n):
    k = torch.arange(n, dtype=torch.float64)
    ang = -2.0 * math.pi * torch.outer(k, k) / n
    return torch.complex(torch.cos(ang), torch.sin(ang)) / math.sqrt(n)


def _dense(pred, target, alpha, loss_weight):
    """The formula plane by plane with DFT matrices (patch_factor 1): no torch.fft, no broadcasting tricks."""
    B, C, H, W = pred.shape
    Fh, Fw = _dft(H), _dft(W)
    total = 0.0
    for b in range(B):
        for c in range(C):
            D = Fh @ pred[b, c].to(torch.complex128) @ Fw.T - Fh @ target[b, c].to(torch.complex128) @ Fw.T
            m = D.abs() ** alpha
            mx = float(m.max())
            wgt = (m / mx).clamp(0.0, 1.0) if mx > 0 else torch.zeros_like(m)
            total += float((wgt * D.abs() ** 2).sum())
    return loss_weight * total / (B * C * H * W)


@pytest.mark.parametrize("shape", [(1, 1, 8, 6), (1, 3, 9, 7)])
@pytest.mark.parametrize("alpha", K.ALPHAS)
def test_restatement_equals_dense_dft_evaluation(shape, alpha):
    pred, target = K.make_pair(shape)
    got = float(ffl_reference(pred, target, alpha, 0.7))
    want = _dense(pred, target, alpha, 0.7)
    assert abs(got - want) <= 1e-13 * abs(want), (got, want)


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("alpha", K.ALPHAS)
def test_half_spectrum_form_equals_restatement_and_its_gradient(shape, alpha):
    pred, target = K.make_pair(shape)
    L, gp, gt = K.reference_loss_and_grad(ffl_reference, pred, target, alpha, 1.3)
    got = K.halfspec_loss(pred, target, alpha, 1.3)
    assert abs(float(got) - float(L)) <= 1e-13 * float(L), (float(got), float(L))
    g = K.halfspec_grad(pred, target, alpha, 1.3)
    scale = float(gp.abs().max())
    assert scale > 0
    assert float((g - gp).abs().max()) <= 1e-12 * scale
    assert float((g + gt).abs().max()) <= 1e-12 * scale
    # the attached form used for the loss bound is the same function of the spectrum
    U = K.spectrum(pred, target)
    att = K.attached_loss_of_spectrum(U, shape[2], shape[3], alpha, 1.3)
    assert abs(float(att) - float(L)) <= 1e-13 * float(L)


def test_half_spectrum_form_with_patches():
    pred, target = K.make_pair((4, 1, 16, 12))
    L, gp, _ = K.reference_loss_and_grad(ffl_reference, pred, target, 1.0, 1.0, 2)
    assert abs(float(K.halfspec_loss(pred, target, 1.0, 1.0, 2)) - float(L)) <= 1e-13 * float(L)
    assert float((K.halfspec_grad(pred, target, 1.0, 1.0, 2) - gp).abs().max()) <= 1e-12 * float(gp.abs().max())


def test_batch_is_the_mean_of_its_samples():
    pred, target = K.make_pair((2, 3, 16, 20))
    whole = float(ffl_reference(pred, target))
    parts = [float(ffl_reference(pred[b:b + 1], target[b:b + 1])) for b in range(2)]
    assert abs(whole - sum(parts) / 2) <= 1e-14 * whole


def test_patch_factor_is_the_mean_over_the_crops():
    pred, target = K.make_pair((4, 1, 16, 12))
    whole = float(ffl_reference(pred, target, patch_factor=2))
    crops = [float(ffl_reference(pred[:, :, i * 8:(i + 1) * 8, j * 6:(j + 1) * 6], target[:, :, i * 8:(i + 1) * 8, j * 6:(j + 1) * 6]))
             for i in range(2) for j in range(2)]
    assert abs(whole - sum(crops) / 4) <= 1e-14 * whole
    assert abs(whole - float(ffl_reference(pred, target))) > 1e-6 * whole          # and it is not the unpatched loss


def test_zero_difference_plane_gives_finite_loss_and_gradient():
    pred, target = K.make_pair((3, 1, 32, 32))
    assert torch.equal(pred[1], target[1])
    L, gp, gt = K.reference_loss_and_grad(ffl_reference, pred, target)
    assert math.isfinite(float(L)) and float(L) > 0
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gt).all())
    assert float(gp[1].abs().max()) == 0.0 and float(gp[0].abs().max()) > 0
    same = pred.clone().requires_grad_(True)
    Z = ffl_reference(same, pred.clone())
    Z.backward()
    assert float(Z.detach()) == 0.0 and float(same.grad.abs().max()) == 0.0


def test_nan_input_gives_nan_loss():
    pred, target = K.make_pair((2, 1, 12, 10))
    pred[1, 0, 3, 4] = float("nan")
    assert math.isnan(float(ffl_reference(pred, target)))
    assert math.isnan(float(focal_frequency_loss(pred.float(), target.float())))


def test_value_errors():
    x = torch.rand(2, 1, 12, 10)
    for fn in (ffl_reference, focal_frequency_loss):
        with pytest.raises(ValueError):
            fn(x[0], x[0])                                   # not 4-D
        with pytest.raises(ValueError):
            fn(x, x[:, :, :8])                               # shape mismatch
        with pytest.raises(ValueError):
            fn(x, x, alpha=0.0)
        with pytest.raises(ValueError):
            fn(x, x, alpha=-1.0)
        with pytest.raises(ValueError):
            fn(x, x, patch_factor=4)                         # divides 12, not 10
        with pytest.raises(ValueError):
            fn(x, x, patch_factor=0)
        assert float(fn(x, x + 0.1, patch_factor=2)) > 0
    with pytest.raises(ValueError):
        charbonnier_ffl_loss(x, x[:, :, :8])


def test_cpu_tensors_take_the_restatement():
    pred, target = K.make_pair((2, 3, 16, 20), dtype=torch.float32)
    p = pred.clone().requires_grad_(True)
    L = focal_frequency_loss(p, target, alpha=2.0, loss_weight=0.5, patch_factor=2)
    L.backward()
    q = pred.clone().requires_grad_(True)
    R = ffl_reference(q, target, 2.0, 0.5, 2)
    R.backward()
    assert torch.equal(L, R) and torch.equal(p.grad, q.grad)


def test_charbonnier_ffl_equals_the_reference_class_arithmetic():
    """Charbonnier_FFL_Loss.forward line by line (eps 1e-6, FFL(loss_weight=1.0, alpha=1.0) on the inputs with a leading axis added: the
    reference passes one (C,H,W) sample; FFL works plane by plane and averages, so the leading axis changes nothing)."""
    X, Y = K.make_pair((1, 3, 9, 7))
    X, Y = X[0], Y[0]
    eps = 1e-6
    diff = torch.add(X, -Y)
    error = torch.sqrt(diff * diff + eps)
    cb_loss = torch.mean(error)
    ffl_loss = ffl_reference(X.unsqueeze(0), Y.unsqueeze(0), alpha=1.0, loss_weight=1.0)
    want = cb_loss + ffl_loss
    got = charbonnier_ffl_loss(X.unsqueeze(0), Y.unsqueeze(0))
    assert float(got) == float(want)
    # a batch: both terms are means over the samples
    P, T = K.make_pair((2, 3, 16, 20))
    per = [float(charbonnier_ffl_loss(P[b:b + 1], T[b:b + 1])) for b in range(2)]
    assert abs(float(charbonnier_ffl_loss(P, T)) - sum(per) / 2) <= 1e-14 * sum(per)
    d = inspect.signature(charbonnier_ffl_loss).parameters
    assert (d["eps"].default, d["ffl_weight"].default, d["alpha"].default) == (1e-6, 1.0, 1.0)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, x):                                    # (b, 7, 1, h, w) -> (b, 1, 4h, 4w)
        return torch.nn.functional.interpolate(self.conv(x[:, 3]), scale_factor=4, mode="nearest")


def _fit(**kw):
    torch.manual_seed(5)
    net = _Net()
    g = torch.Generator().manual_seed(11)
    data = [{"lr_imgs": torch.rand(2, 1, 7, 4, 4, generator=g), "hr_imgs": torch.rand(2, 1, 1, 16, 16, generator=g)} for _ in range(2)]
    hist = fit(net, lambda e: iter(data), epochs=2, device="cpu", log=lambda m: None, **kw)
    return hist, [p.detach().clone() for p in net.parameters()]


def test_fit_keywords_default_to_the_old_behaviour():
    par = inspect.signature(fit).parameters
    assert par["loss_fn"].default is charbonnier_loss and par["reduce_op"].default == "sum"
    assert par["loss_fn"].kind is inspect.Parameter.KEYWORD_ONLY and par["reduce_op"].kind is inspect.Parameter.KEYWORD_ONLY
    h0, w0 = _fit()
    h1, w1 = _fit(loss_fn=charbonnier_loss, reduce_op="sum")
    assert h0 == h1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
    h2, w2 = _fit(loss_fn=charbonnier_ffl_loss, reduce_op="mean")
    assert all(math.isfinite(v) for v in h2) and h2 != h0
    assert not all(torch.equal(a, b) for a, b in zip(w0, w2))


@pytest.mark.parametrize("shape", K.SHAPES + [(4, 1, 128, 128)])
@pytest.mark.parametrize("alpha", K.ALPHAS)
def test_f32_restatement_stays_inside_the_device_bounds(shape, alpha):
    """The bounds tests/test_ffl_gpu.py holds the kernels to, applied to torch's own f32 evaluation of the restatement."""
    pred, target = K.make_pair(shape)
    L, gp, _ = K.reference_loss_and_grad(ffl_reference, pred, target, alpha, 1.0)
    lb, gb = K.bounds(pred, target, alpha, 1.0)
    p32 = pred.float().requires_grad_(True)
    L32 = ffl_reference(p32, target.float(), alpha, 1.0)
    L32.backward()
    assert abs(float(L32.detach()) - float(L)) <= lb, (abs(float(L32.detach()) - float(L)) / lb)
    err = float((p32.grad.double() - gp).abs().max())
    assert err <= gb, err / gb
    # far from vacuous: a structural mistake (a column weight, a factor 2, a plane in the wrong place) is an error of order one.  The
    # gradient bound assumes all N spectrum errors add coherently, so against the gradient of random data it grows like sqrt(N).
    assert lb < 1e-3 * float(L) and gb < 0.05 * float(gp.abs().max())
