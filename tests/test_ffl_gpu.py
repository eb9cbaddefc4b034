"""Focal frequency loss on the device (csrc/ffl.hip around fcvsr_rfft2 / fcvsr_irfft2) against the f64 restatement `ffl_reference`
and its autograd gradient, inside the bounds derived in tests/ffl_cases.py; bit-repeatability, replay from a captured graph,
grad_target == -grad_pred, and that odd plane counts and patch_factor = 2 run on the HIP path.  Run with -s to see the error ratios."""
import ctypes

import pytest
import torch

import ffl_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the shapes of the CPU tests plus an even plane count on a two-stage FFT length (the pair path of the row kernels)
SHAPES = K.SHAPES + [(4, 1, 128, 128)]


def _fns():
    from fcvsr_amd.train import ffl_reference, focal_frequency_loss
    return ffl_reference, focal_frequency_loss


_REF = {}


def _reference(shape, alpha, loss_weight, f):
    """f64 loss, gradients and bounds of a case, computed once."""
    key = (shape, alpha, loss_weight, f)
    if key not in _REF:
        pred, target = K.make_pair(shape)
        L, gp, gt = K.reference_loss_and_grad(_fns()[0], pred, target, alpha, loss_weight, f)
        _REF[key] = (pred, target, float(L), gp, gt) + K.bounds(pred, target, alpha, loss_weight, f)
    return _REF[key]


def _device_call(pred, target, alpha, loss_weight, f):
    p = pred.float().to(DEV).requires_grad_(True)
    t = target.float().to(DEV).requires_grad_(True)
    L = _fns()[1](p, t, alpha=alpha, loss_weight=loss_weight, patch_factor=f)
    L.backward()
    return L.detach(), p.grad, t.grad


def _fft_path():
    from fcvsr_amd import hip
    return hip.lib().fcvsr_last_fft_path().decode()


def _reset_fft_path():
    """Leave another transform's string in fcvsr_last_fft_path(): a 64 x 64 image of two channels, a size no case here transforms."""
    from fcvsr_amd import hip
    x = torch.zeros(1, 64, 64, 2, device=DEV)
    spec = torch.empty(1, 64, 33, 4, device=DEV)
    v = hip.view(x)
    hip.check(hip.lib().fcvsr_rfft2(ctypes.byref(v), 1, 64, 64, 2, spec.data_ptr(), 4, 0, 2, hip.stream_ptr()), "fcvsr_rfft2")
    return _fft_path()


def _check(shape, alpha, loss_weight, f):
    pred, target, L, gp, gt, lb, gb = _reference(shape, alpha, loss_weight, f)
    before = _reset_fft_path()
    got, ggp, ggt = _device_call(pred, target, alpha, loss_weight, f)
    after = _fft_path()
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    le = abs(float(got) - L)
    ge = float((ggp.double().cpu() - gp).abs().max())
    print(f"\n  ffl {shape} alpha={alpha} f={f}: loss err/bound {le / lb:.3g}  grad err/bound {ge / gb:.3g}  [{after}]")
    assert le <= lb, (le, lb)
    assert ge <= gb, (ge, gb)
    assert torch.equal(ggt, -ggp)                                   # bit for bit
    assert float((ggt.double().cpu() - gt).abs().max()) <= gb
    assert after != before and after.startswith("rfft_rows"), (before, after)      # the forward transform of this call ran in the library
    return got, ggp, ggt


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("alpha", K.ALPHAS)
def test_loss_and_gradient_against_f64_restatement(shape, alpha):
    _check(shape, alpha, 1.0, 1)


def test_odd_plane_count_takes_the_hip_path():
    """P = 3 planes, padded to four channels with a zero plane the mean does not count (the shapes above include P = 1 and 3 too);
    here with a loss weight, on every alpha path."""
    for alpha in K.ALPHAS:
        _check((1, 3, 9, 7), alpha, 0.7, 1)


def test_patch_factor_two_takes_the_hip_path():
    _check((4, 1, 16, 12), 1.0, 1.0, 2)                              # 16 planes of 8 x 6
    _check((1, 3, 18, 14), 1.0, 1.3, 2)                              # 12 planes of 9 x 7: odd patch sides


def test_zero_difference_plane_is_exactly_zero():
    pred, target, *_ = _reference((3, 1, 32, 32), 1.0, 1.0, 1)
    got, gp, gt = _device_call(pred, target, 1.0, 1.0, 1)
    assert bool(torch.isfinite(got)) and bool(torch.isfinite(gp).all())
    assert float(gp[1].abs().max()) == 0.0 and float(gp[0].abs().max()) > 0
    z, gz, _ = _device_call(pred, pred, 1.0, 1.0, 1)
    assert float(z) == 0.0 and float(gz.abs().max()) == 0.0


def test_nan_input_gives_nan_loss():
    pred, target = K.make_pair((2, 1, 12, 10))
    pred[1, 0, 3, 4] = float("nan")
    got = _fns()[1](pred.float().to(DEV), target.float().to(DEV))
    assert bool(torch.isnan(got))


@pytest.mark.parametrize("shape,f", [((2, 3, 16, 20), 1), ((4, 1, 128, 128), 1), ((4, 1, 16, 12), 2)])
def test_two_calls_are_bit_equal(shape, f):
    pred, target = K.make_pair(shape)
    a = _device_call(pred, target, 1.0, 1.0, f)
    b = _device_call(pred, target, 1.0, 1.0, f)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_only_the_requested_gradients_are_returned():
    pred, target = K.make_pair((2, 3, 16, 20))
    _, gp, gt = _device_call(pred, target, 1.0, 1.0, 1)
    p = pred.float().to(DEV).requires_grad_(True)
    _fns()[1](p, target.float().to(DEV)).backward()
    assert torch.equal(p.grad, gp)
    t = target.float().to(DEV).requires_grad_(True)
    (2.0 * _fns()[1](pred.float().to(DEV), t)).backward()            # the upstream gradient is read on the device
    assert torch.equal(t.grad, 2.0 * gt)


def test_row_too_long_for_the_fft_kernels_is_a_value_error():
    x = torch.zeros(1, 1, 4, 16384, device=DEV)
    with pytest.raises(ValueError, match="fcvsr_rfft2"):
        _fns()[1](x, x)


@pytest.mark.parametrize("shape", [(2, 3, 16, 20), (4, 1, 128, 128)])
def test_graph_replay_equals_eager(shape):
    """forward + backward captured on static tensors after one eager warm-up call; the replay with NEW contents of the static inputs
    equals the eager call on those contents bit for bit."""
    ffl = _fns()[1]
    pred, target = K.make_pair(shape)
    pred2, target2 = K.make_pair(shape, seed=7)
    sp = pred.float().to(DEV).requires_grad_(True)
    st = target.float().to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ffl(sp, st).backward()                                       # eager warm-up: tables, attributes, allocator
    torch.cuda.current_stream().wait_stream(side)
    sp.grad = None
    st.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ffl(sp, st)
        gp, gt = torch.autograd.grad(loss, (sp, st))
    with torch.no_grad():
        sp.copy_(pred2.float())
        st.copy_(target2.float())
    graph.replay()
    torch.cuda.synchronize()
    want = _device_call(pred2, target2, 1.0, 1.0, 1)
    assert torch.equal(loss.detach(), want[0]) and torch.equal(gp, want[1]) and torch.equal(gt, want[2])
    assert float(want[0]) > 0


def test_charbonnier_ffl_loss_on_the_device():
    from fcvsr_amd.train import charbonnier_ffl_loss
    pred, target = K.make_pair((2, 3, 16, 20))
    p = pred.float().to(DEV).requires_grad_(True)
    got = charbonnier_ffl_loss(p, target.float().to(DEV))
    got.backward()
    q = pred.clone().requires_grad_(True)
    want = charbonnier_ffl_loss(q, target)                           # f64 on the CPU: the restatement
    want.backward()
    # the FFL term inside its bounds, the Charbonnier mean (n terms below 1, gradient entries below 1 / n) a few f32 roundings
    lb, gb = K.bounds(pred, target)
    assert abs(float(got.detach()) - float(want.detach())) <= lb + 2.0 ** -20 * float(want.detach())
    assert float((p.grad.double().cpu() - q.grad).abs().max()) <= gb + 2.0 ** -20 / pred.numel()


def test_fit_iters_with_charbonnier_ffl_deterministic_and_replayed():
    """fit_iters(..., loss_fn=charbonnier_ffl_loss, deterministic=True, use_graph=True) runs, and twice the same way."""
    import json
    import os

    import numpy as np

    from helpers import GOLDEN_DIR, get_ctor, weights_for
    from fcvsr_amd.train import DeviceClipSampler, charbonnier_ffl_loss, fit_iters
    z = np.load(os.path.join(GOLDEN_DIR, "grad_Sreduced_24x16.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    rs = np.random.RandomState(21)
    seqs = [(rs.randint(0, 256, size=(9, 1, 24, 28)).astype(np.uint8), rs.randint(0, 256, size=(9, 1, 96, 112)).astype(np.uint8))]

    def run():
        model = get_ctor(meta["ctor"])(**meta["kwargs"])
        model.load_state_dict(weights_for(meta), strict=True)
        sampler = DeviceClipSampler(seqs, batch=2, crop=16, seed=0, device=DEV)
        losses = fit_iters(model.cuda(), sampler, total_iters=3, device=DEV, lr=1e-4, loss_fn=charbonnier_ffl_loss, deterministic=True,
                           use_graph=True, log=lambda s: None)
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in model.parameters()]

    la, pa = run()
    lb, pb = run()
    assert len(la) == 3 and all(v == v and v > 0 for v in la)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb))
