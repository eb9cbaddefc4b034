"""Deterministic training mode, whole step: `TrainStep(model, deterministic=True)` repeats bit for bit - run against run, replay
against replay and eager against hipGraph replay - on both gradient goldens in both train precisions; the default mode is untouched
and the torch routes with an order-dependent backward are refused."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu

GOLDENS = ["grad_Sreduced_24x16", "grad_S_16x20"]


def _load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _model_for(meta, precision="f32"):
    from helpers import get_ctor, weights_for
    m = get_ctor(meta["ctor"])(**meta["kwargs"])
    m.load_state_dict(weights_for(meta), strict=True)
    m.train_precision = precision
    return m.cuda()


def _three_steps(z, meta, precision, use_graph, deterministic=True):
    """A fresh model and TrainStep from the fixture's weights: (losses of 3 steps, flat gradient after step 1, final parameters, names)"""
    from fcvsr_amd.train import TrainStep
    x, t = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()
    model = _model_for(meta, precision)
    step = TrainStep(model, lr=1e-4, weight_decay=1e-5, use_graph=use_graph, deterministic=deterministic)
    losses = [step(x, t)]
    g1 = step.allreduce.flat.clone()
    losses += [step(x, t) for _ in range(2)]
    torch.cuda.synchronize()
    return losses, g1, [p.detach().clone() for p in step.allreduce.params], step


def _first_difference(step, a, b):
    """name of the first parameter whose slice of the flat gradient buffer differs (names the operator that is not repeatable)"""
    for name, u, v in zip(step.names, a.split(step.allreduce.sizes), b.split(step.allreduce.sizes)):
        if not torch.equal(u, v):
            return f"{name}: max |diff| {float((u - v).abs().max()):.3e} of {float(u.abs().max()):.3e}"
    return "none"


def _assert_same(run_a, run_b, what):
    (la, ga, pa, step), (lb, gb, pb, _) = run_a, run_b
    assert torch.equal(ga, gb), f"{what}: gradients of step 1 differ, first at {_first_difference(step, ga, gb)}"
    assert la == lb, (what, la, lb)
    for name, u, v in zip(step.names, pa, pb):
        assert torch.equal(u, v), f"{what}: parameter {name} differs after 3 steps"


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("golden", GOLDENS)
def test_two_eager_runs_are_bit_identical(golden, precision):
    z, meta = _load(golden)
    _assert_same(_three_steps(z, meta, precision, False), _three_steps(z, meta, precision, False), "eager vs eager")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("golden", GOLDENS)
def test_two_hipgraph_runs_are_bit_identical(golden, precision):
    z, meta = _load(golden)
    _assert_same(_three_steps(z, meta, precision, True), _three_steps(z, meta, precision, True), "hipGraph vs hipGraph")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("golden", GOLDENS)
def test_hipgraph_replay_is_bit_identical_to_eager(golden, precision):
    """Same kernels, same order: with no float atomics on the path the replayed step must give the eager step's bits."""
    z, meta = _load(golden)
    _assert_same(_three_steps(z, meta, precision, False), _three_steps(z, meta, precision, True), "eager vs hipGraph")


@pytest.mark.parametrize("golden", GOLDENS)
def test_deterministic_mode_changes_a_summation_order_only(golden):
    """Exact-f32 mode: the loss of step 1 within 1e-5 relative of the golden's, the gradient within 1e-5 of its largest entry of the
    default mode's (the two numbers of test_train_step_hipgraph_replay_equals_eager)."""
    z, meta = _load(golden)
    ld, gd, _, _ = _three_steps(z, meta, "f32", False, deterministic=True)
    la, ga, _, _ = _three_steps(z, meta, "f32", False, deterministic=False)
    assert abs(ld[0] - float(z["loss"])) <= 1e-5 * float(z["loss"])
    assert float((gd - ga).abs().max()) <= 1e-5 * float(ga.abs().max())
    assert abs(la[0] - float(z["loss"])) <= 1e-5 * float(z["loss"])


class _CountingLib:
    """hip.lib() wrapper that counts calls per entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("fcvsr_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_default_mode_is_untouched(monkeypatch):
    """TrainStep(model) with no flag leaves model.train_deterministic False and runs the scatter form; deterministic=True runs the
    atomic-free form only; a TrainStep keeps one captured graph per mode."""
    from fcvsr_amd import hip
    from fcvsr_amd.train import TrainStep
    z, meta = _load("grad_Sreduced_24x16")
    x, t = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()
    model = _model_for(meta)
    counting = _CountingLib(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: counting)
    step = TrainStep(model)
    assert model.train_deterministic is False
    step(x, t)
    n_iac = counting.calls.get("fcvsr_iac_bwd_warp", 0)
    assert n_iac > 0 and "fcvsr_iac_bwd_warp_det" not in counting.calls
    assert counting.calls["fcvsr_iac_bwd_sac"] == n_iac
    counting.calls.clear()
    step = TrainStep(model, deterministic=True)
    assert model.train_deterministic is True
    step(x, t)
    assert counting.calls.get("fcvsr_iac_bwd_warp_det", 0) == n_iac and "fcvsr_iac_bwd_warp" not in counting.calls
    monkeypatch.undo()
    # the captured graph has the kernel choice baked in: the flag is part of the key
    step = TrainStep(model, use_graph=True, deterministic=False)
    step(x, t)
    model.train_deterministic = True
    step(x, t)
    assert len(step._graphs) == 2 and sorted(k[-1] for k in step._graphs) == [False, True]


def _tiny_input(B, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 7, 1, H, W, generator=g).cuda()


def test_routes_with_an_order_dependent_backward_are_refused():
    """deterministic=True raises ValueError naming the cause on the routes that leave the HIP blocks - fused_blocks=False, a feature
    width outside {32, 64}, odd sizes on the first two pyramid levels - and the first two still run without the flag (the third cannot
    run on any input, see below)."""
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.train import graph as G
    from fcvsr_amd.train.graph import forward_train
    # 1. fused_blocks=False (smallest 32-feature model)
    m = GShiftNet_S(n_features=32, ACNum=2, Freq_Inv=2, SCGroupN=1).cuda().train()
    p = m.state_dict(keep_vars=True)
    x = _tiny_input(1, 16, 20)
    with pytest.raises(ValueError, match="fused_blocks"):
        forward_train(p, x, fused_blocks=False, deterministic=True)
    y = forward_train(p, x, fused_blocks=False)
    y.sum().backward()
    assert y.shape == (1, 1, 64, 80)
    forward_train(p, x, deterministic=True).sum().backward()                          # the HIP route of the same model runs
    # 2. a feature width of 16, through the drop-in module's attribute
    m16 = GShiftNet_S(n_features=16, ACNum=2, Freq_Inv=2, SCGroupN=1).cuda().train()
    m16(x).sum().backward()
    m16.train_deterministic = True
    with pytest.raises(ValueError, match="width"):
        m16(x)
    # 3. odd sizes on the first two pyramid levels.  forward_train accepts only multiples of 4, which makes both levels even, so the
    #    route is entered where it branches off: BlockRCB on an 18x20 level whose second level is 9x10.  Without the flag this route
    #    cannot complete on ANY odd input (F.interpolate's x2 result never has the odd size of the level it is added to), so only the
    #    refusal is asserted here; the torch cross-scale sum itself ran under 1. (fused_blocks=False, even sizes)
    key = "recorb1.body.0.body.0"
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(1, 32, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last) for h, w in ((18, 20), (9, 10), (5, 5))]
    with pytest.raises(ValueError, match="pyramid"):
        G._block_rcb(G._Ctx(p, "f32", deterministic=True), key, xs)
    even = [torch.randn(1, 32, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last) for h, w in ((16, 20), (8, 10), (4, 5))]
    out = G._block_rcb(G._Ctx(p, "f32", deterministic=True), key, even)                # even sizes: the HIP cross-scale sum, no refusal
    assert [tuple(o.shape[2:]) for o in out] == [(16, 20), (8, 10), (4, 5)]
    torch.cuda.synchronize()
