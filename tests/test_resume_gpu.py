"""Resumable training on the device: with deterministic=True and `HipAdam`, a run stopped and continued from its saved state gives the
uninterrupted run's losses, weights and moments bit for bit - at the level of `TrainStep` and of `fit_iters` with its checkpoints -
in both train precisions, eager and replayed; the inference engine sees the weights `HipAdam` wrote; a torch.optim.Adam state loads
into `HipAdam`."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu

GOLDEN = "grad_Sreduced_24x16"
CASES = [("f32", False), ("f32", True), ("bf16", False), ("bf16", True)]
IDS = ["f32-eager", "f32-graph", "bf16-eager", "bf16-graph"]


def _load():
    z = np.load(os.path.join(GOLDEN_DIR, GOLDEN + ".npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _model(meta, precision="f32"):
    from helpers import get_ctor, weights_for
    m = get_ctor(meta["ctor"])(**meta["kwargs"])
    m.load_state_dict(weights_for(meta), strict=True)
    m.train_precision = precision
    return m.cuda()


def _batch(z):
    return torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["target"]).cuda()


def _hip_step(model, use_graph):
    from fcvsr_amd.train import TrainStep
    return TrainStep(model, lr=1e-4, weight_decay=1e-5, optimizer="hip", use_graph=use_graph, deterministic=True)


def _state(step):
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in step.allreduce.params], step.optimizer.exp_avg.clone(), step.optimizer.exp_avg_sq.clone())


@pytest.mark.parametrize("precision,use_graph", CASES, ids=IDS)
def test_train_step_resumes_bit_for_bit(precision, use_graph, tmp_path):
    """Four steps straight == two steps, state saved through torch.save, a fresh model and TrainStep, load, two more steps."""
    z, meta = _load()
    x, t = _batch(z)
    straight = _hip_step(_model(meta, precision), use_graph)
    want_losses = [straight(x, t) for _ in range(4)]
    want_p, want_m, want_v = _state(straight)

    model = _model(meta, precision)
    step = _hip_step(model, use_graph)
    losses = [step(x, t) for _ in range(2)]
    path = str(tmp_path / "state.pth")
    torch.save({"model": model.state_dict(), "train_step": step.state_dict()}, path)
    del model, step

    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["train_step"]["optimizer"]["kind"] == "hip_adam" and saved["train_step"]["optimizer"]["step"] == 2
    assert set(saved["train_step"]["optimizer"]["exp_avg"]) == set(saved["train_step"]["meta"]["names"])
    assert all(not v.is_cuda for v in saved["train_step"]["optimizer"]["exp_avg_sq"].values())
    assert saved["train_step"]["meta"]["train_precision"] == precision and saved["train_step"]["meta"]["deterministic"] is True
    fresh = _model(meta, precision)
    fresh.load_state_dict(saved["model"], strict=True)
    step2 = _hip_step(fresh, use_graph)
    step2.load_state_dict(saved["train_step"])
    assert step2.optimizer.t == 2
    losses += [step2(x, t) for _ in range(2)]
    got_p, got_m, got_v = _state(step2)
    assert losses == want_losses, (losses, want_losses)
    for name, a, b in zip(step2.names, got_p, want_p):
        assert torch.equal(a, b), f"parameter {name} differs after the resumed steps"
    assert torch.equal(got_m, want_m) and torch.equal(got_v, want_v)
    assert float(want_m.abs().max()) > 0 and float(want_v.max()) > 0
    # a state saved under another precision or mode is refused by name
    other = _model(meta, "bf16" if precision == "f32" else "f32")
    with pytest.raises(ValueError, match="`train_precision`"):
        _hip_step(other, False).load_state_dict(saved["train_step"])


def test_inference_engine_follows_the_weights_hip_adam_wrote():
    """The property of test_train_step_adam_reduces_the_loss_and_inference_follows_the_new_weights, for the kernel that writes the
    weights through raw pointers: the packed-weight caches (keyed on the parameter versions) must see every update."""
    z, meta = _load()
    x, t = _batch(z)
    model = _model(meta)
    with torch.no_grad():
        y0 = model(x).clone()                                    # fills the inference engine's caches from the initial weights
    step = _hip_step(model, False)
    versions = [p._version for p in step.allreduce.params]
    losses = [step(x, t) for _ in range(3)]
    assert losses[-1] < losses[0], losses
    assert all(p._version >= v + 3 for p, v in zip(step.allreduce.params, versions))
    with torch.no_grad():
        y1 = model(x).clone()
    assert float((y1 - y0).abs().max()) > 0
    fresh = _model(meta)
    fresh.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        y_fresh = fresh(x)
    assert torch.equal(y1, y_fresh), f"stale cache: max |diff| {float((y1 - y_fresh).abs().max()):.3e}"
    with torch.enable_grad():                                    # the training graph computes the same function of the new weights
        y_train = model(x).detach()
    assert float((y_train - y1).abs().max()) <= 1e-4


def test_torch_adam_state_loads_into_hip_adam():
    """Two steps with torch's Adam, then its state_dict() into HipAdam: moments and step count carry over exactly, directly and through
    TrainStep.load_state_dict; the next HipAdam step then moves the weights."""
    from fcvsr_amd.train import HipAdam, TrainStep
    z, meta = _load()
    x, t = _batch(z)
    model = _model(meta)
    tstep = TrainStep(model, lr=2e-4, weight_decay=1e-5, betas=(0.9, 0.99), deterministic=True)
    for _ in range(2):
        tstep(x, t)
    params = tstep.allreduce.params
    opt = HipAdam(params, tstep.names, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=1.0)
    opt.load_state_dict(tstep.optimizer.state_dict())
    assert opt.t == 2 and opt.lr == 2e-4 and opt.betas == (0.9, 0.99) and opt.eps == 1e-8 and opt.weight_decay == 1e-5
    for p, m, v in zip(params, opt.exp_avg.split(opt.sizes), opt.exp_avg_sq.split(opt.sizes)):
        st = tstep.optimizer.state[p]
        assert int(st["step"]) == 2
        assert torch.equal(m.view(p.shape), st["exp_avg"]) and torch.equal(v.view(p.shape), st["exp_avg_sq"])
    # through TrainStep: a run started with torch's Adam continues with optimizer="hip"
    twin = _model(meta)
    twin.load_state_dict(model.state_dict(), strict=True)
    hstep = TrainStep(twin, lr=2e-4, weight_decay=1e-5, betas=(0.9, 0.99), optimizer="hip", deterministic=True)
    hstep.load_state_dict(tstep.state_dict())
    assert hstep.optimizer.t == 2
    assert torch.equal(hstep.optimizer.exp_avg, opt.exp_avg) and torch.equal(hstep.optimizer.exp_avg_sq, opt.exp_avg_sq)
    before = [p.detach().clone() for p in hstep.allreduce.params]
    hstep(x, t)
    assert hstep.optimizer.t == 3 and any(not torch.equal(a, b) for a, b in zip(before, hstep.allreduce.params))
    # the other direction is refused
    with pytest.raises(ValueError, match="hip"):
        tstep.load_state_dict(hstep.state_dict())


# ---- fit_iters ----
class _Stop(Exception):
    pass


def _sequences():
    rs = np.random.RandomState(21)
    return [(rs.randint(0, 256, size=(9, 1, 24, 28)).astype(np.uint8), rs.randint(0, 256, size=(9, 1, 96, 112)).astype(np.uint8))
            for _ in range(2)]


def _fit(meta, precision, use_graph, ckpt_dir, **kw):
    """fresh model, sampler and loop; returns (losses, model, the `done` of every on_iter call)"""
    from fcvsr_amd.train import DeviceClipSampler, fit_iters
    model = _model(meta, precision)
    sampler = DeviceClipSampler(_sequences(), batch=2, crop=16, seed=0, device="cuda")
    seen = []
    stop_after = kw.pop("stop_after", None)

    def on_iter(done, loss):
        seen.append((done, loss))
        if stop_after is not None and done == stop_after:
            raise _Stop()
    losses = fit_iters(model, sampler, total_iters=6, device="cuda", lr=1e-4, use_graph=use_graph, deterministic=True,
                       ckpt_dir=ckpt_dir, ckpt_interval=2, on_iter=on_iter, log=lambda s: None, **kw)
    torch.cuda.synchronize()
    return losses, model, seen


@pytest.mark.parametrize("precision,use_graph", CASES, ids=IDS)
def test_fit_iters_stopped_and_resumed_equals_the_uninterrupted_run(precision, use_graph, tmp_path):
    from fcvsr_amd.train import latest, load_checkpoint
    _, meta = _load()
    dir_a, dir_b = str(tmp_path / "a"), str(tmp_path / "b")
    losses_a, model_a, seen_a = _fit(meta, precision, use_graph, dir_a)
    assert len(losses_a) == 6 and [d for d, _ in seen_a] == [1, 2, 3, 4, 5, 6] and [l for _, l in seen_a] == losses_a
    assert sorted(os.listdir(dir_a)) == ["iter_4.pth", "iter_6.pth"]               # keep=2

    with pytest.raises(_Stop):
        _fit(meta, precision, use_graph, dir_b, stop_after=3)
    assert latest(dir_b) == os.path.join(dir_b, "iter_2.pth")                       # the last complete checkpoint
    losses_b, model_b, seen_b = _fit(meta, precision, use_graph, dir_b, resume="auto")
    assert [d for d, _ in seen_b] == [3, 4, 5, 6], "the second call must continue from iteration 2"
    assert losses_b == losses_a, (losses_b, losses_a)
    sd_a, sd_b = model_a.state_dict(), model_b.state_dict()
    assert list(sd_a) == list(sd_b)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), f"{k} differs after the resumed run"
    ck_a, ck_b = load_checkpoint(os.path.join(dir_a, "iter_6.pth")), load_checkpoint(os.path.join(dir_b, "iter_6.pth"))
    assert ck_a["iter"] == ck_b["iter"] == 6 and ck_a["loss_history"] == ck_b["loss_history"] == losses_a
    for k in sd_a:
        assert torch.equal(ck_a["model"][k], ck_b["model"][k]) and torch.equal(ck_a["model"][k], sd_a[k].cpu()), k
    for key in ("exp_avg", "exp_avg_sq"):
        for name, v in ck_a["train_step"]["optimizer"][key].items():
            assert torch.equal(v, ck_b["train_step"]["optimizer"][key][name]), (key, name)
    assert ck_a["train_step"]["optimizer"]["step"] == 6 and ck_a["sampler"] == {"seed": 0, "len": 2, "batches": 1, "world": 1}
    assert ck_a["schedule"] == {"name": "cosine_restart", "periods": [6], "restart_weights": [1.0], "min_lr": 1e-7}
    assert len(set(losses_a)) == 6                                                  # six different batches, six different losses


def test_fit_iters_refuses_a_resume_under_another_sampler_or_world(tmp_path):
    from fcvsr_amd.train import DeviceClipSampler, fit_iters, load_checkpoint, save_checkpoint
    _, meta = _load()
    d = str(tmp_path / "c")
    _fit(meta, "f32", False, d)
    ckpt = load_checkpoint(os.path.join(d, "iter_6.pth"))
    kw = dict(total_iters=6, device="cuda", lr=1e-4, deterministic=True, log=lambda s: None)
    longer = DeviceClipSampler(_sequences() + _sequences()[:1], batch=1, crop=16, seed=0, device="cuda")
    with pytest.raises(ValueError, match="sampler len"):
        fit_iters(_model(meta), longer, resume=os.path.join(d, "iter_6.pth"), **kw)
    other_world = str(tmp_path / "w")
    save_checkpoint(other_world, 6, dict(ckpt, sampler=dict(ckpt["sampler"], world=2)))
    same = DeviceClipSampler(_sequences(), batch=2, crop=16, seed=0, device="cuda")
    with pytest.raises(ValueError, match="sampler world"):
        fit_iters(_model(meta), same, resume="auto", ckpt_dir=other_world, **kw)
    # a finished run resumed does nothing more
    losses = fit_iters(_model(meta), same, resume="auto", ckpt_dir=d, **kw)
    assert losses == ckpt["loss_history"]
