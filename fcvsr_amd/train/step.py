"""One data-parallel training step and the epoch loop around it (counterpart of reference
CVSR_train/train_LD_freqCVSR_S_22.py:183-266 on one process per GPU).

Frame windows are independent samples, so the batch shards over ranks (clip data parallel); the only collective of a step is
ONE all-reduce of the flat f32 gradient buffer (3.70 M / 8.81 M elements = 14.8 / 35.2 MB for S / full) over RCCL - a single
large message per step suits xGMI's point-to-point links better than per-layer buckets at these sizes.  The CVSR_train
loss is a SUM over the batch (opt/loss.py:20-31), so ranks add their gradients (op SUM); mmedit's mean loss averages.
Parameters that never receive a gradient (the never-called `DivEnh.Conv`) are left out of the buffer, so no
"unused parameter" machinery is needed (the reference's mmedit configs set find_unused_parameters=True for them).
"""
from __future__ import annotations

import os
import random
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .checkpoint import latest, load_checkpoint, save_checkpoint
from .loss import charbonnier_loss, charbonnier_loss_mmedit
from .ops import accumulate_into_grad
from .schedule import schedule_lr
from .optim import HipAdam


def trainable_parameters(model: torch.nn.Module) -> List[Tuple[str, torch.nn.Parameter]]:
    """Unique parameters that take part in the forward, in registration order (aliases `body.3.*` / `RCB.*` counted once)."""
    out = []
    for name, p in model.named_parameters():                     # named_parameters de-duplicates shared Parameters
        if p.requires_grad and ".DivEnh_block." in name and ".Conv." in name:
            continue                                             # reference CVSR_freq.py:2108: constructed, never called
        if p.requires_grad:
            out.append((name, p))
    return out


class FlatGradAllReduce:
    """Every gradient lives in ONE contiguous f32 buffer: `param.grad` of every trainable parameter is a view of it, so zeroing the
    gradients is one fill, the all-reduce needs no packing, and nothing is unpacked (round 2 copied 303 tensors in and out per step)."""

    def __init__(self, params: Sequence[torch.nn.Parameter], op: str = "sum", group=None):
        if op not in ("sum", "mean"):
            raise ValueError("op must be 'sum' (CVSR_train sum loss) or 'mean' (mmedit mean loss)")
        self.params = list(params)
        self.op, self.group = op, group
        self.sizes = [p.numel() for p in self.params]
        self.numel = int(sum(self.sizes))
        self.flat: Optional[torch.Tensor] = None

    def bind(self) -> torch.Tensor:
        """(Re)attach `.grad` of every parameter to its slice of the flat buffer (idempotent; follows `model.to(device)`)."""
        dev = self.params[0].device
        if self.flat is None or self.flat.device != dev:
            self.flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        for v, p in zip(self.flat.split(self.sizes), self.params):
            if p.grad is None:                                   # no gradient this step: the slice must not carry the last one's
                v.zero_()
                p.grad = v.view(p.shape)
            elif p.grad.data_ptr() != v.data_ptr():              # a gradient produced elsewhere (plain autograd): adopt its values
                v.copy_(p.grad.reshape(-1))
                p.grad = v.view(p.shape)
        return self.flat

    def zero(self) -> None:
        self.bind().zero_()

    def __call__(self) -> torch.Tensor:
        flat = self.bind()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            if flat.is_cuda and dist.get_backend(self.group) == "gloo":         # CPU rehearsals of the N>1 path
                host = flat.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
                flat.copy_(host)
            else:
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)   # backend "nccl" is RCCL on ROCm
            if self.op == "mean":
                flat.div_(dist.get_world_size(self.group))
        return flat


class TrainStep:
    """optimizer.zero_grad(); sr = model(lr); loss = Charbonnier(sr, hr); loss.backward(); all-reduce; optimizer.step()."""

    def __init__(self, model: torch.nn.Module, *, lr: float = 1e-4, weight_decay: float = 1e-5,
                 loss_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor] = charbonnier_loss, reduce_op: str = "sum",
                 optimizer=None, group=None, use_graph: bool = False, deterministic: Optional[bool] = None,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        """use_graph: capture forward + loss + backward of the first batch shape in a hipGraph and replay it (the step is ~4 k
        small launches; replaying removes their host cost).  Gradients then live in static buffers; the all-reduce and the
        optimizer step stay eager.  Batches must keep the captured shape (a different shape is captured anew).
        deterministic: True / False sets `model.train_deterministic` (True: the backward uses no float atomics, so a step from the same
        weights and batch gives the same gradients, loss and updated weights bit for bit, eager or replayed); None leaves it alone.
        optimizer: None (torch.optim.Adam over the trainable parameters, the default), a torch optimizer, "hip" (`HipAdam` with
        `lr`, `betas`, `eps`, `weight_decay`: the whole update in one launch, the state two flat buffers) or a `HipAdam` over
        `trainable_parameters(model)`."""
        self.model = model
        if deterministic is not None:
            if not hasattr(model, "train_deterministic"):
                raise ValueError("deterministic needs a model with a `train_deterministic` attribute (the drop-in modules of "
                                 "fcvsr_amd.arch): on any other module the flag would change nothing")
            model.train_deterministic = bool(deterministic)
        self.use_graph = use_graph
        self._graphs = {}
        named = trainable_parameters(model)
        self.names = [n for n, _ in named]
        params = [p for _, p in named]
        # reference defaults: Adam(lr=1e-4, weight_decay=1e-5) (train_LD_freqCVSR_S_22.py:35,42,204)
        # (torch's fused=True Adam does not advance the parameters' version counters, which the inference engine's packed-weight
        # cache is keyed on: the default multi-tensor implementation stays)
        if isinstance(optimizer, str):
            if optimizer != "hip":
                raise ValueError(f'optimizer must be None, "hip", a HipAdam or a torch optimizer, got {optimizer!r}')
            optimizer = HipAdam(params, self.names, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        elif isinstance(optimizer, HipAdam):
            if len(optimizer.params) != len(params) or any(a is not b for a, b in zip(optimizer.params, params)):
                raise ValueError("a HipAdam passed to TrainStep must be built over trainable_parameters(model), in that order")
        self.optimizer = optimizer or torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.loss_fn = loss_fn
        self.allreduce = FlatGradAllReduce(params, reduce_op, group)

    def local_backward(self, lr_frames: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        """This rank's forward + loss + backward (no collective): gradients end up in `.grad`.  Split from the collective
        half so that a caller can agree on success across ranks BEFORE anybody enters the all-reduce (bench.py does)."""
        if self.use_graph and lr_frames.is_cuda:
            return self._graphed(lr_frames, hr)
        self.allreduce.zero()                              # one fill: every .grad is a view of the flat buffer
        sr = self.model(lr_frames)
        loss = self.loss_fn(sr, hr)
        with accumulate_into_grad(self.allreduce.flat):    # the HIP reductions add weight / bias gradients straight into it
            loss.backward()
        return loss

    def reduce_and_update(self) -> None:
        """The collective half: ONE all-reduce of the flat gradient buffer, then the (replicated) optimizer step."""
        flat = self.allreduce()
        if isinstance(self.optimizer, HipAdam):
            self.optimizer.step(flat)                      # one launch over the flat buffers (eager: not part of the captured graph)
        else:
            self.optimizer.step()

    def set_lr(self, lr: float) -> None:
        """The learning rate of the next update, for either kind of optimizer."""
        if isinstance(self.optimizer, HipAdam):
            self.optimizer.lr = float(lr)
        else:
            for group in self.optimizer.param_groups:
                group["lr"] = float(lr)

    def _meta(self) -> dict:
        world = dist.get_world_size(self.allreduce.group) if dist.is_available() and dist.is_initialized() else 1
        return {"names": list(self.names), "shapes": [list(p.shape) for p in self.allreduce.params],
                "train_precision": getattr(self.model, "train_precision", None),
                "deterministic": getattr(self.model, "train_deterministic", None), "world": world}

    def state_dict(self) -> dict:
        """{"optimizer": the optimizer's state (`HipAdam.state_dict()`, or {"kind": "torch", "state": optimizer.state_dict()} with
        host tensors), "meta": what a resume must match - parameter names and shapes, the model's train_precision and deterministic
        flag (None on a module without them) and the world size}.  The weights are the model's own state_dict, not part of this."""
        if isinstance(self.optimizer, HipAdam):
            opt = self.optimizer.state_dict()
        else:
            opt = {"kind": "torch", "state": _to_host(self.optimizer.state_dict())}
        return {"optimizer": opt, "meta": self._meta()}

    def load_state_dict(self, sd: dict) -> None:
        """Restore `state_dict()`.  Every field of its meta must equal this TrainStep's (ValueError naming the field otherwise).  A
        torch.optim.Adam state loads into a HipAdam (the run switches optimizers); a HipAdam state does not load into a torch
        optimizer."""
        mine, theirs = self._meta(), sd["meta"]
        for field in ("names", "shapes", "train_precision", "deterministic", "world"):
            a, b = theirs.get(field), mine[field]
            if field == "shapes" and a is not None:
                a = [list(s) for s in a]
            if a != b:
                raise ValueError(f"the saved training state does not match this TrainStep in `{field}`: saved {_brief(a)}, here {_brief(b)}")
        opt = sd["optimizer"]
        if isinstance(self.optimizer, HipAdam):
            self.optimizer.load_state_dict(opt["state"] if opt.get("kind") == "torch" else opt)
        elif opt.get("kind") == "torch":
            self.optimizer.load_state_dict(opt["state"])
        else:
            raise ValueError(f"the saved optimizer state is of kind {opt.get('kind')!r}: it loads into TrainStep(optimizer=\"hip\") only")

    def __call__(self, lr_frames: torch.Tensor, hr: torch.Tensor) -> float:
        """lr_frames: (b, 7, C, h, w), hr: (b, C, 4h, 4w) - this rank's share of the batch."""
        loss = self.local_backward(lr_frames, hr)
        self.reduce_and_update()
        return float(loss.detach())

    def _graphed(self, lr_frames: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
        # (the captured graph has the kernel choice of the deterministic mode baked in)
        key = (tuple(lr_frames.shape), tuple(hr.shape), str(lr_frames.device), bool(getattr(self.model, "train_deterministic", False)))
        ent = self._graphs.get(key)
        if ent is None:
            sx, sh = lr_frames.clone(), hr.clone()
            params = self.allreduce.params
            # warm-up on a side stream (allocations, weight packing, per-kernel attributes, per-device zero page), as
            # torch.cuda.graphs requires; leaves .grad tensors allocated so the capture accumulates into static buffers
            side = torch.cuda.Stream(lr_frames.device)
            side.wait_stream(torch.cuda.current_stream(lr_frames.device))
            with torch.cuda.stream(side):
                for _ in range(2):
                    self.allreduce.zero()
                    with accumulate_into_grad(self.allreduce.flat):
                        self.loss_fn(self.model(sx), sh).backward()
            torch.cuda.current_stream(lr_frames.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.allreduce.flat.zero_()                  # gradients accumulate into the static flat buffer
                loss = self.loss_fn(self.model(sx), sh)
                with accumulate_into_grad(self.allreduce.flat):
                    loss.backward()
            # the graph holds raw pointers into the packed-weight plan that was live at capture (fcvsr_amd.train.ops.WeightPacker):
            # keep that plan alive with the graph, whatever the model's packer does later
            packer = self.model.train_packer() if hasattr(self.model, "train_packer") else None
            ent = self._graphs[key] = (graph, sx, sh, loss, packer.plan if packer is not None else None)
        graph, sx, sh, loss, _ = ent
        sx.copy_(lr_frames)
        sh.copy_(hr)
        graph.replay()
        return loss


def _to_host(obj):
    """`obj` with every tensor copied to the host (dicts, lists and tuples walked)."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_host(v) for v in obj)
    return obj


def _brief(v) -> str:
    s = repr(v)
    return s if len(s) <= 120 else s[:117] + "..."


# ---- data transforms of the reference loader (CVSR_train/opt/data_LD_LR.py:248-344), on {lr_imgs (f,h,w), hr_imgs (f',4h,4w)} ----
def random_crop(sample: Dict[str, np.ndarray], size: int = 128, rng=np.random) -> Dict[str, np.ndarray]:
    lr, hr = sample["lr_imgs"], sample["hr_imgs"]
    h, w = lr.shape[1:]
    top, left = rng.randint(0, h - size), rng.randint(0, w - size)           # high end exclusive, as in the reference
    return dict(sample, lr_imgs=lr[:, top:top + size, left:left + size],
                hr_imgs=hr[:, top * 4:(top + size) * 4, left * 4:(left + size) * 4])


def augment(sample: Dict[str, np.ndarray], rng=random) -> Dict[str, np.ndarray]:
    lr, hr = sample["lr_imgs"], sample["hr_imgs"]
    hflip, vflip, rot90 = rng.random() < 0.5, rng.random() < 0.5, rng.random() < 0.5
    if hflip:
        lr, hr = lr[:, :, ::-1], hr[:, :, ::-1]
    if vflip:
        lr, hr = lr[:, ::-1, :], hr[:, ::-1, :]
    if rot90:
        lr, hr = lr.transpose(0, 2, 1), hr.transpose(0, 2, 1)
    return dict(sample, lr_imgs=lr.copy(), hr_imgs=hr.copy())


def _unit_float(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint16:
        # 10-bit samples in uint16 containers: the float contract of the uint16 kernels (`hip.u16_table`, built from this expression):
        # a sample above 1023 reads as 1023, full scale is 1023
        return torch.from_numpy(np.minimum(a, 1023).astype(np.int32)).float() / 1023.0
    return torch.from_numpy(a).float() / 255.0


def to_tensor(sample: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
    """uint8 (f,h,w) -> float (1,f,h,w) / 255 (channel axis first, as the reference's ToTensor); uint16 (10-bit samples) ->
    min(k, 1023) as float / 1023."""
    return {"lr_imgs": _unit_float(sample["lr_imgs"][np.newaxis]), "hr_imgs": _unit_float(sample["hr_imgs"][np.newaxis])}


def fit(model: torch.nn.Module, batches: Callable[[int], Iterable[Dict[str, torch.Tensor]]], *, epochs: int, device,
        lr: float = 1e-4, weight_decay: float = 1e-5, milestones: Sequence[int] = (2000, 8000, 12000, 20000), gamma: float = 0.5,
        val_itv: int = 1, ckpt_dir: Optional[str] = None, warm_start_epoch: int = 0, log: Callable[[str], None] = print,
        val_sequences: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None,
        on_validate: Optional[Callable[[int, float, float], None]] = None, deterministic: Optional[bool] = None,
        loss_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor] = charbonnier_loss, reduce_op: str = "sum") -> List[float]:
    """Epoch loop of the reference (train_LD_freqCVSR_S_22.py:239-266): MultiStepLR stepped at the START of every epoch,
    Charbonnier-sum loss, Adam, `epoch-%d.pth` state_dict checkpoints every `val_itv` epochs (rank 0).
    `batches(epoch)` yields {'lr_imgs': (b,C,7,h,w), 'hr_imgs': (b,C,f',4h,4w)} like the reference DataLoader.

    val_sequences: (lr (N,C,H,W), hr (N,C,4H,4W)) pairs, hr uint8 (8-bit frames, peak 255) or uint16 (10-bit samples, peak 1023),
    lr float in [0,1] or of hr's integer dtype, torch tensors or numpy arrays, scored after the checkpoint of every `val_itv`-th epoch
    on rank 0 (the reference's eval_seq, :263-280): the average over the sequences of each one's mean per-frame PSNR / SSIM
    (`harness.infer.evaluate_sequence` with its defaults: crop border 4, truncating quantisation) is logged as
    `PSNR:%f, SSIM: %f` and passed to `on_validate(epoch, psnr, ssim)` (epoch counted from 1).  It runs under no_grad:
    parameters, gradients and optimizer state are not touched.

    deterministic: passed to `TrainStep` (True: bit-repeatable steps; None leaves `model.train_deterministic` as it is).
    loss_fn, reduce_op: passed to `TrainStep`; the defaults are the reference loop's Charbonnier sum with summed gradients (a mean-type
    loss such as `charbonnier_ffl_loss` goes with reduce_op="mean")."""
    step = TrainStep(model, lr=lr, weight_decay=weight_decay, deterministic=deterministic, loss_fn=loss_fn, reduce_op=reduce_op)
    sched = torch.optim.lr_scheduler.MultiStepLR(step.optimizer, milestones=list(milestones), gamma=gamma)
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    model.train()
    history: List[float] = []
    for epoch in range(warm_start_epoch, epochs):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # the reference steps the scheduler before the optimizer
            sched.step()
        losses = []
        for data in batches(epoch):
            frames = data["lr_imgs"].permute(0, 2, 1, 3, 4).to(device)      # (b, frames, chn, h, w)
            hr = data["hr_imgs"].to(device)[:, :, 0]
            losses.append(step(frames, hr))
        avg = round(sum(losses) / max(1, len(losses)), 5)
        history.append(avg)
        log("Epoch: %d/%d | average epoch loss: %f" % (epoch + 1, epochs, avg))
        if (epoch + 1) % val_itv == 0 and ckpt_dir is not None and rank == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
            torch.save(model.state_dict(), os.path.join(ckpt_dir, "epoch-%d.pth" % (epoch + 1 + warm_start_epoch)))
        if (epoch + 1) % val_itv == 0 and val_sequences and rank == 0:
            psnr, ssim = validate(model, val_sequences)
            log("PSNR:%f, SSIM: %f" % (psnr, ssim))
            if on_validate is not None:
                on_validate(epoch + 1, psnr, ssim)
    return history


def _as_tensor(a) -> torch.Tensor:
    if isinstance(a, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("=")))
    return a


@torch.no_grad()
def validate(model: torch.nn.Module, sequences: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> Tuple[float, float]:
    """Mean over `sequences` of each sequence's mean per-frame PSNR and SSIM, scored on the device (reference
    test_LD_freqCVSR_S_22.py:118-119).  sequences: (lr, hr) pairs as `fit`'s val_sequences: uint8 hr is scored at peak 255, uint16
    hr (10-bit samples) at peak 1023; numpy arrays are taken as they are (no value is converted)."""
    from ..harness.infer import evaluate_sequence
    scores = [evaluate_sequence(model, _as_tensor(lr), _as_tensor(hr)) for lr, hr in sequences]
    return float(np.mean([s.psnr_mean for s in scores])), float(np.mean([s.ssim_mean for s in scores]))


def iter_position(i: int, batches_per_epoch: int) -> Tuple[int, int]:
    """(epoch, batch of that epoch) of iteration `i` (counted from 0) of a loop that walks `batches_per_epoch` batches per epoch."""
    if i < 0 or batches_per_epoch < 1:
        raise ValueError(f"iteration {i} of {batches_per_epoch} batches per epoch")
    return i // batches_per_epoch, i % batches_per_epoch


def _sampler_meta(sampler) -> dict:
    return {"seed": int(sampler.seed), "len": len(sampler), "batches": len(sampler.plan(0)), "world": int(sampler.world)}


def fit_iters(model: torch.nn.Module, sampler, *, total_iters: int, device, lr: float = 1e-5, betas: Tuple[float, float] = (0.9, 0.99),
              weight_decay: float = 0.0, loss_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor] = charbonnier_loss_mmedit,
              reduce_op: str = "mean", schedule: Optional[dict] = None, optimizer="hip", use_graph: bool = False,
              deterministic: Optional[bool] = None, ckpt_dir: Optional[str] = None, ckpt_interval: int = 5000, keep: Optional[int] = 2,
              val_sequences: Optional[Sequence[Tuple[torch.Tensor, torch.Tensor]]] = None, val_interval: int = 5000,
              log_interval: int = 100, resume: Optional[str] = None, on_iter: Optional[Callable[[int, float], None]] = None,
              log: Callable[[str], None] = print, on_validate: Optional[Callable[[int, float, float], None]] = None) -> List[float]:
    """Iteration loop of the reference's mmedit side (configs/restorers/fcvsr/fcvsr_s_redsLD_QP22.py:93-109): Adam with betas
    (0.9, 0.99), a mean Charbonnier loss averaged over ranks, a cosine-restart schedule by iteration, and every `ckpt_interval`
    iterations (and after the last) a checkpoint WITH the optimizer state, from which the run continues (`train/checkpoint.py`).

    sampler: a `DeviceClipSampler` (anything with `seed`, `world`, `__len__`, `plan(epoch)` and `build(batch_plan)`).  An epoch is
    one walk over this rank's batches, n = len(sampler.plan(0)) of them (the same on every rank); iteration i (from 0) is batch
    i % n of epoch i // n, built with `sampler.build(sampler.plan(epoch)[i % n])` - a pure function of (seed, i), so a resumed run
    builds no skipped batch.  The update of iteration i uses the learning rate `schedule` gives for position i.
    schedule: {"name": "cosine_restart" | "multistep", **arguments} (`train/schedule.py`); None: one cosine period of `total_iters`
    down to 1e-7, as the configs have.
    resume: a checkpoint path, or "auto": `latest(ckpt_dir)`, a fresh start when there is none.  The checkpoint's parameter names
    and shapes, train precision, deterministic flag, world size, schedule and sampler (seed, length, batches per epoch, world)
    must be this call's: ValueError otherwise (a resume at another world size is refused).
    on_iter(done, loss): called after every update and whatever checkpoint or validation that iteration makes, done = the number of
    updates so far.  Validation: `validate(model, val_sequences)` on rank 0 every `val_interval` iterations, logged and passed to
    `on_validate(done, psnr, ssim)` as in `fit`.
    Returns the loss of every iteration, those before a resume included.

    With deterministic=True and a seeded sampler, a run stopped at any checkpoint and resumed gives the losses, moments and weights
    of the uninterrupted run bit for bit, eager or with use_graph.  Without it the restored state is exact and the steps that
    follow differ as any two runs do."""
    if total_iters < 0 or ckpt_interval < 1 or val_interval < 1 or log_interval < 1:
        raise ValueError("total_iters must be >= 0 and the intervals >= 1")
    if schedule is None:
        schedule = {"name": "cosine_restart", "periods": [int(total_iters)], "restart_weights": [1.0], "min_lr": 1e-7}
    schedule = dict(schedule)
    step = TrainStep(model, lr=lr, weight_decay=weight_decay, loss_fn=loss_fn, reduce_op=reduce_op, optimizer=optimizer,
                     use_graph=use_graph, deterministic=deterministic, betas=betas)
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    meta = _sampler_meta(sampler)
    n_batches = meta["batches"]
    if n_batches < 1:
        raise ValueError("the sampler plans no batch for this rank")
    history: List[float] = []
    start = 0
    if resume == "auto":
        resume = latest(ckpt_dir) if ckpt_dir is not None else None
    if resume is not None:
        ckpt = load_checkpoint(resume)
        for field in ("world", "len", "batches", "seed"):
            if ckpt["sampler"].get(field) != meta[field]:
                raise ValueError(f"{resume} was written with sampler {field} {ckpt['sampler'].get(field)}, this run has {meta[field]}: "
                                 "a run resumes with the data order it was started with (the same world size and sampler)")
        if dict(ckpt["schedule"]) != schedule:
            raise ValueError(f"{resume} was written under the schedule {ckpt['schedule']}, this run asks for {schedule}")
        if ckpt["iter"] > total_iters:
            raise ValueError(f"{resume} is at iteration {ckpt['iter']}, past total_iters = {total_iters}")
        model.load_state_dict(ckpt["model"], strict=True)
        step.load_state_dict(ckpt["train_step"])
        history = [float(v) for v in ckpt["loss_history"]]
        start = int(ckpt["iter"])
        log("resumed from %s at iteration %d" % (resume, start))
    model.train()
    plans, plans_epoch = None, -1
    for i in range(start, total_iters):
        epoch, k = iter_position(i, n_batches)
        if epoch != plans_epoch:
            plans, plans_epoch = sampler.plan(epoch), epoch
        data = sampler.build(plans[k])
        frames = data["lr_imgs"].permute(0, 2, 1, 3, 4).to(device)          # (b, frames, chn, h, w)
        hr = data["hr_imgs"].to(device)[:, :, 0]
        cur_lr = schedule_lr(schedule, lr, i)
        step.set_lr(cur_lr)
        loss = step(frames, hr)
        history.append(loss)
        done = i + 1
        if done % log_interval == 0:
            log("Iter: %d/%d | lr: %.3e | loss: %f" % (done, total_iters, cur_lr, loss))
        if ckpt_dir is not None and rank == 0 and (done % ckpt_interval == 0 or done == total_iters):
            save_checkpoint(ckpt_dir, done, {"model": _to_host(model.state_dict()), "train_step": step.state_dict(),
                                             "schedule": schedule, "sampler": meta, "loss_history": list(history)}, keep=keep)
        if done % val_interval == 0 and val_sequences and rank == 0:
            psnr, ssim = validate(model, val_sequences)
            model.train()
            log("PSNR:%f, SSIM: %f" % (psnr, ssim))
            if on_validate is not None:
                on_validate(done, psnr, ssim)
        if on_iter is not None:
            on_iter(done, loss)
    return history
