"""Training batches built on the device from resident 8-bit or 10-bit sequences.

The reference loader (CVSR_train/opt/data_LD_LR.py:83-127, :248-344) picks a 7-frame window of a sequence, crops it at a random
place, flips / transposes it and converts it to float on a CPU worker, per clip.  Here the uint8 sequences go to the device once;
per batch the host only makes the draws (`DeviceClipSampler.plan`) and fills one descriptor per output plane, and ONE kernel
(`hip.clip_batch`, csrc/clip_batch.hip) cuts, flips, transposes and converts every LR plane of the batch, a second launch every HR
plane.  The values are the reference chain's bit for bit: `apply_plan_host` is that chain (`random_crop` / `augment` / `to_tensor`
of `train/step.py`, fed the planned draws) and is what the kernel is tested against.

10-bit sequences are uint16 containers (peak 1023): the same sampler, the same descriptors with `pitch` / `top` / `left` in samples,
the 2-byte kernel and the 1024-entry table of `hip.u16_table`.  The reference has no 10-bit loader; the specification is this
project's float contract for 10-bit frames, ``min(k, 1023).float() / 1023`` (`to_tensor`), the floats `super_resolve_u16` feeds the
network for the same samples.  All sequences of one sampler share one dtype.
"""
from __future__ import annotations

import random
from typing import Dict, Iterator, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..harness.sharding import shard
from .step import augment, random_crop, to_tensor

STARTS = ("random", "first", "gop")


class BatchPlan(NamedTuple):
    """The draws of one batch, one entry per clip (integer / bool numpy arrays of equal length)."""
    item: np.ndarray     # sequence index
    first: np.ndarray    # first LR frame of the window; the HR frame is first + frames // 2
    top: np.ndarray      # crop corner in LR pixels
    left: np.ndarray
    hflip: np.ndarray
    vflip: np.ndarray
    rot90: np.ndarray    # the reference's name for transpose(0, 2, 1)


BIT_DEPTH = {torch.uint8: 8, torch.uint16: 10}


def _as_frames(a, what: str):
    if isinstance(a, np.ndarray):
        if a.dtype.kind != "u" or a.dtype.itemsize > 2:
            raise ValueError(f"{what}: frames must be uint8 or uint16, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("=")))
    if not isinstance(a, torch.Tensor) or a.dtype not in BIT_DEPTH:
        raise ValueError(f"{what}: frames must be a uint8 or uint16 tensor or array, got {getattr(a, 'dtype', type(a))}")
    if a.dim() != 4:
        raise ValueError(f"{what}: expected (N,C,H,W), got {tuple(a.shape)}")
    return a


def check_sequences(sequences, crop: int, frames: int, start: str):
    """The constructor's checks (ValueError): uint8 or uint16 (N,C,H,W) / (N,C,4H,4W) pairs of one dtype (LR and HR of every
    sequence alike) and one channel count, frames larger than the crop in both axes (the reference's randint(0, h - size) has an
    exclusive high end), enough frames for the window and the start mode."""
    if start not in STARTS:
        raise ValueError(f"start must be one of {STARTS}, got {start!r}")
    if crop <= 0 or crop % 4:
        raise ValueError(f"crop must be a positive multiple of 4, got {crop}")
    if frames < 1:
        raise ValueError(f"frames must be >= 1, got {frames}")
    if len(sequences) == 0:
        raise ValueError("no sequences")
    out = []
    for i, pair in enumerate(sequences):
        lr, hr = _as_frames(pair[0], f"sequence {i} lr"), _as_frames(pair[1], f"sequence {i} hr")
        if lr.dtype != hr.dtype:
            raise ValueError(f"sequence {i}: lr is {lr.dtype}, hr is {hr.dtype}; a pair must be all uint8 or all uint16")
        if out and lr.dtype != out[0][0].dtype:
            raise ValueError(f"sequence {i}: {lr.dtype} frames, sequence 0 has {out[0][0].dtype}; all sequences of a sampler must "
                             "be uint8 or all uint16")
        N, C, H, W = lr.shape
        if tuple(hr.shape) != (N, C, 4 * H, 4 * W):
            raise ValueError(f"sequence {i}: hr must be 4x the lr frames, (N,C,4H,4W) = {(N, C, 4 * H, 4 * W)}, got {tuple(hr.shape)}")
        if out and C != out[0][0].shape[1]:
            raise ValueError(f"sequence {i}: {C} channels, sequence 0 has {out[0][0].shape[1]}")
        if H <= crop or W <= crop:
            raise ValueError(f"sequence {i}: {H}x{W} frames are not larger than the {crop}x{crop} crop in both axes "
                             "(the crop corner is drawn with randint(0, size - crop), high end exclusive)")
        if N < frames:
            raise ValueError(f"sequence {i}: {N} frames, a window needs {frames}")
        if start == "gop" and 24 + frames > N:
            raise ValueError(f'sequence {i}: start="gop" draws first frames up to 24 and needs {24 + frames} frames, got {N}')
        out.append((lr, hr))
    return out


def item_draws(seed: int, epoch: int, item: int, shape: Tuple[int, int, int], crop: int, frames: int, start: str):
    """The draws of `item` (a sequence of `shape` = (N, H, W)) in `epoch`, in the reference's order, from two private streams:
        numpy.random.RandomState([seed, epoch, item])            top, left (RandomCrop)
        random.Random((seed << 64) | (epoch << 32) | item)        first frame, then hflip, vflip, rot90 (__getitem__, Augment)
    Plain integers, so every process derives the same streams."""
    N, H, W = shape
    rs = np.random.RandomState([seed, epoch, item])
    rnd = random.Random((seed << 64) | (epoch << 32) | item)
    if start == "random":
        first = rnd.randint(0, N - frames)                      # inclusive, as random.randint(0, 25) for N = 32
    elif start == "gop":
        first = rnd.randint(0, 6) * 4
    else:
        first = 0                                               # only_I_frame
    top, left = rs.randint(0, H - crop), rs.randint(0, W - crop)
    hflip, vflip, rot90 = rnd.random() < 0.5, rnd.random() < 0.5, rnd.random() < 0.5
    return first, top, left, hflip, vflip, rot90


def make_plan(shapes: Sequence[Tuple[int, int, int]], epoch: int, *, batch: int, crop: int, frames: int, seed: int, start: str,
              rank: int, world: int) -> List[BatchPlan]:
    """This rank's batches of `epoch` (host only).  The epoch order is RandomState([seed, epoch]).permutation(n), padded by
    wrapping round to its head up to a multiple of `world` (as torch's DistributedSampler), cut into equal contiguous shares
    (`harness.sharding.shard`) and then into batches; the last one may be short."""
    n = len(shapes)
    order = epoch_order(n, epoch, seed, world)
    lo, hi = shard(len(order), rank, world)
    mine = order[lo:hi]
    out = []
    for s in range(0, len(mine), batch):
        items = mine[s:s + batch]
        d = [item_draws(seed, epoch, int(i), shapes[int(i)], crop, frames, start) for i in items]
        cols = list(zip(*d))
        out.append(BatchPlan(np.asarray(items, dtype=np.int64), *(np.asarray(c, dtype=np.int64) for c in cols[:3]),
                             *(np.asarray(c, dtype=bool) for c in cols[3:])))
    return out


def epoch_order(n: int, epoch: int, seed: int, world: int) -> np.ndarray:
    """The padded item order of `epoch`: a permutation of range(n) followed by its first (-n) % world entries."""
    perm = np.random.RandomState([seed, epoch]).permutation(n)
    return np.concatenate([perm, perm[:(-n) % world]])


class _Replay:
    """Stands in for the random module / numpy.random: hands out the planned draws in the order the transforms ask for them."""

    def __init__(self, values):
        self.values = list(values)

    def randint(self, lo, hi):
        return self.values.pop(0)

    def random(self):
        return self.values.pop(0)


def apply_plan_host(sequences, batch_plan: BatchPlan, crop: int, frames: int = 7) -> Dict[str, torch.Tensor]:
    """The batch of `batch_plan` made on the CPU by the reference chain, plane by plane: `random_crop`, `augment`, `to_tensor` with
    the planned draws in place of the random ones.  Returns {'lr_imgs': (b,C,frames,crop,crop), 'hr_imgs': (b,C,1,4crop,4crop)}
    f32 CPU tensors.  uint8 sequences are the reference's k / 255; uint16 (10-bit) ones give min(k, 1023) / 1023 (`to_tensor`).
    This is the specification of the device path (which never calls it) for both depths, and a debugging aid."""
    lrs, hrs = [], []
    for k in range(len(batch_plan.item)):
        lr, hr = sequences[int(batch_plan.item[k])]
        lr = hip.frames_to_numpy(lr) if isinstance(lr, torch.Tensor) else np.asarray(lr)
        hr = hip.frames_to_numpy(hr) if isinstance(hr, torch.Tensor) else np.asarray(hr)
        first = int(batch_plan.first[k])
        centre = first + frames // 2
        lr_c, hr_c = [], []
        for c in range(lr.shape[1]):
            sample = {"lr_imgs": lr[first:first + frames, c], "hr_imgs": hr[centre:centre + 1, c]}
            sample = random_crop(sample, crop, rng=_Replay([int(batch_plan.top[k]), int(batch_plan.left[k])]))
            sample = augment(sample, rng=_Replay([0.0 if f else 1.0 for f in
                                                  (batch_plan.hflip[k], batch_plan.vflip[k], batch_plan.rot90[k])]))
            t = to_tensor(sample)
            lr_c.append(t["lr_imgs"][0])
            hr_c.append(t["hr_imgs"][0])
        lrs.append(torch.stack(lr_c))
        hrs.append(torch.stack(hr_c))
    return {"lr_imgs": torch.stack(lrs), "hr_imgs": torch.stack(hrs)}


_DESC = np.dtype(hip.CropDesc)
_RING = 4


def fill_descs(d: np.ndarray, lr_ptr, hr_ptr, first, top, left, flags, H, W, F: int, C: int, itemsize: int = 1) -> None:
    """Write the b*F*C LR descriptors (clip, frame, channel order: the model's (b,F,C,s,s) layout) and then the b*C HR descriptors
    of a batch into `d` (a numpy.dtype(hip.CropDesc) array).  Per clip: lr_ptr / hr_ptr = first byte of its sequence's dense
    (N,C,H,W) / (N,C,4H,4W) frames, H x W = its LR frame size; the HR window is the LR one times 4, on frame first + F // 2.
    itemsize: bytes per sample (1: uint8, 2: uint16).  The `src` byte addresses scale with it; `pitch` / `top` / `left` are in
    samples whatever it is."""
    b = len(first)
    n_lr = b * F * C
    lr, hr = d[:n_lr].reshape(b, F, C), d[n_lr:].reshape(b, C)
    lr_ptr, hr_ptr = np.asarray(lr_ptr, dtype=np.uint64), np.asarray(hr_ptr, dtype=np.uint64)
    plane = (H * W).astype(np.uint64) * np.uint64(itemsize)                                      # bytes of one LR plane
    frame = (first[:, None] + np.arange(F)[None, :]).astype(np.uint64)                           # (b, F)
    chan = np.arange(C, dtype=np.uint64)
    lr["src"] = lr_ptr[:, None, None] + (frame[:, :, None] * np.uint64(C) + chan[None, None, :]) * plane[:, None, None]
    centre = (first + F // 2).astype(np.uint64)
    hr["src"] = hr_ptr[:, None] + (centre[:, None] * np.uint64(C) + chan[None, :]) * (plane[:, None] * np.uint64(16))
    for dd, k, ix in ((lr, 1, (slice(None), None, None)), (hr, 4, (slice(None), None))):
        dd["pitch"], dd["top"], dd["left"], dd["flags"] = (k * W)[ix], (k * top)[ix], (k * left)[ix], flags[ix]


class DeviceClipSampler:
    """Random training clips cut on the device from uint8 or uint16 (10-bit) sequences that live there.

    sequences: (lr (N,C,H,W), hr (N,C,4H,4W)) pairs, all uint8 or all uint16, torch tensors or numpy arrays, host or device;
    uploaded once and kept (uint16 frames as int16 views of the same bits, `hip.bits16`).  `dtype` is their torch dtype, `bit_depth`
    8 or 10; a 10-bit pixel k becomes ``min(k, 1023) / 1023``, the float `super_resolve_u16` feeds the network for it.
    An item is a sequence.  `sampler(epoch)` yields {'lr_imgs': (b,C,frames,crop,crop), 'hr_imgs': (b,C,1,4crop,4crop)} f32 on the
    device - the `batches` callable of `fit`.  The draws of (seed, epoch, item) are those of `item_draws`, whatever `world`, `rank`
    and `batch` are; the epoch order and its sharding over ranks are `make_plan`'s: every rank yields the same number of batches of
    the same sizes.  start: "random" (random_start), "first" (only_I_frame) or "gop" (first frame a multiple of 4 up to 24)."""

    def __init__(self, sequences, *, batch: int, crop: int = 128, frames: int = 7, seed: int, start: str = "random", rank: int = 0,
                 world: int = 1, device):
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world of {world}")
        if not (0 <= seed < 2 ** 32):
            raise ValueError(f"seed must be in [0, 2**32), got {seed}")
        seqs = check_sequences(sequences, crop, frames, start)
        self.batch, self.crop, self.frames, self.seed, self.start = batch, crop, frames, seed, start
        self.rank, self.world = rank, world
        self.shapes = [(lr.shape[0], lr.shape[2], lr.shape[3]) for lr, _ in seqs]
        self.channels = seqs[0][0].shape[1]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceClipSampler builds its batches on the HIP device only (there is no CPU fallback; "
                               "apply_plan_host is the CPU specification)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dtype = seqs[0][0].dtype
        self.bit_depth = BIT_DEPTH[self.dtype]
        self.sequences = [(hip.bits16(lr).to(self.device).contiguous(), hip.bits16(hr).to(self.device).contiguous()) for lr, hr in seqs]
        self._lr_ptr = np.array([lr.data_ptr() for lr, _ in self.sequences], dtype=np.uint64)
        self._hr_ptr = np.array([hr.data_ptr() for _, hr in self.sequences], dtype=np.uint64)
        self._N, self._H, self._W = (np.array(v, dtype=np.int64) for v in zip(*self.shapes))
        hip.sample_table(self.dtype, self.device)                                       # built here, outside any capture
        # Descriptor lifetime: a ring of _RING (pinned host buffer, device buffer, event) slots per batch size.  A slot's event is
        # recorded behind the two launches that read its device buffer (and so behind the upload that read its host buffer);
        # build() waits for that event before it writes the slot again, so neither buffer changes under queued work, however
        # many batches the caller queues without synchronising.
        self._rings: Dict[int, list] = {}
        self._turn: Dict[int, int] = {}

    @classmethod
    def from_yuv420(cls, pairs, bit_depth=None, **kw) -> "DeviceClipSampler":
        """pairs: (lr_path, hr_path) of I420 files named ``Name_WxH_NF.yuv``; the Y planes become one-channel sequences.
        bit_depth: 8 (one byte per sample), 10 (two bytes, little-endian, uint16 sequences) or None: read off each file name
        (`harness.yuv.yuv_bit_depth`, the ``_10bit`` token); then both files of a pair and all pairs must agree (ValueError)."""
        from ..harness.yuv import parse_yuv_name, read_yuv420, yuv_bit_depth
        if bit_depth is None:
            depths = [(yuv_bit_depth(lr_path), yuv_bit_depth(hr_path)) for lr_path, hr_path in pairs]
            for (lr_path, hr_path), (a, b) in zip(pairs, depths):
                if a != b:
                    raise ValueError(f"{lr_path} names {a}-bit samples, {hr_path} {b}-bit: both files of a pair must agree")
                if a != depths[0][0]:
                    raise ValueError(f"{lr_path} names {a}-bit samples, {pairs[0][0]} {depths[0][0]}-bit: all pairs must agree")
            bit_depth = depths[0][0] if depths else 8
        elif bit_depth not in (8, 10):
            raise ValueError(f"bit_depth must be 8, 10 or None, got {bit_depth!r}")
        seqs = []
        for lr_path, hr_path in pairs:
            planes = []
            for path in (lr_path, hr_path):
                n = parse_yuv_name(path)
                y = read_yuv420(path, n.width, n.height, n.frames, bit_depth=bit_depth)[0]
                planes.append(np.ascontiguousarray(y, dtype=y.dtype.newbyteorder("="))[:, None])
            seqs.append(tuple(planes))
        return cls(seqs, **kw)

    @classmethod
    def from_yuv420_rgb(cls, pairs, colour=None, **kw) -> "DeviceClipSampler":
        """pairs: (lr_path, hr_path) of I420 files named ``Name_WxH_NF.yuv``, for the RGB models: every file is uploaded as it is
        and decoded once on the device to planar RGB (`harness.colour.yuv420_to_rgb`), so the sequences are 3-channel and `fit`
        trains an RGB twin from them unchanged.  colour: a `harness.colour.ColourSpec` (matrix, range, chroma siting, bit depth),
        or None: BT.709, limited range, left-sited chroma, the bit depth read off the file names under the rules of `from_yuv420`.
        device: as the constructor's (the decode runs there)."""
        from ..harness.colour import ColourSpec, i420_planes, yuv420_to_rgb
        from ..harness.yuv import _map_frames, parse_yuv_name, yuv_bit_depth
        if colour is None:
            depths = [(yuv_bit_depth(lr_path), yuv_bit_depth(hr_path)) for lr_path, hr_path in pairs]
            for (lr_path, hr_path), (a, b) in zip(pairs, depths):
                if a != b:
                    raise ValueError(f"{lr_path} names {a}-bit samples, {hr_path} {b}-bit: both files of a pair must agree")
                if a != depths[0][0]:
                    raise ValueError(f"{lr_path} names {a}-bit samples, {pairs[0][0]} {depths[0][0]}-bit: all pairs must agree")
            colour = ColourSpec(bit_depth=depths[0][0] if depths else 8)
        elif not isinstance(colour, ColourSpec):
            raise ValueError(f"colour must be a ColourSpec or None, got {type(colour).__name__}")
        device = torch.device(kw.get("device", "cpu"))
        if device.type != "cuda":
            raise RuntimeError("from_yuv420_rgb decodes on the HIP device only (there is no CPU fallback; "
                               "harness.colour.yuv420_to_rgb_host is the CPU specification)")
        seqs = []
        for lr_path, hr_path in pairs:
            frames = []
            for path in (lr_path, hr_path):
                n = parse_yuv_name(path)
                mm = _map_frames(path, n.width, n.height, n.frames, bit_depth=colour.bit_depth)
                host = torch.from_numpy(np.array(mm, dtype=mm.dtype.newbyteorder("=")))
                dev = hip.bits16(host).to(device).view(colour.dtype)
                frames.append(yuv420_to_rgb(*i420_planes(dev, n.height, n.width), colour))
            seqs.append(tuple(frames))
        return cls(seqs, **kw)

    def __len__(self) -> int:
        return len(self.shapes)

    def plan(self, epoch: int) -> List[BatchPlan]:
        """This rank's batches of `epoch` as draw records: pure host work, no GPU."""
        if not (0 <= epoch < 2 ** 32):
            raise ValueError(f"epoch must be in [0, 2**32), got {epoch}")
        return make_plan(self.shapes, epoch, batch=self.batch, crop=self.crop, frames=self.frames, seed=self.seed,
                         start=self.start, rank=self.rank, world=self.world)

    def _slot(self, planes: int):
        ring = self._rings.setdefault(planes, [])
        turn = self._turn.get(planes, 0)
        self._turn[planes] = (turn + 1) % _RING
        if len(ring) <= turn:
            host = torch.empty(planes * _DESC.itemsize, dtype=torch.uint8).pin_memory()
            ring.append((host, torch.empty(planes * _DESC.itemsize, dtype=torch.uint8, device=self.device), torch.cuda.Event()))
        else:
            ring[turn][2].synchronize()
        return ring[turn]

    def _check(self, bp: BatchPlan):
        item, first, top, left = (np.asarray(a, dtype=np.int64) for a in (bp.item, bp.first, bp.top, bp.left))
        if not (len(item) and len(item) == len(first) == len(top) == len(left) == len(bp.hflip) == len(bp.vflip) == len(bp.rot90)):
            raise ValueError("a batch plan needs at least one clip and arrays of one length")
        if item.min() < 0 or item.max() >= len(self.shapes):
            raise ValueError(f"item outside [0, {len(self.shapes)})")
        N, H, W = self._N[item], self._H[item], self._W[item]
        if (first < 0).any() or (first + self.frames > N).any():
            raise ValueError("window outside its sequence")
        if (top < 0).any() or (left < 0).any() or (top + self.crop > H).any() or (left + self.crop > W).any():
            raise ValueError("crop outside its frame")
        return item, first, top, left, H, W

    def build(self, bp: BatchPlan) -> Dict[str, torch.Tensor]:
        """The device batch of one plan record (every window is checked against its sequence on the host, before any launch)."""
        item, first, top, left, H, W = self._check(bp)
        b, F, C, s = len(item), self.frames, self.channels, self.crop
        flags = (np.asarray(bp.hflip, dtype=bool) * hip.CROP_HFLIP + np.asarray(bp.vflip, dtype=bool) * hip.CROP_VFLIP
                 + np.asarray(bp.rot90, dtype=bool) * hip.CROP_TRANSPOSE).astype(np.int32)
        n_lr, n_hr = b * F * C, b * C
        with torch.cuda.device(self.device):
            host, dev, event = self._slot(n_lr + n_hr)
            fill_descs(host.numpy().view(_DESC), self._lr_ptr[item], self._hr_ptr[item], first, top, left, flags, H, W, F, C,
                       itemsize=self.dtype.itemsize)
            dev.copy_(host, non_blocking=True)
            frames = torch.empty((b, F, C, s, s), dtype=torch.float32, device=self.device)           # the model's layout
            target = torch.empty((b, C, 1, 4 * s, 4 * s), dtype=torch.float32, device=self.device)
            hip.clip_batch(dev[:n_lr * _DESC.itemsize], s, frames, dtype=self.dtype)
            hip.clip_batch(dev[n_lr * _DESC.itemsize:], 4 * s, target, dtype=self.dtype)
            event.record()
        return {"lr_imgs": frames.permute(0, 2, 1, 3, 4), "hr_imgs": target}

    def __call__(self, epoch: int) -> Iterator[Dict[str, torch.Tensor]]:
        for bp in self.plan(epoch):
            yield self.build(bp)
