"""GPU: the clip-batch kernel (csrc/clip_batch.hip) and DeviceClipSampler against `apply_plan_host`, the reference transform chain
on the CPU.  The kernel does nothing but a table look-up, so every comparison is bit for bit (torch.equal)."""
import os
import random

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _seq(seed, n, c, h, w):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n, c, h, w)).astype(np.uint8), rs.randint(0, 256, (n, c, 4 * h, 4 * w)).astype(np.uint8)


def _plan(rows):
    """rows: (item, first, top, left, hflip, vflip, rot90) per clip."""
    from fcvsr_amd.train import BatchPlan
    cols = list(zip(*rows))
    return BatchPlan(*(np.asarray(c, dtype=np.int64) for c in cols[:4]), *(np.asarray(c, dtype=bool) for c in cols[4:]))


def _same(dev_batch, host_batch):
    for k in ("lr_imgs", "hr_imgs"):
        assert dev_batch[k].is_cuda and dev_batch[k].dtype == torch.float32
        assert dev_batch[k].shape == host_batch[k].shape, (k, dev_batch[k].shape, host_batch[k].shape)
        assert torch.equal(dev_batch[k].cpu(), host_batch[k]), k


def _planes(pairs, rows, s, scale):
    """Run hip.clip_batch on hand-made descriptors: pairs = device (N,C,H,W) uint8 tensors of any strides, rows = (tensor index, frame,
    channel, top, left, flags) per output plane in LR units; scale 1 reads them as given, 4 as the HR planes."""
    from fcvsr_amd import hip
    d = np.zeros(len(rows), dtype=np.dtype(hip.CropDesc))
    for i, (t, f, c, top, left, flags) in enumerate(rows):
        x = pairs[t]
        assert x.stride(3) == 1 and 0 <= top * scale and (top + s // scale) * scale <= x.shape[2] and (left + s // scale) * scale <= x.shape[3]
        d[i] = (x[f, c].data_ptr(), x.stride(2), top * scale, left * scale, flags)
    desc = torch.from_numpy(d.view(np.uint8)).to(DEV)
    out = torch.empty((len(rows), s, s), dtype=torch.float32, device=DEV)
    hip.clip_batch(desc, s, out)
    torch.cuda.synchronize()
    return out.cpu()


def _host_plane(x, f, c, top, left, flags, s):
    a = x[f, c, top:top + s, left:left + s]
    if flags & 1:
        a = a[:, ::-1]
    if flags & 2:
        a = a[::-1]
    if flags & 4:
        a = a.T
    return torch.from_numpy(a.copy()).float() / 255.0


@pytest.mark.parametrize("s", [16, 64, 128])
@pytest.mark.parametrize("C", [1, 3])
def test_build_equals_host_chain_for_every_flag_combination_and_border(s, C):
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    H, W = s + 9, s + 21
    seqs = [_seq(10 + s + C, 9, C, H, W)]
    sampler = DeviceClipSampler(seqs, batch=8, crop=s, seed=0, device=DEV)
    rows = [(0, fl % 3, (3 * fl) % (H - s), (5 * fl) % (W - s), fl & 1, fl & 2, fl & 4) for fl in range(8)]
    _same(sampler.build(_plan(rows)), apply_plan_host(seqs, _plan(rows), s))
    # crops touching each border: the first and the last corner the reference can draw
    rows = [(0, 2, 0, 7, 1, 0, 1), (0, 0, 4, 0, 0, 1, 1), (0, 1, H - s - 1, 2, 1, 1, 0), (0, 2, 3, W - s - 1, 0, 0, 1),
            (0, 0, 0, 0, 0, 0, 0), (0, 2, H - s - 1, W - s - 1, 1, 1, 1)]
    got = sampler.build(_plan(rows))
    _same(got, apply_plan_host(seqs, _plan(rows), s))
    assert got["lr_imgs"].shape == (6, C, 7, s, s) and got["hr_imgs"].shape == (6, C, 1, 4 * s, 4 * s)
    assert got["lr_imgs"].permute(0, 2, 1, 3, 4).is_contiguous() and got["hr_imgs"].is_contiguous()


def test_kernel_reads_an_odd_row_pitch_and_an_unaligned_plane():
    """W = 57 rows (no alignment of any row), and planes that begin one row into an allocation: windows of strided views."""
    rs = np.random.RandomState(5)
    base_lr, base_hr = rs.randint(0, 256, (4, 2, 42, 57)).astype(np.uint8), rs.randint(0, 256, (4, 2, 165, 228)).astype(np.uint8)
    lr_d, hr_d = torch.from_numpy(base_lr).to(DEV), torch.from_numpy(base_hr).to(DEV)
    lr_v, hr_v = lr_d[:, :, 1:], hr_d[:, :, 1:]                       # plane pointers offset by one 57- / 228-byte row
    assert lr_v[0, 0].data_ptr() % 4 == 1 and lr_v.stride(2) == 57
    s = 16
    rows = [(0, f, c, top, left, fl) for fl in range(8) for (f, c, top, left) in [(fl % 4, fl % 2, (2 * fl) % 25, (37 * fl + 1) % 41)]]
    rows += [(0, 3, 1, 24, 40, 5), (0, 0, 0, 0, 0, 6), (0, 1, 1, 24, 0, 3), (0, 2, 0, 0, 40, 7)]
    got = _planes([lr_v], rows, s, 1)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_lr[:, :, 1:], f, c, top, left, fl, s)), rows[i]
    got = _planes([hr_v], rows, 4 * s, 4)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_hr[:, :, 1:], f, c, 4 * top, 4 * left, fl, 4 * s)), rows[i]


def test_kernel_handles_plane_sizes_that_are_not_whole_tiles():
    """s = 4 .. 132: partial 64 x 64 tiles in both axes, with and without transpose."""
    rs = np.random.RandomState(6)
    x = rs.randint(0, 256, (2, 1, 150, 171)).astype(np.uint8)
    x_d = torch.from_numpy(x).to(DEV)
    for s in (4, 20, 68, 132):
        rows = [(0, fl % 2, 0, (3 * fl) % (150 - s), (7 * fl) % (171 - s), fl) for fl in range(8)]
        got = _planes([x_d], rows, s, 1)
        for i, (t, f, c, top, left, fl) in enumerate(rows):
            assert torch.equal(got[i], _host_plane(x, f, c, top, left, fl, s)), (s, rows[i])


def test_entry_point_rejects_bad_arguments():
    from fcvsr_amd import hip
    n = np.dtype(hip.CropDesc).itemsize
    desc = torch.zeros(n, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        hip.clip_batch(desc, 16, torch.empty(255, device=DEV))
    with pytest.raises(ValueError):
        hip.clip_batch(desc[:n - 1], 16, torch.empty(256, device=DEV))
    with pytest.raises(hip.HipError, match="multiple of 4"):
        hip.clip_batch(desc, 6, torch.empty(36, device=DEV))
    with pytest.raises(hip.HipError, match="16-byte"):
        hip.clip_batch(desc, 4, torch.empty(20, device=DEV)[1:17])
    with pytest.raises(RuntimeError):
        hip.clip_batch(desc.cpu(), 4, torch.empty(16, device=DEV))


def test_one_batch_mixes_sequences_of_different_frame_sizes():
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    seqs = [_seq(1, 8, 1, 40, 56), _seq(2, 11, 1, 33, 71), _seq(3, 7, 1, 90, 30)]
    sampler = DeviceClipSampler(seqs, batch=4, crop=16, seed=1, device=DEV)
    rows = [(1, 4, 16, 54, 1, 0, 1), (0, 1, 23, 0, 0, 1, 0), (2, 0, 73, 13, 1, 1, 1), (1, 0, 0, 0, 0, 0, 1), (0, 0, 5, 39, 1, 1, 0)]
    _same(sampler.build(_plan(rows)), apply_plan_host(seqs, _plan(rows), 16))
    with pytest.raises(ValueError):                    # windows are checked on the host before any launch
        sampler.build(_plan([(1, 5, 0, 0, 0, 0, 0)]))
    with pytest.raises(ValueError):
        sampler.build(_plan([(2, 0, 75, 0, 0, 0, 0)]))
    with pytest.raises(ValueError):
        sampler.build(_plan([(3, 0, 0, 0, 0, 0, 0)]))


@pytest.mark.parametrize("world", [1, 2])
def test_sampler_epochs_equal_the_host_chain_of_their_plan(world):
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    seqs = [_seq(20 + i, 9 + i, 1, 36 + 3 * i, 50 - 2 * i) for i in range(5)]
    for rank in range(world):
        sampler = DeviceClipSampler(seqs, batch=2, crop=16, seed=9, rank=rank, world=world, device=DEV)
        for epoch in (0, 1):
            plans = sampler.plan(epoch)
            batches = list(sampler(epoch))
            assert len(batches) == len(plans) == (3 if world == 1 else 2)
            for bp, got in zip(plans, batches):
                _same(got, apply_plan_host(seqs, bp, 16))
                assert got["lr_imgs"].permute(0, 2, 1, 3, 4).is_contiguous()
                assert got["lr_imgs"].device == torch.device(DEV) and got["hr_imgs"].device == torch.device(DEV)


def test_device_reproduces_the_reference_loader_fixture():
    """loader_transforms.npz (outputs of the reference's RandomCrop / Augment / ToTensor) on the device: a one-item sampler, the
    draws of each trial injected."""
    from fcvsr_amd.train import BatchPlan, DeviceClipSampler
    g = np.load(os.path.join(GOLDEN_DIR, "loader_transforms.npz"))
    lr, hr, crop = g["lr"], g["hr"], int(g["crop"])
    sampler = DeviceClipSampler([(lr[:, None], np.repeat(hr, 7, 0)[:, None])], batch=1, crop=crop, seed=0, device=DEV)
    for i, t in enumerate(g["seeds"]):
        rs, rnd = np.random.RandomState(int(t)), random.Random(int(t))
        top, left = rs.randint(0, lr.shape[1] - crop), rs.randint(0, lr.shape[2] - crop)
        flips = [rnd.random() < 0.5 for _ in range(3)]
        got = sampler.build(BatchPlan(np.array([0]), np.array([0]), np.array([top]), np.array([left]), *(np.array([f]) for f in flips)))
        assert torch.equal(got["lr_imgs"][0].cpu(), torch.from_numpy(g["lr_out"][i])), f"trial {t}"
        assert torch.equal(got["hr_imgs"][0].cpu(), torch.from_numpy(g["hr_out"][i])), f"trial {t}"


def test_from_yuv420_equals_a_sampler_of_the_y_planes(tmp_path):
    from fcvsr_amd.harness.yuv import write_yuv420
    from fcvsr_amd.train import DeviceClipSampler
    rs = np.random.RandomState(8)
    pairs, seqs = [], []
    for name, n, h, w in (("Alpha_fps30", 9, 36, 48), ("Beta", 8, 40, 44)):
        planes = []
        for k, tag in ((1, "lr"), (4, "hr")):
            y = rs.randint(0, 256, (n, k * h, k * w)).astype(np.uint8)
            u, v = (rs.randint(0, 256, (n, k * h // 2, k * w // 2)).astype(np.uint8) for _ in range(2))
            path = str(tmp_path / f"{name}_{tag}_{k * w}x{k * h}_{n}F.yuv")
            write_yuv420(path, y, u, v)
            planes.append((path, y[:, None]))
        pairs.append((planes[0][0], planes[1][0]))
        seqs.append((planes[0][1], planes[1][1]))
    kw = dict(batch=2, crop=16, seed=4, device=DEV)
    a, b = DeviceClipSampler.from_yuv420(pairs, **dict(kw, device="cuda")), DeviceClipSampler(seqs, **kw)     # "cuda": the current device
    assert a.shapes == b.shapes and a.channels == 1 and a.device == b.device
    for x, y in zip(a(3), b(3)):
        assert torch.equal(x["lr_imgs"], y["lr_imgs"]) and torch.equal(x["hr_imgs"], y["hr_imgs"])


def _reduced_model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    kw = dict(n_features=32, ACNum=2, Freq_Inv=2, SCGroupN=1)
    m = GShiftNet_S(**kw)
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S", **kw), gain=0.5), strict=True)
    return m.cuda()


def test_fit_takes_the_sampler_and_its_first_step_equals_the_host_chain():
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    from fcvsr_amd.train.step import fit
    seqs = [_seq(40 + i, 8, 1, 30, 34) for i in range(3)]
    sampler = DeviceClipSampler(seqs, batch=4, crop=16, seed=2, device=DEV)
    assert [len(sampler.plan(e)) for e in (0, 1)] == [1, 1]              # one batch per epoch: history[0] is the first step's loss
    hist = fit(_reduced_model(), sampler, epochs=2, device=DEV, log=lambda m: None)
    assert len(hist) == 2 and all(np.isfinite(h) for h in hist)

    def host_batches(epoch):
        for bp in sampler.plan(epoch):
            yield apply_plan_host(seqs, bp, 16)

    hist2 = fit(_reduced_model(), host_batches, epochs=2, device=DEV, log=lambda m: None)
    assert hist[0] == hist2[0], (hist, hist2)


def test_batches_queued_back_to_back_keep_their_descriptors():
    """Two samplers on one stream, many batches queued with no host synchronisation in between (more than the descriptor ring
    holds): every batch still has the values of its own plan."""
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    seqs = [_seq(60 + i, 10, 1, 150, 170) for i in range(12)]
    a = DeviceClipSampler(seqs, batch=2, crop=64, seed=5, device=DEV)
    b = DeviceClipSampler(seqs, batch=2, crop=64, seed=6, device=DEV)
    plans = [(pa, pb) for e in (0, 1) for pa, pb in zip(a.plan(e), b.plan(e))]
    assert len(plans) == 12
    ia = (x for e in (0, 1) for x in a(e))
    ib = (x for e in (0, 1) for x in b(e))
    got = [(next(ia), next(ib)) for _ in plans]                            # 24 batches in flight, nothing waited for
    torch.cuda.synchronize()
    for (pa, pb), (ga, gb) in zip(plans, got):
        _same(ga, apply_plan_host(seqs, pa, 64))
        _same(gb, apply_plan_host(seqs, pb, 64))
