"""GPU: the 2-byte clip-batch kernel (csrc/clip_batch.hip, fcvsr_clip_batch_u16) and DeviceClipSampler on uint16 (10-bit) sequences
against `apply_plan_host`.  The reference handles 8-bit frames only: the specification is the project's float contract for 10-bit
frames, ``min(k, 1023).float() / 1023``.  The kernel does nothing but a table look-up, so every comparison is torch.equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_OF_RANGE = np.array([1024, 4095, 32767, 32768, 65535], dtype=np.uint16)


def frames_u16(rs, shape):
    """Samples uniform in [0, 1024), about 5 % of them replaced by values above the 10-bit range: pins the index clamp and a
    sign-extension slip through the int16 views."""
    a = rs.randint(0, 1024, shape).astype(np.uint16)
    hit = rs.random_sample(shape) < 0.05
    a[hit] = OUT_OF_RANGE[rs.randint(0, len(OUT_OF_RANGE), int(hit.sum()))]
    return a


def _seq(seed, n, c, h, w):
    rs = np.random.RandomState(seed)
    return frames_u16(rs, (n, c, h, w)), frames_u16(rs, (n, c, 4 * h, 4 * w))


def _to_dev(a):
    """A uint16 numpy array on the device as a torch.uint16 tensor (uploaded as int16 bits)."""
    return torch.from_numpy(a).view(torch.int16).to(DEV).view(torch.uint16)


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
    """Run hip.clip_batch(dtype=torch.uint16) on hand-made descriptors: pairs = device (N,C,H,W) uint16 tensors of any strides,
    rows = (tensor index, frame, channel, top, left, flags) per output plane in LR units; scale 1 reads them as given, 4 as the HR
    planes.  pitch / top / left are in samples."""
    from fcvsr_amd import hip
    d = np.zeros(len(rows), dtype=np.dtype(hip.CropDesc))
    for i, (t, f, c, top, left, flags) in enumerate(rows):
        x = pairs[t]
        assert x.dtype == torch.uint16 and x.stride(3) == 1
        assert 0 <= top * scale and top * scale + s <= x.shape[2] and 0 <= left * scale and left * scale + s <= x.shape[3]   # in bounds
        d[i] = (x[f, c].data_ptr(), x.stride(2), top * scale, left * scale, flags)
    desc = torch.from_numpy(d.view(np.uint8)).to(DEV)
    out = torch.empty((len(rows), s, s), dtype=torch.float32, device=DEV)
    hip.clip_batch(desc, s, out, dtype=torch.uint16)
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
    return torch.from_numpy(np.minimum(a, 1023).astype(np.int32)).float() / 1023.0


@pytest.mark.parametrize("s", [16, 64, 128])
@pytest.mark.parametrize("C", [1, 3])
def test_build_equals_host_chain_for_every_flag_combination_and_border(s, C):
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    H, W = s + 9, s + 21
    seqs = [_seq(10 + s + C, 9, C, H, W)]
    sampler = DeviceClipSampler(seqs, batch=8, crop=s, seed=0, device=DEV)
    assert sampler.dtype == torch.uint16 and sampler.bit_depth == 10
    rows = [(0, fl % 3, (3 * fl) % (H - s), (5 * fl) % (W - s), fl & 1, fl & 2, fl & 4) for fl in range(8)]
    _same(sampler.build(_plan(rows)), apply_plan_host(seqs, _plan(rows), s))
    # crops touching each border: the first and the last corner the sampler can draw
    rows = [(0, 2, 0, 7, 1, 0, 1), (0, 0, 4, 0, 0, 1, 1), (0, 1, H - s - 1, 2, 1, 1, 0), (0, 2, 3, W - s - 1, 0, 0, 1),
            (0, 0, 0, 0, 0, 0, 0), (0, 2, H - s - 1, W - s - 1, 1, 1, 1)]
    got = sampler.build(_plan(rows))
    _same(got, apply_plan_host(seqs, _plan(rows), s))
    assert got["lr_imgs"].shape == (6, C, 7, s, s) and got["hr_imgs"].shape == (6, C, 1, 4 * s, 4 * s)
    assert got["lr_imgs"].permute(0, 2, 1, 3, 4).is_contiguous() and got["hr_imgs"].is_contiguous()


def test_uint8_sampler_reports_its_depth_and_is_unchanged():
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    rs = np.random.RandomState(1)
    seqs = [(rs.randint(0, 256, (8, 1, 30, 41)).astype(np.uint8), rs.randint(0, 256, (8, 1, 120, 164)).astype(np.uint8))]
    sampler = DeviceClipSampler(seqs, batch=2, crop=16, seed=0, device=DEV)
    assert sampler.dtype == torch.uint8 and sampler.bit_depth == 8
    rows = [(0, 1, 3, 5, 1, 0, 1), (0, 0, 13, 24, 0, 1, 0)]
    _same(sampler.build(_plan(rows)), apply_plan_host(seqs, _plan(rows), 16))


def test_kernel_reads_an_odd_row_pitch_and_a_plane_that_is_not_dword_aligned():
    """W = 57 samples (rows alternate between 0 and 2 mod 4), and planes that begin one row into an allocation (2 mod 4): windows of
    strided views, odd and even `left`, at LR and HR scale."""
    rs = np.random.RandomState(5)
    base_lr, base_hr = frames_u16(rs, (4, 2, 42, 57)), frames_u16(rs, (4, 2, 165, 229))
    lr_d, hr_d = _to_dev(base_lr), _to_dev(base_hr)
    lr_v, hr_v = lr_d[:, :, 1:], hr_d[:, :, 1:]                       # plane pointers offset by one 114- / 458-byte row
    assert lr_v[0, 0].data_ptr() % 4 == 2 and lr_v.stride(2) == 57
    assert hr_v[0, 0].data_ptr() % 4 == 2 and hr_v.stride(2) == 229
    s = 16
    rows = [(0, f, c, top, left, fl) for fl in range(8) for (f, c, top, left) in [(fl % 4, fl % 2, (2 * fl) % 25, (37 * fl + 1) % 41)]]
    rows += [(0, 3, 1, 24, 40, 5), (0, 0, 0, 0, 0, 6), (0, 1, 1, 24, 0, 3), (0, 2, 0, 0, 40, 7), (0, 1, 0, 5, 13, 0), (0, 2, 1, 6, 8, 4)]
    assert {r[4] % 2 for r in rows} == {0, 1}
    got = _planes([lr_v], rows, s, 1)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_lr[:, :, 1:], f, c, top, left, fl, s)), rows[i]
    got = _planes([hr_v], rows, 4 * s, 4)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_hr[:, :, 1:], f, c, 4 * top, 4 * left, fl, 4 * s)), rows[i]
    # the HR planes that belong to W = 57: 228 samples a row, every row 0 mod 4
    base_hr4 = frames_u16(rs, (4, 2, 165, 228))
    hr4_v = _to_dev(base_hr4)[:, :, 1:]
    assert hr4_v[0, 0].data_ptr() % 4 == 0 and hr4_v.stride(2) == 228
    got = _planes([hr4_v], rows, 4 * s, 4)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_hr4[:, :, 1:], f, c, 4 * top, 4 * left, fl, 4 * s)), rows[i]
    # odd `left` at HR scale too: the windows of the LR rows read from the HR planes as they are
    got = _planes([hr_v], rows, s, 1)
    for i, (t, f, c, top, left, fl) in enumerate(rows):
        assert torch.equal(got[i], _host_plane(base_hr[:, :, 1:], f, c, top, left, fl, s)), rows[i]


def test_kernel_handles_plane_sizes_that_are_not_whole_tiles():
    """s = 4 .. 132: partial 64 x 64 tiles in both axes, all 8 flag combinations."""
    rs = np.random.RandomState(6)
    x = frames_u16(rs, (2, 1, 150, 171))
    x_d = _to_dev(x)
    for s in (4, 20, 68, 132):
        rows = [(0, fl % 2, 0, (3 * fl) % (150 - s), (7 * fl) % (171 - s), fl) for fl in range(8)]
        got = _planes([x_d], rows, s, 1)
        for i, (t, f, c, top, left, fl) in enumerate(rows):
            assert torch.equal(got[i], _host_plane(x, f, c, top, left, fl, s)), (s, rows[i])


def test_samples_above_the_10_bit_range_read_as_one_and_lr_planes_are_the_table():
    """Every sample above 1023 in a crop reads as exactly 1.0, and the LR planes of a batch are `hip.u16_table(dev)[min(k, 1023)]`:
    the floats `super_resolve_u16` feeds the network for the same samples."""
    from fcvsr_amd import hip
    from fcvsr_amd.train import DeviceClipSampler
    lr, hr = _seq(7, 8, 1, 40, 52)
    lr[2, 0, 5:9, 7:13] = OUT_OF_RANGE[np.arange(24) % 5].reshape(4, 6)
    sampler = DeviceClipSampler([(lr, hr)], batch=2, crop=32, seed=0, device=DEV)
    got = sampler.build(_plan([(0, 0, 3, 4, 0, 0, 0), (0, 1, 7, 19, 0, 0, 0)]))
    table = hip.u16_table(torch.device(DEV)).cpu()
    assert table.shape == (1024,) and float(table[1023]) == 1.0
    for k, (first, top, left) in enumerate(((0, 3, 4), (1, 7, 19))):
        win = lr[first:first + 7, 0, top:top + 32, left:left + 32]
        idx = torch.from_numpy(np.minimum(win, 1023).astype(np.int64))
        planes = got["lr_imgs"][k, 0].cpu()
        assert torch.equal(planes, table[idx])
        over = torch.from_numpy(win > 1023)
        assert over.any() and bool((planes[over] == 1.0).all())
        assert float(planes.max()) == 1.0 and float(planes.min()) >= 0.0
    win = hr[3:4, 0, 12:140, 16:144]
    assert torch.equal(got["hr_imgs"][0, 0].cpu(), table[torch.from_numpy(np.minimum(win, 1023).astype(np.int64))])


def test_entry_point_rejects_bad_arguments():
    from fcvsr_amd import hip
    n = np.dtype(hip.CropDesc).itemsize
    desc = torch.zeros(n, dtype=torch.uint8, device=DEV)
    u16 = dict(dtype=torch.uint16)
    with pytest.raises(ValueError):
        hip.clip_batch(desc, 16, torch.empty(255, device=DEV), **u16)
    with pytest.raises(ValueError):
        hip.clip_batch(desc[:n - 1], 16, torch.empty(256, device=DEV), **u16)
    with pytest.raises(hip.HipError, match="multiple of 4"):
        hip.clip_batch(desc, 6, torch.empty(36, device=DEV), **u16)
    with pytest.raises(hip.HipError, match="16-byte"):
        hip.clip_batch(desc, 4, torch.empty(20, device=DEV)[1:17], **u16)
    with pytest.raises(RuntimeError):
        hip.clip_batch(desc.cpu(), 4, torch.empty(16, device=DEV), **u16)
    with pytest.raises(ValueError, match="dtype"):
        hip.clip_batch(desc, 4, torch.empty(16, device=DEV), dtype=torch.int16)


def test_one_batch_mixes_sequences_of_different_frame_sizes():
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    seqs = [_seq(1, 8, 1, 40, 56), _seq(2, 11, 1, 33, 71), _seq(3, 7, 1, 90, 30)]
    given = [seqs[0], (torch.from_numpy(seqs[1][0]), torch.from_numpy(seqs[1][1])), (_to_dev(seqs[2][0]), _to_dev(seqs[2][1]))]
    sampler = DeviceClipSampler(given, batch=4, crop=16, seed=1, device=DEV)      # numpy, host tensors and device tensors
    rows = [(1, 4, 16, 54, 1, 0, 1), (0, 1, 23, 0, 0, 1, 0), (2, 0, 73, 13, 1, 1, 1), (1, 0, 0, 0, 0, 0, 1), (0, 0, 5, 39, 1, 1, 0)]
    _same(sampler.build(_plan(rows)), apply_plan_host(seqs, _plan(rows), 16))
    with pytest.raises(ValueError):                    # windows are checked on the host before any launch
        sampler.build(_plan([(1, 5, 0, 0, 0, 0, 0)]))
    with pytest.raises(ValueError):
        sampler.build(_plan([(2, 0, 75, 0, 0, 0, 0)]))
    with pytest.raises(ValueError):
        sampler.build(_plan([(0, 0, 0, 41, 0, 0, 0)]))
    with pytest.raises(ValueError):
        sampler.build(_plan([(3, 0, 0, 0, 0, 0, 0)]))


def test_from_yuv420_on_10_bit_files_equals_a_sampler_of_the_y_planes(tmp_path):
    from fcvsr_amd.harness.yuv import write_yuv420
    from fcvsr_amd.train import DeviceClipSampler
    rs = np.random.RandomState(8)
    pairs, seqs = [], []
    for name, n, h, w in (("Alpha_fps30", 9, 36, 48), ("Beta", 8, 40, 44)):
        planes = []
        for k, tag in ((1, "lr"), (4, "hr")):
            y = frames_u16(rs, (n, k * h, k * w))
            u, v = (frames_u16(rs, (n, k * h // 2, k * w // 2)) for _ in range(2))
            path = str(tmp_path / f"{name}_{tag}_{k * w}x{k * h}_{n}F_10bit.yuv")
            write_yuv420(path, y, u, v)
            planes.append((path, y[:, None]))
        pairs.append((planes[0][0], planes[1][0]))
        seqs.append((planes[0][1], planes[1][1]))
    kw = dict(batch=2, crop=16, seed=4, device=DEV)
    a, b = DeviceClipSampler.from_yuv420(pairs, **dict(kw, device="cuda")), DeviceClipSampler(seqs, **kw)     # "cuda": the current device
    assert a.shapes == b.shapes and a.channels == 1 and a.device == b.device and a.bit_depth == 10 == b.bit_depth
    c = DeviceClipSampler.from_yuv420(pairs, bit_depth=10, **kw)
    for x, y, z in zip(a(3), b(3), c(3)):
        assert torch.equal(x["lr_imgs"], y["lr_imgs"]) and torch.equal(x["hr_imgs"], y["hr_imgs"])
        assert torch.equal(z["lr_imgs"], y["lr_imgs"]) and torch.equal(z["hr_imgs"], y["hr_imgs"])


def _reduced_model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    kw = dict(n_features=32, ACNum=2, Freq_Inv=2, SCGroupN=1)
    m = GShiftNet_S(**kw)
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S", **kw), gain=0.5), strict=True)
    return m.cuda()


def test_fit_takes_the_uint16_sampler_and_its_first_step_equals_the_host_chain():
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


def test_fit_validates_on_uint16_sequences_at_peak_1023():
    from fcvsr_amd.harness.infer import evaluate_sequence
    from fcvsr_amd.train import DeviceClipSampler
    from fcvsr_amd.train.step import fit, validate
    seqs = [_seq(50 + i, 8, 1, 30, 34) for i in range(2)]
    sampler = DeviceClipSampler(seqs, batch=2, crop=16, seed=3, device=DEV)
    rs = np.random.RandomState(9)
    lr_u16, hr_u16 = torch.from_numpy(frames_u16(rs, (3, 1, 16, 20))), torch.from_numpy(frames_u16(rs, (3, 1, 64, 80)))
    seen = []
    model = _reduced_model()
    fit(model, sampler, epochs=1, device=DEV, log=lambda m: None, val_sequences=[(lr_u16, hr_u16)],
        on_validate=lambda e, p, q: seen.append((e, p, q)))
    assert len(seen) == 1 and seen[0][0] == 1
    want = evaluate_sequence(model, lr_u16, hr_u16)
    assert np.isfinite(seen[0][1]) and np.isfinite(seen[0][2])
    assert seen[0][1] == want.psnr_mean and seen[0][2] == want.ssim_mean
    # float lr against uint16 hr: quantised and scored at hr's peak
    lr_f = lr_u16.to(torch.int32).clamp(max=1023).float() / 1023.0
    p, q = validate(model, [(lr_f, hr_u16)])
    want = evaluate_sequence(model, lr_f, hr_u16)
    assert np.isfinite(p) and np.isfinite(q) and p == want.psnr_mean and q == want.ssim_mean


def test_batches_queued_back_to_back_keep_their_descriptors():
    """More batches than the descriptor ring holds, queued with no host synchronisation in between: every batch still has the
    values of its own plan (12 batches, crop 64)."""
    from fcvsr_amd.train import DeviceClipSampler, apply_plan_host
    seqs = [_seq(60 + i, 8, 1, 70, 81) for i in range(12)]
    a = DeviceClipSampler(seqs, batch=2, crop=64, seed=5, device=DEV)
    plans = [p for e in (0, 1) for p in a.plan(e)]
    assert len(plans) == 12
    it = (x for e in (0, 1) for x in a(e))
    got = [next(it) for _ in plans]                                       # 12 batches in flight, nothing waited for
    torch.cuda.synchronize()
    for bp, g in zip(plans, got):
        _same(g, apply_plan_host(seqs, bp, 64))
