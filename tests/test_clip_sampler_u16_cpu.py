"""Host half of the 10-bit (uint16) device clip sampler, no GPU.  The reference loader handles 8-bit frames only, so the specification
for uint16 sequences is the project's float contract for 10-bit frames, ``min(k, 1023).float() / 1023`` (the table of `hip.u16_table`,
what `super_resolve_u16` feeds the network), applied by `apply_plan_host`.  Every comparison is bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fcvsr_amd.train import BatchPlan, DeviceClipSampler, apply_plan_host
from fcvsr_amd.train import data as D
from fcvsr_amd.train.step import to_tensor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT_OF_RANGE = np.array([1024, 4095, 32767, 32768, 65535], dtype=np.uint16)


def frames_u16(rs, shape):
    """Samples uniform in [0, 1024), about 5 % of them replaced by values above the 10-bit range: pins the index clamp and a
    sign-extension slip through the int16 views (32768 and 65535 are negative as int16)."""
    a = rs.randint(0, 1024, shape).astype(np.uint16)
    hit = rs.random_sample(shape) < 0.05
    a[hit] = OUT_OF_RANGE[rs.randint(0, len(OUT_OF_RANGE), int(hit.sum()))]
    return a


def spec(a):
    """The float contract of 10-bit frames, written out: min(k, 1023) as f32, divided by 1023 in f32 by torch."""
    return torch.from_numpy(np.minimum(a.astype(np.int64), 1023).astype(np.float32)) / 1023.0


def test_to_tensor_on_uint16_is_the_clamped_10_bit_contract_for_every_value():
    k = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    out = to_tensor({"lr_imgs": k, "hr_imgs": k[:, ::-1]})
    want = torch.arange(65536, dtype=torch.int32).clamp(max=1023).float() / 1023
    assert out["lr_imgs"].dtype == torch.float32 and out["lr_imgs"].shape == (1, 1, 256, 256)
    assert torch.equal(out["lr_imgs"].reshape(-1), want)
    assert torch.equal(out["hr_imgs"][0, 0], want.reshape(256, 256).flip(0))
    assert torch.equal(out["lr_imgs"].reshape(-1)[:1024], torch.arange(1024, dtype=torch.int32).float() / 1023)     # hip.u16_table
    assert float(out["lr_imgs"].reshape(-1)[1023:].min()) == 1.0 == float(out["lr_imgs"].max())


def test_to_tensor_on_uint8_is_unchanged():
    k = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    out = to_tensor({"lr_imgs": k, "hr_imgs": k})
    want = torch.arange(256, dtype=torch.uint8).float() / 255.0
    assert torch.equal(out["lr_imgs"].reshape(-1), want) and torch.equal(out["hr_imgs"].reshape(-1), want)
    assert out["lr_imgs"].shape == (1, 1, 16, 16)


def _pair(seed, n, c, h, w):
    rs = np.random.RandomState(seed)
    return frames_u16(rs, (n, c, h, w)), frames_u16(rs, (n, c, 4 * h, 4 * w))


BP = BatchPlan(np.array([1, 0, 1]), np.array([5, 2, 0]), np.array([23, 0, 7]), np.array([0, 14, 5]), np.array([True, False, True]),
               np.array([False, True, True]), np.array([True, True, False]))


def _seqs():
    return [_pair(1, 9, 3, 24, 31), _pair(2, 12, 3, 40, 22)]


def _hand(plane, top, left, s, hflip, vflip, rot):
    a = plane[..., top:top + s, left:left + s]
    if hflip:
        a = a[..., ::-1]
    if vflip:
        a = a[..., ::-1, :]
    if rot:
        a = np.swapaxes(a, -1, -2)
    return spec(np.ascontiguousarray(a))


@pytest.mark.parametrize("as_torch", [False, True])
def test_apply_plan_host_on_uint16_equals_a_hand_written_crop_flip_transpose(as_torch):
    seqs = _seqs()
    assert any((lr > 1023).any() and (lr >= 32768).any() for lr, _ in seqs)
    given = [(torch.from_numpy(lr), torch.from_numpy(hr)) for lr, hr in seqs] if as_torch else seqs
    s, F = 16, 7
    out = apply_plan_host(given, BP, s)
    assert out["lr_imgs"].shape == (3, 3, F, s, s) and out["hr_imgs"].shape == (3, 3, 1, 4 * s, 4 * s)
    assert out["lr_imgs"].dtype == torch.float32 and out["hr_imgs"].dtype == torch.float32
    assert float(out["lr_imgs"].max()) == 1.0 and float(out["lr_imgs"].min()) >= 0.0
    for k in range(3):
        lr, hr = seqs[BP.item[k]]
        first, top, left = int(BP.first[k]), int(BP.top[k]), int(BP.left[k])
        fl = (BP.hflip[k], BP.vflip[k], BP.rot90[k])
        for c in range(3):
            assert torch.equal(out["lr_imgs"][k, c], _hand(lr[first:first + F, c], top, left, s, *fl))
            assert torch.equal(out["hr_imgs"][k, c, 0], _hand(hr[first + F // 2, c], 4 * top, 4 * left, 4 * s, *fl))


def _emulate(d, s):
    """What fcvsr_clip_batch_u16 is specified to compute from one descriptor, read from HOST memory through the pointer: samples
    at src + 2 * ((top + r) * pitch + left + c), pixel k as min(k, 1023) / 1023."""
    assert int(d["src"]) % 2 == 0
    rows = [np.ctypeslib.as_array((ctypes.c_uint16 * s).from_address(int(d["src"]) + 2 * ((int(d["top"]) + r) * int(d["pitch"])
                                                                                        + int(d["left"])))).copy() for r in range(s)]
    a = np.stack(rows)
    if d["flags"] & 1:
        a = a[:, ::-1]
    if d["flags"] & 2:
        a = a[::-1]
    if d["flags"] & 4:
        a = a.T
    return spec(a.copy())


def test_descriptors_of_two_byte_samples_name_the_planes_of_the_host_chain():
    """fill_descs(itemsize=2) over host memory: every LR and HR descriptor's window, read as the kernel is specified to read it, is
    the plane `apply_plan_host` makes; pitch / top / left are in samples, the addresses in bytes."""
    from fcvsr_amd import hip
    seqs = _seqs()
    s, F, C, b = 16, 7, 3, 3
    d = np.zeros(b * F * C + b * C, dtype=np.dtype(hip.CropDesc))
    flags = (BP.hflip * 1 + BP.vflip * 2 + BP.rot90 * 4).astype(np.int32)
    H, W = np.array([seqs[i][0].shape[2] for i in BP.item]), np.array([seqs[i][0].shape[3] for i in BP.item])
    D.fill_descs(d, [seqs[i][0].ctypes.data for i in BP.item], [seqs[i][1].ctypes.data for i in BP.item], BP.first, BP.top, BP.left,
                 flags, H, W, F, C, itemsize=2)
    want = apply_plan_host(seqs, BP, s)
    lr, hr = d[:b * F * C].reshape(b, F, C), d[b * F * C:].reshape(b, C)
    for k in range(b):
        assert (lr[k]["pitch"] == W[k]).all() and (hr[k]["pitch"] == 4 * W[k]).all()                  # samples, not bytes
        assert (lr[k]["top"] == BP.top[k]).all() and (hr[k]["left"] == 4 * BP.left[k]).all()
        for c in range(C):
            assert torch.equal(_emulate(hr[k, c], 4 * s), want["hr_imgs"][k, c, 0])
            for f in range(F):
                assert torch.equal(_emulate(lr[k, f, c], s), want["lr_imgs"][k, c, f])
    # the default is one byte per sample, as before
    d1 = np.zeros_like(d)
    D.fill_descs(d1, [0] * b, [0] * b, BP.first, BP.top, BP.left, flags, H, W, F, C)
    d2 = np.zeros_like(d)
    D.fill_descs(d2, [0] * b, [0] * b, BP.first, BP.top, BP.left, flags, H, W, F, C, itemsize=2)
    assert (d2["src"] == 2 * d1["src"]).all() and d1["src"].max() > 0
    for f in ("pitch", "top", "left", "flags"):
        assert (d1[f] == d2[f]).all()


def _zeros(n=32, c=1, h=40, w=56, dtype=np.uint16):
    return np.zeros((n, c, h, w), dtype), np.zeros((n, c, 4 * h, 4 * w), dtype)


KW = dict(crop=16, frames=7, start="random")


def test_check_sequences_takes_uint16_arrays_and_tensors():
    lr, hr = _zeros()
    for pair in ((lr, hr), (torch.from_numpy(lr), torch.from_numpy(hr)), (lr, torch.from_numpy(hr))):
        out = D.check_sequences([pair, pair], **KW)
        assert len(out) == 2 and all(t.dtype == torch.uint16 and t.dim() == 4 for p in out for t in p)
    out = D.check_sequences([_zeros(dtype=np.uint8)], **KW)
    assert out[0][0].dtype == torch.uint8 and out[0][1].dtype == torch.uint8
    big = D.check_sequences([(lr.astype(">u2"), hr.astype("<u2"))], **KW)                                # any byte order, same values
    assert big[0][0].dtype == torch.uint16


@pytest.mark.parametrize("seqs,word", [
    ([(_zeros()[0], _zeros(dtype=np.uint8)[1])], "uint8"),                     # mixed within a pair
    ([(_zeros(dtype=np.uint8)[0], _zeros()[1])], "uint8"),
    ([_zeros(), _zeros(dtype=np.uint8)], "uint8"),                             # mixed across sequences
    ([_zeros(dtype=np.uint8), _zeros()], "uint8"),
    ([(torch.zeros(32, 1, 40, 56, dtype=torch.uint16), torch.zeros(32, 1, 160, 224, dtype=torch.int16))], "uint8"),
    ([_zeros(dtype=np.int16)], "uint8"),
    ([_zeros(dtype=np.uint32)], "uint8"),
    ([_zeros(h=16)], "larger than"),
    ([_zeros(n=6)], "frames"),
])
def test_constructor_rejects_mixed_depths_before_it_looks_for_a_device(seqs, word):
    with pytest.raises(ValueError, match=word):
        DeviceClipSampler(seqs, batch=2, crop=16, frames=7, seed=0, device="cuda:0")
    with pytest.raises(ValueError, match=word):
        DeviceClipSampler(seqs, batch=2, crop=16, frames=7, seed=0, device="cpu")


def test_uint16_sampler_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceClipSampler([_zeros()], batch=2, crop=16, seed=0, device="cpu")
    from fcvsr_amd import hip
    desc = torch.zeros(ctypes.sizeof(hip.CropDesc), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.clip_batch(desc, 16, torch.empty(256), dtype=torch.uint16)
    with pytest.raises(ValueError, match="dtype"):
        hip.clip_batch(desc, 16, torch.empty(256), dtype=torch.int16)


class _Seen(Exception):
    pass


def _capture(monkeypatch):
    """from_yuv420 up to the constructor: the sequences it read and the keywords it passes on."""
    def init(self, sequences, **kw):
        raise _Seen(sequences, kw)
    monkeypatch.setattr(DeviceClipSampler, "__init__", init)


def _write_pair(tmp_path, rs, name, lr_token, hr_token, dtype, n=8, h=20, w=24):
    from fcvsr_amd.harness.yuv import write_yuv420
    out = []
    for k, tag, token in ((1, "lr", lr_token), (4, "hr", hr_token)):
        mk = (lambda shape: frames_u16(rs, shape)) if dtype == np.uint16 else (lambda shape: rs.randint(0, 256, shape).astype(np.uint8))
        y, u, v = mk((n, k * h, k * w)), mk((n, k * h // 2, k * w // 2)), mk((n, k * h // 2, k * w // 2))
        path = str(tmp_path / f"{name}_{tag}_{k * w}x{k * h}_{n}F{token}.yuv")
        write_yuv420(path, y, u, v)
        out.append((path, y))
    return out


def test_from_yuv420_reads_the_bit_depth_off_the_file_names(tmp_path, monkeypatch):
    rs = np.random.RandomState(3)
    a = _write_pair(tmp_path, rs, "Alpha", "_10bit", "_10BIT", np.uint16)
    b = _write_pair(tmp_path, rs, "Beta_fps30", "_10bit", "_10bit", np.uint16, n=9, h=22, w=28)
    c = _write_pair(tmp_path, rs, "Gamma", "", "", np.uint8)
    d = _write_pair(tmp_path, rs, "Delta", "", "", np.uint16)                       # 10-bit samples, no token in the names
    _capture(monkeypatch)
    with pytest.raises(_Seen) as e:
        DeviceClipSampler.from_yuv420([(a[0][0], a[1][0]), (b[0][0], b[1][0])], batch=2, crop=16, seed=4, device="cuda:0")
    seqs, kw = e.value.args
    assert kw == dict(batch=2, crop=16, seed=4, device="cuda:0")
    for (lr, hr), files in zip(seqs, (a, b)):
        assert lr.dtype == np.uint16 and hr.dtype == np.uint16 and lr.flags["C_CONTIGUOUS"]
        assert np.array_equal(lr[:, 0], files[0][1]) and np.array_equal(hr[:, 0], files[1][1])
    assert (seqs[0][0] > 1023).any()
    with pytest.raises(_Seen) as e:                                                 # no token: 8 bits, one byte per sample
        DeviceClipSampler.from_yuv420([(c[0][0], c[1][0])], batch=2, crop=16, seed=4, device="cuda:0")
    assert e.value.args[0][0][0].dtype == np.uint8 and np.array_equal(e.value.args[0][0][1][:, 0], c[1][1])
    with pytest.raises(_Seen) as e:                                                 # an explicit depth overrides the names
        DeviceClipSampler.from_yuv420([(d[0][0], d[1][0])], bit_depth=10, batch=2, crop=16, seed=4, device="cuda:0")
    assert e.value.args[0][0][0].dtype == np.uint16 and np.array_equal(e.value.args[0][0][0][:, 0], d[0][1])


def test_from_yuv420_rejects_names_that_disagree_on_the_bit_depth(tmp_path, monkeypatch):
    rs = np.random.RandomState(4)
    a = _write_pair(tmp_path, rs, "Alpha", "_10bit", "_10bit", np.uint16)
    m = _write_pair(tmp_path, rs, "Mixed", "_10bit", "", np.uint16)                 # the HR name carries no token
    c = _write_pair(tmp_path, rs, "Gamma", "", "", np.uint8)
    _capture(monkeypatch)
    kw = dict(batch=2, crop=16, seed=4, device="cuda:0")
    with pytest.raises(ValueError, match="pair must agree"):
        DeviceClipSampler.from_yuv420([(m[0][0], m[1][0])], **kw)
    with pytest.raises(ValueError, match="pair must agree"):
        DeviceClipSampler.from_yuv420([(a[0][0], a[1][0]), (m[1][0], m[0][0])], **kw)
    with pytest.raises(ValueError, match="all pairs must agree"):
        DeviceClipSampler.from_yuv420([(a[0][0], a[1][0]), (c[0][0], c[1][0])], **kw)
    with pytest.raises(ValueError, match="all pairs must agree"):
        DeviceClipSampler.from_yuv420([(c[0][0], c[1][0]), (a[0][0], a[1][0])], **kw)
    with pytest.raises(ValueError, match="bit_depth"):
        DeviceClipSampler.from_yuv420([(a[0][0], a[1][0])], bit_depth=12, **kw)
    with pytest.raises(_Seen):                                                      # an explicit depth settles it
        DeviceClipSampler.from_yuv420([(m[0][0], m[1][0])], bit_depth=10, **kw)


def test_signature_of_the_uint16_entry_matches_the_header():
    from fcvsr_amd import hip
    assert hip.SIGNATURES["fcvsr_clip_batch_u16"] == hip.SIGNATURES["fcvsr_clip_batch_u8"]
    text = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    m = re.search(r"\bint\s+fcvsr_clip_batch_u16\s*\(([^)]*)\)\s*;", text)
    assert m, "fcvsr_clip_batch_u16 is not declared in include/fcvsr_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(hip.SIGNATURES["fcvsr_clip_batch_u16"]) == 6
    assert params[0].startswith("const fcvsr_crop_desc*") and params[1].startswith("const float*") and params[4].startswith("float*")
    assert [p.split()[0] for p in params[2:4]] == ["int", "int"] and params[5].startswith("void*")
