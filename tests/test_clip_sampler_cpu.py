"""Host half of the device clip sampler (fcvsr_amd/train/data.py), no GPU: `apply_plan_host` against tensors made by the
reference loader's own RandomCrop / Augment / ToTensor (tests/golden/loader_transforms.npz, written by make_golden_loader.py), the
properties of `plan`, the constructor's checks, and the layout of fcvsr_crop_desc."""
import ctypes
import importlib.util
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

from fcvsr_amd.train import BatchPlan, DeviceClipSampler, apply_plan_host
from fcvsr_amd.train import data as D

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _golden():
    return np.load(os.path.join(GOLDEN_DIR, "loader_transforms.npz"))


def seeded_plan(t: int, h: int, w: int, crop: int) -> BatchPlan:
    """The draws the reference chain makes after np.random.seed(t); random.seed(t): top, left from numpy's stream, then three
    random() calls."""
    rs, rnd = np.random.RandomState(t), random.Random(t)
    top, left = rs.randint(0, h - crop), rs.randint(0, w - crop)
    flips = [rnd.random() < 0.5 for _ in range(3)]
    return BatchPlan(np.array([0]), np.array([0]), np.array([top]), np.array([left]), *(np.array([f]) for f in flips))


def test_apply_plan_host_equals_the_reference_transform_classes():
    g = _golden()
    lr, hr, crop = g["lr"], g["hr"], int(g["crop"])
    assert len(g["seeds"]) >= 32
    seq = [(lr[:, None], np.repeat(hr, 7, 0)[:, None])]          # (N,C,H,W); the HR frame of a window starting at 0 is frame 3
    spec = importlib.util.spec_from_file_location("make_golden_loader", os.path.join(GOLDEN_DIR, "make_golden_loader.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    seen = set()
    for i, t in enumerate(g["seeds"]):
        bp = seeded_plan(int(t), lr.shape[1], lr.shape[2], crop)
        out = apply_plan_host(seq, bp, crop)
        assert out["lr_imgs"].dtype == torch.float32 and out["hr_imgs"].dtype == torch.float32
        assert torch.equal(out["lr_imgs"][0], torch.from_numpy(g["lr_out"][i])), f"trial {t}: lr_imgs differ"
        assert torch.equal(out["hr_imgs"][0], torch.from_numpy(g["hr_out"][i])), f"trial {t}: hr_imgs differ"
        fl = gen.flags_of(lr, hr, np.rint(g["lr_out"][i, 0] * 255).astype(np.uint8), np.rint(g["hr_out"][i, 0] * 255).astype(np.uint8))
        assert fl == int(bp.hflip[0]) + 2 * int(bp.vflip[0]) + 4 * int(bp.rot90[0])
        seen.add(fl)
    assert seen == set(range(8)), f"the stored trials cover only the flag combinations {sorted(seen)}"


def test_apply_plan_host_planes_are_independent_for_three_channels():
    g = np.random.RandomState(1)
    lr, hr = g.randint(0, 256, (9, 3, 24, 28)).astype(np.uint8), g.randint(0, 256, (9, 3, 96, 112)).astype(np.uint8)
    bp = BatchPlan(np.array([0, 0]), np.array([1, 2]), np.array([3, 0]), np.array([0, 11]), np.array([True, False]),
                   np.array([False, True]), np.array([True, True]))
    out = apply_plan_host([(lr, hr)], bp, 16)
    assert out["lr_imgs"].shape == (2, 3, 7, 16, 16) and out["hr_imgs"].shape == (2, 3, 1, 64, 64)
    for c in range(3):
        one = apply_plan_host([(lr[:, c:c + 1], hr[:, c:c + 1])], bp, 16)
        assert torch.equal(out["lr_imgs"][:, c], one["lr_imgs"][:, 0]) and torch.equal(out["hr_imgs"][:, c], one["hr_imgs"][:, 0])
    # clip 1: vflip then transpose of the window at (0, 11), frames 2..8, HR frame 5
    want = lr[2:9, 1, 0:16, 11:27][:, ::-1].transpose(0, 2, 1)
    assert torch.equal(out["lr_imgs"][1, 1], torch.from_numpy(want.copy()).float() / 255.0)
    want = hr[5, 2, 0:64, 44:108][::-1].T
    assert torch.equal(out["hr_imgs"][1, 2, 0], torch.from_numpy(want.copy()).float() / 255.0)


SHAPES13 = [(32, 40 + i, 56 + 2 * i) for i in range(13)]
KW = dict(crop=16, frames=7, seed=11, start="random")


def _records(plans):
    out = []
    for bp in plans:
        for k in range(len(bp.item)):
            out.append(tuple(int(a[k]) for a in bp))
    return out


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_plan_gives_every_rank_the_same_batch_sizes_and_covers_every_item(world):
    n, batch, epoch = len(SHAPES13), 3, 4
    plans = [D.make_plan(SHAPES13, epoch, batch=batch, rank=r, world=world, **KW) for r in range(world)]
    sizes = [[len(bp.item) for bp in p] for p in plans]
    assert all(s == sizes[0] for s in sizes), sizes
    share = -(-n // world)
    assert sizes[0] == [batch] * (share // batch) + ([share % batch] if share % batch else [])
    items = [r[0] for p in plans for r in _records(p)]
    count = Counter(items)
    assert set(count) == set(range(n))
    twice = sorted(i for i, c in count.items() if c == 2)
    assert len(twice) == (-n) % world and all(c <= 2 for c in count.values())
    perm = np.random.RandomState([KW["seed"], epoch]).permutation(n)
    assert twice == sorted(int(i) for i in perm[:(-n) % world])
    assert items == [int(i) for i in D.epoch_order(n, epoch, KW["seed"], world)]     # rank shares are contiguous, in order
    if world == 1:
        assert all(c == 1 for c in count.values())


def test_plan_record_of_an_item_does_not_depend_on_world_rank_or_batch():
    base = {r[0]: r for r in _records(D.make_plan(SHAPES13, 2, batch=13, rank=0, world=1, **KW))}
    assert len(base) == 13
    for world, batch in [(2, 1), (3, 4), (8, 2), (1, 5)]:
        for rank in range(world):
            for r in _records(D.make_plan(SHAPES13, 2, batch=batch, rank=rank, world=world, **KW)):
                assert r == base[r[0]]                                        # a padded repeat gets the same draws too
    for i, shape in enumerate(SHAPES13):
        assert base[i][1:] == tuple(int(v) for v in D.item_draws(KW["seed"], 2, i, shape, 16, 7, "random"))


def test_plan_epochs_and_seeds_differ():
    a, b = (_records(D.make_plan(SHAPES13, e, batch=4, rank=0, world=1, **KW)) for e in (0, 1))
    assert [r[0] for r in a] != [r[0] for r in b]
    assert sorted(a) != sorted(b)
    c = _records(D.make_plan(SHAPES13, 0, batch=4, rank=0, world=1, **dict(KW, seed=12)))
    assert sorted(a) != sorted(c)
    assert a == _records(D.make_plan(SHAPES13, 0, batch=4, rank=0, world=1, **KW))


def test_plan_draws_stay_inside_the_reference_ranges():
    shapes = [(32, 17, 18), (40, 40, 56), (31, 270, 480)]
    seen = {m: set() for m in D.STARTS}
    flags = set()
    for start in D.STARTS:
        for epoch in range(60):
            for r in _records(D.make_plan(shapes, epoch, batch=2, crop=16, frames=7, seed=3, start=start, rank=0, world=1)):
                item, first, top, left = r[:4]
                N, H, W = shapes[item]
                assert 0 <= first and first + 7 <= N
                assert 0 <= top and top + 16 < H and 0 <= left and left + 16 < W      # randint's high end is exclusive
                seen[start].add((N, first))
                flags.add(r[4:])
    assert {f for n, f in seen["first"]} == {0}
    assert {f for n, f in seen["gop"]} == {0, 4, 8, 12, 16, 20, 24}
    assert {f for n, f in seen["random"] if n == 32} == set(range(26))                # random.randint(0, 25), inclusive
    assert max(f for n, f in seen["random"] if n == 40) == 33
    assert len(flags) == 8


def _seq(n=32, c=1, h=40, w=56, dtype=np.uint8, scale=4):
    return np.zeros((n, c, h, w), dtype), np.zeros((n, c, scale * h, scale * w), dtype)


@pytest.mark.parametrize("seqs,kw,word", [
    ([_seq(dtype=np.float32)], {}, "uint8"),
    ([(_seq()[0], _seq()[1].astype(np.int16))], {}, "uint8"),
    ([_seq(scale=2)], {}, "4x"),
    ([(_seq()[0], _seq(h=41)[1])], {}, "4x"),
    ([_seq(h=16)], {}, "larger than"),
    ([_seq(w=16)], {}, "larger than"),
    ([_seq(h=12)], {}, "larger than"),
    ([_seq(n=6)], {}, "frames"),
    ([_seq(n=30)], {"start": "gop"}, "gop"),
    ([_seq(), _seq(c=3)], {}, "channels"),
    ([_seq()], {"start": "middle"}, "start"),
    ([_seq()], {"crop": 18}, "multiple of 4"),
    ([], {}, "no sequences"),
])
def test_constructor_rejects_bad_sequences_with_value_errors(seqs, kw, word):
    args = dict(batch=2, crop=16, frames=7, seed=0, device="cuda:0")
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        DeviceClipSampler(seqs, **args)


def test_sampler_and_kernel_wrapper_have_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceClipSampler([_seq()], batch=2, crop=16, seed=0, device="cpu")
    from fcvsr_amd import hip
    desc = torch.zeros(ctypes.sizeof(hip.CropDesc), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.clip_batch(desc, 16, torch.empty(256))


def test_crop_desc_layout_matches_header(tmp_path):
    """sizeof / offsetof of fcvsr_crop_desc as a C compiler reads include/fcvsr_hip.h == the ctypes mirror and its numpy form."""
    from fcvsr_amd import hip
    src = tmp_path / "layout.c"
    fields = ["src", "pitch", "top", "left", "flags"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcvsr_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(fcvsr_crop_desc)' + "".join(f", offsetof(fcvsr_crop_desc, {f})" for f in fields)
                   + '); printf("%d %d %d\\n", FCVSR_CROP_HFLIP, FCVSR_CROP_VFLIP, FCVSR_CROP_TRANSPOSE); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = hip.CropDesc
    assert got[:6] == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert got[6:] == [hip.CROP_HFLIP, hip.CROP_VFLIP, hip.CROP_TRANSPOSE]
    dt = np.dtype(T)
    assert dt.itemsize == got[0] and [dt.fields[f][1] for f in fields] == got[1:6]
    assert 24 <= got[0] <= 32


def _emulate(d, s):
    """What fcvsr_clip_batch_u8 is specified to compute from one descriptor, read from HOST memory through the pointer."""
    buf = (ctypes.c_uint8 * 1).from_address(int(d["src"]))
    rows = [np.ctypeslib.as_array((ctypes.c_uint8 * s).from_address(ctypes.addressof(buf) + (int(d["top"]) + r) * int(d["pitch"])
                                                                     + int(d["left"]))).copy() for r in range(s)]
    a = np.stack(rows)
    if d["flags"] & 1:
        a = a[:, ::-1]
    if d["flags"] & 2:
        a = a[::-1]
    if d["flags"] & 4:
        a = a.T
    return torch.from_numpy(a.copy()).float() / 255.0


def test_descriptors_name_the_planes_of_the_host_chain():
    """fill_descs, the host half of DeviceClipSampler.build, over host memory: every descriptor's window, read as the kernel is
    specified to read it, is the plane `apply_plan_host` makes, in the (b,F,C) / (b,C) order of the device batch."""
    from fcvsr_amd import hip
    rs = np.random.RandomState(0)
    seqs = []
    for n, c, h, w in ((9, 3, 24, 31), (12, 3, 40, 22)):
        seqs.append((rs.randint(0, 256, (n, c, h, w)).astype(np.uint8), rs.randint(0, 256, (n, c, 4 * h, 4 * w)).astype(np.uint8)))
    bp = BatchPlan(np.array([1, 0, 1]), np.array([5, 2, 0]), np.array([23, 0, 7]), np.array([0, 14, 5]), np.array([True, False, True]),
                   np.array([False, True, True]), np.array([True, True, False]))
    s, F, C, b = 16, 7, 3, 3
    d = np.zeros(b * F * C + b * C, dtype=np.dtype(hip.CropDesc))
    flags = (bp.hflip * 1 + bp.vflip * 2 + bp.rot90 * 4).astype(np.int32)
    H, W = np.array([seqs[i][0].shape[2] for i in bp.item]), np.array([seqs[i][0].shape[3] for i in bp.item])
    D.fill_descs(d, [seqs[i][0].ctypes.data for i in bp.item], [seqs[i][1].ctypes.data for i in bp.item], bp.first, bp.top, bp.left,
                 flags, H, W, F, C)
    want = apply_plan_host(seqs, bp, s)
    lr, hr = d[:b * F * C].reshape(b, F, C), d[b * F * C:].reshape(b, C)
    for k in range(b):
        for c in range(C):
            assert torch.equal(_emulate(hr[k, c], 4 * s), want["hr_imgs"][k, c, 0])
            for f in range(F):
                assert torch.equal(_emulate(lr[k, f, c], s), want["lr_imgs"][k, c, f])
