#!/usr/bin/env python3
"""Generate tests/golden/loader_transforms.npz by running the REFERENCE loader's own transform classes (build container only).

Usage:  python tests/golden/make_golden_loader.py            (needs /root/reference; CPU, seconds)

`RandomCrop`, `Augment` and `ToTensor` are imported read-only from /root/reference/CVSR_train/opt/data_LD_LR.py.  That module
imports `skimage`, which is absent from the image and is never used by the three classes: it is stubbed in `sys.modules`, as
make_golden.py stubs `cv2`.  For each trial seed t the script runs ``np.random.seed(t); random.seed(t)`` and then
``ToTensor()(Augment()(RandomCrop(16)(sample)))`` on a fixed uint8 sample (7 x 40 x 56 LR, 1 x 160 x 224 HR, qp = lrbi = None).
Nothing of the reference is written into the repository: the fixture holds the input frames, the seeds and the output tensors.
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OPT = "/root/reference/CVSR_train/opt"
TRIALS, CROP = 40, 16


def import_reference():
    sys.dont_write_bytecode = True
    sk = types.ModuleType("skimage")
    sk.io, sk.transform = types.ModuleType("skimage.io"), types.ModuleType("skimage.transform")
    sys.modules.update({"skimage": sk, "skimage.io": sk.io, "skimage.transform": sk.transform})
    sys.path.insert(0, REF_OPT)
    import data_LD_LR as ref
    return ref


def flags_of(lr_in: np.ndarray, hr_in: np.ndarray, lr_out: np.ndarray, hr_out: np.ndarray) -> int:
    """Which (hflip | vflip << 1 | transpose << 2) and crop corner explain one stored output: a search over all of them (the
    test uses the same function to show that the stored trials cover the 8 combinations).  -1 when none or several do."""
    f, h, w = lr_in.shape
    s = lr_out.shape[-1]
    found = set()
    for top in range(h - s + 1):
        for left in range(w - s + 1):
            a, b = lr_in[:, top:top + s, left:left + s], hr_in[:, 4 * top:4 * (top + s), 4 * left:4 * (left + s)]
            for fl in range(8):
                x, y = a, b
                if fl & 1:
                    x, y = x[:, :, ::-1], y[:, :, ::-1]
                if fl & 2:
                    x, y = x[:, ::-1], y[:, ::-1]
                if fl & 4:
                    x, y = x.transpose(0, 2, 1), y.transpose(0, 2, 1)
                if np.array_equal(x, lr_out) and np.array_equal(y, hr_out):
                    found.add(fl)
    return found.pop() if len(found) == 1 else -1


def main():
    ref = import_reference()
    g = np.random.RandomState(20240607)
    lr = g.randint(0, 256, size=(7, 40, 56)).astype(np.uint8)
    hr = g.randint(0, 256, size=(1, 160, 224)).astype(np.uint8)
    seeds = np.arange(TRIALS, dtype=np.int64)
    lr_out, hr_out = [], []
    for t in seeds:
        np.random.seed(int(t))
        random.seed(int(t))
        out = ref.ToTensor()(ref.Augment()(ref.RandomCrop(CROP)({"lr_imgs": lr, "hr_imgs": hr, "qp": None, "lrbi": None})))
        lr_out.append(out["lr_imgs"].numpy())
        hr_out.append(out["hr_imgs"].numpy())
    lr_out, hr_out = np.stack(lr_out), np.stack(hr_out)
    assert lr_out.shape == (TRIALS, 1, 7, CROP, CROP) and hr_out.shape == (TRIALS, 1, 1, 4 * CROP, 4 * CROP)
    assert lr_out.dtype == np.float32 and hr_out.dtype == np.float32
    # every output value is some k / 255 in f32: recover the k for the search over flag combinations below
    lr_k, hr_k = np.rint(lr_out * 255).astype(np.uint8), np.rint(hr_out * 255).astype(np.uint8)
    table = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    assert np.array_equal(table[lr_k], lr_out) and np.array_equal(table[hr_k], hr_out)
    seen = {flags_of(lr, hr, lr_k[i, 0], hr_k[i, 0]) for i in range(TRIALS)}
    assert seen == set(range(8)), f"the trials do not cover all 8 flag combinations: {sorted(seen)}"
    path = os.path.join(HERE, "loader_transforms.npz")
    np.savez_compressed(path, lr=lr, hr=hr, seeds=seeds, crop=np.int64(CROP), lr_out=lr_out, hr_out=hr_out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, flag combinations {sorted(seen)}")


if __name__ == "__main__":
    main()
