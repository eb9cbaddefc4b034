#!/usr/bin/env python3
"""Record what the REFERENCE's MATLAB-like resize computes at scale 2 and 4 (build container only; CPU, a second).

Usage:  python tests/golden/make_golden_upscale.py        (needs /root/reference; prints "skipped" without it)

The reference module (mmedit_train/mmedit/datasets/pipelines/matlab_like_resize.py, MATLABLikeResize) is loaded read-only by file
path, with sys.modules stubs for the packages and the registry it imports, as make_golden_niqe.py does.  Nothing of the
reference's text is written into the repository: data only.

  upscale_cases.npz
    in_<h>x<w>_u8 / _u10 / _f32      seeded planes, 1x1 1x9 9x1 2x3 5x7 12x16 37x23: uint8; 10-bit values in uint16 (handed to the
                                     reference as f32); f32 in [0, 1]
    in_const_5x7_u8                  a constant plane (the output is the constant)
    in_checker_8x10_u8               a 0 / 255 checkerboard (the strongest overshoot: values below 0 and above 255)
    out_<same name>_x2 / _x4         MATLABLikeResize(scale=2 | 4)._resize of it, stored as f32 (the script asserts that every f64 of the
                                     reference's result is an f32)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mmedit_train"
SIZES = ((1, 1), (1, 9), (9, 1), (2, 3), (5, 7), (12, 16), (37, 23))


def inputs():
    """name -> plane, in a fixed order."""
    out = {}
    for k, (h, w) in enumerate(SIZES):
        rs = np.random.RandomState(100 + k)
        out[f"{h}x{w}_u8"] = rs.randint(0, 256, (h, w)).astype(np.uint8)
        out[f"{h}x{w}_u10"] = rs.randint(0, 1024, (h, w)).astype(np.uint16)
        out[f"{h}x{w}_f32"] = rs.random_sample((h, w)).astype(np.float32)
    out["const_5x7_u8"] = np.full((5, 7), 201, dtype=np.uint8)
    yy, xx = np.mgrid[0:8, 0:10]
    out["checker_8x10_u8"] = (((yy + xx) & 1) * 255).astype(np.uint8)
    return out


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    for pkg in ("mmedit", "mmedit.datasets", "mmedit.datasets.pipelines"):
        stub(pkg)
    stub("mmedit.datasets.registry", PIPELINES=Registry())
    name = "mmedit.datasets.pipelines.matlab_like_resize"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "mmedit/datasets/pipelines/matlab_like_resize.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(REF):
        print("skipped: the reference is absent")
        return
    sys.dont_write_bytecode = True
    resize = load_reference()
    arrays = {}
    for name, plane in inputs().items():
        arrays[f"in_{name}"] = plane
        given = plane.astype(np.float32) if plane.dtype == np.uint16 else plane
        for factor in (2, 4):
            got = resize.MATLABLikeResize(keys=None, scale=factor)._resize(given[:, :, None])[:, :, 0]
            assert got.shape == (factor * plane.shape[0], factor * plane.shape[1]) and got.dtype == np.float64
            assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
            arrays[f"out_{name}_x{factor}"] = got.astype(np.float32)
    path = os.path.join(HERE, "upscale_cases.npz")
    np.savez_compressed(path, **arrays)
    print("upscale_cases.npz:", os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
