#!/usr/bin/env python3
"""Record what the REFERENCE's NIQE and its MATLAB-like resize compute (build container only; CPU, some seconds).

Usage:  python tests/golden/make_golden_niqe.py        (needs /root/reference, scipy and PIL; prints "skipped" without them)

The reference functions (mmedit_train/mmedit/core/evaluation/metrics.py niqe_core, mmedit/datasets/pipelines/matlab_like_resize.py
MATLABLikeResize) are loaded read-only by file path, with sys.modules stubs for cv2, mmcv and the registries they import but do not
use here.  Nothing of the reference's text is written into the repository: data only.

  niqe_pris_params.npz   a copy of the reference's pristine model (mu_pris_param, cov_pris_param, gaussian_window)
  niqe_cases.npz
    baboon_b                       the blue channel of tests/data/gt/baboon.png (480 x 500 uint8)
    baboon_score_0 / _6            niqe_core of it as an f64 plane with crop_border 0 / 6: 5.624713, 5.827623.  (The published 5.62525
                                   and 5.82981 are those of niqe(), which hands niqe_core an f32 plane: scipy then returns the two
                                   convolutions rounded to f32.  Every plane here goes in as f64.)
    syn_<name>, syn_<name>_features, syn_<name>_score
                                   seeded synthetic Y planes (uint8: drifting sinusoids + Gaussian noise sigma 6, rounded; no flat
                                   non-zero region), the reference's (blocks, 36) features sorted into row-major block order, and its
                                   score.  bar_288x384 has rows 0..111 black (a letterbox bar: the whole top block row is NaN blocks),
                                   corner_192x192 has [:112, :112] black.
    rs_<h>x<w>, rs_<h>x<w>_half / _quarter
                                   a random uint8 plane and MATLABLikeResize(scale 0.5 / 0.25) of it (f64, 0..255 scale)
"""
import importlib.util
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mmedit_train"


def synthetic(h, w, seed):
    """Sum of drifting sinusoids plus Gaussian noise (sigma 6), rounded and clipped to uint8."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 118.0)
    for _ in range(6):
        fy, fx = rs.uniform(0.01, 0.25, 2)
        drift = rs.uniform(-4e-4, 4e-4)
        img += rs.uniform(8, 28) * np.sin(fy * yy + fx * xx + drift * yy * xx + rs.uniform(0, 2 * np.pi))
    img += rs.normal(0.0, 6.0, (h, w))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def cases():
    out = {"96x192": synthetic(96, 192, 11), "192x288": synthetic(192, 288, 12), "200x301": synthetic(200, 301, 13)}
    bar = synthetic(288, 384, 14)
    bar[:112] = 0
    out["bar_288x384"] = bar
    corner = synthetic(192, 192, 15)
    corner[:112, :112] = 0
    out["corner_192x192"] = corner
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

    stub("cv2")
    stub("mmcv")
    for pkg in ("mmedit", "mmedit.datasets", "mmedit.datasets.pipelines", "mmedit.core", "mmedit.core.evaluation"):
        stub(pkg)
    stub("mmedit.datasets.registry", PIPELINES=Registry())
    stub("mmedit.core.evaluation.metric_utils", gauss_gradient=None)

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    resize = load("mmedit.datasets.pipelines.matlab_like_resize", "mmedit/datasets/pipelines/matlab_like_resize.py")
    metrics = load("mmedit.core.evaluation.metrics", "mmedit/core/evaluation/metrics.py")
    return metrics, resize


def main():
    try:
        import scipy  # noqa: F401  (the reference's metrics.py needs it)
        from PIL import Image
    except ImportError as e:
        print(f"skipped: {e}")
        return
    if not os.path.isdir(REF):
        print("skipped: the reference is absent")
        return
    sys.dont_write_bytecode = True
    metrics, resize = load_reference()
    params = os.path.join(REF, "mmedit/core/evaluation/niqe_pris_params.npz")
    shutil.copyfile(params, os.path.join(HERE, "niqe_pris_params.npz"))
    p = np.load(params)
    model = (p["mu_pris_param"], p["cov_pris_param"], p["gaussian_window"])

    arrays = {}
    rgb = np.asarray(Image.open(os.path.join(REF, "tests/data/gt/baboon.png")).convert("RGB"))
    blue = np.ascontiguousarray(rgb[:, :, 2])
    assert blue.shape == (480, 500) and blue.dtype == np.uint8
    arrays["baboon_b"] = blue
    for crop in (0, 6):
        plane = blue.astype(np.float64)
        plane = plane[crop:-crop, crop:-crop] if crop else plane
        arrays[f"baboon_score_{crop}"] = np.float64(metrics.niqe_core(plane, *model))
        print(f"baboon crop_border={crop}: {arrays[f'baboon_score_{crop}']:.6f}")

    # the features niqe_core fits its Gaussian to are local to it: record them through np.nanmean, which it calls once on them
    for name, img in cases().items():
        seen = []
        real = metrics.np.nanmean

        def spy(a, *args, **kw):
            seen.append(np.array(a))
            return real(a, *args, **kw)

        metrics.np.nanmean = spy
        try:
            score = float(metrics.niqe_core(img.astype(np.float64), *model))
        finally:
            metrics.np.nanmean = real
        feats = seen[0]
        nbh, nbw = img.shape[0] // 96, img.shape[1] // 96
        assert feats.shape == (nbh * nbw, 36)
        feats = feats.reshape(nbw, nbh, 36).transpose(1, 0, 2).reshape(nbh * nbw, 36)     # column-major -> row-major blocks
        assert np.isfinite(score)
        arrays[f"syn_{name}"] = img
        arrays[f"syn_{name}_features"] = feats
        arrays[f"syn_{name}_score"] = np.float64(score)
        print(f"{name}: score {score:.6f}, NaN blocks {int(np.isnan(feats).any(axis=1).sum())} of {feats.shape[0]}")

    for (h, w), seed in (((40, 56), 21), ((16, 16), 22)):
        plane = np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)
        arrays[f"rs_{h}x{w}"] = plane
        for key, scale in (("half", 0.5), ("quarter", 0.25)):
            arrays[f"rs_{h}x{w}_{key}"] = resize.MATLABLikeResize(keys=None, scale=scale)._resize(plane[:, :, None])[:, :, 0]

    np.savez_compressed(os.path.join(HERE, "niqe_cases.npz"), **arrays)
    print("niqe_cases.npz:", os.path.getsize(os.path.join(HERE, "niqe_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
