#!/usr/bin/env python3
"""Record the REFERENCE's BRISQUE on seeded planes (build container only; CPU, a few seconds).

Usage:  python tests/golden/make_golden_brisque.py REFERENCE_ROOT

REFERENCE_ROOT is a checkout of the reference project; its CVSR_train/metric/brisque.py (a piq / pyiqa port in f32 torch) is loaded
read-only by file path.  Nothing of its text is written into the repository: brisque_cases.npz holds data only.

Planes: three uint8 planes of sinusoids plus Gaussian noise (48x64, 74x102 - no multiple of any tile, odd halves - and 192x288), one
74x102 RGB frame, one constant-128 48x64 plane and one 48x64 plane with a +-100 checkerboard on a gentle texture.  Per plane: the 36 features of the reference's own natural_scene_statistics / imresize
chain and the score of its brisque() under a seeded synthetic regressor (12 support vectors uniform in [-1,1], normal coefficients,
handed over as a temporary .pth and stored here as `sv`, `sv_coef`).  For the RGB frame also the reference's rounded YIQ luma.

The script fails unless
  - the contract's (fcvsr_amd/harness/brisque.py) grid index equals the reference's for all 10 alpha entries of every plane,
  - the contract's integer YIQ luma equals the reference's rounded luma at every pixel of the RGB frame (the frame's seed is the
    first for which no pixel has (299 R + 587 G + 114 B) % 1000 == 500, the one case where f32 and integer rounding may differ),
  - the NaN pattern of the checkerboard plane is the reference's and is not empty: at scale 1 the sign of its MSCN alternates, so
    the horizontal and vertical products have no positive sample and the diagonal ones no negative sample.

The constant plane: in the reference's f32 the 7 x 7 mean of 128 is 128 in the interior, the MSCN is non-zero only near the zero-padded
border, no product is negative and the AGGD entries are NaN.  The contract's window is the same f32 numbers used as f64; they sum to
1 + 1.1e-8, so in f64 the interior MSCN is -1.4e-6, its products with the positive border ring are negative and every entry is
finite.  The two cannot agree on the sign of a residue that is pure rounding, so this plane's AGGD entries are recorded but not
asserted: `const_48x64_comparable` lists the entries that do not depend on it (alpha and sigma^2 of the two GGD fits), which are
held to the same bounds as every other plane's.  The checkerboard plane pins the NaN handling instead: its empty sides are empty in
exact arithmetic.
It measures the largest difference between contract and reference in scaled-feature units and in the score and stores them as
`max_scaled_diff` and `max_score_diff`: tests/test_brisque_cpu.py takes its bounds from them.
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
PLANES = (("48x64", 48, 64, 201), ("74x102", 74, 102, 202), ("192x288", 192, 288, 203))
RGB_FIRST_SEED = 300


def sibling(seed, h, w):
    """Sinusoids plus Gaussian noise, no flat region (tests/test_niqe_gpu.py _sibling at any size)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 120.0 + 40 * np.sin(rs.uniform(0.02, 0.2) * yy + rs.uniform(0.02, 0.2) * xx) + 25 * np.sin(rs.uniform(0.05, 0.3) * xx)
    return np.clip(np.round(img + rs.normal(0, 6.0, img.shape)), 0, 255).astype(np.uint8)


def checkerboard(seed, h, w):
    """128 +- 100 in a one-pixel checkerboard over a gentle texture: the alternation decides the sign of every MSCN sample, at the
    zero-padded border too; the 2x down-scale removes it (its taps weigh both colours 1/2) and leaves the texture."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 128.0 + 12 * np.sin(rs.uniform(0.1, 0.3) * yy + rs.uniform(0.1, 0.3) * xx) + rs.normal(0, 3.0, (h, w))
    return np.clip(np.round(img + 100.0 * (1 - 2 * ((yy + xx) % 2))), 0, 255).astype(np.uint8)


def rgb_frame(h, w):
    """The first seed from RGB_FIRST_SEED on whose frame has no pixel on a rounding tie of the luma."""
    for seed in range(RGB_FIRST_SEED, RGB_FIRST_SEED + 100000):
        rs = np.random.RandomState(seed)
        base = sibling(seed, h, w).astype(np.int32)
        rgb = np.clip(np.stack([base + rs.randint(-20, 21, base.shape) for _ in range(3)]), 0, 255).astype(np.uint8)
        c = rgb.astype(np.int64)
        v = 299 * c[0] + 587 * c[1] + 114 * c[2]
        if not (v % 1000 == 500).any():
            return seed, rgb
    raise SystemExit("no RGB seed without a rounding tie")


def alpha_index(features):
    from fcvsr_amd.harness.brisque import ALPHA
    return np.rint((np.asarray(features, dtype=np.float64)[list(ALPHA)] - 0.2) / 0.001).astype(np.int64)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    torch.set_num_threads(1)
    from fcvsr_amd.harness import brisque as contract
    spec = importlib.util.spec_from_file_location("ref_brisque", os.path.join(sys.argv[1], "CVSR_train", "metric", "brisque.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rs = np.random.RandomState(2025)
    sv = rs.uniform(-1, 1, (12, 36)).astype(np.float32)
    sv_coef = rs.normal(0, 1, 12).astype(np.float32)
    model = contract.BrisqueModel(sv, sv_coef)
    arrays = {"sv": sv.astype(np.float64), "sv_coef": sv_coef.astype(np.float64)}

    cases = [(name, sibling(seed, h, w), None) for name, h, w, seed in PLANES]
    cases.append(("const_48x64", np.full((48, 64), 128, dtype=np.uint8), None))
    cases.append(("alt_48x64", checkerboard(204, 48, 64), None))
    arrays["const_48x64_comparable"] = np.array([0, 1, 18, 19], dtype=np.int64)
    rgb_seed, rgb = rgb_frame(74, 102)
    cases.append(("rgb_74x102", None, rgb))
    arrays["rgb_seed"] = np.int64(rgb_seed)

    max_scaled, max_score = 0.0, 0.0
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        pth = os.path.join(tmp, "weights.pth")
        for name, plane, frame in cases:
            if frame is not None:
                x01 = torch.from_numpy(frame.astype(np.float32) / np.float32(255.0))[None]          # (1,3,H,W) in [0,1]
                luma = ref.to_y_channel(x01, 255.)
                ref_luma = luma[0, 0].numpy()
                plane = contract.yiq_luma(frame)
                assert np.array_equal(ref_luma, plane.astype(np.float32)), f"{name}: the integer luma differs from the reference's"
                arrays["rgb_74x102"], arrays["rgb_74x102_luma"] = frame, plane
            else:
                x01 = torch.from_numpy(plane.astype(np.float32) / np.float32(255.0))[None, None]
                luma = x01 * 255
                arrays[f"plane_{name}"] = plane
            f1 = ref.natural_scene_statistics(luma, 7, 7. / 6)
            f2 = ref.natural_scene_statistics(ref.imresize(luma, scale=0.5, antialiasing=True), 7, 7. / 6)
            ref_f = torch.cat([f1, f2], dim=-1).reshape(36).numpy().astype(np.float64)
            torch.save((torch.from_numpy(sv_coef.copy()), torch.from_numpy(sv.copy())), pth)      # brisque() transposes sv in place
            ref_score = float(ref.brisque(x01, pretrained_model_path=pth).reshape(-1)[0])

            got = contract.brisque_features(plane)
            arrays[f"feat_{name}"], arrays[f"score_{name}"] = ref_f, np.float64(ref_score)
            if name == "const_48x64":
                assert np.isnan(ref_f).any() and not np.isnan(got).any(), "the constant plane: see the module docstring"
                keep = arrays["const_48x64_comparable"]
                assert np.array_equal(alpha_index(got)[[0, 5]], alpha_index(ref_f)[[0, 5]]), f"{name}: GGD alpha {got[[0, 18]]} vs {ref_f[[0, 18]]}"
                d = float(np.abs(contract.scale_features(got)[keep] - contract.scale_features(ref_f)[keep]).max())
                max_scaled = max(max_scaled, d)
                print(f"{name}: scaled-feature diff of the GGD entries {d:.3e}; reference NaN entries {int(np.isnan(ref_f).sum())}")
                continue
            assert np.array_equal(np.isnan(got), np.isnan(ref_f)), f"{name}: NaN pattern {np.isnan(got)} vs {np.isnan(ref_f)}"
            assert np.array_equal(alpha_index(got), alpha_index(ref_f)), f"{name}: alpha index {alpha_index(got)} vs {alpha_index(ref_f)}"
            ok = ~np.isnan(ref_f)
            d = float(np.abs(contract.scale_features(got)[ok] - contract.scale_features(ref_f)[ok]).max())
            max_scaled = max(max_scaled, d)
            score = contract.brisque_score(got, model)
            assert np.isnan(score) == np.isnan(ref_score), name
            if not np.isnan(ref_score):
                max_score = max(max_score, abs(score - ref_score))
            print(f"{name}: scaled-feature diff {d:.3e}, score {score:.9f} vs reference {ref_score:.9f}, NaN entries {int((~ok).sum())}")
    assert np.isnan(arrays["feat_alt_48x64"][:18]).sum() == 8 and not np.isnan(arrays["feat_alt_48x64"][18:]).any()
    arrays["max_scaled_diff"], arrays["max_score_diff"] = np.float64(max_scaled), np.float64(max_score)
    np.savez_compressed(os.path.join(HERE, "brisque_cases.npz"), **arrays)
    print(f"brisque_cases.npz: rgb seed {rgb_seed}, max_scaled_diff {max_scaled:.3e}, max_score_diff {max_score:.3e}")


if __name__ == "__main__":
    main()
