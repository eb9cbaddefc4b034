#!/usr/bin/env python3
"""Record what the REFERENCE's MATLAB-like resize computes at general scales and output shapes (build container only; CPU, seconds).

Usage:  python tests/golden/make_golden_imresize.py        (needs /root/reference; prints "skipped" without it)

The reference module (mmedit_train/mmedit/datasets/pipelines/matlab_like_resize.py, MATLABLikeResize) is loaded read-only by file
path with the stubs of make_golden_upscale.py.  Nothing of the reference's text is written into the repository: data only.

  imresize_cases.npz
    in_<h>x<w>_u8 / _u10 / _f32      seeded planes, 2x3 5x7 12x16 37x23 45x80: uint8; 10-bit values in uint16 (handed to the
                                     reference as f32); f32 in [0, 1]
    in_const_5x7_u8                  a constant plane (the output is the constant)
    in_checker_8x10_u8               a 0 / 255 checkerboard (values below 0 and above 255)
    out_<name>_s<i>                  MATLABLikeResize(scale=SCALES[i])._resize of it, as f32 (scale 3 only up to 37x23)
    out_<name>_<Ho>x<Wo>             MATLABLikeResize(output_shape=(Ho, Wo))._resize of it: (h+1, w+1), (2h, max(2, w//2)) - columns
                                     first -, (max(2, h//3), 3w), and 45x80 -> (27, 48)
    scales                           SCALES as f64

No case runs a pass of 8 or more stored taps over a plane whose other extent is 1 (numpy then sums pairwise, not in tap order): a
case whose output has an extent below 2 is left out, which guarantees it.  The script asserts that every f64 of the reference's
result is an f32 and that the reference's weight tables are f32.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_upscale import REF, load_reference  # noqa: E402

SIZES = ((2, 3), (5, 7), (12, 16), (37, 23), (45, 80))
SCALES = (0.75, 2.0 / 3.0, 0.3, 1.25, 1.5, 3.0, 1.0)


def inputs():
    """name -> plane, in a fixed order."""
    out = {}
    for k, (h, w) in enumerate(SIZES):
        rs = np.random.RandomState(300 + k)
        out[f"{h}x{w}_u8"] = rs.randint(0, 256, (h, w)).astype(np.uint8)
        out[f"{h}x{w}_u10"] = rs.randint(0, 1024, (h, w)).astype(np.uint16)
        out[f"{h}x{w}_f32"] = rs.random_sample((h, w)).astype(np.float32)
    out["const_5x7_u8"] = np.full((5, 7), 201, dtype=np.uint8)
    yy, xx = np.mgrid[0:8, 0:10]
    out["checker_8x10_u8"] = (((yy + xx) & 1) * 255).astype(np.uint8)
    return out


def shapes_for(h, w):
    s = [(h + 1, w + 1), (2 * h, max(2, w // 2)), (max(2, h // 3), 3 * w)]
    if (h, w) == (45, 80):
        s.append((27, 48))
    return s


def cases(name, plane):
    """(key suffix, constructor keywords) of every case of one plane."""
    h, w = plane.shape
    for i, s in enumerate(SCALES):
        if s == 3.0 and h * w > 37 * 23:
            continue
        if min(int(np.ceil(s * h)), int(np.ceil(s * w))) >= 2:
            yield f"s{i}", dict(scale=s)
    for ho, wo in shapes_for(h, w):
        yield f"{ho}x{wo}", dict(output_shape=(ho, wo))


def main():
    if not os.path.isdir(REF):
        print("skipped: the reference is absent")
        return
    sys.dont_write_bytecode = True
    resize = load_reference()
    arrays = {"scales": np.array(SCALES, dtype=np.float64)}
    for n_in, n_out, s in ((45, 27, 27 / 45), (37, 111, 3.0), (80, 24, 0.3)):
        wt, _ = resize.get_weights_indices(n_in, n_out, s, resize._cubic, 4.0)
        assert wt.dtype == np.float32, wt.dtype
    for name, plane in inputs().items():
        arrays[f"in_{name}"] = plane
        given = plane.astype(np.float32) if plane.dtype == np.uint16 else plane
        for key, kw in cases(name, plane):
            got = resize.MATLABLikeResize(keys=None, **kw)._resize(given[:, :, None])[:, :, 0]
            assert got.dtype == np.float64 and min(got.shape) >= 2
            assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
            arrays[f"out_{name}_{key}"] = got.astype(np.float32)
    path = os.path.join(HERE, "imresize_cases.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:     # np.savez_compressed with a fixed time stamp, so
        for key, val in arrays.items():                                          # that the file regenerates byte for byte
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(val), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("imresize_cases.npz:", os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
