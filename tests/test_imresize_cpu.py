"""Host: the any-size resize contract (fcvsr_amd/harness/resize.py imresize_host, resize_tables) against the reference's recorded
outputs (tests/golden/imresize_cases.npz, made by tests/golden/make_golden_imresize.py), against the fixed-scale contracts it
generalises, its tables, the error cases, and the C ABI / binding / harness surface of fcvsr_imresize and output_shape=."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "imresize_cases.npz"))


@pytest.fixture(scope="module")
def maker(golden_dir):
    """The script that recorded the fixture: its list of inputs and cases is the list the tests walk."""
    sys.path.insert(0, golden_dir)
    try:
        import make_golden_imresize
    finally:
        sys.path.remove(golden_dir)
    return make_golden_imresize


def _walk(maker, cases):
    for name, plane in maker.inputs().items():
        assert np.array_equal(cases[f"in_{name}"], plane) and cases[f"in_{name}"].dtype == plane.dtype
        for key, kw in maker.cases(name, plane):
            yield name, plane, key, kw, cases[f"out_{name}_{key}"]


def test_the_fixture_holds_every_case(maker, cases):
    seen = {(name, key) for name, _, key, _, _ in _walk(maker, cases)}
    assert len(seen) == len([f for f in cases.files if f.startswith("out_")]) == 167
    assert np.array_equal(cases["scales"], np.array([0.75, 2 / 3, 0.3, 1.25, 1.5, 3, 1.0]))
    for size in ("2x3", "5x7", "12x16", "37x23", "45x80"):
        for kind, dtype in (("u8", np.uint8), ("u10", np.uint16), ("f32", np.float32)):
            assert cases[f"in_{size}_{kind}"].dtype == dtype
    assert cases["in_45x80_u10"].max() <= 1023
    assert "out_37x23_u8_s5" in cases.files and "out_45x80_u8_s5" not in cases.files         # scale 3 only up to 37x23
    assert cases["out_45x80_u8_27x48"].shape == (27, 48) and cases["out_12x16_f32_24x8"].shape == (24, 8)
    for f in cases.files:                                     # the condition under which the reference sums in tap order
        if f.startswith("out_"):
            assert min(cases[f].shape) >= 2, f


def test_contract_has_the_bits_of_the_reference(maker, cases):
    from fcvsr_amd.harness.resize import imresize_host
    for name, plane, key, kw, ref in _walk(maker, cases):
        got = imresize_host(plane, **kw)
        assert got.dtype == np.float64 and got.shape == ref.shape, (name, key)
        assert np.array_equal(got, ref.astype(np.float64)), (name, key)
        if plane.dtype != np.float32:
            peak = 255 if plane.dtype == np.uint8 else 1023
            goti = imresize_host(plane, out="int", **kw)
            assert goti.dtype == plane.dtype
            assert np.array_equal(goti, np.around(np.clip(ref, 0, peak)).astype(plane.dtype)), (name, key)


def test_checkerboard_clips_and_constant_stays(cases):
    from fcvsr_amd.harness.resize import imresize_host
    chk = cases["in_checker_8x10_u8"]
    f32 = imresize_host(chk, scale=1.5)
    assert (f32 < 0).any() and (f32 > 255).any()
    got = imresize_host(chk, scale=1.5, out="int")
    assert got.min() == 0 and got.max() == 255
    const = cases["in_const_5x7_u8"]
    for kw in (dict(scale=0.3), dict(scale=2 / 3), dict(scale=3), dict(output_shape=(11, 4)), dict(output_shape=(2, 21))):
        assert np.all(imresize_host(const, out="int", **kw) == 201), kw
        # f32: per pass P rounded products, P rounded sums of at most ~1.3 c and a row sum within P ulp of 1 - under 4 P c 2^-24;
        # two passes of at most 16 taps (scale 0.3) stay below c 2^-17
        assert np.abs(imresize_host(const, **kw) - 201).max() <= 201 * 2.0 ** -17, kw


def test_equals_the_fixed_scale_contracts_bit_for_bit():
    from fcvsr_amd.harness.niqe import bicubic_downscale, bicubic_upscale
    from fcvsr_amd.harness.resize import imresize_host
    rs = np.random.RandomState(5)
    for shape in ((1, 1), (1, 9), (9, 1), (2, 3), (5, 7), (2, 12, 16)):
        for x in (rs.randint(0, 256, shape).astype(np.uint8), rs.randint(0, 1024, shape).astype(np.uint16),
                  rs.random_sample(shape).astype(np.float32)):
            for factor in (2, 4):
                assert np.array_equal(imresize_host(x, scale=factor), bicubic_upscale(x, factor)), (shape, x.dtype, factor)
                h, w = shape[-2:]
                assert np.array_equal(imresize_host(x, output_shape=(factor * h, factor * w)), bicubic_upscale(x, factor))
                if x.dtype != np.float32:
                    assert np.array_equal(imresize_host(x, scale=factor, out="int"), bicubic_upscale(x, factor, out="int"))
    for shape in ((8, 8), (16, 24), (3, 12, 20), (8, 36)):
        for x in (rs.randint(0, 256, shape).astype(np.uint8), rs.random_sample(shape).astype(np.float32)):
            for factor in (2, 4):
                if shape[-2] // factor >= 2 and shape[-1] // factor >= 2 and shape[-2] % factor == 0 and shape[-1] % factor == 0:
                    assert np.array_equal(imresize_host(x, scale=1 / factor), bicubic_downscale(x, factor)), (shape, factor)


def test_identity_batches_and_wild_uint16():
    from fcvsr_amd.harness.resize import imresize_host
    rs = np.random.RandomState(6)
    for x in (rs.randint(0, 256, (2, 5, 7)).astype(np.uint8), rs.random_sample((9, 4)).astype(np.float32)):
        same = imresize_host(x, output_shape=x.shape[-2:])
        assert np.array_equal(same, x.astype(np.float64))
        assert np.array_equal(imresize_host(x, scale=1.0), same)
    batch = rs.randint(0, 256, (3, 2, 6, 9)).astype(np.uint8)
    got = imresize_host(batch, output_shape=(9, 5))
    assert got.shape == (3, 2, 9, 5) and np.array_equal(got[1, 1], imresize_host(batch[1, 1], output_shape=(9, 5)))
    x = rs.randint(0, 1024, (2, 9, 13)).astype(np.uint16)
    wild = x.copy()
    at = rs.rand(*x.shape) < 0.2
    x[at] = 1023
    wild[at] = rs.randint(1024, 65536, int(at.sum())).astype(np.uint16)
    for out in ("f32", "int"):
        assert np.array_equal(imresize_host(wild, scale=0.75, out=out), imresize_host(x, scale=0.75, out=out))
    assert imresize_host(wild, scale=1.5, out="int").max() <= 1023


def test_pass_order_follows_the_smaller_scale():
    """(2h, w//2): the column pass runs first.  The other order rounds differently somewhere on a random plane."""
    from fcvsr_amd.harness.resize import imresize_host, resize_geometry, resize_tables
    assert resize_geometry(12, 16, output_shape=(24, 8))[2] is False
    assert resize_geometry(12, 16, output_shape=(4, 48))[2] is True
    assert resize_geometry(12, 16, scale=1.5)[2] is True                                  # a tie: rows first
    x = np.random.RandomState(7).random_sample((12, 16)).astype(np.float32)
    got = imresize_host(x, output_shape=(24, 8))
    wx, ix = resize_tables(16, 8, 0.5)
    wy, iy = resize_tables(12, 24, 2.0)
    mid = sum((wx[:, k] * x[:, ix[:, k]] for k in range(1, wx.shape[1])), wx[:, 0] * x[:, ix[:, 0]])
    want = sum((wy[:, k, None] * mid[iy[:, k]] for k in range(1, wy.shape[1])), wy[:, 0, None] * mid[iy[:, 0]])
    assert want.dtype == np.float32 and np.array_equal(got, want.astype(np.float64))


@pytest.mark.parametrize("scale", [1 / 8, 0.3, 1 / 3, 0.5, 2 / 3, 0.75, 0.9, 1.0, 1.25, 1.5, 3.0, 8.0])
def test_table_properties(scale):
    from fcvsr_amd.harness.resize import MAX_TAPS, resize_taps, resize_tables
    for n_in in (1, 2, 7, 40):
        n_out = int(math.ceil(scale * n_in))
        w, idx = resize_tables(n_in, n_out, scale)
        stored = math.ceil(4 / min(scale, 1.0)) + 2
        assert w.dtype == np.float32 and idx.dtype == np.int32 and w.shape == idx.shape and w.shape[0] == n_out
        assert 1 <= w.shape[1] <= stored <= MAX_TAPS
        assert idx.min() >= 0 and idx.max() < n_in
        # each weight is a quotient by the f32 row sum: the quotient's and the sum's roundings, half an ulp per tap each, on
        # weights whose magnitudes add up to under 2
        assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 2 * w.shape[1] * 2.0 ** -23
        assert np.any(w[:, 0]) and np.any(w[:, -1])               # the outer all-zero taps are left out
        w2, first = resize_taps(n_in, n_out, scale)
        assert np.array_equal(w2, w) and first.dtype == np.int32 and first.shape == (n_out,)
        # what the kernel's LDS tile relies on: first never decreases, and the 8 rows / 32 columns of a tile span at most
        # 7 * 8 + 2 / 31 * 8 + 2 inputs before the taps
        assert np.all(np.diff(first) >= 0)
        assert all(np.all(first[k:] - first[:-k] <= k * 8 + 1) for k in (7, 31) if k < n_out)
        m = np.mod(first[:, None].astype(np.int64) + np.arange(w.shape[1]), 2 * n_in)
        assert np.array_equal(idx, np.where(m < n_in, m, 2 * n_in - 1 - m))
    assert resize_tables(40, 5, 1 / 8)[0].shape[1] >= 32
    if scale == 0.75:
        assert stored == 8
    if scale == 1 / 8:
        assert stored == 34


def test_error_cases():
    from fcvsr_amd.harness.resize import imresize_host, resize_tables
    x = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="exactly one"):
        imresize_host(x)
    with pytest.raises(ValueError, match="exactly one"):
        imresize_host(x, scale=2, output_shape=(16, 16))
    for bad in (0.1, 8.5, 0, -1, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            imresize_host(x, scale=bad)
    for bad in ((0, 8), (8, 65), (8,), (8.5, 8), "ab", (-8, 8)):
        with pytest.raises(ValueError, match="output_shape"):
            imresize_host(x, output_shape=bad)
    with pytest.raises(ValueError, match="int"):
        imresize_host(x.astype(np.float32), scale=2, out="int")
    with pytest.raises(ValueError, match="out"):
        imresize_host(x, scale=2, out="u8")
    with pytest.raises(ValueError, match="uint8, uint16 or f32"):
        imresize_host(x.astype(np.float64), scale=2)
    with pytest.raises(ValueError, match="non-empty"):
        imresize_host(np.zeros((0, 4), dtype=np.uint8), scale=2)
    with pytest.raises(ValueError, match="non-empty"):
        imresize_host(np.zeros(4, dtype=np.uint8), scale=2)
    with pytest.raises(ValueError):
        resize_tables(8, 1, 1 / 16)
    assert imresize_host(x, output_shape=(1, 64)).shape == (1, 64)                        # the two ends of the range


def test_device_wrappers_check_before_any_launch():
    """Host tensors raise (no CPU fallback); the argument errors need no device."""
    import torch
    from fcvsr_amd import hip
    from fcvsr_amd.harness.resize import imresize
    p = inspect.signature(imresize).parameters
    assert list(p) == ["x", "scale", "output_shape", "out"] and p["out"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["scale"].default is None and p["output_shape"].default is None and p["out"].default == "f32"
    assert list(inspect.signature(hip.imresize).parameters) == ["x", "scale", "output_shape", "out"]
    for fn in (imresize, hip.imresize):
        with pytest.raises(TypeError):
            fn(np.zeros((4, 4), dtype=np.uint8), scale=2)
        for dtype in (torch.uint8, torch.uint16, torch.float32):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(torch.zeros(1, 1, 4, 4, dtype=dtype), scale=2)


def test_new_symbol_is_declared_bound_and_exported_at_abi_version_2():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"#define\s+FCVSR_ABI_VERSION\s+2\b", hdr)
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build())
    name = "fcvsr_imresize"
    assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
    assert name in hip.SIGNATURES, f"{name} has no row in hip.SIGNATURES"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES[name]) == 17
    assert hip.lib().fcvsr_abi_version() == 2
    fn = hip.lib().fcvsr_imresize
    # FCVSR_E_ARG before any device call.  good: u8 -> f32, 8x8 -> 12x12, 6 taps
    good = dict(src=4096, sd=hip.U8, planes=1, H=8, W=8, Ho=12, Wo=12, wy=8192, fy=12288, Py=6, wx=16384, fx=20480, Px=6, rf=1,
                out=24576, od=hip.F32)
    bad = [dict(src=None), dict(out=None), dict(wy=None), dict(fy=None), dict(wx=None), dict(fx=None),
           dict(planes=0), dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=0), dict(Py=0), dict(Py=35), dict(Px=0), dict(Px=35),
           dict(sd=hip.F32, od=hip.U8), dict(sd=hip.U8, od=hip.U16), dict(sd=hip.U16, od=hip.U8), dict(sd=hip.BF16), dict(od=hip.BF16),
           dict(out=24578), dict(sd=hip.U16, src=4097), dict(wy=8194), dict(fx=20482),
           dict(Ho=65), dict(H=8, Ho=1, W=17, Wo=2)]
    for change in bad:
        a = {**good, **change}
        assert fn(*a.values(), None) == -1, change


def test_harness_surface():
    import torch
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb, upscale_yuv420
    for fn in (super_resolve_sequence, evaluate_sequence, super_resolve_yuv420, super_resolve_yuv420_rgb, upscale_yuv420):
        p = inspect.signature(fn).parameters["output_shape"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    lr, hr = torch.zeros(2, 1, 4, 4, dtype=torch.uint8), torch.zeros(2, 1, 16, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="hr must be"):                        # hr is (N,C,Ho,Wo) with the keyword
        evaluate_sequence(object(), lr, hr, output_shape=(12, 12))
    with pytest.raises(ValueError, match="hr must be"):
        evaluate_sequence(object(), lr, torch.zeros(2, 1, 12, 12, dtype=torch.uint8))
    # the range, before any model pass (the model is never touched): relative to the 4x frame, and to LR for the baseline
    with pytest.raises(ValueError, match=r"outside \[1/8, 8\]"):
        super_resolve_sequence(object(), lr, output_shape=(1, 16))
    with pytest.raises(ValueError, match=r"outside \[1/8, 8\]"):
        evaluate_sequence(object(), lr, torch.zeros(2, 1, 16, 129, dtype=torch.uint8), output_shape=(16, 129))
    with pytest.raises(ValueError, match=r"outside \[1/8, 8\]"):
        evaluate_sequence(object(), lr, torch.zeros(2, 1, 40, 16, dtype=torch.uint8), output_shape=(40, 16), baseline="bicubic")
    for call in (lambda s: super_resolve_yuv420(object(), "absent_8x8.yuv", "absent.out", 8, 8, output_shape=s),
                 lambda s: super_resolve_yuv420_rgb(object(), "absent_8x8.yuv", "absent.out", 8, 8, output_shape=s),
                 lambda s: upscale_yuv420("absent_8x8.yuv", "absent.out", 8, 8, output_shape=s)):
        for odd in ((23, 24), (24, 23)):
            with pytest.raises(ValueError, match="even"):
                call(odd)
        with pytest.raises(ValueError, match="output_shape"):
            call((24,))
    with pytest.raises(ValueError, match=r"outside \[1/8, 8\]"):              # chroma goes from LR straight to (Ho/2, Wo/2)
        super_resolve_yuv420(object(), "absent_8x8.yuv", "absent.out", 8, 8, output_shape=(80, 80))
    with pytest.raises(ValueError, match="factor"):
        upscale_yuv420("absent_8x8.yuv", "absent.out", 8, 8, factor=2, output_shape=(24, 24))
