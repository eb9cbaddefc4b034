"""Host: the bicubic up-scale contract (fcvsr_amd/harness/niqe.py bicubic_upscale) against the reference's recorded outputs
(tests/golden/upscale_cases.npz, made by tests/golden/make_golden_upscale.py), its tap tables, the integer form, the error cases, and
the C ABI / binding / harness surface of the new entry point."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = ("1x1", "1x9", "9x1", "2x3", "5x7", "12x16", "37x23")
KINDS = ("u8", "u10", "f32")
INT_TAPS = {4: [[-45, 399, 745, -75], [-7, 93, 987, -49], [-49, 987, 93, -7], [-75, 745, 399, -45]],
            2: [[-3, 29, 111, -9], [-9, 111, 29, -3]]}


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "upscale_cases.npz"))


def _names():
    return [f"{s}_{k}" for s in SIZES for k in KINDS] + ["const_5x7_u8", "checker_8x10_u8"]


def test_the_fixture_holds_every_case(cases):
    for name in _names():
        assert f"in_{name}" in cases.files
        for factor in (2, 4):
            h, w = cases[f"in_{name}"].shape
            assert cases[f"out_{name}_x{factor}"].shape == (factor * h, factor * w)
    assert cases["in_37x23_u10"].dtype == np.uint16 and cases["in_37x23_u10"].max() <= 1023
    assert cases["in_37x23_f32"].dtype == np.float32 and cases["in_37x23_u8"].dtype == np.uint8


@pytest.mark.parametrize("factor", [2, 4])
def test_contract_has_the_bits_of_the_reference(cases, factor):
    from fcvsr_amd.harness.niqe import bicubic_upscale
    for name in _names():
        got, ref = bicubic_upscale(cases[f"in_{name}"], factor), cases[f"out_{name}_x{factor}"]
        assert got.dtype == np.float64 and got.shape == ref.shape, name
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got), name          # every value is an f32
        assert np.array_equal(got, ref.astype(np.float64)), name
    const = bicubic_upscale(cases["in_const_5x7_u8"], factor)
    assert np.array_equal(const, np.full_like(const, 201.0))
    batch = np.stack([cases["in_5x7_f32"], cases["in_5x7_f32"][::-1]])                       # leading axes are batch axes
    assert np.array_equal(bicubic_upscale(batch, factor)[1], bicubic_upscale(cases["in_5x7_f32"][::-1], factor))


def test_taps_are_the_cubic_at_the_output_phases():
    from fcvsr_amd.harness.niqe import UPSCALE_TAPS

    def cubic(x):
        x = np.abs(x)
        return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x <= 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))

    assert sorted(UPSCALE_TAPS) == [2, 4]
    for f, denom in ((2, 128), (4, 1024)):
        t = UPSCALE_TAPS[f]
        assert t.shape == (f, 4)
        assert np.array_equal(t * denom, np.array(INT_TAPS[f], dtype=np.float64))
        assert all(row.sum() == 1.0 for row in t)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)                    # exact in f32
        for o in range(f):
            c = (o + 0.5) / f - 0.5
            assert np.array_equal(t[o], cubic(c - (np.floor(c) - 1 + np.arange(4))))


@pytest.mark.parametrize("factor", [2, 4])
def test_integer_form_is_the_clipped_rounded_golden(cases, factor):
    from fcvsr_amd.harness.niqe import bicubic_upscale
    for name in _names():
        x = cases[f"in_{name}"]
        if x.dtype == np.float32:
            continue
        peak = 255 if x.dtype == np.uint8 else 1023
        got = bicubic_upscale(x, factor, out="int")
        assert got.dtype == x.dtype, name
        assert np.array_equal(got, np.around(np.clip(cases[f"out_{name}_x{factor}"], 0, peak)).astype(x.dtype)), name
    chk = cases[f"out_checker_8x10_u8_x{factor}"]
    assert (chk < 0).any() and (chk > 255).any()                                             # the clip does something
    got = bicubic_upscale(cases["in_checker_8x10_u8"], factor, out="int")
    assert got.min() == 0 and got.max() == 255
    # half to even: 0.5 -> 0, 1.5 -> 2 (a constant plane of k + 0.5 cannot be made from integers, so check the rounding rule itself)
    assert np.array_equal(np.around(np.array([0.5, 1.5, 2.5])), [0.0, 2.0, 2.0])


def test_uint16_samples_above_1023_read_as_1023(cases):
    from fcvsr_amd.harness.niqe import bicubic_upscale
    x = cases["in_5x7_u10"].copy()
    wild = x.copy()
    x[1, 2], x[4, 6], x[0, 0] = 1023, 1023, 1023
    wild[1, 2], wild[4, 6], wild[0, 0] = 1024, 65535, 4000
    for factor in (2, 4):
        assert np.array_equal(bicubic_upscale(wild, factor), bicubic_upscale(x, factor))
        assert np.array_equal(bicubic_upscale(wild, factor, out="int"), bicubic_upscale(x, factor, out="int"))
        assert bicubic_upscale(wild, factor, out="int").max() <= 1023


def test_down_of_up_of_a_constant_is_the_constant():
    from fcvsr_amd.harness.niqe import bicubic_downscale, bicubic_upscale
    for factor in (2, 4):
        for value, dtype in ((201, np.uint8), (1023, np.uint16), (0.625, np.float32)):
            const = np.full((6, 10), value, dtype=dtype)
            back = bicubic_downscale(bicubic_upscale(const, factor), factor)
            assert back.shape == (6, 10) and np.array_equal(back, np.full((6, 10), float(value)))


def test_error_cases():
    from fcvsr_amd.harness.niqe import bicubic_upscale
    for bad_factor in (1, 3, 8, 2.5, 0.5):
        with pytest.raises(ValueError, match="factor"):
            bicubic_upscale(np.zeros((8, 8)), bad_factor)
    with pytest.raises(ValueError, match="int"):
        bicubic_upscale(np.zeros((4, 4), dtype=np.float32), 4, out="int")
    with pytest.raises(ValueError, match="int"):
        bicubic_upscale(np.zeros((4, 4), dtype=np.float64), 2, out="int")
    with pytest.raises(ValueError, match="out"):
        bicubic_upscale(np.zeros((4, 4), dtype=np.uint8), 4, out="u8")
    with pytest.raises(ValueError, match="non-empty"):
        bicubic_upscale(np.zeros((0, 4)), 4)
    with pytest.raises(ValueError, match="non-empty"):
        bicubic_upscale(np.zeros(4), 4)


def test_device_wrappers_check_before_any_launch():
    """Host tensors raise (no CPU fallback); the argument errors need no device."""
    import torch
    from fcvsr_amd import hip
    from fcvsr_amd.harness.resize import bicubic_upscale
    assert inspect.signature(bicubic_upscale).parameters["out"].default == "f32"
    assert inspect.signature(bicubic_upscale).parameters["out"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(hip.bicubic_upscale).parameters["out"].default == "f32"
    with pytest.raises(TypeError):
        bicubic_upscale(np.zeros((4, 4), dtype=np.uint8), 4)
    for dtype in (torch.uint8, torch.uint16, torch.float32):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            bicubic_upscale(torch.zeros(1, 1, 4, 4, dtype=dtype), 4)


def test_new_symbol_is_declared_bound_and_exported_at_abi_version_2():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"#define\s+FCVSR_ABI_VERSION\s+2\b", hdr)
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build())
    name = "fcvsr_bicubic_upscale"
    assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
    assert name in hip.SIGNATURES, f"{name} has no row in hip.SIGNATURES"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES[name]) == 9
    assert hip.lib().fcvsr_abi_version() == 2
    assert callable(hip.bicubic_upscale)
    # argument errors return FCVSR_E_ARG before any device call: null pointers, and with non-null ones a bad factor, a bad dtype pair
    # and empty sizes
    fn = hip.lib().fcvsr_bicubic_upscale
    assert fn(None, hip.U8, 1, 4, 4, 4, None, hip.F32, None) == -1
    for args in ((hip.U8, 1, 4, 4, 3, hip.F32), (hip.U8, 1, 4, 4, 4, hip.U16), (hip.F32, 1, 4, 4, 4, hip.U8), (hip.BF16, 1, 4, 4, 4, hip.F32),
                 (hip.U8, 0, 4, 4, 4, hip.U8), (hip.U8, 1, 0, 4, 4, hip.U8), (hip.U8, 1, 4, 0, 2, hip.U8)):
        sd, planes, H, W, factor, od = args
        assert fn(4096, sd, planes, H, W, factor, 8192, od, None) == -1, args


def test_harness_surface():
    import torch
    from fcvsr_amd.harness.infer import SequenceScores, evaluate_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, upscale_yuv420
    assert inspect.signature(evaluate_sequence).parameters["baseline"].default is None
    s = SequenceScores(np.zeros(1), np.zeros(1), 0.0, 0.0)                                   # positional construction keeps working
    for name in ("baseline_psnr", "baseline_ssim", "baseline_psnr_mean", "baseline_ssim_mean", "baseline_niqe", "baseline_niqe_mean"):
        assert getattr(s, name) is None
    s.baseline_psnr = np.ones(1)
    assert SequenceScores(np.zeros(1), np.zeros(1), 0.0, 0.0).baseline_psnr is None          # set per instance
    with pytest.raises(ValueError, match="baseline"):
        evaluate_sequence(object(), torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 16, 16, dtype=torch.uint8), baseline="bilinear")
    p = inspect.signature(upscale_yuv420).parameters
    assert [p[k].default for k in ("factor", "bit_depth", "batch")] == [4, 8, 8]
    assert list(p)[:4] == ["src", "dst", "width", "height"]
    assert "baseline" not in inspect.signature(super_resolve_yuv420).parameters
    with pytest.raises(ValueError, match="factor"):
        upscale_yuv420("absent_8x8.yuv", "absent.out", 8, 8, factor=3)
