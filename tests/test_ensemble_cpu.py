"""Host: the self-ensemble's specification functions against the recorded behaviour of the reference class
(tests/golden/ensemble_order.npz, made by tests/golden/make_golden_ensemble.py), the temporal extension, the C ABI / binding of the
two kernels, and the harness keyword's validation (which happens before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("fcvsr_ensemble_windows", "fcvsr_ensemble_windows_u8", "fcvsr_ensemble_windows_u16", "fcvsr_ensemble_merge")


def standin(t: torch.Tensor) -> torch.Tensor:
    """The stand-in model of make_golden_ensemble.py, restated: (B,7,C,H,W) -> (B,C,4H,4W), not equivariant."""
    o = (t[:, 3] + 0.5 * t[:, 0]).repeat_interleave(4, -2).repeat_interleave(4, -1)
    y = torch.arange(o.shape[-2], dtype=torch.float32)[:, None]
    x = torch.arange(o.shape[-1], dtype=torch.float32)[None, :]
    return o * (1.0 + 0.01 * y + 0.0001 * x)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ensemble_order.npz"))


def test_restore_inverts_variant_on_a_non_square_array():
    from fcvsr_amd.harness.ensemble import restore_host, variant_host
    a = np.random.RandomState(0).rand(2, 3, 5, 7).astype(np.float32)
    t = torch.from_numpy(a)
    seen = set()
    for i in range(8):
        v = variant_host(a, i)
        assert v.shape == ((2, 3, 7, 5) if i & 4 else (2, 3, 5, 7))
        assert np.array_equal(restore_host(v, i), a)
        assert torch.equal(restore_host(variant_host(t, i), i), t)
        assert np.array_equal(variant_host(t, i).numpy(), v)          # numpy and torch forms agree
        seen.add(v.tobytes())
    assert len(seen) == 8                                              # eight different variants
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            variant_host(a, bad)
        with pytest.raises(ValueError):
            restore_host(a, bad)


def test_variants_are_the_tensors_the_reference_hands_its_model(golden):
    from fcvsr_amd.harness.ensemble import variant_host
    x = golden["x"]
    assert x.shape == (1, 7, 2, 6, 10)
    for i in range(8):
        assert np.array_equal(variant_host(x, i), golden[f"in_{i}"]), i


def test_ensemble_host_matches_the_reference_output(golden):
    from fcvsr_amd.harness.ensemble import ensemble_host
    got = ensemble_host(torch.from_numpy(golden["x"]), standin).numpy()
    ref = golden["out"]
    assert got.shape == ref.shape == (1, 2, 24, 40) and got.dtype == np.float32
    # two orders of an 8-term f32 sum: at most 7 roundings each of partial sums <= 8 max|o|, divided by 8
    atol = 16 * 2.0 ** -24 * float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"ensemble_host vs reference: max-abs {err:.3e}, bound {atol:.3e}")
    assert err <= atol


def test_ensemble_host_padding_rule():
    """multiple=4: every variant is padded at its own bottom / right and the output cropped to its own top-left."""
    from fcvsr_amd.harness.ensemble import ensemble_host, restore_host, variant_host
    win = torch.from_numpy(np.random.RandomState(1).rand(1, 7, 1, 6, 9).astype(np.float32))
    shapes = []

    def fn(t):
        shapes.append(tuple(t.shape[-2:]))
        return standin(t)

    got = ensemble_host(win, fn, multiple=4)
    assert shapes == [(8, 12)] * 4 + [(12, 8)] * 4
    acc = None
    for i in range(8):
        v = variant_host(win, i)
        vh, vw = v.shape[-2:]
        o = standin(torch.nn.functional.pad(v, (0, (-vw) % 4, 0, (-vh) % 4)))[..., :4 * vh, :4 * vw]
        acc = restore_host(o, i) if acc is None else acc + restore_host(o, i)
    assert torch.equal(got, acc * 0.125) and got.shape == (1, 1, 24, 36)


def test_temporal_host_spec_is_the_mean_of_the_two_means():
    from fcvsr_amd.harness.ensemble import ensemble_host
    win = torch.from_numpy(np.random.RandomState(2).rand(2, 7, 1, 6, 10).astype(np.float32))
    fwd = ensemble_host(win, standin)
    rev = ensemble_host(win.flip(1), standin)
    got = ensemble_host(win, standin, temporal=True)
    assert torch.equal(got, (fwd + rev) * 0.5)
    assert not torch.equal(got, fwd)                                   # the stand-in reads frames 0 and 3: time reversal matters


def test_new_symbols_are_declared_bound_and_exported_at_abi_version_2():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert re.search(r"#define\s+FCVSR_ABI_VERSION\s+2\b", hdr)
    declared = set(re.findall(r"\b(fcvsr_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fcvsr_hip.h"
        assert name in hip.SIGNATURES, f"{name} has no row in hip.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES["fcvsr_ensemble_windows"]) == 12
    assert len(hip.SIGNATURES["fcvsr_ensemble_windows_u8"]) == len(hip.SIGNATURES["fcvsr_ensemble_windows_u16"]) == 13
    assert len(hip.SIGNATURES["fcvsr_ensemble_merge"]) == 12
    assert hip.lib().fcvsr_abi_version() == 2
    assert callable(hip.ensemble_windows) and callable(hip.ensemble_merge)


def test_wrappers_reject_host_tensors_without_a_fallback():
    from fcvsr_amd import hip
    from fcvsr_amd.harness.ensemble import SelfEnsemble
    idx = torch.zeros(1, 7, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.ensemble_windows(torch.zeros(3, 1, 6, 10), idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.ensemble_merge(torch.zeros(4, 1, 1, 32, 48), torch.zeros(4, 1, 1, 48, 32), 6, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SelfEnsemble(object())(torch.zeros(1, 7, 1, 8, 8))
    with pytest.raises(ValueError):
        hip.ensemble_windows(torch.zeros(3, 1, 6, 10, dtype=torch.float64), idx)
    with pytest.raises(ValueError):
        hip.ensemble_windows(torch.zeros(3, 1, 6, 10), idx.long())


@pytest.mark.parametrize("bad", ["temporal", "SPATIAL", "", 8, True])
def test_bad_ensemble_value_raises_before_touching_the_device(bad, tmp_path):
    from fcvsr_amd.harness.infer import evaluate_sequence, super_resolve_sequence
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, super_resolve_yuv420_rgb
    model = object()                                                   # never looked at: the keyword is checked first
    lr = torch.zeros(3, 1, 8, 8)
    hr = torch.zeros(3, 1, 32, 32, dtype=torch.uint8)
    missing = str(tmp_path / "absent_8x8.yuv")
    with pytest.raises(ValueError, match="ensemble"):
        super_resolve_sequence(model, lr, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        evaluate_sequence(model, lr, hr, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        super_resolve_yuv420(model, missing, missing + ".out", 8, 8, ensemble=bad)
    with pytest.raises(ValueError, match="ensemble"):
        super_resolve_yuv420_rgb(model, missing, missing + ".out", 8, 8, ensemble=bad)


def test_accepted_ensemble_values():
    from fcvsr_amd.harness.ensemble import MODES, SelfEnsemble, check_mode, for_mode
    assert MODES == (None, "spatial", "spatial+temporal")
    for mode in MODES:
        assert check_mode(mode) == mode
    assert for_mode(object(), None) is None
    assert isinstance(for_mode(object(), "spatial"), SelfEnsemble) and not for_mode(object(), "spatial").temporal
    assert for_mode(object(), "spatial+temporal").temporal
