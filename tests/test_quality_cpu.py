"""CPU: the on-device quality metrics are wired through every layer (library export, ctypes binding, Python API) and refuse
host tensors (no CPU fallback)."""
import ctypes

import numpy as np
import pytest
import torch

NAMES = ("fcvsr_frame_metrics", "fcvsr_frame_metrics_scratch_bytes")


def test_library_exports_the_frame_metric_entry_points():
    from fcvsr_amd.build import build
    lib = ctypes.CDLL(build())
    for name in NAMES:
        assert hasattr(lib, name), name


def test_bindings_declare_the_frame_metric_entry_points():
    from fcvsr_amd import hip
    for name in NAMES:
        assert name in hip.SIGNATURES, name
    assert hip._RESTYPES["fcvsr_frame_metrics_scratch_bytes"] is ctypes.c_longlong


def test_scratch_size_counts_one_partial_pair_per_plane_and_tile():
    """16 x 64 map tiles, two f64 per (plane, tile): 720x1280, crop 4 -> 702 x 1262 map = 44 x 20 tiles."""
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    build()
    f = hip.lib().fcvsr_frame_metrics_scratch_bytes
    assert f(16, 1, 720, 1280, 4, 0) == 16 * 44 * 20 * 16
    assert f(16, 3, 720, 1280, 4, 0) == 3 * f(16, 1, 720, 1280, 4, 0)
    assert f(16, 3, 720, 1280, 4, 1) == f(16, 1, 720, 1280, 4, 0)


def test_frame_metrics_on_cpu_tensors_raises():
    from fcvsr_amd.harness.device_metrics import frame_metrics
    a = torch.from_numpy(np.ones((1, 1, 32, 32), np.uint8))
    with pytest.raises(RuntimeError):
        frame_metrics(a, a, quantise=None)
    with pytest.raises(RuntimeError):
        frame_metrics(a.float() / 255, a)
