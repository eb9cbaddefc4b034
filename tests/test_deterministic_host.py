"""Host-side checks of the deterministic training mode (no GPU needed): the two C entry points of the atomic-free IAC warp backward
are declared, bound and exported, the Python layers accept `deterministic`, and float atomics stay fenced inside the scatter form
of `iac_bwd_warp_kernel`."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = ("fcvsr_iac_bwd_warp_det_workspace", "fcvsr_iac_bwd_warp_det")


def test_deterministic_entry_points_are_declared_bound_and_exported():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    lib = ctypes.CDLL(build())
    for name in DET:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fcvsr_hip.h"
        assert name in hip.SIGNATURES, name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert len(hip.SIGNATURES["fcvsr_iac_bwd_warp_det"]) == 13 and len(hip.SIGNATURES["fcvsr_iac_bwd_warp_det_workspace"]) == 5
    assert "#define FCVSR_ABI_VERSION 2" in hdr                   # additive: the ABI version stays


def test_python_layers_accept_deterministic():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.train import TrainStep
    from fcvsr_amd.train.step import fit
    from fcvsr_amd.train.blocks import iac_both
    from fcvsr_amd.train.graph import forward_train
    for fn, default in ((TrainStep.__init__, None), (fit, None), (iac_both, False), (forward_train, False)):
        par = inspect.signature(fn).parameters
        assert "deterministic" in par, fn
        assert par["deterministic"].default is default, fn
    m = GShiftNet_S(n_features=32, ACNum=1, Freq_Inv=2, SCGroupN=1)
    assert m.train_deterministic is False
    assert not any("deterministic" in k for k in m.state_dict())   # a plain attribute, like train_precision
    TrainStep(m)
    assert m.train_deterministic is False                          # None leaves the attribute alone
    TrainStep(m, deterministic=True)
    assert m.train_deterministic is True
    TrainStep(m)
    assert m.train_deterministic is True
    TrainStep(m, deterministic=False)
    assert m.train_deterministic is False
    import torch
    other = torch.nn.Linear(2, 2)                                  # not a drop-in module: the flag would change nothing there
    TrainStep(other)
    with pytest.raises(ValueError, match="train_deterministic"):
        TrainStep(other, deterministic=True)


FLOAT_ATOMIC = re.compile(r"\b(global_atomic_add_f32|global_atomic_add_f64|global_atomic_pk_add_\w+|buffer_atomic_add_f32|"
                          r"buffer_atomic_pk_add_\w+|ds_add_f32|ds_add_rtn_f32|ds_pk_add_\w+)\b")


def test_float_atomics_only_in_the_scatter_form_of_the_iac_warp_backward(tmp_path):
    """Every code object of the BUILT library is disassembled: a float atomic (global, buffer or LDS) may occur only inside an
    instantiation of `iac_bwd_warp_kernel` with its scatter on (`<NE, true>`).  Everything else - the deterministic form's source pass
    (`<NE, false>`), sort and gather included - sums in a fixed order.  Integer atomics (the library sort uses them for counts) are
    not matched on purpose."""
    from fcvsr_amd import build as B
    if shutil.which(B.HIPCC) is None:
        pytest.skip("no hipcc on this machine: nothing was built here")
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(objdump), f"{objdump} is missing although hipcc exists: the float-atomic guard cannot run"
    so = tmp_path / "libfcvsr_hip.so"
    shutil.copy(B.build(), so)
    subprocess.check_call([objdump, "--offloading", str(so)], stdout=subprocess.DEVNULL, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert len(cos) >= 10, cos
    hits = {}
    symbols = set()
    for co in cos:
        text = subprocess.check_output([objdump, "-d", "--demangle", str(tmp_path / co)]).decode()
        sym = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                sym = m.group(1)
                symbols.add(sym)
                continue
            a = FLOAT_ATOMIC.search(line)
            if a:
                hits.setdefault(sym, []).append(a.group(1))
    scatter = re.compile(r"iac_bwd_warp_kernel<\d+, true>")
    bad = {s: v for s, v in hits.items() if s is None or not scatter.search(s)}
    assert not bad, f"float atomics outside the scatter form of iac_bwd_warp_kernel: { {s: sorted(set(v)) for s, v in bad.items()} }"
    # the fence is not vacuous: the scatter form is there and has its atomics, the source pass of the deterministic form has none
    assert any(scatter.search(s) for s in hits), sorted(hits)
    assert any(re.search(r"iac_bwd_warp_kernel<\d+, false>", s) for s in symbols)
    assert any("iac_gather_kernel" in s for s in symbols)
