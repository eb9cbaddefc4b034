"""No GPU: tests/infer_conv_refs.py is right, its bounds discriminate, and its cases declare the dispatch the planner takes.

(a) With rounding off the reference equals a plain F.conv2d / F.prelu / F.pixel_shuffle composition to 1e-12 of the largest entry.
(b) At the shapes and inputs of EVERY case of tests/test_infer_conv_gpu.py: the reference evaluated in f32 and stored in the case's
    destination dtype stays inside `bound` everywhere (the bound accepts a correct kernel), and every deliberately wrong f64 variant
    that can differ at the case (infer_conv_refs.cannot_differ) leaves it at one element or more (it rejects a wrong one).
(c) fcvsr_conv2d_mfma_plan gives, for synthetic addresses, the kernel string each case declares under its policy; every kernel string
    recorded in tests/golden/conv_plan_table.json is declared by a case."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F

import infer_conv_refs as R
from infer_kernel_refs import F32
from test_conv_plan_cpu import _descs

MFMA = R.mfma_cases()
F32C = R.f32_cases()


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------

PLAIN = [
    R.problem("plain_3src", 3, [8, 4, 4], 12, [(5, 7)], 2, "bf16", "f32", src="f32", act=2, slope=0.1),
    R.problem("plain_s2", 3, [8], 8, [(5, 7), (4, 6)], 2, "bf16", "f32", stride=2, act=1),
    R.problem("plain_ps", 1, [8], 16, [(5, 7)], 2, "f16", "f16", ps=True, act=3, slope_v=-0.1),
    R.problem("plain_2res", 3, [8], 8, [(5, 7)], 2, "bf16", "bf16", nres=2, act=0),
    R.problem("plain_ps_res", 3, [8], 16, [(3, 4)], 1, "bf16", "f32", ps=True, nres=1, res="f32", act=2, slope=1.5),
]


@pytest.mark.parametrize("p", PLAIN, ids=lambda p: p["name"])
def test_reference_equals_plain_torch(p):
    inp = R.make_inputs(p)
    outs = R.conv_ref(p, inp, rounding=False)
    for gi, o in zip(inp["groups"], outs):
        x = torch.cat([s.double() for s in gi["srcs"]], 3).permute(0, 3, 1, 2)
        y = F.conv2d(x, inp["w"].double(), inp["bias"].double(), stride=p["stride"], padding=p["ksize"] // 2)
        if p["act"] == 1:
            y = F.relu(y)
        elif p["act"] == 2:
            y = F.leaky_relu(y, float(torch.tensor(p["slope"], dtype=torch.float32)))
        elif p["act"] == 3:
            y = F.prelu(y, inp["slope_t"].double())
        for q, r in enumerate(gi["res"]):
            y = y + p["res_scale"][q] * r.double().permute(0, 3, 1, 2)
        if p["pixel_shuffle"]:
            y = F.pixel_shuffle(y, 2)
        y = y.permute(0, 2, 3, 1)
        assert o["ref"].shape == y.shape
        assert float((o["ref"] - y).abs().max()) <= 1e-12 * float(y.abs().max())


def test_conv_last_reference_equals_plain_torch():
    for cimg in (1, 3):
        q = R.conv_last_inputs(cimg, torch.bfloat16, 2, 3, 5)
        ref, _ = R.conv_last_ref(q, cimg)
        w = q["wl"].double()[:9 * cimg].view(3, 3, cimg, 64).permute(2, 3, 0, 1)
        y = F.conv2d(q["u"].double().permute(0, 3, 1, 2), w, q["bias"].double(), padding=1).permute(0, 2, 3, 1) + q["base"].double()
        assert float((ref - y).abs().max()) <= 1e-12 * float(y.abs().max())


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------

def _outside(got, ref, bound):
    """Does `got` leave the bound anywhere (a non-finite value counts as outside)?"""
    err = (got.double() - ref.double()).abs()
    return bool((~(err <= bound)).any())


def _leaves(p, o_w, o_r):
    """Does the wrong evaluation o_w (per group) leave the reference's bounds o_r at one element or more?"""
    for w, r in zip(o_w, o_r):
        if _outside(w["ref"], r["ref"], r["bound"]):
            return True
        if p["gc"] and (_outside(w["tiles"]["lse"], r["tiles"]["lse"], r["tiles"]["b_lse"]) or
                        _outside(w["tiles"]["mu"], r["tiles"]["mu"], r["tiles"]["b_mu"])):
            return True
    return False


@pytest.mark.parametrize("c", MFMA + F32C, ids=lambda c: c["id"])
def test_bounds_accept_f32_and_reject_wrong_variants(c):
    p = c["problem"]
    inp = R.make_inputs(p)
    ref_fn = R.gc_ref if p["gc"] else R.conv_ref
    o_r = ref_fn(p, inp)
    o_32 = ref_fn(p, inp, cd=F32)
    for gs, a, r in zip(p["groups"], o_32, o_r):
        stored = a["ref"].to(R.DT[gs["dst"]["dtype"]])
        assert not _outside(stored, r["ref"], r["bound"]), "f32 evaluation outside the element bound"
        if p["gc"]:
            for key in ("lse", "mu"):
                assert not _outside(a["tiles"][key], r["tiles"][key], r["tiles"]["b_" + key]), f"f32 evaluation outside the {key} bound"
            assert not _outside(a["add"], r["add"], r["b_add"]), "f32 evaluation outside the add bound"
    missed = [w for w in R.WRONG if not R.cannot_differ(p, w) and not _leaves(p, ref_fn(p, inp, wrong=w), o_r)]
    assert not missed, missed


@pytest.mark.parametrize("c", R.gc_cases(), ids=lambda c: c["id"])
def test_add_bound_rejects_a_wrong_finish(c):
    """The bound of the image-level vector is wide (module docstring of infer_conv_refs) but not empty: the leaky slope on the wrong side
    leaves it at every level, a first partial that never arrives at one level or more."""
    from freq_kernel_refs import gc_context, tile_partition
    p = c["problem"]
    inp = R.make_inputs(p)
    dropped = []
    for r in R.gc_ref(p, inp):
        q = dict(r=r["ref"], wmask=inp["wmask"], w1=inp["w1"], w2=inp["w2"])
        assert _outside(gc_context(q, tile_partition, wrong="lreluside")[0], r["add"], r["b_add"])
        dropped.append(_outside(gc_context(q, tile_partition, wrong="droptile")[0], r["add"], r["b_add"]))
    assert any(dropped)


@pytest.mark.parametrize("case", R.CONV_LAST_CASES, ids=lambda c: f"c{c[0]}-{str(c[1])[6:]}-{c[3]}x{c[4]}")
def test_conv_last_bound_accepts_f32_and_rejects_clamp_padding(case):
    cimg, dt, B, H, W = case
    q = R.conv_last_inputs(cimg, dt, B, H, W)
    ref, bound = R.conv_last_ref(q, cimg)
    assert not _outside(R.conv_last_ref(q, cimg, cd=F32)[0], ref, bound)
    assert _outside(R.conv_last_ref(q, cimg, pad="clamp")[0], ref, bound)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planner():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    lib = ctypes.CDLL(build())
    lib.fcvsr_conv2d_mfma_plan.argtypes = hip.SIGNATURES["fcvsr_conv2d_mfma_plan"]
    lib.fcvsr_last_error.restype = ctypes.c_char_p

    def plan(p, lean, res):
        descs, n = _descs(hip, p)
        name = ctypes.create_string_buffer(96)
        rc = lib.fcvsr_conv2d_mfma_plan(descs, n, hip.BF16 if p["mma"] == "bf16" else hip.F16, R.LEAN[lean], R.RES[res], name, len(name))
        return name.value.decode() if rc == 0 else "rejected: " + lib.fcvsr_last_error().decode()
    return plan


def test_cases_declare_the_planned_kernel(planner):
    wrong = [(c["id"], c["kernel"], got) for c in MFMA for got in [planner(c["problem"], c["lean"], c["res"])] if got != c["kernel"]]
    assert not wrong, wrong
    assert len({c["id"] for c in MFMA + F32C}) == len(MFMA + F32C)


def test_every_recorded_kernel_string_is_declared():
    with open(R.TABLE) as f:
        tab = json.load(f)
    recorded = {r["kernel"] for p in tab["problems"] for r in p["results"].values() if "kernel" in r}
    assert len(recorded) >= 33
    assert recorded <= {c["kernel"] for c in MFMA}, recorded - {c["kernel"] for c in MFMA}


def test_now_rejected_is_the_list_of_the_plan_test():
    import test_conv_plan_cpu
    assert R.NOW_REJECTED == test_conv_plan_cpu.NOW_REJECTED
