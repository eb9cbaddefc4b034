"""No GPU: the decisions of fcvsr_conv2d_mfma's planner against the table recorded from real launches.

tests/golden/conv_plan_table.json (scripts/record_conv_plan_table.py) holds, for a fixed set of problems and the six policies the
environment variables FCVSR_MFMA_LEAN in {unset, 0} x FCVSR_MFMA_RES in {unset, 0, 1} can express, the kernel name
fcvsr_last_conv_kernel() reported after the launch, or the text of the rejection.  It was recorded from the dispatcher as it was
before the planner existed.  Here every descriptor is rebuilt with synthetic addresses of the recorded alignment and handed to
fcvsr_conv2d_mfma_plan, which must give the same string or the same rejection.

The one deliberate difference: 16-bit residuals and ContextBlock fusion into a 16-bit destination are layouts the generic kernel
cannot address.  The old dispatcher checked for them before it applied FCVSR_MFMA_LEAN=0 and then launched the generic kernel on
them; the planner rejects them.  NOW_REJECTED lists those problems by name; nothing else may differ."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")
LEAN = {"unset": 1, "0": 0}
RES = {"unset": 2, "0": 0, "1": 1}
MSG_RES16 = "16-bit residuals are only supported by the lean 3x3 path"
MSG_GC16 = "ContextBlock fusion with a 16-bit destination needs the lean 3x3 path, no residuals"
# problem -> the rejection it now gets under every policy with FCVSR_MFMA_LEAN=0 (recorded there: conv_mfma_kernel<...>)
NOW_REJECTED = {
    "shape_case2_64to128": MSG_RES16, "shape_case5_128to128": MSG_RES16, "shape_case7_64to64": MSG_RES16, "shape_case9_64to128": MSG_RES16,
    "shape_case1_64to64": MSG_RES16, "shape_case4_128to64": MSG_RES16,
    "bitwise0_128to64": MSG_RES16, "bitwise2_64to64": MSG_RES16, "bitwise3_64to128": MSG_RES16,
    "groupconv_2res_dst_f32": MSG_RES16, "groupconv_2res_dst_bf16": MSG_RES16,
    "gc_fused_dst_bf16": MSG_GC16,
}


@pytest.fixture(scope="module")
def planner():
    from fcvsr_amd import hip
    from fcvsr_amd.build import build
    lib = ctypes.CDLL(build())
    lib.fcvsr_conv2d_mfma_plan.argtypes = hip.SIGNATURES["fcvsr_conv2d_mfma_plan"]
    lib.fcvsr_last_error.restype = ctypes.c_char_p

    def plan(problem, lean, res):
        """{"kernel": name} or {"error": text} for one table entry under the policy (lean, res)."""
        descs, n = _descs(hip, problem)
        name = ctypes.create_string_buffer(96)
        rc = lib.fcvsr_conv2d_mfma_plan(descs, n, hip.BF16 if problem["mma"] == "bf16" else hip.F16, lean, res, name, len(name))
        if rc == 0:
            return {"kernel": name.value.decode()}
        text = lib.fcvsr_last_error().decode()                     # "fcvsr_conv2d_mfma: <text> (<file>:<line>)"
        return {"error": text[text.index(": ") + 2:text.rindex(" (")]}
    return plan


def _descs(hip, p):
    """The descriptors hip.conv2d_mfma fills for the recorded problem: every tensor at a synthetic address of its own with the
    recorded alignment (mod 256); weights, bias, slope and ContextBlock arrays at 256-byte-aligned ones."""
    code = {"f32": hip.F32, "bf16": hip.BF16, "f16": hip.F16}
    nxt = [1 << 32]

    def addr(align=0):
        nxt[0] += 1 << 32
        return nxt[0] + align

    def view(t):
        sb, sy, sx, sc = t["strides"]
        return hip.View(addr(t["align"]), sb, sy, sx, 1 if t["shape"][3] == 1 else sc, t["shape"][3], code[t["dtype"]])

    groups = p["groups"]
    descs = (hip.ConvDesc * len(groups))()
    weight, bias, slope_ptr, wmask = addr(), addr(), addr(), addr()
    for d, g in zip(descs, groups):
        d.n_src = len(g["srcs"])
        for i, s in enumerate(g["srcs"]):
            d.src[i] = view(s)
        d.B, d.H, d.W = g["srcs"][0]["shape"][:3]
        d.kh = d.kw = p["ksize"]
        d.stride, d.pad, d.cout = p["stride"], p["ksize"] // 2, p["cout"]
        d.weight, d.cout_pad = weight, (p["cout"] + 127) // 128 * 128
        d.bias = bias if p["bias"] else None
        d.act, d.slope = p["act"], p["slope"]
        d.slope_ptr = slope_ptr if p["slope_t"] else None
        d.n_res = len(g["res"])
        for i, r in enumerate(g["res"]):
            d.res[i] = view(r)
            d.res_scale[i] = p["res_scale"][i]
        d.dst = view(g["dst"])
        d.pixel_shuffle = int(p["pixel_shuffle"])
        if p["gc"]:
            d.gc_wmask, d.gc_partial = wmask, addr()
    return descs, len(groups)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_planner_reproduces_the_recorded_dispatch(planner, table):
    problems = {p["name"]: p for p in table["problems"]}
    assert len(problems) >= 50 and sorted(table["policies"]) == sorted(f"{l},{r}" for l in LEAN for r in RES)
    assert set(NOW_REJECTED) <= set(problems)
    kernels, wrong = set(), []
    for name, p in problems.items():
        for policy in table["policies"]:
            lean, res = policy.split(",")
            want = p["results"][policy]
            if name in NOW_REJECTED and lean == "0":
                assert want["kernel"].startswith("conv_mfma_kernel<"), (name, policy, want)   # what the old dispatcher launched
                want = {"error": NOW_REJECTED[name]}
            got = planner(p, LEAN[lean], RES[res])
            if got != want:
                wrong.append((name, policy, want, got))
            kernels.add(got.get("kernel", "").split("<")[0])
    assert not wrong, wrong
    # the table reaches every path and both kinds of answer
    assert kernels == {"", "conv_mfma_kernel", "conv3_lean_kernel", "conv3s2_lean_kernel", "conv1_lean_kernel", "conv1ps_res_kernel",
                       "conv3_res_kernel"}, kernels


def test_size_rule_has_both_sides(planner, table):
    problems = {p["name"]: p for p in table["problems"]}
    for cin, nch in ((64, 1), (128, 2)):
        big, small = problems[f"size_rule_{cin}to64_w512"], problems[f"size_rule_{cin}to64_w480"]
        assert planner(big, 1, 2) == {"kernel": f"conv3_res_kernel<true, 2, {nch}, 1>"}        # 768 workgroup-tiles
        assert planner(small, 1, 2) == {"kernel": "conv3_lean_kernel<true, 64, true, true>"}    # 720
        assert planner(small, 1, 1) == planner(big, 1, 2)                                       # res = 1 skips the size test


def test_planner_ignores_the_environment(planner, table, monkeypatch):
    """An explicit policy is the whole input: the variables fcvsr_conv2d_mfma reads do not reach fcvsr_conv2d_mfma_plan."""
    before = {(p["name"], pol): planner(p, LEAN[pol.split(",")[0]], RES[pol.split(",")[1]])
              for p in table["problems"] for pol in table["policies"]}
    for lean_env, res_env in (("0", "0"), ("1", "1")):
        monkeypatch.setenv("FCVSR_MFMA_LEAN", lean_env)
        monkeypatch.setenv("FCVSR_MFMA_RES", res_env)
        after = {(p["name"], pol): planner(p, LEAN[pol.split(",")[0]], RES[pol.split(",")[1]])
                 for p in table["problems"] for pol in table["policies"]}
        assert after == before


def test_plan_entry_point_is_declared_and_bound(planner):
    from fcvsr_amd import hip
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    assert "int fcvsr_conv2d_mfma_plan(const fcvsr_conv_desc* descs, int n_groups, int mma_dtype, int lean, int res, char* kernel_name, int cap)" in hdr
    assert len(hip.SIGNATURES["fcvsr_conv2d_mfma_plan"]) == 7
