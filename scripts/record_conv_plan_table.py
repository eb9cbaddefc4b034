"""Record which kernel fcvsr_conv2d_mfma launches for a fixed table of problems under every policy the two environment
variables can express (FCVSR_MFMA_LEAN in {unset, 0} x FCVSR_MFMA_RES in {unset, 0, 1}): the golden table that
tests/test_conv_plan_cpu.py replays through fcvsr_conv2d_mfma_plan without a GPU.

  python scripts/record_conv_plan_table.py [--out tests/golden/conv_plan_table.json]

Needs a GPU: every problem is really launched and fcvsr_last_conv_kernel() (or the text of the rejection) is recorded.  Each
entry keeps what rebuilds its descriptors with synthetic addresses: shapes, strides, dtypes, pointer alignment and keywords.
Every tensor lives at the start of a buffer of more than twice its extent: the library this table was first recorded from
let a 16-bit residual or a ContextBlock-fused 16-bit destination reach the generic kernel under FCVSR_MFMA_LEAN=0, which
addresses them as f32."""
import argparse
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fcvsr_amd import hip  # noqa: E402

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
POLICIES = [(lean, res) for lean in ("unset", "0") for res in ("unset", "0", "1")]


def T(shape, dtype, strides=None, offset=0):
    """One (b, y, x, c) tensor: dense NHWC unless `strides` (elements) says otherwise, `offset` elements into its buffer."""
    b, y, x, c = shape
    return dict(shape=list(shape), dtype=dtype, strides=list(strides or (y * x * c, x * c, c, 1)), offset=offset)


def conv3(name, cin, cout, levels, B, dst, nres, mma, act, ps=False, src=None, res=None, stride=1, **kw):
    """A 3x3 problem shaped like those of tests/test_conv_mfma_shape_gpu.py: one source per level, residuals like the output."""
    groups = []
    for (H, W) in levels:
        ho, wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
        oshape = (B, 2 * H, 2 * W, cout // 4) if ps else (B, ho, wo, cout)
        groups.append(dict(srcs=[T((B, H, W, cin), src or (mma if cin % 8 == 0 else "f32"))],
                           res=[T((B, ho, wo, cout), res or mma) for _ in range(nres)], dst=T(oshape, dst)))
    return dict(name=name, ksize=3, stride=stride, cout=cout, mma=mma, act=act, slope=0.1, slope_t=True, bias=True,
                res_scale=[1.0, -0.5][:nres], pixel_shuffle=ps, gc=False, groups=groups, **kw)


def table():
    P = []
    # tests/test_conv_mfma_shape_gpu.py: CASES, then BITWISE (B = 2)
    shape_cases = [(64, 64, [(21, 37), (11, 19), (6, 10)], 2, True, 0, "bf16", False, 2),
                   (64, 64, [(19, 70)], 3, False, 2, "bf16", False, 0),
                   (64, 128, [(40, 70), (20, 35)], 1, True, 1, "bf16", False, 2),
                   (64, 256, [(17, 33)], 1, True, 0, "f16", False, 3),
                   (128, 64, [(23, 41), (12, 21), (6, 11)], 2, False, 1, "bf16", False, 3),
                   (128, 128, [(17, 45)], 2, True, 2, "f16", False, 2),
                   (64, 256, [(13, 37)], 2, True, 0, "bf16", True, 3),
                   (64, 64, [(21, 37), (11, 19)], 2, True, 1, "bf16", False, 2),
                   (128, 64, [(17, 35)], 2, False, 0, "f16", False, 3),
                   (64, 128, [(9, 40)], 2, True, 2, "bf16", False, 0),
                   (84, 64, [(15, 29), (8, 15)], 2, False, 0, "bf16", False, 2),
                   (64, 64, [(15, 29)], 2, True, 0, "f16", False, 3),
                   (64, 256, [(11, 21)], 2, True, 0, "bf16", True, 3)]
    for i, (cin, cout, levels, B, d16, nres, mma, ps, act) in enumerate(shape_cases):
        P.append(conv3(f"shape_case{i}_{cin}to{cout}", cin, cout, levels, B, mma if d16 else "f32", nres, mma, act, ps=ps))
    bitwise = [(128, 64, [(23, 41), (12, 21)], False, 1, "bf16", 3), (128, 128, [(17, 45)], False, 0, "f16", 2),
               (64, 64, [(21, 37), (11, 19), (6, 10)], True, 1, "f16", 3), (64, 128, [(19, 70)], False, 2, "f16", 3),
               (128, 64, [(23, 41)], False, 0, "bf16", 3), (64, 64, [(21, 37)], True, 0, "f16", 3)]
    for i, (cin, cout, levels, d16, nres, mma, act) in enumerate(bitwise):
        P.append(conv3(f"bitwise{i}_{cin}to{cout}", cin, cout, levels, 2, mma if d16 else "f32", nres, mma, act))
    # tests/test_conv_pyramid_paths_gpu.py: stride 2, the 1x1 pixel-shuffle up-convolution, the 16-bit pyramid-fuse producers
    for i, (levels, B, io, mma) in enumerate([([(90, 160)], 3, "bf16", "bf16"), ([(37, 53)], 2, "f16", "f16"),
                                              ([(37, 53)], 2, "f32", "bf16"), ([(21, 70), (11, 35)], 2, "bf16", "bf16")]):
        p = conv3(f"stride2_{i}", 64, 64, levels, B, io, 0, mma, 2, src=io, stride=2)
        p["slope_t"] = False
        P.append(p)
    for cout, B, H, W, mma in [(256, 2, 90, 160, "bf16"), (256, 1, 37, 53, "f16"), (128, 2, 45, 80, "bf16"), (32, 1, 9, 11, "bf16"),
                               (128, 1, 9, 11, "bf16")]:
        P.append(dict(name=f"upconv1_ps_{cout}_{H}x{W}", ksize=1, stride=1, cout=cout, mma=mma, act=3, slope=0.0, slope_t=True,
                      bias=True, res_scale=[], pixel_shuffle=True, gc=False,
                      groups=[dict(srcs=[T((B, H, W, 64), mma)], res=[], dst=T((B, 2 * H, 2 * W, cout // 4), mma))]))
    for dst in ("f32", "bf16"):
        p = conv3(f"groupconv_2res_dst_{dst}", 64, 64, [(24, 70), (12, 35), (6, 18)], 2, dst, 2, "bf16", 0)
        p.update(res_scale=[1.0, 1.0], slope_t=False)
        P.append(p)
    for dst in ("f32", "f16"):
        P.append(dict(name=f"upconv1_L2_2_dst_{dst}", ksize=1, stride=1, cout=64, mma="f16", act=0, slope=0.0, slope_t=False,
                      bias=True, res_scale=[1.0], pixel_shuffle=True, gc=False,
                      groups=[dict(srcs=[T((2, 23, 41, 64), "f32"), T((2, 23, 41, 16), "f32")], res=[T((2, 23, 41, 64), "f32")],
                                   dst=T((2, 46, 82, 16), dst))]))
    for i, srcs in enumerate([["f32", "f32", "f32"], ["bf16", "bf16", "bf16"]]):
        cs = [64, 16, 4 if srcs[0] == "f32" else 8]
        P.append(dict(name=f"upconv_fuse_{srcs[0]}", ksize=3, stride=1, cout=64, mma="bf16", act=0, slope=0.0, slope_t=False, bias=True,
                      res_scale=[], pixel_shuffle=False, gc=False,
                      groups=[dict(srcs=[T((1, 37, 52, c), d) for c, d in zip(cs, srcs)], res=[], dst=T((1, 37, 52, 64), "bf16"))]))
    # a planar (NCHW) f32 3-channel source
    B, H, W = 2, 19, 45
    P.append(dict(name="planar_f32_3ch", ksize=3, stride=1, cout=64, mma="bf16", act=1, slope=0.0, slope_t=False, bias=True, res_scale=[],
                  pixel_shuffle=False, gc=False,
                  groups=[dict(srcs=[T((B, H, W, 3), "f32", strides=(3 * H * W, W, 1, H * W))], res=[], dst=T((B, H, W, 64), "bf16"))]))
    # three sources, 1x1, a residual and pixel shuffle
    P.append(dict(name="conv1_3src_res_ps", ksize=1, stride=1, cout=64, mma="bf16", act=2, slope=0.2, slope_t=False, bias=True,
                  res_scale=[0.5], pixel_shuffle=True, gc=False,
                  groups=[dict(srcs=[T((2, 13, 21, 64), "f32"), T((2, 13, 21, 64), "f32"), T((2, 13, 21, 16), "f32")],
                               res=[T((2, 13, 21, 64), "f32")], dst=T((2, 26, 42, 16), "f32"))]))
    # the same 1x1 shapes the lean kernel takes: two 64-channel sources, with and without a residual
    for nres in (0, 1):
        P.append(dict(name=f"conv1_2src_r{nres}", ksize=1, stride=1, cout=64, mma="bf16", act=0, slope=0.0, slope_t=False, bias=True,
                      res_scale=[1.0][:nres], pixel_shuffle=False, gc=False,
                      groups=[dict(srcs=[T((2, 13, 21, 64), "bf16"), T((2, 13, 21, 64), "bf16")],
                                   res=[T((2, 13, 21, 64), "f32")][:nres], dst=T((2, 13, 21, 64), "bf16"))]))
    # ContextBlock fusion into an f32 and into a 16-bit destination (three levels, as BlockRCB runs it)
    for dst in ("f32", "bf16"):
        p = conv3(f"gc_fused_dst_{dst}", 64, 64, [(21, 37), (11, 19), (6, 10)], 2, dst, 0, "bf16", 0)
        p.update(gc=True, slope_t=False)
        P.append(p)
    # a destination that is a channel slice (sx > c), an NCHW f32 destination, cout = 48
    p = conv3("dst_channel_slice", 64, 64, [(17, 45)], 2, "bf16", 0, "bf16", 1)
    p["groups"][0]["dst"] = T((2, 17, 45, 64), "bf16", strides=(17 * 45 * 96, 45 * 96, 96, 1), offset=16)
    P.append(p)
    p = conv3("dst_nchw_f32", 64, 64, [(17, 45)], 2, "f32", 0, "bf16", 1)
    p["groups"][0]["dst"] = T((2, 17, 45, 64), "f32", strides=(64 * 17 * 45, 45, 1, 17 * 45))
    P.append(p)
    P.append(conv3("cout48", 64, 48, [(17, 45)], 2, "bf16", 0, "bf16", 2))
    P.append(conv3("cout48_f32_src_dst", 64, 48, [(17, 45)], 2, "f32", 0, "f16", 2, src="f32"))
    # both sides of the size rule (768 workgroup-tiles), all else equal
    for cin, BH in ((64, (3, 128)), (128, (3, 64))):
        for W in (512, 480):
            P.append(conv3(f"size_rule_{cin}to64_w{W}", cin, 64, [(BH[1], W)], BH[0], "bf16", 0, "bf16", 2))
    # the four problems of tests/test_conv_plan_gpu.py
    P.append(conv3("plan_gpu_lean3", 64, 64, [(9, 40)], 1, "bf16", 0, "bf16", 1))
    P.append(conv3("plan_gpu_s2", 64, 64, [(21, 70)], 1, "bf16", 0, "bf16", 1, stride=2))
    P.append(conv3("plan_gpu_res3", 128, 64, [(17, 45)], 1, "bf16", 0, "bf16", 1))
    # rejected whatever the policy
    p = conv3("reject_prelu_without_slope", 64, 64, [(9, 40)], 1, "bf16", 0, "bf16", 3)
    p["slope_t"] = False
    P.append(p)
    P.append(conv3("reject_ps_cout40", 64, 40, [(9, 40)], 1, "bf16", 0, "bf16", 0, ps=True))
    P.append(conv3("reject_src_6_channels", 6, 64, [(9, 40)], 1, "f32", 0, "bf16", 0))
    p = conv3("reject_1x1_stride2", 64, 64, [(9, 40)], 1, "bf16", 0, "bf16", 0, stride=2)
    p["ksize"] = 1
    P.append(p)
    return P


def alloc(spec):
    """The tensor of `spec` at the start (+ offset) of a zero buffer of more than twice its extent."""
    extent = spec["offset"] + 1 + sum((n - 1) * s for n, s in zip(spec["shape"], spec["strides"]))
    buf = torch.zeros(2 * extent + 1024, dtype=TORCH_DT[spec["dtype"]], device="cuda")
    buf[:extent] = (torch.rand(extent, device="cuda") - 0.5).to(buf.dtype)
    return buf.as_strided(spec["shape"], spec["strides"], spec["offset"])


def run(p):
    dt = TORCH_DT[p["mma"]]
    k, cout = p["ksize"], p["cout"]
    cin = sum(s["shape"][3] for s in p["groups"][0]["srcs"])
    wp = ((torch.rand(k * k, (cout + 127) // 128 * 128, (cin + 63) // 64 * 64, device="cuda") - 0.5) / (k * cin ** 0.5)).to(dt)
    bias = torch.rand(cout, device="cuda") if p["bias"] else None
    slope_t = torch.tensor([0.25], device="cuda") if p["slope_t"] else None
    wmask = torch.rand(cout, device="cuda") if p["gc"] else None
    groups = []
    for g in p["groups"]:
        G = dict(srcs=[alloc(s) for s in g["srcs"]], res=[alloc(r) for r in g["res"]], dst=alloc(g["dst"]), ps=p["pixel_shuffle"])
        if p["gc"]:
            B, H, W, _ = g["srcs"][0]["shape"]
            G["gc_partial"] = torch.zeros(B, ((H + 3) // 4) * ((W + 31) // 32), cout + 2, device="cuda")
        groups.append(G)
        for key in ("srcs", "res"):
            for spec, t in zip(g[key], G[key]):
                spec["align"] = t.data_ptr() % 256
        g["dst"]["align"] = G["dst"].data_ptr() % 256
    results = {}
    for lean, res in POLICIES:
        for var, val in (("FCVSR_MFMA_LEAN", lean), ("FCVSR_MFMA_RES", res)):
            os.environ.pop(var, None)
            if val != "unset":
                os.environ[var] = val
        try:
            hip.conv2d_mfma(groups, wp, k, cout, hip.BF16 if p["mma"] == "bf16" else hip.F16, stride=p["stride"], bias=bias, act=p["act"],
                            slope=p["slope"], slope_t=slope_t, res_scale=p["res_scale"], pixel_shuffle=p["pixel_shuffle"], gc_wmask=wmask)
            torch.cuda.synchronize()
            results[f"{lean},{res}"] = dict(kernel=hip.lib().fcvsr_last_conv_kernel().decode())
        except hip.HipError as e:
            m = re.search(r"\(rc=-?\d+\): \w+: (.*) \([^()]*:\d+\)$", str(e))
            if m is None:
                raise                   # not an argument rejection: stop here
            results[f"{lean},{res}"] = dict(error=m.group(1))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("tests", "golden", "conv_plan_table.json"))
    args = ap.parse_args()
    problems = table()
    assert len({p["name"] for p in problems}) == len(problems)
    for p in problems:
        p["results"] = run(p)
        print(p["name"], p["results"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(policies=[f"{l},{r}" for l, r in POLICIES], problems=problems), f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {len(problems)} problems x {len(POLICIES)} policies")


if __name__ == "__main__":
    main()
