"""fcvsr_rcb_tail (BlockRCB's second half in two launches) against the five-launch sequence it replaces:
fcvsr_gc_apply_levels -> 1x1 up.0 -> fcvsr_rcb_level0 -> 1x1 down.0 -> fcvsr_xscale_levels.  Every output must be
bit-identical, and so must the whole S model with the fused tail against the generic one."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _reference(L, hip, xs, rr, zz, adds, wu, bu, wd, bd, tdt, code, mdt, st):
    """The five-launch sequence (what the engine ran before the fused tail)."""
    B, n = xs[0].shape[0], 64
    H, W = xs[0].shape[1], xs[0].shape[2]
    R = [None, torch.empty_like(zz[1]), torch.empty_like(zz[2])]
    P = [torch.empty(B, H // 2, W // 2, n, device="cuda", dtype=tdt), torch.empty(B, H // 4, W // 4, n, device="cuda", dtype=tdt)]
    al = (hip.GcApplyLevel * 3)()
    for i, l in enumerate((1, 2)):
        al[i].r, al[i].add, al[i].z, al[i].out = rr[l].data_ptr(), adds[l].data_ptr(), zz[l].data_ptr(), R[l].data_ptr()
        al[i].pool = P[1].data_ptr() if l == 1 else None
        al[i].B, al[i].H, al[i].W = B, xs[l].shape[1], xs[l].shape[2]
    hip.check(L.fcvsr_gc_apply_levels(al, 2, code, code, 0.2, n, st), "gc_apply_levels")
    up = [torch.empty_like(R[1]), torch.empty_like(R[2])]
    hip.conv2d_mfma([dict(srcs=[R[l]], dst=up[l - 1]) for l in (1, 2)], wu, 1, n, mdt, bias=bu)
    outs = [torch.empty_like(x) for x in xs]
    hip.check(L.fcvsr_rcb_level0(xs[0].data_ptr(), rr[0].data_ptr(), adds[0].data_ptr(), zz[0].data_ptr(), up[0].data_ptr(),
                                 outs[0].data_ptr(), P[0].data_ptr(), 0.2, 2.0, code, B, H, W, n, st), "rcb_level0")
    dn = [torch.empty_like(P[0]), torch.empty_like(P[1])]
    hip.conv2d_mfma([dict(srcs=[P[l]], dst=dn[l]) for l in (0, 1)], wd, 1, n, mdt, bias=bd)
    xl = (hip.XscaleLevel * 3)()
    for i, l in enumerate((1, 2)):
        xl[i].x, xl[i].r, xl[i].out = xs[l].data_ptr(), R[l].data_ptr(), outs[l].data_ptr()
        xl[i].dn = dn[l - 1].data_ptr()
        xl[i].up = up[1].data_ptr() if l == 1 else None
        xl[i].r_scale = 2.0 if l == 2 else 1.0
        xl[i].dn_pooled = 1
        xl[i].B, xl[i].H, xl[i].W = B, xs[l].shape[1], xs[l].shape[2]
    hip.check(L.fcvsr_xscale_levels(xl, 2, code, n, st), "xscale_levels")
    return outs, R[1], up[0], up[1]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B,H,W", [(2, 180, 320), (1, 4, 4), (3, 12, 20), (2, 36, 68), (1, 20, 136), (3, 44, 36)])
def test_rcb_tail_equals_five_launch_sequence(dt, B, H, W):
    """Production pyramid 180x320 / 90x160 / 45x80, and small pyramids whose tiles straddle the image borders with odd
    level-2 sizes (1x1, 3x5, 9x17, 5x34, 11x9)."""
    from fcvsr_amd import hip
    L = hip.lib()
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    code = hip.BF16 if dt == "bf16" else hip.F16
    n = 64
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    sizes = [(H, W), (H // 2, W // 2), (H // 4, W // 4)]
    mk = lambda h, w: torch.randn(B, h, w, n, generator=g).to(tdt).cuda()
    xs = [mk(*s) for s in sizes]
    rr = [mk(*s) for s in sizes]
    zz = [mk(*s) for s in sizes]
    adds = [torch.randn(B, n, generator=g).cuda() for _ in sizes]
    wu = hip.pack_conv_weight_mfma((torch.randn(n, n, 1, 1, generator=g) / 8).cuda(), tdt)
    wd = hip.pack_conv_weight_mfma((torch.randn(n, n, 1, 1, generator=g) / 8).cuda(), tdt)
    bu, bd = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    st = hip.stream_ptr()
    ref, R1_ref, U1_ref, U2_ref = _reference(L, hip, xs, rr, zz, adds, wu, bu, wd, bd, tdt, code, code, st)

    outs = [torch.full_like(x, float("nan")) for x in xs]
    R1, U1, U2 = (torch.full_like(zz[1], float("nan")), torch.full_like(zz[1], float("nan")), torch.full_like(zz[2], float("nan")))
    a = hip.RcbTailArgs()
    for l in range(3):
        a.x[l], a.r[l], a.z[l], a.add[l], a.out[l] = (xs[l].data_ptr(), rr[l].data_ptr(), zz[l].data_ptr(), adds[l].data_ptr(),
                                                      outs[l].data_ptr())
    a.r1, a.u1, a.u2 = R1.data_ptr(), U1.data_ptr(), U2.data_ptr()
    a.w_up, a.b_up, a.w_dn, a.b_dn = wu.data_ptr(), bu.data_ptr(), wd.data_ptr(), bd.data_ptr()
    a.B, a.H, a.W = B, H, W
    hip.check(L.fcvsr_rcb_tail(C.byref(a), 0.2, code, n, st), "rcb_tail")
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16)
    for l in range(3):
        assert torch.equal(bits(outs[l]), bits(ref[l])), f"out{l}"
    assert torch.equal(bits(R1), bits(R1_ref))
    assert torch.equal(bits(U1), bits(U1_ref))
    assert torch.equal(bits(U2), bits(U2_ref))


def test_rcb_tail_rejects_ineligible_shapes():
    from fcvsr_amd import hip
    L = hip.lib()
    a = hip.RcbTailArgs()
    a.B, a.H, a.W = 1, 6, 8            # level 1 would be 3 x 4: odd
    assert L.fcvsr_rcb_tail(C.byref(a), 0.2, hip.BF16, 64, hip.stream_ptr()) != 0
    a.H = 8
    assert L.fcvsr_rcb_tail(C.byref(a), 0.2, hip.BF16, 32, hip.stream_ptr()) != 0


@pytest.mark.parametrize("precision,shape", [("bf16", (2, 7, 1, 36, 68)), ("bf16", (1, 7, 1, 24, 40)), ("f16", (1, 7, 1, 24, 40))])
def test_model_with_fused_tail_equals_generic_tail(precision, shape):
    """The whole S model: the fused BlockRCB tail (fcvsr_rcb_tail) against the generic level-grouped sequence.  Not f16 at
    36 x 68: there the generic sequence already differed from the level-0 one-pass kernel it shares the contract with
    (fcvsr_rcb_level0, by <= 7e-5 of the output) before the fused tail existed; test_rcb_tail_equals_five_launch_sequence
    pins the kernels to that sequence bit for bit."""
    from fcvsr_amd.arch import CVSR_freq as A
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = A.GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S")))
    m = m.cuda()
    m.precision = precision
    m.use_graph = False
    x = torch.from_numpy(np.random.RandomState(sum(shape)).rand(*shape).astype("float32")).cuda()
    outs = []
    with torch.no_grad():
        for fused in (True, False):
            m.fuse_rcb_l0 = fused
            outs.append(m(x).clone())
    assert torch.equal(outs[0], outs[1])
