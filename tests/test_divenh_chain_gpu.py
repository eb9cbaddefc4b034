"""GPU: the DivEnh chain without the round trip of the running sums (fcvsr_divenh_stage: bands j0..i replayed in registers, a
checkpoint of s_f, s_o every four bands) against the chain it replaces (fcvsr_divenh reduce, then fcvsr_divenh_apply_next per
band): the per-stage sums, the final s_o and the checkpointed s_f, s_o must be the same bits."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gate(s, inv_hw):
    """Stand-in for the CALayer gate: any fixed function of the sums serves (both chains get the same bits from the same sums)."""
    return torch.sigmoid(s * inv_hw * 3.0).contiguous()


def _inputs(Q, B, H, W, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    bands = [(torch.randn(B, H, W, Cn, generator=g) * (0.4 / (1 + q))).cuda() for q in range(Q)]
    ab = [((0.5 + torch.rand(Cn, generator=g)).cuda(), (torch.randn(Cn, generator=g) * 0.5).cuda()) for _ in range(Q)]
    return bands, ab


def _reference(bands, ab, B, H, W, Cn):
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    Q = len(bands)
    inv_hw = 1.0 / (H * W)
    nblk = (H * W + 255) // 256
    scratch = torch.empty(2 * B * nblk * Cn, device="cuda")
    s_f, s_o = torch.zeros_like(bands[0]), torch.zeros_like(bands[0])
    mean_sum = bands[0].sum(dim=(1, 2)).contiguous()
    sums = torch.empty(2, B, Cn, device="cuda")
    hip.check(L.fcvsr_divenh(0, 1, bands[0].data_ptr(), s_f.data_ptr(), s_o.data_ptr(), ab[0][0].data_ptr(), ab[0][1].data_ptr(),
                             mean_sum.data_ptr(), inv_hw, None, None, sums.data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W,
                             Cn, st), "fcvsr_divenh")
    all_sums, ckpts = [sums], {}
    for i in range(Q):
        g1 = _gate(sums[0], inv_hw)
        g2 = _gate(sums[1], inv_hw) if i > 0 else None
        sums = torch.empty(2, B, Cn, device="cuda")
        nxt = i + 1 < Q
        hip.check(L.fcvsr_divenh_apply_next(1 if i == 0 else 0, bands[i].data_ptr(), s_f.data_ptr(), s_o.data_ptr(),
                                            ab[i][0].data_ptr(), ab[i][1].data_ptr(), mean_sum.data_ptr(), inv_hw, g1.data_ptr(),
                                            hip.ptr(g2), bands[i + 1].data_ptr() if nxt else None,
                                            ab[i + 1][0].data_ptr() if nxt else None, ab[i + 1][1].data_ptr() if nxt else None,
                                            sums.data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W, Cn, st),
                  "fcvsr_divenh_apply_next")
        all_sums.append(sums)
        ckpts[i] = (s_f.clone(), s_o.clone())
    return mean_sum, all_sums, ckpts


def _staged(bands, ab, mean_sum, sums0, B, H, W, Cn):
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    Q = len(bands)
    inv_hw = 1.0 / (H * W)
    nblk = (H * W + 255) // 256
    scratch = torch.empty(2 * B * nblk * Cn, device="cuda")
    # poisoned: a stage that read s_f / s_o before a checkpoint was stored, or stored one unasked, would show
    s_f = torch.full_like(bands[0], float("nan"))
    s_o = torch.full_like(bands[0], float("nan"))
    sums, all_sums, gates, ckpts, j0 = sums0, [sums0], [], {}, 0
    for i in range(Q):
        gates.append((_gate(sums[0], inv_hw), _gate(sums[1], inv_hw) if i > 0 else None))
        sums = torch.empty(2, B, Cn, device="cuda")
        nxt = i + 1 < Q
        a = hip.DivEnhStageArgs()
        if j0 > 0:
            a.ck_s_f, a.ck_s_o = s_f.data_ptr(), s_o.data_ptr()
        for k, j in enumerate(range(j0, i + 1)):
            a.f[k], a.a[k], a.b[k] = bands[j].data_ptr(), ab[j][0].data_ptr(), ab[j][1].data_ptr()
            a.g1[k], a.g2[k] = gates[j][0].data_ptr(), hip.ptr(gates[j][1])
        a.mean_f_sum = mean_sum.data_ptr()
        if nxt:
            a.f_next, a.a_next, a.b_next = bands[i + 1].data_ptr(), ab[i + 1][0].data_ptr(), ab[i + 1][1].data_ptr()
        ckpt = nxt and i - j0 == 3
        if ckpt:
            a.out_s_f = s_f.data_ptr()
        if ckpt or not nxt:
            a.out_s_o = s_o.data_ptr()
        a.sums, a.scratch, a.scratch_elems = sums.data_ptr(), scratch.data_ptr(), scratch.numel()
        a.inv_hw, a.n_bands, a.B, a.H, a.W, a.C = inv_hw, i - j0 + 1, B, H, W, Cn
        hip.check(L.fcvsr_divenh_stage(C.byref(a), st), "fcvsr_divenh_stage")
        all_sums.append(sums)
        if ckpt:
            ckpts[i] = (s_f.clone(), s_o.clone())
            j0 = i + 1
    return all_sums, ckpts, s_f, s_o


@pytest.mark.parametrize("hw", [(20, 24), (37, 29), (180, 320)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", [4, 8])
def test_stage_chain_equals_apply_next_chain(Q, B, hw):
    H, W = hw
    Cn = 64
    bands, ab = _inputs(Q, B, H, W, Cn, seed=Q * 100 + B * 10 + H)
    mean_sum, ref_sums, ref_ck = _reference(bands, ab, B, H, W, Cn)
    got_sums, got_ck, s_f, s_o = _staged(bands, ab, mean_sum, ref_sums[0], B, H, W, Cn)
    assert len(got_sums) == len(ref_sums) == Q + 1
    for i, (g, r) in enumerate(zip(got_sums, ref_sums)):
        assert torch.isfinite(r).all()
        assert torch.equal(g, r), f"sums after stage {i - 1}: max |d| = {float((g - r).abs().max())}"
    assert torch.equal(s_o, ref_ck[Q - 1][1]), "final s_o"
    if Q == 8:
        assert sorted(got_ck) == [3]
        assert torch.equal(got_ck[3][0], ref_ck[3][0]), "checkpointed s_f"
        assert torch.equal(got_ck[3][1], ref_ck[3][1]), "checkpointed s_o"
    else:
        assert not got_ck and torch.isnan(s_f).all()          # Q <= 4: s_f is never written


def test_narrow_channel_count_and_bad_arguments():
    """C = 32 (eight pixel sub-lanes per channel quad instead of sixteen) and the argument checks of the entry point."""
    from fcvsr_amd import hip
    Q, B, H, W, Cn = 4, 2, 19, 23, 32
    bands, ab = _inputs(Q, B, H, W, Cn, seed=5)
    mean_sum, ref_sums, ref_ck = _reference(bands, ab, B, H, W, Cn)
    got_sums, _, _, s_o = _staged(bands, ab, mean_sum, ref_sums[0], B, H, W, Cn)
    for g, r in zip(got_sums, ref_sums):
        assert torch.equal(g, r)
    assert torch.equal(s_o, ref_ck[Q - 1][1])
    a = hip.DivEnhStageArgs()
    assert hip.lib().fcvsr_divenh_stage(C.byref(a), hip.stream_ptr()) == -1          # nothing set
    a.sums = a.scratch = got_sums[0].data_ptr()
    a.n_bands, a.B, a.H, a.W, a.C = 5, 1, 4, 4, 64
    assert hip.lib().fcvsr_divenh_stage(C.byref(a), hip.stream_ptr()) == -1          # more than four replayed bands
    a.n_bands, a.C = 1, 30
    assert hip.lib().fcvsr_divenh_stage(C.byref(a), hip.stream_ptr()) == -1          # C % 4 != 0
