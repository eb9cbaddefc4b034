"""GPU: fcvsr_convblk_heads (all ConvBlk heads of an MGAA call in two launches) against one fcvsr_convblk call per head.
Every output element keeps its operation order, so the comparison is bit for bit: ospec, every u_i and every partial_i."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPES = (0.25, 0.0, -0.1)
SENTINEL = -777.0


def _rand(*s, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(s).astype(np.float32))


def _heads(A, rot):
    from fcvsr_amd import hip
    hs = []
    for i in range(A):
        k = 2 * i + 1
        hs.append(dict(k=k,
                       w1=hip.pack_conv_weight(_rand(4, 4, k, k, seed=300 + i).cuda() / (2.0 * k)),
                       w2=hip.pack_conv_weight(_rand(4, 4, k, k, seed=320 + i).cuda() / (2.0 * k)),
                       slope=torch.tensor([SLOPES[(i + rot) % 3]], device="cuda"),
                       cw1=_rand(4, 4, seed=340 + i).cuda(), cw2=_rand(4, 4, seed=360 + i).cuda()))
    return hs


def _check(B, H, Wf, A, rot=0):
    from fcvsr_amd import hip
    L = hip.lib()
    st = hip.stream_ptr()
    x = _rand(2 * B, H, Wf, 4, seed=1000 + H * Wf + B).cuda()
    sim = _rand(B, H, Wf, 4, seed=2000 + H * Wf + B).cuda()
    hs = _heads(A, rot)
    ntile = ((H + 15) // 16) * ((Wf + 15) // 16)
    # reference: one fcvsr_convblk call per head into the same records
    ref = torch.zeros(B, H, Wf, 8 * A, device="cuda")
    u_ref = torch.zeros(A, 2 * B, H, Wf, 4, device="cuda")
    p_ref = torch.zeros(A, 2 * B * ntile * 4, device="cuda")
    for i, h in enumerate(hs):
        hip.check(L.fcvsr_convblk(x.data_ptr(), h["w1"].data_ptr(), h["w2"].data_ptr(), h["slope"].data_ptr(), h["k"],
                                  h["cw1"].data_ptr(), h["cw2"].data_ptr(), sim.data_ptr(), B, 2, H, Wf, u_ref[i].data_ptr(),
                                  p_ref[i].data_ptr(), p_ref[i].numel(), ref.data_ptr(), 8 * A, 0, 4 * A, A, i, st), "convblk")
    out = torch.full((B, H, Wf, 8 * A), SENTINEL, device="cuda")
    u = torch.full((A, 2 * B, H, Wf, 4), SENTINEL, device="cuda")
    part = torch.full((A, 2 * B * ntile * 4), SENTINEL, device="cuda")
    PA = C.c_void_p * A
    hip.check(L.fcvsr_convblk_heads(x.data_ptr(), A, PA(*[h["w1"].data_ptr() for h in hs]), PA(*[h["w2"].data_ptr() for h in hs]),
                                    PA(*[h["slope"].data_ptr() for h in hs]), PA(*[h["cw1"].data_ptr() for h in hs]),
                                    PA(*[h["cw2"].data_ptr() for h in hs]), sim.data_ptr(), B, H, Wf, u.data_ptr(),
                                    part.data_ptr(), part.numel(), out.data_ptr(), 8 * A, 0, 4 * A, st), "convblk_heads")
    torch.cuda.synchronize()
    assert not bool((ref == SENTINEL).any())
    for i in range(A):
        assert torch.equal(u[i], u_ref[i]), f"u of head {i}"
        assert torch.equal(part[i], p_ref[i]), f"partial sums of head {i}"
    assert torch.equal(out, ref)


# 5x3: one partial tile smaller than the 5x5 halo; 16x16: exactly one tile; 21x19, 33x17: partial tiles both ways
@pytest.mark.parametrize("A", [3, 6])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,Wf", [(5, 3), (16, 16), (21, 19), (33, 17)])
def test_convblk_heads_bit_equal_to_per_head_calls(H, Wf, B, A):
    _check(B, H, Wf, A)


@pytest.mark.parametrize("A", [3, 6])
def test_convblk_heads_bit_equal_at_flagship_spectrum_size(A):
    _check(2, 180, 161, A)


@pytest.mark.parametrize("rot", [1, 2])
def test_convblk_heads_every_slope_on_every_head(rot):
    """rot = 0 (the cases above) gives head i the slope SLOPES[i % 3]; the two rotations give each head the other two."""
    _check(1, 21, 19, 3, rot)
