"""GPU: fcvsr_freq_mlp3 with its workgroups numbered so that the two directions of a 128-pixel tile are 8 block indices apart
(groups of 8 tiles, surplus blocks of the last group return at once): every pixel of both directions is still computed once
and agrees bit for bit with the three stand-alone 1x1 launches, at tile counts below, at and above a multiple of 8."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64


def _rand(*s, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(s).astype(np.float32))


@pytest.fixture(scope="module")
def weights():
    from fcvsr_amd import hip
    ws = (_rand(128, 256, 1, 1, seed=112) / 16, _rand(128, 128, 1, 1, seed=113) / 11, _rand(128, 128, 1, 1, seed=114) / 11)
    return tuple(hip.pack_conv_weight_mfma(w.cuda(), torch.bfloat16) for w in ws)


# pixels -> 128-pixel tiles: 1407 -> 11 (one group of 8 and a tail of 3), 1024 -> 8 (exactly one group),
# 2176 -> 17 (two groups and a tail of one), 130 -> 2 (a tail only, last tile partial)
@pytest.mark.parametrize("n_dirs", [2, 1])
@pytest.mark.parametrize("B,H,Wf", [(1, 21, 67), (2, 16, 32), (2, 17, 64), (1, 10, 13)])
def test_freq_mlp3_tile_numbering_covers_every_pixel_once(weights, B, H, Wf, n_dirs):
    from fcvsr_amd import hip
    L = hip.lib()
    p0, p2, p4 = weights
    spec = _rand(B, H, Wf, 6 * N, seed=120 + H * Wf).cuda()
    x1f, x2f, x3f = spec[..., :2 * N], spec[..., 2 * N:4 * N], spec[..., 4 * N:]
    dt = torch.bfloat16
    dirs = list(enumerate((x1f, x3f)))[:n_dirs]
    ref = torch.empty(n_dirs * B, H, Wf, 2 * N, device="cuda", dtype=dt)
    t0, t1 = torch.empty_like(ref), torch.empty_like(ref)
    hip.conv2d_mfma([dict(srcs=[xa, x2f], dst=t0[d * B:(d + 1) * B]) for d, xa in dirs], p0, 1, 128, hip.BF16, act=hip.ACT_RELU)
    hip.conv2d_mfma([dict(srcs=[t0], dst=t1)], p2, 1, 128, hip.BF16, act=hip.ACT_RELU)
    hip.conv2d_mfma([dict(srcs=[t1[d * B:(d + 1) * B]], dst=ref[d * B:(d + 1) * B], res=[xa, x2f]) for d, xa in dirs], p4, 1, 128,
                    hip.BF16, res_scale=[1.0, -1.0])
    out = torch.full_like(ref, float("nan"))                 # a pixel no workgroup writes stays NaN
    P2 = C.c_void_p * 2
    last = out[(n_dirs - 1) * B:]
    hip.check(L.fcvsr_freq_mlp3(P2(x1f.data_ptr(), x3f.data_ptr()), P2(x2f.data_ptr(), x2f.data_ptr()), n_dirs, 6 * N, B * H * Wf,
                                p0.data_ptr(), p2.data_ptr(), p4.data_ptr(), P2(out[:B].data_ptr(), last.data_ptr()), 2 * N,
                                hip.stream_ptr()), "freq_mlp3")
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
