"""GPU: fcvsr_convcorr_strip (convcorr on the CorrBlock strip x < xs, written into off4 in place) against the sequence it
replaces - f32 strip copy, convcorr.0 per direction on [strip | lookup], convcorr.2, convcorr.4, paste - bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64                                                     # n_feats: spectra are 2N channels per pixel


def _rand(*s, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(s).astype(np.float32))


@pytest.fixture(scope="module")
def weights():
    from fcvsr_amd import hip
    w0 = torch.zeros(64, 2 * N + 84, 1, 1)
    w0[:, :2 * N + 81] = _rand(64, 2 * N + 81, 1, 1, seed=401) / 14      # the 3 pad channels of the lookup carry zero weights
    w2 = _rand(64, 64, 1, 1, seed=402) / 8
    w4 = _rand(4, 64, 1, 1, seed=403) / 8
    return tuple(hip.pack_conv_weight_mfma(w.cuda(), torch.bfloat16) for w in (w0, w2, w4))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [5, 21])
@pytest.mark.parametrize("Wf", [5, 8, 19, 161])
def test_convcorr_strip_bit_equal_to_separate_launches(weights, Wf, H, B):
    from fcvsr_amd import hip
    L = hip.lib()
    st = hip.stream_ptr()
    p0, p2, p4 = weights
    xs = min(Wf, 8)
    seed = 500 + 7 * Wf + 3 * H + B
    x1f = _rand(B, H, Wf, 2 * N, seed=seed).cuda()
    x2f = _rand(B, H, Wf, 2 * N, seed=seed + 1).cuda()
    off = _rand(2 * B, H, Wf, 2 * N, seed=seed + 2).cuda().to(torch.bfloat16)
    fill = _rand(2 * B, H, Wf, 4, seed=seed + 3).cuda()     # what the full-grid convcorr launch left in off4
    corr = torch.empty(B, H, xs, 84, device="cuda")
    cv = hip.view(corr)
    hip.check(L.fcvsr_corr_lookup(x1f.data_ptr(), x2f.data_ptr(), 2 * N, B, H, Wf, 2 * N, 4, xs, C.byref(cv), st), "corr_lookup")
    assert float(corr.abs().max()) > 0.0
    # the replaced sequence
    ref = fill.clone()
    off_s = off[:, :, :xs].to(torch.float32, memory_format=torch.contiguous_format)
    c0_s = torch.empty(2 * B, H, xs, N, device="cuda", dtype=torch.bfloat16)
    c1_s = torch.empty_like(c0_s)
    off4_s = torch.empty(2 * B, H, xs, 4, device="cuda")
    for d in range(2):
        hip.conv2d_mfma([dict(srcs=[off_s[d * B:(d + 1) * B], corr], dst=c0_s[d * B:(d + 1) * B])], p0, 1, N, hip.BF16,
                        act=hip.ACT_RELU)
    hip.conv2d_mfma([dict(srcs=[c0_s], dst=c1_s)], p2, 1, N, hip.BF16, act=hip.ACT_RELU)
    hip.conv2d_mfma([dict(srcs=[c1_s], dst=off4_s)], p4, 1, 4, hip.BF16)
    ref[:, :, :xs].copy_(off4_s)
    # one launch, in place
    out = fill.clone()
    hip.check(L.fcvsr_convcorr_strip(off.data_ptr(), corr.data_ptr(), B, H, Wf, xs, p0.data_ptr(), p2.data_ptr(), p4.data_ptr(),
                                     out.data_ptr(), st), "convcorr_strip")
    torch.cuda.synchronize()
    assert torch.equal(out[:, :, xs:], fill[:, :, xs:]), "columns >= xs must be left untouched"
    assert not torch.equal(ref[:, :, :xs], fill[:, :, :xs])
    assert torch.equal(out[:, :, :xs], ref[:, :, :xs])
