"""GPU: hip.conv_plan names the kernel that fcvsr_conv2d_mfma really launches, one small problem per non-generic path.
What those kernels compute is pinned per element by tests/test_infer_conv_gpu.py (rounded-operand f64 reference, every kernel string)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (expected kernel, ksize, stride, cin, cout, H, W, pixel shuffle, FCVSR_MFMA_RES or None)
CASES = [
    ("conv3_lean_kernel", 3, 1, 64, 64, 9, 40, False, None),
    ("conv3s2_lean_kernel", 3, 2, 64, 64, 21, 70, False, None),
    ("conv1ps_res_kernel", 1, 1, 64, 128, 9, 11, True, None),
    ("conv3_res_kernel", 3, 1, 128, 64, 17, 45, False, "1"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_equals_launched_kernel(case, monkeypatch):
    from fcvsr_amd import hip
    kernel, k, stride, cin, cout, H, W, ps, res_env = case
    g0 = torch.Generator().manual_seed(cin + cout + H)
    dt = torch.bfloat16
    wp = hip.pack_conv_weight_mfma((torch.randn(cout, cin, k, k, generator=g0) / (k * cin ** 0.5)).cuda(), dt, ps=ps)
    bias = torch.randn(cout, generator=g0).cuda()
    x = torch.randn(1, H, W, cin, generator=g0).cuda().to(dt)
    oshape = (1, 2 * H, 2 * W, cout // 4) if ps else (1, (H + stride - 1) // stride, (W + stride - 1) // stride, cout)
    y = torch.full(oshape, float("nan"), device="cuda", dtype=dt)
    kw = dict(stride=stride, bias=bias, act=hip.ACT_RELU, pixel_shuffle=ps)
    if res_env is not None:
        monkeypatch.setenv("FCVSR_MFMA_RES", res_env)
    hip.conv2d_mfma([dict(srcs=[x], dst=y)], wp, k, cout, hip.BF16, **kw)
    torch.cuda.synchronize()
    launched = hip.lib().fcvsr_last_conv_kernel().decode()
    planned = hip.conv_plan([dict(srcs=[x], dst=y)], wp, k, cout, hip.BF16, lean=1, res=2 if res_env is None else int(res_env), **kw)
    assert launched.startswith(kernel + "<"), launched
    assert planned == launched
    assert not torch.isnan(y.float()).any()
