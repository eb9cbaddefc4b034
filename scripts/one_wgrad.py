"""Matrix-core weight gradient micro-benchmark (fcvsr_conv2d_wgrad_mfma, reduction included, no bias): python scripts/one_wgrad.py"""
import os, sys, ctypes as C
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from fcvsr_amd import hip
L = hip.lib()
def run(B, H, W, cin, cout, k, iters):
    g = torch.Generator().manual_seed(B * 7 + H + cin + k)
    x = torch.randn(B, H, W, cin, generator=g).cuda()
    gy = torch.randn(B, H, W, cout, generator=g).cuda()
    n = L.fcvsr_conv2d_wgrad_mfma_scratch_elems(B, H, W, cin, cout, k, k)
    scratch = torch.empty(n, device="cuda")
    dw = torch.zeros(cout, cin, k, k, device="cuda")
    xv, gv = hip.view(x), hip.view(gy)
    def f():
        hip.check(L.fcvsr_conv2d_wgrad_mfma(C.byref(xv), C.byref(gv), B, H, W, k, k, 1, k // 2, dw.data_ptr(), None, scratch.data_ptr(), n, 0, 0,
                                            hip.stream_ptr()), "wgrad")
    for _ in range(4): f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters
for cfg in ((4, 128, 128, 64, 64, 3), (4, 64, 64, 64, 64, 3), (4, 32, 32, 64, 64, 3), (4, 128, 128, 64, 128, 3), (4, 128, 128, 128, 64, 3), (4, 128, 128, 64, 64, 1), (8, 128, 128, 64, 64, 3)):
    us = run(*cfg, iters=20)
    fl = 2.0 * cfg[0] * cfg[1] * cfg[2] * cfg[3] * cfg[4] * cfg[5] * cfg[5]
    print("B=%d %dx%d %d->%d k%d: %.1f us (%.0f TFLOP/s) incl. reduction" % (*cfg, us, fl / us * 1e-6))
