"""IAC warp backward micro-benchmark: the scatter form (fcvsr_iac_bwd_warp + its zero fill) against the atomic-free form
(fcvsr_iac_bwd_warp_det: source pass, sort, gather), alternating, with the algorithmic bytes of each:
python scripts/one_iac_bwd_warp.py [--shape N] [--once]    (--once: warm-up plus one call of each form, for a rocprofv3 --kernel-trace run)"""
import os, sys, ctypes as C
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
from fcvsr_amd import hip
L = hip.lib()
once = "--once" in sys.argv
def setup(B, H, W, Cn, sigma):
    g = torch.Generator().manual_seed(B * 7 + H + Cn)
    gv = torch.randn(B, H, W, Cn, generator=g).cuda()
    prev = torch.randn(B, H, W, Cn, generator=g).cuda()
    K = (0.4 * torch.randn(B, H, W, 6 * Cn, generator=g)).cuda()
    off = (sigma * torch.randn(B, 2, H, W, generator=g)).cuda().permute(0, 2, 3, 1)
    kv, ov = hip.view(K[..., :3 * Cn]), hip.view(off)
    goff = torch.empty(B, H, W, 2, device="cuda")
    gprev = torch.empty(B, H, W, Cn, device="cuda")
    n = C.c_size_t(0)
    hip.check(L.fcvsr_iac_bwd_warp_det_workspace(B, H, W, Cn, C.byref(n)), "workspace")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    keep = (gv, prev, K, off)
    def scatter():
        gprev.zero_()
        hip.check(L.fcvsr_iac_bwd_warp(gv.data_ptr(), C.byref(kv), prev.data_ptr(), C.byref(ov), B, H, W, Cn, gprev.data_ptr(), goff.data_ptr(),
                                       hip.stream_ptr()), "scatter")
    def det():
        hip.check(L.fcvsr_iac_bwd_warp_det(gv.data_ptr(), C.byref(kv), prev.data_ptr(), C.byref(ov), B, H, W, Cn, gprev.data_ptr(), goff.data_ptr(),
                                           ws.data_ptr(), ws.numel(), hip.stream_ptr()), "det")
    return scatter, det, n.value, keep
def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters
# the bench's training shape (4 clips: the outer alignment call runs on 2 x 4 samples of 128 x 128) and one inference-sized image batch
SHAPES = ((8, 128, 128, 64, 0.7), (8, 128, 128, 64, 4.0), (4, 180, 320, 64, 0.7))
if "--shape" in sys.argv:
    SHAPES = (SHAPES[int(sys.argv[sys.argv.index("--shape") + 1])],)
for (B, H, W, Cn, sigma) in SHAPES:
    scatter, det, wsb, keep = setup(B, H, W, Cn, sigma)
    for _ in range(4): scatter(); det()
    torch.cuda.synchronize()
    if once:
        scatter(); det(); torch.cuda.synchronize()
        continue
    ts, td = [], []
    for _ in range(5):                                   # alternate the two forms
        ts.append(timed(scatter, 50)); td.append(timed(det, 50))
    npix = B * H * W
    b_sc = npix * (4 * Cn * 4 + Cn * 4)                  # added by atomics + zero fill (inputs: gv 3x, prev 4x, k1 apart)
    b_det = npix * (Cn * 4 + 4 * Cn * 4 + Cn * 4 + 8)    # g_s written once, read ~4x, g_prev stored once, 8 B through the sort
    print("B=%d %dx%d C=%d off sigma %.1f: scatter+fill %.1f us (min %.1f max %.1f; %.0f GB/s of %d MB atomic+fill) | det %.1f us (min %.1f max %.1f; "
          "%.0f GB/s of %d MB g_s/g_prev/sort) | workspace %.1f MB" % (B, H, W, Cn, sigma, sorted(ts)[2], min(ts), max(ts), b_sc / sorted(ts)[2] * 1e-3,
          b_sc >> 20, sorted(td)[2], min(td), max(td), b_det / sorted(td)[2] * 1e-3, b_det >> 20, wsb / 2 ** 20))
