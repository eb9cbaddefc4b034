"""Cases shared by the `active=` tests (tests/test_active_cpu.py, test_active_kernels_gpu.py, test_active_gpu.py): frames with
planted bars, and the brute-force form of the window rule."""
import numpy as np

from fcvsr_amd.harness import active as A


def barred(bits, n, C, H, W, box, seed=0, noise=5, picture=(0.3, 0.9)):
    """(n,C,H,W) frames of `bits` bits: noise in [0, noise] 8-bit steps everywhere (below the default limit of 24), picture at
    `picture` of the peak inside box = (top, bottom, left, right), or inside box(i) of frame i."""
    rs = np.random.RandomState(seed)
    peak, step = (255, 1) if bits == 8 else (1023, 4)
    f = rs.randint(0, noise * step + 1, (n, C, H, W))
    for i in range(n):
        t, b, l, r = box(i) if callable(box) else box
        f[i, :, t:b, l:r] = rs.randint(int(picture[0] * peak), int(picture[1] * peak), (C, b - t, r - l))
    return f.astype(np.uint8 if bits == 8 else np.uint16)


def brute_box(frames, bits, last, spec):
    """The used box of a window whose last frame is `last`: the union of `frame_box` over frames 0 .. last, by the definition."""
    n, C, H, W = frames.shape
    rows, cols = A.line_sums_host(frames[:last + 1])
    boxes = [A.frame_box(rows[i], cols[i], C, H, W, bits, spec) for i in range(last + 1)]
    boxes = [b for b in boxes if b is not None]
    union = None if not boxes else (min(b[0] for b in boxes), max(b[1] for b in boxes), min(b[2] for b in boxes),
                                    max(b[3] for b in boxes))
    return A.used_box(union, H, W, spec)
