"""tOF, the temporal-consistency metric of the reference's test configs (``metrics=['PSNR', 'SSIM', 'tOF']``;
CVSR_train/metric/psnr_ssim.py calculate_tOF): the mean end-point distance between the dense Farneback flow of the ground truth
pair (previous -> current frame) and that of the delivered pair.

This module is the contract (host, numpy only) and the device entry `frame_tof`.  `farneback_host` restates
``cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0)``, the only call the reference makes, as the algorithm of
the OpenCV 4.x implementation is remembered: cv2 is not a dependency of this project, was never installed next to it and was
NEVER RUN against this restatement.  Agreement with cv2 is by reading only.  The kernels of csrc/flow.hip are pinned to this
module, not to cv2; the known answers of the tests (integer shifts of a smooth texture, the polynomial expansion of an exact
quadratic) need no cv2.

One deliberate restatement: OpenCV's blur step updates the matrices in row stripes that lag the flow by a few rows; here every
iteration but the last recomputes the matrices from the new flow at every pixel (a Jacobi step), which is what the stripes amount to.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, FLAGS = 0.5, 3, 15, 3, 5, 1.2, 0
MIN_SIZE = 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
Y_COEF = (65.481, 128.553, 24.966)                     # R, G, B of metrics.to_y_channel


def check_params(pyr_scale=PYR_SCALE, levels=LEVELS, winsize=WINSIZE, iterations=ITERATIONS, poly_n=POLY_N, poly_sigma=POLY_SIGMA,
                 flags=FLAGS) -> None:
    """The device path is built for the reference's one call: any other parameter value is a ValueError."""
    got = (pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    if got != (PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, FLAGS):
        raise ValueError(f"the device Farneback flow is built for (0.5, 3, 15, 3, 5, 1.2, 0) only, got {got}")


def level_count(h: int, w: int, levels: int = LEVELS, pyr_scale: float = PYR_SCALE) -> int:
    """Scales of an h x w frame: halvings stop before a side falls under 32."""
    k, s = 0, 1.0
    while k < levels:
        s *= pyr_scale
        if w * s < MIN_SIZE or h * s < MIN_SIZE:
            break
        k += 1
    return k + 1


def level_geometry(h: int, w: int, k: int, pyr_scale: float = PYR_SCALE):
    """(sigma, taps of the blur, (hl, wl)) of level k; Python's round() is round-half-even."""
    s = pyr_scale ** k
    sigma = (1.0 / s - 1.0) * 0.5
    ks = max(int(round(sigma * 5)) | 1, 3)
    return sigma, ks, (int(round(h * s)), int(round(w * s)))


def gaussian_taps(ks: int, sigma: float) -> np.ndarray:
    """f64 taps of the level blur: [0.25, 0.5, 0.25] at sigma 0, else exp(-x^2 / 2 sigma^2) normalised."""
    if sigma <= 0:
        if ks != 3:
            raise ValueError("sigma 0 has the 3-tap kernel only")
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ks, dtype=np.float64) - (ks - 1) // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def poly_constants(n: int = POLY_N, sigma: float = POLY_SIGMA):
    """(g, xg, xxg, ig11, ig03, ig33, ig55) in f64."""
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g = g / g.sum()
    G = np.zeros((6, 6))
    for iy, y in enumerate(x):
        for ix, xx in enumerate(x):
            b = np.array([1.0, xx, y, xx * xx, y * y, xx * y])
            G += g[iy] * g[ix] * np.outer(b, b)
    ig = np.linalg.inv(G)
    return g, x * g, x * x * g, ig[1, 1], ig[0, 3], ig[3, 3], ig[5, 5]


def read_plane(a, dtype=np.float64) -> np.ndarray:
    """A plane as float: uint8 as it is, uint16 as min(k, 1023), floats cast."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"expected an (h,w) plane, got {a.shape}")
    if a.dtype == np.uint16:
        a = np.minimum(a, 1023)
    elif a.dtype != np.uint8 and a.dtype.kind != "f":
        raise ValueError(f"planes are uint8, uint16 or float, got {a.dtype}")
    return a.astype(dtype)


def rgb_to_y(rgb, dtype=np.float64) -> np.ndarray:
    """(3,h,w) uint8 RGB -> the float Y of `metrics.to_y_channel`, evaluated in `dtype` as
    ``((65.481 R + 128.553 G) + 24.966 B) / 255 + 16``."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[0] != 3 or rgb.dtype != np.uint8:
        raise ValueError(f"expected (3,h,w) uint8, got {rgb.dtype} {rgb.shape}")
    r, g, b = (rgb[c].astype(dtype) for c in range(3))
    c = [dtype(v) for v in Y_COEF]
    return ((c[0] * r + c[1] * g) + c[2] * b) / dtype(255.0) + dtype(16.0)


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def blur_host(img: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """Separable Gaussian, rows first, taps added in ascending order, REFLECT_101 borders; in img.dtype."""
    dt = img.dtype.type
    h, w = img.shape
    r = (len(taps) - 1) // 2
    t = [dt(v) for v in taps]
    xi = np.arange(w)
    row = np.zeros_like(img)
    for k in range(-r, r + 1):
        row = row + t[k + r] * img[:, _reflect101(xi + k, w)]
    yi = np.arange(h)
    out = np.zeros_like(img)
    for k in range(-r, r + 1):
        out = out + t[k + r] * row[_reflect101(yi + k, h), :]
    return out


def _resize_axis(n_src: int, n_dst: int, dt):
    """Source indices and the fraction of bilinear resizing along one axis, in dt arithmetic."""
    scale = dt(n_src) / dt(n_dst)
    f = (np.arange(n_dst).astype(dt) + dt(0.5)) * scale - dt(0.5)
    i0 = np.floor(f)
    fr = (f - i0).astype(dt)
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), fr


def resize_host(img: np.ndarray, shape) -> np.ndarray:
    """Bilinear, source coordinate (i + 0.5) src/dst - 0.5, indices clamped; any trailing channel axes; in img.dtype."""
    dt = img.dtype.type
    y0, y1, fy = _resize_axis(img.shape[0], shape[0], dt)
    x0, x1, fx = _resize_axis(img.shape[1], shape[1], dt)
    tail = (1,) * (img.ndim - 2)
    fx = fx.reshape((1, -1) + tail)
    fy = fy.reshape((-1, 1) + tail)
    one = dt(1.0)
    top = img[y0][:, x0] * (one - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (one - fx) + img[y1][:, x1] * fx
    return top * (one - fy) + bot * fy


def level_image_host(plane, h: int, w: int, k: int, dtype=np.float64) -> np.ndarray:
    """The level-k image of a float plane: blur at full size, then resize."""
    sigma, ks, shape = level_geometry(h, w, k)
    return resize_host(blur_host(np.asarray(plane, dtype=dtype), gaussian_taps(ks, sigma)), shape)


def poly_exp_host(img: np.ndarray) -> np.ndarray:
    """(h,w) -> (h,w,5), channels (y, x, yy, xx, xy); the vertical pass first, taps ascending, replicate borders; in img.dtype."""
    dt = img.dtype.type
    n = POLY_N
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_constants()
    g, xg, xxg = ([dt(v) for v in a] for a in (g, xg, xxg))
    ig11, ig03, ig33, ig55 = dt(ig11), dt(ig03), dt(ig33), dt(ig55)
    h, w = img.shape
    yi, xi = np.arange(h), np.arange(w)
    v0, v1, v2 = np.zeros_like(img), np.zeros_like(img), np.zeros_like(img)
    for k in range(-n, n + 1):
        s = img[np.clip(yi + k, 0, h - 1), :]
        v0, v1, v2 = v0 + g[k + n] * s, v1 + xg[k + n] * s, v2 + xxg[k + n] * s
    b1, bx, bxx, by, bxy, byy = (np.zeros_like(img) for _ in range(6))
    for k in range(-n, n + 1):
        c = np.clip(xi + k, 0, w - 1)
        a0, a1, a2 = v0[:, c], v1[:, c], v2[:, c]
        b1, bx, bxx = b1 + g[k + n] * a0, bx + xg[k + n] * a0, bxx + xxg[k + n] * a0
        by, bxy = by + g[k + n] * a1, bxy + xg[k + n] * a1
        byy = byy + g[k + n] * a2
    return np.stack([by * ig11, bx * ig11, b1 * ig03 + byy * ig33, b1 * ig03 + bxx * ig33, bxy * ig55], -1)


def poly_exp_condition(img) -> np.ndarray:
    """(h,w,5) f64: per output element the sum of the absolute tap products behind it (the error scale of an f32 evaluation)."""
    img = np.abs(np.asarray(img, dtype=np.float64))
    n = POLY_N
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_constants()
    h, w = img.shape
    yi, xi = np.arange(h), np.arange(w)
    v = [np.zeros_like(img) for _ in range(3)]
    for k in range(-n, n + 1):
        s = img[np.clip(yi + k, 0, h - 1), :]
        for j, t in enumerate((g, xg, xxg)):
            v[j] = v[j] + abs(t[k + n]) * s
    b1, bx, bxx, by, bxy, byy = (np.zeros_like(img) for _ in range(6))
    for k in range(-n, n + 1):
        c = np.clip(xi + k, 0, w - 1)
        b1, bx, bxx = b1 + abs(g[k + n]) * v[0][:, c], bx + abs(xg[k + n]) * v[0][:, c], bxx + abs(xxg[k + n]) * v[0][:, c]
        by, bxy = by + abs(g[k + n]) * v[1][:, c], bxy + abs(xg[k + n]) * v[1][:, c]
        byy = byy + abs(g[k + n]) * v[2][:, c]
    return np.stack([by * ig11, bx * ig11, b1 * abs(ig03) + byy * ig33, b1 * abs(ig03) + bxx * ig33, bxy * ig55], -1)


def border_scale(h: int, w: int, dt) -> np.ndarray:
    """(h,w): the product of the border table over the near edges, 1 in the interior."""
    tab = np.array([dt(v) for v in BORDER] + [dt(1.0)], dtype=dt)
    yi, xi = np.arange(h), np.arange(w)
    sx = tab[np.minimum(xi, 5)] * tab[np.minimum(w - 1 - xi, 5)]
    sy = tab[np.minimum(yi, 5)] * tab[np.minimum(h - 1 - yi, 5)]
    return (sx[None, :] * sy[:, None]).astype(dt)


def matrices_host(R0: np.ndarray, R1: np.ndarray, flow: np.ndarray, return_mask: bool = False):
    """(h,w,5) expansions of both frames and the (h,w,2) flow [dx, dy] -> M (h,w,5); in R0.dtype."""
    dt = R0.dtype.type
    h, w = R0.shape[:2]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dx, dy = flow[..., 0].astype(dt), flow[..., 1].astype(dt)
    fx, fy = xx.astype(dt) + dx, yy.astype(dt) + dy
    x1f, y1f = np.floor(fx), np.floor(fy)
    inside = (x1f >= 0) & (x1f < w - 1) & (y1f >= 0) & (y1f < h - 1)
    x1 = np.where(inside, x1f, 0).astype(np.int64)
    y1 = np.where(inside, y1f, 0).astype(np.int64)
    fx, fy = (fx - x1f).astype(dt), (fy - y1f).astype(dt)
    one = dt(1.0)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    s = (a00[..., None] * R1[y1, x1] + a01[..., None] * R1[y1, x2] + a10[..., None] * R1[y2, x1] + a11[..., None] * R1[y2, x2])
    half, quarter, zero = dt(0.5), dt(0.25), dt(0.0)
    r2 = np.where(inside, s[..., 0], zero)
    r3 = np.where(inside, s[..., 1], zero)
    r4 = np.where(inside, (R0[..., 2] + s[..., 2]) * half, R0[..., 2])
    r5 = np.where(inside, (R0[..., 3] + s[..., 3]) * half, R0[..., 3])
    r6 = np.where(inside, (R0[..., 4] + s[..., 4]) * quarter, R0[..., 4] * half)
    r2 = (R0[..., 0] - r2) * half
    r3 = (R0[..., 1] - r3) * half
    r2 = r2 + r4 * dy + r6 * dx
    r3 = r3 + r6 * dy + r5 * dx
    sc = border_scale(h, w, dt)
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    M = np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], -1).astype(dt)
    return (M, inside) if return_mask else M


def box_solve_host(M: np.ndarray) -> np.ndarray:
    """(h,w,5) -> the (h,w,2) flow: the 15x15 box average (rows added first, ascending; replicate borders) and the 2x2 solve."""
    dt = M.dtype.type
    h, w = M.shape[:2]
    r = WINSIZE // 2
    yi, xi = np.arange(h), np.arange(w)
    v = np.zeros_like(M)
    for k in range(-r, r + 1):
        v = v + M[np.clip(yi + k, 0, h - 1)]
    s = np.zeros_like(M)
    for k in range(-r, r + 1):
        s = s + v[:, np.clip(xi + k, 0, w - 1)]
    s = s * dt(1.0 / (WINSIZE * WINSIZE))
    g11, g12, g22, h1, h2 = (s[..., c] for c in range(5))
    idet = dt(1.0) / (g11 * g22 - g12 * g12 + dt(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1).astype(dt)


def farneback_host(prev, next, dtype=np.float64, pyr_scale=PYR_SCALE, levels=LEVELS, winsize=WINSIZE, iterations=ITERATIONS,
                   poly_n=POLY_N, poly_sigma=POLY_SIGMA, flags=FLAGS) -> np.ndarray:
    """(h,w) planes (uint8, uint16 read as min(k, 1023), or float) -> the (h,w,2) flow [dx, dy] from `prev` to `next`, every
    operation evaluated in `dtype`.  Only the reference's parameter values are implemented."""
    check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    dtype = np.dtype(dtype).type
    a, b = read_plane(prev, dtype), read_plane(next, dtype)
    if a.shape != b.shape:
        raise ValueError(f"the frames differ in shape: {a.shape}, {b.shape}")
    h, w = a.shape
    flow = None
    for k in range(level_count(h, w) - 1, -1, -1):
        shape = level_geometry(h, w, k)[2]
        R0, R1 = (poly_exp_host(level_image_host(p, h, w, k, dtype)) for p in (a, b))
        flow = np.zeros(shape + (2,), dtype=dtype) if flow is None else resize_host(flow, shape) * dtype(1.0 / pyr_scale)
        M = matrices_host(R0, R1, flow)
        for i in range(iterations):
            flow = box_solve_host(M)
            if i + 1 < iterations:
                M = matrices_host(R0, R1, flow)
    return flow


def epe_host(flow_a, flow_b) -> float:
    """The mean over pixels of sqrt(ddx^2 + ddy^2), each in f32 as the reference's float32 flows give it, added in f64.  (The
    reference's np.mean adds the f32 values pairwise in f32: the last bits differ, nothing else.)"""
    d = np.asarray(flow_a, dtype=np.float32) - np.asarray(flow_b, dtype=np.float32)
    e = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return float(e.astype(np.float64).mean())


def tof_host(pred_cur, true_cur, pred_pre, true_pre, dtype=np.float64) -> float:
    """calculate_tOF: the flow previous -> current of the ground truth against that of the prediction."""
    return epe_host(farneback_host(true_pre, true_cur, dtype), farneback_host(pred_pre, pred_cur, dtype))


def shot_starts(n: int, cuts: Sequence[int] = ()) -> np.ndarray:
    """bool (n,): frame 0 and every frame a shot starts at."""
    first = np.zeros(n, dtype=bool)
    if n:
        first[0] = True
    for c in cuts:
        c = int(c)
        if not 0 <= c < max(n, 1):
            raise ValueError(f"cut {c} is outside the {n} frames")
        first[c] = True
    return first


def sequence_summary(tof, cuts: Sequence[int] = ()) -> dict:
    """Per-frame values (0.0 at shot starts) -> {"tof", "tof_mean" over all frames (mmedit's average, frame 0 counted as 0),
    "tof_pairs_mean" over the real pairs only}."""
    tof = np.asarray(tof, dtype=np.float64).reshape(-1)
    pairs = ~shot_starts(tof.size, cuts)
    return {"tof": tof, "tof_mean": float(tof.mean()) if tof.size else float("nan"),
            "tof_pairs_mean": float(tof[pairs].mean()) if pairs.any() else float("nan")}


def sequence_tof_host(pred, true, cuts: Sequence[int] = (), dtype=np.float64) -> dict:
    """pred, true: (N,h,w) planes.  Frame 0 scores 0.0 (mmedit's forward_test takes pre = cur for the first frame, and that 0 enters
    its average); so does the first frame of every shot in `cuts`, this project's extension: a flow across a cut measures nothing."""
    pred, true = np.asarray(pred), np.asarray(true)
    if pred.ndim != 3 or pred.shape != true.shape:
        raise ValueError(f"expected two (N,h,w) arrays of one shape, got {pred.shape}, {true.shape}")
    first = shot_starts(pred.shape[0], cuts)
    vals = [0.0 if first[i] else tof_host(pred[i], true[i], pred[i - 1], true[i - 1], dtype) for i in range(pred.shape[0])]
    return sequence_summary(vals, cuts)


def tof_csv(stats: dict) -> str:
    """One line per frame, ``frame,tof``."""
    return "frame,tof\n" + "".join(f"{i},{float(v)!r}\n" for i, v in enumerate(stats["tof"]))


# ---- the device entry ----------------------------------------------------------------------------------------------------------

def frame_tof(pred, true, *, first=None, cuts: Sequence[int] = (), rgb: bool = False):
    """pred, true: (N,h,w) planes on the HIP device (uint8, uint16 or f32, one dtype).  `first`: the optional (pred_prev, true_prev)
    pair of (h,w) planes that precedes plane 0; without it plane 0 scores 0.0.  Planes named in `cuts` score 0.0.  Returns f64 (N,)
    on the device: per plane the tOF of `tof_host`, by `hip.farneback_flow` and `hip.flow_epe` (no host sync).  ``rgb=True``: the
    "planes" are (N,3,h,w) uint8 RGB frames (`first` a pair of (3,h,w) frames), scored on the float Y of `rgb_to_y`."""
    import torch
    from .. import hip
    if not isinstance(pred, torch.Tensor) or not isinstance(true, torch.Tensor):
        raise TypeError("pred and true must be torch tensors")
    if not pred.is_cuda or not true.is_cuda:
        raise RuntimeError("frame_tof runs on the HIP device only (the host path is harness.tof.sequence_tof_host)")
    if pred.dim() != (4 if rgb else 3) or pred.shape != true.shape or pred.dtype != true.dtype or pred.device != true.device:
        raise ValueError(f"expected pred and true of one (N,h,w) - (N,3,h,w) with rgb - shape, dtype and device, got {pred.dtype} {tuple(pred.shape)}, "
                         f"{true.dtype} {tuple(true.shape)}")
    N = pred.shape[0]
    starts = shot_starts(N, cuts)
    pred, true = (t.view(torch.int16) if t.dtype == torch.uint16 else t for t in (pred, true))    # torch.cat has no uint16
    if first is not None:
        fp, ft = (t.view(torch.int16) if t.dtype == torch.uint16 else t for t in first)
        if tuple(fp.shape) != tuple(pred.shape[1:]) or tuple(ft.shape) != tuple(pred.shape[1:]) or fp.dtype != pred.dtype or \
                ft.dtype != pred.dtype or fp.device != pred.device or ft.device != pred.device:
            raise ValueError("first: a (pred_prev, true_prev) pair of planes of the shape, dtype and device of one plane of pred")
        starts[0] = 0 in [int(c) for c in cuts]
        pred, true = torch.cat([fp[None], pred]), torch.cat([ft[None], true])
    out = torch.zeros((N,), dtype=torch.float64, device=pred.device)
    if pred.shape[0] < 2:
        return out
    n = pred.shape[0] - 1                                              # pairs; both flows of all of them in one set of launches
    flows = hip.farneback_flow(torch.cat([pred[:-1], true[:-1]]), torch.cat([pred[1:], true[1:]]), rgb=rgb)
    epe = hip.flow_epe(flows[:n], flows[n:])
    keep = torch.from_numpy(~starts[N - n:]).to(pred.device)
    out[N - n:] = torch.where(keep, epe, torch.zeros_like(epe))
    return out
