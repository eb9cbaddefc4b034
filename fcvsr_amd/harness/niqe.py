"""NIQE (Natural Image Quality Evaluator), the no-reference score of SR frames that have no ground truth (reference
mmedit/core/evaluation/metrics.py:398-590 estimate_aggd_param / compute_feature / niqe_core / niqe, used by
CVSR_train/metric/cal_VideoLQ.py; known answers at tests/test_metrics/test_metrics.py:107-138), and the MATLAB-style antialiased
bicubic down-scale it needs between its two scales (mmedit/datasets/pipelines/matlab_like_resize.py), with the up-scale half of the
same function (`bicubic_upscale`: MATLAB `imresize`, the bicubic baseline of SR tables) next to it.

The numpy functions here are the contract (f64, gamma from `math`); `frame_niqe` / `frame_niqe_features` compute the 36 features
per 96 x 96 block on the HIP device (fcvsr_niqe_features) and only the 36 x 36 multivariate-Gaussian distance runs on the host.
There is no CPU fallback behind the device functions: host tensors raise.

The pristine model (`NiqeModel`) is user-supplied, like a checkpoint: mmedit ships it as
mmedit/core/evaluation/niqe_pris_params.npz.  It is defined on 8-bit samples, so uint16 (10-bit) frames raise ValueError; 10-bit
scoring is out of scope, as convert_to="Y" is for 10-bit PSNR / SSIM."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .nss import GAM, check_frames, corr7, device_tables

BLOCK = 96                                                  # block side at scale 1 (the official value; 48 at scale 2)
_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))                 # np.roll shifts of the four paired products
# antialiased cubic taps 0.5 cubic(0.5 x) at 2x (inputs 2i-3 .. 2i+4) and 0.25 cubic(0.25 x) at 4x (inputs 4i-6 .. 4i+9)
_TAPS = {2: np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0,
         4: np.array([-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7], dtype=np.float64) / 4096.0}


@dataclass(frozen=True)
class NiqeModel:
    """The pristine multivariate-Gaussian model: mu (36,), cov (36,36) and the 7 x 7 Gaussian window of the MSCN stage."""
    mu: np.ndarray
    cov: np.ndarray
    window: np.ndarray

    def __post_init__(self):
        for name, shape in (("mu", (36,)), ("cov", (36, 36)), ("window", (7, 7))):
            a = np.asarray(getattr(self, name), dtype=np.float64)
            if name == "mu" and a.shape == (1, 36):             # the row vector of mmedit's file
                a = a[0]
            if a.shape != shape:
                raise ValueError(f"NiqeModel.{name} must have shape {shape}, got {a.shape}")
            object.__setattr__(self, name, np.ascontiguousarray(a))

    @classmethod
    def load(cls, path) -> "NiqeModel":
        """Read an npz with the mmedit key names mu_pris_param, cov_pris_param, gaussian_window."""
        with np.load(path) as f:
            return cls(f["mu_pris_param"], f["cov_pris_param"], f["gaussian_window"])


def _check_model(model) -> NiqeModel:
    if not isinstance(model, NiqeModel):
        raise ValueError(f"model must be a NiqeModel, got {type(model).__name__}")
    return NiqeModel(model.mu, model.cov, model.window)     # re-validates the shapes of a hand-made instance


_TABLES = None


def aggd_tables() -> np.ndarray:
    """(4, 9801) f64 over `GAM`: r_gam = G(2/g)^2 / (G(1/g) G(3/g)), sqrt(G(1/g) / G(3/g)) (std -> beta), G(2/g) / G(1/g) (the mean
    feature's factor) and g itself.  Computed once; the device kernel reads an uploaded copy, so host and device use the same
    numbers."""
    global _TABLES
    if _TABLES is None:
        t = np.empty((4, GAM.size), dtype=np.float64)
        t[3] = GAM
        for i, g in enumerate(GAM):
            rec = 1.0 / g
            g1, g2, g3 = math.gamma(rec), math.gamma(rec * 2), math.gamma(rec * 3)
            t[0, i] = g2 * g2 / (g1 * g3)
            t[1, i] = math.sqrt(math.gamma(1 / g) / math.gamma(3 / g))
            t[2, i] = math.gamma(2 / g) / math.gamma(1 / g)
        t.setflags(write=False)
        _TABLES = t
    return _TABLES


def _reflect(idx: np.ndarray, n: int) -> np.ndarray:
    """Out-of-range indices reflected with edge repeat: -1 -> 0, -2 -> 1, n -> n-1."""
    m = np.mod(idx, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def bicubic_downscale(img: np.ndarray, factor: int) -> np.ndarray:
    """MATLAB-style antialiased bicubic down-scale of the last two axes by 2 or 4 (both multiples of `factor`), on the input's
    scale.  Rows first, then columns.  The arithmetic is the reference's, so the result has its bits: the input of each pass is
    rounded to f32, every tap's product is an f32, and the products are added in tap order in f32 (the taps are exact in f32).
    Returned as f64 (every value is an f32)."""
    if factor not in _TAPS:
        raise ValueError(f"factor must be 2 or 4, got {factor!r}")
    x = np.asarray(img)
    if x.ndim < 2 or x.shape[-2] % factor or x.shape[-1] % factor or 0 in x.shape[-2:]:
        raise ValueError(f"the last two axes must be non-empty multiples of {factor}, got shape {x.shape}")
    w = _TAPS[factor].astype(np.float32)
    first = factor // 2 - w.size // 2                       # input index of tap 0 at output 0: -3 at 2x, -6 at 4x
    x = x.astype(np.float32)
    for axis in (-2, -1):
        n = x.shape[axis]
        base = np.arange(n // factor) * factor + first
        acc = w[0] * np.take(x, _reflect(base, n), axis=axis)
        for k in range(1, w.size):
            acc = acc + w[k] * np.take(x, _reflect(base + k, n), axis=axis)
        x = acc
    assert x.dtype == np.float32
    return x.astype(np.float64)


# cubic(x) taps of the up-scale (a = -0.5, no antialiasing): row `o mod factor` holds the weights of inputs floor(c) - 1 .. floor(c) + 2
# around the centre c = (o + 0.5) / factor - 0.5 of output o.  Multiples of 1/128 (2x) and 1/1024 (4x), exact in f32.
UPSCALE_TAPS = {2: np.array([[-3, 29, 111, -9], [-9, 111, 29, -3]], dtype=np.float64) / 128.0,
                4: np.array([[-45, 399, 745, -75], [-7, 93, 987, -49], [-49, 987, 93, -7], [-75, 745, 399, -45]],
                            dtype=np.float64) / 1024.0}
_INT_PEAK = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 1023}


def bicubic_upscale(img: np.ndarray, factor: int, out: str = "f32") -> np.ndarray:
    """MATLAB-style bicubic up-scale (`imresize`, a = -0.5, symmetric border: the "Bicubic" row of SR tables) of the last two axes
    by 2 or 4, on the input's scale; any H, W >= 1.  Rows first, then columns, with the reference's arithmetic and so its bits:
    the input of each pass is rounded to f32, every tap's product is an f32, and the four products are added in tap order in f32.
    Out-of-range taps are reflected with edge repeat (period 2n, so a plane narrower than the kernel reflects several times).
    uint16 input is 10-bit: a sample above 1023 is read as 1023.

    out="f32": f64 in which every value is an f32, neither clipped nor rounded (uint8 input gives values around [0, 255]).
    out="int" (uint8 / uint16 input only): clipped to [0, peak] (255 or 1023), rounded half to even, in the input's dtype - what
    `imresize` returns for an integer image."""
    if factor not in UPSCALE_TAPS:
        raise ValueError(f"factor must be 2 or 4, got {factor!r}")
    if out not in ("f32", "int"):
        raise ValueError(f'out must be "f32" or "int", got {out!r}')
    x = np.asarray(img)
    if x.ndim < 2 or 0 in x.shape[-2:]:
        raise ValueError(f"the last two axes must be non-empty, got shape {x.shape}")
    peak = _INT_PEAK.get(x.dtype)
    if out == "int" and peak is None:
        raise ValueError(f'out="int" needs uint8 or uint16 input, got {x.dtype}')
    src_dtype = x.dtype
    if x.dtype == np.uint16:
        x = np.minimum(x, 1023)
    w = UPSCALE_TAPS[factor].astype(np.float32)
    x = x.astype(np.float32)
    for axis in (-2, -1):
        n = x.shape[axis]
        o = np.arange(n * factor)
        first = (o - factor // 2) // factor - 1             # floor(c) - 1
        shape = (-1, 1) if axis == -2 else (-1,)
        acc = w[o % factor, 0].reshape(shape) * np.take(x, _reflect(first, n), axis=axis)
        for k in range(1, 4):
            acc = acc + w[o % factor, k].reshape(shape) * np.take(x, _reflect(first + k, n), axis=axis)
        x = acc
    assert x.dtype == np.float32
    if out == "int":
        return np.around(np.clip(x, 0, peak)).astype(src_dtype)
    return x.astype(np.float64)


def _conv7(img: np.ndarray, window: np.ndarray) -> np.ndarray:
    """scipy.ndimage.convolve(img, window, mode='nearest'): a true convolution (flipped window) with replicated borders,
    accumulated from 0 in the row-major order of the flipped window."""
    return corr7(img, window[::-1, ::-1], "edge")


def _mscn(img: np.ndarray, window: np.ndarray, f32: bool = False) -> np.ndarray:
    """(img - mu) / (sigma + 1).  ``f32``: the reference's niqe() hands niqe_core an f32 plane, so at scale 1 scipy returns both
    convolutions rounded to f32 and mu^2, the difference, the square root, the sum and the quotient are f32 operations; the same
    roundings are applied here (sqrt and the quotient are formed in f64 and rounded once, which equals the f32 operation).  The
    result then holds f32 values.  Scale 2 runs on the f64 output of the down-scale, in the reference as here."""
    mu, e2 = _conv7(img, window), _conv7(img * img, window)
    if not f32:
        return (img - mu) / (np.sqrt(np.abs(e2 - mu * mu)) + 1.0)
    r = lambda a: a.astype(np.float32).astype(np.float64)       # one rounding to f32
    mu = r(mu)
    sigma = r(np.sqrt(np.abs(r(r(e2) - r(mu * mu)))))
    return r(r(img - mu) / r(sigma + 1.0))


def _aggd(v: np.ndarray):
    """estimate_aggd_param on every row of v (blocks, n): (grid index of alpha, left_std, right_std)."""
    r_gam = aggd_tables()[0]
    sq = v * v
    neg, pos = v < 0, v > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.sqrt(np.where(neg, sq, 0.0).sum(axis=1) / neg.sum(axis=1))
        right = np.sqrt(np.where(pos, sq, 0.0).sum(axis=1) / pos.sum(axis=1))
        gammahat = left / right
        g2, mean_abs = gammahat * gammahat, np.abs(v).sum(axis=1) / v.shape[1]
        rhat = (mean_abs * mean_abs) / (sq.sum(axis=1) / v.shape[1])
        rhatnorm = (rhat * (g2 * gammahat + 1) * (gammahat + 1)) / ((g2 + 1) * (g2 + 1))
        pos_idx = np.argmin((r_gam[None, :] - rhatnorm[:, None]) ** 2, axis=1)   # first minimum; index 0 for a NaN row
    return pos_idx, left, right


def _scale_features(mscn: np.ndarray, bs: int) -> np.ndarray:
    nbh, nbw = mscn.shape[0] // bs, mscn.shape[1] // bs
    blocks = mscn.reshape(nbh, bs, nbw, bs).transpose(0, 2, 1, 3).reshape(nbh * nbw, bs, bs)   # row-major block order
    t = aggd_tables()
    feat = np.empty((blocks.shape[0], 18), dtype=np.float64)
    idx, left, right = _aggd(blocks.reshape(blocks.shape[0], -1))
    feat[:, 0] = GAM[idx]
    feat[:, 1] = (left * t[1, idx] + right * t[1, idx]) / 2
    for k, shift in enumerate(_SHIFTS):
        prod = blocks * np.roll(blocks, shift, axis=(1, 2))      # circular inside the block
        idx, left, right = _aggd(prod.reshape(prod.shape[0], -1))
        bl, br = left * t[1, idx], right * t[1, idx]
        feat[:, 2 + 4 * k] = GAM[idx]
        feat[:, 3 + 4 * k] = (br - bl) * t[2, idx]
        feat[:, 4 + 4 * k] = bl
        feat[:, 5 + 4 * k] = br
    return feat


def crop_geometry(h: int, w: int, crop_border: int):
    """(rows, columns, block rows, block columns) of the scored plane: crop_border off every side, then the largest top-left
    multiple of 96.  ValueError when fewer than 2 blocks remain (the covariance of the block features is undefined)."""
    if crop_border < 0:
        raise ValueError(f"crop_border must be >= 0, got {crop_border}")
    nbh, nbw = max(h - 2 * crop_border, 0) // BLOCK, max(w - 2 * crop_border, 0) // BLOCK
    if nbh * nbw < 2:
        raise ValueError(f"a {h}x{w} plane with crop_border={crop_border} holds {nbh * nbw} 96x96 blocks; NIQE needs at least 2")
    return nbh * BLOCK, nbw * BLOCK, nbh, nbw


def niqe_features(y: np.ndarray, model: NiqeModel, crop_border: int = 0) -> np.ndarray:
    """y: (H,W) Y plane in [0,255] holding integers (the reference rounds before it scores).  Returns (blocks, 36) f64, blocks in
    row-major order: 18 AGGD features at scale 1 and 18 at scale 2 (after the 2x down-scale of the cropped plane).  A block with no
    negative or no positive sample (an all-black letterbox block) has alpha 0.2 and NaN in its other entries, as in the reference.
    uint16 (10-bit) planes raise ValueError: the pristine model is defined on the 8-bit range.

    The arithmetic follows the plane's dtype as the reference's niqe_core does: integer and f64 planes are scored in f64 throughout
    (so is the device); a float32 plane - what the reference's niqe() makes of every input, and what its published known answers
    contain - gets the f32 roundings of that path in the scale-1 MSCN stage (`_mscn`).  The two differ where a plane is nearly flat
    and bright, by 1e-4 relative on mmedit's baboon test image."""
    model = _check_model(model)
    y = np.asarray(y)
    as_f32 = y.dtype == np.float32
    if y.dtype == np.uint16:
        raise ValueError("NIQE is defined on 8-bit frames: uint16 (10-bit) planes are not supported")
    if y.ndim != 2:
        raise ValueError(f"expected an (H,W) plane, got shape {y.shape}")
    hc, wc, _, _ = crop_geometry(y.shape[0], y.shape[1], crop_border)
    img = y[crop_border:crop_border + hc, crop_border:crop_border + wc].astype(np.float64)
    feats = []
    for scale in (1, 2):
        feats.append(_scale_features(_mscn(img, model.window, f32=as_f32 and scale == 1), BLOCK // scale))
        if scale == 1:
            img = bicubic_downscale(img / 255.0, 2) * 255.0
    return np.concatenate(feats, axis=1)


def niqe_score(features: np.ndarray, model: NiqeModel) -> float:
    """The distance between the pristine model and the Gaussian fitted to (blocks, 36) features: the mean ignores NaN entries, the
    covariance uses the rows without NaN."""
    model = _check_model(model)
    f = np.asarray(features, dtype=np.float64)
    if f.ndim != 2 or f.shape[1] != 36 or f.shape[0] < 2:
        raise ValueError(f"expected (blocks >= 2, 36) features, got shape {f.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
        mu_d = np.nanmean(f, axis=0)
        cov_d = np.cov(f[~np.isnan(f).any(axis=1)], rowvar=False)
        inv = np.linalg.pinv((model.cov + cov_d) / 2)
        d = model.mu - mu_d
        return float(np.sqrt(d @ inv @ d))


def niqe(y: np.ndarray, model: NiqeModel, crop_border: int = 0) -> float:
    """NIQE of one (H,W) Y plane in [0,255] (integers); lower is better.  8-bit only (see `niqe_features`)."""
    return niqe_score(niqe_features(y, model, crop_border), model)


# ---- device ------------------------------------------------------------------------------------------------------------------------
def frame_niqe_features(frames, model: NiqeModel, *, crop_border: int = 0, quantise: Optional[str] = None,
                        convert_to: Optional[str] = None):
    """frames: (N,C,H,W) on the HIP device, uint8 with `quantise=None`, or f32 model output in [0,1] with any strides, quantised in
    the kernel ("truncate" / "round", as `device_metrics.frame_metrics`).  C = 1, or 3 (RGB) with convert_to="Y": the Y of YCbCr,
    rounded half to even.  Returns the (N, blocks, 36) f64 device tensor of `niqe_features` per frame without a host sync.
    uint16 (10-bit) frames raise ValueError."""
    import torch
    from .. import hip
    from .device_metrics import _QUANTISE
    model = _check_model(model)
    to_y = check_frames(frames, quantise, convert_to, "NIQE")
    N, _, H, W = frames.shape
    _, _, nbh, nbw = crop_geometry(H, W, crop_border)
    if N == 0:
        return torch.empty((0, nbh * nbw, 36), dtype=torch.float64, device=frames.device)
    with torch.cuda.device(frames.device):
        return hip.niqe_features(frames, _QUANTISE[quantise], int(crop_border), to_y, model.window[::-1, ::-1],
                                 device_tables("niqe", aggd_tables(), frames.device))


def scores_from_features(features: np.ndarray, model: NiqeModel) -> np.ndarray:
    """(N, blocks, 36) host features -> (N,) f64 NIQE, one `niqe_score` per frame."""
    return np.array([niqe_score(f, model) for f in features], dtype=np.float64)


def frame_niqe(frames, model: NiqeModel, *, crop_border: int = 0, quantise: Optional[str] = None,
               convert_to: Optional[str] = None) -> np.ndarray:
    """NIQE of N device frames (arguments as `frame_niqe_features`): the features are computed on the device, fetched in one copy,
    and the 36 x 36 Gaussian distance (`niqe_score`) runs on the host in f64 per frame.  Returns (N,) f64 numpy."""
    feats = frame_niqe_features(frames, model, crop_border=crop_border, quantise=quantise, convert_to=convert_to)
    return scores_from_features(feats.cpu().numpy(), model)
