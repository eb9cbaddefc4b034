"""BRISQUE (Blind/Referenceless Image Spatial Quality Evaluator), the second no-reference score of the reference's real-world table
(CVSR_train/metric/cal_VideoLQ.py::get_Real_world, next to NIQE; the implementation is CVSR_train/metric/brisque.py, a piq / pyiqa
port in f32 torch).

The numpy functions here are the contract (f64, `math.lgamma`); `frame_brisque` / `frame_brisque_features` compute the 36 features
per frame on the HIP device (fcvsr_brisque_features) and only the range scaling and the RBF support-vector regressor run on the
host.  There is no CPU fallback behind the device functions: host tensors raise.

The regressor (`BrisqueModel`: support vectors and their coefficients) is user-supplied, like a checkpoint: piq and pyiqa ship it
as brisque_svm_weights.pt / .pth.  It was trained on 8-bit material, so uint16 (10-bit) frames raise ValueError.

Domain: the scored plane holds 8-bit integers in [0,255], which is what the reference's brisque() works on after its own `* 255`,
what piq / pyiqa compute and what published BRISQUE numbers mean.  The reference's call site (cal_VideoLQ.py) hands brisque()
tensors that are already in [0,255], so its luma is 255 times too large; that quirk is not reproduced.

RGB frames are scored on the luma of YIQ (`yiq_luma`, convert_to="Y"), as the reference's brisque() does.  This "Y" is not the
BT.601 Y of YCbCr that NIQE and PSNR / SSIM take under the same keyword."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .niqe import bicubic_downscale
from .nss import GAM, check_frames, corr7, device_tables

SHIFTS = ((0, 1), (1, 0), (1, 1), (-1, 1))                  # np.roll shifts of the four paired products, over the whole plane
EPS32 = 2.0 ** -23                                          # the reference's safe_sqrt adds the f32 epsilon under the root
ALPHA = (0, 2, 6, 10, 14, 18, 20, 24, 28, 32)               # the entries of the 36 features that are grid values
RBF_GAMMA, RHO = 0.05, -153.591                             # the SVR's kernel width and offset (official MATLAB release)
# (lo, hi) of each feature in the official MATLAB release's training set; the regressor sees -1 + 2 (f - lo) / (hi - lo)
FEATURE_RANGES = np.array([
    [0.338, 10], [0.017204, 0.806612], [0.236, 1.642], [-0.123884, 0.20293], [0.000155, 0.712298], [0.001122, 0.470257],
    [0.244, 1.641], [-0.123586, 0.179083], [0.000152, 0.710456], [0.000975, 0.470984], [0.249, 1.555], [-0.135687, 0.100858],
    [0.000174, 0.684173], [0.000913, 0.534174], [0.258, 1.561], [-0.143408, 0.100486], [0.000179, 0.685696], [0.000888, 0.536508],
    [0.471, 3.264], [0.012809, 0.703171], [0.218, 1.046], [-0.094876, 0.187459], [1.5e-005, 0.442057], [0.001272, 0.40803],
    [0.222, 1.042], [-0.115772, 0.162604], [1.6e-005, 0.444362], [0.001374, 0.40243], [0.227, 0.996],
    [-0.117188, 0.09832299999999999], [3e-005, 0.531903], [0.001122, 0.369589], [0.228, 0.99], [-0.12243, 0.098658],
    [2.8e-005, 0.530092], [0.001118, 0.370399]], dtype=np.float64)
FEATURE_RANGES.setflags(write=False)


def gaussian_window() -> np.ndarray:
    """MATLAB fspecial('gaussian', 7, 7/6): computed in f64, thresholded at eps * max, normalised, then rounded once to f32 (the
    reference makes it `.float()`) and used as f64.  Symmetric, so correlation and convolution agree."""
    y, x = np.ogrid[-3.0:4.0, -3.0:4.0]
    sigma = 7.0 / 6
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    h /= h.sum()
    return h.astype(np.float32).astype(np.float64)


@dataclass(frozen=True)
class BrisqueModel:
    """The RBF support-vector regressor: sv (n, 36) support vectors in scaled-feature units and sv_coef (n,) coefficients."""
    sv: np.ndarray
    sv_coef: np.ndarray

    def __post_init__(self):
        sv = np.asarray(self.sv, dtype=np.float64)
        coef = np.asarray(self.sv_coef, dtype=np.float64)
        if coef.ndim == 2 and 1 in coef.shape:                  # the column vector of the piq file
            coef = coef.reshape(-1)
        if sv.ndim != 2 or sv.shape[1] != 36 or sv.shape[0] < 1:
            raise ValueError(f"BrisqueModel.sv must have shape (n, 36), got {sv.shape}")
        if coef.shape != (sv.shape[0],):
            raise ValueError(f"BrisqueModel.sv_coef must have shape ({sv.shape[0]},), got {coef.shape}")
        object.__setattr__(self, "sv", np.ascontiguousarray(sv))
        object.__setattr__(self, "sv_coef", np.ascontiguousarray(coef))

    @classmethod
    def load(cls, path) -> "BrisqueModel":
        """Read the piq / pyiqa weights file (`torch.load` of a `(sv_coef, sv)` tuple; sv as (n,36) or (36,n)), or an .npz with the
        keys sv_coef and sv."""
        if str(path).endswith(".npz"):
            with np.load(path) as f:
                coef, sv = f["sv_coef"], f["sv"]
        else:
            import torch
            obj = torch.load(path, map_location="cpu", weights_only=True)
            if not isinstance(obj, (tuple, list)) or len(obj) != 2:
                raise ValueError(f"{path}: expected a (sv_coef, sv) pair, got {type(obj).__name__}")
            coef, sv = (np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64) for t in obj)
        sv = np.asarray(sv, dtype=np.float64)
        if sv.ndim == 2 and sv.shape[1] != 36 and sv.shape[0] == 36:
            sv = sv.T
        return cls(sv, coef)


def _check_model(model) -> BrisqueModel:
    if not isinstance(model, BrisqueModel):
        raise ValueError(f"model must be a BrisqueModel, got {type(model).__name__}")
    return BrisqueModel(model.sv, model.sv_coef)            # re-validates the shapes of a hand-made instance


_TABLES = None


def brisque_tables() -> np.ndarray:
    """(4, 9801) f64 over `GAM`, from `math.lgamma`: the GGD ratio G(1/g) G(3/g) / G(2/g)^2, the AGGD ratio G(2/g)^2 / (G(1/g) G(3/g)),
    the eta factor G(2/g) / sqrt(G(1/g) G(3/g)) and g itself.  Computed once; the device kernel reads an uploaded copy, so host and
    device search the same numbers."""
    global _TABLES
    if _TABLES is None:
        t = np.empty((4, GAM.size), dtype=np.float64)
        t[3] = GAM
        for i, g in enumerate(GAM):
            l1, l2, l3 = math.lgamma(1.0 / g), math.lgamma(2.0 / g), math.lgamma(3.0 / g)
            t[0, i] = math.exp(l1 + l3 - 2 * l2)
            t[1, i] = math.exp(2 * l2 - (l1 + l3))
            t[2, i] = math.exp(l2 - (l1 + l3) / 2)
        t.setflags(write=False)
        _TABLES = t
    return _TABLES


def yiq_luma(rgb: np.ndarray) -> np.ndarray:
    """The rounded YIQ luma of (3,H,W) uint8 RGB as the reference's to_y_channel(., 255, 'yiq') gives it, defined on integers:
    round_half_even((299 R + 587 G + 114 B) / 1000), uint8.  Not the Y of YCbCr that NIQE scores."""
    x = np.asarray(rgb)
    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[0] != 3:
        raise ValueError(f"expected (3,H,W) uint8 RGB, got {x.dtype} {x.shape}")
    v = 299 * x[0].astype(np.int64) + 587 * x[1].astype(np.int64) + 114 * x[2].astype(np.int64)
    q, r = v // 1000, v % 1000
    return (q + ((r > 500) | ((r == 500) & (q % 2 == 1)))).astype(np.uint8)


def _mscn(img: np.ndarray, w: np.ndarray) -> np.ndarray:
    """(img - mu) / (sigma + 1) over a zero-padded plane: the reference's padding='same' is F.pad 'constant'."""
    mu, e2 = corr7(img, w, "constant"), corr7(img * img, w, "constant")
    return (img - mu) / (np.sqrt(np.abs(e2 - mu * mu) + EPS32) + 1.0)


def _first_min(table: np.ndarray, target: float) -> int:
    """Index of the first minimum of |table - target|; 0 when the target is NaN (argmin over all-NaN)."""
    if math.isnan(target):
        return 0
    return int(np.argmin(np.abs(table - target)))


def _shifted(m: np.ndarray, shift) -> np.ndarray:
    return np.roll(m, shift, axis=(0, 1))


def _plane_features(m: np.ndarray, shifted=_shifted) -> np.ndarray:
    """The 18 features of one MSCN plane.  `shifted` is np.roll over the whole plane; the tests swap it to show that the wrap
    matters."""
    t = brisque_tables()
    n, total = np.float64(m.size), lambda a: np.float64(a.sum())
    f = np.empty(18, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma_sq, e = total(m * m) / n, total(np.abs(m)) / n
        i = _first_min(t[0], float(sigma_sq / (e * e)))
        f[0], f[1] = t[3, i], sigma_sq
        for k, shift in enumerate(SHIFTS):
            p = m * shifted(m, shift)
            sq, neg, pos = p * p, p < 0, p > 0
            sq_l, sq_r = total(np.where(neg, sq, 0.0)), total(np.where(pos, sq, 0.0))
            left, right = np.sqrt(sq_l / total(neg)), np.sqrt(sq_r / total(pos))            # 0 / 0 = NaN for an empty side
            gh = left / right
            mean_abs = total(np.abs(p)) / n
            rhat = (mean_abs * mean_abs) / ((sq_l + sq_r) / n)
            g2 = gh * gh
            rhatnorm = (rhat * (g2 * gh + 1.0) * (gh + 1.0)) / ((g2 + 1.0) * (g2 + 1.0))
            i = _first_min(t[1], float(rhatnorm))
            f[2 + 4 * k:6 + 4 * k] = t[3, i], (right - left) * t[2, i], left * left, right * right
    return f


def _check_plane(y) -> np.ndarray:
    y = np.asarray(y)
    if y.dtype == np.uint16:
        raise ValueError("BRISQUE is defined on 8-bit frames: uint16 (10-bit) planes are not supported")
    if y.ndim != 2:
        raise ValueError(f"expected an (H,W) plane, got shape {y.shape}")
    _check_size(*y.shape)
    return y.astype(np.float64)


def _check_size(h: int, w: int):
    if h % 2 or w % 2 or h < 16 or w < 16:
        raise ValueError(f"BRISQUE needs even H and W of at least 16, got {h}x{w}")


def _check_variance(features: np.ndarray):
    """The reference asserts a non-zero variance of the MSCN plane (torch.isclose of its sigma against 0)."""
    f = np.asarray(features).reshape(-1, 36)
    if (np.sqrt(f[:, [1, 19]]) <= 1e-8).any():
        raise ValueError("BRISQUE needs a plane with non-zero variance: the MSCN plane is identically zero")


def brisque_features(y: np.ndarray, _shifted=_shifted) -> np.ndarray:
    """y: (H,W) plane in [0,255] holding integers (uint8, or a float plane of integer values), H and W even and >= 16.  Returns
    (36,) f64 in the reference's order: scale 1, then scale 2 (the MATLAB-style 2x down-scale of y / 255, times 255, not rounded);
    per scale [alpha, sigma^2] of the MSCN plane's GGD fit, then (alpha, eta, sigma_l^2, sigma_r^2) of the AGGD fit of each of the
    four shifted products.  A product with no negative or no positive sample gives alpha 0.2 and NaN where the formulas give NaN.
    A plane whose MSCN is identically zero raises ValueError, where the reference asserts."""
    img = _check_plane(y)
    w = gaussian_window()
    feats = []
    for scale in (1, 2):
        feats.append(_plane_features(_mscn(img, w), _shifted))
        if scale == 1:
            img = bicubic_downscale(img / 255.0, 2) * 255.0
    feats = np.concatenate(feats)
    _check_variance(feats)
    return feats


def scale_features(features: np.ndarray) -> np.ndarray:
    """-1 + 2 (f - lo) / (hi - lo) with `FEATURE_RANGES`, on the last axis (36)."""
    f = np.asarray(features, dtype=np.float64)
    if f.shape[-1:] != (36,):
        raise ValueError(f"expected (..., 36) features, got shape {f.shape}")
    return -1.0 + 2.0 * (f - FEATURE_RANGES[:, 0]) / (FEATURE_RANGES[:, 1] - FEATURE_RANGES[:, 0])


def brisque_score(features: np.ndarray, model: BrisqueModel) -> float:
    """sum_k sv_coef[k] exp(-0.05 ||scale_features(f) - sv[k]||^2) + 153.591 in f64; lower is better."""
    model = _check_model(model)
    f = np.asarray(features, dtype=np.float64)
    if f.shape != (36,):
        raise ValueError(f"expected (36,) features, got shape {f.shape}")
    d = scale_features(f)[None, :] - model.sv
    return float(np.exp(-RBF_GAMMA * (d * d).sum(axis=1)) @ model.sv_coef - RHO)


def brisque(y: np.ndarray, model: BrisqueModel) -> float:
    """BRISQUE of one (H,W) plane in [0,255] (integers); 8-bit only (see `brisque_features`)."""
    return brisque_score(brisque_features(y), model)


# ---- device ------------------------------------------------------------------------------------------------------------------------
def frame_brisque_features(frames, *, quantise: Optional[str] = None, convert_to: Optional[str] = None):
    """frames: (N,C,H,W) on the HIP device, uint8 with `quantise=None`, or f32 model output in [0,1] with any strides, quantised in
    the kernel ("truncate" / "round", as `device_metrics.frame_metrics`).  C = 1, or 3 (RGB) with convert_to="Y": the integer luma
    of YIQ (`yiq_luma`) - this "Y" is not the Y of YCbCr that NIQE's convert_to="Y" selects.  H and W even and >= 16.  Returns the
    (N, 36) f64 device tensor of `brisque_features` per frame without a host sync.  uint16 (10-bit) frames raise ValueError."""
    import torch
    from .. import hip
    from .device_metrics import _QUANTISE
    to_y = check_frames(frames, quantise, convert_to, "BRISQUE")
    N, _, H, W = frames.shape
    _check_size(H, W)
    if N == 0:
        return torch.empty((0, 36), dtype=torch.float64, device=frames.device)
    with torch.cuda.device(frames.device):
        return hip.brisque_features(frames, _QUANTISE[quantise], to_y, gaussian_window(),
                                    device_tables("brisque", brisque_tables(), frames.device))


def scores_from_features(features: np.ndarray, model: BrisqueModel) -> np.ndarray:
    """(N, 36) host features -> (N,) f64 BRISQUE, one `brisque_score` per frame.  ValueError for a frame whose MSCN plane is
    identically zero, as `brisque_features` raises."""
    f = np.asarray(features, dtype=np.float64)
    if f.ndim != 2 or f.shape[1] != 36:
        raise ValueError(f"expected (N, 36) features, got shape {f.shape}")
    _check_variance(f)
    return np.array([brisque_score(row, model) for row in f], dtype=np.float64)


def frame_brisque(frames, model: BrisqueModel, *, quantise: Optional[str] = None, convert_to: Optional[str] = None) -> np.ndarray:
    """BRISQUE of N device frames (arguments as `frame_brisque_features`): the features are computed on the device, fetched in one
    copy, and the regressor (`brisque_score`) runs on the host in f64 per frame.  Returns (N,) f64 numpy."""
    model = _check_model(model)
    feats = frame_brisque_features(frames, quantise=quantise, convert_to=convert_to)
    return scores_from_features(feats.cpu().numpy(), model)
