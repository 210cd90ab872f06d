"""PSNR / SSIM of super-resolved images the way the reference's tester scores them.

The reference computes both on the HOST with scikit-image (metrics/sr_metrics.py:8-14: ``peak_signal_noise_ratio(GT, P,
data_range=1)`` and ``structural_similarity(GT, P, data_range=1, multichannel=True)``) on (H, W, C) images whose borders
were cropped by ``margin = ceil(sr_scale)`` pixels (metrics/sr_metrics.py:108-115, metrics/sr_evaluation.py:152).  They
stay host-side numpy here too: they are the caller's bookkeeping around the hot path, not part of it.

scikit-image is not installed in the build image, so this is a restatement of the published algorithms:
  * PSNR  = 10 log10(data_range^2 / mean((GT - P)^2)) in float64 — identical to oracle.psnr, which the golden fixtures pin;
  * SSIM  = scikit-image's default (Wang et al. 2004): 7x7 uniform window (scipy.ndimage.uniform_filter, reflect
    borders), K1 = 0.01, K2 = 0.03, sample covariance (N / (N - 1)), mean over the map cropped by (win - 1) / 2 pixels,
    averaged over channels.  **Parity unpinned** (no scikit-image here to generate vectors from); the tests check the
    definition on closed-form cases.

``device_scores`` computes both on the GPU (the HIP kernel behind rdst_sr_scores, include/rdst_hip.h) to this file's float64
precision, with only 2 N doubles per batch left for the host; ``SRMetrics(..., device="cuda")`` scores tensors with it.

``msssim`` is the third pixel metric the reference's list names (metrics/sr_metrics.py:36): multi-scale SSIM by the definition of
include/rdst_hip_msssim.h, float64 numpy here and the value-only call of rdst_msssim_loss in ``device_msssim``.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Sequence, Union

import numpy as np

try:  # scipy is available in the image; the pure-numpy path below is the same filter for when it is not
    from scipy.ndimage import uniform_filter as _uniform_filter
except Exception:  # noqa: BLE001
    _uniform_filter = None


def psnr(gt: np.ndarray, pred: np.ndarray, data_range: float = 1.0) -> float:
    """skimage.metrics.peak_signal_noise_ratio (metrics/sr_metrics.py:8-9)."""
    gt = np.asarray(gt, dtype=np.float64)
    pred = np.asarray(pred, dtype=np.float64)
    err = np.mean((gt - pred) ** 2)
    if err == 0:
        return float("inf")
    return float(10.0 * math.log10((data_range ** 2) / err))


def _box(a: np.ndarray, win: int) -> np.ndarray:
    if _uniform_filter is not None:
        return _uniform_filter(a, size=win, mode="reflect")
    pad = win // 2
    ap = np.pad(a, pad, mode="symmetric")          # scipy's 'reflect' = numpy's 'symmetric'
    c = np.cumsum(np.cumsum(np.pad(ap, ((1, 0), (1, 0))), 0), 1)
    H, W = a.shape
    return (c[win:win + H, win:win + W] - c[:H, win:win + W] - c[win:win + H, :W] + c[:H, :W]) / (win * win)


def ssim(gt: np.ndarray, pred: np.ndarray, data_range: float = 1.0, win_size: int = 7) -> float:
    """skimage.metrics.structural_similarity(GT, P, data_range=1, multichannel=True) on (H, W, C) images
    (metrics/sr_metrics.py:12-13)."""
    gt = np.asarray(gt, dtype=np.float64)
    pred = np.asarray(pred, dtype=np.float64)
    if gt.ndim == 2:
        gt, pred = gt[..., None], pred[..., None]
    if gt.shape != pred.shape or min(gt.shape[:2]) < win_size:
        raise ValueError("ssim: images must have the same shape and be at least win_size in both dimensions")
    NP = win_size * win_size
    cov_norm = NP / (NP - 1.0)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    pad = (win_size - 1) // 2
    vals = []
    for c in range(gt.shape[-1]):
        X, Y = gt[..., c], pred[..., c]
        ux, uy = _box(X, win_size), _box(Y, win_size)
        uxx, uyy, uxy = _box(X * X, win_size), _box(Y * Y, win_size), _box(X * Y, win_size)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        vals.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())
    return float(np.mean(vals))


def _pool2(a: np.ndarray) -> np.ndarray:
    """2x2 average of a float32 (H, W) image in float32, floor sizes: ((a + b) + (c + d)) * 0.25, the upper pair first."""
    H2, W2 = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * H2, :2 * W2]
    return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * np.float32(0.25)


def _valid_filter(a: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """The separable weighted window sum of a float64 (H, W) image at the valid positions."""
    win = taps.shape[0]
    Ho, Wo = a.shape[0] - win + 1, a.shape[1] - win + 1
    rows = sum(taps[k] * a[:, k:k + Wo] for k in range(win))
    return sum(taps[k] * rows[k:k + Ho] for k in range(win))


def msssim(gt: np.ndarray, pred: np.ndarray, data_range: float = 1.0, levels: int = 5, weights=None, win_size: int = 11,
           sigma: float = 1.5) -> float:
    """Multi-scale SSIM (Wang et al. 2003) of (H, W, C) or (H, W) images with a Gaussian window, by the definition of
    include/rdst_hip_msssim.h: the images are taken as float32 and averaged 2x2 in float32 from level to level (floor
    sizes), the window sums are float64 over the valid positions; the mean contrast-structure term of every level but the
    last and the mean SSIM of the last, each to the power of its weight, multiplied per channel (0 when a mean is not
    positive) and averaged over the channels.  The reference's metric list names it (metrics/sr_metrics.py:36)."""
    from .loss.msssim import check_size, level_weights
    from .loss.ssim import window_taps
    w = level_weights(levels, weights)
    taps, cn = window_taps("gaussian", win_size, sigma)
    if not data_range > 0:
        raise ValueError(f"msssim: data_range={data_range} must be positive")
    gt = np.asarray(gt, dtype=np.float32)
    pred = np.asarray(pred, dtype=np.float32)
    if gt.ndim == 2:
        gt, pred = gt[..., None], pred[..., None]
    if gt.shape != pred.shape or gt.ndim != 3:
        raise ValueError("msssim: images must have the same (H, W, C) shape")
    check_size("msssim", gt.shape[0], gt.shape[1], taps.shape[0], w.shape[0])
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for c in range(gt.shape[-1]):
        x32, y32 = np.ascontiguousarray(gt[..., c]), np.ascontiguousarray(pred[..., c])
        ms = 1.0
        for j in range(w.shape[0]):
            if j:
                x32, y32 = _pool2(x32), _pool2(y32)
            X, Y = x32.astype(np.float64), y32.astype(np.float64)
            ux, uy = _valid_filter(X, taps), _valid_filter(Y, taps)
            uxx, uyy, uxy = _valid_filter(X * X, taps), _valid_filter(Y * Y, taps), _valid_filter(X * Y, taps)
            vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
            term = (2 * vxy + C2) / (vx + vy + C2)
            if j == w.shape[0] - 1:
                term = term * (2 * ux * uy + C1) / (ux * ux + uy * uy + C1)
            m = float(term.mean())
            ms = ms * m ** w[j] if (m > 0 and ms > 0) else 0.0
        vals.append(ms)
    return float(np.mean(vals))


_FUNCS = {"psnr": psnr, "ssim": ssim, "msssim": msssim}


def _to_hwc_list(imgs, margin: int) -> List[np.ndarray]:
    """SRMetrics.prepare_data (metrics/sr_metrics.py:96-118): tensors (N, C, H, W) / (C, H, W) or arrays (N, H, W, C) /
    (H, W, C), lists of either; borders cropped by ``margin``."""
    import torch
    if isinstance(imgs, (list, tuple)):
        imgs = torch.stack(list(imgs)) if isinstance(imgs[0], torch.Tensor) else np.stack(list(imgs))
    if isinstance(imgs, torch.Tensor):
        a = imgs.detach().float().cpu().numpy()
        a = a.transpose(1, 2, 0) if a.ndim == 3 else a.transpose(0, 2, 3, 1)
    else:
        a = np.asarray(imgs)
    if a.ndim not in (3, 4):
        raise AssertionError("images should have 3 or 4 dimensions")
    H, W = a.shape[-3:-1]
    a = a[..., margin:H - margin, margin:W - margin, :]
    return [a] if a.ndim == 3 else list(a)


def device_scores(gt, pred, margin: int = 0, data_range: float = 1.0, win_size: int = 7):
    """Per-image ``(mse, ssim)`` of fp32 CUDA tensors (N, C, H, W) or (C, H, W) after cropping ``margin`` border pixels, as
    float64 CUDA tensors of length N: ``psnr`` and ``ssim`` above (``psnr = 10 log10(data_range^2 / mse)``), computed on the
    device in float64 by one HIP kernel and a fixed-order sum (bit-identical run to run), enqueued on the current stream
    without a host sync (graph-capturable)."""
    import torch
    from . import _lib
    if not (isinstance(gt, torch.Tensor) and isinstance(pred, torch.Tensor)):
        raise TypeError("device_scores: gt and pred must be torch tensors")
    if gt.dtype != torch.float32 or pred.dtype != torch.float32:
        raise TypeError(f"device_scores: gt and pred must be float32 tensors, got {gt.dtype} and {pred.dtype}")
    if gt.dim() == 3:
        gt, pred = gt.unsqueeze(0), pred.unsqueeze(0)
    if gt.dim() != 4:
        raise AssertionError("images should have 3 or 4 dimensions")
    margin, win_size = int(margin), int(win_size)
    if margin < 0:
        raise ValueError(f"device_scores: margin={margin} must not be negative")
    if win_size % 2 == 0 or not 3 <= win_size <= 15:
        raise ValueError(f"device_scores: win_size={win_size} must be odd and in [3, 15]")
    if not data_range > 0:
        raise ValueError(f"device_scores: data_range={data_range} must be positive")
    N, C, H, W = gt.shape
    if gt.shape != pred.shape or min(H, W) - 2 * margin < win_size:
        raise ValueError("ssim: images must have the same shape and be at least win_size in both dimensions")
    if not (gt.is_cuda and pred.is_cuda) or gt.device != pred.device:
        raise ValueError("device_scores: gt and pred must be CUDA tensors on one device")
    gt, pred = gt.detach().contiguous(), pred.detach().contiguous()
    lib = _lib.load()
    ws_bytes = lib.rdst_sr_scores_workspace(N, C, H, W, margin, win_size)
    if ws_bytes == 0:
        _lib.check(_lib.EINVAL, "rdst_sr_scores_workspace")
    with torch.cuda.device(gt.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gt.device)
        out = torch.empty(2, N, dtype=torch.float64, device=gt.device)
        _lib.check(lib.rdst_sr_scores(gt.data_ptr(), pred.data_ptr(), N, C, H, W, margin, win_size, float(data_range),
                                      out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws_bytes,
                                      torch.cuda.current_stream().cuda_stream), "rdst_sr_scores")
    return out[0], out[1]


def device_msssim(gt, pred, margin: int = 0, data_range: float = 1.0, levels: int = 5, weights=None, win_size: int = 11,
                  sigma: float = 1.5):
    """Per-image ``msssim`` above of fp32 CUDA tensors (N, C, H, W) or (C, H, W) after cropping ``margin`` border pixels, as a
    float64 CUDA tensor of length N: the value-only call of rdst_msssim_loss (include/rdst_hip_msssim.h), enqueued on the
    current stream without a host sync."""
    import torch
    from . import _lib
    from .loss.msssim import call_msssim_loss, check_size, level_weights
    from .loss.ssim import window_taps
    if not (isinstance(gt, torch.Tensor) and isinstance(pred, torch.Tensor)):
        raise TypeError("device_msssim: gt and pred must be torch tensors")
    if gt.dtype != torch.float32 or pred.dtype != torch.float32:
        raise TypeError(f"device_msssim: gt and pred must be float32 tensors, got {gt.dtype} and {pred.dtype}")
    if gt.dim() == 3:
        gt, pred = gt.unsqueeze(0), pred.unsqueeze(0)
    if gt.dim() != 4:
        raise AssertionError("images should have 3 or 4 dimensions")
    margin = int(margin)
    if margin < 0:
        raise ValueError(f"device_msssim: margin={margin} must not be negative")
    if not data_range > 0:
        raise ValueError(f"device_msssim: data_range={data_range} must be positive")
    if gt.shape != pred.shape:
        raise ValueError("msssim: images must have the same shape")
    w = level_weights(levels, weights)
    taps, cn = window_taps("gaussian", win_size, sigma)
    H, W = gt.shape[-2:]
    check_size("device_msssim", H - 2 * margin, W - 2 * margin, taps.shape[0], w.shape[0])
    if not (gt.is_cuda and pred.is_cuda) or gt.device != pred.device:
        raise ValueError("device_msssim: gt and pred must be CUDA tensors on one device")
    gt = gt.detach()[..., margin:H - margin, margin:W - margin].contiguous()
    pred = pred.detach()[..., margin:H - margin, margin:W - margin].contiguous()
    return call_msssim_loss(_lib.load(), gt, pred, taps, cn, float(data_range), w, False)[1]


def psnr_from_mse(mse: float, data_range: float = 1.0) -> float:
    """``psnr`` above from its mean squared error."""
    if mse == 0:
        return float("inf")
    return float(10.0 * math.log10((data_range ** 2) / mse))


def _as_batch(imgs):
    """A (N, C, H, W) / (C, H, W) tensor or a list of (C, H, W) tensors -> one fp32 (N, C, H, W) tensor."""
    import torch
    if isinstance(imgs, (list, tuple)) and len(imgs) and all(isinstance(t, torch.Tensor) for t in imgs):
        imgs = torch.stack([t.detach() for t in imgs])
    if not isinstance(imgs, torch.Tensor):
        raise TypeError("SRMetrics(device=...): images must be torch tensors or lists of tensors")
    return imgs.detach().float()


class SRMetrics:
    """The pixel metrics of the reference's ``SRMetrics`` that the shipped configs ask for ('psnr ssim',
    config_files/RDST_E1_OASIS_example_SRx4.ini): ``SRMetrics('psnr ssim')(gts, preds, margin)`` -> {'psnr': [...], ...}.
    'msssim' (5 levels, Gaussian window of 11 taps: images of at least 176 pixels after the margin) is scored as well.
    The other metrics of the reference (sewar's, FID) are outside this repository's scope and raise.
    ``device="cuda"``: tensors (a batch or a list of images) are scored on the GPU by ``device_scores`` and ``device_msssim``
    (the ground truth and the predictions are moved there if they are not on it), with one host copy of the 2 N or 3 N
    results per call; anything else raises TypeError.  ``device=None`` (default): the host path above."""

    def __init__(self, metrics: str = "psnr ssim", return_mode: str = "full", device=None):
        self.metrics = metrics.split()
        for m in self.metrics:
            if m not in _FUNCS:
                raise ValueError("Do not support this metric: {}".format(m))
        if return_mode not in ("full", "mean"):
            raise ValueError("return mode must be one of [mean, full]")
        self.return_mode = return_mode
        self.device = None
        if device is not None:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise ValueError(f"SRMetrics: device must be None or a CUDA device, got {device!r}")

    def _device_report(self, gts, preds, margin: int) -> Dict[str, List[float]]:
        import torch
        g, p = _as_batch(gts), _as_batch(preds)
        dev = p.device if p.is_cuda else g.device if g.is_cuda else self.device
        g, p = g.to(dev), p.to(dev)
        rows = []
        if "psnr" in self.metrics or "ssim" in self.metrics:
            rows += list(device_scores(g, p, margin))
        if "msssim" in self.metrics:
            rows.append(device_msssim(g, p, margin))
        host = torch.stack(rows).cpu().tolist()
        rep = {}
        for m in self.metrics:
            rep[m] = [psnr_from_mse(v) for v in host[0]] if m == "psnr" else host[1] if m == "ssim" else host[-1]
        return rep

    def __call__(self, gts, preds, margin: int = 0) -> Dict[str, Union[List[float], float]]:
        if self.device is not None:
            rep = self._device_report(gts, preds, margin)
        else:
            g, p = _to_hwc_list(gts, margin), _to_hwc_list(preds, margin)
            rep = {m: [_FUNCS[m](a, b) for a, b in zip(g, p)] for m in self.metrics}
        if self.return_mode == "mean":
            rep = {m: float(np.mean(v)) for m, v in rep.items()}
        return rep
