"""The multi-scale SSIM training loss: ``loss = 1 - mean_n MS-SSIM(pred_n, target_n)`` (Wang, Simoncelli & Bovik 2003; the
SSIM term of Zhao et al.'s L1 + MS-SSIM mix), value and gradient on the HIP SSIM path (rdst_msssim_loss,
include/rdst_hip_msssim.h carries the definition; rdst_amd/csrc/msssim_loss.hip the kernels).

    loss = ms_ssim_loss(pred, target)                                   # 5 levels, 11-tap Gaussian, the published weights
    loss = ms_ssim_loss(pred, target, levels=4)                         # 96-pixel patches: the first 4 weights, renormalised
    loss, per_image = ms_ssim_loss(pred, target, return_msssim=True)    # + the fp64 MS-SSIM of every image
    SRLoss(paras) with 'MSSSIM' in paras.training_losses                # e.g. {'L1': 0.16, 'MSSSIM': 0.84}

Level j+1 is level j averaged 2x2 in fp32 (floor sizes: a trailing odd row or column is dropped); every level but the last
contributes the mean of the contrast-structure term, the last the mean of SSIM; a plane with a non-positive level mean scores
exactly 0 and has an exactly zero gradient.  The images must hold ``win << (levels - 1)`` pixels on their least side: the
levels are never reduced silently.  Window sums run in fp64 on the device, nothing syncs with the host (the loss captures into
the training step's HIP graph), the gradient is taken with respect to ``pred`` only and cannot be differentiated again.
There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .ssim import window_taps

# Wang, Simoncelli & Bovik, "Multi-scale structural similarity for image quality assessment" (2003), section 3.2
PUBLISHED_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_LEVELS = len(PUBLISHED_WEIGHTS)


def level_weights(levels: int = MAX_LEVELS, weights: Optional[Sequence[float]] = None) -> np.ndarray:
    """The float64 exponents of ``levels`` levels: ``weights`` as given (finite and > 0, one per level), else the published
    five as they are, or the first ``levels`` of them divided by their sum."""
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"ms_ssim: levels={levels} must be in [1, {MAX_LEVELS}]")
    if weights is None:
        w = np.asarray(PUBLISHED_WEIGHTS[:levels], dtype=np.float64)
        return w if levels == MAX_LEVELS else w / w.sum()
    w = np.array([float(v) for v in weights], dtype=np.float64)
    if w.shape != (levels,):
        raise ValueError(f"ms_ssim: {w.size} weights for levels={levels}")
    if not all(math.isfinite(v) and v > 0 for v in w):
        raise ValueError(f"ms_ssim: the weights {w.tolist()} must be finite and positive")
    return w


def check_size(who: str, H: int, W: int, win: int, levels: int) -> None:
    """Raise when (H, W) does not hold ``levels`` levels of a ``win``-tap window."""
    if (min(H, W) >> (levels - 1)) < win:
        raise ValueError(f"{who}: the images ({H} x {W}) are too small for levels={levels} at win_size={win}: the least "
                         f"side is win << (levels-1) = {win << (levels - 1)}; ask for fewer levels or a smaller window")


def call_msssim_loss(lib, t, p, taps, cov_norm, data_range, weights, need_grad):
    """rdst_msssim_loss on contiguous fp32 device tensors: (loss, msssim, means, grad or None)."""
    N, C, H, W = p.shape
    win, levels = int(taps.shape[0]), int(weights.shape[0])
    ws_bytes = lib.rdst_msssim_loss_workspace(N, C, H, W, win, levels, int(need_grad))
    if ws_bytes == 0:
        _lib.check(_lib.EINVAL, "rdst_msssim_loss_workspace")
    with torch.cuda.device(p.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
        msssim = torch.empty(N, dtype=torch.float64, device=p.device)
        means = torch.empty(N * C, levels, dtype=torch.float64, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p) if need_grad else None
        _lib.check(lib.rdst_msssim_loss(t.data_ptr(), p.data_ptr(), N, C, H, W, win, taps.ctypes.data, float(cov_norm),
                                        float(data_range), levels, weights.ctypes.data, msssim.data_ptr(), means.data_ptr(),
                                        loss.data_ptr(), grad.data_ptr() if need_grad else None, ws.data_ptr(), ws_bytes,
                                        torch.cuda.current_stream().cuda_stream), "rdst_msssim_loss")
    return loss, msssim, means, grad


class _MSSSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, taps, cov_norm, data_range, weights):
        need_grad = bool(ctx.needs_input_grad[0])
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        loss, msssim, _, grad = call_msssim_loss(_lib.load(), t, p, taps, cov_norm, data_range, weights, need_grad)
        if need_grad:
            ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(msssim)
        return loss, msssim

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_msssim):
        grad, = ctx.saved_tensors
        return grad_loss * grad, None, None, None, None, None


def ms_ssim_loss(pred: torch.Tensor, target: torch.Tensor, levels: int = MAX_LEVELS, weights: Optional[Sequence[float]] = None,
                 window: str = "gaussian", win_size: Optional[int] = None, sigma: float = 1.5, data_range: float = 1.0,
                 return_msssim: bool = False):
    """``1 - mean_n MS-SSIM(pred_n, target_n)`` of fp32 CUDA tensors (N, C, H, W) as a 0-dim fp32 tensor, differentiable with
    respect to ``pred``; with ``return_msssim=True`` also the per-image MS-SSIM (float64, length N, not differentiable)."""
    if not (isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor)):
        raise TypeError("ms_ssim_loss: pred and target must be torch tensors")
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("rdst_amd.loss.ms_ssim_loss: the HIP path needs GPU tensors; there is no CPU fallback")
    if pred.device != target.device:
        raise ValueError("ms_ssim_loss: pred and target must be on one device")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"ms_ssim_loss: pred and target must be float32 tensors, got {pred.dtype} and {target.dtype}")
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"ms_ssim_loss: pred and target must share one (N, C, H, W) shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if target.requires_grad:
        raise ValueError("ms_ssim_loss: the gradient with respect to the target is not computed; detach it")
    if not data_range > 0:
        raise ValueError(f"ms_ssim_loss: data_range={data_range} must be positive")
    w = level_weights(levels, weights)
    taps, cov_norm = window_taps(window, win_size, sigma)
    check_size("ms_ssim_loss", int(pred.shape[-2]), int(pred.shape[-1]), int(taps.shape[0]), int(w.shape[0]))
    loss, msssim = _MSSSIMLoss.apply(pred, target, taps, cov_norm, float(data_range), w)
    return (loss, msssim) if return_msssim else loss


class MSSSIMLoss(object):
    """The 'MSSSIM' component of ``SRLoss``, shaped like ``RecLoss``: ``__call__(rec, gt) -> (loss, {'Rec_MSSSIM': loss})``."""

    def __init__(self, levels: int = MAX_LEVELS, weights: Optional[Sequence[float]] = None, window: str = "gaussian",
                 win_size: Optional[int] = None, sigma: float = 1.5, data_range: float = 1.0):
        level_weights(levels, weights)                 # refuse bad levels, weights or windows when the loss is built
        window_taps(window, win_size, sigma)
        if not data_range > 0:
            raise ValueError(f"MSSSIMLoss: data_range={data_range} must be positive")
        self.levels, self.weights = int(levels), None if weights is None else tuple(float(v) for v in weights)
        self.window, self.win_size, self.sigma, self.data_range = window, win_size, float(sigma), float(data_range)
        self.loss_names = ["Rec_MSSSIM"]

    def __call__(self, rec, gt):
        from .sr_loss import LazyScalars
        loss = ms_ssim_loss(rec, gt, self.levels, self.weights, self.window, self.win_size, self.sigma, self.data_range)
        return loss, LazyScalars({self.loss_names[0]: loss.detach()})
