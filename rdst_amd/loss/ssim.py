"""The SSIM training loss: ``loss = 1 - mean_n SSIM(pred_n, target_n)``, value and gradient from ONE HIP kernel
(rdst_ssim_loss, include/rdst_hip.h carries the definition; rdst_amd/csrc/ssim_loss.hip the kernel).

    loss = ssim_loss(pred, target)                                   # 7x7 uniform window: metrics.ssim at margin 0
    loss = ssim_loss(pred, target, window='gaussian')                # 11 taps, sigma 1.5 (Wang et al. 2004)
    loss, per_image = ssim_loss(pred, target, return_ssim=True)      # + the fp64 SSIM of every image, not differentiable
    SRLoss(paras) with 'SSIM' in paras.training_losses               # e.g. {'L1': 0.16, 'SSIM': 0.84}

The window sums run in fp64 on the device and every gradient element is rounded to fp32 once; the forward enqueues the
kernel on the current stream without a host sync, so the loss captures into the training step's HIP graph.  The gradient is
taken with respect to ``pred`` only and cannot be differentiated again.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib

_DEFAULT_WIN = {"uniform": 7, "gaussian": 11}


def window_taps(window: str = "uniform", win_size: Optional[int] = None, sigma: float = 1.5) -> Tuple[np.ndarray, float]:
    """``(taps, cov_norm)`` of a 1-D window; the 2-D weight is ``taps[k] * taps[l]``.
    'uniform':  ``1 / win`` (default win 7) with the sample covariance ``win^2 / (win^2 - 1)`` — scikit-image's SSIM;
    'gaussian': ``exp(-(k - (win-1)/2)^2 / (2 sigma^2))`` normalised in float64 (default win 11), ``cov_norm = 1``."""
    if window not in _DEFAULT_WIN:
        raise ValueError(f"window_taps: window={window!r} must be 'uniform' or 'gaussian'")
    win = _DEFAULT_WIN[window] if win_size is None else int(win_size)
    if win % 2 == 0 or not 3 <= win <= 15:
        raise ValueError(f"window_taps: win_size={win} must be odd and in [3, 15]")
    if window == "uniform":
        return np.full(win, 1.0 / win, dtype=np.float64), float(win * win) / float(win * win - 1)
    if not sigma > 0:
        raise ValueError(f"window_taps: sigma={sigma} must be positive")
    k = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return w / w.sum(), 1.0


class _SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, taps, cov_norm, data_range):
        N, C, H, W = pred.shape
        win = int(taps.shape[0])
        lib = _lib.load()
        ws_bytes = lib.rdst_ssim_loss_workspace(N, C, H, W, win)
        if ws_bytes == 0:
            _lib.check(_lib.EINVAL, "rdst_ssim_loss_workspace")
        need_grad = bool(ctx.needs_input_grad[0])
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        with torch.cuda.device(pred.device):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pred.device)
            ssim = torch.empty(N, dtype=torch.float64, device=pred.device)
            loss = torch.empty((), dtype=torch.float32, device=pred.device)
            grad = torch.empty_like(p) if need_grad else None
            _lib.check(lib.rdst_ssim_loss(t.data_ptr(), p.data_ptr(), N, C, H, W, win, taps.ctypes.data, float(cov_norm),
                                          float(data_range), ssim.data_ptr(), loss.data_ptr(),
                                          grad.data_ptr() if need_grad else None, ws.data_ptr(), ws_bytes,
                                          torch.cuda.current_stream().cuda_stream), "rdst_ssim_loss")
        if need_grad:
            ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(ssim)
        return loss, ssim

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_ssim):
        grad, = ctx.saved_tensors
        return grad_loss * grad, None, None, None, None


def ssim_loss(pred: torch.Tensor, target: torch.Tensor, window: str = "uniform", win_size: Optional[int] = None,
              sigma: float = 1.5, data_range: float = 1.0, return_ssim: bool = False):
    """``1 - mean_n SSIM(pred_n, target_n)`` of fp32 CUDA tensors (N, C, H, W) as a 0-dim fp32 tensor, differentiable with
    respect to ``pred``; with ``return_ssim=True`` also the per-image SSIM (float64, length N, not differentiable)."""
    if not (isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor)):
        raise TypeError("ssim_loss: pred and target must be torch tensors")
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("rdst_amd.loss.ssim_loss: the HIP path needs GPU tensors; there is no CPU fallback")
    if pred.device != target.device:
        raise ValueError("ssim_loss: pred and target must be on one device")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"ssim_loss: pred and target must be float32 tensors, got {pred.dtype} and {target.dtype}")
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"ssim_loss: pred and target must share one (N, C, H, W) shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if target.requires_grad:
        raise ValueError("ssim_loss: the gradient with respect to the target is not computed; detach it")
    if not data_range > 0:
        raise ValueError(f"ssim_loss: data_range={data_range} must be positive")
    taps, cov_norm = window_taps(window, win_size, sigma)
    if min(pred.shape[-2:]) < taps.shape[0]:
        raise ValueError(f"ssim_loss: the images ({pred.shape[-2]} x {pred.shape[-1]}) are smaller than the window "
                         f"({taps.shape[0]})")
    loss, ssim = _SSIMLoss.apply(pred, target, taps, cov_norm, float(data_range))
    return (loss, ssim) if return_ssim else loss


class SSIMLoss(object):
    """The 'SSIM' component of ``SRLoss``, shaped like ``RecLoss``: ``__call__(rec, gt) -> (loss, {'Rec_SSIM': loss})``."""

    def __init__(self, window: str = "uniform", win_size: Optional[int] = None, sigma: float = 1.5, data_range: float = 1.0):
        window_taps(window, win_size, sigma)           # refuse a bad window when the loss is built, not at the first step
        if not data_range > 0:
            raise ValueError(f"SSIMLoss: data_range={data_range} must be positive")
        self.window, self.win_size, self.sigma, self.data_range = window, win_size, float(sigma), float(data_range)
        self.loss_names = ["Rec_SSIM"]

    def __call__(self, rec, gt):
        from .sr_loss import LazyScalars
        loss = ssim_loss(rec, gt, self.window, self.win_size, self.sigma, self.data_range)
        return loss, LazyScalars({self.loss_names[0]: loss.detach()})
