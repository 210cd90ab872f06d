"""The LR-consistency loss: ``mean |A(pred) - lr|`` (or its square) under a known degradation ``A``, the "dual regression" /
data-consistency term trained beside L1 (rdst_lrc_residual / rdst_lrc_adjoint, include/rdst_hip_consistency.h carries the
definitions; rdst_amd/csrc/consistency.hip the kernels).

    loss = lr_consistency_loss(pred, lr)                                   # 'cubic', L1
    loss = lr_consistency_loss(pred, lr, degradation='fourier', norm='l2')
    SRLoss(paras) with 'LRC' in paras.training_losses                      # e.g. {'L1': 1, 'LRC': 0.1}

``A`` is ``rdst_amd.data.resample`` (``operator_table``): the degraded prediction has ``resample(pred)``'s bits.  The forward is
one tile launch and one finish launch and keeps the LR-sized unit gradient; the backward is ONE launch, the adjoint of the
operator with the upstream scalar multiplied in its epilogue.  Nothing waits for the device, so the loss captures into the
training step's HIP graph.  The gradient is taken with respect to ``pred`` only and cannot be differentiated again.  There is
no CPU fallback.

``lrc_residual`` / ``lrc_adjoint`` are the two entry points as functions (``SRTester``'s back-projection uses them).  Where an
entry point answers RDST_ENOTSUP (an image too large for its LDS images) they go through ``data.resample`` /
``data.resample_adjoint`` and torch elementwise operations instead, which give the same bits per element.
"""
from __future__ import annotations

import functools
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..data import (Degradation, _device_adjoint_table, _device_op_table, _pair, _stream, operator_table, resample,
                    resample_adjoint)

NORMS = {"l1": 1, "l2": 2}


def _norm_code(norm) -> int:
    code = NORMS.get(norm.lower() if isinstance(norm, str) else norm)
    if code is None:
        raise ValueError(f"lr_consistency_loss: norm={norm!r} must be 'l1' or 'l2'")
    return code


def unit_scales(n: int) -> Tuple[float, float]:
    """``(inv_n, scale)`` of rdst_lrc_residual as the fp32 values it uses: ``(float)(1 / n)`` and ``(float)(2 / n)``."""
    return float(np.float32(1.0 / n)), float(np.float32(2.0 / n))


@functools.lru_cache(maxsize=None)
def _operator_ok(d: Degradation, n_in: int, n_out: int) -> bool:
    """The operator's own refusals ('fourier' only shrinks, ...), once per axis: building a table on the host costs a
    millisecond, which a loss called every step must not pay."""
    operator_table(d, n_in, n_out)
    return True


def _check_pair(who: str, pred: torch.Tensor, lr: torch.Tensor, d: Degradation) -> None:
    if not (isinstance(pred, torch.Tensor) and isinstance(lr, torch.Tensor)):
        raise TypeError(f"{who}: pred and lr must be torch tensors")
    if not (pred.is_cuda and lr.is_cuda):
        raise RuntimeError(f"rdst_amd.loss.{who}: the HIP path needs GPU tensors; there is no CPU fallback")
    if pred.device != lr.device:
        raise ValueError(f"{who}: pred and lr must be on one device")
    if pred.dtype != torch.float32 or lr.dtype != torch.float32:
        raise TypeError(f"{who}: pred and lr must be float32 tensors, got {pred.dtype} and {lr.dtype}")
    if pred.dim() != 4 or lr.dim() != 4 or pred.shape[:2] != lr.shape[:2] or min(pred.shape) <= 0 or min(lr.shape) <= 0:
        raise ValueError(f"{who}: pred (N, C, H, W) and lr (N, C, oh, ow) must share N and C and be non-empty, got "
                         f"{tuple(pred.shape)} and {tuple(lr.shape)}")
    for n_in, n_out in zip(pred.shape[-2:], lr.shape[-2:]):
        _operator_ok(d, int(n_in), int(n_out))


def lrc_residual(pred: torch.Tensor, lr: torch.Tensor, degradation: Union[str, Degradation] = "cubic", norm: Optional[str] = None,
                 want_resid: bool = True, want_g: bool = False, want_loss: bool = False):
    """rdst_lrc_residual: ``(resid, g, loss)`` of fp32 CUDA ``pred`` (N, C, H, W) against ``lr`` (N, C, oh, ow), ``None`` for
    what was not asked for.  ``resid = resample(pred) - lr``; with ``norm`` 'l1' / 'l2', ``g`` is the gradient of the mean of
    ``|resid|`` / ``resid^2`` with respect to the degraded prediction and ``loss`` that mean (0-dim fp32).  Not differentiable."""
    d = Degradation.of(degradation)
    _check_pair("lrc_residual", pred, lr, d)
    code = 0 if norm is None else _norm_code(norm)
    if code == 0 and (want_g or want_loss):
        raise ValueError("lrc_residual: g and loss need a norm ('l1' or 'l2')")
    if not (want_resid or want_g or want_loss):
        raise ValueError("lrc_residual: nothing asked for")
    p, t = pred.detach().contiguous(), lr.detach().contiguous()
    N, C, H, W = p.shape
    oh, ow = t.shape[-2:]
    lib = _lib.load()
    with torch.cuda.device(p.device):
        iy, wy = _device_op_table(d, H, oh, p.device)
        ix, wx = _device_op_table(d, W, ow, p.device)
        resid = torch.empty_like(t) if want_resid else None
        g = torch.empty_like(t) if want_g else None
        loss = torch.empty((), dtype=torch.float32, device=p.device) if want_loss else None
        ws_bytes = lib.rdst_lrc_workspace(N, C, oh, ow) if want_loss else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device) if want_loss else None
        ptr = lambda x: None if x is None else x.data_ptr()     # noqa: E731
        rc = lib.rdst_lrc_residual(p.data_ptr(), t.data_ptr(), N, C, H, W, oh, ow, iy.shape[1], iy.data_ptr(), wy.data_ptr(),
                                   ix.shape[1], ix.data_ptr(), wx.data_ptr(), code, ptr(resid), ptr(g), ptr(loss), ptr(ws),
                                   ws_bytes, _stream())
        if rc == _lib.ENOTSUP:
            return _residual_composed(p, t, d, code, want_resid, want_g, want_loss)
        _lib.check(rc, "rdst_lrc_residual")
    return resid, g, loss


def _residual_composed(p, t, d, code, want_resid=True, want_g=True, want_loss=True):
    """``lrc_residual`` through ``resample`` and torch elementwise operations: the same bits per element (one rounding each);
    the loss is summed in float64 in torch's order."""
    R = resample(p, t.shape[-2:], d) - t
    n = R.numel()
    inv_n, scale = unit_scales(n)
    g = loss = None
    if want_g:
        g = torch.where(R == 0, torch.zeros_like(R), torch.copysign(torch.full_like(R, inv_n), R)) if code == 1 else R * scale
    if want_loss:
        Rd = R.double()
        loss = ((Rd.abs() if code == 1 else Rd * Rd).sum() / n).float()
    return (R if want_resid else None), g, loss


def lrc_adjoint(g: torch.Tensor, size, degradation: Union[str, Degradation] = "cubic", scale: float = 1.0,
                scale_dev: Optional[torch.Tensor] = None, base: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rdst_lrc_adjoint: ``s * resample_adjoint(g, size)`` (+ ``base``) with ``s = scale`` (times the fp32 device scalar
    ``scale_dev``), one rounding per element (an fma with ``base``).  ``out`` may be ``base``.  Not differentiable."""
    d = Degradation.of(degradation)
    H, W = _pair(size)
    if not isinstance(g, torch.Tensor) or g.dim() != 4 or min(g.shape) <= 0:
        raise ValueError("lrc_adjoint: g must be a non-empty (N, C, oh, ow) tensor")
    if not g.is_cuda:
        raise RuntimeError("rdst_amd.loss.lrc_adjoint: the HIP path needs GPU tensors; there is no CPU fallback")
    N, C, oh, ow = g.shape
    for what, x, shape in (("g", g, tuple(g.shape)), ("scale_dev", scale_dev, ()), ("base", base, (N, C, H, W)),
                           ("out", out, (N, C, H, W))):
        if x is None:
            continue
        if x.dtype != torch.float32 or x.device != g.device or tuple(x.shape) != shape:
            raise ValueError(f"lrc_adjoint: {what} must be a float32 tensor of shape {shape} on {g.device}")
        if what in ("base", "out") and not x.is_contiguous():
            raise ValueError(f"lrc_adjoint: {what} must be contiguous")
    _operator_ok(d, H, int(oh)), _operator_ok(d, W, int(ow))
    g = g.detach().contiguous()
    lib = _lib.load()
    with torch.cuda.device(g.device):
        iy, wy = _device_adjoint_table(d, H, oh, g.device)
        ix, wx = _device_adjoint_table(d, W, ow, g.device)
        if out is None:
            out = torch.empty(N, C, H, W, dtype=torch.float32, device=g.device)
        rc = lib.rdst_lrc_adjoint(g.data_ptr(), N, C, oh, ow, H, W, iy.shape[1], iy.data_ptr(), wy.data_ptr(), ix.shape[1],
                                  ix.data_ptr(), wx.data_ptr(), None if scale_dev is None else scale_dev.data_ptr(),
                                  float(scale), None if base is None else base.data_ptr(), out.data_ptr(), _stream())
        if rc == _lib.ENOTSUP:
            a = resample_adjoint(g, (H, W), d)
            s = torch.full((), float(scale), dtype=torch.float32, device=g.device)
            if scale_dev is not None:
                s = s * scale_dev
            out.copy_(s * a if base is None else torch.addcmul(base, s, a))
            return out
        _lib.check(rc, "rdst_lrc_adjoint")
    return out


def warm_tables(degradation: Union[str, Degradation], hr_size, lr_size, device) -> None:
    """Put the four device tables of a shape pair into their caches (an upload must not happen inside a graph capture)."""
    d, device = Degradation.of(degradation), torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    for n_in, n_out in zip(_pair(hr_size), _pair(lr_size)):
        _device_op_table(d, n_in, n_out, device)
        _device_adjoint_table(d, n_in, n_out, device)


class _LRCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, lr, d, norm):
        need_grad = bool(ctx.needs_input_grad[0])
        _, g, loss = lrc_residual(pred, lr, d, norm, want_resid=False, want_g=need_grad, want_loss=True)
        if need_grad:
            ctx.save_for_backward(g)
        ctx.hw, ctx.d = tuple(pred.shape[-2:]), d
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        g, = ctx.saved_tensors
        s = grad_loss if grad_loss.dtype == torch.float32 and grad_loss.device == g.device else grad_loss.to(g.device, torch.float32)
        return lrc_adjoint(g, ctx.hw, ctx.d, 1.0, scale_dev=s.contiguous()), None, None, None


def lr_consistency_loss(pred: torch.Tensor, lr: torch.Tensor, degradation: Union[str, Degradation] = "cubic",
                        norm: str = "l1") -> torch.Tensor:
    """``mean |resample(pred, lr.shape[-2:], degradation) - lr|`` ('l1') or the mean of its square ('l2') of fp32 CUDA tensors
    ``pred`` (N, C, H, W) and ``lr`` (N, C, oh, ow) as a 0-dim fp32 tensor, differentiable with respect to ``pred``."""
    d = Degradation.of(degradation)
    _norm_code(norm)
    _check_pair("lr_consistency_loss", pred, lr, d)
    if lr.requires_grad:
        raise ValueError("lr_consistency_loss: the gradient with respect to lr is not computed; detach it")
    return _LRCLoss.apply(pred, lr, d, norm)


class LRConsistencyLoss(object):
    """The 'LRC' component of ``SRLoss``, shaped like ``RecLoss``: ``__call__(rec, gt) -> (loss, {'Rec_LRC': loss})`` against
    ``target(gt) = resample(gt, (H // scale, W // scale), degradation)``: for a batch of ``DevicePatchSampler`` under the same
    degradation that is ``batch['in']`` bit for bit.  ``rec`` must have ``gt``'s shape."""

    def __init__(self, degradation: Union[str, Degradation] = "cubic", scale: float = 4, norm: str = "l1"):
        self.degradation = Degradation.of(degradation)
        if float(scale) != int(scale) or int(scale) < 1:
            raise ValueError(f"LRConsistencyLoss: scale={scale!r} must be a positive integer")
        self.scale = int(scale)
        _norm_code(norm)
        self.norm = norm.lower()
        self.loss_names = ["Rec_LRC"]

    def target(self, gt: torch.Tensor) -> torch.Tensor:
        """The LR image the loss compares the degraded reconstruction with."""
        if not isinstance(gt, torch.Tensor) or gt.dim() != 4:
            raise ValueError("LRConsistencyLoss: gt must be a (N, C, H, W) tensor")
        H, W = gt.shape[-2:]
        s = self.scale
        if H % s or W % s or H < s or W < s:
            raise ValueError(f"LRConsistencyLoss: gt is {H} x {W}, not a multiple of the scale {s}")
        if gt.is_cuda:
            warm_tables(self.degradation, (H, W), (H // s, W // s), gt.device)
        return resample(gt.detach(), (H // s, W // s), self.degradation)

    def __call__(self, rec, gt):
        from .sr_loss import LazyScalars
        if isinstance(rec, torch.Tensor) and isinstance(gt, torch.Tensor) and rec.shape != gt.shape:
            raise ValueError(f"LRConsistencyLoss: rec {tuple(rec.shape)} and gt {tuple(gt.shape)} must have one shape")
        loss = lr_consistency_loss(rec, self.target(gt), self.degradation, self.norm)
        return loss, LazyScalars({self.loss_names[0]: loss.detach()})
