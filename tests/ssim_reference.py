"""The float64 reference of the SSIM training loss (include/rdst_hip.h, rdst_ssim_loss), shared by test_ssim_loss_host.py
and test_ssim_loss_gpu.py: per-channel valid ``conv2d`` with the outer product of the taps in float64 and torch autograd on
a float64 copy of the fp32 inputs.  Nothing here touches the code under test; the taps are written out again."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def taps_of(window, win, sigma=1.5):
    """(float64 taps, cov_norm): 'u' = uniform with the sample covariance, 'g' = Gaussian of `sigma` with cov_norm 1."""
    if window == "u":
        return np.full(win, 1.0 / win), win * win / (win * win - 1.0)
    k = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-k * k / (2.0 * sigma * sigma))
    return w / w.sum(), 1.0


def images(shape, seed, dr=1.0):
    """tests/test_srmetrics_gpu.py::_images."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = (dr * rng.random(shape)).astype(np.float32)
    p = np.clip(g + 0.1 * dr * rng.standard_normal(shape), 0, dr).astype(np.float32)
    return torch.from_numpy(g), torch.from_numpy(p)


def _weight(taps, C):
    t = torch.from_numpy(np.asarray(taps, dtype=np.float64))
    return torch.outer(t, t)[None, None].repeat(C, 1, 1, 1)


def terms(X, Y, taps, cn, dr):
    """Float64 (N, C, Ho, Wo) maps ux, uy, A1, A2, B1, B2, S of float64 X (target) and Y (prediction)."""
    C = X.shape[1]
    w = _weight(taps, C)
    f = lambda t: F.conv2d(t, w, groups=C)
    ux, uy, uxx, uyy, uxy = f(X), f(Y), f(X * X), f(Y * Y), f(X * Y)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux * ux + uy * uy + C1, vx + vy + C2
    return ux, uy, A1, A2, B1, B2, A1 * A2 / (B1 * B2)


def reference(target, pred, taps, cn, dr):
    """(ssim (N,), loss, dloss/dpred) in float64 by autograd, from fp32 (or float64) target / pred."""
    X = target.detach().double()
    Y = pred.detach().double().clone().requires_grad_(True)
    S = terms(X, Y, taps, cn, dr)[-1]
    ssim = S.mean(dim=(1, 2, 3))
    loss = 1.0 - ssim.mean()
    loss.backward()
    return ssim.detach(), loss.detach(), Y.grad


def closed_form_grad(target, pred, taps, cn, dr):
    """The gradient written out (the comment on rdst_ssim_loss): the adjoint of the window sums applied to a, b, c."""
    X, Y = target.detach().double(), pred.detach().double()
    ux, uy, A1, A2, B1, B2, S = terms(X, Y, taps, cn, dr)
    a = 2 * ux * A2 / (B1 * B2) - 2 * uy * S / B1 - 2 * cn * ux * A1 / (B1 * B2) + 2 * cn * uy * S / B2
    b = -cn * S / B2
    c = 2 * cn * A1 / (B1 * B2)
    C = X.shape[1]
    w = _weight(taps, C)
    ft = lambda t: F.conv_transpose2d(t, w, groups=C)
    return -(ft(a) + 2 * Y * ft(b) + X * ft(c)) / S.numel()


@functools.lru_cache(maxsize=None)
def case(N, C, H, W, window, win, dr, kind="random"):
    """One seeded test case with its reference, computed once: dict(target, pred, taps, cn, ssim, loss, grad).
    kind 'slice': a zero background in the target (rows 0..11 and columns 50..); 'range': a prediction that leaves [0, 1],
    clipped to [-0.1, 1.1]."""
    taps, cn = taps_of(window, win)
    g, p = images((N, C, H, W), 17 + H * W + C, dr)
    if kind == "slice":
        g[..., :12, :] = 0
        g[..., :, 50:] = 0
    elif kind == "range":
        rng = np.random.Generator(np.random.PCG64(99))
        p = torch.from_numpy(np.clip(g.numpy() + 0.3 * rng.standard_normal(g.shape), -0.1, 1.1).astype(np.float32))
    elif kind != "random":
        raise ValueError(kind)
    ssim, loss, grad = reference(g, p, taps, cn, dr)
    return dict(target=g, pred=p, taps=taps, cn=cn, ssim=ssim, loss=loss, grad=grad)
