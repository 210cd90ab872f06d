"""The float64 reference of the MS-SSIM loss (include/rdst_hip_msssim.h, rdst_msssim_loss), shared by test_msssim_host.py and
test_msssim_loss_gpu.py.  The window maps are ssim_reference.terms; the levels are pooled in fp32 by the spelled-out slices; the
prediction's pyramid is carried as ``Yp + (y32.double() - Yp).detach()`` with ``Yp = avg_pool2d`` in float64, so its VALUE is the
fp32 level and its GRADIENT the exact average (straight through the rounding).  Nothing here touches the code under test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ssim_reference import images, taps_of, terms

PUBLISHED = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # Wang, Simoncelli & Bovik 2003


def default_weights(levels):
    w = np.asarray(PUBLISHED[:levels], dtype=np.float64)
    return w if levels == 5 else w / w.sum()


def pool32(x):
    """fp32 (..., H, W) -> fp32 (..., H // 2, W // 2): ((a + b) + (c + d)) * 0.25, a trailing odd row or column dropped."""
    assert x.dtype == torch.float32
    H2, W2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., :2 * H2, :2 * W2]
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * 0.25


def pyramid(target, pred, levels):
    """[(X_j float64, Y_j float64 with the straight-through graph to pred's float64 leaf, y32_j)], and the leaf."""
    x32, y32 = target.detach().float(), pred.detach().float()
    leaf = y32.double().clone().requires_grad_(True)
    out = [(x32.double(), leaf, y32)]
    Y = leaf
    for _ in range(1, levels):
        x32, y32 = pool32(x32), pool32(y32)
        Yp = F.avg_pool2d(Y, 2)
        Y = Yp + (y32.double() - Yp).detach()
        out.append((x32.double(), Y, y32))
    return out, leaf


def level_mean(X, Y, taps, cn, dr, last):
    """(N, C) mean over the valid positions of S (last) or cs = A2 / B2."""
    _, _, _, A2, _, B2, S = terms(X, Y, taps, cn, dr)
    return (S if last else A2 / B2).mean(dim=(2, 3))


def combine(m, beta):
    """m (N, C, M) -> MS (N, C), exactly 0 (and constant) where some level mean is not positive; k (N, C, M) detached."""
    N, C, _ = m.shape
    b = torch.from_numpy(np.asarray(beta, dtype=np.float64))
    ok = (m > 0).all(dim=-1)
    safe = torch.where(ok[..., None], m, torch.ones_like(m))
    MS = torch.where(ok, (safe ** b).prod(dim=-1), torch.zeros_like(ok, dtype=torch.float64))
    k = torch.where(ok[..., None], -MS[..., None] * b / (safe * N * C), torch.zeros_like(m)).detach()
    return MS, k


def reference(target, pred, taps, cn, dr, weights):
    """dict(msssim (N,), means (N, C, M), loss, grad, terms [t_1 .. t_M] with sum_j t_j == grad, k (N, C, M)), float64."""
    M = len(weights)
    pyr, leaf = pyramid(target, pred, M)
    m = torch.stack([level_mean(X, Y, taps, cn, dr, j == M - 1) for j, (X, Y, _) in enumerate(pyr)], dim=-1)
    MS, k = combine(m, weights)
    msssim = MS.mean(dim=1)
    loss = 1.0 - msssim.mean()
    t = [torch.autograd.grad((k[..., j] * m[..., j]).sum(), leaf, retain_graph=True)[0] for j in range(M)]
    grad, = torch.autograd.grad(loss, leaf, allow_unused=True)
    if grad is None:                                  # every plane clamped
        grad = torch.zeros_like(leaf)
    return dict(msssim=msssim.detach(), means=m.detach(), loss=loss.detach(), grad=grad, terms=t, k=k)


def closed_form_level_grad(X, Y, taps, cn, dr, last):
    """d mean_positions(term) / d Y per plane, written out: the adjoint of the window sums applied to a, b, c (S, the comment on
    rdst_ssim_loss) or a', b', c' (cs, include/rdst_hip_msssim.h)."""
    ux, uy, A1, A2, B1, B2, S = terms(X, Y, taps, cn, dr)
    if last:
        a = 2 * ux * A2 / (B1 * B2) - 2 * uy * S / B1 - 2 * cn * ux * A1 / (B1 * B2) + 2 * cn * uy * S / B2
        b = -cn * S / B2
        c = 2 * cn * A1 / (B1 * B2)
    else:
        cs = A2 / B2
        a = 2 * cn * (cs * uy - ux) / B2
        b = -cn * cs / B2
        c = 2 * cn / B2
    C = X.shape[1]
    t = torch.from_numpy(np.asarray(taps, dtype=np.float64))
    w = torch.outer(t, t)[None, None].repeat(C, 1, 1, 1)
    ft = lambda v: F.conv_transpose2d(v, w, groups=C)
    return (ft(a) + 2 * Y * ft(b) + X * ft(c)) / (S.shape[2] * S.shape[3])


def upsample_quarter(acc, H, W, quarter=0.25, clamp=False):
    """The coarse term at a level of H x W: quarter * acc[r // 2][c // 2], zero on a dropped row or column (``clamp``: the
    mutation that reads the last coarse row / column there instead)."""
    up = acc.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1) * quarter
    out = torch.zeros(*acc.shape[:-2], H, W, dtype=acc.dtype)
    out[..., :up.shape[-2], :up.shape[-1]] = up
    if clamp:
        if H > up.shape[-2]:
            out[..., up.shape[-2]:, :up.shape[-1]] = up[..., -1:, :]
        if W > up.shape[-1]:
            out[..., :, up.shape[-1]:] = out[..., :, up.shape[-1] - 1:up.shape[-1]]
    return out


def composed_grad(target, pred, taps, cn, dr, weights, mutation=None):
    """The gradient as the kernels form it, in float64 without their roundings: acc_M = k_M g_M, acc_j = k_j g_j + 0.25
    acc_{j+1}[r // 2][c // 2], grad = acc_1.  ``mutation`` builds a WRONG gradient for the tests of the gate:
    'no_quarter', 'clamp_dropped', 'weight_shift' (level 2's weight at level 3), 's_at_level_1'."""
    M = len(weights)
    pyr, _ = pyramid(target, pred, M)
    lv = [(X, Y.detach()) for X, Y, _ in pyr]
    m = torch.stack([level_mean(X, Y, taps, cn, dr, j == M - 1) for j, (X, Y) in enumerate(lv)], dim=-1)
    _, k = combine(m, weights)
    if mutation == "weight_shift":
        assert M >= 3
        k = k.clone()
        k[..., 2] *= weights[1] / weights[2]
    acc = None
    for j in range(M - 1, -1, -1):
        X, Y = lv[j]
        last = j == M - 1 or (mutation == "s_at_level_1" and j == 0)
        g = k[..., j, None, None] * closed_form_level_grad(X, Y, taps, cn, dr, last)
        if acc is not None:
            g = g + upsample_quarter(acc, X.shape[-2], X.shape[-1], 1.0 if mutation == "no_quarter" else 0.25,
                                     mutation == "clamp_dropped")
        acc = g
    return acc


def gate_excess(got, ref, roundings, scale=1.0):
    """max over the elements of |got - scale g64| - tol,  tol = roundings * 2^-24 * scale * sum_j |t_j| + 1e-10 max|scale g64|:
    <= 0 passes.  At most one fp32 rounding of the running sum per level, each relative to a partial sum that sum_j |t_j| bounds."""
    want = scale * ref["grad"]
    bound = scale * sum(t.abs() for t in ref["terms"])
    tol = roundings * 2.0 ** -24 * bound + 1e-10 * want.abs().max()
    err = (got.detach().double().cpu() - want).abs()
    return float((err - tol).max()), float(err.max())


CASES = [
    # (N, C, H, W, window, win, levels)
    (2, 1, 40, 48, "g", 5, 3),        # six tiles
    (1, 2, 24, 28, "u", 3, 3),        # per-plane products, then the channel mean; last level 6 x 7
    (1, 1, 37, 43, "g", 5, 3),        # odd sides at two levels
    (2, 1, 44, 52, "g", 11, 3),       # last level 11 x 13: one row of three window positions
    (1, 1, 176, 192, "g", 11, 5),     # the smallest image of the published configuration
    (2, 1, 96, 96, "g", 11, 4),
    (1, 1, 48, 80, "u", 3, 5),
]


def case_id(c):
    return "N{}C{}_{}x{}_{}{}_L{}".format(*c)


@functools.lru_cache(maxsize=None)
def case(N, C, H, W, window, win, levels, weights=None):
    """One seeded case with its reference, computed once: ssim_reference.images(shape, 17)."""
    taps, cn = taps_of(window, win)
    g, p = images((N, C, H, W), 17)
    w = default_weights(levels) if weights is None else np.asarray(weights, dtype=np.float64)
    ref = reference(g, p, taps, cn, 1.0, w)
    return dict(target=g, pred=p, taps=taps, cn=cn, weights=w, **ref)
