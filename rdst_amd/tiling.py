"""Slices of any size cut into fixed-size overlapping tiles and put back together, on the device: the reference's
``ImageFolder`` / ``UnFolder`` / ``Folder`` (datasets/basic_dataset.py:347-449, wired up per scale in
datasets/OASIS_dataset.py:246-271) around two HIP copy kernels (rdst_unfold_tiles / rdst_fold_tiles, include/rdst_hip.h).

The reference unfolds an LR slice with ``nn.Unfold``, runs the network on the patches and folds the SR patches with ``nn.Fold``,
the overlaps averaged by a precomputed reciprocal divisor image.  Here:

  * ``TilePlan(H, W, patch, stride, scale, pad_mode)``   the arithmetic of the plan, on the host;
  * ``unfold_tiles(x, plan)``                            (N, C, H, W) -> (N Ly Lx, C, p, p), one launch, a pure copy;
  * ``fold_tiles(tiles, plan, N)``                       (N Ly Lx, C, P, P) -> (N, C, scale H, scale W), one launch: every
                                                         output pixel is the fp32 sum of its covering tile pixels (ascending tile
                                                         row, then tile column) times ``1.0f / count``.

The plan of an axis of ``n`` pixels restates ``ImageFolder``:

    margin = n - int((n - p) / s + 1) * s          (int() truncates toward zero)
    pad    = 0 if margin == 0 else ceil((p - margin) / 2)
    L      = (n + 2 pad - p) // s + 1

Tile ``t`` covers the padded coordinates ``[t s, t s + p)`` and the image sits at ``[pad, pad + n)``.  A plan that leaves a pixel
uncovered (only some ``n < p`` do) raises ``ValueError``.

**The HR side is the LR plan times the integer scale** (``P = scale p``, ``S = scale s``, ``pad_hr = scale pad``), so SR tile
``t`` lies exactly over LR tile ``t``.  This deliberately differs from the reference, which builds an independent HR
``ImageFolder``: when ``p - margin`` is odd its HR padding is ``ceil(scale (p - margin) / 2)``, not ``scale ceil((p - margin) /
2)``, and its SR tiles are folded up to ``scale / 2`` pixels away from where their LR tiles were cut.  Non-integer scales raise.

**The x8 geometric self-ensemble** (``SRTester(self_ensemble=True)``): ``dihedral(x, k)`` / ``dihedral_inverse(y, k)``, k in
0..7, are the eight flips and transposes of the last two dims and their inverses (torch views, any device: the semantics and
the tests' oracle).  ``unfold_tiles_d8`` is ``unfold_tiles`` with every tile written eight times, slot ``8 t + k`` holding
``dihedral(tile t, k)``; ``merge_tiles_d8`` maps the network's outputs ``y (8 n, C, P, P)`` to ``(n, C, P, P)``,
``((((y0' + y1') + y2') + ...) + y7') * 0.125`` with ``yk' = dihedral_inverse(y[8 t + k], k)``, in fp32, k ascending.  One launch
each (rdst_unfold_tiles_d8 / rdst_merge_tiles_d8); the merged tiles are folded by ``fold_tiles`` as they are.

``pad_mode='zero'`` pads the LR slice with zeros, as ``nn.Unfold(padding=...)`` and the reference do; ``'edge'`` repeats the
edge, as ``data.edge_pad`` does.  The unfold, fold and merge functions run on GPU tensors only; there is no CPU path."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

PAD_MODES = {"zero": 0, "edge": 1}


class Grid(NamedTuple):
    """The tiles of one side (LR or HR) of a plan: image size, patch, stride, padding before each axis, tiles per axis."""
    H: int
    W: int
    patch: int
    stride: int
    pad_y: int
    pad_x: int
    Ly: int
    Lx: int


def axis_plan(n: int, p: int, s: int):
    """``(pad, L)`` of an axis of ``n`` pixels, patch ``p``, stride ``s`` (the module docstring's three lines, in integers)."""
    num = n - p + s                                     # (n - p) / s + 1 = num / s
    q = num // s if num >= 0 else -((-num) // s)        # int(): toward zero
    margin = n - q * s
    pad = 0 if margin == 0 else -((margin - p) // 2)    # ceil((p - margin) / 2)
    return pad, (n + 2 * pad - p) // s + 1


def axis_cover(n: int, p: int, s: int, pad: int, L: int) -> np.ndarray:
    """How many of the ``L`` tiles cover each of the ``n`` pixels of an axis (int64)."""
    X = np.arange(n, dtype=np.int64) + pad
    lo = np.where(X < p, 0, (X - p) // s + 1)
    hi = np.minimum(X // s, L - 1)
    return np.maximum(hi - lo + 1, 0)


class TilePlan:
    """The tile plan of ``H x W`` slices: ``lr`` and ``hr`` (``Grid``), ``tiles_per_slice``, ``cover()``."""

    def __init__(self, H: int, W: int, patch: int, stride: int, scale=1, pad_mode: str = "zero"):
        H, W, patch, stride = int(H), int(W), int(patch), int(stride)
        if min(H, W, patch, stride) <= 0:
            raise ValueError(f"TilePlan: sizes must be positive, got H={H} W={W} patch={patch} stride={stride}")
        if float(scale) != int(scale) or int(scale) < 1:
            raise ValueError(f"TilePlan: the HR plan is the LR plan times an integer scale >= 1, got scale={scale}")
        if pad_mode not in PAD_MODES:
            raise ValueError(f"TilePlan: pad_mode must be one of {sorted(PAD_MODES)}, got {pad_mode!r}")
        self.scale, self.pad_mode = int(scale), pad_mode
        (pad_y, Ly), (pad_x, Lx) = axis_plan(H, patch, stride), axis_plan(W, patch, stride)
        for name, n, pad, L in (("H", H, pad_y, Ly), ("W", W, pad_x, Lx)):
            if pad < 0 or L <= 0 or stride > patch or (L - 1) * stride + patch < pad + n:
                raise ValueError(f"TilePlan: patch={patch} stride={stride} leaves pixels of {name}={n} uncovered "
                                 f"(pad={pad}, {L} tiles)")
        self.lr = Grid(H, W, patch, stride, pad_y, pad_x, Ly, Lx)
        k = self.scale
        self.hr = Grid(k * H, k * W, k * patch, k * stride, k * pad_y, k * pad_x, Ly, Lx)
        self.tiles_per_slice = Ly * Lx

    def cover(self, hr: bool = False) -> np.ndarray:
        """The cover count of every pixel (the reference's divisor image), ``(H, W)`` int64, of the LR or the HR side."""
        g = self.hr if hr else self.lr
        return np.outer(axis_cover(g.H, g.patch, g.stride, g.pad_y, g.Ly), axis_cover(g.W, g.patch, g.stride, g.pad_x, g.Lx))

    def __repr__(self) -> str:
        return f"TilePlan(lr={self.lr}, scale={self.scale}, pad_mode={self.pad_mode!r})"


def dihedral(x: torch.Tensor, k: int) -> torch.Tensor:
    """Transform ``k`` (0..7) of the last two dims, a view: flip the columns if ``k & 1``, flip the rows if ``k & 2``, then
    transpose if ``k & 4``.  On a ``p x p`` image ``dihedral(x, k)[i, j] = x[a, b]`` with ``(a, b) = (j, i) if k & 4 else (i, j)``,
    then ``a = p - 1 - a if k & 2`` and ``b = p - 1 - b if k & 1``."""
    if not 0 <= int(k) < 8:
        raise ValueError(f"dihedral: k must be in 0..7, got {k}")
    if k & 1:
        x = x.flip(-1)
    if k & 2:
        x = x.flip(-2)
    if k & 4:
        x = x.transpose(-1, -2)
    return x


def dihedral_inverse(y: torch.Tensor, k: int) -> torch.Tensor:
    """Undo ``dihedral(., k)``: the same three steps in the opposite order (``dihedral`` itself is NOT its inverse for
    ``k`` = 5 and 6, a flip of one axis followed by the transpose)."""
    if not 0 <= int(k) < 8:
        raise ValueError(f"dihedral_inverse: k must be in 0..7, got {k}")
    if k & 4:
        y = y.transpose(-1, -2)
    if k & 2:
        y = y.flip(-2)
    if k & 1:
        y = y.flip(-1)
    return y


def _need_gpu(what: str, *ts: torch.Tensor) -> None:
    for t in ts:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"rdst_amd.tiling.{what}: expected a torch tensor")
        if not t.is_cuda:
            raise RuntimeError(f"rdst_amd.tiling.{what}: the HIP path needs GPU tensors; there is no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"rdst_amd.tiling.{what}: tensors must be float32, got {t.dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def unfold_tiles(x: torch.Tensor, plan: TilePlan, out: Optional[torch.Tensor] = None, first_tile: int = 0,
                 n_slots: Optional[int] = None) -> torch.Tensor:
    """fp32 CUDA ``(N, C, H, W)`` -> tiles ``[first_tile, first_tile + n_slots)`` of the ``N Ly Lx`` tiles of ``plan.lr`` as a
    contiguous ``(n_slots, C, p, p)`` tensor (``out``, or a new one); slice-major, then tile row, then tile column, the order of
    ``nn.Unfold(...).transpose(1, 2)``.  ``n_slots`` defaults to the tiles from ``first_tile`` to the last (the shape of ``out``
    when that is given); slots past the last tile are filled with zeros."""
    _need_gpu("unfold_tiles", x)
    g = plan.lr
    if x.dim() != 4 or tuple(x.shape[-2:]) != (g.H, g.W) or x.shape[0] <= 0 or x.shape[1] <= 0:
        raise ValueError(f"unfold_tiles: x must be (N, C, {g.H}, {g.W}), got {tuple(x.shape)}")
    N, C = int(x.shape[0]), int(x.shape[1])
    first_tile = int(first_tile)
    if n_slots is None:
        n_slots = int(out.shape[0]) if out is not None else N * plan.tiles_per_slice - first_tile
    n_slots = int(n_slots)
    if first_tile < 0 or n_slots <= 0:
        raise ValueError(f"unfold_tiles: first_tile={first_tile} n_slots={n_slots} select no tile of {N * plan.tiles_per_slice}")
    shape = (n_slots, C, g.patch, g.patch)
    x = x.contiguous()
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        else:
            _need_gpu("unfold_tiles", out)
            if tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
                raise ValueError(f"unfold_tiles: out must be a contiguous float32 {shape} tensor on {x.device}")
        _lib.check(_lib.load().rdst_unfold_tiles(x.data_ptr(), out.data_ptr(), N, C, g.H, g.W, g.patch, g.stride, g.pad_y,
                                                 g.pad_x, g.Ly, g.Lx, PAD_MODES[plan.pad_mode], first_tile, n_slots, _stream()),
                   "rdst_unfold_tiles")
    return out


def fold_tiles(tiles: torch.Tensor, plan: TilePlan, N: int) -> torch.Tensor:
    """fp32 CUDA tiles ``(N Ly Lx, C, P, P)`` of ``plan.hr``, in the order ``unfold_tiles`` writes them -> ``(N, C, scale H,
    scale W)``, overlaps averaged.  Deterministic: the same tiles give the same bits."""
    _need_gpu("fold_tiles", tiles)
    g, N = plan.hr, int(N)
    if N <= 0 or tiles.dim() != 4 or tuple(tiles.shape[-2:]) != (g.patch, g.patch) or tiles.shape[1] <= 0 \
            or tiles.shape[0] != N * plan.tiles_per_slice:
        raise ValueError(f"fold_tiles: tiles must be ({N} * {plan.tiles_per_slice}, C, {g.patch}, {g.patch}), got "
                         f"{tuple(tiles.shape)}")
    C = int(tiles.shape[1])
    tiles = tiles.contiguous()
    with torch.cuda.device(tiles.device):
        out = torch.empty(N, C, g.H, g.W, dtype=torch.float32, device=tiles.device)
        _lib.check(_lib.load().rdst_fold_tiles(tiles.data_ptr(), out.data_ptr(), N, C, g.H, g.W, g.patch, g.stride, g.pad_y,
                                               g.pad_x, g.Ly, g.Lx, _stream()), "rdst_fold_tiles")
    return out


def unfold_tiles_d8(x: torch.Tensor, plan: TilePlan, out: Optional[torch.Tensor] = None, first_tile: int = 0,
                    n_slots: Optional[int] = None) -> torch.Tensor:
    """``unfold_tiles`` with every tile written eight times: slot ``j`` of the contiguous ``(n_slots, C, p, p)`` result holds
    ``dihedral(tile first_tile + j // 8, j % 8)``, the pad rule applied before the transform.  ``n_slots`` (a multiple of 8)
    defaults to 8 times the tiles from ``first_tile`` to the last (the shape of ``out`` when that is given); the slots of tiles
    past the last are zeros."""
    _need_gpu("unfold_tiles_d8", x)
    g = plan.lr
    if x.dim() != 4 or tuple(x.shape[-2:]) != (g.H, g.W) or x.shape[0] <= 0 or x.shape[1] <= 0:
        raise ValueError(f"unfold_tiles_d8: x must be (N, C, {g.H}, {g.W}), got {tuple(x.shape)}")
    N, C = int(x.shape[0]), int(x.shape[1])
    first_tile = int(first_tile)
    if n_slots is None:
        n_slots = int(out.shape[0]) if out is not None else 8 * (N * plan.tiles_per_slice - first_tile)
    n_slots = int(n_slots)
    if first_tile < 0 or n_slots <= 0:
        raise ValueError(f"unfold_tiles_d8: first_tile={first_tile} n_slots={n_slots} select no tile of "
                         f"{N * plan.tiles_per_slice}")
    if n_slots % 8:
        raise ValueError(f"unfold_tiles_d8: n_slots={n_slots} must be a multiple of 8 (eight slots per tile)")
    shape = (n_slots, C, g.patch, g.patch)
    x = x.contiguous()
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        else:
            _need_gpu("unfold_tiles_d8", out)
            if tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
                raise ValueError(f"unfold_tiles_d8: out must be a contiguous float32 {shape} tensor on {x.device}")
        _lib.check(_lib.load().rdst_unfold_tiles_d8(x.data_ptr(), out.data_ptr(), N, C, g.H, g.W, g.patch, g.stride, g.pad_y,
                                                    g.pad_x, g.Ly, g.Lx, PAD_MODES[plan.pad_mode], first_tile, n_slots,
                                                    _stream()), "rdst_unfold_tiles_d8")
    return out


def merge_tiles_d8(y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 CUDA ``y (8 n, C, P, P)``, slot ``8 t + k`` the network's output for ``dihedral(tile t, k)`` -> ``(n, C, P, P)``
    (``out``, e.g. a run of rows of a larger tile buffer, or a new tensor): the fp32 sum of ``dihedral_inverse(y[8 t + k], k)``
    over ascending ``k``, left to right, times 0.125.  Deterministic: the same ``y`` gives the same bits."""
    _need_gpu("merge_tiles_d8", y)
    if y.dim() != 4 or y.shape[0] <= 0 or y.shape[0] % 8 or y.shape[1] <= 0 or y.shape[2] != y.shape[3] or y.shape[2] <= 0:
        raise ValueError(f"merge_tiles_d8: y must be (8 n, C, P, P), got {tuple(y.shape)}")
    n, C, P = int(y.shape[0]) // 8, int(y.shape[1]), int(y.shape[2])
    shape = (n, C, P, P)
    y = y.contiguous()
    with torch.cuda.device(y.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=y.device)
        else:
            _need_gpu("merge_tiles_d8", out)
            if tuple(out.shape) != shape or out.device != y.device or not out.is_contiguous():
                raise ValueError(f"merge_tiles_d8: out must be a contiguous float32 {shape} tensor on {y.device}")
        _lib.check(_lib.load().rdst_merge_tiles_d8(y.data_ptr(), out.data_ptr(), n, C, P, _stream()), "rdst_merge_tiles_d8")
    return out
