"""Host side of rdst_amd.tiling (no GPU): the plan arithmetic against torch's own nn.Unfold / nn.Fold on an all-ones image,
the refusals, the scaled HR plan, and the argument checks of the two C entry points (called through ctypes: they return before
any pointer is used or anything is launched)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from rdst_amd import tiling as T

# (H, W, patch, stride); the first is the reference-shaped OASIS slice at x4 (176 x 208, 20 cut off each side)
PLANS = [(34, 42, 24, 16), (34, 42, 16, 8), (20, 27, 16, 8), (33, 16, 16, 8), (16, 16, 16, 8), (40, 48, 8, 8), (44, 52, 32, 24),
         (17, 63, 8, 6), (64, 64, 64, 48), (100, 90, 48, 40), (9, 31, 8, 3), (259, 8, 40, 25), (24, 40, 24, 24), (25, 41, 24, 24)]


def _ones_oracle(H, W, p, s, pad_y, pad_x):
    """Tile count and cover counts from nn.Unfold / nn.Fold in float64 (padding = the plan's)."""
    unfold = nn.Unfold(kernel_size=p, stride=s, padding=(pad_y, pad_x))
    fold = nn.Fold(output_size=(H, W), kernel_size=p, stride=s, padding=(pad_y, pad_x))
    cols = unfold(torch.ones(1, 1, H, W, dtype=torch.float64))
    return cols.shape[-1], fold(torch.ones_like(cols))[0, 0].numpy()


@pytest.mark.parametrize("H,W,p,s", PLANS)
def test_plan_is_the_unfold_fold_geometry(H, W, p, s):
    plan = T.TilePlan(H, W, p, s)
    g = plan.lr
    assert (g.H, g.W, g.patch, g.stride) == (H, W, p, s) and plan.hr == g and plan.scale == 1
    # the three lines of ImageFolder, per axis, in floating point as the reference evaluates them
    for n, pad, L in ((H, g.pad_y, g.Ly), (W, g.pad_x, g.Lx)):
        margin = n - int((n - p) / s + 1) * s
        assert pad == (0 if margin == 0 else math.ceil((p - margin) / 2))
        assert L == (n + 2 * pad - p) // s + 1
    count, cover = _ones_oracle(H, W, p, s, g.pad_y, g.pad_x)
    assert plan.tiles_per_slice == g.Ly * g.Lx == count
    assert np.array_equal(plan.cover(), cover.astype(np.int64)) and np.array_equal(cover, np.round(cover))
    assert plan.cover().min() >= 1 and plan.cover().max() <= 16


def test_the_oasis_slice_at_x4():
    plan = T.TilePlan(34, 42, 24, 16, scale=4)
    assert plan.lr == T.Grid(34, 42, 24, 16, 3, 7, 2, 3) and plan.tiles_per_slice == 6
    assert plan.hr == T.Grid(136, 168, 96, 64, 12, 28, 2, 3)


def test_every_axis_at_least_one_patch_long_is_covered():
    for p in (8, 16, 24, 40, 64):
        for s in sorted({1, p // 4, p // 2, p - 1, p} - {0}):
            for n in range(p, 260):
                pad, L = T.axis_plan(n, p, s)
                cover = T.axis_cover(n, p, s, pad, L)
                assert pad >= 0 and L >= 1 and cover.min() >= 1, (n, p, s)
                if s >= p // 4 and s > 1:
                    assert cover.max() <= 4, (n, p, s)


@pytest.mark.parametrize("scale", [2, 3, 4, 4.0])
def test_hr_plan_is_the_scaled_lr_plan(scale):
    plan = T.TilePlan(20, 27, 16, 8, scale=scale)
    k, lr, hr = int(scale), plan.lr, plan.hr
    assert hr == T.Grid(k * lr.H, k * lr.W, k * lr.patch, k * lr.stride, k * lr.pad_y, k * lr.pad_x, lr.Ly, lr.Lx)
    # so an SR pixel is covered by exactly the tiles that cover its LR pixel
    assert np.array_equal(plan.cover(hr=True), np.kron(plan.cover(), np.ones((k, k), dtype=np.int64)))
    count, cover = _ones_oracle(hr.H, hr.W, hr.patch, hr.stride, hr.pad_y, hr.pad_x)
    assert count == plan.tiles_per_slice and np.array_equal(plan.cover(hr=True), cover.astype(np.int64))


def test_plan_refuses_what_it_cannot_cover():
    with pytest.raises(ValueError, match="uncovered"):
        T.TilePlan(4, 32, 8, 2)                   # H < patch: no tile fits
    with pytest.raises(ValueError, match="uncovered"):
        T.TilePlan(32, 4, 8, 2)
    with pytest.raises(ValueError, match="uncovered"):
        T.TilePlan(32, 32, 8, 12)                 # stride > patch: gaps between the tiles
    for scale in (1.5, 2.5, 0, -1, 0.5):
        with pytest.raises(ValueError, match="integer scale"):
            T.TilePlan(32, 32, 8, 8, scale=scale)
    with pytest.raises(ValueError):
        T.TilePlan(32, 32, 8, 8, pad_mode="reflect")
    with pytest.raises(ValueError):
        T.TilePlan(32, 0, 8, 8)
    with pytest.raises(ValueError):
        T.TilePlan(32, 32, 8, 0)


def test_functions_refuse_host_tensors():
    plan = T.TilePlan(20, 27, 16, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.unfold_tiles(torch.rand(1, 1, 20, 27), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.fold_tiles(torch.rand(plan.tiles_per_slice, 1, 16, 16), plan, 1)


def test_entry_points_refuse_bad_arguments():
    """The host checks come before any pointer is used or anything is launched: no GPU needed."""
    import ctypes
    from rdst_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)         # a non-null pointer that is never dereferenced: every call below is refused
    ptr = ctypes.addressof(buf)
    good = dict(x=ptr, out=ptr, N=2, C=1, H=34, W=42, p=24, s=16, pad_y=3, pad_x=7, Ly=2, Lx=3, mode=0, first=0, slots=4)

    def unfold(**kw):
        a = {**good, **kw}
        return lib.rdst_unfold_tiles(a["x"], a["out"], a["N"], a["C"], a["H"], a["W"], a["p"], a["s"], a["pad_y"], a["pad_x"],
                                     a["Ly"], a["Lx"], a["mode"], a["first"], a["slots"], None)

    def fold(**kw):
        a = {**good, **kw}
        return lib.rdst_fold_tiles(a["x"], a["out"], a["N"], a["C"], a["H"], a["W"], a["p"], a["s"], a["pad_y"], a["pad_x"],
                                   a["Ly"], a["Lx"], None)

    for call in (unfold, fold):
        assert call(x=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
        assert call(out=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
        for name in ("N", "C", "H", "W", "p", "s", "Ly", "Lx"):
            assert call(**{name: 0}) == _lib.EINVAL, name
            assert call(**{name: -3}) == _lib.EINVAL, name
        assert call(pad_y=-1) == _lib.EINVAL and call(pad_x=-1) == _lib.EINVAL
        # plans that leave pixels uncovered: too few tiles on an axis, too much padding in front, gaps between the tiles
        assert call(Ly=1) == _lib.EINVAL and b"do not reach" in lib.rdst_last_error()
        assert call(Lx=2) == _lib.EINVAL and b"do not reach" in lib.rdst_last_error()
        assert call(pad_y=7) == _lib.EINVAL and call(pad_x=23) == _lib.EINVAL
        assert call(H=4, W=32, p=8, s=2, pad_y=1, pad_x=0, Ly=0, Lx=13) == _lib.EINVAL
        assert call(s=25, Ly=9, Lx=9) == _lib.EINVAL and b"stride > patch" in lib.rdst_last_error()
    assert unfold(slots=0) == _lib.EINVAL and unfold(first=-1) == _lib.EINVAL and unfold(mode=2) == _lib.EINVAL
