"""Host side of rdst_amd.data (no GPU): the tap tables of the bicubic resize against the closed form in float64, the edge
padding against numpy, and the index draws of DevicePatchSampler."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rdst_amd import data as D

SIZE_PAIRS = [((96, 96), (24, 24)), ((256, 256), (64, 64)), ((176, 208), (44, 52)), ((160, 200), (64, 80)),
              ((100, 90), (66, 60)), ((44, 52), (176, 208)), ((97, 131), (27, 37))]
AXES = sorted({(i, o) for a, b in SIZE_PAIRS for i, o in zip(a, b)})


def _keys(d, a=Fraction(-3, 4)):
    """The Keys cubic-convolution kernel at distance d >= 0."""
    if d <= 1:
        return ((a + 2) * d - (a + 3)) * d * d + 1
    if d < 2:
        return ((a * d - 5 * a) * d + 8 * a) * d - 4 * a
    return Fraction(0)


def _closed_form(n_in, n_out):
    """The resize of one axis as a matrix: half-pixel mapping, four taps, clamped tap indices.  In exact rationals, rounded
    to float64 at the end (the coordinate reaches 256, where float64 arithmetic on it alone would cost 3e-14)."""
    M = [[Fraction(0)] * n_in for _ in range(n_out)]
    for o in range(n_out):
        src = Fraction((2 * o + 1) * n_in - n_out, 2 * n_out)        # (o + 0.5) * n_in / n_out - 0.5
        f = math.floor(src)
        for p in range(f - 1, f + 3):
            M[o][min(max(p, 0), n_in - 1)] += _keys(abs(src - p))
    return np.array([[float(v) for v in row] for row in M])


def _matrix(index, weight, n_in):
    M = np.zeros((len(index), n_in))
    for o in range(len(index)):
        for k in range(4):
            M[o, index[o, k]] += weight[o, k]
    return M


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_tap_table_is_the_closed_form(n_in, n_out):
    index, weight = D.tap_table(n_in, n_out)
    assert index.shape == weight.shape == (n_out, 4) and index.dtype == np.int32 and weight.dtype == np.float64
    assert index.min() >= 0 and index.max() <= n_in - 1
    assert (np.diff(index, axis=1) >= 0).all() and (np.diff(index[:, 0]) >= 0).all()
    assert np.abs(weight.sum(axis=1) - 1.0).max() <= 1e-15
    M = _matrix(index, weight, n_in)
    assert np.abs(M - _closed_form(n_in, n_out)).max() <= 1e-14
    # and it is torch's float64 bicubic: the operator read off an identity image (the width is resized 1:1)
    eye = torch.eye(n_in, dtype=torch.float64)[None, None]
    T = F.interpolate(eye, size=(n_out, n_in), mode="bicubic", align_corners=False)[0, 0].numpy()
    # (torch forms the coordinate in float64 arithmetic: up to 256 it carries a few roundings of 2.8e-14 each, and the
    # kernel's slope is at most 1.5)
    assert np.abs(M - T).max() <= 2e-13


def test_tap_table_at_ratio_four_is_dyadic():
    index, weight = D.tap_table(64, 16)
    assert (index == (4 * np.arange(16)[:, None] + np.arange(4)[None, :])).all()
    assert (weight.astype(np.float32) == np.array([-3 / 32, 19 / 32, 19 / 32, -3 / 32], dtype=np.float32)).all()
    with pytest.raises(ValueError):
        D.tap_table(0, 4)


@pytest.mark.parametrize("shape,size", [((3, 2, 10, 13), 16), ((2, 1, 20, 9), 16), ((2, 3, 20, 24), 16), ((4, 7, 11), (12, 11))])
def test_edge_pad_is_numpy_edge_padding(shape, size):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    th, tw = (size, size) if isinstance(size, int) else size
    H, W = shape[-2:]
    ph, pw = max(th - H, 0), max(tw - W, 0)
    pads = [(0, 0)] * (len(shape) - 2) + [(math.ceil(ph / 2), ph // 2), (math.ceil(pw / 2), pw // 2)]
    want = np.pad(x.numpy(), pads, mode="edge")
    got = D.edge_pad(x, size)
    assert tuple(got.shape) == want.shape == shape[:-2] + (max(H, th), max(W, tw))
    assert np.array_equal(got.numpy(), want)
    if ph == 0 and pw == 0:
        assert got is x
    lab = (x * 5).to(torch.uint8)
    assert np.array_equal(D.edge_pad(lab, size).numpy(), np.pad(lab.numpy(), pads, mode="edge"))


def _slices(S=12, C=1, H=20, W=20, seed=0):
    return torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(seed))


def test_sampler_pads_and_normalises_like_the_reference():
    imgs = [np.random.RandomState(i).rand(10, 30, 2).astype(np.float32) for i in range(5)]
    labs = [np.random.RandomState(i).randint(0, 4, (10, 30)) for i in range(5)]
    s = D.DevicePatchSampler(imgs, 2, 4, sr_scales=(2.0, 4.0), labels=labs, device="cpu")
    padded = np.stack([np.pad(a, ((3, 3), (0, 0), (0, 0)), mode="edge") for a in imgs])
    assert (s.S, s.C, s.H, s.W) == (5, 2, 16, 30) and s.hr_patch_sizes == [8, 16] and len(s) == 5
    assert np.array_equal(s.hr_images.permute(0, 2, 3, 1).numpy(), padded)
    assert np.array_equal(s.labels.numpy(), np.stack([np.pad(a, ((3, 3), (0, 0)), mode="edge") for a in labs]))
    assert np.array_equal(s.mean, np.mean(padded, axis=(0, 1, 2))) and np.array_equal(s.std, np.std(padded, axis=(0, 1, 2)))
    with pytest.raises(RuntimeError):
        s.sample()


def test_draws_are_seeded_distinct_and_cover_the_range():
    def sampler(seed):
        return D.DevicePatchSampler(_slices(), 4, 4, sr_scales=(4.0,), device="cpu",
                                    generator=torch.Generator().manual_seed(seed))
    a, b = sampler(7), sampler(7)
    seen = [set(), set()]
    for _ in range(64):
        da, db = a.draw(), b.draw()
        assert da.sr_factor == 4.0 and da.hr_patch_size == 16
        assert da.indices.dtype == torch.int32 and tuple(da.indices.shape) == (4, 3)
        assert torch.equal(da.indices, db.indices)
        t = da.indices.numpy()
        assert len(set(t[:, 0])) == 4 and t[:, 0].min() >= 0 and t[:, 0].max() < 12
        assert t[:, 1:].min() >= 0 and t[:, 1:].max() <= 4
        seen[0] |= set(t[:, 1])
        seen[1] |= set(t[:, 2])
    assert {0, 4} <= seen[0] and {0, 4} <= seen[1]
    assert not torch.equal(sampler(8).draw().indices, sampler(7).draw().indices)
    # several scales: one per batch, the patch size follows it
    m = D.DevicePatchSampler(_slices(), 4, 4, sr_scales=(2.0, 2.5, 4.0), device="cpu", generator=torch.Generator().manual_seed(1))
    draws = [m.draw() for _ in range(32)]
    assert {(d.sr_factor, d.hr_patch_size) for d in draws} == {(2.0, 8), (2.5, 10), (4.0, 16)}
    assert all(d.indices[:, 1:].max() <= 20 - d.hr_patch_size for d in draws)
    assert m.batch_shapes(draws[0]) == ((4, 1, 4, 4), (4, 1, draws[0].hr_patch_size, draws[0].hr_patch_size))


def test_sampler_refuses_what_it_cannot_do():
    with pytest.raises(ValueError):
        D.DevicePatchSampler(_slices(S=3), 4, 4, device="cpu")                       # fewer slices than the batch
    with pytest.raises(ValueError):
        D.DevicePatchSampler([np.zeros((20, 20, 1)), np.zeros((20, 21, 1))], 1, 4, device="cpu")
    with pytest.raises(ValueError):
        D.DevicePatchSampler(_slices(), 4, 4, blur_method="gaussian", device="cpu")
    with pytest.raises(ValueError):
        D.DevicePatchSampler(_slices(), 4, 4, labels=torch.zeros(12, 20, 21), device="cpu")
    D.DevicePatchSampler(_slices(), 4, 4, blur_method="", device="cpu")
    # a slice smaller than the patch is padded up to it, never refused: the patch then is the whole padded slice
    s = D.DevicePatchSampler(_slices(H=8, W=30), 4, 4, device="cpu")
    assert (s.H, s.W) == (16, 30) and int(s.draw().indices[:, 1].max()) == 0


def test_resize_refuses_host_tensors_and_gradients():
    with pytest.raises(RuntimeError):
        D.bicubic_resize(torch.rand(1, 1, 8, 8), 4)
    with pytest.raises(RuntimeError):
        D.make_test_pair(torch.rand(1, 1, 8, 8), 2)


def test_entry_points_refuse_sizes_that_cannot_hold_a_patch():
    """The host checks come before any pointer is used or anything is launched: no GPU needed."""
    from rdst_amd import _lib
    lib = _lib.load()
    args = dict(S=4, C=1, H=20, W=30, B=2, hp=16, lp=4)

    def call(**kw):
        a = {**args, **kw}
        return lib.rdst_sample_patches(None, None, None, None, None, None, a["S"], a["C"], a["H"], a["W"], a["B"], a["hp"],
                                       a["lp"], None, None, None)
    assert call(hp=24) == _lib.EINVAL and b"does not fit" in lib.rdst_last_error()      # taller than the slice
    assert call(H=40, hp=32) == _lib.EINVAL                                              # wider than the slice
    assert call(B=0) == _lib.EINVAL and call(lp=0) == _lib.EINVAL and call(S=-1) == _lib.EINVAL
    assert call() == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()            # sizes fine, nothing to read
    assert lib.rdst_resize_bicubic(None, None, 1, 1, 8, 8, 0, 4, None, None, None, None, None) == _lib.EINVAL
    assert lib.rdst_resize_bicubic(None, None, 1, 1, 8, 8, 4, 4, None, None, None, None, None) == _lib.EINVAL
