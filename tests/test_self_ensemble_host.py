"""Host side of the x8 geometric self-ensemble (no GPU): the eight transforms and their inverses (rdst_amd.tiling.dihedral /
dihedral_inverse), the constructor checks of SRTester(self_ensemble=True), and the argument checks of the two C entry points
(called through ctypes: they return before any pointer is used or anything is launched)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from rdst_amd import tiling as T


def _ramp(h, w):
    """A ramp without any symmetry: every pixel has its own value."""
    return torch.arange(h * w, dtype=torch.float32).reshape(h, w) * 3.0 + 1.0


@pytest.mark.parametrize("h,w", [(6, 6), (5, 7)])
def test_dihedral_is_eight_transforms_with_their_inverses(h, w):
    x = _ramp(h, w)
    imgs = [T.dihedral(x, k) for k in range(8)]
    for k, y in enumerate(imgs):
        assert tuple(y.shape) == ((w, h) if k & 4 else (h, w))
        assert torch.equal(T.dihedral_inverse(y, k), x), k
        # the index form the kernels use: (a, b) = (j, i) if k & 4 else (i, j), then the flips of the source's own axes
        for i in range(y.shape[0]):
            for j in range(y.shape[1]):
                a, b = (j, i) if k & 4 else (i, j)
                if k & 2:
                    a = h - 1 - a
                if k & 1:
                    b = w - 1 - b
                assert y[i, j] == x[a, b], (k, i, j)
    for k in range(8):
        for m in range(k):
            assert imgs[k].shape != imgs[m].shape or not torch.equal(imgs[k], imgs[m]), (k, m)
    # leading dims are left alone
    xb = torch.stack([x, x + 100.0])[None]
    for k in range(8):
        assert torch.equal(T.dihedral(xb, k)[0, 1], T.dihedral(x + 100.0, k))
        assert torch.equal(T.dihedral_inverse(T.dihedral(xb, k), k), xb)


def test_dihedral_is_its_own_inverse_except_for_5_and_6():
    """The classic bug: undoing a transform by applying it again.  Wrong exactly for a single flip followed by the transpose."""
    x = _ramp(6, 6)
    wrong = {k for k in range(8) if not torch.equal(T.dihedral(T.dihedral(x, k), k), x)}
    assert wrong == {5, 6}
    with pytest.raises(ValueError):
        T.dihedral(x, 8)
    with pytest.raises(ValueError):
        T.dihedral_inverse(x, -1)


class _StandIn(nn.Module):
    def __init__(self):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x.repeat_interleave(2, -1).repeat_interleave(2, -2)


def test_tester_constructor_checks():
    from rdst_amd.tester import SRTester
    net = _StandIn()
    with pytest.raises(ValueError, match="one tile"):
        SRTester(net, sr_scale=2, self_ensemble=True)
    with pytest.raises(ValueError, match="multiple of 8"):
        SRTester(net, sr_scale=2, tile=16, tile_batch=12, self_ensemble=True)
    t = SRTester(net, sr_scale=2, tile=16, tile_batch=16, self_ensemble=True)
    assert t.self_ensemble and t.tile_batch == 16
    plain = SRTester(net, sr_scale=2, tile=16, tile_batch=5, self_ensemble=False)
    assert not plain.self_ensemble and not SRTester(net, sr_scale=2, tile=16, tile_batch=5).self_ensemble


def test_functions_refuse_host_tensors():
    plan = T.TilePlan(20, 27, 16, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.unfold_tiles_d8(torch.rand(1, 1, 20, 27), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.merge_tiles_d8(torch.rand(8, 1, 16, 16))


def test_entry_points_refuse_bad_arguments():
    """The host checks come before any pointer is used or anything is launched: no GPU needed."""
    from rdst_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)         # a non-null pointer that is never dereferenced: every call below is refused
    ptr = ctypes.addressof(buf)
    good = dict(x=ptr, out=ptr, N=2, C=1, H=34, W=42, p=24, s=16, pad_y=3, pad_x=7, Ly=2, Lx=3, mode=0, first=0, slots=16)

    def unfold(**kw):
        a = {**good, **kw}
        return lib.rdst_unfold_tiles_d8(a["x"], a["out"], a["N"], a["C"], a["H"], a["W"], a["p"], a["s"], a["pad_y"], a["pad_x"],
                                        a["Ly"], a["Lx"], a["mode"], a["first"], a["slots"], None)

    assert unfold(slots=12) == _lib.EINVAL and b"multiple of 8" in lib.rdst_last_error()
    assert unfold(slots=0) == _lib.EINVAL and b"n_slots=0" in lib.rdst_last_error()
    assert unfold(slots=-8) == _lib.EINVAL and unfold(first=-1) == _lib.EINVAL
    assert unfold(Ly=1) == _lib.EINVAL and b"do not reach" in lib.rdst_last_error()
    assert unfold(Lx=2) == _lib.EINVAL and b"do not reach" in lib.rdst_last_error()
    assert unfold(s=25, Ly=9, Lx=9) == _lib.EINVAL and b"stride > patch" in lib.rdst_last_error()
    assert unfold(mode=2) == _lib.EINVAL and b"bad pad mode" in lib.rdst_last_error()
    assert unfold(x=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
    assert unfold(out=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
    for name in ("N", "C", "H", "W", "p", "s", "Ly", "Lx"):
        assert unfold(**{name: 0}) == _lib.EINVAL and unfold(**{name: -3}) == _lib.EINVAL, name
    assert b"rdst_unfold_tiles_d8" in lib.rdst_last_error()

    def merge(y=ptr, out=ptr, n=2, C=1, P=24):
        return lib.rdst_merge_tiles_d8(y, out, n, C, P, None)

    assert merge(n=0) == _lib.EINVAL and b"n_tiles=0" in lib.rdst_last_error()
    assert merge(P=0) == _lib.EINVAL and b"P=0" in lib.rdst_last_error()
    assert merge(n=-1) == _lib.EINVAL and merge(C=0) == _lib.EINVAL and merge(P=-4) == _lib.EINVAL
    assert merge(y=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
    assert merge(out=None) == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()
    assert merge(P=(1 << 24) + 1) == _lib.EINVAL and b"too large" in lib.rdst_last_error()
    assert merge(n=1 << 20, C=1 << 10, P=1 << 10) == _lib.EINVAL and b"too large" in lib.rdst_last_error()
    assert b"rdst_merge_tiles_d8" in lib.rdst_last_error()
