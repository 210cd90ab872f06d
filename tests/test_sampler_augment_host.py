"""Host side of the sampler's augmentation (no GPU): what DevicePatchSampler(augment=...) draws and from where in the
generator's stream, the values it refuses, and the argument checks of rdst_sample_patches_d8 before any launch."""
import pytest
import torch

from rdst_amd import data as D


def _slices(S=12, C=1, H=20, W=20, seed=0):
    return torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(seed))


def _sampler(seed, **kw):
    return D.DevicePatchSampler(_slices(), 4, 4, sr_scales=(4.0,), device="cpu", generator=torch.Generator().manual_seed(seed),
                                **kw)


@pytest.mark.parametrize("off", [False, None])
def test_without_augment_the_draws_are_todays(off):
    a, b = _sampler(7), _sampler(7, augment=off)
    for _ in range(8):
        da, db = a.draw(), b.draw()
        assert da.variants is None and db.variants is None
        assert torch.equal(da.indices, db.indices)
    # the generator was consumed alike
    assert torch.equal(a.generator.get_state(), b.generator.get_state())
    # the fourth field is optional: a draw spelled with three still is one
    d = D.Draw(4.0, 16, da.indices)
    assert d.variants is None and d == da


@pytest.mark.parametrize("augment,n", [(True, 8), ("d8", 8), ("flip", 4)])
def test_variants_are_drawn_after_the_origins(augment, n):
    plain, aug = _sampler(7), _sampler(7, augment=augment)
    first = aug.draw()
    assert torch.equal(first.indices, plain.draw().indices)          # slice / top / left: the integers drawn today, first
    seen = set()
    for d in [first] + [aug.draw() for _ in range(63)]:
        v = d.variants
        assert v.dtype == torch.int32 and tuple(v.shape) == (4,) and not v.is_cuda
        assert d.indices.dtype == torch.int32 and tuple(d.indices.shape) == (4, 3)
        assert int(v.min()) >= 0 and int(v.max()) < n
        seen |= set(v.tolist())
    assert seen == set(range(n))
    # the same seed gives the same variants
    c, e = _sampler(9, augment=augment), _sampler(9, augment=augment)
    for _ in range(4):
        dc, de = c.draw(), e.draw()
        assert torch.equal(dc.variants, de.variants) and torch.equal(dc.indices, de.indices)


def test_augment_refuses_other_values():
    for bad in ("rot90", "D8", 1, 8, 0.5, ("flip",), ["d8"]):
        with pytest.raises(ValueError):
            _sampler(0, augment=bad)


def test_a_host_sampler_draws_and_does_not_sample():
    s = _sampler(3, augment=True)
    assert s.draw().variants is not None
    with pytest.raises(RuntimeError):
        s.sample()
    with pytest.raises(RuntimeError):
        s.sample(draw=D.Draw(4.0, 16, torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)))


def test_d8_entry_point_refuses_before_any_launch():
    """As tests/test_data_host.py::test_entry_points_refuse_sizes_that_cannot_hold_a_patch for the plain entry point: the
    host checks come before any pointer is used or anything is launched."""
    from rdst_amd import _lib
    lib = _lib.load()
    args = dict(S=4, C=1, H=20, W=30, B=2, hp=16, lp=4)

    def call(**kw):
        a = {**args, **kw}
        return lib.rdst_sample_patches_d8(None, None, None, None, None, None, None, a["S"], a["C"], a["H"], a["W"], a["B"],
                                          a["hp"], a["lp"], None, None, None)
    assert call(hp=24) == _lib.EINVAL and b"does not fit" in lib.rdst_last_error()      # taller than the slice
    assert b"rdst_sample_patches_d8" in lib.rdst_last_error()
    assert call(H=40, hp=32) == _lib.EINVAL                                              # wider than the slice
    assert call(B=0) == _lib.EINVAL and call(lp=0) == _lib.EINVAL and call(S=-1) == _lib.EINVAL and call(C=0) == _lib.EINVAL
    assert call() == _lib.EINVAL and b"null pointer" in lib.rdst_last_error()            # sizes fine, nothing to read
    # every pointer but the variant table (host memory here: the refusal comes before anything would read it)
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.rdst_sample_patches_d8(p, None, p, None, p, p, None, 4, 1, 20, 30, 2, 16, 4, None, None, None) == _lib.EINVAL
    assert b"null pointer" in lib.rdst_last_error()
    assert lib.rdst_abi_version() == _lib.ABI_VERSION == 11                              # an additive entry point
