"""CPU: the noise term of the device data path (rdst_amd.data.Noise, DevicePatchSampler(noise=), include/rdst_hip_noise.h).  The
float64 reference of tests/noise_reference.py against the Random123 known-answer vectors and against the statistical
thresholds tests/test_noise_gpu.py holds the device field to (so those are shown to hold for the reference alone, on the same
seed and shapes); the Python argument handling; what the sampler draws from its generator and how it packs the pinned buffer;
and every refusal of the three C entry points (returned before any launch: the library loads without a GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import noise_reference as R
from rdst_amd import _lib
from rdst_amd import data as D

N_STAT = 8 * 64 * 64                    # 8 planes of 64 x 64
T_MEAN = 5 / math.sqrt(N_STAT)          # 0.0276: five standard errors of a mean, of a correlation
T_VAR = 5 * math.sqrt(2 / N_STAT)       # 0.0391: five standard errors of the variance of unit normals


@pytest.mark.parametrize("counter,key,want", R.KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in R.philox4x32_10(*counter, *key)) == want


def test_counter_layout_of_the_reference():
    w = R.words(3, 4, 5, 0xA4093822_00000007)
    assert w.shape == (3, 4, 5, 4) and w.dtype == np.uint32
    one = R.philox4x32_10(2, 3, 1, 0, 0x00000007, 0xA4093822)           # x = 2, y = 3, plane = 1
    assert tuple(int(v) for v in w[1, 3, 2]) == tuple(int(v) for v in one)
    assert np.array_equal(R.words(1, 4, 5, 0xA4093822_00000007, plane0=2), w[2:])


def test_reference_statistics_hold_the_thresholds():
    """The thresholds of the device test on the reference alone: seed 0x0123456789ABCDEF, 8 planes of 64 x 64, n = 32768."""
    w = R.words(8, 64, 64, R.SEED)
    z0, z1 = R.normals(w)
    assert np.isfinite(z0).all() and np.isfinite(z1).all() and max(np.abs(z0).max(), np.abs(z1).max()) <= math.sqrt(48 * math.log(2))
    st = R.field_stats(z0, z1)
    print("[reference]", {k: round(v, 5) for k, v in st.items()}, "thresholds", round(T_MEAN, 4), round(T_VAR, 4))
    assert abs(st["mean0"]) < T_MEAN and abs(st["mean1"]) < T_MEAN
    assert abs(st["var0"] - 1) < T_VAR and abs(st["var1"] - 1) < T_VAR
    assert abs(st["corr01"]) < T_MEAN and abs(st["lag_x"]) < T_MEAN and abs(st["lag_y"]) < T_MEAN
    sigma = 0.05
    y, _ = R.apply(np.zeros((8, 1, 64, 64)), w, R.RICIAN, [sigma] * 8, [0.0] * 8)
    se = y.std() / math.sqrt(y.size)
    print(f"[reference] Rician mean at 0: {y.mean():.6f} against {sigma * math.sqrt(math.pi / 2):.6f}, standard error {se:.2e}")
    assert abs(y.mean() - sigma * math.sqrt(math.pi / 2)) < 5 * se
    # the hetero model at two intensities: the variances in the ratio of sd^2
    for v, gain, floor in ((0.25, 0.01, 0.0), (0.75, 0.01, 0.02)):
        y, sd = R.apply(np.full((8, 1, 64, 64), v), w, R.HETERO, [gain] * 8, [floor] * 8)
        assert np.allclose(sd, math.sqrt(gain * v + floor * floor)) and abs(((y - v) / sd).var() - 1) < T_VAR


def test_noise_value():
    n = D.Noise("gaussian", sigma=0.05)
    assert n == D.Noise("gaussian", sigma=0.05, clip=None) and hash(n) == hash(D.Noise.of(n)) and D.Noise.of(n) is n
    assert n != D.Noise("gaussian", sigma=0.05, clip=(0, 1)) and n != D.Noise("rician", sigma=0.05)
    assert len({n, D.Noise("gaussian", sigma=0.05), D.Noise("gaussian", sigma=(0.0, 0.05))}) == 2
    assert repr(D.Noise("poisson-gaussian", gain=(0, 0.02), clip=(0, 1))) == \
        "Noise('poisson-gaussian', gain=(0.0, 0.02), sigma=0.02, clip=(0.0, 1.0))"
    with pytest.raises(AttributeError):
        n.kind = "rician"
    # defaults, and where each level goes
    assert D.Noise.of("gaussian") == D.Noise("gaussian", sigma=D.DEFAULT_NOISE_SIGMA) and D.DEFAULT_NOISE_SIGMA == 0.02
    assert D.Noise.of("poisson-gaussian") == D.Noise("poisson-gaussian", gain=D.DEFAULT_NOISE_GAIN, sigma=D.DEFAULT_NOISE_SIGMA)
    assert (n.model, n.ranges) == (_lib.NOISE_HETERO, ((0.0, 0.0), (0.05, 0.05)))
    pg = D.Noise("poisson-gaussian", gain=(0.0, 0.02), sigma=0.01)
    assert (pg.model, pg.ranges) == (_lib.NOISE_HETERO, ((0.0, 0.02), (0.01, 0.01)))
    ri = D.Noise("rician", sigma=(0.01, 0.03))
    assert (ri.model, ri.ranges) == (_lib.NOISE_RICIAN, ((0.01, 0.03), (0.0, 0.0)))
    assert (_lib.NOISE_HETERO, _lib.NOISE_RICIAN) == (R.HETERO, R.RICIAN) == (0, 1)
    assert n.clip_range == (-math.inf, math.inf) and D.Noise("rician", clip=(0, 1)).clip_range == (0.0, 1.0)
    # levels: lo + (hi - lo) u in float64, rounded once
    u = torch.tensor([[0.0, 0.5], [0.25, 0.75], [0.999, 0.1]])
    got = D.Noise("poisson-gaussian", gain=(0.01, 0.03), sigma=(0.0, 0.1)).levels_from(u)
    want = torch.stack([0.01 + 0.02 * u[:, 0].double(), 0.1 * u[:, 1].double()], dim=1).float()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(ri.levels_from(u)[:, 1], torch.zeros(3))


def test_noise_refusals():
    for bad in (dict(kind="salt"), dict(kind="gaussian", gain=0.1), dict(kind="rician", gain=0.1), dict(kind="gaussian", sigma=-0.1),
                dict(kind="gaussian", sigma=math.inf), dict(kind="gaussian", sigma=math.nan), dict(kind="gaussian", sigma=(0.2, 0.1)),
                dict(kind="gaussian", sigma=(0.1, math.inf)), dict(kind="gaussian", sigma=(-0.1, 0.1)),
                dict(kind="gaussian", sigma=(0.1, 0.2, 0.3)), dict(kind="gaussian", sigma="0.1"), dict(kind="gaussian", sigma=True),
                dict(kind="poisson-gaussian", gain=-1), dict(kind="poisson-gaussian", blur=1), dict(kind="gaussian", clip=(1, 0)),
                dict(kind="gaussian", clip=(0, math.nan)), dict(kind="gaussian", clip=1.0), dict(kind="gaussian", clip=(0, 1, 2))):
        with pytest.raises(ValueError):
            D.Noise(**bad)
    with pytest.raises(TypeError):
        D.Noise.of(3)
    with pytest.raises(ValueError):
        D.Noise.of("speckle")
    with pytest.raises(RuntimeError):
        D.add_noise(torch.rand(1, 1, 8, 8), "gaussian")
    with pytest.raises(RuntimeError):
        D.noise_words(1, 4, 4, 1, device="cpu")
    with pytest.raises(ValueError):
        D.DevicePatchSampler(torch.rand(6, 1, 20, 24), 4, 4, noise="speckle", device="cpu")


def test_noise_from_paras():
    class P:
        pass
    assert D.Noise.from_paras(P()) is None
    P.noise_method = ""
    assert D.Noise.from_paras(P()) is None
    P.noise_method = None
    assert D.Noise.from_paras(P()) is None
    P.noise_method = "rician"
    assert D.Noise.from_paras(P()) == D.Noise("rician")
    P.noise_sigma, P.noise_gain, P.noise_clip = (0.01, 0.04), 0.5, (0.0, 1.0)
    assert D.Noise.from_paras(P()) == D.Noise("rician", sigma=(0.01, 0.04), clip=(0.0, 1.0))       # 'rician' takes no gain
    P.noise_method = "poisson-gaussian"
    assert D.Noise.from_paras(P()) == D.Noise("poisson-gaussian", sigma=(0.01, 0.04), gain=0.5, clip=(0.0, 1.0))
    P.noise_method = "speckle"
    with pytest.raises(ValueError):
        D.Noise.from_paras(P())


def _parent_sequence(g, S, B, H, W, hp, n_scales, n_variants):
    """What DevicePatchSampler.draw() asked of its generator before there was any noise."""
    k = int(torch.randint(n_scales, (1,), generator=g)) if n_scales > 1 else 0
    idx = torch.stack([torch.randperm(S, generator=g)[:B], torch.randint(0, H - hp[k] + 1, (B,), generator=g),
                       torch.randint(0, W - hp[k] + 1, (B,), generator=g)], dim=1).to(torch.int32)
    var = torch.randint(0, n_variants, (B,), generator=g).to(torch.int32) if n_variants else None
    return k, idx, var


@pytest.mark.parametrize("augment", [False, True, "flip"])
def test_generator_consumption(augment):
    S, B, lp, scales = 8, 5, 4, (2.0, 4.0)
    slices = torch.rand(S, 1, 30, 34)
    nv = {False: 0, True: 8, "flip": 4}[augment]
    noise = D.Noise("poisson-gaussian", gain=(0.0, 0.02), sigma=(0.01, 0.05))
    clean = D.DevicePatchSampler(slices, B, lp, sr_scales=scales, device="cpu", augment=augment, noise=None,
                                 generator=torch.Generator().manual_seed(3))
    noisy = D.DevicePatchSampler(slices, B, lp, sr_scales=scales, device="cpu", augment=augment, noise=noise,
                                 generator=torch.Generator().manual_seed(3))
    assert clean.noise is None and noisy.noise == noise
    g_clean, g_noisy = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    hp = [int(lp * s) for s in scales]
    for _ in range(4):
        # noise=None: exactly the parent's sequence, and the fields default to None
        k, idx, var = _parent_sequence(g_clean, S, B, 30, 34, hp, 2, nv)
        d = clean.draw()
        assert d.sr_factor == scales[k] and torch.equal(d.indices, idx) and d.noise_seed is None and d.noise_levels is None
        assert (d.variants is None) == (var is None) and (var is None or torch.equal(d.variants, var))
        # a noisy sampler: the same origins and variants first, then one 64-bit seed and rand(B, 2), nothing else
        k, idx, var = _parent_sequence(g_noisy, S, B, 30, 34, hp, 2, nv)
        seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64, generator=g_noisy)) & ((1 << 64) - 1)
        u = torch.rand(B, 2, generator=g_noisy)
        d = noisy.draw()
        assert d.sr_factor == scales[k] and torch.equal(d.indices, idx)
        assert (d.variants is None) == (var is None) and (var is None or torch.equal(d.variants, var))
        assert d.noise_seed == seed and 0 <= d.noise_seed < 1 << 64
        want = torch.stack([0.02 * u[:, 0].double(), 0.01 + 0.04 * u[:, 1].double()], dim=1).float()
        assert d.noise_levels.dtype == torch.float32 and torch.equal(d.noise_levels, want)
    assert torch.equal(clean.generator.get_state(), g_clean.get_state())
    assert torch.equal(noisy.generator.get_state(), g_noisy.get_state())


def test_draw_defaults():
    d = D.Draw(4.0, 16, torch.zeros(2, 3, dtype=torch.int32))
    assert d.variants is None and d.noise_seed is None and d.noise_levels is None
    assert D.Draw._fields == ("sr_factor", "hr_patch_size", "indices", "variants", "noise_seed", "noise_levels")
    d = D.Draw(4.0, 16, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))      # positional, as before
    assert d.variants is not None and d.noise_seed is None


@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("augment", [False, True])
def test_packing_of_the_host_buffer(B, augment):
    """One buffer: the index table, the variants, a pad word where needed, the seed on an 8-byte boundary, the levels."""
    vo, so, lo, total = D.DevicePatchSampler._layout(B, augment, True)
    assert vo == (3 * B if augment else None) and so % 2 == 0 and lo == so + 2 and total == lo + 2 * B
    assert so - (4 * B if augment else 3 * B) in (0, 1)
    assert D.DevicePatchSampler._layout(B, augment, False) == (vo, None, None, 4 * B if augment else 3 * B)
    s = D.DevicePatchSampler(torch.rand(8, 1, 30, 34), B, 4, device="cpu", augment=augment, noise=D.Noise("rician", sigma=(0.0, 0.1)),
                             generator=torch.Generator().manual_seed(5))
    d = s.draw()
    both, lay = s._packed(d)
    assert lay == (vo, so, lo, total) and both is d.indices._base and both.dtype == torch.int32 and tuple(both.shape) == (total,)

    def check(buf, draw):
        assert torch.equal(buf[:3 * B].view(B, 3), draw.indices.to(torch.int32))
        if augment:
            assert torch.equal(buf[vo:vo + B], draw.variants.to(torch.int32))
        raw = buf[so:so + 2].numpy().view(np.uint64)[0]
        assert int(raw) == draw.noise_seed
        assert torch.equal(buf[lo:].view(torch.float32).view(B, 2), draw.noise_levels)
        assert (buf.data_ptr() + 4 * so) % 8 == 0
    check(both, d)
    # forced tables: packed anew, under the same layout; a seed with its top bit set survives
    forced = D.Draw(d.sr_factor, d.hr_patch_size, d.indices.clone(), d.variants.clone() if augment else None, (1 << 63) + 12345,
                    torch.rand(B, 2))
    b2, lay2 = s._packed(forced)
    assert lay2 == lay and b2 is not both
    check(b2, forced)
    # a draw whose seed was replaced is not served from the stale buffer
    swapped = d._replace(noise_seed=77)
    b3, _ = s._packed(swapped)
    assert b3 is not both
    check(b3, swapped)
    with pytest.raises(ValueError):
        s._packed(d._replace(noise_levels=torch.rand(B, 3)))


def test_a_noisy_sampler_on_the_host_draws_but_does_not_sample():
    s = D.DevicePatchSampler(torch.rand(8, 1, 30, 34), 4, 4, device="cpu", noise="gaussian")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        s.sample()


def test_binding_comes_from_the_noise_header():
    assert set(_lib.NOISE_SIGNATURES) == {"rdst_noise_words", "rdst_add_noise", "rdst_sample_patches_noise"}
    for other in (_lib.SIGNATURES, _lib.DATA_SIGNATURES, _lib.LRC_SIGNATURES, _lib.MSSSIM_SIGNATURES):
        assert not set(_lib.NOISE_SIGNATURES) & set(other)
    assert _lib.NOISE_PARAMS["rdst_noise_words"] == ("out", "planes", "H", "W", "seed", "stream")
    assert _lib.NOISE_PARAMS["rdst_add_noise"] == ("x", "y", "N", "C", "H", "W", "model", "levels", "seed", "clip_lo", "clip_hi", "stream")
    assert _lib.NOISE_PARAMS["rdst_sample_patches_noise"] == _lib.DATA_PARAMS["rdst_sample_patches_op"][:-1] + (
        "model", "levels", "seed", "clip_lo", "clip_hi", "stream")
    V, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.NOISE_SIGNATURES["rdst_noise_words"] == (I, [V, I, I, I, V, V])
    assert _lib.NOISE_SIGNATURES["rdst_add_noise"] == (I, [V, V, I, I, I, I, I, V, V, Fl, Fl, V])
    assert _lib.NOISE_SIGNATURES["rdst_sample_patches_noise"] == (I, _lib.DATA_SIGNATURES["rdst_sample_patches_op"][1][:-1]
                                                                  + [I, V, V, Fl, Fl, V])
    lib = _lib.load()
    for name, (res, args) in _lib.NOISE_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert _lib.ABI_VERSION == lib.rdst_abi_version()


def test_c_entry_points_refuse_before_any_launch():
    """Pointers here are host memory nobody may follow on the device: every call must return before a launch."""
    lib = _lib.load()
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 63) & ~63
    P, ODD = base, base + 4                       # a 16-byte aligned address and one that is not
    inf, nan = math.inf, math.nan

    def words(**kw):
        a = dict(out=P, planes=2, H=8, W=8, seed=P)
        a.update(kw)
        return lib.rdst_noise_words(a["out"], a["planes"], a["H"], a["W"], a["seed"], None)
    for kw in (dict(out=None), dict(seed=None), dict(planes=0), dict(H=0), dict(W=-1), dict(out=ODD),
               dict(planes=1 << 20, H=1 << 12, W=1 << 12), dict(planes=0x7fffffff, H=0x7fffffff, W=0x7fffffff)):
        assert words(**kw) == _lib.EINVAL, kw
    assert words(seed=None) == _lib.EINVAL and b"seed" in lib.rdst_last_error()
    assert words(out=ODD) == _lib.EINVAL and b"16-byte aligned" in lib.rdst_last_error()
    assert words(planes=1 << 20, H=1 << 12, W=1 << 12) == _lib.EINVAL and b"too many for one launch" in lib.rdst_last_error()

    def add(**kw):
        a = dict(x=P, y=P, N=2, C=1, H=8, W=8, model=0, levels=P, seed=P, lo=-inf, hi=inf)
        a.update(kw)
        return lib.rdst_add_noise(a["x"], a["y"], a["N"], a["C"], a["H"], a["W"], a["model"], a["levels"], a["seed"], a["lo"],
                                  a["hi"], None)
    for kw in (dict(x=None), dict(y=None), dict(N=0), dict(C=0), dict(H=-2), dict(W=0), dict(levels=None), dict(seed=None),
               dict(model=2), dict(model=-1), dict(lo=1.0, hi=0.0), dict(lo=nan), dict(hi=nan), dict(lo=inf, hi=-inf),
               dict(N=1 << 16, C=1 << 16), dict(N=1 << 10, C=1 << 10, H=1 << 12, W=1 << 12),
               dict(N=0x7fffffff, C=1, H=0x7fffffff, W=0x7fffffff)):
        assert add(**kw) == _lib.EINVAL, kw
    assert add(levels=None) == _lib.EINVAL and b"levels" in lib.rdst_last_error()
    assert add(seed=None) == _lib.EINVAL and b"seed" in lib.rdst_last_error()
    assert add(model=2) == _lib.EINVAL and b"model" in lib.rdst_last_error()
    assert add(lo=1.0, hi=0.0) == _lib.EINVAL and b"clip_lo" in lib.rdst_last_error()
    assert add(hi=nan) == _lib.EINVAL and b"NaN" in lib.rdst_last_error()
    assert add(N=1 << 10, C=1 << 10, H=1 << 12, W=1 << 12) == _lib.EINVAL and b"too many for one launch" in lib.rdst_last_error()

    def op(**kw):
        a = dict(stack=P, labels=None, index=P, variant=None, hr=P, lr=P, label_out=None, S=4, C=1, H=20, W=30, B=2, hp=16,
                 lp=4, K=12, ti=P, tw=P, model=1, levels=P, seed=P, lo=0.0, hi=1.0)
        a.update(kw)
        return lib.rdst_sample_patches_noise(a["stack"], a["labels"], a["index"], a["variant"], a["hr"], a["lr"], a["label_out"],
                                             a["S"], a["C"], a["H"], a["W"], a["B"], a["hp"], a["lp"], a["K"], a["ti"], a["tw"],
                                             a["model"], a["levels"], a["seed"], a["lo"], a["hi"], None)
    # the refusals of rdst_sample_patches_op ...
    for kw in (dict(S=0), dict(C=0), dict(B=0), dict(lp=0), dict(hp=-1), dict(stack=None), dict(index=None), dict(hr=None),
               dict(lr=None), dict(ti=None), dict(tw=None), dict(K=0), dict(K=10), dict(K=-4), dict(ti=ODD), dict(tw=ODD),
               dict(labels=P), dict(label_out=P), dict(B=1 << 21)):
        assert op(**kw) == _lib.EINVAL, kw
    assert op(hp=24) == _lib.EINVAL and b"rdst_sample_patches_noise" in lib.rdst_last_error() and b"does not fit" in lib.rdst_last_error()
    assert op(labels=P) == _lib.EINVAL and b"go together" in lib.rdst_last_error()
    assert op(K=6) == _lib.EINVAL and b"multiple of 4" in lib.rdst_last_error()
    assert op(B=1 << 21) == _lib.EINVAL and b"too large for one launch" in lib.rdst_last_error()
    assert op(S=1, H=6000, W=6000, B=1, hp=6000, lp=1500) == _lib.ENOTSUP and b"LDS" in lib.rdst_last_error()
    # ... and its own
    for kw in (dict(levels=None), dict(seed=None), dict(model=2), dict(model=-1), dict(lo=1.0, hi=0.0), dict(lo=nan), dict(hi=nan)):
        assert op(**kw) == _lib.EINVAL, kw
    assert op(levels=None) == _lib.EINVAL and b"levels" in lib.rdst_last_error()
    assert op(seed=None) == _lib.EINVAL and b"seed" in lib.rdst_last_error()
    assert op(model=7) == _lib.EINVAL and b"model" in lib.rdst_last_error()
    assert op(lo=0.5, hi=0.25) == _lib.EINVAL and b"clip_lo" in lib.rdst_last_error()
