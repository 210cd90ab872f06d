"""CPU: the degradations of the device data path as tables (rdst_amd.data.operator_table, Degradation) against independent
float64 references, the properties a table promises the kernels, the error gate of tests/test_degrade_gpu.py held against
mutated operators, the Python argument handling, and every refusal of the two C entry points of include/rdst_hip_data.h
(returned before any launch: the library loads without a GPU)."""
import ctypes

import numpy as np
import pytest
import scipy.signal
import torch
import torch.nn.functional as F

from rdst_amd import _lib
from rdst_amd import data as D

NEW_KINDS = ("cubic+gaussian", "cubic_aa", "fourier")
SIZES = [(16, 4), (24, 8), (20, 6), (18, 5), (15, 4)]
GATE = 1e-13            # absolute, inputs in [0, 1]
U = 2.0 ** -24          # the unit roundoff of fp32


def dense(kind, n_in, n_out, **opts):
    """The table as a matrix (n_out, n_in), float64."""
    index, weight = D.operator_table(kind, n_in, n_out, **opts)
    M = np.zeros((n_out, n_in))
    np.add.at(M, (np.arange(n_out)[:, None], index), weight)
    return M


def gaussian_taps(k, sigma):
    if sigma <= 0:
        return {3: [.25, .5, .25], 5: [.0625, .25, .375, .25, .0625],
                7: [.03125, .109375, .21875, .28125, .21875, .109375, .03125]}[k]
    w = [np.exp(-((i - (k - 1) / 2) ** 2) / (2 * sigma * sigma)) for i in range(k)]
    return [v / sum(w) for v in w]


def reference(kind, x, oh, ow, k=3, sigma=0.0):
    """The degradation of a float64 image (H, W) by means that share nothing with operator_table."""
    xt = torch.from_numpy(x)[None, None]
    if kind == "cubic":
        return F.interpolate(xt, size=(oh, ow), mode="bicubic", align_corners=False)[0, 0].numpy()
    if kind == "cubic_aa":
        return F.interpolate(xt, size=(oh, ow), mode="bicubic", align_corners=False, antialias=True)[0, 0].numpy()
    if kind == "cubic+gaussian":
        r = F.interpolate(xt, size=(oh, ow), mode="bicubic", align_corners=False)
        g = torch.tensor(gaussian_taps(k, sigma), dtype=torch.float64)
        p = k // 2
        return F.conv2d(F.pad(r, (p, p, p, p), mode="reflect"), (g[:, None] * g[None, :])[None, None])[0, 0].numpy()
    return scipy.signal.resample(scipy.signal.resample(x, oh, axis=0), ow, axis=1)


def bound(kind, n_in_y, oh, n_in_x, ow, xmax):
    """The bound of tests/test_degrade_gpu.py, per pixel: gamma * Sy[oy] * Sx[ox] * max|x|, gamma = n u / (1 - n u), n = Ky +
    Kx + 2: two chained fp32 dot products (Kx, then Ky roundings at most) with once-rounded weights (one more each)."""
    (iy, wy), (ix, wx) = D.operator_table(kind, n_in_y, oh), D.operator_table(kind, n_in_x, ow)
    n = iy.shape[1] + ix.shape[1] + 2
    gamma = n * U / (1 - n * U)
    return gamma * np.abs(wy).sum(1)[:, None] * np.abs(wx).sum(1)[None, :] * xmax


@pytest.mark.parametrize("kind,n_in,n_out", [(k, *sz) for k in D.KINDS for sz in SIZES] + [("fourier", 256, 64)])
def test_tables_against_float64_references(kind, n_in, n_out):
    rng = np.random.default_rng(n_in * 100 + n_out)
    x = rng.random((n_in, n_in + 3 if n_in < 256 else n_in))      # H != W: both axes' tables
    My, Mx = dense(kind, x.shape[0], n_out), dense(kind, x.shape[1], n_out + 1 if n_in < 256 else n_out)
    err = np.abs(My @ x @ Mx.T - reference(kind, x, My.shape[0], Mx.shape[0])).max()
    print(f"[table] {kind} {n_in} -> {n_out}: max|d| = {err:.3e}")
    assert err <= GATE


@pytest.mark.parametrize("k,sigma", [(5, 0.0), (7, 0.0), (3, 1.3), (5, 1.3), (7, 1.3)])
def test_gaussian_options_against_an_explicit_convolution(k, sigma):
    rng = np.random.default_rng(k)
    x = rng.random((24, 20))
    My = dense("cubic+gaussian", 24, 8, blur_kernel=k, blur_sigma=sigma)
    Mx = dense("cubic+gaussian", 20, 6, blur_kernel=k, blur_sigma=sigma)
    assert np.abs(My @ x @ Mx.T - reference("cubic+gaussian", x, 8, 6, k, sigma)).max() <= GATE
    assert D.Degradation("cubic+gaussian", blur_kernel=k, blur_sigma=sigma) != D.Degradation("cubic+gaussian")


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("n_in,n_out", SIZES + [(256, 64), (16, 8), (32, 8)])
def test_table_properties(kind, n_in, n_out):
    index, weight = D.operator_table(kind, n_in, n_out)
    K = index.shape[1]
    assert index.dtype == np.int32 and weight.dtype == np.float64 and index.shape == weight.shape == (n_out, K)
    assert K % 4 == 0 and K >= 4
    assert index.min() >= 0 and index.max() <= n_in - 1
    assert np.abs(weight.sum(1) - 1).max() <= 4 * 2.0 ** -52
    if kind == "cubic":
        ti, tw = D.tap_table(n_in, n_out)
        assert np.array_equal(index, ti) and np.array_equal(weight, tw)
        assert (np.diff(index, axis=1) >= 0).all()
        return
    if kind == "fourier":
        assert K == -(-n_in // 4) * 4
    longest = 0
    for o in range(n_out):
        d = np.diff(index[o])
        real = 1 + int((d > 0).sum())                  # strictly ascending taps, then the last index again
        assert (d[:real - 1] > 0).all() and (d[real - 1:] == 0).all()
        assert (weight[o, real:] == 0).all()
        longest = max(longest, real)
    assert K == -(-longest // 4) * 4                   # no wider than the longest row needs


def test_dyadic_weights_for_the_exact_gpu_cases():
    """What tests/test_degrade_gpu.py's exact cases rest on.  'cubic+gaussian' at ratio 4: every weight a multiple of 1/128
    (blur_kernel = 3; 1/512 with 5, 1/2048 with 7).  'cubic_aa' at 16 -> 8: multiples of 1/256 on the rows 2..5, whose windows lie
    inside the signal; the rows 0, 1, 6, 7 are cut at the border and renormalised by 239/128 and the like, so they are not
    dyadic, and since a shrinking window (half-width 2 scale >= 2) always reaches past sample 0 at row 0, no size other than
    n_out == n_in (the identity) has only dyadic rows.  The GPU test therefore holds the interior outputs exact."""
    for k, den in ((3, 128), (5, 512), (7, 2048)):
        _, w = D.operator_table("cubic+gaussian", 32, 8, blur_kernel=k)
        assert np.array_equal(w * den, np.round(w * den))
    _, w = D.operator_table("cubic_aa", 16, 8)
    dyadic = (w * 256 == np.round(w * 256)).all(axis=1)
    assert dyadic.tolist() == [False, False, True, True, True, True, False, False]
    _, w = D.operator_table("cubic_aa", 16, 16)
    assert np.array_equal(w[:, 0], np.ones(16)) and (w[:, 1:] == 0).all()


@pytest.mark.parametrize("lo", [0.0, 100.0], ids=["unit", "offcentre"])
@pytest.mark.parametrize("kind,n_in,n_out", [(k, 32, 8) for k in NEW_KINDS] + [("cubic", 32, 8), ("fourier", 256, 64)])
def test_the_error_gate_refuses_mutated_operators(kind, n_in, n_out, lo):
    """The derived bound on the test's own inputs: the float64 operator with one tap dropped from one row, and with two
    neighbouring weights swapped, must violate it somewhere; the float64 result of the fp32-rounded weights must keep it."""
    rng = np.random.default_rng(5)
    x = lo + rng.random((n_in, n_in))
    index, weight = D.operator_table(kind, n_in, n_out)
    M = dense(kind, n_in, n_out)
    ref = M @ x @ M.T
    b = bound(kind, n_in, n_out, n_in, n_out, np.abs(x).max())

    def mat(w):
        A = np.zeros((n_out, n_in))
        np.add.at(A, (np.arange(n_out)[:, None], index), w)
        return A
    rounded = mat(weight.astype(np.float32).astype(np.float64))
    assert (np.abs(rounded @ x @ rounded.T - ref) <= b).all()
    row = n_out // 2
    # a tap of the middle row's median magnitude, and the two neighbours that differ most swapped.  (A dropped tap of weight w
    # moves an output by about |w| max|x|, so the gate sees taps down to gamma Sy Sx in weight: 1e-6 for 12 taps, 3e-4 for the
    # dense 256-tap rows, whose smallest taps, 1e-5, lie below what fp32 chains of that length resolve.)
    real = np.flatnonzero(weight[row])
    drop = weight.copy()
    drop[row, real[np.argsort(np.abs(weight[row, real]))[len(real) // 2]]] = 0.0
    swap = weight.copy()
    p = int(np.argmax(np.abs(np.diff(weight[row, real]))))
    swap[row, [real[p], real[p + 1]]] = swap[row, [real[p + 1], real[p]]]
    for name, w in (("drop", drop), ("swap", swap)):
        A = mat(w)
        worst = (np.abs(A @ x @ M.T - ref) / b).max()       # the rows of the y operator mutated
        print(f"[gate] {kind} {n_in}->{n_out} lo={lo} {name}: worst |d| / bound = {worst:.3e}")
        assert worst > 1.0


def test_degradation_value():
    d = D.Degradation("cubic+gaussian", blur_sigma=1.3)
    assert d == D.Degradation("cubic+gaussian", blur_kernel=3, blur_sigma=1.3) and hash(d) == hash(D.Degradation.of(d))
    assert repr(d) == "Degradation('cubic+gaussian', blur_kernel=3, blur_sigma=1.3)"
    assert D.Degradation() == D.Degradation.of("cubic") and D.Degradation.of("fourier").kind == "fourier"
    assert len({D.Degradation("cubic_aa"), D.Degradation.of("cubic_aa"), D.Degradation("fourier")}) == 2
    with pytest.raises(AttributeError):
        d.kind = "cubic"

    class P:
        blur_method = None
    assert D.Degradation.from_paras(P()) == D.Degradation("cubic")
    P.blur_method = ""
    assert D.Degradation.from_paras(P()) == D.Degradation("cubic")
    P.blur_method = "gaussian"
    assert D.Degradation.from_paras(P()) == D.Degradation("cubic+gaussian")
    P.blur_kernel, P.blur_sigma = 5, 1.5
    assert D.Degradation.from_paras(P()) == D.Degradation("cubic+gaussian", blur_kernel=5, blur_sigma=1.5)
    P.blur_method = "median"
    with pytest.raises(ValueError):
        D.Degradation.from_paras(P())


def test_python_refusals():
    with pytest.raises(ValueError):
        D.Degradation("lanczos")
    with pytest.raises(ValueError):
        D.operator_table("box", 16, 4)
    for bad in (4, 2, 9, 1, 3.0):
        with pytest.raises(ValueError):
            D.Degradation("cubic+gaussian", blur_kernel=bad)
    with pytest.raises(ValueError):
        D.Degradation("fourier", blur_kernel=3)
    with pytest.raises(ValueError):
        D.operator_table("fourier", 8, 16)
    with pytest.raises(ValueError):
        D.operator_table("cubic+gaussian", 8, 1)
    with pytest.raises(ValueError):
        D.operator_table("cubic_aa", 0, 4)
    with pytest.raises(TypeError):
        D.Degradation.of(3)
    with pytest.raises(RuntimeError):
        D.resample(torch.rand(1, 1, 8, 8), 4, "cubic_aa")
    with pytest.raises(ValueError):
        D.resample(torch.rand(1, 1, 8, 8), 4, "nearest")
    slices = torch.rand(6, 1, 20, 24)
    with pytest.raises(ValueError, match=r"degradation='cubic\+gaussian'.*from_paras"):
        D.DevicePatchSampler(slices, 4, 4, blur_method="gaussian", device="cpu")
    with pytest.raises(ValueError):
        D.DevicePatchSampler(slices, 4, 4, degradation="sinc", device="cpu")
    with pytest.raises(ValueError):
        D.DevicePatchSampler(slices, 4, 1, degradation="cubic+gaussian", device="cpu")      # an LR patch of one pixel
    s = D.DevicePatchSampler(slices, 4, 4, degradation="cubic", device="cpu")
    assert s.degradation is None                                                            # the 4-tap entry points
    s = D.DevicePatchSampler(slices, 4, 4, degradation="fourier", device="cpu")
    assert s.degradation == D.Degradation("fourier")


def test_sampler_draws_do_not_depend_on_the_degradation():
    slices = torch.rand(8, 1, 30, 34)
    draws = []
    for deg in (None, "cubic", "cubic_aa"):
        s = D.DevicePatchSampler(slices, 4, 4, sr_scales=(2.0, 4.0), device="cpu", augment=True, degradation=deg,
                                 generator=torch.Generator().manual_seed(3))
        draws.append([s.draw() for _ in range(4)])
    for a, b in zip(draws[0], draws[1]):
        assert a.sr_factor == b.sr_factor and torch.equal(a.indices, b.indices) and torch.equal(a.variants, b.variants)
    for a, b in zip(draws[0], draws[2]):
        assert a.sr_factor == b.sr_factor and torch.equal(a.indices, b.indices) and torch.equal(a.variants, b.variants)


def test_binding_comes_from_the_second_header():
    assert set(_lib.DATA_SIGNATURES) == {"rdst_resample_sep", "rdst_sample_patches_op"}
    assert not set(_lib.DATA_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.DATA_PARAMS["rdst_resample_sep"] == ("x", "y", "tmp", "N", "C", "H", "W", "oh", "ow", "Ky", "index_y", "weight_y",
                                                     "Kx", "index_x", "weight_x", "stream")
    assert _lib.DATA_PARAMS["rdst_sample_patches_op"] == ("stack", "labels", "index", "variant", "hr", "lr", "label_out", "S", "C",
                                                          "H", "W", "B", "hp", "lp", "K", "tap_index", "tap_weight", "stream")
    lib = _lib.load()
    for name, (res, args) in _lib.DATA_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_c_entry_points_refuse_before_any_launch():
    """Pointers here are host memory or small integers nobody may follow: every call must return before a launch."""
    lib = _lib.load()
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 63) & ~63
    P, ODD = base, base + 4                       # a 16-byte aligned address and one that is not

    def sep(**kw):
        a = dict(x=P, y=P, tmp=P, N=1, C=1, H=8, W=8, oh=4, ow=4, Ky=4, iy=P, wy=P, Kx=4, ix=P, wx=P)
        a.update(kw)
        return lib.rdst_resample_sep(a["x"], a["y"], a["tmp"], a["N"], a["C"], a["H"], a["W"], a["oh"], a["ow"], a["Ky"], a["iy"],
                                     a["wy"], a["Kx"], a["ix"], a["wx"], None)
    for kw in (dict(N=0), dict(H=0), dict(ow=-1), dict(x=None), dict(y=None), dict(tmp=None), dict(iy=None), dict(wy=None),
               dict(ix=None), dict(wx=None), dict(Ky=0), dict(Ky=6), dict(Kx=5), dict(Kx=-4), dict(iy=ODD), dict(wy=ODD),
               dict(ix=ODD), dict(wx=ODD)):
        assert sep(**kw) == _lib.EINVAL, kw
    assert sep(Kx=6) == _lib.EINVAL and b"multiple of 4" in lib.rdst_last_error()
    assert sep(wx=ODD) == _lib.EINVAL and b"16-byte aligned" in lib.rdst_last_error()

    def op(**kw):
        a = dict(stack=P, labels=None, index=P, variant=None, hr=P, lr=P, label_out=None, S=4, C=1, H=20, W=30, B=2, hp=16,
                 lp=4, K=12, ti=P, tw=P)
        a.update(kw)
        return lib.rdst_sample_patches_op(a["stack"], a["labels"], a["index"], a["variant"], a["hr"], a["lr"], a["label_out"],
                                          a["S"], a["C"], a["H"], a["W"], a["B"], a["hp"], a["lp"], a["K"], a["ti"], a["tw"], None)
    for kw in (dict(S=0), dict(C=0), dict(B=0), dict(lp=0), dict(hp=-1), dict(stack=None), dict(index=None), dict(hr=None),
               dict(lr=None), dict(ti=None), dict(tw=None), dict(K=0), dict(K=10), dict(K=-4), dict(ti=ODD), dict(tw=ODD),
               dict(labels=P), dict(label_out=P), dict(B=1 << 21)):
        assert op(**kw) == _lib.EINVAL, kw
    assert op(hp=24) == _lib.EINVAL and b"does not fit" in lib.rdst_last_error()          # taller than the slice
    assert op(H=40, hp=32) == _lib.EINVAL and b"does not fit" in lib.rdst_last_error()    # wider than the slice
    assert op(labels=P) == _lib.EINVAL and b"go together" in lib.rdst_last_error()
    assert op(K=6) == _lib.EINVAL and b"multiple of 4" in lib.rdst_last_error()
    # one LR column of horizontal sums and one staged row past the 64 KB of LDS
    assert op(S=1, H=6000, W=6000, B=1, hp=6000, lp=1500) == _lib.ENOTSUP and b"LDS" in lib.rdst_last_error()
