"""Training batches and test pairs made on the device: the data side of the reference's trainer around the HIP hot path.

The reference builds every batch on the CPU (``BasicMultiSRTrain.__getitem__``, datasets/basic_dataset.py:190-217:
``batch_size`` random slices, one random HR crop each, ``cv2.resize(INTER_CUBIC)`` of every crop down to the LR patch, in
DataLoader workers, models/trans_sr_trainer.py:116-121) and copies it to the GPU (:143); the test side does the same to whole
slices (``get_test_pair``, basic_dataset.py:258-301).  The training volumes fit in device memory many times over, so here the
slices are moved to the GPU once and a batch is cut and degraded where it is consumed:

  * ``bicubic_resize(x, size)``      the resize itself (rdst_resize_bicubic, include/rdst_hip.h);
  * ``resample(x, size, degradation)``  the same under any ``Degradation``: a separable linear operator given as a table of K
                                     taps per output (``operator_table``; rdst_resample_sep, include/rdst_hip_data.h);
  * ``resample_adjoint(g, size, d)``  its adjoint, the same kernels under the transposed tables (``adjoint_table``);
                                     ``degrade`` is ``resample`` with that backward, ``operator_norm`` the spectral norm;
  * ``make_test_pair(hr, s)``        ``get_test_pair`` for one scale: what ``SRTester.evaluate`` / ``DPTrainStep.quick_eva`` take;
  * ``DevicePatchSampler``           ``__getitem__``: one HIP launch per batch (rdst_sample_patches), three random integers per
                                     patch drawn on the host, nothing read back; ``DPTrainStep.step_from(sampler)`` trains on it.
                                     ``augment=True`` adds the random flips and transposes of the EDSR / RCAN / SwinIR recipes
                                     (the eight of ``tiling.dihedral``, which the x8 self-ensemble averages over at test time),
                                     one more integer per patch and still one launch (rdst_sample_patches_d8).  The reference
                                     itself does not augment.

The resize is what ``cv2.resize(INTER_CUBIC)`` computes on float images and what ``torch.nn.functional.interpolate(
mode="bicubic", align_corners=False, antialias=False)`` computes: separable, four taps per axis, Keys kernel with a = -0.75,
source coordinate ``(dst + 0.5) * in / out - 0.5``, tap indices clamped to the image, no antialiasing, values not clamped (the
overshoot below 0 and above 1 is kept, basic_dataset.py:74).  **cv2 is not installed in the build image**: the tests pin the
resize to torch's float64 bicubic, and equality with cv2 is argued from its documented algorithm, not tested.

Degradations (``Degradation``, ``operator_table``): ``'cubic'`` is the resize above; ``'cubic+gaussian'`` the reference's
``blur_method='gaussian'`` (cv2.GaussianBlur of the resized image, basic_dataset.py:112-116); ``'cubic_aa'`` the antialiased
bicubic of Pillow / ``interpolate(antialias=True)`` behind the SwinIR / EDSR benchmark sets; ``'fourier'`` k-space truncation,
the low-resolution acquisition of MR slices.  Each is ``LR = A_y . patch . A_x^T`` with K taps per output; the sampler, the
whole-image resample and the test pair take any of them through one K-tap kernel family (csrc/resample.hip).

Noise (``Noise``, ``add_noise``, ``noise_words``; include/rdst_hip_noise.h): the second term of ``LR = A(HR) + n``, the detector
where the operator is the acquisition geometry: ``'gaussian'``, ``'poisson-gaussian'`` (signal-dependent, CT and photon-limited
images) and ``'rician'`` (magnitude MRI).  The reference has no noise option; it is off by default and no gain in trained models
is claimed.  The field is counter-based (Philox4x32-10 keyed by one 64-bit seed, one call per pixel at its own (plane, y, x)), so
the sampler applies it in its one launch and the whole-image ``add_noise`` returns the same bits; the seed and the per-patch
levels come from the sampler's CPU generator like everything else that is random.

One of each on the host side: the whole-image calls check their input through ``_whole_images``; every device table is
``_on_device`` of its host table (``tap_table``, ``operator_table``, ``adjoint_table``), cached per arguments and device;
``Degradation`` and ``Noise`` are ``_Frozen`` values; and every draw, plain or not, is the one pinned buffer ``_layout``
describes, which ``sample()`` copies to the device once and from which the four C entry points are chosen as before.

Out of scope, and refused where they could be asked for: augmentation other than the eight flips / transposes,
``return_res_image``, reading volumes from disk.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

A_KEYS = -0.75   # the cubic-convolution parameter of cv2.INTER_CUBIC and of torch's bicubic


def tap_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """The 1-D operator of the resize of ``n_in`` samples to ``n_out``: ``(index, weight)``, int32 and float64 ``(n_out, 4)``,
    taps in ascending order, indices clamped to ``[0, n_in - 1]``.  The source coordinate ``(o + 0.5) n_in / n_out - 0.5`` is
    split exactly, in integers, into its floor and the fraction ``t`` (one rounding); the weights are the Keys polynomials in
    ``t`` with the last one taken as ``1 - w0 - w1 - w2``, as cv2 takes it, so every row sums to 1 to the last bit or two."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"tap_table: sizes must be positive, got {n_in} -> {n_out}")
    o = np.arange(n_out, dtype=np.int64)
    num = (2 * o + 1) * n_in - n_out              # source coordinate = num / (2 n_out)
    base = num // (2 * n_out)                     # its floor (numpy floors negative quotients too)
    t = (num - base * (2 * n_out)).astype(np.float64) / float(2 * n_out)
    a = A_KEYS
    w0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    w1 = ((a + 2) * t - (a + 3)) * t * t + 1
    u = 1 - t
    w2 = ((a + 2) * u - (a + 3)) * u * u + 1
    w3 = 1.0 - w0 - w1 - w2
    index = np.clip(base[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], 0, n_in - 1).astype(np.int32)
    return index, np.stack([w0, w1, w2, w3], axis=1)


_TABLES: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def _on_device(table, device: torch.device, *args) -> Tuple[torch.Tensor, torch.Tensor]:
    """``table(*args)`` on the device, the weights rounded once to fp32; cached per (table, arguments, device)."""
    key = (table, *args, device.type, device.index)
    tab = _TABLES.get(key)
    if tab is None:
        index, weight = table(*args)
        tab = _TABLES[key] = (torch.from_numpy(np.ascontiguousarray(index)).to(device),
                              torch.from_numpy(weight.astype(np.float32)).to(device))
    return tab


def _device_table(n_in: int, n_out: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tap_table`` on the device; cached per (in, out, device)."""
    return _on_device(tap_table, device, int(n_in), int(n_out))


# ---- degradations as K-tap tables ------------------------------------------------------------------------------------------
KINDS = ("cubic", "cubic+gaussian", "cubic_aa", "fourier")
A_KEYS_AA = -0.5   # the cubic-convolution parameter of Pillow's BICUBIC and of torch's antialiased bicubic
# cv2.getGaussianKernel's fixed tables for sigma <= 0 (ksize 3, 5, 7)
_CV2_SMALL_GAUSSIAN = {3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
                       7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}
_OPTS = {"cubic": {}, "cubic+gaussian": {"blur_kernel": 3, "blur_sigma": 0.0}, "cubic_aa": {}, "fourier": {}}


class _Frozen:
    """A frozen, hashable value: ``kind``, ``opts`` (a sorted tuple of pairs) and whatever else the subclass names in
    ``__slots__``, set once by ``_freeze``.  A kind's name is accepted wherever the value is (``of``)."""
    __slots__ = ()

    def _freeze(self, *fields):
        for name, value in zip(self.__slots__, fields):
            object.__setattr__(self, name, value)

    def _key(self) -> tuple:
        return tuple(getattr(self, name) for name in self.__slots__)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is frozen")

    __delattr__ = __setattr__

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        more = [f"{name}={getattr(self, name)!r}" for name in self.__slots__[2:]]
        return type(self).__name__ + "(" + ", ".join([repr(self.kind)] + [f"{k}={v!r}" for k, v in self.opts] + more) + ")"

    @classmethod
    def of(cls, v):
        if isinstance(v, cls):
            return v
        if isinstance(v, str):
            return cls(v)
        raise TypeError(f"a {cls.__name__.lower()} is a {cls.__name__} or the name of a kind, not {type(v).__name__}")


class Degradation(_Frozen):
    """How an HR patch becomes its LR input: ``Degradation(kind='cubic', **opts)``, a frozen, hashable value.  A plain string
    is accepted wherever a ``Degradation`` is.  Kinds and options: ``'cubic'``; ``'cubic+gaussian'`` (``blur_kernel=3``: odd,
    3..7; ``blur_sigma=0``: cv2's fixed kernel if <= 0); ``'cubic_aa'``; ``'fourier'``.  ``operator_table`` defines them."""
    __slots__ = ("kind", "opts")

    def __init__(self, kind: str = "cubic", **opts):
        if kind not in KINDS:
            raise ValueError(f"Degradation: kind={kind!r} is not one of {KINDS}")
        known = _OPTS[kind]
        for k in opts:
            if k not in known:
                raise ValueError(f"Degradation: {kind!r} takes no option {k!r} (it takes {tuple(known) or 'none'})")
        full = {**known, **opts}
        if kind == "cubic+gaussian":
            bk = full["blur_kernel"]
            if isinstance(bk, bool) or not isinstance(bk, (int, np.integer)) or bk % 2 == 0 or not 3 <= bk <= 7:
                raise ValueError(f"Degradation: blur_kernel={bk!r} must be odd and in 3..7")
            sg = float(full["blur_sigma"])
            if not math.isfinite(sg):
                raise ValueError(f"Degradation: blur_sigma={full['blur_sigma']!r} must be finite")
            full = {"blur_kernel": int(bk), "blur_sigma": sg}
        self._freeze(kind, tuple(sorted(full.items())))

    @classmethod
    def from_paras(cls, paras) -> "Degradation":
        """``paras.blur_method`` of the reference's configuration (``None`` / ``''`` / ``'gaussian'``) as a ``Degradation``.
        ``paras.blur_kernel`` / ``paras.blur_sigma`` are taken where they exist."""
        bm = getattr(paras, "blur_method", None)
        if bm in (None, ""):
            return cls("cubic")
        if bm == "gaussian":
            opts = {k: getattr(paras, k) for k in ("blur_kernel", "blur_sigma") if getattr(paras, k, None) is not None}
            return cls("cubic+gaussian", **opts)
        raise ValueError(f"Degradation.from_paras: blur_method={bm!r} is not None, '' or 'gaussian'")


def _keys(x: np.ndarray, a: float) -> np.ndarray:
    """The cubic-convolution kernel of Keys with parameter ``a``."""
    x = np.abs(x)
    near = ((a + 2) * x - (a + 3)) * x * x + 1
    far = ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return np.where(x < 1, near, np.where(x < 2, far, 0.0))


def _reflect101(p: int, n: int) -> int:
    """cv2's BORDER_REFLECT_101 (-1 -> 1, n -> n - 2), repeated until the index is inside."""
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _cubic_matrix(n_in: int, n_out: int) -> np.ndarray:
    index, weight = tap_table(n_in, n_out)
    R = np.zeros((n_out, n_in))
    np.add.at(R, (np.arange(n_out)[:, None], index), weight)      # clamped taps meet on the border sample
    return R


def _gaussian_matrix(n: int, blur_kernel: int, blur_sigma: float) -> np.ndarray:
    if blur_sigma <= 0:
        g = np.array(_CV2_SMALL_GAUSSIAN[blur_kernel])
    else:
        d = np.arange(blur_kernel, dtype=np.float64) - (blur_kernel - 1) / 2
        g = np.exp(-(d * d) / (2.0 * blur_sigma * blur_sigma))
        g /= g.sum()
    G, half = np.zeros((n, n)), blur_kernel // 2
    for o in range(n):
        for t in range(blur_kernel):
            G[o, _reflect101(o + t - half, n)] += g[t]
    return G


def _aa_matrix(n_in: int, n_out: int) -> np.ndarray:
    scale = n_in / n_out
    s = max(scale, 1.0)
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        c = scale * (o + 0.5)
        lo, hi = max(int(c - 2 * s + 0.5), 0), min(int(c + 2 * s + 0.5), n_in)
        w = _keys((np.arange(lo, hi) + 0.5 - c) / s, A_KEYS_AA)
        M[o, lo:hi] = w / w.sum()
    return M


def _fourier_matrix(n_in: int, n_out: int) -> np.ndarray:
    X = np.fft.rfft(np.eye(n_in), axis=0)           # column i: the spectrum of the unit sample i
    Y = X[:n_out // 2 + 1].copy()
    if n_out % 2 == 0 and n_out < n_in:
        Y[n_out // 2] *= 2.0
    return np.fft.irfft(Y, n_out, axis=0) * (n_out / n_in)


def _table_of(M: np.ndarray, support: np.ndarray, empty_rows: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """A matrix (n_out, n_in) and the boolean mask of its taps -> ``(index, weight)`` of K columns.  A row without taps is
    refused, or with ``empty_rows`` left as weights 0.0 on index 0."""
    counts = support.sum(axis=1)
    if not empty_rows and counts.min() < 1:
        raise ValueError("operator_table: an output without taps")
    K = max(4, -(-int(counts.max()) // 4) * 4)
    index = np.zeros((M.shape[0], K), dtype=np.int32)
    weight = np.zeros((M.shape[0], K), dtype=np.float64)
    for o in range(M.shape[0]):
        j = np.flatnonzero(support[o])
        if len(j):
            index[o, :len(j)], index[o, len(j):] = j, j[-1]
            weight[o, :len(j)] = M[o, j]
    return index, weight


def _degradation_of(what: str, kind: Union[str, Degradation], opts: dict) -> Degradation:
    """``kind`` with its options, or a ``Degradation`` (and then no options)."""
    d = Degradation(kind, **opts) if isinstance(kind, str) else Degradation.of(kind)
    if not isinstance(kind, str) and opts:
        raise ValueError(f"{what}: options go with a kind's name, not with a Degradation")
    return d


def operator_table(kind: Union[str, Degradation], n_in: int, n_out: int, **opts) -> Tuple[np.ndarray, np.ndarray]:
    """The 1-D operator of a degradation along an axis of ``n_in`` samples, ``n_out`` outputs: ``(index, weight)``, int32 and
    float64 ``(n_out, K)``.  Taps stand in ascending source order, every source sample once (taps that clamping or reflection
    puts on one sample are merged), K is the longest row's number of taps rounded up to a multiple of 4, and a shorter row is
    padded at its end with weight 0.0 and its last real index.  ``kind`` is a name with its options, or a ``Degradation``.

    ``'cubic'``: ``tap_table``, as it is (K = 4, border taps not merged).

    ``'cubic+gaussian'``: ``G . R``, formed in float64: ``R`` the cubic operator ``n_in -> n_out`` and ``G`` the ``n_out x
    n_out`` blur ``cv2.GaussianBlur(img, (k, k), sigma)`` applies to the RESIZED image (basic_dataset.py:112-116): ``k =
    blur_kernel`` taps, border BORDER_REFLECT_101 (cv2's default: index -1 -> 1, n -> n - 2), weights cv2's fixed tables for
    ``sigma <= 0`` ([1 2 1] / 4, [1 4 6 4 1] / 16, [4 14 28 36 28 14 4] / 128: getGaussianKernel's small_gaussian_tab, used
    for ksize <= 7) and the normalised ``exp(-(i - c)^2 / (2 sigma^2))`` otherwise.  cv2.GaussianBlur is separable with that
    kernel on both axes, so the blurred resize is ``(G_y R_y) patch (G_x R_x)^T``.  **cv2 is not installed in the build
    image**: as for the resize, equality with cv2 is argued from its documented algorithm, and the tests pin the operator to
    a reflect-padded convolution of torch's float64 bicubic.  (cv2 rounds the resized image to fp32 before it blurs and sums in
    its own order; this operator rounds once, at the end.)  ``n_out < 2`` is refused (the border needs two samples).

    ``'cubic_aa'``: what ``F.interpolate(mode='bicubic', align_corners=False, antialias=True)`` and Pillow's BICUBIC compute.
    With ``scale = n_in / n_out``, ``s = max(scale, 1)`` and ``c = scale (o + 0.5)``, output ``o`` takes the samples ``lo =
    max(int(c - 2 s + 0.5), 0) .. hi = min(int(c + 2 s + 0.5), n_in)`` (exclusive) with the weights ``keys((j + 0.5 - c) / s)``,
    a = -0.5, divided by their sum: the window is cut at the border and renormalised, not clamped.  Samples of weight exactly
    0 (the window's ends) are not taps.

    ``'fourier'``: band-limited resampling, ``scipy.signal.resample``'s definition for real signals: the ``rfft`` of the axis,
    bins ``0 .. n_out // 2`` kept, the bin ``n_out // 2`` doubled when ``n_out`` is even and below ``n_in`` (it stands for the
    +- Nyquist pair of the short signal, so the operator is real), ``irfft`` to ``n_out`` samples, times ``n_out / n_in``.
    Dense: every sample is a tap, K = ``n_in`` rounded up to a multiple of 4; every row sums to 1.  Only ``n_out <= n_in``.
    A raw centred crop of k-space (``fftshift``, keep the middle ``n_out``, inverse transform) differs for even ``n_out``: it
    keeps the -Nyquist row alone, without its partner, so its result is complex and its real part carries half of that bin."""
    d = _degradation_of("operator_table", kind, opts)
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"operator_table: sizes must be positive, got {n_in} -> {n_out}")
    o = dict(d.opts)
    if d.kind == "cubic":
        return tap_table(n_in, n_out)
    if d.kind == "cubic+gaussian":
        if n_out < 2:
            raise ValueError(f"operator_table: 'cubic+gaussian' needs at least 2 outputs (BORDER_REFLECT_101), got {n_out}")
        R, G = _cubic_matrix(n_in, n_out), _gaussian_matrix(n_out, o["blur_kernel"], o["blur_sigma"])
        return _table_of(G @ R, ((G != 0).astype(np.int64) @ (R != 0).astype(np.int64)) > 0)
    if d.kind == "cubic_aa":
        M = _aa_matrix(n_in, n_out)
        return _table_of(M, M != 0)
    if n_out > n_in:
        raise ValueError(f"operator_table: 'fourier' only shrinks, got {n_in} -> {n_out}")
    M = _fourier_matrix(n_in, n_out)
    return _table_of(M, np.ones(M.shape, dtype=bool))


def _device_op_table(d: Degradation, n_in: int, n_out: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``operator_table`` on the device; cached per (kind, options, in, out, device)."""
    return _on_device(operator_table, device, d, int(n_in), int(n_out))


def _need_gpu(what: str, *ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"rdst_amd.data.{what}: the HIP path needs GPU tensors; there is no CPU fallback")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _pair(size) -> Tuple[int, int]:
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


@contextlib.contextmanager
def _whole_images(what: str, name: str, x, size=None):
    """The front end of the whole-image calls: ``x`` must be a float32 CUDA tensor of 3 or 4 dimensions outside autograd, and
    every size positive.  Yields ``(x as a contiguous (N, C, H, W), whether the result drops that N again, size as a pair)``
    with ``x``'s device current."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch tensor")
    _need_gpu(what, x)
    if x.requires_grad:
        raise RuntimeError(f"{what} is not differentiable: detach the input")
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be float32, got {x.dtype}")
    squeeze = x.dim() == 3
    x4 = x.unsqueeze(0) if squeeze else x
    if x4.dim() != 4:
        raise ValueError(f"{what}: {name} must have 3 or 4 dimensions")
    to = () if size is None else _pair(size)
    if min(*x4.shape, *to) <= 0:
        raise ValueError(f"{what}: sizes must be positive, got {tuple(x4.shape)}" + (f" -> {to}" if to else ""))
    with torch.cuda.device(x.device):
        yield x4.contiguous(), squeeze, to


def bicubic_resize(x: torch.Tensor, size) -> torch.Tensor:
    """fp32 CUDA ``(N, C, H, W)`` (or ``(C, H, W)``) -> a new tensor of spatial ``size`` (an int or ``(oh, ow)``), down or up.
    Not differentiable."""
    with _whole_images("bicubic_resize", "x", x, size) as (x, squeeze, (oh, ow)):
        N, C, H, W = x.shape
        iy, wy = _device_table(H, oh, x.device)
        ix, wx = _device_table(W, ow, x.device)
        y = torch.empty(N, C, oh, ow, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().rdst_resize_bicubic(x.data_ptr(), y.data_ptr(), N, C, H, W, oh, ow, iy.data_ptr(), wy.data_ptr(),
                                                   ix.data_ptr(), wx.data_ptr(), _stream()), "rdst_resize_bicubic")
    return y[0] if squeeze else y


def _resample_sep(what: str, name: str, x, size, table) -> torch.Tensor:
    """rdst_resample_sep of ``x`` to ``size`` under the tables ``table(n_in, n_out, device)`` of its two axes."""
    with _whole_images(what, name, x, size) as (x, squeeze, (oh, ow)):
        N, C, H, W = x.shape
        iy, wy = table(H, oh, x.device)
        ix, wx = table(W, ow, x.device)
        y = torch.empty(N, C, oh, ow, dtype=torch.float32, device=x.device)
        tmp = torch.empty(N * C * H * ow, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().rdst_resample_sep(x.data_ptr(), y.data_ptr(), tmp.data_ptr(), N, C, H, W, oh, ow, iy.shape[1],
                                                 iy.data_ptr(), wy.data_ptr(), ix.shape[1], ix.data_ptr(), wx.data_ptr(),
                                                 _stream()), "rdst_resample_sep")
    return y[0] if squeeze else y


def resample(x: torch.Tensor, size, degradation: Union[str, Degradation] = "cubic") -> torch.Tensor:
    """``bicubic_resize`` under any degradation: fp32 CUDA ``(N, C, H, W)`` (or ``(C, H, W)``) -> a new tensor of spatial
    ``size``, the operator ``operator_table(degradation, H, oh)`` along the rows and ``(W, ow)`` along the columns
    (rdst_resample_sep: the horizontal sums, then the vertical chains).  With ``'cubic'`` it gives ``bicubic_resize``'s bits.
    Not differentiable."""
    d = Degradation.of(degradation)
    return _resample_sep("resample", "x", x, size, lambda n_in, n_out, dev: _device_op_table(d, n_in, n_out, dev))


# ---- the adjoints of the K-tap operators --------------------------------------------------------------------------------
def _operator_matrix(d: Degradation, n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """The float64 matrix ``(n_out, n_in)`` of ``operator_table(d, n_in, n_out)`` and the boolean mask of its real taps.  Taps
    of one row that stand on one sample (the clamped border taps of ``'cubic'``; a padding tap of weight 0.0 on the row's
    last index) are added in float64; a tap whose weight is exactly 0.0 (three of the four of ``'cubic'`` at an integer ratio
    and an odd phase, 24 -> 8) is not a real tap."""
    index, weight = operator_table(d, n_in, n_out)
    M = np.zeros((index.shape[0], int(n_in)), dtype=np.float64)
    rows = np.arange(index.shape[0])[:, None]
    np.add.at(M, (rows, index), weight)
    support = np.zeros(M.shape, dtype=bool)
    support[rows, index] = True
    return M, support & (M != 0)


def adjoint_table(kind: Union[str, Degradation], n_in: int, n_out: int, **opts) -> Tuple[np.ndarray, np.ndarray]:
    """The table of ``A^T`` for ``A = operator_table(kind, n_in, n_out)``: ``(index, weight)``, int32 and float64 ``(n_in,
    Kt)`` over ``[0, n_out)``, in ``operator_table``'s format: the taps of source sample ``i`` are the outputs that read it, in
    ascending order, with the weights of the forward table's float64 matrix (the border taps of ``'cubic'`` that meet on one
    sample are merged by one float64 addition; taps of weight exactly 0.0 are left out); ``Kt`` is the longest row rounded up to a multiple of 4 and a shorter row is
    padded with weight 0.0 and its last index.  A source sample no output reads (``'cubic'`` 64 -> 8 and 24 -> 8 have such samples) gives a
    row of weights 0.0 and index 0."""
    M, support = _operator_matrix(_degradation_of("adjoint_table", kind, opts), n_in, n_out)
    return _table_of(M.T, support.T, empty_rows=True)


_OP_NORMS: Dict[tuple, float] = {}


def operator_norm(kind: Union[str, Degradation], n_in: int, n_out: int, **opts) -> float:
    """The spectral norm (largest singular value) of the float64 matrix of ``operator_table(kind, n_in, n_out)``."""
    d = _degradation_of("operator_norm", kind, opts)
    key = (d, int(n_in), int(n_out))
    if key not in _OP_NORMS:
        _OP_NORMS[key] = float(np.linalg.norm(_operator_matrix(d, n_in, n_out)[0], 2))
    return _OP_NORMS[key]


def _device_adjoint_table(d: Degradation, n_in: int, n_out: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``adjoint_table`` on the device; cached per (kind, options, in, out, device)."""
    return _on_device(adjoint_table, device, d, int(n_in), int(n_out))


def resample_adjoint(g: torch.Tensor, size, degradation: Union[str, Degradation] = "cubic") -> torch.Tensor:
    """The adjoint of ``resample``: fp32 CUDA ``(N, C, oh, ow)`` (or ``(C, oh, ow)``) -> a new ``(N, C, H, W)`` tensor with
    ``size = (H, W)``, ``A_y^T . g . A_x`` for the operators ``A`` of ``resample(x, (oh, ow), degradation)`` on an ``H x W``
    image.  It is rdst_resample_sep under the transposed tables (``adjoint_table``): the horizontal sums over the LR columns
    first, then the vertical chains, two launches.  Not differentiable."""
    d = Degradation.of(degradation)      # the table of an axis maps its LR samples to its HR ones: A's sizes, the other way round
    return _resample_sep("resample_adjoint", "g", g, size, lambda n_lr, n_hr, dev: _device_adjoint_table(d, n_hr, n_lr, dev))


class _Degrade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, d):
        ctx.hw, ctx.d = tuple(x.shape[-2:]), d
        return resample(x.detach(), size, d)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        return resample_adjoint(grad.contiguous(), ctx.hw, ctx.d), None, None


def degrade(x: torch.Tensor, size, degradation: Union[str, Degradation] = "cubic") -> torch.Tensor:
    """``resample`` that takes part in autograd: the forward has ``resample``'s bits, the backward is ``resample_adjoint`` of
    the incoming gradient.  It cannot be differentiated twice."""
    d = Degradation.of(degradation)
    if not isinstance(x, torch.Tensor):
        raise TypeError("degrade: x must be a torch tensor")
    _need_gpu("degrade", x)
    return _Degrade.apply(x, _pair(size), d)


# ---- the noise term: LR = A(HR) + n -----------------------------------------------------------------------------------------
NOISE_KINDS = ("gaussian", "poisson-gaussian", "rician")
DEFAULT_NOISE_SIGMA = 0.02      # 2 % of the unit intensity range the slices are normalised to
DEFAULT_NOISE_GAIN = 0.01       # variance 0.01 v on top of the floor: sd 0.1 at full intensity
# kind -> its options with their defaults, and where each goes: (model, option of p0, option of p1); None = the level 0
_NOISE_OPTS = {"gaussian": {"sigma": DEFAULT_NOISE_SIGMA}, "poisson-gaussian": {"gain": DEFAULT_NOISE_GAIN, "sigma": DEFAULT_NOISE_SIGMA},
               "rician": {"sigma": DEFAULT_NOISE_SIGMA}}
_NOISE_SLOTS = {"gaussian": (_lib.NOISE_HETERO, None, "sigma"), "poisson-gaussian": (_lib.NOISE_HETERO, "gain", "sigma"),
                "rician": (_lib.NOISE_RICIAN, "sigma", None)}
_SEED_MASK = (1 << 64) - 1


def _noise_level(name: str, v) -> Union[float, Tuple[float, float]]:
    """A level as the constructor keeps it: a non-negative finite float, or a ``(lo, hi)`` pair of them with ``lo <= hi``."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"Noise: {name}={v!r} must be a number or a (lo, hi) pair")
        lo, hi = (_noise_level(name, t) for t in v)
        if isinstance(lo, tuple) or isinstance(hi, tuple) or lo > hi:
            raise ValueError(f"Noise: {name}={v!r} must be a (lo, hi) pair with lo <= hi")
        return (lo, hi)
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"Noise: {name}={v!r} must be a number or a (lo, hi) pair")
    f = float(v)
    if not math.isfinite(f) or f < 0:
        raise ValueError(f"Noise: {name}={v!r} must be finite and not negative")
    return f


class Noise(_Frozen):
    """The noise term of ``LR = A(HR) + n``: ``Noise(kind, **opts)``, a frozen, hashable value like ``Degradation``; a kind's
    name is accepted wherever a ``Noise`` is and stands for its default levels.  include/rdst_hip_noise.h defines the models.

    ``'gaussian'`` (``sigma``): additive, signal-independent.  ``'poisson-gaussian'`` (``gain``, ``sigma``): signal-dependent,
    variance ``gain * max(v, 0) + sigma^2``, the Gaussian approximation of photon-limited detectors (CT).  ``'rician'``
    (``sigma``): the modulus of the value with complex Gaussian noise, magnitude MRI.  A level is a non-negative finite float, or a
    ``(lo, hi)`` pair with ``lo <= hi`` from which every patch (or image) draws its own level uniformly.  The defaults are
    ``sigma = 0.02`` and ``gain = 0.01``, for intensities in [0, 1].  ``clip=None`` or ``(lo, hi)``: the noisy value is clamped
    to that range (``(0, 1)`` keeps the inputs in the range of the clean ones)."""
    __slots__ = ("kind", "opts", "clip")

    def __init__(self, kind: str = "gaussian", clip=None, **opts):
        if kind not in NOISE_KINDS:
            raise ValueError(f"Noise: kind={kind!r} is not one of {NOISE_KINDS}")
        known = _NOISE_OPTS[kind]
        for k in opts:
            if k not in known:
                raise ValueError(f"Noise: {kind!r} takes no option {k!r} (it takes {tuple(known)} and clip)")
        full = {k: _noise_level(k, v) for k, v in {**known, **opts}.items()}
        if clip is not None:
            if not isinstance(clip, (tuple, list)) or len(clip) != 2:
                raise ValueError(f"Noise: clip={clip!r} must be None or a (lo, hi) pair")
            clip = (float(clip[0]), float(clip[1]))
            if math.isnan(clip[0]) or math.isnan(clip[1]) or clip[0] > clip[1]:
                raise ValueError(f"Noise: clip={clip!r} must be a (lo, hi) pair with lo <= hi")
        self._freeze(kind, tuple(sorted(full.items())), clip)

    @classmethod
    def from_paras(cls, paras) -> Optional["Noise"]:
        """``paras.noise_method`` (``None`` / ``''``: no noise, returned as ``None``; otherwise a kind's name) with the optional
        ``paras.noise_sigma``, ``paras.noise_gain`` and ``paras.noise_clip``.  The reference's configuration has none of them."""
        nm = getattr(paras, "noise_method", None)
        if nm in (None, ""):
            return None
        if nm not in NOISE_KINDS:
            raise ValueError(f"Noise.from_paras: noise_method={nm!r} is not None, '' or one of {NOISE_KINDS}")
        opts = {k: getattr(paras, "noise_" + k) for k in _NOISE_OPTS[nm] if getattr(paras, "noise_" + k, None) is not None}
        return cls(nm, clip=getattr(paras, "noise_clip", None), **opts)

    @property
    def model(self) -> int:
        """RDST_NOISE_HETERO or RDST_NOISE_RICIAN."""
        return _NOISE_SLOTS[self.kind][0]

    @property
    def ranges(self) -> Tuple[Tuple[float, float], Tuple[float, float]]:
        """``((lo, hi) of p0, (lo, hi) of p1)``: the two levels the kernels take, a fixed level as ``(v, v)``."""
        o = dict(self.opts)
        out = []
        for name in _NOISE_SLOTS[self.kind][1:]:
            v = 0.0 if name is None else o[name]
            out.append(v if isinstance(v, tuple) else (v, v))
        return tuple(out)

    @property
    def clip_range(self) -> Tuple[float, float]:
        return (-math.inf, math.inf) if self.clip is None else self.clip

    def levels_from(self, u: torch.Tensor) -> torch.Tensor:
        """Uniforms ``(n, 2)`` in [0, 1) -> the levels ``(n, 2)``: ``lo + (hi - lo) * u`` in float64, rounded once to fp32."""
        t = _LEVEL_TERMS.get(self)
        if t is None:       # (draw() is host time in front of every batch: the two constants are made once per value)
            (l0, h0), (l1, h1) = self.ranges
            t = _LEVEL_TERMS[self] = (torch.tensor([l0, l1], dtype=torch.float64), torch.tensor([h0 - l0, h1 - l1], dtype=torch.float64))
        return (t[0] + t[1] * u.to(torch.float64)).to(torch.float32)

    def draw(self, n: int, generator: Optional[torch.Generator] = None) -> Tuple[int, torch.Tensor]:
        """One 64-bit seed, then ``torch.rand(n, 2)``: ``(seed, levels)``, the levels fp32 ``(n, 2)`` on the host."""
        return _draw_seed(generator), self.levels_from(torch.rand(n, 2, generator=generator))


_LEVEL_TERMS: Dict["Noise", Tuple[torch.Tensor, torch.Tensor]] = {}      # Noise -> (lo, hi - lo) of its two levels, float64


def _draw_seed(generator: Optional[torch.Generator]) -> int:
    return int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64, generator=generator)) & _SEED_MASK


def _signed64(seed: int) -> int:
    seed = int(seed) & _SEED_MASK
    return seed - (1 << 64) if seed >> 63 else seed


def _host_levels(levels, n: int, what: str) -> torch.Tensor:
    if not isinstance(levels, torch.Tensor) or levels.is_cuda or tuple(levels.shape) != (n, 2) or not levels.is_floating_point():
        raise ValueError(f"{what}: levels must be a host tensor of shape ({n}, 2)")
    return levels.to(torch.float32)


def noise_words(planes: int, H: int, W: int, seed: int, device="cuda") -> torch.Tensor:
    """The four Philox4x32-10 words of every pixel under ``seed`` (rdst_noise_words): int32 ``(planes, H, W, 4)`` bit patterns
    on the device, key = the seed's halves, counter = ``(x, y, plane, 0)``.  What the noise of ``add_noise`` and of the sampler
    is made from, words 0 and 1 of each pixel."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rdst_amd.data.noise_words: the HIP path needs a GPU; there is no CPU fallback")
    planes, H, W = int(planes), int(H), int(W)
    if min(planes, H, W) <= 0:
        raise ValueError(f"noise_words: sizes must be positive, got {(planes, H, W)}")
    lib = _lib.load()
    with torch.cuda.device(device):
        sd = torch.tensor([_signed64(seed)], dtype=torch.int64).to(device)
        out = torch.empty(planes, H, W, 4, dtype=torch.int32, device=device)
        _lib.check(lib.rdst_noise_words(out.data_ptr(), planes, H, W, sd.data_ptr(), _stream()), "rdst_noise_words")
    return out


def add_noise(x: torch.Tensor, noise: Union[str, Noise], levels: Optional[torch.Tensor] = None, seed: Optional[int] = None,
              generator: Optional[torch.Generator] = None, out: Optional[torch.Tensor] = None, return_draw: bool = False):
    """The noise term on whole images (rdst_add_noise, one launch): fp32 CUDA ``(N, C, H, W)`` (or ``(C, H, W)``) -> a new tensor
    of that shape, or ``out`` (``out=x`` works in place).  Pixel ``(n, c, y, x)`` gets the normals of ``(seed, n * C + c, y, x)``
    under the levels of image ``n``.  ``levels``: an ``(N, 2)`` tensor of ``(p0, p1)`` per image (``Noise.ranges`` says which
    option is which), on the host or on ``x``'s device; ``None`` draws them from ``noise``.  ``seed``: an int (its low 64 bits),
    or ``None`` to draw one.  What is drawn comes from ``generator`` (a CPU generator; torch's default one if ``None``), the seed
    first.  Seed and host levels go to the device in one non-blocking copy from pinned memory: the call neither waits for the
    device nor reads from it.  ``return_draw=True`` returns ``(y, seed, levels)``, the levels as a host tensor (or the device
    tensor that was passed).  Not differentiable."""
    nz = Noise.of(noise)
    with _whole_images("add_noise", "x", x) as (x4, squeeze, _):
        N, C, H, W = x4.shape
        if out is not None and (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != torch.float32
                                or out.device != x.device or not out.is_contiguous()):
            raise ValueError(f"add_noise: out must be a contiguous float32 {tuple(x.shape)} tensor on {x.device}")
        if out is not None and out.data_ptr() == x.data_ptr() and not x.is_contiguous():
            raise ValueError("add_noise: in place needs a contiguous x")
        if seed is None:
            seed = _draw_seed(generator)
        seed = int(seed) & _SEED_MASK
        dev_levels = isinstance(levels, torch.Tensor) and levels.is_cuda
        if levels is None:
            levels = nz.levels_from(torch.rand(N, 2, generator=generator))
        elif dev_levels:
            if tuple(levels.shape) != (N, 2) or levels.dtype != torch.float32 or levels.device != x.device:
                raise ValueError(f"add_noise: device levels must be a float32 ({N}, 2) tensor on {x.device}")
            levels = levels.contiguous()
        else:
            levels = _host_levels(levels, N, "add_noise")
        # the seed on its 8-byte boundary, then the host levels: one pinned buffer, one copy
        buf = torch.empty(2 + (0 if dev_levels else 2 * N), dtype=torch.int32, pin_memory=True)
        buf[:2].view(torch.int64)[0] = _signed64(seed)
        if not dev_levels:
            buf[2:].view(torch.float32).view(N, 2).copy_(levels)
        dbuf = buf.to(x.device, non_blocking=True)
        lv = levels.data_ptr() if dev_levels else dbuf.data_ptr() + 8
        y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
        lo, hi = nz.clip_range
        _lib.check(_lib.load().rdst_add_noise(x4.data_ptr(), y.data_ptr(), N, C, H, W, nz.model, lv, dbuf.data_ptr(), lo, hi,
                                              _stream()), "rdst_add_noise")
    return (y, seed, levels) if return_draw else y


def make_test_pair(hr: torch.Tensor, s: float, degradation: Union[None, str, Degradation] = None,
                   noise: Union[None, str, Noise] = None, generator: Optional[torch.Generator] = None,
                   seed: Optional[int] = None):
    """``get_test_pair`` (datasets/basic_dataset.py:258-301) for one scale, on the device: ``hr`` fp32 CUDA ``(N, C, H, W)``
    -> ``(lr, gt, real_sr_scale)`` with ``lr = resize(hr, (H // s, W // s))``, ``gt = hr`` itself if ``(int(lr_h * s),
    int(lr_w * s)) == (H, W)`` else ``resize(hr, that size)`` (:276), and the real scale of :286.  ``degradation``: ``None``
    the plain cubic resize above; otherwise ``lr = resample(hr, (H // s, W // s), degradation)``, while ``gt``, where it needs
    a resize, stays the plain cubic one (the reference blurs the LR image only, :276 against :112-116).  ``noise``: ``None``,
    or a ``Noise`` (or its name) for ``lr = add_noise(lr, noise, seed=seed, generator=generator)``: one level pair per image,
    drawn from ``generator`` (after the seed, when ``seed`` is ``None``); ``gt`` never gets any."""
    if hr.dim() != 4:
        raise ValueError("make_test_pair: hr must be (N, C, H, W)")
    H, W = hr.shape[-2:]
    lr_h, lr_w = int(H // s), int(W // s)
    if lr_h <= 0 or lr_w <= 0:
        raise ValueError(f"make_test_pair: a {H} x {W} slice is too small for scale {s}")
    lr = bicubic_resize(hr, (lr_h, lr_w)) if degradation is None else resample(hr, (lr_h, lr_w), degradation)
    if noise is not None:
        lr = add_noise(lr, noise, seed=seed, generator=generator, out=lr)
    gh, gw = int(lr_h * s), int(lr_w * s)
    gt = hr if (gh, gw) == (H, W) else bicubic_resize(hr, (gh, gw))
    return lr, gt, (gh / lr_h, gw / lr_w)


def edge_pad(x: torch.Tensor, size) -> torch.Tensor:
    """``ImagePadding(x.shape[-2:], size).pad`` (datasets/basic_dataset.py:585-600) on the last two dimensions: an axis shorter
    than ``size`` grows to it by repeating its edge, ceil((size - n) / 2) before and floor after; a longer one is kept."""
    th, tw = _pair(size)
    for dim, target in ((-2, th), (-1, tw)):
        n = x.shape[dim]
        if target > n:
            before = math.ceil((target - n) / 2)
            src = torch.arange(-before, target - before, device=x.device).clamp_(0, n - 1)
            x = x.index_select(dim, src)
    return x


def _as_stack(images, what: str, channels: bool) -> torch.Tensor:
    """A tensor ((S, C, H, W) / (S, H, W)) or a list of (H, W, C) / (H, W) arrays of one shape -> one host tensor."""
    if isinstance(images, torch.Tensor):
        t = images.detach().cpu()
    else:
        arrs = [np.asarray(a) for a in images]
        if not arrs:
            raise ValueError(f"DevicePatchSampler: {what} is empty")
        if any(a.shape != arrs[0].shape for a in arrs):
            raise ValueError(f"DevicePatchSampler: the slices of {what} must all have one shape")
        t = torch.from_numpy(np.stack(arrs))
        if channels:
            if t.dim() == 3:
                t = t.unsqueeze(-1)
            if t.dim() == 4:
                t = t.permute(0, 3, 1, 2)       # (S, H, W, C), the layout of the reference's hr_images
    if t.dim() != (4 if channels else 3):
        raise ValueError(f"DevicePatchSampler: {what} must be {'(S, C, H, W)' if channels else '(S, H, W)'}, got {tuple(t.shape)}")
    return t


class Draw(NamedTuple):
    """The random part of one batch: the scale, its HR patch size, the host copy of the index table and, when the batch is
    augmented, of the variant table; when it is noisy, the seed of the noise field and the levels of every patch."""
    sr_factor: float
    hr_patch_size: int
    indices: torch.Tensor                       # (B, 3) int32 on the host: slice, top, left
    variants: Optional[torch.Tensor] = None     # (B,) int32 on the host: the ``tiling.dihedral`` transform of every patch
    noise_seed: Optional[int] = None            # the 64-bit seed of the batch's noise field, in [0, 2^64)
    noise_levels: Optional[torch.Tensor] = None     # (B, 2) fp32 on the host: (p0, p1) of every patch


_AUGMENT = {False: 0, None: 0, True: 8, "d8": 8, "flip": 4}      # augment= -> how many of the eight transforms are drawn


class DevicePatchSampler:
    """``BasicMultiSRTrain`` / ``OASISMultiSRTrain`` with the slices resident on the GPU.

    ``hr_images``: a ``(S, C, H, W)`` tensor or a list of ``(H, W, C)`` arrays of one shape; edge-padded once to at least the
    largest HR patch (``edge_pad``) and moved to ``device`` once.  ``labels`` (``(S, H, W)`` or a list of ``(H, W)``, values
    0..255) are padded the same way.  ``mean`` / ``std`` are those of datasets/OASIS_dataset.py:154-160 (over the padded slices,
    per channel), for ``make_RDSTSR(paras, mean, std)``.

    ``sample()`` -> ``{'in', 'out', 'sr_factor', 'real_sr_scale', 'indices'}`` (+ ``'label'``, int64 ``(B, 1, hp, hp)``):
    ``batch_size`` DISTINCT slices (:192), one scale per batch (:193), ``hp = int(lp * s)`` (:222-223), origins uniform on
    ``[0, H - hp] x [0, W - hp]`` inclusive (:492-497).  Everything random comes from ``generator`` (a CPU torch.Generator), the
    3 B integers go to the device with a non-blocking copy from pinned memory, and one HIP launch writes the batch: the call
    neither waits for the device nor reads from it.  ``sample(out=(inputs, targets))`` writes into the caller's tensors.

    ``augment``: ``False`` / ``None`` the sampler above; ``True`` / ``'d8'`` one of the eight transforms of ``tiling.dihedral``
    per patch, uniformly (``k`` in 0..7: flip the columns if ``k & 1``, the rows if ``k & 2``, then transpose if ``k & 4``);
    ``'flip'`` one of the four without the transpose.  Crop, then transform, then degrade: ``out[b] = dihedral(crop_b, k_b)``, the
    label likewise, and ``in[b]`` is the resize of the TRANSFORMED patch, so ``in == bicubic_resize(out, lp)`` holds bit for bit
    as it does without (resizing first and flipping afterwards would not give the same bits).  The ``B`` variants are drawn
    after the integers above (without ``augment`` the generator is consumed exactly as before), travel with the origins in the
    same pinned copy and are returned as ``batch['variants']`` (int32 ``(B,)`` on the host; the key exists only in an augmented
    batch).  A ``draw=`` decides: ``Draw(..., variants=t)`` forces the transforms as it forces the origins, whatever
    ``augment`` is, and a draw without variants gives a plain batch.

    ``degradation``: ``None`` / ``'cubic'`` the sampler above, bit for bit; any other ``Degradation`` (or its name) makes
    ``in[b]`` that degradation of the cut and turned patch, still in one launch (rdst_sample_patches_op), with or without
    ``augment`` and ``labels`` and for every scale (one table per ``(hp, lp)``): ``in == resample(out, lp, degradation)`` bit
    for bit, ``out`` / ``label`` and the generator's use are unchanged, and the batch carries ``batch['degradation']``.
    ``blur_method`` stays the reference's argument and is still refused unless ``None`` / ``''``: the Gaussian blur is asked
    for with ``degradation='cubic+gaussian'`` or ``Degradation.from_paras(paras)``.

    ``noise``: ``None`` the sampler above, bit for bit, the generator consumed exactly as before; a ``Noise`` (or its name) adds
    the noise term to ``in[b]`` in the same one launch (rdst_sample_patches_noise; ``'cubic'`` goes through it under its K = 4
    table): ``in == add_noise(resample(out, lp, degradation), noise, levels=batch['noise_levels'], seed=batch['noise_seed'])``
    bit for bit, while ``out`` and ``label`` are those of the clean sampler.  ``draw()`` then draws, after the variants, one 64-bit
    seed and ``torch.rand(B, 2)``, from which every patch gets its own levels (``Noise.levels_from``); nothing else is drawn.
    Seed and levels travel with the index table and the variants in the same pinned buffer and the same single copy (the seed
    on an 8-byte boundary) and are returned as ``batch['noise_seed']`` / ``batch['noise_levels']`` beside ``batch['noise']``.
    A ``draw=`` decides here too: a draw with ``noise_seed`` and ``noise_levels`` gives a noisy batch, one without a clean one.

    ``device='cpu'`` keeps the slices on the host: ``draw()`` works, ``sample()`` raises (there is no CPU path)."""

    def __init__(self, hr_images, batch_size: int, lr_patch_size: int, sr_scales: Sequence[float] = (4.0,), labels=None,
                 blur_method: Optional[str] = None, device="cuda", generator: Optional[torch.Generator] = None,
                 augment=False, degradation: Union[None, str, Degradation] = None, noise: Union[None, str, Noise] = None):
        if blur_method not in (None, ""):
            raise ValueError(f"DevicePatchSampler: blur_method={blur_method!r} is not taken here: pass "
                             "degradation='cubic+gaussian' (cv2.GaussianBlur of the resized patch) or "
                             "degradation=Degradation.from_paras(paras); the shipped configuration has blur_method = ''")
        d = None if degradation is None else Degradation.of(degradation)
        self.degradation = None if d is None or d.kind == "cubic" else d     # None: the two 4-tap entry points, as before
        self.noise = None if noise is None else Noise.of(noise)
        if not isinstance(augment, (bool, str, type(None))) or augment not in _AUGMENT:
            raise ValueError(f"DevicePatchSampler: augment={augment!r} is not one of False, True, 'd8', 'flip'")
        self.n_variants = _AUGMENT[augment]
        self.batch_size, self.lr_patch_size = int(batch_size), int(lr_patch_size)
        self.sr_scales = [float(s) for s in sr_scales]
        if self.batch_size <= 0 or self.lr_patch_size <= 0 or not self.sr_scales:
            raise ValueError("DevicePatchSampler: batch_size, lr_patch_size and the number of scales must be positive")
        self.hr_patch_sizes = [int(self.lr_patch_size * s) for s in self.sr_scales]     # get_hr_patch_size
        if min(self.hr_patch_sizes) <= 0:
            raise ValueError(f"DevicePatchSampler: scales {self.sr_scales} give an empty HR patch")
        if self.degradation is not None:
            for hp in self.hr_patch_sizes:       # refuse what the operator refuses here, not at the first batch
                operator_table(self.degradation, hp, self.lr_patch_size)
        hr = _as_stack(hr_images, "hr_images", True).to(torch.float32)
        if hr.shape[0] < self.batch_size:
            raise ValueError(f"DevicePatchSampler: {hr.shape[0]} slices cannot give {self.batch_size} distinct ones per batch")
        self.input_shape = tuple(hr.shape[-2:])
        hr = edge_pad(hr, max(self.hr_patch_sizes)).contiguous()          # OASIS_dataset.py:142-144
        self.S, self.C, self.H, self.W = hr.shape
        if max(self.hr_patch_sizes) > min(self.H, self.W):
            raise ValueError(f"DevicePatchSampler: a {max(self.hr_patch_sizes)}-pixel patch does not fit the padded slices "
                             f"({self.H} x {self.W})")
        hwc = np.ascontiguousarray(hr.permute(0, 2, 3, 1).numpy())       # the reference's layout: numpy sums in its order
        self.mean = np.mean(hwc, axis=(0, 1, 2))                          # OASIS_dataset.py:158
        self.std = np.std(hwc, axis=(0, 1, 2))                            # :160
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.hr_images = hr.to(self.device)
        self.labels = None
        if labels is not None:
            lab = _as_stack(labels, "labels", False)
            if tuple(lab.shape) != (self.S,) + self.input_shape:
                raise ValueError(f"DevicePatchSampler: labels {tuple(lab.shape)} do not match the slices "
                                 f"{(self.S,) + self.input_shape}")
            if lab.numel() and (lab.min() < 0 or lab.max() > 255):
                raise ValueError("DevicePatchSampler: labels must lie in 0..255")
            self.labels = edge_pad(lab.to(torch.uint8), max(self.hr_patch_sizes)).contiguous().to(self.device)
        self.generator = generator if generator is not None else torch.Generator()
        self._pin = self.device.type == "cuda"

    def __len__(self) -> int:
        return self.S

    def draw(self) -> Draw:
        """The random integers of the next batch, on the host (no device involved)."""
        g, B = self.generator, self.batch_size
        k = int(torch.randint(len(self.sr_scales), (1,), generator=g)) if len(self.sr_scales) > 1 else 0
        hp = self.hr_patch_sizes[k]
        noisy = self.noise is not None
        # one buffer: the index table and what else the kernel reads behind it; sample() copies it to the device as it is
        vo, so, lo, total = self._layout(B, bool(self.n_variants), noisy)
        both = torch.empty(total, dtype=torch.int32, pin_memory=self._pin)
        tab, var = both[:3 * B].view(B, 3), both[vo:vo + B] if vo is not None else None
        tab[:, 0] = torch.randperm(self.S, generator=g)[:B]
        tab[:, 1] = torch.randint(0, self.H - hp + 1, (B,), generator=g)
        tab[:, 2] = torch.randint(0, self.W - hp + 1, (B,), generator=g)
        if var is not None:
            var[:] = torch.randint(0, self.n_variants, (B,), generator=g)
        if not noisy:
            return Draw(self.sr_scales[k], hp, tab, var)
        seed = _draw_seed(g)
        if so != self._layout(B, var is not None, False)[3]:
            both[so - 1] = 0        # the pad word in front of the seed
        both[so:so + 2].view(torch.int64)[0] = _signed64(seed)
        lev = both[lo:].view(torch.float32).view(B, 2)
        lev.copy_(self.noise.levels_from(torch.rand(B, 2, generator=g)))
        return Draw(self.sr_scales[k], hp, tab, var, seed, lev)

    @staticmethod
    def _layout(B: int, variants: bool, noisy: bool):
        """The host buffer of one draw in int32 units: ``(variants, seed, levels, total)``, ``None`` for a part it does not
        have.  The index table (3 B), the variants (B), a pad word where the seed would not stand on an 8-byte boundary, the
        seed (2), the levels (2 B fp32)."""
        n = 3 * B
        vo = n if variants else None
        n += B if variants else 0
        if not noisy:
            return vo, None, None, n
        so = n + (n & 1)
        return vo, so, so + 2, so + 2 + 2 * B

    def _packed(self, d: Draw):
        """The host buffer of a draw and its ``_layout``.  A draw of ``draw()`` is one already; forced tables are packed into a
        new one."""
        B, idx, var, lev = self.batch_size, d.indices, d.variants, d.noise_levels
        noisy = d.noise_seed is not None
        vo, so, lo, total = lay = self._layout(B, var is not None, noisy)
        both = getattr(idx, "_base", None)      # draw()'s views have the whole buffer as their base
        if (both is not None and both.dtype == torch.int32 and tuple(both.shape) == (total,)
                and tuple(idx.shape) == (B, 3) and idx.is_contiguous() and idx.data_ptr() == both.data_ptr()
                and (var is None or (getattr(var, "_base", None) is both and tuple(var.shape) == (B,)
                                     and var.data_ptr() == both.data_ptr() + 4 * vo))
                # (a view under another dtype has a base of its own: the levels are known by the storage they share)
                and (not noisy or (isinstance(lev, torch.Tensor) and tuple(lev.shape) == (B, 2) and lev.is_contiguous()
                                   and lev.untyped_storage().data_ptr() == both.untyped_storage().data_ptr()
                                   and lev.dtype == torch.float32 and lev.data_ptr() == both.data_ptr() + 4 * lo
                                   and int(both[so:so + 2].view(torch.int64)[0]) == _signed64(d.noise_seed)))):
            return both, lay
        if var is not None and (not isinstance(var, torch.Tensor) or var.is_cuda or var.is_floating_point()
                                or tuple(var.shape) != (B,)):
            raise ValueError(f"DevicePatchSampler.sample: draw.variants must be a host tensor of {B} integers")
        both = torch.zeros(total, dtype=torch.int32, pin_memory=self._pin)
        both[:3 * B].view(B, 3).copy_(idx)
        if var is not None:
            both[vo:vo + B].copy_(var)
        if noisy:
            both[so:so + 2].view(torch.int64)[0] = _signed64(d.noise_seed)
            both[lo:].view(torch.float32).view(B, 2).copy_(_host_levels(lev, B, "DevicePatchSampler.sample: draw.noise_levels"))
        return both, lay

    def batch_shapes(self, draw: Draw):
        """(shape of 'in', shape of 'out') of the batch ``draw`` leads to."""
        B, C, lp, hp = self.batch_size, self.C, self.lr_patch_size, draw.hr_patch_size
        return (B, C, lp, lp), (B, C, hp, hp)

    def sample(self, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, draw: Optional[Draw] = None) -> dict:
        if self.device.type != "cuda":
            raise RuntimeError("rdst_amd.data.DevicePatchSampler.sample: the HIP path needs a GPU; there is no CPU fallback")
        d = draw if draw is not None else self.draw()
        noisy = d.noise_seed is not None
        if noisy != (d.noise_levels is not None):
            raise ValueError("DevicePatchSampler.sample: draw.noise_seed and draw.noise_levels go together")
        if noisy and self.noise is None:
            raise ValueError("DevicePatchSampler.sample: a draw with noise needs a sampler built with noise= (it names the model)")
        lr_shape, hr_shape = self.batch_shapes(d)
        lp, hp = self.lr_patch_size, d.hr_patch_size
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if out is None:
                lr = torch.empty(lr_shape, dtype=torch.float32, device=self.device)
                hr = torch.empty(hr_shape, dtype=torch.float32, device=self.device)
            else:
                lr, hr = out
                for t, shape, name in ((lr, lr_shape, "inputs"), (hr, hr_shape, "targets")):
                    if (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device
                            or not t.is_contiguous()):
                        raise ValueError(f"DevicePatchSampler.sample: out {name} must be a contiguous float32 {shape} tensor "
                                         f"on {self.device}")
            # the variants, the seed and the levels sit behind the 3 B int32 of the table, at _layout's offsets
            both, (vo, so, lo, _) = self._packed(d)
            index = both.to(self.device, non_blocking=True)
            variant = index.data_ptr() + 4 * vo if vo is not None else None
            lab = None
            if self.labels is not None:
                lab = torch.empty(hr_shape[0], 1, hp, hp, dtype=torch.uint8, device=self.device)
            stack, labels = self.hr_images.data_ptr(), self.labels.data_ptr() if lab is not None else None
            sizes = (hr.data_ptr(), lr.data_ptr(), lab.data_ptr() if lab is not None else None, self.S, self.C, self.H, self.W,
                     self.batch_size, hp, lp)
            if noisy:       # 'cubic' under its K = 4 table: the 4-tap kernels' bits, then the noise
                ti, tw = _device_op_table(self.degradation or Degradation("cubic"), hp, lp, self.device)
                clip_lo, clip_hi = self.noise.clip_range
                _lib.check(lib.rdst_sample_patches_noise(stack, labels, index.data_ptr(), variant, *sizes, ti.shape[1],
                                                         ti.data_ptr(), tw.data_ptr(), self.noise.model, index.data_ptr() + 4 * lo,
                                                         index.data_ptr() + 4 * so, clip_lo, clip_hi, _stream()),
                           "rdst_sample_patches_noise")
            elif self.degradation is not None:
                ti, tw = _device_op_table(self.degradation, hp, lp, self.device)
                _lib.check(lib.rdst_sample_patches_op(stack, labels, index.data_ptr(), variant, *sizes, ti.shape[1],
                                                      ti.data_ptr(), tw.data_ptr(), _stream()), "rdst_sample_patches_op")
            else:
                ti, tw = _device_table(hp, lp, self.device)
                tail = (*sizes, ti.data_ptr(), tw.data_ptr(), _stream())
                if variant is None:
                    _lib.check(lib.rdst_sample_patches(stack, labels, index.data_ptr(), *tail), "rdst_sample_patches")
                else:
                    _lib.check(lib.rdst_sample_patches_d8(stack, labels, index.data_ptr(), variant, *tail),
                               "rdst_sample_patches_d8")
        batch = {"in": lr, "out": hr, "sr_factor": d.sr_factor, "real_sr_scale": hp / lp, "indices": d.indices}
        if d.variants is not None:
            batch["variants"] = d.variants
        if self.degradation is not None:
            batch["degradation"] = self.degradation
        if noisy:
            batch["noise"], batch["noise_seed"], batch["noise_levels"] = self.noise, int(d.noise_seed) & _SEED_MASK, d.noise_levels
        if lab is not None:
            batch["label"] = lab.to(torch.int64)          # the dtype SegUNet_F('label-gt') takes
        return batch
