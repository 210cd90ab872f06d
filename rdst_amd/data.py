"""Training batches and test pairs made on the device: the data side of the reference's trainer around the HIP hot path.

The reference builds every batch on the CPU (``BasicMultiSRTrain.__getitem__``, datasets/basic_dataset.py:190-217:
``batch_size`` random slices, one random HR crop each, ``cv2.resize(INTER_CUBIC)`` of every crop down to the LR patch, in
DataLoader workers, models/trans_sr_trainer.py:116-121) and copies it to the GPU (:143); the test side does the same to whole
slices (``get_test_pair``, basic_dataset.py:258-301).  The training volumes fit in device memory many times over, so here the
slices are moved to the GPU once and a batch is cut and degraded where it is consumed:

  * ``bicubic_resize(x, size)``      the resize itself (rdst_resize_bicubic, include/rdst_hip.h);
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

Out of scope, and refused where they could be asked for: the Gaussian blur option (``blur_method='gaussian'``,
cv2.GaussianBlur), augmentation other than the eight flips / transposes, ``return_res_image``, reading volumes from disk.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

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


def _device_table(n_in: int, n_out: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tap_table`` on the device, the weights rounded once to fp32; cached per (in, out, device)."""
    key = (int(n_in), int(n_out), device.type, device.index)
    tab = _TABLES.get(key)
    if tab is None:
        index, weight = tap_table(n_in, n_out)
        tab = (torch.from_numpy(index).to(device), torch.from_numpy(weight.astype(np.float32)).to(device))
        _TABLES[key] = tab
    return tab


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


def bicubic_resize(x: torch.Tensor, size) -> torch.Tensor:
    """fp32 CUDA ``(N, C, H, W)`` (or ``(C, H, W)``) -> a new tensor of spatial ``size`` (an int or ``(oh, ow)``), down or up.
    Not differentiable."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("bicubic_resize: x must be a torch tensor")
    _need_gpu("bicubic_resize", x)
    if x.requires_grad:
        raise RuntimeError("bicubic_resize is not differentiable: detach the input")
    if x.dtype != torch.float32:
        raise TypeError(f"bicubic_resize: x must be float32, got {x.dtype}")
    squeeze = x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError("bicubic_resize: x must have 3 or 4 dimensions")
    oh, ow = _pair(size)
    N, C, H, W = x.shape
    if min(N, C, H, W) <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"bicubic_resize: sizes must be positive, got {tuple(x.shape)} -> {(oh, ow)}")
    x = x.contiguous()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        iy, wy = _device_table(H, oh, x.device)
        ix, wx = _device_table(W, ow, x.device)
        y = torch.empty(N, C, oh, ow, dtype=torch.float32, device=x.device)
        _lib.check(lib.rdst_resize_bicubic(x.data_ptr(), y.data_ptr(), N, C, H, W, oh, ow, iy.data_ptr(), wy.data_ptr(),
                                           ix.data_ptr(), wx.data_ptr(), _stream()), "rdst_resize_bicubic")
    return y[0] if squeeze else y


def make_test_pair(hr: torch.Tensor, s: float):
    """``get_test_pair`` (datasets/basic_dataset.py:258-301) for one scale, on the device: ``hr`` fp32 CUDA ``(N, C, H, W)``
    -> ``(lr, gt, real_sr_scale)`` with ``lr = resize(hr, (H // s, W // s))``, ``gt = hr`` itself if ``(int(lr_h * s),
    int(lr_w * s)) == (H, W)`` else ``resize(hr, that size)`` (:276), and the real scale of :286."""
    if hr.dim() != 4:
        raise ValueError("make_test_pair: hr must be (N, C, H, W)")
    H, W = hr.shape[-2:]
    lr_h, lr_w = int(H // s), int(W // s)
    if lr_h <= 0 or lr_w <= 0:
        raise ValueError(f"make_test_pair: a {H} x {W} slice is too small for scale {s}")
    lr = bicubic_resize(hr, (lr_h, lr_w))
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
    augmented, of the variant table."""
    sr_factor: float
    hr_patch_size: int
    indices: torch.Tensor                       # (B, 3) int32 on the host: slice, top, left
    variants: Optional[torch.Tensor] = None     # (B,) int32 on the host: the ``tiling.dihedral`` transform of every patch


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

    ``device='cpu'`` keeps the slices on the host: ``draw()`` works, ``sample()`` raises (there is no CPU path)."""

    def __init__(self, hr_images, batch_size: int, lr_patch_size: int, sr_scales: Sequence[float] = (4.0,), labels=None,
                 blur_method: Optional[str] = None, device="cuda", generator: Optional[torch.Generator] = None,
                 augment=False):
        if blur_method not in (None, ""):
            raise ValueError(f"DevicePatchSampler: blur_method={blur_method!r} is not supported (cv2.GaussianBlur is out of "
                             "scope; the shipped configuration has blur_method = '')")
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
        if not self.n_variants:
            tab = torch.empty(B, 3, dtype=torch.int32, pin_memory=self._pin)
            var = None
        else:       # one buffer, the variants behind the index table: sample() copies it to the device as it is
            both = torch.empty(4 * B, dtype=torch.int32, pin_memory=self._pin)
            tab, var = both[:3 * B].view(B, 3), both[3 * B:]
        tab[:, 0] = torch.randperm(self.S, generator=g)[:B]
        tab[:, 1] = torch.randint(0, self.H - hp + 1, (B,), generator=g)
        tab[:, 2] = torch.randint(0, self.W - hp + 1, (B,), generator=g)
        if var is not None:
            var[:] = torch.randint(0, self.n_variants, (B,), generator=g)
        return Draw(self.sr_scales[k], hp, tab, var)

    def _packed(self, d: Draw) -> torch.Tensor:
        """The host buffer of an augmented draw, 4 B int32: the index table, then the variants.  A draw of ``draw()`` is one
        already; forced tables are packed into a new one."""
        B, idx, var = self.batch_size, d.indices, d.variants
        both = getattr(var, "_base", None)      # draw()'s two views have the whole buffer as their base
        if (both is not None and both is idx._base and both.dtype == torch.int32 and tuple(both.shape) == (4 * B,)
                and tuple(idx.shape) == (B, 3) and idx.is_contiguous() and idx.data_ptr() == both.data_ptr()
                and tuple(var.shape) == (B,) and var.data_ptr() == both.data_ptr() + 12 * B):
            return both
        if not isinstance(var, torch.Tensor) or var.is_cuda or var.is_floating_point() or tuple(var.shape) != (B,):
            raise ValueError(f"DevicePatchSampler.sample: draw.variants must be a host tensor of {B} integers")
        both = torch.empty(4 * B, dtype=torch.int32, pin_memory=self._pin)
        both[:3 * B].view(B, 3).copy_(idx)
        both[3 * B:].copy_(var)
        return both

    def batch_shapes(self, draw: Draw):
        """(shape of 'in', shape of 'out') of the batch ``draw`` leads to."""
        B, C, lp, hp = self.batch_size, self.C, self.lr_patch_size, draw.hr_patch_size
        return (B, C, lp, lp), (B, C, hp, hp)

    def sample(self, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, draw: Optional[Draw] = None) -> dict:
        if self.device.type != "cuda":
            raise RuntimeError("rdst_amd.data.DevicePatchSampler.sample: the HIP path needs a GPU; there is no CPU fallback")
        d = draw if draw is not None else self.draw()
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
            if d.variants is None:
                index, variant = d.indices.to(self.device, non_blocking=True), None
            else:
                index = self._packed(d).to(self.device, non_blocking=True)
                variant = index.data_ptr() + 12 * self.batch_size        # the variants sit behind the 3 B int32 of the table
            lab = None
            if self.labels is not None:
                lab = torch.empty(hr_shape[0], 1, hp, hp, dtype=torch.uint8, device=self.device)
            ti, tw = _device_table(hp, lp, self.device)
            tail = (hr.data_ptr(), lr.data_ptr(), lab.data_ptr() if lab is not None else None, self.S, self.C, self.H, self.W,
                    self.batch_size, hp, lp, ti.data_ptr(), tw.data_ptr(), _stream())
            stack, labels = self.hr_images.data_ptr(), self.labels.data_ptr() if lab is not None else None
            if variant is None:
                _lib.check(lib.rdst_sample_patches(stack, labels, index.data_ptr(), *tail), "rdst_sample_patches")
            else:
                _lib.check(lib.rdst_sample_patches_d8(stack, labels, index.data_ptr(), variant, *tail),
                           "rdst_sample_patches_d8")
        batch = {"in": lr, "out": hr, "sr_factor": d.sr_factor, "real_sr_scale": hp / lp, "indices": d.indices}
        if d.variants is not None:
            batch["variants"] = d.variants
        if lab is not None:
            batch["label"] = lab.to(torch.int64)          # the dtype SegUNet_F('label-gt') takes
        return batch
