"""CPU: argument checks of the PSNR / SSIM scoring entry points (rdst_sr_scores*, include/rdst_hip.h) and of the Python
layer above them (rdst_amd.metrics.device_scores, SRMetrics(device=...)).  Every call here is refused before any launch,
so no GPU is needed; the pointers passed are never dereferenced."""
import ctypes

import numpy as np
import pytest
import torch

from rdst_amd import _lib
from rdst_amd import metrics as M

FAKE = 256          # a non-null "device pointer" for calls that must be refused before any launch
SHAPE = dict(N=2, C=3, H=40, W=36, margin=2, win=7)


def _ws(N, C, H, W, margin, win):
    return _lib.load().rdst_sr_scores_workspace(N, C, H, W, margin, win)


def _call(N=2, C=3, H=40, W=36, margin=2, win=7, data_range=1.0, gt=FAKE, pred=FAKE, mse=FAKE, ssim=FAKE, ws=FAKE,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 20
    lib = _lib.load()
    rc = lib.rdst_sr_scores(gt, pred, N, C, H, W, margin, win, data_range, mse, ssim, ws, ws_bytes, None)
    return rc, lib.rdst_last_error().decode()


def test_workspace_size():
    # 40 x 36 cropped by 2 -> 36 x 32, SSIM interior (win 7) 30 x 26: 2 row tiles x 1 column tile, 3 channels, 2 images
    assert _ws(**SHAPE) == 2 * 3 * 2 * 1 * 2 * 8
    assert _ws(64, 1, 176, 208, 4, 7) == 64 * 11 * 4 * 2 * 8
    assert _ws(1, 1, 7, 7, 0, 7) == 16          # the minimal image: a one-pixel interior
    assert _ws(1, 1, 7, 7, 0, 9) == 0           # refused shapes report 0 bytes
    assert _ws(0, 1, 7, 7, 0, 7) == 0


@pytest.mark.parametrize("kw", [dict(N=0), dict(C=0), dict(H=0), dict(W=-1), dict(N=-3), dict(margin=-1)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_bad_sizes(kw):
    rc, msg = _call(**kw)
    assert rc == _lib.EINVAL and "rdst_sr_scores" in msg and "bad shape" in msg


@pytest.mark.parametrize("win", [2, 6, 1, 17, 0, -7])
def test_bad_window(win):
    rc, msg = _call(win=win)
    assert rc == _lib.EINVAL and "win" in msg


@pytest.mark.parametrize("kw", [dict(H=10, margin=2), dict(W=12, margin=3), dict(H=6, W=6, margin=0),
                                dict(H=40, W=40, margin=20, win=3)], ids=str)
def test_cropped_side_smaller_than_window(kw):
    rc, msg = _call(**kw)
    assert rc == _lib.EINVAL and "smaller than win" in msg


@pytest.mark.parametrize("dr", [0.0, -1.0, float("nan")])
def test_bad_data_range(dr):
    rc, msg = _call(data_range=dr)
    assert rc == _lib.EINVAL and "data_range" in msg


@pytest.mark.parametrize("which", ["gt", "pred", "mse", "ssim", "ws"])
def test_null_pointers(which):
    rc, msg = _call(**{which: None})
    assert rc == _lib.EINVAL and "null pointer" in msg


def test_short_workspace():
    need = _ws(**SHAPE)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == _lib.EINVAL and "workspace" in msg and str(need) in msg
    rc, msg = _call(ws_bytes=0)
    assert rc == _lib.EINVAL and "workspace" in msg


def test_too_many_pixels():
    rc, msg = _call(N=1 << 16, C=1, H=256, W=257, margin=0)     # 2^32 + 2^24 pixels
    assert rc == _lib.EINVAL and "2^31" in msg
    assert _ws(1 << 16, 1, 256, 257, 0, 7) == 0


def test_device_scores_rejects_before_the_device():
    f32 = torch.zeros(1, 1, 16, 16)
    with pytest.raises(TypeError):
        M.device_scores(f32.double(), f32.double())
    with pytest.raises(TypeError):
        M.device_scores(f32, f32.bfloat16())
    with pytest.raises(TypeError):
        M.device_scores(f32.numpy(), f32.numpy())
    # the cases numpy's ssim() refuses, with its message
    with pytest.raises(ValueError, match="same shape and be at least win_size"):
        M.device_scores(f32, torch.zeros(1, 1, 16, 15))
    with pytest.raises(ValueError, match="same shape and be at least win_size"):
        M.device_scores(f32, f32, margin=5)
    with pytest.raises(ValueError, match="same shape and be at least win_size"):
        M.device_scores(torch.zeros(1, 1, 6, 40), torch.zeros(1, 1, 6, 40))
    with pytest.raises(ValueError, match="at least win_size"):
        M.ssim(np.zeros((6, 40)), np.zeros((6, 40)))
    # what the kernel cannot do
    for kw in (dict(win_size=6), dict(win_size=17), dict(win_size=1), dict(data_range=0.0), dict(margin=-1)):
        with pytest.raises(ValueError):
            M.device_scores(f32, f32, **kw)
    with pytest.raises(ValueError, match="CUDA"):
        M.device_scores(f32, f32)            # host tensors


def test_srmetrics_device_argument():
    with pytest.raises(ValueError):
        M.SRMetrics("psnr ssim", device="cpu")
    with pytest.raises(ValueError, match="Do not support"):
        M.SRMetrics("psnr fid", device="cuda")
    with pytest.raises(ValueError):
        M.SRMetrics("psnr", "median", device="cuda")
    m = M.SRMetrics("psnr ssim", "mean", device="cuda")
    with pytest.raises(TypeError):
        m(np.zeros((1, 16, 16, 1), np.float32), np.zeros((1, 16, 16, 1), np.float32))
    # the default stays the host path
    a = np.random.default_rng(0).random((2, 16, 16, 1)).astype(np.float32)
    host = M.SRMetrics("psnr ssim")(a, a * 0.5, 2)
    assert M.SRMetrics("psnr ssim").device is None and set(host) == {"psnr", "ssim"} and len(host["psnr"]) == 2
