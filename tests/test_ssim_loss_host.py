"""CPU: the yardstick of the SSIM training loss (tests/ssim_reference.py) against rdst_amd.metrics.ssim and the written-out
gradient, the window taps, every refusal of the two C entry points (rdst_ssim_loss*, include/rdst_hip.h: refused before any
launch, so the pointers passed are never dereferenced) and the Python layer's own refusals."""
import types

import numpy as np
import pytest
import torch

import ssim_reference as R
from rdst_amd import _lib
from rdst_amd import metrics as M

FAKE = 256          # a non-null "device pointer" for calls that must be refused before any launch


# ---- the yardstick ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,win,dr", [((2, 3, 23, 37), 7, 1.0), ((1, 1, 40, 70), 11, 255.0), ((1, 2, 9, 12), 3, 1.0)], ids=str)
def test_reference_is_metrics_ssim_for_the_uniform_window(shape, win, dr):
    g, p = R.images(shape, 5, dr)
    taps, cn = R.taps_of("u", win)
    ssim, loss, _ = R.reference(g, p, taps, cn, dr)
    for n in range(shape[0]):
        want = M.ssim(g[n].numpy().transpose(1, 2, 0), p[n].numpy().transpose(1, 2, 0), dr, win)
        assert abs(float(ssim[n]) - want) <= 1e-12, (n, float(ssim[n]), want)
    assert abs(float(loss) - (1.0 - float(ssim.mean()))) <= 1e-15


@pytest.mark.parametrize("shape,window,win,dr", [((2, 1, 40, 70), "u", 7, 1.0), ((2, 1, 40, 70), "g", 11, 1.0),
                                                 ((1, 3, 23, 37), "g", 5, 255.0), ((1, 1, 15, 15), "u", 15, 1.0)], ids=str)
def test_autograd_gradient_is_the_closed_form(shape, window, win, dr):
    g, p = R.images(shape, 6, dr)
    taps, cn = R.taps_of(window, win)
    _, _, grad = R.reference(g, p, taps, cn, dr)
    closed = R.closed_form_grad(g, p, taps, cn, dr)
    assert grad.shape == closed.shape == torch.Size(shape)
    assert float((grad - closed).abs().max()) <= 1e-12 * float(grad.abs().max())


# ---- window_taps ------------------------------------------------------------------------------------------------------

def test_window_taps():
    from rdst_amd.loss import window_taps
    t, cn = window_taps("uniform")
    assert t.dtype == np.float64 and t.shape == (7,) and np.all(t == 1.0 / 7) and cn == 49.0 / 48.0
    t, cn = window_taps("uniform", 3)
    assert t.shape == (3,) and cn == 9.0 / 8.0
    t, cn = window_taps("gaussian")
    assert t.dtype == np.float64 and t.shape == (11,) and cn == 1.0
    assert abs(t.sum() - 1.0) <= 1e-15 and np.array_equal(t, t[::-1]) and t.argmax() == 5
    assert abs(t[4] / t[5] - np.exp(-1.0 / 4.5)) <= 1e-15           # sigma 1.5
    ref, _ = R.taps_of("g", 11)
    assert np.abs(t - ref).max() <= 1e-16
    t, _ = window_taps("gaussian", 5, sigma=0.8)
    assert t.shape == (5,) and abs(t.sum() - 1.0) <= 1e-15 and abs(t[1] / t[2] - np.exp(-1.0 / 1.28)) <= 1e-15
    for bad in (dict(window="box"), dict(win_size=6), dict(win_size=17), dict(win_size=1),
                dict(window="gaussian", sigma=0.0)):
        with pytest.raises(ValueError):
            window_taps(**bad)


# ---- the C entry points -----------------------------------------------------------------------------------------------

def _call(N=2, C=3, H=40, W=36, win=7, taps="default", cov_norm=49.0 / 48.0, data_range=1.0, target=FAKE, pred=FAKE, ssim=FAKE,
          loss=FAKE, grad=FAKE, ws=FAKE, ws_bytes=1 << 20):
    lib = _lib.load()
    keep = None if taps is None or isinstance(taps, str) else np.ascontiguousarray(taps, dtype=np.float64)
    rc = lib.rdst_ssim_loss(target, pred, N, C, H, W, win, None if keep is None else keep.ctypes.data, cov_norm, data_range,
                            ssim, loss, grad, ws, ws_bytes, None)
    return rc, lib.rdst_last_error().decode()


def _ws(N, C, H, W, win):
    return _lib.load().rdst_ssim_loss_workspace(N, C, H, W, win)


def test_workspace_query():
    for shape in ((2, 3, 40, 36, 7), (1, 1, 7, 7, 7), (1, 1, 3, 5, 3), (32, 1, 256, 256, 11), (1, 1, 15, 15, 15)):
        n = _ws(*shape)
        assert n > 0 and n % 8 == 0, shape
    assert _ws(4, 1, 64, 64, 7) == 2 * _ws(2, 1, 64, 64, 7)          # one fp64 per workgroup, per image
    for shape in ((0, 1, 7, 7, 7), (1, 0, 7, 7, 7), (1, 1, -7, 7, 7), (1, 1, 7, 7, 9), (1, 1, 16, 16, 6), (1, 1, 16, 16, 17),
                  (1 << 16, 1, 256, 257, 7)):
        assert _ws(*shape) == 0, shape
        assert "rdst_ssim_loss_workspace" in _lib.load().rdst_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(N=0), "bad shape"), (dict(C=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"), (dict(N=-3), "bad shape"),
    (dict(win=2), "win"), (dict(win=6), "win"), (dict(win=1), "win"), (dict(win=17), "win"), (dict(win=-7), "win"),
    (dict(H=6), "smaller than win"), (dict(W=10, win=11), "smaller than win"),
    (dict(N=1 << 16, C=1, H=256, W=257), "2^31"),
    (dict(target=None), "null pointer"), (dict(pred=None), "null pointer"), (dict(ssim=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(ws_bytes=0), "workspace"),
    (dict(taps=[0.2, 0.2, 0.2, 0.2, 0.2, 0.2, float("nan")]), "finite"),
    (dict(taps=[0.2, 0.2, float("inf"), 0.2, 0.2, 0.2, 0.2]), "finite"),
    (dict(taps=[1.0 / 7] * 6 + [1.0 / 7 + 1e-8]), "sum"),
    (dict(taps=[0.0] * 7), "sum"),
    (dict(cov_norm=0.0), "cov_norm"), (dict(cov_norm=-1.0), "cov_norm"), (dict(cov_norm=float("nan")), "cov_norm"),
    (dict(data_range=0.0), "data_range"), (dict(data_range=-1.0), "data_range"), (dict(data_range=float("nan")), "data_range"),
], ids=lambda v: v if isinstance(v, str) else ",".join(f"{a}={b}" for a, b in v.items())[:40])
def test_refusals(kw, word):
    rc, msg = _call(**kw)
    assert rc == _lib.EINVAL and "rdst_ssim_loss" in msg and word in msg, (rc, msg)


def test_short_workspace_names_the_size():
    need = _ws(2, 3, 40, 36, 7)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == _lib.EINVAL and "rdst_ssim_loss" in msg and "workspace" in msg and str(need) in msg


def test_signatures_bound_and_abi_version_unchanged():
    assert "rdst_ssim_loss" in _lib.SIGNATURES and "rdst_ssim_loss_workspace" in _lib.SIGNATURES
    assert _lib.load().rdst_abi_version() == _lib.ABI_VERSION == 11


# ---- the Python layer -------------------------------------------------------------------------------------------------

def _paras(**kw):
    return types.SimpleNamespace(gpu_id=-1, precision=False, training_losses=["L1", "SSIM"],
                                 loss_scalars={"S": {"L1": 0.16, "SSIM": 0.84}}, training_states=["S"], **kw)


def test_srloss_builds_with_ssim():
    from rdst_amd.loss import SRLoss, SSIMLoss
    sl = SRLoss(_paras())
    assert sl.loss_components == ["Rec_L1", "Rec_SSIM"]
    f = sl.loss_functions["SSIM"]
    assert isinstance(f, SSIMLoss) and (f.window, f.win_size, f.sigma, f.data_range) == ("uniform", None, 1.5, 1.0)
    f = SRLoss(_paras(ssim_window="gaussian", ssim_win_size=9, ssim_sigma=2.0, ssim_data_range=255.0)).loss_functions["SSIM"]
    assert (f.window, f.win_size, f.sigma, f.data_range) == ("gaussian", 9, 2.0, 255.0)
    with pytest.raises(ValueError):
        SRLoss(_paras(ssim_win_size=8))
    for other in ("VGG54", "GAN"):
        p = _paras()
        p.training_losses = ["L1", other]
        with pytest.raises(NotImplementedError):
            SRLoss(p)


def test_ssim_loss_refuses_before_the_device():
    from rdst_amd.loss import SRLoss, ssim_loss
    a, b = torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ssim_loss(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SRLoss(_paras())(a, b)
    with pytest.raises(TypeError):
        ssim_loss(a.numpy(), b.numpy())
