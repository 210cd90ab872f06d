"""CPU: the yardstick of the MS-SSIM loss (tests/msssim_reference.py) against itself (closed forms, the single level, dropped rows),
rdst_amd.metrics.msssim against it, the default weights, every refusal of the C entry points (rdst_msssim_loss*,
include/rdst_hip_msssim.h: refused before any launch, so the pointers passed are never dereferenced), the Python layer's own
refusals, and the gradient gate of test_msssim_loss_gpu.py applied to gradients that are wrong on purpose."""
import types

import numpy as np
import pytest
import torch

import msssim_reference as MR
import ssim_reference as R
from rdst_amd import _lib
from rdst_amd import metrics as M

FAKE = 256          # a non-null "device pointer" for calls that must be refused before any launch


# ---- the yardstick ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,window,win,last", [((2, 1, 40, 70), "g", 11, False), ((1, 3, 23, 37), "g", 5, False),
                                                   ((1, 2, 19, 16), "u", 7, False), ((1, 2, 19, 16), "u", 7, True)], ids=str)
def test_closed_form_level_gradient_is_autograd(shape, window, win, last):
    g, p = R.images(shape, 6)
    taps, cn = R.taps_of(window, win)
    X, Y = g.double(), p.double().requires_grad_(True)
    MR.level_mean(X, Y, taps, cn, 1.0, last).sum().backward()
    closed = MR.closed_form_level_grad(X, Y.detach(), taps, cn, 1.0, last)
    assert float((Y.grad - closed).abs().max()) <= 1e-15


@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_terms_sum_to_the_gradient_and_the_composition_is_autograd(case):
    ref = MR.case(*case)
    total = sum(ref["terms"])
    scale = float(ref["grad"].abs().max())
    assert float((total - ref["grad"]).abs().max()) <= 1e-14 * scale
    composed = MR.composed_grad(ref["target"], ref["pred"], ref["taps"], ref["cn"], 1.0, ref["weights"])
    assert float((composed - ref["grad"]).abs().max()) <= 1e-13 * scale
    assert float(ref["means"].min()) > 0.9                  # no plane of the GPU cases is clamped
    assert abs(float(ref["loss"]) - (1.0 - float(ref["msssim"].mean()))) <= 1e-15


def test_single_level_is_the_ssim_reference():
    g, p = R.images((2, 1, 23, 37), 5)
    taps, cn = R.taps_of("g", 11)
    ref = MR.reference(g, p, taps, cn, 1.0, np.array([1.0]))
    ssim, loss, grad = R.reference(g, p, taps, cn, 1.0)
    assert float((ref["msssim"] - ssim).abs().max()) <= 1e-15 and abs(float(ref["loss"] - loss)) <= 1e-15
    assert float((ref["grad"] - grad).abs().max()) <= 1e-15 * float(grad.abs().max()) + 1e-18


def test_coarse_terms_vanish_on_dropped_rows_and_columns():
    ref = MR.case(1, 1, 37, 43, "g", 5, 3)
    t1, t2, t3 = ref["terms"]
    assert float(t1[..., 36, :].abs().max()) > 0 and float(t1[..., :, 42].abs().max()) > 0
    for t in (t2, t3):
        assert torch.all(t[..., 36, :] == 0) and torch.all(t[..., :, 42] == 0)
    # level 2 is 18 x 21: its column 20 is dropped on the way to level 3, pixels 40 and 41 of level 1
    assert torch.all(t3[..., :, 40:] == 0) and float(t2[..., :36, 40:42].abs().max()) > 0


def test_clamped_plane_has_zero_gradient_and_is_finite():
    g, p = R.images((2, 1, 40, 48), 17)
    p[0] = 1.0 - g[0]
    taps, cn = R.taps_of("g", 5)
    ref = MR.reference(g, p, taps, cn, 1.0, np.array([0.2, 0.3, 0.5]))
    assert float(ref["means"][0].max()) < -0.8 and float(ref["msssim"][0]) == 0.0
    assert torch.all(ref["grad"][0] == 0) and torch.isfinite(ref["grad"]).all() and float(ref["grad"][1].abs().max()) > 0
    assert all(torch.all(t[0] == 0) for t in ref["terms"])


# ---- the gate catches mistakes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_gradient_gate_refuses_wrong_gradients(case):
    """The GPU test's gate, (levels + 2) roundings, passes the float64 composition rounded to fp32 and fails each mutation.
    'clamp_dropped' changes something only where a level has an odd side (37 x 43 among the cases): there it must fail, and
    elsewhere the mutated gradient is the right one, bit for bit."""
    N, C, H, W, _, _, levels = case
    ref = MR.case(*case)
    args = (ref["target"], ref["pred"], ref["taps"], ref["cn"], 1.0, ref["weights"])
    good = MR.composed_grad(*args)
    assert MR.gate_excess(good.float(), ref, levels + 2)[0] <= 0
    for mutation in ("no_quarter", "weight_shift", "s_at_level_1"):
        assert MR.gate_excess(MR.composed_grad(*args, mutation=mutation).float(), ref, levels + 2)[0] > 0, mutation
    clamped = MR.composed_grad(*args, mutation="clamp_dropped")
    if any((H >> j) % 2 or (W >> j) % 2 for j in range(levels - 1)):
        assert MR.gate_excess(clamped.float(), ref, levels + 2)[0] > 0
    else:
        assert torch.equal(clamped, good)


# ---- metrics.msssim -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,levels,margin", [((2, 3, 50, 60), 2, 0), ((2, 1, 184, 200), 5, 4), ((1, 2, 101, 95), 4, 3)], ids=str)
def test_metrics_msssim_is_the_reference(shape, levels, margin):
    g, p = R.images(shape, 8)
    H, W = shape[-2:]
    gc, pc = g[..., margin:H - margin, margin:W - margin], p[..., margin:H - margin, margin:W - margin]
    taps, cn = R.taps_of("g", 11)
    want = MR.reference(gc, pc, taps, cn, 1.0, MR.default_weights(levels))["msssim"]
    for n in range(shape[0]):
        got = M.msssim(gc[n].numpy().transpose(1, 2, 0), pc[n].numpy().transpose(1, 2, 0), levels=levels)
        assert abs(got - float(want[n])) <= 1e-12
    # SRMetrics on the host: tensors, HWC arrays and lists of them, cropped by the margin
    sm = M.SRMetrics("psnr msssim") if levels == 5 else None
    if sm is not None:
        for gts, preds in ((g, p), (list(g), list(p)), (g.numpy().transpose(0, 2, 3, 1), p.numpy().transpose(0, 2, 3, 1)),
                           ([a.numpy().transpose(1, 2, 0) for a in g], [a.numpy().transpose(1, 2, 0) for a in p])):
            rep = sm(gts, preds, margin)
            assert list(rep) == ["psnr", "msssim"] and np.abs(np.asarray(rep["msssim"]) - want.numpy()).max() <= 1e-12


def test_metrics_msssim_refusals_and_other_windows():
    g, p = R.images((1, 1, 60, 64), 9)
    a, b = g[0, 0].numpy(), p[0, 0].numpy()
    taps, cn = R.taps_of("g", 7, 1.0)
    want = MR.reference(g, p, taps, cn, 255.0, np.array([0.5, 0.25, 0.25]))["msssim"]
    assert abs(M.msssim(a, b, 255.0, 3, (0.5, 0.25, 0.25), 7, 1.0) - float(want[0])) <= 1e-12
    with pytest.raises(ValueError, match="176"):
        M.msssim(a, b)
    with pytest.raises(ValueError):
        M.msssim(a, b, levels=6)
    with pytest.raises(ValueError):
        M.msssim(a, b, levels=2, weights=(0.5, -0.5))
    with pytest.raises(ValueError):
        M.SRMetrics("psnr fid")


def test_default_weights():
    from rdst_amd.loss import level_weights
    w = level_weights(5)
    assert w.dtype == np.float64 and w.tolist() == [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
    w3 = level_weights(3)
    assert np.array_equal(w3, np.array([0.0448, 0.2856, 0.3001]) / np.array([0.0448, 0.2856, 0.3001]).sum())
    assert abs(w3.sum() - 1.0) <= 1e-15 and level_weights(1).tolist() == [1.0]
    assert level_weights(2, (0.3, 0.9)).tolist() == [0.3, 0.9]              # given weights are taken as they are
    for bad in (dict(levels=0), dict(levels=6), dict(levels=2, weights=(1.0,)), dict(levels=2, weights=(1.0, 0.0)),
                dict(levels=2, weights=(1.0, float("nan"))), dict(levels=2, weights=(float("inf"), 1.0))):
        with pytest.raises(ValueError):
            level_weights(**bad)


# ---- the C entry points -------------------------------------------------------------------------------------------------

def _call(N=2, C=3, H=40, W=36, win=5, taps="default", cov_norm=1.0, data_range=1.0, levels=3, weights=(0.2, 0.3, 0.5), target=FAKE,
          pred=FAKE, msssim=FAKE, means=FAKE, loss=FAKE, grad=FAKE, ws=FAKE, ws_bytes=1 << 24):
    lib = _lib.load()
    keep = None if taps is None or isinstance(taps, str) else np.ascontiguousarray(taps, dtype=np.float64)
    wk = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rc = lib.rdst_msssim_loss(target, pred, N, C, H, W, win, None if keep is None else keep.ctypes.data, cov_norm, data_range,
                              levels, None if wk is None else wk.ctypes.data, msssim, means, loss, grad, ws, ws_bytes, None)
    return rc, lib.rdst_last_error().decode()


def _ws(*a):
    return _lib.load().rdst_msssim_loss_workspace(*a)


def test_workspace_query():
    for shape in ((2, 3, 40, 36, 5, 3), (1, 1, 176, 176, 11, 5), (32, 1, 256, 256, 11, 5), (1, 1, 7, 7, 7, 1), (1, 1, 37, 43, 5, 3)):
        v, g = _ws(*shape, 0), _ws(*shape, 1)
        assert v > 0 and v % 16 == 0 and g % 16 == 0, shape
        # the gradient adds the running sums of the levels 2 .. M: the pooled images once more
        pooled = sum(((shape[0] * shape[1] * (shape[2] >> j) * (shape[3] >> j) * 4 + 15) & ~15) for j in range(1, shape[5]))
        assert g - v == pooled, shape
    for shape in ((0, 1, 40, 40, 5, 3), (1, 0, 40, 40, 5, 3), (1, 1, -40, 40, 5, 3), (1, 1, 40, 40, 6, 3), (1, 1, 40, 40, 17, 1),
                  (1, 1, 40, 40, 5, 0), (1, 1, 40, 40, 5, 6), (1, 1, 40, 19, 5, 3), (1, 1, 175, 256, 11, 5),
                  (1 << 16, 1, 256, 257, 7, 2)):
        assert _ws(*shape, 1) == 0, shape
        assert "rdst_msssim_loss_workspace" in _lib.load().rdst_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(N=0), "bad shape"), (dict(C=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"),
    (dict(win=2), "win"), (dict(win=6), "win"), (dict(win=17), "win"),
    (dict(levels=0), "levels"), (dict(levels=6), "levels"), (dict(levels=-1), "levels"),
    (dict(W=19), "too small"), (dict(H=39, levels=4, weights=(0.25,) * 4), "too small"), (dict(H=4, levels=1, weights=(1.0,)), "too small"),
    (dict(N=1 << 16, C=1, H=256, W=257), "2^31"),
    (dict(target=None), "null pointer"), (dict(pred=None), "null pointer"), (dict(msssim=None), "null pointer"),
    (dict(ws=None), "null pointer"), (dict(weights=None), "null pointer"),
    (dict(ws_bytes=0), "workspace"),
    (dict(weights=(0.2, 0.0, 0.5)), "weight"), (dict(weights=(0.2, -0.3, 0.5)), "weight"),
    (dict(weights=(0.2, 0.3, float("nan"))), "weight"), (dict(weights=(float("inf"), 0.3, 0.5)), "weight"),
    (dict(taps=[0.2, 0.2, 0.2, 0.2, float("nan")]), "finite"),
    (dict(taps=[0.2] * 4 + [0.2 + 1e-8]), "sum"),
    (dict(cov_norm=0.0), "cov_norm"), (dict(cov_norm=float("nan")), "cov_norm"),
    (dict(data_range=0.0), "data_range"), (dict(data_range=float("nan")), "data_range"),
], ids=lambda v: v if isinstance(v, str) else ",".join(f"{a}={b}" for a, b in v.items())[:40])
def test_refusals(kw, word):
    rc, msg = _call(**kw)
    assert rc == _lib.EINVAL and "rdst_msssim_loss" in msg and word in msg, (rc, msg)


def test_too_small_names_the_least_side_and_short_workspace_the_size():
    rc, msg = _call(H=175, W=300, win=11, levels=5, weights=MR.PUBLISHED)
    assert rc == _lib.EINVAL and "too small" in msg and "176" in msg
    for with_grad in (0, 1):
        need = _ws(2, 3, 40, 36, 5, 3, with_grad)
        rc, msg = _call(ws_bytes=need - 1, grad=FAKE if with_grad else None)
        assert rc == _lib.EINVAL and "workspace" in msg and str(need) in msg


def test_signatures_bound_and_abi_version_unchanged():
    assert set(_lib.MSSSIM_SIGNATURES) == {"rdst_msssim_loss", "rdst_msssim_loss_workspace"}
    assert not set(_lib.MSSSIM_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.LRC_SIGNATURES))
    assert _lib.MSSSIM_PARAMS["rdst_msssim_loss"] == (
        "target", "pred", "N", "C", "H", "W", "win", "taps", "cov_norm", "data_range", "levels", "weights", "msssim", "means",
        "loss", "grad", "workspace", "workspace_bytes", "stream")
    lib = _lib.load()
    assert lib.rdst_msssim_loss.argtypes == _lib.MSSSIM_SIGNATURES["rdst_msssim_loss"][1]
    assert lib.rdst_abi_version() == _lib.ABI_VERSION == 11


# ---- the Python layer ---------------------------------------------------------------------------------------------------

def _paras(**kw):
    return types.SimpleNamespace(gpu_id=-1, precision=False, training_losses=["L1", "MSSSIM"],
                                 loss_scalars={"S": {"L1": 0.16, "MSSSIM": 0.84}}, training_states=["S"], **kw)


def test_srloss_builds_with_msssim():
    from rdst_amd.loss import MSSSIMLoss, SRLoss
    sl = SRLoss(_paras())
    assert sl.loss_components == ["Rec_L1", "Rec_MSSSIM"]
    f = sl.loss_functions["MSSSIM"]
    assert isinstance(f, MSSSIMLoss) and f.loss_names == ["Rec_MSSSIM"]
    assert (f.levels, f.weights, f.window, f.win_size, f.sigma, f.data_range) == (5, None, "gaussian", None, 1.5, 1.0)
    f = SRLoss(_paras(msssim_levels=3, msssim_weights=(0.2, 0.3, 0.5), msssim_window="uniform", msssim_win_size=9,
                      msssim_sigma=2.0, msssim_data_range=255.0)).loss_functions["MSSSIM"]
    assert (f.levels, f.weights, f.window, f.win_size, f.sigma, f.data_range) == (3, (0.2, 0.3, 0.5), "uniform", 9, 2.0, 255.0)
    for bad in (dict(msssim_levels=6), dict(msssim_win_size=8), dict(msssim_levels=2, msssim_weights=(1.0,)),
                dict(msssim_data_range=0.0), dict(msssim_window="box")):
        with pytest.raises(ValueError):
            SRLoss(_paras(**bad))
    for other in ("VGG54", "GAN"):
        p = _paras()
        p.training_losses = ["L1", other]
        with pytest.raises(NotImplementedError, match="SSIM and LRC are this repository's own"):
            SRLoss(p)


def test_ms_ssim_loss_refuses_before_the_device():
    from rdst_amd.loss import SRLoss, ms_ssim_loss
    a, b = torch.rand(1, 1, 176, 176), torch.rand(1, 1, 176, 176)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms_ssim_loss(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SRLoss(_paras())(a, b)
    with pytest.raises(TypeError):
        ms_ssim_loss(a.numpy(), b.numpy())
    with pytest.raises(TypeError):
        M.device_msssim(a.numpy(), b.numpy())
    with pytest.raises(ValueError, match="176"):
        M.device_msssim(a, b, margin=1)               # the size is checked before the device is
    with pytest.raises(ValueError):
        M.device_msssim(a, b, levels=3, weights=(1.0, 1.0))
