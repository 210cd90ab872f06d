"""CPU: the host side of the LR-consistency feature (rdst_amd.data.adjoint_table / operator_norm, rdst_amd.loss.consistency,
SRLoss 'LRC', SRTester(back_project=...)): the transposed tables against the dense float64 matrices, the step size of the
back-projection in float64 numpy, the argument handling, and every refusal that happens before the device (the library loads
without a GPU, and the C entry points return before any launch)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from rdst_amd import _lib
from rdst_amd import data as D

# (n_in, n_out) of every axis of the shapes tests/test_consistency_gpu.py runs
AXES = [(24, 6), (40, 10), (21, 8), (40, 16), (64, 8), (72, 18), (104, 26), (256, 64), (24, 8), (520, 130), (20, 5)]


def dense(index, weight, n_cols):
    M = np.zeros((index.shape[0], n_cols))
    np.add.at(M, (np.arange(index.shape[0])[:, None], index), weight)
    return M


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("n_in, n_out", AXES)
def test_adjoint_table_is_the_transpose(kind, n_in, n_out):
    fi, fw = D.operator_table(kind, n_in, n_out)
    ti, tw = D.adjoint_table(kind, n_in, n_out)
    assert ti.dtype == np.int32 and tw.dtype == np.float64 and ti.shape == tw.shape == (n_in, ti.shape[1])
    assert ti.shape[1] > 0 and ti.shape[1] % 4 == 0
    assert ti.min() >= 0 and ti.max() < n_out
    M, MT = dense(fi, fw, n_in), dense(ti, tw, n_out)
    assert np.abs(MT - M.T).max() <= 1e-15
    # taps ascend; padding repeats the last index with weight 0; a row's real taps are the outputs whose table names it with
    # a weight that is not exactly 0
    reads = [sorted({o for o in range(n_out) if i in fi[o] and M[o, i] != 0}) for i in range(n_in)]
    for i in range(n_in):
        n = len(reads[i])
        if n == 0:
            assert not tw[i].any() and not ti[i].any()
            continue
        assert list(ti[i, :n]) == reads[i]
        assert (ti[i, n:] == reads[i][-1]).all() and not tw[i, n:].any()
    assert ti.shape[1] == max(4, -(-max(len(r) for r in reads) // 4) * 4)


@pytest.mark.parametrize("n_in, n_out", [(64, 8), (24, 8)])
def test_cubic_has_source_samples_nobody_reads(n_in, n_out):
    ti, tw = D.adjoint_table("cubic", n_in, n_out)
    empty = ~tw.any(axis=1)
    assert empty.any() and not ti[empty].any()
    fi, fw = D.operator_table("cubic", n_in, n_out)
    assert set(np.flatnonzero(empty)) == set(range(n_in)) - set(fi[fw != 0].tolist())


def test_cubic_border_taps_are_merged_by_one_addition():
    fi, fw = D.operator_table("cubic", 21, 8)
    ti, tw = D.adjoint_table("cubic", 21, 8)
    assert (fi[0] == 0).sum() == 2                                  # the clamped taps of output 0 meet on sample 0
    assert ti[0, 0] == 0 and tw[0, 0] == fw[0, 0] + fw[0, 1]


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("n_in, n_out", AXES)
def test_operator_norm(kind, n_in, n_out):
    M = dense(*D.operator_table(kind, n_in, n_out), n_in)
    assert D.operator_norm(kind, n_in, n_out) == float(np.linalg.norm(M, 2))


def test_operator_norm_at_x4():
    got = {k: D.operator_norm(k, 256, 64) for k in D.KINDS}
    assert abs(got["cubic"] - 0.8501) < 1e-4 and abs(got["cubic+gaussian"] - 0.857) < 1e-3
    assert abs(got["cubic_aa"] - 0.503) < 1e-3 and abs(got["fourier"] - 0.70710678) < 1e-7
    assert D.operator_norm(D.Degradation("cubic+gaussian", blur_kernel=5), 64, 16) != D.operator_norm("cubic+gaussian", 64, 16)
    with pytest.raises(ValueError, match="options go with a kind's name"):
        D.adjoint_table(D.Degradation("cubic"), 8, 2, blur_kernel=3)


def _landweber(kind, n_in, n_out, steps):
    A = dense(*D.operator_table(kind, n_in, n_out), n_in)
    tau = 1.0 / (D.operator_norm(kind, n_in, n_out) ** 4)
    rng = np.random.default_rng(3)
    P, lr = rng.random((n_in, n_in)), rng.random((n_out, n_out))
    rms = []
    for _ in range(steps + 1):
        R = A @ P @ A.T - lr
        rms.append(float(np.sqrt(np.mean(R * R))))
        P = P - tau * (A.T @ R @ A)
    return rms


@pytest.mark.parametrize("kind", ["cubic+gaussian", "cubic_aa", "fourier"])
def test_landweber_steps_shrink_the_residual(kind):
    rms = _landweber(kind, 64, 16, 5)
    assert all(b < a for a, b in zip(rms, rms[1:])), rms


def test_one_landweber_step_solves_cubic_x4():
    """The rows of the x4 cubic operator are disjoint and of one length, so A A^T is a multiple of the identity and the step
    1 / |A|^4 lands on the solution."""
    rms = _landweber("cubic", 64, 16, 1)
    assert rms[1] < 1e-10 * rms[0], rms


# ---- SRLoss 'LRC' ------------------------------------------------------------------------------------------------------------
def _paras(**kw):
    return types.SimpleNamespace(gpu_id=-1, precision=False, training_losses=["L1", "LRC"],
                                 loss_scalars={"S": {"L1": 1.0, "LRC": 0.1}}, training_states=["S"], sr_scale=4, **kw)


def test_srloss_builds_the_component_from_paras():
    from rdst_amd.loss import LRConsistencyLoss, SRLoss
    sl = SRLoss(_paras())
    f = sl.loss_functions["LRC"]
    assert isinstance(f, LRConsistencyLoss) and sl.loss_components == ["Rec_L1", "Rec_LRC"]
    assert (f.degradation, f.scale, f.norm) == (D.Degradation("cubic"), 4, "l1")
    f = SRLoss(_paras(blur_method="gaussian", blur_kernel=5)).loss_functions["LRC"]
    assert f.degradation == D.Degradation("cubic+gaussian", blur_kernel=5)
    f = SRLoss(_paras(lrc_degradation="fourier", lrc_norm="L2", lrc_scale=2, blur_method="gaussian")).loss_functions["LRC"]
    assert (f.degradation, f.scale, f.norm) == (D.Degradation("fourier"), 2, "l2")
    with pytest.raises(ValueError, match="norm"):
        SRLoss(_paras(lrc_norm="huber"))
    with pytest.raises(ValueError, match="scale"):
        SRLoss(_paras(lrc_scale=2.5))
    with pytest.raises(ValueError, match="kind"):
        SRLoss(_paras(lrc_degradation="lanczos"))


def test_srloss_still_refuses_what_is_out_of_scope():
    from rdst_amd.loss import SRLoss
    p = _paras()
    p.training_losses = ["L1", "VGG54"]
    with pytest.raises(NotImplementedError, match=r"'VGG54'.*SSIM and LRC are this repository's own"):
        SRLoss(p)


# ---- refusals before the device ----------------------------------------------------------------------------------------------
def test_python_refusals():
    from rdst_amd.loss import LRConsistencyLoss, lr_consistency_loss, lrc_adjoint, lrc_residual
    from rdst_amd.tester import SRTester
    pred, lr = torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lr_consistency_loss(pred, lr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lrc_residual(pred, lr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lrc_adjoint(lr, (16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.resample_adjoint(lr, (16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.degrade(pred, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LRConsistencyLoss("cubic", 4)(pred, pred)
    with pytest.raises(ValueError, match="not a multiple of the scale"):
        LRConsistencyLoss("cubic", 4)(torch.zeros(1, 1, 18, 16), torch.zeros(1, 1, 18, 16))
    with pytest.raises(ValueError, match="must have one shape"):
        LRConsistencyLoss("cubic", 4)(torch.zeros(1, 1, 32, 32), pred)
    with pytest.raises(ValueError, match="'l1' or 'l2'"):
        lr_consistency_loss(pred, lr, norm="l3")
    with pytest.raises(TypeError, match="torch tensors"):
        lr_consistency_loss(pred.numpy(), lr)
    with pytest.raises(TypeError, match="a Degradation or the name"):
        lr_consistency_loss(pred, lr, degradation=3)

    net = torch.nn.Conv2d(1, 1, 1)
    net.sr_scale = 4
    assert SRTester(net).back_project == 0
    t = SRTester(net, back_project=3, degradation="fourier", bp_step=0.5)
    assert (t.back_project, t.degradation, t.bp_step) == (3, D.Degradation("fourier"), 0.5)
    assert SRTester(net, back_project=2).degradation == D.Degradation("cubic")
    with pytest.raises(ValueError, match="integer scale"):
        SRTester(net, sr_scale=2.5, back_project=1)
    SRTester(net, sr_scale=2.5)                                        # without back-projection the scale is not looked at
    with pytest.raises(ValueError, match="back_project"):
        SRTester(net, back_project=-1)
    with pytest.raises(ValueError, match="back_project"):
        SRTester(net, back_project=1.5)
    with pytest.raises(ValueError, match="bp_step"):
        SRTester(net, back_project=1, bp_step=0.0)
    with pytest.raises(ValueError, match="kind"):
        SRTester(net, back_project=1, degradation="lanczos")


def test_binding_comes_from_the_third_header():
    assert set(_lib.LRC_SIGNATURES) == {"rdst_lrc_workspace", "rdst_lrc_residual", "rdst_lrc_adjoint"}
    assert not set(_lib.LRC_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DATA_SIGNATURES))
    assert _lib.LRC_PARAMS["rdst_lrc_adjoint"] == ("g", "N", "C", "oh", "ow", "H", "W", "KyT", "index_yT", "weight_yT", "KxT",
                                                   "index_xT", "weight_xT", "scale_dev", "scale_host", "base", "out", "stream")
    lib = _lib.load()
    for name, (res, args) in _lib.LRC_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res


def test_c_entry_points_refuse_before_any_launch():
    """Every argument check returns before a launch, so the calls run without a GPU on made-up (aligned) addresses."""
    lib = _lib.load()
    P, Q = 0x10000, 0x10004                                            # Q: not 16-byte aligned

    def residual(**kw):
        a = dict(pred=P, lr=P, N=1, C=1, H=16, W=16, oh=4, ow=4, Ky=4, index_y=P, weight_y=P, Kx=4, index_x=P, weight_x=P,
                 norm=1, resid=P, g=P, loss=P, workspace=P, workspace_bytes=1 << 20, stream=None)
        a.update(kw)
        return lib.rdst_lrc_residual(*[a[k] for k in _lib.LRC_PARAMS["rdst_lrc_residual"]])

    def adjoint(**kw):
        a = dict(g=P, N=1, C=1, oh=4, ow=4, H=16, W=16, KyT=4, index_yT=P, weight_yT=P, KxT=4, index_xT=P, weight_xT=P,
                 scale_dev=None, scale_host=1.0, base=None, out=P, stream=None)
        a.update(kw)
        return lib.rdst_lrc_adjoint(*[a[k] for k in _lib.LRC_PARAMS["rdst_lrc_adjoint"]])

    def says(rc, code, text):
        assert rc == code and text in lib.rdst_last_error().decode()

    says(residual(H=0), _lib.EINVAL, "bad shape")
    says(residual(pred=None), _lib.EINVAL, "null pointer")
    says(residual(norm=3), _lib.EINVAL, "norm=3")
    says(residual(norm=0), _lib.EINVAL, "g and loss must be null")
    says(residual(resid=None, g=None, loss=None), _lib.EINVAL, "nothing to write")
    says(residual(Ky=6), _lib.EINVAL, "K y=6")
    says(residual(index_x=Q), _lib.EINVAL, "16-byte aligned")
    says(residual(weight_y=None), _lib.EINVAL, "null tap table")
    says(residual(workspace_bytes=4), _lib.EINVAL, "workspace of 4 bytes")
    says(residual(workspace=None), _lib.EINVAL, "workspace of 0 bytes")
    says(residual(H=8200, W=8, oh=2050, ow=2), _lib.ENOTSUP, "larger than the LDS holds")
    says(adjoint(W=-1), _lib.EINVAL, "bad shape")
    says(adjoint(out=None), _lib.EINVAL, "null pointer")
    says(adjoint(KxT=0), _lib.EINVAL, "K xT=0")
    says(adjoint(weight_xT=Q), _lib.EINVAL, "16-byte aligned")
    says(adjoint(oh=8200, ow=2, H=32800, W=8), _lib.ENOTSUP, "larger than the LDS holds")
    assert lib.rdst_lrc_workspace(2, 3, 6, 10) >= 2 * 3 * 10 * 8 and lib.rdst_lrc_workspace(0, 1, 4, 4) == 0
    assert isinstance(ctypes.c_size_t(lib.rdst_lrc_workspace(1, 1, 1, 1)).value, int)
