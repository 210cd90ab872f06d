"""GPU: the MS-SSIM loss and score (rdst_msssim_loss, rdst_amd.loss.ms_ssim_loss / MSSSIMLoss / SRLoss 'MSSSIM',
rdst_amd.metrics.device_msssim) against the float64 reference of tests/msssim_reference.py on seeded images.  The gates:
  |msssim[n] - ref| <= 1e-10, |means - ref| <= 1e-10     the scoring kernel's own tolerance (test_srmetrics_gpu.py)
  |loss - ref|      <= 2^-23
  C ABI:     |grad - g64| <= (levels + 2) 2^-24 sum_j |t_j| + 1e-10 max|g64|
             at most one fp32 rounding of the running sum per level, two more for a design that keeps k or the per-level image
             in fp32, each relative to a partial sum that sum_j |t_j| (the per-level terms of the reference) bounds
  autograd:  levels + 3 roundings (one more fp32 multiply by the upstream gradient)"""
import types

import numpy as np
import pytest
import torch

import msssim_reference as MR
import ssim_reference as R
from oracle import rdst_oracle as O
from rdst_amd import _lib
from rdst_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_VALUE, TOL_LOSS = 1e-10, 2.0 ** -23
WINDOW = {"u": "uniform", "g": "gaussian"}


def _raw(target, pred, taps, cn, weights, dr=1.0, want_grad=True, want_means=True):
    """rdst_msssim_loss through the C ABI: (msssim fp64 (N,), means fp64 (N, C, M), loss fp32 (), grad fp32 or None)."""
    N, C, H, W = pred.shape
    win, levels = len(taps), len(weights)
    lib = _lib.load()
    nb = lib.rdst_msssim_loss_workspace(N, C, H, W, win, levels, int(want_grad))
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)                 # NaNs where nothing was written
    msssim = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    means = torch.full((N, C, levels), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    grad = torch.full(pred.shape, float("nan"), dtype=torch.float32, device=DEV) if want_grad else None
    tp = np.ascontiguousarray(taps, dtype=np.float64)
    wt = np.ascontiguousarray(weights, dtype=np.float64)
    _lib.check(lib.rdst_msssim_loss(target.data_ptr(), pred.data_ptr(), N, C, H, W, win, tp.ctypes.data, cn, dr, levels,
                                    wt.ctypes.data, msssim.data_ptr(), means.data_ptr() if want_means else None, loss.data_ptr(),
                                    grad.data_ptr() if want_grad else None, ws.data_ptr(), nb,
                                    torch.cuda.current_stream().cuda_stream), "rdst_msssim_loss")
    torch.cuda.synchronize()
    return msssim, means, loss, grad


def _check_value(ref, msssim, means, loss, images=slice(None)):
    e_ms = float((msssim.cpu() - ref["msssim"])[images].abs().max())
    e_mean = float((means.cpu() - ref["means"])[images].abs().max())
    e_loss = abs(float(loss) - float(ref["loss"]))
    print(f"msssim: max|err| {e_ms:.3e}; means: max|err| {e_mean:.3e}; loss err {e_loss:.3e}")
    assert torch.isfinite(msssim).all() and torch.isfinite(means).all() and torch.isfinite(loss)
    assert e_ms <= TOL_VALUE and e_mean <= TOL_VALUE and e_loss <= TOL_LOSS


def _gate(got, ref, roundings, scale=1.0):
    assert torch.isfinite(got).all()
    excess, err = MR.gate_excess(got, ref, roundings, scale)
    print(f"gradient: max|err| {err:.3e}, max|g64| {scale * float(ref['grad'].abs().max()):.3e}, worst err - tol {excess:.3e}")
    assert excess <= 0, (err, excess)


@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_parity_c_abi(case):
    levels = case[6]
    ref = MR.case(*case)
    g, p = ref["target"].to(DEV), ref["pred"].to(DEV)
    msssim, means, loss, grad = _raw(g, p, ref["taps"], ref["cn"], ref["weights"])
    _check_value(ref, msssim, means, loss)
    _gate(grad, ref, levels + 2)
    # value only: the same bits, with and without the means; and a second run of the gradient call
    ms0, mean0, loss0, _ = _raw(g, p, ref["taps"], ref["cn"], ref["weights"], want_grad=False)
    assert torch.equal(ms0, msssim) and torch.equal(mean0, means) and torch.equal(loss0, loss)
    ms1, _, loss1, _ = _raw(g, p, ref["taps"], ref["cn"], ref["weights"], want_grad=False, want_means=False)
    assert torch.equal(ms1, msssim) and torch.equal(loss1, loss)
    again = _raw(g, p, ref["taps"], ref["cn"], ref["weights"])
    assert all(torch.equal(a, b) for a, b in zip(again, (msssim, means, loss, grad)))


@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_parity_autograd(case):
    from rdst_amd.loss import ms_ssim_loss
    N, C, H, W, window, win, levels = case
    ref = MR.case(*case)
    g = ref["target"].to(DEV)
    p = ref["pred"].to(DEV).requires_grad_(True)
    loss, msssim = ms_ssim_loss(p, g, levels, None, WINDOW[window], win, return_msssim=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert msssim.shape == (N,) and msssim.dtype == torch.float64 and not msssim.requires_grad
    (loss * 0.37).backward()
    assert float((msssim.cpu() - ref["msssim"]).abs().max()) <= TOL_VALUE
    assert abs(float(loss.detach()) - float(ref["loss"])) <= TOL_LOSS
    _gate(p.grad, ref, levels + 3, scale=float(np.float32(0.37)))
    # the value alone (no gradient asked for) has the same bits; the defaults need not be named
    assert torch.equal(ms_ssim_loss(p.detach(), g, levels, None, WINDOW[window], win), loss.detach())
    if (window, win, levels) == ("g", 11, 5):
        assert torch.equal(ms_ssim_loss(p.detach(), g), loss.detach())


@pytest.mark.parametrize("shape,window,win", [((2, 1, 33, 65), "g", 11), ((1, 1, 23, 37), "u", 7), ((2, 1, 70, 150), "g", 5)], ids=str)
def test_single_level_is_the_ssim_loss(shape, window, win):
    g, p = R.images(shape, 17)
    g, p = g.to(DEV), p.to(DEV)
    taps, cn = R.taps_of(window, win)
    msssim, means, loss, grad = _raw(g, p, taps, cn, [1.0])
    N, C, H, W = shape
    lib = _lib.load()
    nb = lib.rdst_ssim_loss_workspace(N, C, H, W, win)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    ssim = torch.empty(N, dtype=torch.float64, device=DEV)
    sloss = torch.empty((), dtype=torch.float32, device=DEV)
    sgrad = torch.empty_like(p)
    tp = np.ascontiguousarray(taps, dtype=np.float64)
    _lib.check(lib.rdst_ssim_loss(g.data_ptr(), p.data_ptr(), N, C, H, W, win, tp.ctypes.data, cn, 1.0, ssim.data_ptr(),
                                  sloss.data_ptr(), sgrad.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream),
               "rdst_ssim_loss")
    torch.cuda.synchronize()
    assert float((msssim - ssim).abs().max()) <= 1e-12 and float((means.reshape(N) - ssim).abs().max()) <= 1e-12
    assert abs(float(loss) - float(sloss)) <= 2.0 ** -23
    a, b = grad.double(), sgrad.double()
    tol = 2 * 2.0 ** -24 * b.abs() + 1e-10 * b.abs().max()
    print(f"single level: max|grad - ssim grad| {float((a - b).abs().max()):.3e}")
    assert float(((a - b).abs() - tol).max()) <= 0


@pytest.mark.parametrize("window,win,levels", [("g", 5, 3), ("g", 11, 2), ("u", 7, 3)], ids=str)
def test_identical_images(window, win, levels):
    """pred == target: cs = S = 1 at every position of every level, and the gradient is analytically zero."""
    N, C, H, W = 2, 3, 61, 57
    g, _ = R.images((N, C, H, W), 3)
    g = g.to(DEV)
    taps, cn = R.taps_of(window, win)
    msssim, means, loss, grad = _raw(g, g.clone(), taps, cn, MR.default_weights(levels))
    print(f"loss {float(loss):.3e}, max|grad| {float(grad.abs().max()):.3e}, max|1 - mean| {(1 - means).abs().max().item():.3e}")
    assert float(loss) <= 1e-12 and float((1 - means).abs().max()) <= 1e-12 and float((1 - msssim).abs().max()) <= 1e-12
    assert torch.isfinite(grad).all()
    assert float(grad.abs().max()) <= 1e-9 / (N * C)


def test_clamped_plane():
    """Image 0 is the target's negative: every level mean is negative there (-0.988, -0.950, -0.820 in the reference), so its
    MS-SSIM is exactly 0 and its gradient exactly 0.0; image 1 holds the gates against the reference of the whole batch."""
    g, p = R.images((2, 1, 40, 48), 17)
    p[0] = 1.0 - g[0]
    taps, cn = R.taps_of("g", 5)
    weights = np.array([0.2, 0.3, 0.5])
    ref = MR.reference(g, p, taps, cn, 1.0, weights)
    assert float(ref["means"][0].max()) < -0.8
    msssim, means, loss, grad = _raw(g.to(DEV), p.to(DEV), taps, cn, weights)
    assert torch.isfinite(msssim).all() and torch.isfinite(means).all() and torch.isfinite(loss) and torch.isfinite(grad).all()
    assert float(msssim[0]) == 0.0 and torch.all(grad[0] == 0)
    _check_value(ref, msssim, means, loss)
    _gate(grad, ref, 3 + 2)
    assert float(grad[1].abs().max()) > 0
    from rdst_amd.loss import ms_ssim_loss
    q = p.to(DEV).requires_grad_(True)
    ms_ssim_loss(q, g.to(DEV), 3, weights, "gaussian", 5).backward()
    assert torch.isfinite(q.grad).all() and torch.all(q.grad[0] == 0) and torch.equal(q.grad, grad)


def test_non_contiguous_inputs_and_refusals():
    from rdst_amd.loss import ms_ssim_loss
    ref = MR.case(1, 2, 24, 28, "u", 3, 3)
    g, p = ref["target"].to(DEV), ref["pred"].to(DEV)
    pt = p.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)       # same values, column-major planes
    gt = g.transpose(2, 3).contiguous().transpose(2, 3)
    assert not pt.is_contiguous()
    loss = ms_ssim_loss(pt, gt, 3, None, "uniform", 3)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) <= TOL_LOSS
    _gate(pt.grad, ref, 3 + 3)
    kw = dict(levels=3, window="uniform", win_size=3)
    with pytest.raises(ValueError):
        ms_ssim_loss(p, g.clone().requires_grad_(True), **kw)
    with pytest.raises(TypeError):
        ms_ssim_loss(p.double(), g.double(), **kw)
    with pytest.raises(TypeError):
        ms_ssim_loss(p.bfloat16(), g, **kw)
    with pytest.raises(ValueError):
        ms_ssim_loss(p, g[:, :, :-1], **kw)
    with pytest.raises(ValueError):
        ms_ssim_loss(p[0], g[0], **kw)
    with pytest.raises(ValueError, match="176"):
        ms_ssim_loss(p, g)                                  # 24 x 28 does not hold the default 5 levels of 11 taps
    with pytest.raises(ValueError, match="12"):
        ms_ssim_loss(p[..., :11, :], g[..., :11, :], **kw)
    with pytest.raises(ValueError):
        ms_ssim_loss(p, g, levels=6)
    with pytest.raises(ValueError):
        ms_ssim_loss(p, g, levels=2, weights=(0.5, 0.0), window="uniform", win_size=3)
    with pytest.raises(ValueError):
        ms_ssim_loss(p, g, levels=3, window="uniform", win_size=3, data_range=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms_ssim_loss(p.cpu(), g, **kw)


def test_bit_identical_runs_and_graph_replay():
    from rdst_amd.loss import ms_ssim_loss
    g, p0 = R.images((4, 1, 60, 90), 12)
    g, p0 = g.to(DEV), p0.to(DEV)

    def run(p):
        p.grad = None
        loss, msssim = ms_ssim_loss(p, g, 3, return_msssim=True)
        loss.backward()
        return loss.detach(), msssim, p.grad

    p = p0.clone().requires_grad_(True)
    first = [t.clone() for t in run(p)]
    second = run(p)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(ms_ssim_loss(p.detach(), g, 3), first[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(p)
    torch.cuda.current_stream().wait_stream(side)
    p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, msssim = ms_ssim_loss(p, g, 3, return_msssim=True)
        loss.backward()
    out = (loss.detach(), msssim, p.grad)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, first))
    # the replay reads the captured inputs' CURRENT contents
    with torch.no_grad():
        p.mul_(0.9)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    q = p.detach().clone().requires_grad_(True)
    eager = run(q)
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager)) and not torch.equal(replayed[0], first[0])


def test_trainer_graph_step_with_l1_and_msssim_equals_eager():
    """DPTrainStep(loss_fn=SRLoss with {'L1': 0.16, 'MSSSIM': 0.84}, msssim_levels=3, graph=True): the step captured into a HIP
    graph lands on the same parameters as the eager step, bit for bit, and both components are recorded every step.  The
    relative-position bias tables are frozen, as in test_ssim_loss_gpu.py::test_trainer_graph_step_with_l1_and_ssim_equals_eager
    (their gradient is summed with LDS float atomics); everything else, the loss kernels included, has a fixed order."""
    from rdst_amd.loss import LazyScalars, SRLoss
    from rdst_amd.trainer import DPTrainStep
    from util import build_net
    cfg = O.make_cfg(**{**O.CFG_TINY, "img_size": 16})
    gen = torch.Generator().manual_seed(5)
    data = [(torch.rand(4, 1, 16, 16, generator=gen).to(DEV), torch.rand(4, 1, 64, 64, generator=gen).to(DEV)) for _ in range(5)]
    res = {}
    for use_graph in (False, True):
        net = build_net(cfg)
        net.load_state_dict(O.make_weights(cfg, 9), strict=True)
        net.to(DEV).train()
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=["L1", "MSSSIM"], msssim_levels=3,
                                          loss_scalars={"S": {"L1": 0.16, "MSSSIM": 0.84}}, training_states=["S"]))
        tr = DPTrainStep(net, lr=1e-3, loss_fn=sl, graph=use_graph, graph_warmup=2)
        losses = [tr.step(x, t).clone() for x, t in data]
        torch.cuda.synchronize()
        assert (tr.graph is not None) == use_graph
        assert isinstance(tr.last_report, LazyScalars) and isinstance(tr.last_report.raw("Rec_MSSSIM"), torch.Tensor)
        recs = tr.loss_records()
        assert sorted(recs) == ["Rec_L1", "Rec_MSSSIM"] and len(recs["Rec_L1"]) == len(recs["Rec_MSSSIM"]) == 5
        assert all(0.0 < v < 2.0 for v in recs["Rec_MSSSIM"]) and len(set(recs["Rec_MSSSIM"])) == 5
        res[use_graph] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), recs)
    assert res[False][0] == res[True][0] and res[False][2] == res[True][2]
    assert torch.equal(res[False][1], res[True][1])


def test_metrics_on_the_device_and_quick_eva():
    g, p = R.images((3, 2, 190, 206), 21)
    host = M.SRMetrics("psnr ssim msssim")(g, p, 4)
    dev = M.SRMetrics("psnr ssim msssim", device="cuda")(g.to(DEV), p.to(DEV), 4)
    assert list(dev) == ["psnr", "ssim", "msssim"]
    for k, tol in (("psnr", 1e-9), ("ssim", 1e-10), ("msssim", 1e-10)):
        assert np.abs(np.asarray(dev[k]) - np.asarray(host[k])).max() <= tol, k
    only = M.SRMetrics("msssim", "mean", device="cuda")(list(g.to(DEV)), list(p), 4)
    assert list(only) == ["msssim"] and abs(only["msssim"] - float(np.mean(host["msssim"]))) <= 1e-10
    ms = M.device_msssim(g.to(DEV), p.to(DEV), 4)
    assert ms.dtype == torch.float64 and ms.shape == (3,) and np.abs(ms.cpu().numpy() - np.asarray(host["msssim"])).max() <= 1e-10
    assert torch.equal(M.device_msssim(g[0].to(DEV), p[0].to(DEV), 4), ms[:1])
    # device_scores keeps its results beside it
    mse, ss = M.device_scores(g.to(DEV), p.to(DEV), 4)
    assert np.abs(ss.cpu().numpy() - np.asarray(host["ssim"])).max() <= 1e-10

    from rdst_amd.trainer import DPTrainStep
    from util import build_net
    cfg = O.make_cfg(**{**O.CFG_TINY, "img_size": 16})
    net = build_net(cfg)
    net.load_state_dict(O.make_weights(cfg, 7), strict=True)
    net.to(DEV).train()
    tr = DPTrainStep(net, lr=1e-3)
    gen = torch.Generator().manual_seed(2)
    lr, hr = torch.rand(3, 1, 48, 48, generator=gen), torch.rand(3, 1, 192, 192, generator=gen)
    rep = tr.quick_eva(lr, hr, metrics="psnr msssim", num_samples=2, batch_size=1, generator=torch.Generator().manual_seed(11))
    assert list(rep) == ["psnr_4.0", "msssim_4.0"] and all(isinstance(v, float) and np.isfinite(v) for v in rep.values())
    idx = torch.randperm(3, generator=torch.Generator().manual_seed(11))[:2]
    net.eval()
    with torch.no_grad():
        rec = torch.cat([net(x.to(DEV)) for x in lr[idx].split(4)])
    net.train()
    want = M.SRMetrics("psnr msssim", "mean")(hr[idx], rec, 4)
    assert abs(rep["msssim_4.0"] - want["msssim"]) <= 1e-10 and abs(rep["psnr_4.0"] - want["psnr"]) <= 1e-9
