"""GPU: the SSIM training loss (rdst_ssim_loss, rdst_amd.loss.ssim_loss / SSIMLoss / SRLoss 'SSIM') against the float64
reference of tests/ssim_reference.py (valid per-channel conv2d with the taps and torch autograd in float64, on seeded
images).  The gates, all derived:
  |ssim[n] - ref| <= 1e-10                              the scoring kernel's own tolerance (test_srmetrics_gpu.py)
  |loss - ref|    <= 2^-23
  C ABI:     |grad - g64| <= 2^-23 |g64| + 1e-10 max|g64|    one fp32 rounding (2^-24) doubled + a floor for fp64 cancellation
  autograd:  |grad - g64| <= 2^-22 |g64| + 1e-10 max|g64|    one more fp32 multiply by the upstream gradient"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_reference as R
from oracle import rdst_oracle as O
from rdst_amd import _lib
from rdst_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_SSIM, TOL_LOSS = 1e-10, 2.0 ** -23

CASES = [
    # (N, C, H, W, window, win, data_range[, kind])
    (1, 1, 7, 7, "u", 7, 1.0),
    (1, 1, 3, 5, "u", 3, 1.0),
    (1, 1, 11, 11, "g", 11, 1.0),           # a single window position
    (2, 3, 23, 37, "u", 7, 1.0),
    (2, 3, 37, 53, "g", 11, 1.0),
    (1, 1, 53, 37, "u", 15, 255.0),
    (2, 1, 33, 65, "u", 7, 1.0),            # one pixel past a 32- or 64-wide tile (and past two 16-row tiles)
    (2, 1, 70, 150, "g", 11, 255.0),        # five row tiles and five column tiles of 16 x 32
    (2, 1, 40, 70, "u", 7, 1.0, "slice"),   # a zero background in the target
    (2, 1, 40, 70, "g", 11, 1.0, "slice"),
    (2, 1, 40, 70, "u", 7, 1.0, "range"),   # a prediction in [-0.1, 1.1]
    (2, 1, 40, 70, "g", 11, 1.0, "range"),
]
WINDOW = {"u": "uniform", "g": "gaussian"}


def _id(c):
    return "N{}C{}_{}x{}_{}{}_dr{:g}".format(*c[:7]) + ("_" + c[7] if len(c) > 7 else "")


def _raw(target, pred, taps, cn, dr, want_grad=True):
    """rdst_ssim_loss through the C ABI: (ssim fp64 (N,), loss fp32 (), grad fp32 or None), device tensors."""
    N, C, H, W = pred.shape
    win = len(taps)
    lib = _lib.load()
    nb = lib.rdst_ssim_loss_workspace(N, C, H, W, win)
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)                 # NaNs where nothing was written
    ssim = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    grad = torch.full(pred.shape, float("nan"), dtype=torch.float32, device=DEV) if want_grad else None
    tp = np.ascontiguousarray(taps, dtype=np.float64)
    _lib.check(lib.rdst_ssim_loss(target.data_ptr(), pred.data_ptr(), N, C, H, W, win, tp.ctypes.data, cn, dr, ssim.data_ptr(),
                                  loss.data_ptr(), grad.data_ptr() if want_grad else None, ws.data_ptr(), nb,
                                  torch.cuda.current_stream().cuda_stream), "rdst_ssim_loss")
    torch.cuda.synchronize()
    return ssim, loss, grad


def _gate(got, g64, rel, scale=1.0, extra=None):
    """Elementwise |got - scale g64| <= rel |scale g64| + 1e-10 max|scale g64| (+ extra), in float64."""
    want = scale * g64
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all()
    tol = rel * want.abs() + 1e-10 * want.abs().max()
    if extra is not None:
        tol = tol + extra
    err = (got - want).abs()
    worst = (err - tol).max()
    print(f"gradient: max|err| {err.max():.3e}, max|g64| {want.abs().max():.3e}, worst err - tol {worst:.3e}")
    assert worst <= 0, (float(err.max()), float(worst))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_c_abi(case):
    N, C, H, W, window, win, dr = case[:7]
    ref = R.case(*case)
    g, p = ref["target"].to(DEV), ref["pred"].to(DEV)
    ssim, loss, grad = _raw(g, p, ref["taps"], ref["cn"], dr)
    print(f"ssim: max|err| {float((ssim.cpu() - ref['ssim']).abs().max()):.3e}; loss err {abs(float(loss) - float(ref['loss'])):.3e}")
    assert torch.isfinite(ssim).all() and torch.isfinite(loss)
    assert float((ssim.cpu() - ref["ssim"]).abs().max()) <= TOL_SSIM
    assert abs(float(loss) - float(ref["loss"])) <= TOL_LOSS
    _gate(grad, ref["grad"], 2.0 ** -23)
    if window == "u":       # the scoring kernel computes the same number
        assert float((M.device_scores(g, p, 0, dr, win)[1] - ssim).abs().max()) <= TOL_SSIM
    # value only: the same bits
    ssim0, loss0, _ = _raw(g, p, ref["taps"], ref["cn"], dr, want_grad=False)
    assert torch.equal(loss0, loss) and torch.equal(ssim0, ssim)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_autograd(case):
    from rdst_amd.loss import ssim_loss
    N, C, H, W, window, win, dr = case[:7]
    ref = R.case(*case)
    g = ref["target"].to(DEV)
    p = ref["pred"].to(DEV).requires_grad_(True)
    loss, ssim = ssim_loss(p, g, WINDOW[window], win, data_range=dr, return_ssim=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert ssim.shape == (N,) and ssim.dtype == torch.float64 and not ssim.requires_grad
    (loss * 0.37).backward()
    assert float((ssim.cpu() - ref["ssim"]).abs().max()) <= TOL_SSIM
    assert abs(float(loss.detach()) - float(ref["loss"])) <= TOL_LOSS
    _gate(p.grad, ref["grad"], 2.0 ** -22, scale=float(np.float32(0.37)))
    # defaults: window sizes 7 / 11 need not be named
    if win == {"u": 7, "g": 11}[window]:
        assert torch.equal(ssim_loss(p.detach(), g, WINDOW[window], data_range=dr), loss.detach())


def test_non_contiguous_inputs_and_refusals():
    from rdst_amd.loss import ssim_loss
    ref = R.case(2, 3, 23, 37, "u", 7, 1.0)
    g = ref["target"].to(DEV)
    p = ref["pred"].to(DEV)
    pt = p.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)       # same values, column-major planes
    gt = g.transpose(2, 3).contiguous().transpose(2, 3)
    assert not pt.is_contiguous()
    loss = ssim_loss(pt, gt)
    loss.backward()
    assert abs(float(loss) - float(ref["loss"])) <= TOL_LOSS
    _gate(pt.grad, ref["grad"], 2.0 ** -22)
    with pytest.raises(ValueError):
        ssim_loss(p, g.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        ssim_loss(p.double(), g.double())
    with pytest.raises(TypeError):
        ssim_loss(p.bfloat16(), g)
    with pytest.raises(ValueError):
        ssim_loss(p, g[:, :, :-1])
    with pytest.raises(ValueError):
        ssim_loss(p[0], g[0])
    with pytest.raises(ValueError):
        ssim_loss(p[..., :5, :], g[..., :5, :])
    with pytest.raises(RuntimeError):
        ssim_loss(p.cpu(), g)


@pytest.mark.parametrize("window,win,dr", [("u", 7, 1.0), ("g", 11, 1.0), ("u", 15, 255.0)], ids=str)
def test_identical_images(window, win, dr):
    """pred == target: S = 1 at every position and the gradient is analytically zero."""
    N, C, H, W = 2, 3, 37, 53
    g, _ = R.images((N, C, H, W), 3, dr)
    g = g.to(DEV)
    taps, cn = R.taps_of(window, win)
    ssim, loss, grad = _raw(g, g.clone(), taps, cn, dr)
    print(f"loss {float(loss):.3e}, max|grad| {float(grad.abs().max()):.3e}, 1 - ssim {(1 - ssim).abs().max().item():.3e}")
    assert float(loss) <= 1e-12 and float((1 - ssim).abs().max()) <= 1e-12
    assert torch.isfinite(grad).all()
    assert float(grad.abs().max()) <= 1e-9 / (N * C * (H - win + 1) * (W - win + 1))


def test_bit_identical_runs_and_graph_replay():
    from rdst_amd.loss import ssim_loss
    g, p0 = R.images((4, 1, 60, 90), 12)
    g, p0 = g.to(DEV), p0.to(DEV)

    def run(p):
        p.grad = None
        loss, ssim = ssim_loss(p, g, "gaussian", return_ssim=True)
        loss.backward()
        return loss.detach(), ssim, p.grad

    p = p0.clone().requires_grad_(True)
    first = [t.clone() for t in run(p)]
    second = run(p)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    # the value alone: the same bits
    assert torch.equal(ssim_loss(p.detach(), g, "gaussian"), first[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(p)
    torch.cuda.current_stream().wait_stream(side)
    p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, ssim = ssim_loss(p, g, "gaussian", return_ssim=True)
        loss.backward()
    out = (loss.detach(), ssim, p.grad)
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


def test_l1_ssim_mix_gradient():
    """0.16 L1 + 0.84 (1 - SSIM), the mix of the training step: pred.grad against float64 autograd of the whole mix, under
    the autograd gate for the SSIM term plus the same gate for the L1 term."""
    from rdst_amd.loss import ssim_loss
    ref = R.case(2, 3, 37, 53, "g", 11, 1.0)
    g = ref["target"].to(DEV)
    p = ref["pred"].to(DEV).requires_grad_(True)
    (0.16 * F.l1_loss(p, g) + 0.84 * ssim_loss(p, g, "gaussian")).backward()
    X, Y = ref["target"].double(), ref["pred"].double().requires_grad_(True)
    S = R.terms(X, Y, ref["taps"], ref["cn"], 1.0)[-1]
    l1 = (Y - X).abs().mean()
    (0.16 * l1 + 0.84 * (1.0 - S.mean(dim=(1, 2, 3)).mean())).backward()
    g_l1 = 0.16 * torch.sign(Y.detach() - X) / X.numel()
    g_ss = 0.84 * ref["grad"]
    assert float((Y.grad - (g_l1 + g_ss)).abs().max()) <= 1e-15
    tol = (2.0 ** -22 * g_ss.abs() + 1e-10 * g_ss.abs().max()) + (2.0 ** -22 * g_l1.abs() + 1e-10 * g_l1.abs().max())
    err = (p.grad.double().cpu() - Y.grad).abs()
    print(f"mix: max|err| {err.max():.3e}, worst err - tol {(err - tol).max():.3e}")
    assert torch.isfinite(p.grad).all() and float((err - tol).max()) <= 0


def test_trainer_graph_step_with_l1_and_ssim_equals_eager():
    """DPTrainStep(loss_fn=SRLoss with {'L1': 0.16, 'SSIM': 0.84}, graph=True): the step captured into a HIP graph lands on
    the same parameters as the eager step, bit for bit, and both components are recorded every step.
    The relative-position bias tables are frozen, as test_step_guard_gpu.py::_tiny_rdst_fixed_tables freezes them: the
    attention backward sums their gradient with LDS float atomics, so in fp32 two EAGER runs of this trainer with L1 alone
    already differ (measured here, these five steps: parameters 3e-8 apart after step 1, 7e-6 after step 5); everything
    else, the loss kernel included, has a fixed order."""
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
        sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=["L1", "SSIM"],
                                          loss_scalars={"S": {"L1": 0.16, "SSIM": 0.84}}, training_states=["S"]))
        tr = DPTrainStep(net, lr=1e-3, loss_fn=sl, graph=use_graph, graph_warmup=2)
        losses = [tr.step(x, t).clone() for x, t in data]
        torch.cuda.synchronize()
        assert (tr.graph is not None) == use_graph
        assert isinstance(tr.last_report, LazyScalars) and isinstance(tr.last_report.raw("Rec_SSIM"), torch.Tensor)
        recs = tr.loss_records()
        assert sorted(recs) == ["Rec_L1", "Rec_SSIM"] and len(recs["Rec_L1"]) == len(recs["Rec_SSIM"]) == 5
        assert all(0.0 < v < 2.0 for v in recs["Rec_SSIM"]) and len(set(recs["Rec_SSIM"])) == 5
        res[use_graph] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), recs)
    assert res[False][0] == res[True][0] and res[False][2] == res[True][2]
    assert torch.equal(res[False][1], res[True][1])
