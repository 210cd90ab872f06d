"""GPU: the LR-consistency kernels (rdst_lrc_residual, rdst_lrc_adjoint: csrc/consistency.hip) against the composed path they
must reproduce bit for bit (data.resample / data.resample_adjoint and torch elementwise operations), the loss against float64
autograd of the dense-matrix formula, and the loss and the back-projection where they are used: SRLoss 'LRC' under
DPTrainStep's HIP graph, DevicePatchSampler batches, SRTester(back_project=...).

Shapes: rectangular x4; a non-integer ratio (transposed rows of unequal length); 64 -> 8 (transposed rows without taps); 72 x
104 -> 18 x 26, which has four ragged column bands (8 LR columns) and three row chunks (32) in the residual kernel and three
ragged row bands (32) and four column bands (32) in the adjoint kernel under a sparse table; 520 x 20 -> 130 x 5 for the
adjoint kernel's dense cut ('fourier': row bands of 256, 256, 8 and column bands of 8, 8, 4); and the training shape once."""
import types

import numpy as np
import pytest
import torch

from oracle import rdst_oracle as O
from rdst_amd import _lib
from rdst_amd import data as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ALL = D.KINDS
SHAPES = [((2, 3, 24, 40), (6, 10), ALL),
          ((1, 1, 21, 40), (8, 16), ALL),
          ((1, 2, 64, 64), (8, 8), ("cubic", "cubic+gaussian")),
          ((1, 1, 72, 104), (18, 26), ALL),
          ((1, 1, 520, 20), (130, 5), ("fourier",)),
          ((2, 1, 256, 256), (64, 64), ("cubic", "fourier"))]
CASES = [pytest.param(hr, lr, k, id=f"{k}-{'x'.join(map(str, hr))}") for hr, lr, kinds in SHAPES for k in kinds]
SMALL = [c for c in CASES if c.values[0][-2] * c.values[0][-1] <= 64 * 64]


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


def _pair(hr, lr, seed=1):
    return _rand(hr, seed), _rand(hr[:2] + lr, seed + 100)


def _dense32(kind, n_in, n_out):
    """The operator as the device holds it: float64 matrix of the fp32-rounded weights."""
    index, weight = D.operator_table(kind, n_in, n_out)
    M = np.zeros((n_out, n_in))
    np.add.at(M, (np.arange(n_out)[:, None], index), weight.astype(np.float32).astype(np.float64))
    return torch.from_numpy(M)


# ---- rdst_lrc_residual -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hr, lr, kind", CASES)
def test_residual(hr, lr, kind):
    from rdst_amd.loss.consistency import lrc_residual, unit_scales
    pred, low = _pair(hr, lr)
    R = D.resample(pred, lr, kind) - low
    n = R.numel()
    inv_n, scale = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in unit_scales(n))
    assert float(inv_n) == float(np.float32(1.0 / n)) and float(scale) == float(np.float32(2.0 / n))
    resid, g, loss = lrc_residual(pred, low, kind)
    assert g is None and loss is None and torch.equal(resid, R)
    for norm, g_ref, mean in (("l1", torch.sign(R) * inv_n, R.double().abs().mean()), ("l2", R * scale, (R.double() ** 2).mean())):
        resid, g, loss = lrc_residual(pred, low, kind, norm, want_g=True, want_loss=True)
        assert torch.equal(resid, R) and torch.equal(g, g_ref)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        ref = np.float32(float(mean))
        print(f"{kind} {hr} {norm}: loss {float(loss):.9g} float64 mean {float(mean):.17g}")
        assert abs(np.float32(float(loss)) - ref) <= np.spacing(ref)
        _, g2, loss2 = lrc_residual(pred, low, kind, norm, want_resid=False, want_g=True, want_loss=True)
        assert torch.equal(loss2, loss) and torch.equal(g2, g)


@pytest.mark.parametrize("hr, lr, kind", SMALL)
def test_residual_of_the_degraded_target_is_exactly_zero(hr, lr, kind):
    from rdst_amd.loss.consistency import lrc_residual
    gt = _rand(hr, 4)
    low = D.resample(gt, lr, kind)
    for norm in ("l1", "l2"):
        resid, g, loss = lrc_residual(gt, low, kind, norm, want_g=True, want_loss=True)
        assert float(loss) == 0.0 and not resid.any() and not g.any()      # sign(0) must be 0, not +-inv_n


# ---- rdst_lrc_adjoint --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hr, lr, kind", CASES)
def test_adjoint(hr, lr, kind):
    from rdst_amd.loss.consistency import lrc_adjoint
    size = hr[-2:]
    g = _rand(hr[:2] + lr, 7, -1.0, 1.0)
    a = D.resample_adjoint(g, size, kind)
    assert tuple(a.shape) == hr
    assert torch.equal(lrc_adjoint(g, size, kind), a)
    s_dev = torch.tensor(0.37, dtype=torch.float32, device=DEV)
    assert torch.equal(lrc_adjoint(g, size, kind, scale_dev=s_dev), s_dev * a)
    assert torch.equal(lrc_adjoint(g, size, kind, scale=-0.5, scale_dev=s_dev), (s_dev * -0.5) * a)
    base = _rand(hr, 8)
    assert torch.equal(lrc_adjoint(g, size, kind, scale=-1.0, base=base), base - a)
    half = lrc_adjoint(g, size, kind, scale=-0.5, base=base)
    assert torch.equal(half, base - 0.5 * a)
    inplace = base.clone()
    assert lrc_adjoint(g, size, kind, scale=-0.5, base=inplace, out=inplace) is inplace and torch.equal(inplace, half)
    # <A x, y> = <x, A^T y>, summed in float64 from the device results, to 1e-5 of the inner product itself: fp32 chains of
    # at most 256 taps.  x and y are drawn from [0, 1], so the terms do not cancel and the product has the size of its terms
    x, y = _rand(hr, 9), _rand(hr[:2] + lr, 10)
    lhs = float((D.resample(x, lr, kind).double() * y.double()).sum())
    rhs = float((x.double() * lrc_adjoint(y, size, kind).double()).sum())
    print(f"{kind} {hr}: <Ax,y> {lhs:.12g} <x,A^T y> {rhs:.12g} relative difference {abs(lhs - rhs) / abs(lhs):.3g}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_composed_path_answers_when_an_entry_point_says_notsup(monkeypatch):
    """RDST_ENOTSUP (the C refusal itself is held by tests/test_consistency_host.py) sends both functions through resample /
    resample_adjoint and torch elementwise operations: the same elements, the loss within one ulp."""
    from rdst_amd.loss.consistency import lrc_adjoint, lrc_residual
    hr, lr, kind = (2, 3, 24, 40), (6, 10), "cubic_aa"
    pred, low = _pair(hr, lr)
    g = _rand(hr[:2] + lr, 7, -1.0, 1.0)
    s_dev = torch.tensor(0.37, dtype=torch.float32, device=DEV)
    base = _rand(hr, 8)
    fused = {n: lrc_residual(pred, low, kind, n, want_g=True, want_loss=True) for n in ("l1", "l2")}
    fused_a = (lrc_adjoint(g, hr[-2:], kind, scale=-0.5, scale_dev=s_dev), lrc_adjoint(g, hr[-2:], kind, scale=-0.5, base=base))
    lib = _lib.load()

    def notsup(*_a):
        return _lib.ENOTSUP
    monkeypatch.setattr(lib, "rdst_lrc_residual", notsup)
    monkeypatch.setattr(lib, "rdst_lrc_adjoint", notsup)
    for n in ("l1", "l2"):
        resid, gg, loss = lrc_residual(pred, low, kind, n, want_g=True, want_loss=True)
        assert torch.equal(resid, fused[n][0]) and torch.equal(gg, fused[n][1])
        assert abs(np.float32(float(loss)) - np.float32(float(fused[n][2]))) <= np.spacing(np.float32(float(loss)))
    assert torch.equal(lrc_adjoint(g, hr[-2:], kind, scale=-0.5, scale_dev=s_dev), fused_a[0])
    assert torch.equal(lrc_adjoint(g, hr[-2:], kind, scale=-0.5, base=base), fused_a[1])


def test_degrade_is_resample_with_the_adjoint_as_backward():
    x = _rand((2, 1, 21, 40), 3).requires_grad_(True)
    y = D.degrade(x, (8, 16), "cubic+gaussian")
    assert torch.equal(y.detach(), D.resample(x.detach(), (8, 16), "cubic+gaussian"))
    up = _rand((2, 1, 8, 16), 5, -1.0, 1.0)
    y.backward(up)
    assert torch.equal(x.grad, D.resample_adjoint(up, (21, 40), "cubic+gaussian"))
    with pytest.raises(RuntimeError, match="not differentiable"):
        D.resample(x, (8, 16))                                       # resample itself still refuses
    with pytest.raises(RuntimeError, match="not differentiable"):
        D.resample_adjoint(up.requires_grad_(True), (21, 40))


# ---- lr_consistency_loss -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["l1", "l2"])
@pytest.mark.parametrize("hr, lr, kind", CASES)
def test_loss_gradient_is_the_composed_path(hr, lr, kind, norm):
    from rdst_amd.loss import lr_consistency_loss
    from rdst_amd.loss.consistency import _residual_composed
    pred, low = _pair(hr, lr, seed=11)
    p = pred.clone().requires_grad_(True)
    loss = lr_consistency_loss(p, low, kind, norm)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (0.37 * loss).backward()
    _, g, ref_loss = _residual_composed(pred, low, D.Degradation.of(kind), {"l1": 1, "l2": 2}[norm])
    w = torch.tensor(1.0, dtype=torch.float32, device=DEV) * 0.37
    assert torch.equal(p.grad, w * D.resample_adjoint(g, hr[-2:], kind))
    assert abs(np.float32(float(loss.detach())) - np.float32(float(ref_loss))) <= np.spacing(np.float32(float(ref_loss)))
    with torch.no_grad():                                            # without a gradient asked for: the value alone
        assert torch.equal(lr_consistency_loss(pred, low, kind, norm), loss.detach())


@pytest.mark.parametrize("norm", ["l1", "l2"])
@pytest.mark.parametrize("hr, lr, kind", SMALL)
def test_loss_against_float64_autograd(hr, lr, kind, norm):
    from rdst_amd.loss import lr_consistency_loss
    pred, low = _pair(hr, lr, seed=13)
    p = pred.clone().requires_grad_(True)
    loss = lr_consistency_loss(p, low, kind, norm)
    loss.backward()
    Ay, Ax = _dense32(kind, hr[-2], lr[0]), _dense32(kind, hr[-1], lr[1])
    q = pred.double().cpu().requires_grad_(True)
    R = Ay @ q @ Ax.T - low.double().cpu()
    assert float(R.detach().abs().min()) > 1e-6                               # no residual near the kink of |.|
    ref = R.abs().mean() if norm == "l1" else (R * R).mean()
    ref.backward()
    err = float((p.grad.double().cpu() - q.grad).norm() / q.grad.norm())
    got, want = float(loss.detach()), float(ref.detach())
    print(f"{kind} {hr} {norm}: loss {got:.9g} / {want:.12g}, gradient relative L2 error {err:.3g}")
    assert err <= 1e-5 and abs(got - want) <= 1e-5 * want


def test_loss_refusals():
    from rdst_amd.loss import lr_consistency_loss
    pred, low = _pair((1, 1, 16, 16), (4, 4))
    with pytest.raises(TypeError, match="float32"):
        lr_consistency_loss(pred.double(), low)
    with pytest.raises(TypeError, match="float32"):
        lr_consistency_loss(pred, low.half())
    with pytest.raises(ValueError, match="share N and C"):
        lr_consistency_loss(pred, low.expand(2, 1, 4, 4))
    with pytest.raises(ValueError, match="share N and C"):
        lr_consistency_loss(pred[0], low[0])
    with pytest.raises(ValueError, match="'fourier' only shrinks"):
        lr_consistency_loss(low, pred, "fourier")
    with pytest.raises(ValueError, match="detach"):
        lr_consistency_loss(pred, low.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lr_consistency_loss(pred, low.cpu())
    p = pred.clone().requires_grad_(True)
    gr, = torch.autograd.grad(lr_consistency_loss(p, low), p, create_graph=True)
    assert not gr.requires_grad                                      # once differentiable: no second derivative


# ---- the sampler's batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL)
def test_loss_of_a_sampled_batch_against_itself_is_zero(kind):
    from rdst_amd.loss import LRConsistencyLoss
    stack = torch.rand(6, 1, 40, 48, generator=torch.Generator().manual_seed(2))
    sampler = D.DevicePatchSampler(stack, batch_size=4, lr_patch_size=8, sr_scales=(4.0,), device=DEV,
                                   generator=torch.Generator().manual_seed(3), degradation=kind, augment=True)
    batch = sampler.sample()
    f = LRConsistencyLoss(kind, 4)
    loss, rep = f(batch["out"], batch["out"])
    assert torch.equal(f.target(batch["out"]), batch["in"])
    assert float(loss) == 0.0 and rep["Rec_LRC"] == 0.0
    with pytest.raises(ValueError, match="not a multiple of the scale"):
        f(batch["out"][..., :30], batch["out"][..., :30])
    with pytest.raises(ValueError, match="must have one shape"):
        f(batch["out"][..., :16, :16], batch["out"])


# ---- SRLoss 'LRC' under the trainer's graph ----------------------------------------------------------------------------------
def test_trainer_graph_step_with_l1_and_lrc_equals_eager():
    """DPTrainStep(loss_fn=SRLoss with {'L1': 1, 'LRC': 0.1}, graph=True): the capture succeeds (the tables are on the device
    before it), three graph steps give the eager steps' losses bit for bit, and Rec_LRC is recorded every step.  The
    relative-position bias tables are frozen as in tests/test_ssim_loss_gpu.py (their gradient is summed with LDS atomics)."""
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
        sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=["L1", "LRC"], sr_scale=4,
                                          lrc_degradation="cubic_aa", loss_scalars={"S": {"L1": 1.0, "LRC": 0.1}},
                                          training_states=["S"]))
        tr = DPTrainStep(net, lr=1e-3, loss_fn=sl, graph=use_graph, graph_warmup=2)
        losses = [tr.step(x, t).clone() for x, t in data]
        torch.cuda.synchronize()
        assert (tr.graph is not None) == use_graph
        assert isinstance(tr.last_report, LazyScalars) and isinstance(tr.last_report.raw("Rec_LRC"), torch.Tensor)
        recs = tr.loss_records()
        assert sorted(recs) == ["Rec_L1", "Rec_LRC"] and len(recs["Rec_L1"]) == len(recs["Rec_LRC"]) == 5
        assert all(0.0 < v < 2.0 for v in recs["Rec_LRC"]) and len(set(recs["Rec_LRC"])) == 5
        res[use_graph] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), recs)
    assert res[False][0] == res[True][0] and res[False][2] == res[True][2]
    assert torch.equal(res[False][1], res[True][1])


# ---- SRTester(back_project=...) ----------------------------------------------------------------------------------------------
def _net(seed=7):
    from rdst_amd.networks.rdst_variations import RDSTSR
    cfg = O.make_cfg(**{**O.CFG_TINY, "img_size": 16})
    net = RDSTSR(img_size=16, in_chans=1, sr_scale=4, embed_dim=48, dense_layer_depths=[2, 2], num_heads=[6, 6],
                 window_size=[8, 8], rdb_depths=[3, 3], mlp_ratio=2.0, growth_rate=24, pre_norm=True,
                 feature_last_operation=True)
    net.load_state_dict(O.make_weights(cfg, seed), strict=True)
    return net.to(DEV)


@pytest.fixture(scope="module")
def net():
    return _net()


TESTERS = [pytest.param({}, (2, 1, 16, 24), id="whole"),
           pytest.param(dict(tile=16, tile_stride=8, tile_batch=5), (2, 1, 20, 27), id="tiled")]


@pytest.mark.parametrize("kw, shape", TESTERS)
def test_back_projection_is_the_spelled_out_loop(net, kw, shape):
    from rdst_amd.tester import SRTester
    lr = torch.rand(*shape, generator=torch.Generator().manual_seed(2))
    H, W = 4 * shape[-2], 4 * shape[-1]
    plain = SRTester(net, **kw).inference(lr)
    assert torch.equal(SRTester(net, back_project=0, **kw).inference(lr), plain)      # 0 steps: today's tester
    for kind in ("cubic", "fourier"):
        got = SRTester(net, back_project=3, degradation=kind, bp_step=0.5, **kw).inference(lr)
        P = plain.clone()
        for _ in range(3):
            a = D.resample_adjoint(D.resample(P, shape[-2:], kind) - lr.to(DEV), (H, W), kind)
            P = P - 0.5 * a
        assert got.shape == plain.shape and torch.equal(got, P)
    assert torch.equal(SRTester(net, **kw).inference(lr), plain)                       # and the network is left as it was


class _Fixed(torch.nn.Module):
    """A 'network' whose SR slices are given: the back-projection of a random start."""

    def __init__(self, P):
        super().__init__()
        self.P = torch.nn.Parameter(P, requires_grad=False)
        self.sr_scale = 4

    def forward(self, x):
        return self.P[:x.shape[0]]


def _rms_after(kind, k, P, lr):
    from rdst_amd.tester import SRTester
    out = SRTester(_Fixed(P), back_project=k, degradation=kind).inference(lr)
    return float((D.resample(out, lr.shape[-2:], kind) - lr).double().pow(2).mean().sqrt())


@pytest.mark.parametrize("kind", ["cubic_aa", "fourier"])
def test_default_step_shrinks_the_residual(kind):
    P, lr = _rand((2, 1, 64, 96), 21), _rand((2, 1, 16, 24), 22)
    rms = [_rms_after(kind, k, P, lr) for k in range(4)]
    print(kind, rms)
    assert all(b < a for a, b in zip(rms, rms[1:])), rms


def test_default_step_solves_cubic_x4_at_once():
    P, lr = _rand((2, 1, 64, 96), 21), _rand((2, 1, 16, 24), 22)
    rms = [_rms_after("cubic", k, P, lr) for k in range(2)]
    print("cubic", rms)
    assert rms[1] < rms[0] / 100, rms
