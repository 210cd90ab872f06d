"""GPU: the x8 geometric self-ensemble of the tiled path.  rdst_amd.tiling.unfold_tiles_d8 against nn.Unfold on the CPU composed
with tiling.dihedral, merge_tiles_d8 against its stated fp32 sum spelled with torch ops on the CPU (and a float64 mean), and
SRTester(self_ensemble=True) against the same loop spelled out, its graph path against its eager path; a network that is
equivariant must give the plain result back exactly, and a training run must not notice the ensemble."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from rdst_amd import ops
from rdst_amd import tiling as T
from test_tiling_gpu import _fold_restated, _net, _rand, _slices, _unfold_oracle, _weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -24          # the unit roundoff of fp32


# ---- oracles ---------------------------------------------------------------------------------------------------------------
def _d8(tiles):
    """(n, C, p, p) -> (8 n, C, p, p): slot 8 t + k holds dihedral(tile t, k)."""
    return torch.stack([T.dihedral(tiles, k) for k in range(8)], dim=1).reshape(-1, *tiles.shape[1:]).contiguous()


def _merge_restated(y):
    """The merge as rdst_merge_tiles_d8 states it, in fp32 torch ops on the host: the inverse transforms added in ascending k,
    left to right, then one (exact) multiply by 0.125."""
    y = y.float().cpu()
    acc = T.dihedral_inverse(y[0::8], 0).clone()
    for k in range(1, 8):
        acc += T.dihedral_inverse(y[k::8], k)
    return acc * 0.125


# ---- 1. unfold -------------------------------------------------------------------------------------------------------------
# (N, C, H, W, patch, stride): overlap and padding on both axes; three channels; a patch that is no multiple of four pixels (the
# scalar stores); one tile without padding; a patch above one 32-block and no multiple of it (a partial LDS block)
UNFOLD_CASES = [(2, 1, 20, 27, 16, 8), (2, 3, 17, 63, 8, 6), (2, 1, 9, 31, 6, 3), (1, 3, 16, 16, 16, 16), (1, 1, 50, 45, 40, 24)]


def test_the_plan_of_the_partial_block_case():
    assert T.TilePlan(50, 45, 40, 24).lr == T.Grid(50, 45, 40, 24, 7, 10, 2, 2)


@pytest.mark.parametrize("pad_mode", ["zero", "edge"])
@pytest.mark.parametrize("N,C,H,W,p,s", UNFOLD_CASES)
def test_unfold_d8_is_nn_unfold_and_dihedral(N, C, H, W, p, s, pad_mode):
    plan = T.TilePlan(H, W, p, s, pad_mode=pad_mode)
    x = _rand(N, C, H, W, seed=H + W)
    want = _d8(_unfold_oracle(x, plan))
    total = N * plan.tiles_per_slice
    xd = x.to(DEV)
    got = T.unfold_tiles_d8(xd, plan)
    assert tuple(got.shape) == (8 * total, C, p, p) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    # a window of slots that runs past the last tile: exact zeros there, whatever the caller's tensor held
    first = max(total - 2, 0)
    out = torch.full((32, C, p, p), float("nan"), device=DEV)
    assert T.unfold_tiles_d8(xd, plan, out=out, first_tile=first) is out
    live = 8 * (total - first)
    assert torch.equal(out[:live].cpu(), want[8 * first:]) and not out[live:].any() and not out.isnan().any()
    # rows of a larger buffer that start at an odd element: the scalar stores, also where p % 4 == 0
    flat = torch.empty(8 * total * C * p * p + 1, device=DEV)
    odd = T.unfold_tiles_d8(xd, plan, out=flat[1:].view(8 * total, C, p, p))
    assert torch.equal(odd.cpu(), want)


def test_unfold_d8_windows_and_refusals():
    plan = T.TilePlan(20, 27, 16, 8)
    x = _rand(2, 1, 20, 27, seed=3)
    want = _d8(_unfold_oracle(x, plan))
    assert want.shape[0] == 96
    xd = x.to(DEV)
    out = torch.full((16, 1, 16, 16), float("nan"), device=DEV)
    T.unfold_tiles_d8(xd, plan, out=out, first_tile=3, n_slots=16)
    assert torch.equal(out.cpu(), want[24:40])
    assert torch.equal(T.unfold_tiles_d8(xd, plan, first_tile=10).cpu(), want[80:])
    with pytest.raises(ValueError, match="multiple of 8"):
        T.unfold_tiles_d8(xd, plan, n_slots=12)
    with pytest.raises(ValueError, match="multiple of 8"):
        T.unfold_tiles_d8(xd, plan, out=torch.empty(12, 1, 16, 16, device=DEV))
    with pytest.raises(ValueError):
        T.unfold_tiles_d8(xd, plan, out=torch.empty(16, 1, 16, 8, device=DEV))
    with pytest.raises(ValueError):
        T.unfold_tiles_d8(xd[:, :, :19], plan)
    with pytest.raises(ValueError):
        T.unfold_tiles_d8(xd, plan, first_tile=-1)
    with pytest.raises(TypeError):
        T.unfold_tiles_d8(xd.double(), plan)


# ---- 2. merge --------------------------------------------------------------------------------------------------------------
# (n_tiles, C, P): P no multiple of the 32-block; two whole blocks; a partial block; three blocks
MERGE_CASES = [(5, 3, 12), (3, 1, 64), (2, 2, 40), (1, 1, 96)]


@pytest.mark.parametrize("n,C,P", MERGE_CASES)
def test_merge_d8_is_the_stated_sum(n, C, P):
    y = _rand(8 * n, C, P, P, seed=n + P)
    want = _merge_restated(y)
    yd = y.to(DEV)
    got = T.merge_tiles_d8(yd)
    assert tuple(got.shape) == (n, C, P, P) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    if (n, C, P) == (3, 1, 64):
        assert torch.equal(T.merge_tiles_d8(yd), got)                   # no atomics: the same bits on every run
    # against the float64 mean: seven rounded adds left to right, the scale by 0.125 exact
    inv = torch.stack([T.dihedral_inverse(y[k::8], k).double() for k in range(8)])
    exact, sum_abs = inv.mean(0), inv.abs().sum(0)
    bound = 7 * EPS * sum_abs / 8
    err = (got.cpu().double() - exact).abs()
    print(f"merge n={n} C={C} P={P}: max err = {(err / (EPS * sum_abs / 8)).max().item():.2f} x 2^-24 mean|v| (bound 56)")
    assert (err <= bound).all()
    # an unaligned source and destination take the scalar path
    flat_in, flat_out = torch.empty(y.numel() + 1, device=DEV), torch.empty(want.numel() + 1, device=DEV)
    flat_in[1:].copy_(yd.reshape(-1))
    odd = T.merge_tiles_d8(flat_in[1:].view(8 * n, C, P, P), out=flat_out[1:].view(n, C, P, P))
    assert torch.equal(odd.cpu(), want)


def test_merge_d8_into_rows_of_a_larger_buffer_and_refusals():
    y = _rand(24, 1, 64, 64, seed=11)
    buf = torch.full((7, 1, 64, 64), 7.0, device=DEV)
    back = T.merge_tiles_d8(y.to(DEV), out=buf[2:5])
    assert back.data_ptr() == buf[2:5].data_ptr()
    assert torch.equal(buf[2:5].cpu(), _merge_restated(y))
    assert (buf[:2] == 7.0).all() and (buf[5:] == 7.0).all()
    yd = y.to(DEV)
    with pytest.raises(ValueError):
        T.merge_tiles_d8(yd[:12])
    with pytest.raises(ValueError):
        T.merge_tiles_d8(yd[:, :, :, :32])
    with pytest.raises(ValueError):
        T.merge_tiles_d8(yd, out=buf[2:6])
    with pytest.raises(TypeError):
        T.merge_tiles_d8(yd.bfloat16())
    with pytest.raises(TypeError):
        T.merge_tiles_d8(yd, out=buf[2:5].double())


# ---- 3. the inverse really is the inverse ----------------------------------------------------------------------------------
class _NearestX2(nn.Module):
    """Equivariant under every flip and transpose: the ensemble of its outputs is its output."""

    def __init__(self):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x.repeat_interleave(2, -1).repeat_interleave(2, -2)


def test_an_equivariant_network_gives_the_plain_result_back():
    """Slices of 16-bit values: all partial sums of eight equal values are exact, and so are the fold's sums of up to four, so
    a wrong inverse (k = 5, 6) or a wrong slot order shows as a difference, never as rounding."""
    from rdst_amd.tester import SRTester
    net = _NearestX2().to(DEV)
    lr = torch.randint(0, 65536, (2, 1, 20, 27), generator=torch.Generator().manual_seed(6)).float() / 65536
    kw = dict(sr_scale=2, tile=16, tile_stride=8, tile_batch=16)
    x8, plain = SRTester(net, self_ensemble=True, **kw), SRTester(net, self_ensemble=False, **kw)
    a, b = x8.inference(lr), plain.inference(lr)
    assert tuple(a.shape) == (2, 1, 40, 54)
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), lr.repeat_interleave(2, -1).repeat_interleave(2, -2))


# ---- 4. the tester is the spelled-out loop ---------------------------------------------------------------------------------
def _spelled_out_x8(net, lr, tile, stride, tile_batch, pad_mode="zero"):
    """What the ensembled tester must compute: nn.Unfold tiles, their eight transforms in slot order 8 t + k, the network in
    eval mode on tile_batch slots at a time, the merge restatement, the fp32 fold restatement."""
    plan = T.TilePlan(lr.shape[-2], lr.shape[-1], tile, stride, scale=4, pad_mode=pad_mode)
    slots = _d8(_unfold_oracle(lr, plan)).to(DEV)
    was = net.training
    net.eval()
    with torch.no_grad(), ops.keep_pack_plan(net):      # (the caller may be in the middle of a training run)
        sr = torch.cat([net(b) for b in slots.split(tile_batch)]).float().cpu()
    net.train(was)
    return torch.from_numpy(_fold_restated(_merge_restated(sr).numpy(), plan.hr, lr.shape[0])[0])


SLICES = [(3, 20, 27), (2, 33, 16)]
KW = dict(tile=16, tile_stride=8, tile_batch=40)       # five tiles per call, and a short last call


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_ensembled_inference_is_the_spelled_out_loop(mode):
    from rdst_amd.tester import SRTester
    net = _net(mode)
    code = net.compute_code
    tester = SRTester(net, self_ensemble=True, **KW)
    for i, (n, h, w) in enumerate(SLICES):
        lr = _slices(n, h, w, seed=i)
        rec = tester.inference(lr)
        assert tuple(rec.shape) == (n, 1, 4 * h, 4 * w) and rec.dtype == torch.float32 and rec.is_cuda
        assert torch.equal(rec.cpu(), _spelled_out_x8(net, lr, 16, 8, 40))
        # chunks of whole slices (a budget of one slice's tiles) and slices that are already on the device change nothing
        small = SRTester(net, self_ensemble=True, tile_buffer_bytes=1, **KW)
        assert torch.equal(small.inference(lr.to(DEV)), rec)
        if mode == "fp32":      # the network is not equivariant: the ensemble did something
            assert not torch.equal(rec, SRTester(net, **KW).inference(lr))
    assert net.compute_code == code and tester.graph_captures == 0 and tester.graph_replays == 0
    edge = SRTester(net, self_ensemble=True, pad_mode="edge", **KW)
    lr = _slices(2, 20, 27, seed=5)
    assert torch.equal(edge.inference(lr).cpu(), _spelled_out_x8(net, lr, 16, 8, 40, "edge"))


# ---- 5. graph --------------------------------------------------------------------------------------------------------------
def test_ensembled_graph_replays_equal_the_eager_tiles():
    from rdst_amd.tester import SRTester
    net = _net("fp32")
    eager = SRTester(net, self_ensemble=True, **KW)
    graph = SRTester(net, self_ensemble=True, graph=True, **KW)
    for i, (n, h, w) in enumerate(SLICES + SLICES):
        lr = _slices(n, h, w, seed=10 + i)
        assert torch.equal(graph.inference(lr), eager.inference(lr)), (i, h, w)
    assert graph.graph_captures == 1 and graph.graph is not None and graph.graph_replays > 0
    assert tuple(graph._static_in.shape) == (40, 1, 16, 16)              # the plain path's static batch
    replays = graph.graph_replays
    # other weights, loaded in place: the captured forward reads the live parameters, nothing is captured again
    net.load_state_dict(_weights(8), strict=True)
    lr = _slices(3, 20, 27, seed=20)
    got = graph.inference(lr)
    assert graph.graph_captures == 1 and graph.graph_replays == replays + math.ceil(18 * 8 / 40) == replays + 4
    assert torch.equal(got.cpu(), _spelled_out_x8(net, lr, 16, 8, 40))
    # another compute mode is another forward: the graph is dropped and captured again
    net.set_compute_dtype("bf16")
    assert torch.equal(graph.inference(lr).cpu(), _spelled_out_x8(net, lr, 16, 8, 40))
    assert graph.graph_captures == 2


# ---- 6. scoring ------------------------------------------------------------------------------------------------------------
def test_evaluate_on_device_with_the_ensemble():
    from rdst_amd.tester import SRTester
    net = _net("bf16")
    tester = SRTester(net, self_ensemble=True, tile=16, tile_stride=8, tile_batch=16)
    lr, gt = _slices(3, 20, 27), torch.rand(3, 1, 80, 108, generator=torch.Generator().manual_seed(9))
    dev, host = tester.evaluate(lr, gt, on_device=True), tester.evaluate(lr, gt)
    assert set(dev) == set(host) == {"psnr", "ssim"} and len(dev["psnr"]) == len(dev["ssim"]) == 3
    assert np.allclose(dev["psnr"], host["psnr"], rtol=0, atol=1e-9) and np.allclose(dev["ssim"], host["ssim"], rtol=0, atol=1e-10)
    # they are the scores of the ensembled reconstruction, not of the plain one
    plain = SRTester(net, tile=16, tile_stride=8, tile_batch=16).evaluate(lr, gt)
    assert plain["psnr"] != host["psnr"]


# ---- 7. between training steps ---------------------------------------------------------------------------------------------
def test_training_run_unchanged_by_ensembled_inference():
    """Six captured training steps with a graph-replayed ensembled inference after steps 2 and 4 give the losses and parameters
    of six steps without it, bit for bit (tests/test_tiling_gpu.py: test_training_run_unchanged_by_tiled_inference, with the
    ensemble; the relative-position bias tables are frozen as there)."""
    from rdst_amd.tester import SRTester
    from rdst_amd.trainer import DPTrainStep
    g = torch.Generator().manual_seed(5)
    data = [(torch.rand(2, 1, 16, 16, generator=g).to(DEV), torch.rand(2, 1, 64, 64, generator=g).to(DEV)) for _ in range(6)]
    lr = _slices(3, 20, 27, seed=4)
    res = {}
    for with_inference in (False, True):
        net = _net("bf16")
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        tr = DPTrainStep(net, lr=1e-3, graph=True, graph_warmup=2)
        tester = SRTester(net, tile=16, tile_stride=8, tile_batch=16, graph=True, self_ensemble=True)
        losses = []
        for i, (x, t) in enumerate(data):
            losses.append(tr.step(x, t).clone())
            if with_inference and i in (1, 3):
                plan = ops.pack_plan_of(net)
                rec = tester.inference(lr)
                assert ops.pack_plan_of(net) is plan
                assert torch.equal(rec.cpu(), _spelled_out_x8(net, lr, 16, 8, 16))
                assert ops.pack_plan_of(net) is plan
        torch.cuda.synchronize()
        assert tr.graph is not None
        if with_inference:
            assert tester.graph_captures == 1 and tester.graph_replays >= 5
        res[with_inference] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), tr.loss_records()["L1"])
    assert res[False][0] == res[True][0]
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2] == res[True][2] == res[False][0]
