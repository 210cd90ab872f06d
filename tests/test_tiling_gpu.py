"""GPU: rdst_amd.tiling and the tiled path of SRTester.  The oracle of the tiling is torch's own nn.Unfold / nn.Fold on the
CPU with the plan's padding; the fold is also pinned bit for bit to an fp32 numpy restatement of its stated order (ascending
tile row, then tile column, one multiply by the rounded reciprocal of the cover count).  The tiled tester is compared with the
same loop spelled out, its graph path with its eager path, and a training run must not notice it."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import rdst_oracle as O
from rdst_amd import ops
from rdst_amd import tiling as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -24          # the unit roundoff of fp32


# ---- oracles ---------------------------------------------------------------------------------------------------------------
def _unfold_oracle(x, plan):
    """(N, C, H, W) on the host -> (N Ly Lx, C, p, p): nn.Unfold with the plan's padding, tiles slice-major."""
    g = plan.lr
    if plan.pad_mode == "edge":
        x = F.pad(x, (g.pad_x, g.pad_x, g.pad_y, g.pad_y), mode="replicate")
        cols = nn.Unfold(kernel_size=g.patch, stride=g.stride)(x)
    else:
        cols = nn.Unfold(kernel_size=g.patch, stride=g.stride, padding=(g.pad_y, g.pad_x))(x)
    assert cols.shape[-1] == plan.tiles_per_slice
    return cols.transpose(1, 2).reshape(-1, x.shape[1], g.patch, g.patch).contiguous()


def _fold_restated(tiles, g, N):
    """The fold as rdst_fold_tiles states it, in fp32 numpy: every pixel accumulates its covering tile pixels in ascending
    tile row, then ascending tile column, and is multiplied once by the rounded reciprocal of its cover count."""
    tiles = np.asarray(tiles, dtype=np.float32).reshape(N, g.Ly, g.Lx, -1, g.patch, g.patch)
    acc = np.zeros((N, tiles.shape[3], g.H, g.W), dtype=np.float32)
    cnt = np.zeros((g.H, g.W), dtype=np.int64)
    for ty in range(g.Ly):
        y0 = ty * g.stride - g.pad_y
        a, b = max(y0, 0), min(y0 + g.patch, g.H)
        for tx in range(g.Lx):
            x0 = tx * g.stride - g.pad_x
            c, d = max(x0, 0), min(x0 + g.patch, g.W)
            if a < b and c < d:
                acc[:, :, a:b, c:d] += tiles[:, ty, tx, :, a - y0:b - y0, c - x0:d - x0]
                cnt[a:b, c:d] += 1
    assert cnt.min() >= 1
    return acc * (np.float32(1.0) / cnt.astype(np.float32)), cnt


def _fold_float64(tiles, g, N):
    """nn.Fold(...) / divisor in float64, the sum of |v| per pixel and the cover counts."""
    fold = nn.Fold(output_size=(g.H, g.W), kernel_size=g.patch, stride=g.stride, padding=(g.pad_y, g.pad_x))
    cols = tiles.double().reshape(N, g.Ly * g.Lx, -1).transpose(1, 2)
    k = fold(torch.ones_like(cols[:1, :g.patch * g.patch]))[0, 0]
    return fold(cols) / k, fold(cols.abs()), k


def _rand(*shape, seed=0):
    """Values with full 24-bit significands (torch.rand alone leaves the low bits of small values empty)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) + 0.5) * torch.exp2(torch.randint(-3, 3, shape, generator=g).float()) \
        * (1 - 2 * torch.randint(0, 2, shape, generator=g).float())


# ---- unfold ----------------------------------------------------------------------------------------------------------------
# (N, C, H, W, patch, stride): the OASIS slice at x4, odd sizes, three channels, a patch that is no multiple of four pixels
UNFOLD_CASES = [(2, 1, 34, 42, 24, 16), (3, 3, 20, 27, 16, 8), (2, 1, 33, 16, 16, 8), (2, 3, 17, 63, 8, 6), (2, 1, 9, 31, 6, 3),
                (1, 3, 16, 16, 16, 16)]


@pytest.mark.parametrize("pad_mode", ["zero", "edge"])
@pytest.mark.parametrize("N,C,H,W,p,s", UNFOLD_CASES)
def test_unfold_is_nn_unfold(N, C, H, W, p, s, pad_mode):
    plan = T.TilePlan(H, W, p, s, pad_mode=pad_mode)
    x = _rand(N, C, H, W, seed=H + W)
    want = _unfold_oracle(x, plan)
    total = N * plan.tiles_per_slice
    got = T.unfold_tiles(x.to(DEV), plan)
    assert tuple(got.shape) == (total, C, p, p) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    # a window of slots that crosses the end: the tail is zeros, whatever the caller's tensor held
    first, slots = max(total - 3, 0), 7
    out = torch.full((slots, C, p, p), float("nan"), device=DEV)
    back = T.unfold_tiles(x.to(DEV), plan, out=out, first_tile=first)
    assert back is out
    assert torch.equal(out[:total - first].cpu(), want[first:]) and not out[total - first:].any() and not out.isnan().any()
    mid = T.unfold_tiles(x.to(DEV), plan, first_tile=1, n_slots=2)
    assert torch.equal(mid.cpu(), want[1:3]) if total >= 3 else tuple(mid.shape) == (2, C, p, p)
    # an unaligned destination takes the scalar stores
    flat = torch.empty(total * C * p * p + 1, device=DEV)
    odd = T.unfold_tiles(x.to(DEV), plan, out=flat[1:].view(total, C, p, p))
    assert torch.equal(odd.cpu(), want)


def test_unfold_and_fold_refuse_what_does_not_fit():
    plan = T.TilePlan(20, 27, 16, 8, scale=2)
    x = torch.rand(2, 1, 20, 27, device=DEV)
    with pytest.raises(ValueError):
        T.unfold_tiles(x[:, :, :19], plan)
    with pytest.raises(ValueError):
        T.unfold_tiles(x, plan, out=torch.empty(3, 1, 16, 8, device=DEV))
    with pytest.raises(ValueError):
        T.unfold_tiles(x, plan, first_tile=-1)
    with pytest.raises(TypeError):
        T.unfold_tiles(x.double(), plan)
    with pytest.raises(ValueError):
        T.fold_tiles(torch.rand(12, 1, 16, 16, device=DEV), plan, 2)        # LR-sized tiles for the x2 side
    with pytest.raises(ValueError):
        T.fold_tiles(torch.rand(11, 1, 32, 32, device=DEV), plan, 2)


# ---- fold ------------------------------------------------------------------------------------------------------------------
# (N, C, H, W, patch, stride, scale)
FOLD_CASES = [(2, 1, 34, 42, 24, 16, 4), (3, 3, 20, 27, 16, 8, 2), (2, 1, 33, 16, 16, 8, 4), (2, 3, 17, 63, 8, 6, 1),
              (2, 1, 9, 31, 6, 3, 1), (2, 2, 21, 30, 8, 2, 1), (1, 1, 16, 16, 16, 16, 4)]


@pytest.mark.parametrize("N,C,H,W,p,s,scale", FOLD_CASES)
def test_fold_is_the_stated_sum(N, C, H, W, p, s, scale):
    plan = T.TilePlan(H, W, p, s, scale=scale)
    g = plan.hr
    tiles = _rand(N * plan.tiles_per_slice, C, g.patch, g.patch, seed=H * W)
    want, cnt = _fold_restated(tiles.numpy(), g, N)
    assert np.array_equal(cnt, plan.cover(hr=True))
    got = T.fold_tiles(tiles.to(DEV), plan, N)
    again = T.fold_tiles(tiles.to(DEV), plan, N)
    assert tuple(got.shape) == (N, C, scale * H, scale * W) and got.dtype == torch.float32
    assert torch.equal(got, again)                                   # no atomics: the same bits on every run
    assert np.array_equal(got.cpu().numpy(), want)
    # against float64 nn.Fold / divisor: k - 1 rounded adds, one rounded reciprocal, one rounded multiply
    exact, sum_abs, k = _fold_float64(tiles, g, N)
    assert np.array_equal(k.numpy(), cnt)
    bound = (k + 1) * EPS * sum_abs / k
    err = (got.cpu().double() - exact).abs()
    print(f"fold {H}x{W} p={p} s={s} x{scale}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}, "
          f"k up to {int(k.max())}")
    assert (err <= bound).all()


@pytest.mark.parametrize("pad_mode", ["zero", "edge"])
@pytest.mark.parametrize("N,C,H,W,p,s", UNFOLD_CASES + [(2, 2, 21, 30, 8, 2)])
def test_fold_of_unfold_gives_the_slices_back(N, C, H, W, p, s, pad_mode):
    """Every covering tile holds the pixel's own value v, so the fold sums k copies of it.  The running sums 2v and (proved
    below) 4v are exact, and so is a multiply by the exact reciprocal of a power of two: the pixel comes back bit for bit
    where k is 1, 2 or 4.  (3v rounds to a multiple r of the spacing with |r - 3v| at most half of it, and r + v = 4v + (r - 3v)
    rounds back to 4v: in a tie, r - 3v is half a spacing only when 3v's significand is 2 mod 4, so v's is even, and the tie
    goes to the even neighbour 4v.)  Longer running sums of copies (5v, 6v, 7v before 8v) round on the way: in the fp32 numpy
    restatement of the stated order itself, on the 21 x 30 / 8 / 2 case below, 217 of the 480 pixels with k = 8 and 566 of the
    800 with k = 16 do not come back exactly (k = 3: 22 of 80), and the kernel equals that restatement bit for bit
    (test_fold_is_the_stated_sum).  So for 8 and 16, as for every k that is no power of two, the bound of the fold holds
    instead; every plan with stride >= patch / 2 has k in {1, 2, 4} only."""
    plan = T.TilePlan(H, W, p, s, pad_mode=pad_mode)
    x = _rand(N, C, H, W, seed=3 * H + W)
    back = T.fold_tiles(T.unfold_tiles(x.to(DEV), plan), plan, N).cpu()
    k = torch.from_numpy(plan.cover()).expand(N, C, H, W)
    exact = (k == 1) | (k == 2) | (k == 4)
    assert torch.equal(back[exact], x[exact])
    bound = (k + 1).double() * EPS * x.abs().double()
    assert ((back.double() - x.double()).abs() <= bound).all()


# ---- the tiled tester ------------------------------------------------------------------------------------------------------
def _net(mode="fp32", seed=7):
    from rdst_amd.networks.rdst_variations import RDSTSR
    cfg = O.make_cfg(**{**O.CFG_TINY, "img_size": 16})
    net = RDSTSR(img_size=16, in_chans=1, sr_scale=4, embed_dim=48, dense_layer_depths=[2, 2], num_heads=[6, 6],
                 window_size=[8, 8], rdb_depths=[3, 3], mlp_ratio=2.0, growth_rate=24, pre_norm=True,
                 feature_last_operation=True)
    net.load_state_dict(O.make_weights(cfg, seed), strict=True)
    net.to(DEV).train()
    if mode != "fp32":
        net.set_compute_dtype(mode)
    return net


def _weights(seed):
    return O.make_weights(O.make_cfg(**{**O.CFG_TINY, "img_size": 16}), seed)


def _slices(n, h, w, seed=2):
    return torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(seed))


def _spelled_out(net, lr, tile, stride, tile_batch, pad_mode="zero"):
    """What the tiled tester must compute: nn.Unfold tiles, the network in eval mode on tile_batch of them at a time, the fp32
    fold restatement."""
    plan = T.TilePlan(lr.shape[-2], lr.shape[-1], tile, stride, scale=4, pad_mode=pad_mode)
    tiles = _unfold_oracle(lr, plan).to(DEV)
    was = net.training
    net.eval()
    with torch.no_grad(), ops.keep_pack_plan(net):      # (the caller may be in the middle of a training run)
        sr = torch.cat([net(b) for b in tiles.split(tile_batch)]).float().cpu()
    net.train(was)
    return torch.from_numpy(_fold_restated(sr.numpy(), plan.hr, lr.shape[0])[0])


SLICES = [(3, 20, 27), (2, 33, 16)]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_tiled_inference_is_the_spelled_out_loop(mode):
    from rdst_amd.tester import SRTester
    net = _net(mode)
    code = net.compute_code
    tester = SRTester(net, tile=16, tile_stride=8, tile_batch=5)
    for i, (n, h, w) in enumerate(SLICES):
        lr = _slices(n, h, w, seed=i)
        rec = tester.inference(lr)
        assert tuple(rec.shape) == (n, 1, 4 * h, 4 * w) and rec.dtype == torch.float32 and rec.is_cuda
        assert torch.equal(rec.cpu(), _spelled_out(net, lr, 16, 8, 5))
        # chunks of whole slices (a budget of one slice's tiles) and slices that are already on the device change nothing
        small = SRTester(net, tile=16, tile_stride=8, tile_batch=5, tile_buffer_bytes=1)
        assert torch.equal(small.inference(lr.to(DEV)), rec)
    assert net.compute_code == code and tester.graph_captures == 0 and tester.graph_replays == 0
    edge = SRTester(net, tile=16, tile_stride=8, tile_batch=4, pad_mode="edge")
    lr = _slices(2, 20, 27, seed=5)
    assert torch.equal(edge.inference(lr).cpu(), _spelled_out(net, lr, 16, 8, 4, "edge"))


def test_evaluate_on_device_takes_the_tiled_path():
    from rdst_amd.tester import SRTester
    net = _net("bf16")
    tester = SRTester(net, tile=16, tile_stride=8, tile_batch=8)
    lr, gt = _slices(3, 20, 27), torch.rand(3, 1, 80, 108, generator=torch.Generator().manual_seed(9))
    dev, host = tester.evaluate(lr, gt, on_device=True), tester.evaluate(lr, gt)
    assert set(dev) == set(host) == {"psnr", "ssim"} and len(dev["psnr"]) == 3
    assert np.allclose(dev["psnr"], host["psnr"], rtol=0, atol=1e-9) and np.allclose(dev["ssim"], host["ssim"], rtol=0, atol=1e-10)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_graph_replays_equal_the_eager_tiles(mode):
    from rdst_amd.tester import SRTester
    net = _net(mode)
    eager = SRTester(net, tile=16, tile_stride=8, tile_batch=5)
    graph = SRTester(net, tile=16, tile_stride=8, tile_batch=5, graph=True)
    for i, (n, h, w) in enumerate(SLICES + SLICES):
        lr = _slices(n, h, w, seed=10 + i)
        assert torch.equal(graph.inference(lr), eager.inference(lr)), (i, h, w)
    assert graph.graph_captures == 1 and graph.graph is not None and graph.graph_replays > 0
    replays = graph.graph_replays
    # other weights, loaded in place: the captured forward repacks the live parameters, nothing is captured again
    net.load_state_dict(_weights(8), strict=True)
    lr = _slices(3, 20, 27, seed=20)
    got = graph.inference(lr)
    assert graph.graph_captures == 1 and graph.graph_replays == replays + 4          # 18 tiles in batches of 5
    assert torch.equal(got.cpu(), _spelled_out(net, lr, 16, 8, 5))
    assert torch.equal(got, SRTester(net, tile=16, tile_stride=8, tile_batch=5).inference(lr))
    net.load_state_dict(_weights(7), strict=True)
    assert not torch.equal(graph.inference(lr), got)
    # another compute mode is another forward: the graph is dropped and captured again
    other = "bf16" if mode != "bf16" else "fp32"
    net.set_compute_dtype(other)
    assert torch.equal(graph.inference(lr).cpu(), _spelled_out(net, lr, 16, 8, 5))
    assert graph.graph_captures == 2


def test_graph_refreshes_the_packed_weights_it_reads():
    """A network of the E1 widths (its bf16 forward reads prepacked weight images, refreshed at the start of every forward): the
    captured forward holds that refresh, so parameters changed in place show in the next replay, and the network's own plan
    (none here: it never ran outside the tester) is as it was after every call."""
    from rdst_amd.networks.rdst_variations import RDSTSR
    from rdst_amd.tester import SRTester
    torch.manual_seed(0)
    net = RDSTSR(img_size=16, patch_size=1, in_chans=1, sr_scale=4, embed_dim=60, dense_layer_depths=[2, 2], num_heads=[6, 6],
                 window_size=[8, 8], rdb_depths=[3, 3], mlp_ratio=2., growth_rate=30, pre_norm=True, feature_last_operation=True)
    net.to(DEV).train().set_compute_dtype(torch.bfloat16)
    eager = SRTester(net, tile=16, tile_stride=8, tile_batch=5)
    graph = SRTester(net, tile=16, tile_stride=8, tile_batch=5, graph=True)
    lr = _slices(3, 20, 27, seed=1)
    first = graph.inference(lr)
    assert ops.pack_plan_of(net) is None
    assert graph.graph_captures == 1 and graph._graph_plan is not None and graph._graph_plan.valid(net)
    assert torch.equal(first, eager.inference(lr)) and ops.pack_plan_of(net) is None
    with torch.no_grad():
        for prm in net.parameters():
            prm.mul_(1.03125)
    second = graph.inference(lr)
    assert graph.graph_captures == 1 and not torch.equal(second, first)
    assert torch.equal(second, eager.inference(lr))
    assert torch.equal(second.cpu(), _spelled_out(net, lr, 16, 8, 5))


def test_a_slice_of_one_tile_is_the_whole_slice_path():
    from rdst_amd.tester import SRTester
    net = _net("bf16")
    lr = _slices(4, 16, 16)
    whole = SRTester(net).inference(lr)
    for graph in (False, True):
        tester = SRTester(net, tile=16, tile_stride=16, tile_batch=4, graph=graph)
        assert tester._tile_plan(16, 16).tiles_per_slice == 1
        for _ in range(4):          # (with graph=True: up to two eager batches, then the capture and replays)
            assert torch.equal(tester.inference(lr), whole)
        assert tester.graph_captures == int(graph) and tester.graph_replays == (0 if not graph else 4 - tester._eager_full)


def test_constructor_refuses_bad_tiles():
    from rdst_amd.tester import SRTester
    net = _net()
    with pytest.raises(ValueError, match="window size"):
        SRTester(net, tile=12)
    with pytest.raises(ValueError):
        SRTester(net, tile=16, tile_stride=24)
    with pytest.raises(ValueError):
        SRTester(net, tile=16, tile_batch=0)
    with pytest.raises(ValueError):
        SRTester(net, tile=16, pad_mode="reflect")
    with pytest.raises(ValueError):
        SRTester(net, tile=16, sr_scale=2.5)
    with pytest.raises(ValueError, match="uncovered"):
        SRTester(net, tile=16, tile_stride=4).inference(_slices(1, 4, 32))
    SRTester(net, tile=None, graph=True).inference(_slices(1, 16, 16))       # tile=None: nothing changes


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_run_unchanged_by_tiled_inference(graph):
    """Six steps with a graph-replayed tiled inference after steps 2 and 4 give the losses and parameters of six steps without
    it, bit for bit; in the graph run the first call falls between the eager warm-up and the capture of the training step, the
    second between its replays.  (The relative-position bias tables are frozen as in tests/test_quick_eva_gpu.py: their
    gradient is summed with LDS float atomics.)  The second call replays the graph captured by the first and must see the
    parameters as the steps in between left them."""
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
        tr = DPTrainStep(net, lr=1e-3, graph=graph, graph_warmup=2)
        tester = SRTester(net, tile=16, tile_stride=8, tile_batch=4, graph=True)
        losses = []
        for i, (x, t) in enumerate(data):
            losses.append(tr.step(x, t).clone())
            if with_inference and i in (1, 3):
                plan = ops.pack_plan_of(net)
                rec = tester.inference(lr)
                assert ops.pack_plan_of(net) is plan
                assert torch.equal(rec.cpu(), _spelled_out(net, lr, 16, 8, 4))
                assert ops.pack_plan_of(net) is plan
        torch.cuda.synchronize()
        assert (tr.graph is not None) == graph
        if with_inference:
            assert tester.graph_captures == 1 and tester.graph_replays >= 5
        res[with_inference] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), tr.loss_records()["L1"])
    assert res[False][0] == res[True][0]
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2] == res[True][2] == res[False][0]
