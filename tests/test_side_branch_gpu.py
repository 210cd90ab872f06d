"""The side branch of the deferred reductions (rdst_amd/side.py, csrc/reduce_batch.hip): a DenseSTLayer's slab sums and
LayerNorm finishes run on a side stream beside the next layer's backward.  The kernels, their job order and their summation
order are the same on either stream, so every comparison with the serial step is ``torch.equal``.

The network has widths 60 / 90 / 120: three layer flushes and the final join, the smallest shape that turns the ring of
generations over."""
import pytest
import torch
import torch.nn.functional as F

from rdst_amd import _lib, dp, ops, side
from rdst_amd.networks.rdst_variations import RDSTSR
from rdst_amd.trainer import DPTrainStep

gpu = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 5        # graph_warmup = 2 eager steps, then the capture and three replays


def make_net(img=16):
    torch.manual_seed(0)
    net = RDSTSR(img_size=img, in_chans=1, sr_scale=2, embed_dim=60, dense_layer_depths=[2], num_heads=[6], window_size=[8],
                 rdb_depths=[3], growth_rate=30, pre_norm=True, feature_last_operation=True)
    return net.to(DEV).train().set_compute_dtype("bf16")


def batches(img=16, n=STEPS):
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(2, 1, img, img, generator=g).to(DEV), torch.rand(2, 1, 2 * img, 2 * img, generator=g).to(DEV))
            for _ in range(n)]


def dirty_allocator():
    """Freed blocks full of NaN: a slab released before its sum has read it, or a gradient read before its deferred write,
    would see them."""
    junk = [torch.full((1 << 20,), float("nan"), device=DEV) for _ in range(8)]
    del junk


def run_steps(graph, img=16, n=STEPS):
    """[(bucket, parameters)] after each of n trainer steps, and the trainer."""
    tr = DPTrainStep(make_net(img), lr=1e-3, graph=graph, graph_warmup=2)
    out = []
    for x, t in batches(img, n):
        tr.step(x, t)
        out.append((tr.bucket.flat.clone(), tr.optimizer.flat_param.clone()))
    torch.cuda.synchronize()
    return out, tr


def plain_grads(net, x, t, passes=1, zero=None):
    """Gradients of `passes` plain backward passes (no trainer around them), flattened."""
    if zero is not None:
        zero()
    for _ in range(passes):
        dirty_allocator()
        F.l1_loss(net(x), t).backward()
    torch.cuda.synchronize()
    return torch.cat([p.grad.reshape(-1) for p in net.parameters() if p.grad is not None]).clone()


@pytest.fixture(autouse=True)
def stage_one(monkeypatch):
    """Every test starts with the reductions on the side branch and the conv stage off, whatever the process's switches say,
    and leaves the branch off."""
    monkeypatch.setattr(side, "SIDE_BRANCH", True)    # what RDST_SIDE_BRANCH / RDST_SIDE_CONV set at import
    monkeypatch.setattr(side, "SIDE_CONV", False)
    yield
    side.disable()


@pytest.fixture
def side_off(stage_one, monkeypatch):
    monkeypatch.setattr(side, "SIDE_BRANCH", False)


@pytest.fixture(scope="module")
def serial():
    """The serial step (both switches 0), computed once: the graph trainer's five steps."""
    was = side.SIDE_BRANCH, side.SIDE_CONV
    side.SIDE_BRANCH = side.SIDE_CONV = False
    try:
        out, tr = run_steps(graph=True)
        assert tr.graph is not None
        return out
    finally:
        side.SIDE_BRANCH, side.SIDE_CONV = was


@gpu
def test_eager_fwd_bwd_equals_serial(serial):
    tr = DPTrainStep(make_net(), lr=1e-3)
    x, t = batches()[0]
    seen = []
    first = next(p for p in tr.net.parameters() if p.requires_grad)   # its gradient comes last: every layer has flushed by then
    h = first.register_hook(lambda g: seen.append((side.enabled(), len(side._parked.get(torch.cuda.current_device(), ())))))
    dirty_allocator()
    tr.fwd_bwd(x, t)
    h.remove()
    torch.cuda.synchronize()
    assert torch.equal(tr.bucket.flat, serial[0][0])
    # the branch was on inside the backward and at most two layers' slabs were parked; the join released them
    assert seen and seen[-1][0] and 1 <= seen[-1][1] <= 2, seen
    assert not side._parked and not side.enabled()


@gpu
def test_graph_step_equals_serial(serial):
    out, tr = run_steps(graph=True)
    assert tr.graph is not None                         # a failed capture falls back to eager: that would pass everything below
    for k, ((gb, gp), (wb, wp)) in enumerate(zip(out, serial)):
        assert torch.equal(gb, wb), f"bucket after step {k}"
        assert torch.equal(gp, wp), f"parameters after step {k}"
    assert _lib.load().rdst_side_enable(0) == 0         # step() left the branch off


@gpu
@pytest.mark.parametrize("reductions", [True, False])
def test_conv_weight_gradients_on_the_side_equal_serial(side_off, monkeypatch, reductions):
    """The conv stage (RDST_SIDE_CONV=1), with and without the reductions beside it: at 32 x 32 the 150 -> 60, 60 -> 60 and
    60 -> 240 + PixelShuffle convs take the register-stationary weight-gradient kernels and the tail conv the one-channel
    ones, the four that move to the side stream.  Two eager steps, the capture and two replays."""
    want, tr = run_steps(graph=True, img=32, n=4)
    assert tr.graph is not None
    side.SIDE_BRANCH = reductions                        # (the fixture restores it)
    monkeypatch.setattr(side, "SIDE_CONV", True)
    got, tr = run_steps(graph=True, img=32, n=4)
    assert tr.graph is not None
    for k, ((gb, gp), (wb, wp)) in enumerate(zip(got, want)):
        assert torch.equal(gb, wb), f"bucket after step {k}"
        assert torch.equal(gp, wp), f"parameters after step {k}"
    assert _lib.load().rdst_side_enable(0) == 0 and not side._parked


@gpu
def test_fresh_destinations_and_accumulation_equal_serial(side_off):
    """bucket.zero() + backward without detach_grads(): every destination is fresh, autograd reads it when the node returns,
    so every such flush joins.  Then two passes without zeroing in between."""
    x, t = batches()[0]
    net = make_net()
    bucket = dp.FlatGradBucket(net.parameters())
    want1 = plain_grads(net, x, t, zero=bucket.zero)
    want2 = plain_grads(net, x, t, passes=2, zero=bucket.zero)
    side.SIDE_BRANCH = True                              # (the fixture restores it)
    for want, passes in ((want1, 1), (want2, 2)):
        assert side.enable()
        try:
            got = plain_grads(net, x, t, passes=passes, zero=bucket.zero)
        finally:
            side.join()
            side.disable()
        assert bucket.check_views()
        assert torch.equal(got, want), passes


@gpu
def test_backward_that_raises_then_reset(serial):
    tr = DPTrainStep(make_net(), lr=1e-3)
    mid = [p for n, p in tr.net.named_parameters() if n.endswith("attn.proj.weight")][3]   # second layer, second block: the layer's batch is open around it

    def boom(_g):
        raise RuntimeError("boom")
    h = mid.register_hook(boom)
    x, t = batches()[0]
    with pytest.raises(RuntimeError, match="boom"):
        tr.fwd_bwd(x, t)
    h.remove()
    assert not side.enabled()                            # fwd_bwd's finally
    ops.reset_backward_state()
    assert not side._parked
    for k, (x, t) in enumerate(batches()[:2]):
        tr.step(x, t)
        torch.cuda.synchronize()
        assert torch.equal(tr.bucket.flat, serial[k][0]), k
        assert torch.equal(tr.optimizer.flat_param, serial[k][1]), k


@gpu
def test_plain_backward_after_a_step_is_the_serial_one(side_off):
    x, t = batches()[0]
    net = make_net()
    want = plain_grads(net, x, t)
    side.SIDE_BRANCH = True
    tr = DPTrainStep(make_net(), lr=0.0)                 # lr 0: the step leaves the parameters as they were
    tr.step(x, t)
    assert _lib.load().rdst_side_enable(0) == 0          # already off
    for p in tr.net.parameters():
        p.grad = None
    assert torch.equal(plain_grads(tr.net, x, t), want)
    assert not side._parked


def test_entry_points_load_without_a_device():
    lib = _lib.load()
    for name in ("rdst_side_enable", "rdst_side_join", "rdst_side_reset"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.rdst_side_enable(0) == 0
    assert lib.rdst_side_reset() == 0
    assert lib.rdst_side_enable(1) == 0 and lib.rdst_side_enable(0) == 1   # the previous value, no HIP call behind it
    assert lib.rdst_side_reset() == 0
