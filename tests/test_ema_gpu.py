"""GPU: the weight EMA - rdst_adam_step_ema / rdst_adam_step_dev_ema / rdst_swap_f32 (include/rdst_hip.h) behind
FlatAdam(ema_decay=...) and DPTrainStep(ema_decay=...).

Optimizer level, on synthetic flat parameters of 3 (tail only), 4, 1027 (tail of 3) and 2^21 + 2^10 + 3 elements (grid-stride
wrap plus tail): the EMA leaves Adam's bits alone, follows the float64 recurrence on the kernel's own parameter trajectory,
agrees between the host-count and the device-count launch, stands still on a skipped step, and the in-place exchange is exact.

The gate of the rule is derived, not tuned: after K updates, elementwise |e - E| <= 3 K 2^-24 max(|p|, |e|).  Per update
the kernel rounds three times - the subtraction p_new - e, the factor omd = (float)(1 - d_t), and the fmaf - each by at most
2^-24 relative to a term bounded by that maximum, and the error of earlier updates is damped by d_t <= 1.  The oracle is
E <- E + (p_new - E) (1 - d_t) in float64 with d_t from ema_decay_at.

Trainer level, on the tiny RDSTSR of tests/test_quick_eva_gpu.py (batch 2, 16x16 LR, fp32 and bf16; the relative-position
bias tables frozen where runs are compared bit for bit, as tests/test_step_guard_gpu.py explains): graph against eager,
training unaffected by the EMA and by evaluations on it, evaluation sees the average, an SRTester graph captured on the live
weights survives the exchange, and checkpoints resume bit for bit."""
import pytest
import torch

from rdst_amd import ops
from test_optim_gpu import _nets
from test_quick_eva_gpu import _net as _tiny_rdst
from test_quick_eva_gpu import _validation_set
from test_step_guard_gpu import BIG, LOSSES, _tiny_rdst_fixed_tables

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYPER = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8)
SIZES = [3, 4, 1027, BIG]
K = 6
U = 2.0 ** -24


def _opt(n, **kw):
    from rdst_amd.optim import FlatAdam
    w = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    return FlatAdam([torch.nn.Parameter(w)], **HYPER, **kw)


def _grads(n, k=K, seed=0):
    """Seeded gradients, from 1e-3 to 1e2 in size (step k has scale 10^(k - 3))."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(n, device="cuda", generator=gen) * 10.0 ** float(i - 3) for i in range(k)]


def _oracle_update(E, p_new, t, decay, warmup):
    from rdst_amd.optim import ema_decay_at
    return E + (p_new.double() - E) * (1.0 - ema_decay_at(t, decay, warmup))


def _magnitude(opt):
    return torch.maximum(opt.flat_param.double().abs(), opt.ema.double().abs())


def _worst_ratio(opt, E, k, magnitude=None):
    """max over the elements of |e - E| / (3 k 2^-24 max(|p|, |e|)); an element where both are 0 must match exactly.
    ``magnitude``: the elementwise maximum to use instead of the one of the final p and e."""
    e = opt.ema.double()
    gate = 3.0 * k * U * (magnitude if magnitude is not None else _magnitude(opt))
    err = (e - E).abs()
    assert bool((err[gate == 0] == 0).all())
    return (err[gate > 0] / gate[gate > 0]).max().item() if bool((gate > 0).any()) else 0.0


# ---- 1. the EMA does not perturb Adam ----------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("device_state", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_does_not_perturb_adam(n, device_state, wd):
    oa = _opt(n, weight_decay=wd, device_state=device_state, ema_decay=0.999)
    ob = _opt(n, weight_decay=wd, device_state=device_state)
    assert ob.ema is None and torch.equal(oa.ema, oa.flat_param)
    for k, gr in enumerate(_grads(n)):
        oa.bucket.flat.copy_(gr)
        ob.bucket.flat.copy_(gr)
        oa.step()
        ob.step()
        for name in ("flat_param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(oa, name), getattr(ob, name)), (k, name)
    assert not torch.equal(oa.ema, oa.flat_param)
    if device_state:
        assert oa.sync_host()["kept"] == ob.sync_host()["kept"] == K
    else:
        assert oa._steps == ob._steps == K


# ---- 2. the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_state", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("decay", [0.999, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_ema_follows_the_float64_recurrence(n, decay, warmup, device_state):
    opt = _opt(n, device_state=device_state, ema_decay=decay, ema_warmup=warmup)
    E = opt.flat_param.double()
    for k, gr in enumerate(_grads(n), start=1):
        opt.bucket.flat.copy_(gr)
        opt.step()
        E = _oracle_update(E, opt.flat_param, k, decay, warmup)      # the kernel's own parameter trajectory
    ratio = _worst_ratio(opt, E, K)
    print(f"n={n} decay={decay} warmup={warmup} device_state={device_state}: worst |e - E| / gate = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("device_state", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_gradients_are_a_fixed_point(n, device_state):
    opt = _opt(n, device_state=device_state, ema_decay=0.5, ema_warmup=True)
    start = opt.flat_param.clone()
    for _ in range(3):
        opt.bucket.flat.zero_()
        opt.step()
        assert torch.equal(opt.ema, opt.flat_param)
    assert torch.equal(opt.flat_param, start)


# ---- 3. the host-count and the device-count launch agree ---------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("n", SIZES)
def test_host_and_device_count_paths_agree(n, warmup):
    oh = _opt(n, weight_decay=0.01, ema_decay=0.999, ema_warmup=warmup)
    od = _opt(n, weight_decay=0.01, ema_decay=0.999, ema_warmup=warmup, device_state=True)
    for gr in _grads(n):
        oh.bucket.flat.copy_(gr)
        od.bucket.flat.copy_(gr)
        oh.step()
        od.step()                    # no guard() before it: the step is kept
    assert torch.equal(oh.flat_param, od.flat_param)
    assert torch.equal(oh.ema, od.ema)


# ---- 4. skipped steps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("n", SIZES)
def test_a_skipped_step_leaves_the_ema_alone(n, warmup):
    """On a skipped step (NaN, inf, above the threshold) the EMA is bit for bit what it was; after the sequence it matches
    the oracle driven by the KEPT updates only.
    The gate here is the derivation of the module docstring taken at its word: each of the three roundings of an update is
    relative to a term of THAT update, so the bound is 3 K 2^-24 times the largest |p|, |e| the element had on the way, not
    the ones it ends with.  The two differ only where an element shrinks: Adam moves every element by about lr = 1e-3 per
    update whatever the gradient, so among 2^21 elements some cross zero and end near it with an |e - E| of a few
    2^-24 x 1e-3 from the updates before.  Measured on an MI355X against the FINAL values: worst ratio 0.04 / 0.12 at
    3, 4 / 1027 elements, 1.76 (flat) and 1.30 (warm-up) at 2^21 + 2^10 + 3; test_ema_follows_the_float64_recurrence holds
    the final-value form at every size (worst 0.71)."""
    decay = 0.5                      # with warmup, d_t = (1 + t) / (10 + t) < 0.5 for all five kept updates: t must be `kept`
    opt = _opt(n, device_state=True, ema_decay=decay, ema_warmup=warmup)
    E = opt.flat_param.double()
    seen = _magnitude(opt)
    kept = 0
    for gr, lv in zip(_grads(n, len(LOSSES)), LOSSES):
        opt.bucket.flat.copy_(gr)
        before = [t.clone() for t in (opt.ema, opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        opt.guard(torch.tensor(lv, device="cuda"), 1.0)
        opt.step()
        if lv < 1.0:
            kept += 1
            E = _oracle_update(E, opt.flat_param, kept, decay, warmup)
            seen = torch.maximum(seen, _magnitude(opt))
            assert not torch.equal(opt.flat_param, before[1])
        else:                        # NaN, inf, above the threshold
            for t, b in zip((opt.ema, opt.flat_param, opt.exp_avg, opt.exp_avg_sq), before):
                assert torch.equal(t, b), lv
    st = opt.sync_host()
    assert (st["kept"], st["skipped"]) == (kept, len(LOSSES) - kept) == (5, 3)
    ratio = _worst_ratio(opt, E, kept, seen)
    print(f"n={n} warmup={warmup}: worst |e - E| / gate = {ratio:.3f} (against the final values: {_worst_ratio(opt, E, kept):.3f})")
    assert ratio <= 1.0


# ---- 5. the exchange ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_state", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_in_place_and_blocks_training(n, device_state):
    opt = _opt(n, device_state=device_state, ema_decay=0.999)
    opt.ema.copy_(torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)))
    p0, e0 = opt.flat_param.clone(), opt.ema.clone()
    ptrs = (opt.flat_param.data_ptr(), opt.ema.data_ptr())
    assert not torch.equal(p0, e0)
    opt.swap_ema()
    assert opt.ema_active and torch.equal(opt.flat_param, e0) and torch.equal(opt.ema, p0)
    assert torch.equal(opt.param_groups[0]["params"][0].data, e0)       # the parameter is a view: it sees the average
    opt.swap_ema()
    assert not opt.ema_active and torch.equal(opt.flat_param, p0) and torch.equal(opt.ema, e0)
    assert ptrs == (opt.flat_param.data_ptr(), opt.ema.data_ptr())
    opt.bucket.flat.fill_(0.5)
    with opt.ema_scope():
        assert opt.ema_active and torch.equal(opt.flat_param, e0)
        with pytest.raises(RuntimeError, match="averaged"):
            opt.step()
        if device_state:
            with pytest.raises(RuntimeError, match="averaged"):
                opt.guard(None, 0.0)
        with pytest.raises(RuntimeError):
            opt.reset_ema()
    assert not opt.ema_active
    with pytest.raises(KeyError):
        with opt.ema_scope():
            raise KeyError("the body fails")
    assert not opt.ema_active and torch.equal(opt.flat_param, p0) and torch.equal(opt.ema, e0)
    assert torch.equal(opt.exp_avg, torch.zeros_like(p0))               # none of the refused steps launched
    opt.step()                                                          # outside the scope training goes on
    assert not torch.equal(opt.flat_param, p0)


# ---- trainer level -----------------------------------------------------------------------------------------------------
def _batches(n=6):
    g = torch.Generator().manual_seed(5)
    return [(torch.rand(2, 1, 16, 16, generator=g).to(DEV), torch.rand(2, 1, 64, 64, generator=g).to(DEV)) for _ in range(n)]


def _fresh(mode, state_dict):
    """A freshly constructed network with ``state_dict`` loaded strictly, in eval mode."""
    net = _tiny_rdst(mode)
    net.load_state_dict(state_dict, strict=True)
    return net.eval()


# ---- 6. graph against eager --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graph_step_updates_the_ema_like_the_eager_step(mode):
    from rdst_amd.trainer import DPTrainStep
    kw = dict(lr=1e-3, device_guard=True, ema_decay=0.999, ema_warmup=True)
    gr_tr = DPTrainStep(_tiny_rdst_fixed_tables(mode), graph=True, graph_warmup=2, **kw)
    eg_tr = DPTrainStep(_tiny_rdst_fixed_tables(mode), **kw)
    for x, t in _batches():
        gr_tr.step(x, t)
        eg_tr.step(x, t)
    assert gr_tr.graph is not None and gr_tr._graph_has_update and eg_tr.graph is None
    assert gr_tr.guard_stats()["kept"] == eg_tr.guard_stats()["kept"] == 6
    assert torch.equal(gr_tr.optimizer.flat_param, eg_tr.optimizer.flat_param)
    assert torch.equal(gr_tr.optimizer.ema, eg_tr.optimizer.ema)
    assert not torch.equal(gr_tr.optimizer.ema, gr_tr.optimizer.flat_param)


# ---- 7. training is unaffected -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["eager", "graph", "graph_guard"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_run_unchanged_by_the_ema(mode, variant):
    from rdst_amd.trainer import DPTrainStep
    kw = dict(lr=1e-3, graph=variant != "eager", graph_warmup=2, device_guard=variant == "graph_guard")
    lr, hr = _validation_set(n=6, h=16, w=16)
    res = {}
    for with_ema in (False, True):
        net = _tiny_rdst_fixed_tables(mode)
        tr = DPTrainStep(net, **kw, **(dict(ema_decay=0.999) if with_ema else {}))
        losses = []
        for i, (x, t) in enumerate(_batches()):
            losses.append(tr.step(x, t).clone())
            if with_ema and i in (1, 3):
                plan, graph = ops.pack_plan_of(net), tr.graph
                tr.quick_eva(lr, hr, num_samples=4, batch_size=1, generator=torch.Generator().manual_seed(i), use_ema=True)
                assert ops.pack_plan_of(net) is plan and tr.graph is graph and not tr.optimizer.ema_active
        torch.cuda.synchronize()
        assert (tr.graph is not None) == (variant != "eager")
        assert len(tr.quick_validation_reports) == (2 if with_ema else 0)
        res[with_ema] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), tr.loss_records()["L1"])
    assert res[False][0] == res[True][0]
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2] == res[True][2]


# ---- 8. evaluation sees the average ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_evaluation_sees_the_average(mode):
    from rdst_amd.trainer import DPTrainStep
    net = _tiny_rdst_fixed_tables(mode)              # frozen parameters and buffers next to the trainable ones
    tr = DPTrainStep(net, lr=1e-2, ema_decay=0.999)
    for x, t in _batches(3):
        tr.step(x, t)
    x = _batches(1)[0][0]
    esd, sd = tr.ema_state_dict(), net.state_dict()
    assert list(esd) == list(sd)
    views = dict(zip([n for n, p in net.named_parameters() if p.requires_grad], tr.optimizer.ema_views()))
    assert 0 < len(views) < len(list(net.parameters())) < len(sd)
    for k in sd:
        assert esd[k].shape == sd[k].shape and esd[k].dtype == sd[k].dtype
        assert torch.equal(esd[k], views[k] if k in views else sd[k]), k
        assert k not in views or esd[k].data_ptr() != views[k].data_ptr()       # a clone, not a view of the buffer
    assert sum(not torch.equal(esd[k], sd[k]) for k in views) > len(views) // 2
    net.eval()
    with torch.no_grad():
        with tr.ema_scope():
            y_ema = net(x).clone()
            inside = tr.ema_state_dict()             # inside the scope it is still the average
            for call in (tr.step, tr.fwd_bwd, tr.capture):           # no gradients of, and no graph on, the average
                with pytest.raises(RuntimeError, match="averaged"):
                    call(x, _batches(1)[0][1])
            assert tr.graph is None and tr._static is None
        y_live = net(x).clone()
        assert all(torch.equal(inside[k], esd[k]) for k in esd)
        assert torch.equal(y_ema, _fresh(mode, esd)(x))
        assert torch.equal(y_live, _fresh(mode, sd)(x))
    assert not torch.equal(y_ema, y_live)            # a swap that does nothing would pass everything above
    # quick_eva: the averaged weights by default, the live ones on request
    net.train()
    lr, hr = _validation_set(n=4, h=16, w=16)
    rep = {u: tr.quick_eva(lr, hr, num_samples=4, generator=torch.Generator().manual_seed(1), use_ema=u)
           for u in (None, True, False)}
    assert rep[None] == rep[True] and rep[True] != rep[False]
    plain = DPTrainStep(_fresh(mode, sd).train(), lr=1e-2)
    assert plain.quick_eva(lr, hr, num_samples=4, generator=torch.Generator().manual_seed(1)) == rep[False]
    with pytest.raises(RuntimeError):
        plain.quick_eva(lr, hr, num_samples=4, use_ema=True)


# ---- 9. the tester's graph survives ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_tester_graph_survives_the_exchange(mode):
    from rdst_amd.tester import SRTester
    from rdst_amd.trainer import DPTrainStep
    net = _tiny_rdst(mode)
    tr = DPTrainStep(net, lr=1e-2, ema_decay=0.999)
    for x, t in _batches(3):
        tr.step(x, t)
    slices = torch.rand(4, 1, 24, 24, generator=torch.Generator().manual_seed(9)).to(DEV)    # 9 tiles each: 4 full batches + 4
    kw = dict(tile=16, tile_stride=8, tile_batch=8)
    tester = SRTester(net, graph=True, **kw)
    live = tester.inference(slices).clone()          # captured on the live weights
    assert tester.graph_captures == 1 and tester.graph is not None
    replays = tester.graph_replays
    assert replays > 0
    assert torch.equal(live, SRTester(_fresh(mode, net.state_dict()), **kw).inference(slices))
    want = SRTester(_fresh(mode, tr.ema_state_dict()), **kw).inference(slices)
    with tr.ema_scope():
        got = tester.inference(slices).clone()
    assert torch.equal(got, want) and not torch.equal(got, live)
    assert tester.graph_captures == 1 and tester.graph_replays >= replays + 5     # every batch of the second call replayed
    assert torch.equal(tester.inference(slices), live)                             # and back on the live weights
    assert tester.graph_captures == 1
    net.train()
    tr.step(*_batches(1)[0])                         # training goes on


# ---- 10. checkpoints ---------------------------------------------------------------------------------------------------
def _linear_data(n=6):
    g = torch.Generator(device="cuda").manual_seed(1)
    return ([torch.randn(6, 7, device="cuda", generator=g) for _ in range(n)],
            [torch.randn(6, 5, device="cuda", generator=g) for _ in range(n)])


def _linear_trainer(device_guard, ema=True):
    from rdst_amd.trainer import DPTrainStep
    return DPTrainStep(_nets()[0], milestones=[2], gamma=0.5, device_guard=device_guard,
                       **(dict(ema_decay=0.3, ema_warmup=True) if ema else {}), **HYPER)


@pytest.mark.parametrize("device_guard", [False, True], ids=["host_count", "device_count"])
def test_checkpoint_resumes_the_ema_bitwise(tmp_path, device_guard):
    xs, ys = _linear_data()
    tr = _linear_trainer(device_guard)
    for i in range(3):
        tr.step(xs[i], ys[i])
    path = str(tmp_path / "checkpoint.tar")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=False)
    assert ck["ema"] == {"decay": 0.3, "warmup": True}      # (1 + t) / (10 + t) crosses 0.3 at t = 3: both branches run
    assert list(ck["model_g_ema"]) == list(ck["model_g"])
    assert not all(torch.equal(ck["model_g_ema"][k], ck["model_g"][k]) for k in ck["model_g"])
    tr2 = _linear_trainer(device_guard)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.optimizer.ema, tr.optimizer.ema) and torch.equal(tr2.optimizer.flat_param, tr.optimizer.flat_param)
    for i in range(3, 6):
        tr.step(xs[i], ys[i])
        tr2.step(xs[i], ys[i])
    assert torch.equal(tr.optimizer.flat_param, tr2.optimizer.flat_param)
    assert torch.equal(tr.optimizer.ema, tr2.optimizer.ema)
    assert not torch.equal(tr.optimizer.ema, tr.optimizer.flat_param)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_checkpoint_resumes_the_ema_bitwise_on_the_network(tmp_path, mode):
    """The same on the tiny RDSTSR, through torch.save: frozen parameters (the bias tables) and buffers sit between the
    trainable entries of ``model_g_ema``, which ``_load_ema`` must step over.  (The two tests around this one use the small
    linear network of tests/test_optim_gpu.py: they are about which keys are written and read, on both step counts.)"""
    from rdst_amd.trainer import DPTrainStep
    kw = dict(lr=1e-3, device_guard=True, ema_decay=0.3, ema_warmup=True)
    data = _batches()
    tr = DPTrainStep(_tiny_rdst_fixed_tables(mode), **kw)
    for x, t in data[:3]:
        tr.step(x, t)
    path = str(tmp_path / "checkpoint.tar")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=False)
    assert list(ck["model_g_ema"]) == list(ck["model_g"]) == list(tr.net.state_dict())
    trainable = {n for n, p in tr.net.named_parameters() if p.requires_grad}
    assert 0 < len(trainable) < len(ck["model_g"])
    for k, v in ck["model_g"].items():
        if k not in trainable:
            assert torch.equal(ck["model_g_ema"][k], v), k
    assert any(not torch.equal(ck["model_g_ema"][k], ck["model_g"][k]) for k in trainable)
    _fresh(mode, ck["model_g_ema"])                                  # loads strictly into a plain network
    tr2 = DPTrainStep(_tiny_rdst_fixed_tables(mode), **kw)
    tr2.optimizer.ema.fill_(7.0)                                     # every trainable entry must come from the checkpoint
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.optimizer.ema, tr.optimizer.ema) and torch.equal(tr2.optimizer.flat_param, tr.optimizer.flat_param)
    for x, t in data[3:]:
        tr.step(x, t)
        tr2.step(x, t)
    assert tr.guard_stats()["kept"] == tr2.guard_stats()["kept"] == 6
    assert torch.equal(tr.optimizer.flat_param, tr2.optimizer.flat_param)
    assert torch.equal(tr.optimizer.ema, tr2.optimizer.ema)
    assert not torch.equal(tr.optimizer.ema, tr.optimizer.flat_param)


def test_checkpoints_cross_load_with_and_without_ema():
    xs, ys = _linear_data()
    with_ema, without = _linear_trainer(True), _linear_trainer(True, ema=False)
    for i in range(3):
        with_ema.step(xs[i], ys[i])
        without.step(xs[i], ys[i])
    ck_ema, ck_plain = with_ema.checkpoint(), without.checkpoint()
    assert set(ck_ema) - set(ck_plain) == {"model_g_ema", "ema"} and set(ck_plain) <= set(ck_ema)
    # an EMA checkpoint into a trainer without one: the keys are ignored
    dst = _linear_trainer(True, ema=False)
    dst.load_checkpoint(ck_ema)
    assert torch.equal(dst.optimizer.flat_param, with_ema.optimizer.flat_param) and dst.optimizer.ema is None
    dst.step(xs[3], ys[3])
    # a checkpoint without the key into an EMA trainer: the average restarts from the loaded parameters
    dst = _linear_trainer(True)
    dst.step(xs[4], ys[4])                           # its own average has moved away from its parameters by now
    dst.load_checkpoint(ck_plain)
    assert torch.equal(dst.optimizer.flat_param, without.optimizer.flat_param)
    assert torch.equal(dst.optimizer.ema, dst.optimizer.flat_param)
    dst.step(xs[3], ys[3])
    assert not torch.equal(dst.optimizer.ema, dst.optimizer.flat_param)
