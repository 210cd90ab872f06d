"""CPU: the host side of the weight EMA (FlatAdam(ema_decay=...), DPTrainStep(ema_decay=...)) - the argument checks of the
three C entry points (every check returns before a launch, so they answer without a device), the decay rule in double, the
constructor checks, the buffer a CPU network gets, and the checkpoint's key sets.  Nothing here launches a kernel."""
import ctypes

import pytest
import torch


def _params():
    torch.manual_seed(0)
    return list(torch.nn.Linear(3, 2).parameters())


def _lib_and_buffers():
    from rdst_amd import _lib
    lib = _lib.load()
    raw = (ctypes.c_float * 128)()                  # host memory: a refused call never reads it
    base = (ctypes.addressof(raw) + 15) & ~15
    return _lib, lib, [base + 64 * i for i in range(4)] + [base + 256]


def _sched(_lib, count=0, milestones=()):
    s = _lib.LrSchedule()
    s.lr[0] = 1e-3
    s.count = count
    for i, m in enumerate(milestones):
        s.milestones[i] = m
    return s


def test_adam_step_ema_refuses_bad_arguments():
    _lib, lib, (p, g, m, v, e) = _lib_and_buffers()

    def call(p=p, g=g, m=m, v=v, e=e, n=8, step=1, decay=0.999):
        return lib.rdst_adam_step_ema(p, g, m, v, e, n, 1e-3, 0.9, 0.99, 1e-8, 0.0, step, decay, 0, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(e=None), dict(n=-1), dict(step=0),
               dict(p=p + 4), dict(g=g + 4), dict(m=m + 8), dict(v=v + 4), dict(e=e + 4), dict(e=e + 8),
               dict(decay=1.0), dict(decay=-1e-9), dict(decay=1.5), dict(decay=float("nan"))):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"rdst_adam_step_ema" in lib.rdst_last_error()
    assert call(n=0) == 0 and call(n=0, decay=0.0) == 0       # valid arguments, nothing to do: no launch either


def test_adam_step_dev_ema_refuses_bad_arguments():
    _lib, lib, (p, g, m, v, e) = _lib_and_buffers()
    st = e + 64

    def call(p=p, g=g, m=m, v=v, e=e, n=8, decay=0.999, st=st, sched=None):
        return lib.rdst_adam_step_dev_ema(p, g, m, v, e, n, sched if sched is not None else _sched(_lib), 0.9, 0.99, 1e-8,
                                          0.0, decay, 1, st, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(e=None), dict(st=None), dict(n=-1),
               dict(p=p + 4), dict(g=g + 8), dict(m=m + 4), dict(v=v + 4), dict(e=e + 4), dict(st=st + 8),
               dict(decay=1.0), dict(decay=-0.5), dict(decay=float("nan")),
               dict(sched=_sched(_lib, 17)), dict(sched=_sched(_lib, -1)), dict(sched=_sched(_lib, 2, (5, 3)))):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"rdst_adam_step_dev_ema" in lib.rdst_last_error()
    assert call(n=0) == 0


def test_swap_refuses_bad_arguments():
    _lib, lib, (a, b, *_rest) = _lib_and_buffers()
    for args in ((None, b, 8), (a, None, 8), (a + 4, b, 8), (a, b + 8, 8), (a, b, -1),
                 (a, a, 8), (a, a + 16, 8), (a + 16, a, 5), (a, b, 17)):      # b = a + 64 bytes: 17 floats overlap
        assert lib.rdst_swap_f32(*args, None) == _lib.EINVAL, args
        assert b"rdst_swap_f32" in lib.rdst_last_error()
    assert lib.rdst_swap_f32(a, b, 0, None) == 0
    assert lib.rdst_abi_version() == _lib.ABI_VERSION == 11                   # additive entry points: the version stays
    assert _lib.STEP_STATE_BYTES == 48


@pytest.mark.parametrize("t", [1, 2, 10, 10 ** 6])
def test_decay_rule_is_the_closed_form(t):
    from rdst_amd.optim import ema_decay_at
    for decay in (0.999, 0.5, 0.0):
        assert ema_decay_at(t, decay, False) == decay
        assert ema_decay_at(t, decay) == decay
        assert ema_decay_at(t, decay, True) == min(decay, (1.0 + t) / (10.0 + t))
    # the values themselves: 2/11, 3/12 and 11/20 are below 0.999, (1 + 10^6) / (10 + 10^6) is above it
    want = {1: 2.0 / 11.0, 2: 0.25, 10: 0.55, 10 ** 6: 0.999}[t]
    assert ema_decay_at(t, 0.999, True) == want


@pytest.mark.parametrize("decay", [1.0, -0.1, 1.5, float("nan")])
def test_decay_outside_the_unit_interval_is_refused(decay):
    from rdst_amd.optim import FlatAdam
    from rdst_amd.trainer import DPTrainStep
    with pytest.raises(ValueError):
        FlatAdam(_params(), ema_decay=decay)
    with pytest.raises(ValueError):
        DPTrainStep(torch.nn.Linear(3, 2), ema_decay=decay)


@pytest.mark.parametrize("device_state", [False, True])
def test_cpu_network_gets_the_buffer_but_no_kernel(device_state):
    from rdst_amd.optim import FlatAdam
    params = _params()
    opt = FlatAdam(params, ema_decay=0.999, ema_warmup=True, device_state=device_state)
    assert opt.ema.dtype == torch.float32 and opt.ema.shape == opt.flat_param.shape
    assert torch.equal(opt.ema, opt.flat_param) and opt.ema.data_ptr() != opt.flat_param.data_ptr()
    assert (opt.ema_decay, opt.ema_warmup, opt.ema_active) == (0.999, True, False)
    views = opt.ema_views()
    assert [v.shape for v in views] == [p.shape for p in params]
    assert all(torch.equal(v, p) for v, p in zip(views, params))
    assert views[1].data_ptr() == opt.ema.data_ptr() + 4 * params[0].numel()
    with torch.no_grad():
        params[0].add_(1.0)
    assert not torch.equal(opt.ema, opt.flat_param)
    opt.reset_ema()
    assert torch.equal(opt.ema, opt.flat_param)
    opt.zero_grad()
    for p in params:
        p.grad.fill_(0.5)
    for call in (opt.step, opt.swap_ema):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with opt.ema_scope():
            pass
    assert opt.ema_active is False
    sd = opt.state_dict()                                     # torch.optim.Adam's layout: the EMA is not part of it
    assert set(sd) == {"state", "param_groups"} and not any("ema" in k for k in sd["param_groups"][0])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())


def test_without_a_decay_nothing_is_allocated():
    from rdst_amd.optim import FlatAdam
    opt = FlatAdam(_params())
    assert opt.ema is None and opt.ema_decay is None and opt.ema_active is False
    for call in (opt.reset_ema, opt.swap_ema, opt.ema_views):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()


def _bn_net():
    """Trainable parameters next to a frozen one and BatchNorm's buffers."""
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2), torch.nn.Linear(2, 2))
    net[2].bias.requires_grad_(False)
    return net


def test_checkpoint_key_sets():
    from rdst_amd.trainer import DPTrainStep
    plain = DPTrainStep(torch.nn.Linear(3, 2), milestones=[2])
    base = {"Time", "model_g", "optimizer_g", "loss", "training_loss_names", "training_loss_records",
            "quick_validation_reports", "current_training_state_id", "current_epoch", "training_epoch_costs", "scheduler_g"}
    assert set(plain.checkpoint()) == base and not plain.ema_enabled
    with pytest.raises(RuntimeError):
        plain.ema_state_dict()
    with pytest.raises(RuntimeError):
        plain.quick_eva(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8), use_ema=True)
    net = _bn_net()
    tr = DPTrainStep(net, milestones=[2], ema_decay=0.5, ema_warmup=True)
    ck = tr.checkpoint()
    assert set(ck) == base | {"model_g_ema", "ema"} and tr.ema_enabled
    assert ck["ema"] == {"decay": 0.5, "warmup": True}
    assert list(ck["model_g_ema"]) == list(net.state_dict())
    with torch.no_grad():
        tr.optimizer.ema.add_(1.0)
    esd, sd = tr.ema_state_dict(), net.state_dict()
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    assert trainable == {"0.weight", "0.bias", "1.weight", "1.bias", "2.weight"}
    for k, v in sd.items():
        assert torch.equal(esd[k], v + 1.0 if k in trainable else v), k
        assert esd[k].data_ptr() != tr.optimizer.ema.data_ptr()
    fresh = _bn_net()
    fresh.load_state_dict(esd, strict=True)
    # the loads: a checkpoint with the key into a trainer without an EMA (ignored), and the other two ways round
    plain2 = DPTrainStep(_bn_net(), milestones=[2])
    plain2.load_checkpoint(tr.checkpoint())
    assert torch.equal(plain2.net[0].weight, net[0].weight) and not plain2.ema_enabled
    tr2 = DPTrainStep(_bn_net(), milestones=[2], ema_decay=0.5)
    tr2.load_checkpoint(tr.checkpoint())
    assert torch.equal(tr2.net[0].weight, net[0].weight)
    got = tr2.ema_state_dict()
    assert all(torch.equal(got[k], esd[k]) for k in esd)
    no_ema = {k: v for k, v in tr.checkpoint().items() if k not in ("model_g_ema", "ema")}
    tr2.load_checkpoint(no_ema)
    assert torch.equal(tr2.optimizer.ema, tr2.optimizer.flat_param)
