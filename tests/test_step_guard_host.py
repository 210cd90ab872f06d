"""CPU: the host side of the device step guard (FlatAdam(device_state=True), DPTrainStep(device_guard=True)) - the
MultiStepLR rate table the kernel indexes, the scheduler fields sync_host() writes, the record filter of
_flush_records and the constructor checks.  Nothing here launches a kernel."""
import copy

import numpy as np
import pytest
import torch


def _params():
    torch.manual_seed(0)
    return list(torch.nn.Linear(3, 2).parameters())


def _torch_last_lrs(base, milestones, gamma, epochs):
    """_last_lr of a torch MultiStepLR (utils/optim.py:56-75) after 0, 1, ..., epochs scheduler steps."""
    opt = torch.optim.Adam(_params(), lr=base)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(milestones), gamma=gamma)
    out = [sch.get_last_lr()[0]]
    for _ in range(epochs):
        opt.step()
        sch.step()
        out.append(sch.get_last_lr()[0])
    return out, sch


@pytest.mark.parametrize("gamma", [0.5, 0.3])
@pytest.mark.parametrize("milestones", [[], [1], [2, 4, 4, 9]])
def test_rate_table_matches_multisteplr(milestones, gamma):
    from rdst_amd.optim import FlatAdam
    base = 1e-3
    opt = FlatAdam(_params(), lr=base, device_state=True)
    opt.set_schedule(milestones, gamma)
    table = opt.lr_table
    assert len(table) == len(milestones) + 1
    want, _ = _torch_last_lrs(base, milestones, gamma, 12)
    for epoch, lr in enumerate(want):
        k = sum(m <= epoch for m in milestones)          # the kernel's index: milestones <= kept - 1, kept = epoch + 1
        assert np.float32(table[k]) == np.float32(lr), (epoch, k, table[k], lr)
        assert table[k] == float(np.float32(lr))
    c = opt._c_schedule()                                 # what goes to rdst_adam_step_dev by value
    assert c.count == len(milestones) and list(c.milestones)[:c.count] == sorted(milestones)
    assert [np.float32(v) for v in list(c.lr)[:c.count + 1]] == [np.float32(v) for v in table]


def test_more_than_16_milestones_are_refused():
    from rdst_amd.optim import FlatAdam
    opt = FlatAdam(_params(), lr=1e-3, device_state=True)
    opt.set_schedule(list(range(1, 17)), 0.5)
    with pytest.raises(ValueError):
        opt.set_schedule(list(range(1, 18)), 0.5)
    with pytest.raises(RuntimeError):
        FlatAdam(_params(), lr=1e-3).set_schedule([1], 0.5)       # needs device_state=True


def test_device_guard_needs_a_gpu_network():
    from rdst_amd.trainer import DPTrainStep
    net = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError):
        DPTrainStep(net, device_guard=True)
    with pytest.raises(ValueError):
        DPTrainStep(net, max_grad_norm=1.0)                        # the new options belong to the device guard
    tr = DPTrainStep(net)                                          # the defaults still build on the CPU
    assert tr.device_guard is False and tr.optimizer.device_state is False and tr.optimizer._dev_state is None


def test_record_filter_drops_skipped_steps():
    from rdst_amd.trainer import DPTrainStep
    vals = [torch.tensor(0.5), torch.tensor(9.0), 0.25, torch.tensor(float("nan")), torch.tensor(0.125)]
    keeps = [torch.tensor(1, dtype=torch.int32), torch.tensor(0, dtype=torch.int32), None,
             torch.tensor(0, dtype=torch.int32), torch.tensor(1, dtype=torch.int32)]
    assert DPTrainStep._filter_records(vals, keeps) == [0.5, 0.25, 0.125]
    assert DPTrainStep._filter_records(vals[:3], [None] * 3) == [0.5, 9.0, 0.25]      # no device guard: all kept
    assert DPTrainStep._filter_records([], []) == []
    # through _flush_records: the parked flags travel with the parked losses and both lists are emptied
    tr = DPTrainStep(torch.nn.Linear(3, 2))
    tr._pending = {"L1": list(vals)}
    tr._pending_keep = {"L1": list(keeps)}
    assert tr.loss_records()["L1"] == [0.5, 0.25, 0.125]
    assert tr._pending == {} and tr._pending_keep == {}


@pytest.mark.parametrize("kept", [0, 2, 5])
def test_sync_host_sets_the_scheduler_fields(kept):
    from rdst_amd.optim import FlatAdam
    base, milestones, gamma = 1e-3, [2, 4], 0.3
    opt = FlatAdam(_params(), lr=base, device_state=True)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=gamma)
    opt.set_schedule(milestones, gamma)
    opt.attach_scheduler(sch)
    opt._dev_state[0] = kept              # the state lives where the parameters live: here on the CPU
    opt._dev_state[1] = 3
    st = opt.sync_host()
    _, ref = _torch_last_lrs(base, milestones, gamma, kept)
    assert st["kept"] == kept and st["skipped"] == 3 and st["last_keep"] == 1 and st["last_grad_norm"] is None
    assert sch.last_epoch == ref.last_epoch == kept
    assert sch._step_count == ref._step_count
    assert sch._last_lr == pytest.approx(ref._last_lr, rel=1e-12)
    assert opt.param_groups[0]["lr"] == ref.optimizer.param_groups[0]["lr"]
    assert opt._steps == kept and float(opt.state[opt.param_groups[0]["params"][0]]["step"]) == float(kept)
    sd_a, sd_b = copy.deepcopy(sch.state_dict()), ref.state_dict()
    assert sd_a["last_epoch"] == sd_b["last_epoch"] and sd_a["_step_count"] == sd_b["_step_count"]


STATE_FORMAT = "<qqiiffdq"          # rdst_step_state as include/rdst_hip.h lays it out
STATE_FIELDS = ("kept", "skipped", "last_keep", "last_reason", "last_clip", "last_lr", "last_sumsq", "reserved")


def test_step_state_is_read_by_field_name():
    import struct
    from rdst_amd import _lib
    from rdst_amd.optim import FlatAdam
    values = (7, 3, 1, 5, 0.375, 2.5e-4, 1234.5625, -9)            # distinct, each exact in its field's type
    packed = struct.pack(STATE_FORMAT, *values)
    assert len(packed) == _lib.STEP_STATE_BYTES == 48
    opt = FlatAdam(_params(), lr=1e-3, device_state=True)
    opt._dev_state.copy_(torch.frombuffer(bytearray(packed), dtype=torch.int64))
    st = opt.host_state()
    assert tuple(getattr(st, n) for n in STATE_FIELDS) == struct.unpack(STATE_FORMAT, packed)
    assert struct.unpack(STATE_FORMAT, packed) == (7, 3, 1, 5, 0.375, float(np.float32(2.5e-4)), 1234.5625, -9)
    # the view of a field where the state lives: the same value, aliasing the state (what the trainer parks per step)
    for n, want in zip(STATE_FIELDS, struct.unpack(STATE_FORMAT, packed)):
        view = opt.state_field(n)
        assert view.dim() == 0 and view.item() == want, n
        assert view.data_ptr() == opt._dev_state.data_ptr() + getattr(_lib.StepState, n).offset
    assert opt.state_field("last_keep").dtype == torch.int32
    got = opt.sync_host()
    assert got == {"kept": 7, "skipped": 3, "last_keep": 1, "last_reason": 5, "last_grad_norm": 1234.5625 ** 0.5,
                   "last_clip": 0.375, "last_lr": float(np.float32(2.5e-4))}
    with pytest.raises(RuntimeError):
        FlatAdam(_params(), lr=1e-3).state_field("last_keep")      # needs device_state=True


@pytest.mark.parametrize("k", [0, 5, 2 ** 40 + 1])
def test_push_state_writes_exactly_these_bytes(k):
    import struct
    from rdst_amd.optim import FlatAdam
    opt = FlatAdam(_params(), lr=1e-3, device_state=True)
    opt._dev_state.fill_(-1)
    opt._guard_pending = True
    opt._push_state(k)
    assert opt._dev_state.dtype == torch.int64
    assert opt._dev_state.numpy().tobytes() == struct.pack(STATE_FORMAT, k, 0, 1, 0, 1.0, 0.0, -1.0, 0)
    assert opt._guard_pending is False


def test_flat_views_tile_the_buffer_in_order():
    from rdst_amd.dp import flat_views
    like = [torch.empty(2, 3), torch.empty(5), torch.empty(())]    # the last one is 0-dim: one element
    flat = torch.arange(12, dtype=torch.float32)
    views = list(flat_views(flat, like))
    assert [v.shape for v in views] == [t.shape for t in like]
    assert torch.equal(torch.cat([v.reshape(-1) for v in views]), flat)          # in order, nothing left over
    assert [v.data_ptr() - flat.data_ptr() for v in views] == [0, 24, 44]
    for i, v in enumerate(views):                                                # they alias the buffer
        v.fill_(-float(i + 1))
    assert flat.tolist() == [-1.0] * 6 + [-2.0] * 5 + [-3.0]
