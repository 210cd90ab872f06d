"""Fused Adam for the data-parallel training step.

``FlatAdam`` is a ``torch.optim.Optimizer`` with torch.optim.Adam's update rule — the optimizer the
reference builds in utils/optim.py:30-53 (Adam, betas (0.9, 0.99), eps 1e-8, lr 1e-4, weight_decay 0;
config_files/RDST_E1_OASIS_example_SRx4.ini:128-135) and steps in models/trans_sr_trainer.py:170-173 —
but parameters, gradients and both moments each live in ONE contiguous fp32 buffer and a step is ONE
HIP launch (``rdst_adam_step``) instead of a multi-tensor sweep per moment plus per-parameter
bookkeeping kernels.  Being an ``Optimizer`` it works with ``torch.optim.lr_scheduler`` (the
reference's MultiStepLR, utils/optim.py:56-75) and its ``state_dict()`` has torch.optim.Adam's layout,
so the optimizer part of a reference ``checkpoint.tar`` (models/basic_trainer.py:187-208) loads.

``FlatAdam(device_state=True)`` keeps the step count, the MultiStepLR rate and the keep / skip decision of the
reference's update guard (models/trans_sr_trainer.py:162-174) in device memory (``rdst_step_guard`` +
``rdst_adam_step_dev``, include/rdst_hip.h): ``guard()`` and ``step()`` enqueue launches whose arguments never change,
so both are graph-capturable, and nothing is read back until ``sync_host()``.
"""
from __future__ import annotations

import bisect
import math
from typing import Iterable, Optional, Sequence

import torch

from . import _lib
from .dp import FlatGradBucket


def multistep_table(base_lr: float, milestones: Sequence[int], gamma: float) -> list:
    """The rates of torch's MultiStepLR (utils/optim.py:56-75) as a table: entry k is the rate once k of the (sorted,
    possibly repeated) milestones have passed.  Multiplied up in double precision the way MultiStepLR.get_lr does it,
    ``lr * gamma ** multiplicity`` once per DISTINCT milestone, so every entry a run can reach holds the bits of the
    scheduler's ``_last_lr`` (an entry inside a run of equal milestones is never reached)."""
    ms = sorted(int(m) for m in milestones)
    table = [float(base_lr)]
    i = 0
    while i < len(ms):
        mult = ms.count(ms[i])
        for j in range(1, mult):
            table.append(table[i] * gamma ** j)
        table.append(table[i] * gamma ** mult)
        i += mult
    return table


def scheduler_fields(kept: int, table: Sequence[float], milestones: Sequence[int]) -> dict:
    """What a torch MultiStepLR stepped ``kept`` times holds (``table`` from multistep_table, ``milestones`` sorted)."""
    return {"last_epoch": int(kept), "_step_count": int(kept) + 1,
            "_last_lr": [table[bisect.bisect_right(list(milestones), int(kept))]]}


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-4, betas=(0.9, 0.99), eps: float = 1e-8,
                 weight_decay: float = 0.0, bucket: Optional[FlatGradBucket] = None, device_state: bool = False):
        params = [p for p in params if p.requires_grad]
        if bucket is not None and [id(p) for p in bucket.params] != [id(p) for p in params]:
            raise ValueError("FlatAdam: the gradient bucket must hold exactly these parameters, in this order")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdam: one parameter group only")
        self.bucket = bucket if bucket is not None else FlatGradBucket(params)
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self.flat_param = torch.empty(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self._steps = 0
        # device-resident step state (rdst_step_state) and the sum-of-squares workspace: allocated once, only on request
        self.device_state = bool(device_state)
        self._dev_state = None
        self._workspace = None
        self._milestones: list = []
        self._lr_table: Optional[list] = None      # doubles; None = no schedule, the rate is param_groups[0]["lr"]
        self._guard_pending = False
        self.scheduler = None                      # a MultiStepLR that sync_host() keeps in step (attach_scheduler)
        if self.device_state:
            self._dev_state = torch.zeros(_lib.STEP_STATE_BYTES // 8, dtype=torch.int64, device=dev)
            nbytes = int(_lib.load().rdst_step_guard_workspace(n)) if dev.type == "cuda" else 0
            self._workspace = torch.empty(max(nbytes, 16) // 8, dtype=torch.float64, device=dev)
            self._push_state(0)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                self.flat_param[off:off + k].copy_(p.data.reshape(-1))
                p.data = self.flat_param[off:off + k].view_as(p)  # the module now computes from the flat buffer
                off += k
        self._point_state()

    def _point_state(self) -> None:
        # ONE host-side step counter shared by all 750 per-parameter states (torch.optim.Adam's layout wants a
        # "step" entry per parameter; they are always equal here): a step() updates it once, not 750 times
        self._step_t = torch.tensor(float(self._steps))
        off = 0
        for p in self.param_groups[0]["params"]:
            k = p.numel()
            self.state[p] = {"step": self._step_t,
                             "exp_avg": self.exp_avg[off:off + k].view_as(p),
                             "exp_avg_sq": self.exp_avg_sq[off:off + k].view_as(p)}
            off += k

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self.flat_param.is_cuda:
            raise RuntimeError("rdst_amd.optim.FlatAdam.step: the fused update is a HIP kernel; there is no CPU fallback")
        if not self.bucket.check_views():
            raise RuntimeError("FlatAdam.step: p.grad no longer aliases the gradient bucket "
                               "(use bucket.zero() / bucket.detach_grads()+gather(), not zero_grad(set_to_none=True))")
        g = self.param_groups[0]
        lib = _lib.load()
        if self.device_state:
            if not self._guard_pending:     # no guard() before this step: it is kept
                self.guard(None, 0.0)
            self._guard_pending = False
            _lib.check(lib.rdst_adam_step_dev(self.flat_param.data_ptr(), self.bucket.flat.data_ptr(),
                                              self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.flat_param.numel(),
                                              self._c_schedule(), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                              float(g["weight_decay"]), self._dev_state.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "rdst_adam_step_dev")
            return loss
        self._steps += 1
        _lib.check(lib.rdst_adam_step(self.flat_param.data_ptr(), self.bucket.flat.data_ptr(), self.exp_avg.data_ptr(),
                                      self.exp_avg_sq.data_ptr(), self.flat_param.numel(), float(g["lr"]),
                                      float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                      float(g["weight_decay"]), self._steps,
                                      torch.cuda.current_stream().cuda_stream), "rdst_adam_step")
        self._step_t.fill_(float(self._steps))
        return loss

    def zero_grad(self, set_to_none: bool = False) -> None:  # noqa: D401 - keeps p.grad aliased to the bucket
        self.bucket.zero()

    # ---- device-resident step state (device_state=True) ------------------------------------------------------------
    def _need_device_state(self, what: str) -> None:
        if not self.device_state:
            raise RuntimeError(f"FlatAdam.{what}: needs FlatAdam(device_state=True)")

    def set_schedule(self, milestones: Sequence[int], gamma: float, base_lr: Optional[float] = None) -> None:
        """The MultiStepLR of utils/optim.py:56-75 as the rate table ``rdst_adam_step_dev`` indexes with the number of
        milestones <= kept - 1.  ``lr_table`` is that table after the cast ``step()`` applies to ``g["lr"]`` (fp32)."""
        self._need_device_state("set_schedule")
        ms = sorted(int(m) for m in milestones)
        if len(ms) > _lib.LrSchedule.MAX_MILESTONES:
            raise ValueError(f"FlatAdam.set_schedule: {len(ms)} milestones, the device table holds "
                             f"{_lib.LrSchedule.MAX_MILESTONES}")
        g = self.param_groups[0]
        base = float(base_lr if base_lr is not None else g.get("initial_lr", g["lr"]))
        self._milestones = ms
        self._lr_table = multistep_table(base, ms, float(gamma))

    @property
    def lr_table(self) -> list:
        """The fp32 rates the kernel applies, entry k once k milestones have passed."""
        t = self._lr_table if self._lr_table is not None else [float(self.param_groups[0]["lr"])]
        return torch.tensor(t, dtype=torch.float64).to(torch.float32).tolist()

    def _c_schedule(self) -> "_lib.LrSchedule":
        s = _lib.LrSchedule()
        table = self._lr_table if self._lr_table is not None else [float(self.param_groups[0]["lr"])]
        for i, m in enumerate(self._milestones if self._lr_table is not None else []):
            s.milestones[i] = m
        for i, v in enumerate(table):
            s.lr[i] = v                          # ctypes rounds the double to fp32 as it does for rdst_adam_step's lr
        s.count = len(table) - 1
        return s

    def attach_scheduler(self, scheduler) -> None:
        """``scheduler``: the MultiStepLR object a checkpoint needs; it is not stepped per step, sync_host() sets it."""
        self.scheduler = scheduler

    @torch.no_grad()
    def guard(self, loss: Optional[torch.Tensor], threshold: float, max_grad_norm: Optional[float] = None,
              skip_nonfinite: bool = False, peer_skip: Optional[torch.Tensor] = None) -> None:
        """Enqueue the decision for the next ``step()`` (``rdst_step_guard``): keep when ``loss < threshold`` (a device
        fp32 scalar; None = no loss test), no rank asked to skip (``peer_skip``: device int32) and, with
        ``skip_nonfinite``, the gradient bucket is finite; ``max_grad_norm`` sets the clip coefficient the step applies.
        Call it once the bucket holds the (averaged) gradient."""
        self._need_device_state("guard")
        if not self.flat_param.is_cuda:
            raise RuntimeError("rdst_amd.optim.FlatAdam.guard: the guard is a HIP kernel; there is no CPU fallback")
        if loss is not None and (loss.dtype != torch.float32 or loss.device != self.flat_param.device or loss.numel() != 1):
            raise ValueError("FlatAdam.guard: loss must be one fp32 element on the optimizer's device")
        if peer_skip is not None and (peer_skip.dtype != torch.int32 or peer_skip.device != self.flat_param.device
                                      or peer_skip.numel() != 1):
            raise ValueError("FlatAdam.guard: peer_skip must be one int32 element on the optimizer's device")
        mx = float(max_grad_norm) if max_grad_norm is not None else 0.0
        _lib.check(_lib.load().rdst_step_guard(loss.data_ptr() if loss is not None else None, float(threshold),
                                               peer_skip.data_ptr() if peer_skip is not None else None,
                                               self.bucket.flat.data_ptr(), self.bucket.flat.numel(), mx,
                                               int(bool(skip_nonfinite)), self._workspace.data_ptr(),
                                               self._workspace.numel() * 8, self._dev_state.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "rdst_step_guard")
        self._guard_pending = True

    def sync_host(self) -> dict:
        """The ONE place that reads the step state back (one copy): brings ``_steps``, the shared "step" tensor,
        ``param_groups[0]["lr"]`` and an attached scheduler to where ``kept`` applied updates leave them."""
        self._need_device_state("sync_host")
        h = self._dev_state.cpu()
        i32, f32, f64 = h.view(torch.int32), h.view(torch.float32), h.view(torch.float64)
        kept, sumsq = int(h[0]), float(f64[4])
        self._steps = kept
        self._step_t.fill_(float(kept))
        if self._lr_table is not None:
            fields = scheduler_fields(kept, self._lr_table, self._milestones)
            self.param_groups[0]["lr"] = fields["_last_lr"][0]
            if self.scheduler is not None:
                for k, v in fields.items():
                    setattr(self.scheduler, k, v)
        return {"kept": kept, "skipped": int(h[1]), "last_keep": int(i32[4]), "last_reason": int(i32[5]),
                "last_grad_norm": None if sumsq == -1.0 else math.sqrt(sumsq) if sumsq < math.inf else sumsq,
                "last_clip": float(f32[6]), "last_lr": float(f32[7])}

    def _push_state(self, kept: int) -> None:
        h = torch.zeros(_lib.STEP_STATE_BYTES // 8, dtype=torch.int64)
        h[0] = int(kept)
        h.view(torch.int32)[4] = 1
        h.view(torch.float32)[6] = 1.0
        h.view(torch.float64)[4] = -1.0
        self._dev_state.copy_(h)
        self._guard_pending = False

    def state_dict(self):
        if self.device_state:
            self.sync_host()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        """Accepts a torch.optim.Adam state dict (same layout as ours) and re-flattens it."""
        super().load_state_dict(state_dict)
        off = 0
        steps = 0
        with torch.no_grad():
            for p in self.param_groups[0]["params"]:
                k = p.numel()
                st = self.state.get(p, {})
                if "exp_avg" in st:
                    self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                    steps = max(steps, int(float(st["step"])))
                else:
                    self.exp_avg[off:off + k].zero_()
                    self.exp_avg_sq[off:off + k].zero_()
                off += k
        self._steps = steps
        self._point_state()
        if self.device_state:
            self._push_state(steps)
