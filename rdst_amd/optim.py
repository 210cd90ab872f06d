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

``FlatAdam(ema_decay=d)`` keeps an exponential moving average of the parameters (BasicSR / SwinIR: 0.999) in one more flat
fp32 buffer, updated INSIDE the same launch (``rdst_adam_step_ema`` / ``rdst_adam_step_dev_ema``) while the new parameter
is in registers: ``e += (p_new - e) * (1 - d_t)``.  ``swap_ema()`` / ``ema_scope()`` exchange the two buffers in place
(``rdst_swap_f32``) for evaluation: no address moves, so pack plans and captured graphs stay valid.  The reference keeps no
EMA; it is off by default and no PSNR gain is claimed for it here.
"""
from __future__ import annotations

import bisect
import contextlib
import ctypes as C
import math
from typing import Iterable, Optional, Sequence

import torch

from . import _lib
from .dp import FlatGradBucket, flat_views

_TORCH_DTYPE = {C.c_int64: torch.int64, C.c_int32: torch.int32, C.c_float: torch.float32, C.c_double: torch.float64}


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


def ema_decay_at(t: int, decay: float, warmup: bool = False) -> float:
    """The EMA decay of update ``t`` (1-based count of APPLIED updates) in double, as the kernels derive it
    (include/rdst_hip.h): ``decay``, or with ``warmup`` ``min(decay, (1 + t) / (10 + t))``."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(t)) / (10.0 + float(t)))
    return d


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-4, betas=(0.9, 0.99), eps: float = 1e-8,
                 weight_decay: float = 0.0, bucket: Optional[FlatGradBucket] = None, device_state: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        params = [p for p in params if p.requires_grad]
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"FlatAdam: ema_decay {ema_decay} is not in [0, 1)")
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
        with torch.no_grad():
            for p, view in zip(params, flat_views(self.flat_param, params)):
                view.copy_(p.data)
                p.data = view  # the module now computes from the flat buffer
        # the weight EMA: one more flat buffer, a copy of the parameters as they are now; nothing without ema_decay
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema_active = False                    # True while flat_param holds the averaged weights (swap_ema)
        self.ema = self.flat_param.clone() if self.ema_decay is not None else None
        self._point_state()

    def _need_gpu(self, where: str, what: str) -> None:
        if not self.flat_param.is_cuda:
            raise RuntimeError(f"rdst_amd.optim.FlatAdam.{where}: the {what} is a HIP kernel; there is no CPU fallback")

    def _point_state(self) -> None:
        # ONE host-side step counter shared by all 750 per-parameter states (torch.optim.Adam's layout wants a
        # "step" entry per parameter; they are always equal here): a step() updates it once, not 750 times
        self._step_t = torch.tensor(float(self._steps))
        params = self.param_groups[0]["params"]
        for p, m, v in zip(params, flat_views(self.exp_avg, params), flat_views(self.exp_avg_sq, params)):
            self.state[p] = {"step": self._step_t, "exp_avg": m, "exp_avg_sq": v}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._need_gpu("step", "fused update")
        if self.ema_active:
            raise RuntimeError("FlatAdam.step: the parameters hold the averaged weights (swap_ema / ema_scope is active); "
                               "the network must not train on them")
        if not self.bucket.check_views():
            raise RuntimeError("FlatAdam.step: p.grad no longer aliases the gradient bucket "
                               "(use bucket.zero() / bucket.detach_grads()+gather(), not zero_grad(set_to_none=True))")
        g = self.param_groups[0]
        lib = _lib.load()
        ema = self.ema is not None      # the *_ema entry points: the buffer right behind the moments, decay and warmup last
        bufs = [self.flat_param.data_ptr(), self.bucket.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()]
        if ema:
            bufs.append(self.ema.data_ptr())
        hyper = [float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])]
        ema_args = [self.ema_decay, int(self.ema_warmup)] if ema else []
        n, stream = self.flat_param.numel(), torch.cuda.current_stream().cuda_stream
        # the four entry points differ in where rate and count come from: (lr, ..., step) from the host, or (schedule, ..., state)
        if self.device_state:
            if not self._guard_pending:     # no guard() before this step: it is kept
                self.guard(None, 0.0)
            self._guard_pending = False
            rate, count = self._c_schedule(), [*ema_args, self._dev_state.data_ptr()]
        else:
            self._steps += 1
            rate, count = float(g["lr"]), [self._steps, *ema_args]
        name = "rdst_adam_step" + ("_dev" if self.device_state else "") + ("_ema" if ema else "")
        _lib.check(getattr(lib, name)(*bufs, n, rate, *hyper, *count, stream), name)
        if not self.device_state:
            self._step_t.fill_(float(self._steps))
        return loss

    def zero_grad(self, set_to_none: bool = False) -> None:  # noqa: D401 - keeps p.grad aliased to the bucket
        self.bucket.zero()

    # ---- the weight EMA (ema_decay=...) ------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if self.ema is None:
            raise RuntimeError(f"FlatAdam.{what}: needs FlatAdam(ema_decay=...)")

    @torch.no_grad()
    def reset_ema(self) -> None:
        """``ema <- flat_param`` (the state a fresh optimizer has); refused while the two are exchanged."""
        self._need_ema("reset_ema")
        if self.ema_active:
            raise RuntimeError("FlatAdam.reset_ema: swap_ema / ema_scope is active")
        self.ema.copy_(self.flat_param)

    @torch.no_grad()
    def swap_ema(self) -> None:
        """Exchange ``flat_param`` and ``ema`` in place (ONE ``rdst_swap_f32``) and toggle ``ema_active``.  Every parameter
        of the network is a view of ``flat_param``, so the network computes from the averaged weights until the next call;
        no address moves, so pack plans and captured graphs (whose pack refresh is one of their nodes) stay valid."""
        self._need_ema("swap_ema")
        self._need_gpu("swap_ema", "exchange")
        _lib.check(_lib.load().rdst_swap_f32(self.flat_param.data_ptr(), self.ema.data_ptr(), self.flat_param.numel(),
                                             torch.cuda.current_stream().cuda_stream), "rdst_swap_f32")
        self.ema_active = not self.ema_active

    @contextlib.contextmanager
    def ema_scope(self):
        """``with opt.ema_scope():`` the network holds the averaged weights inside; swapped back on exit, also when the body
        raises.  ``step()`` and ``guard()`` raise inside."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_views(self) -> list:
        """Per-parameter views of ``ema``, in parameter order.  Inside ``ema_scope()`` the buffers are exchanged: these
        views then show the live weights and the parameters the averaged ones."""
        self._need_ema("ema_views")
        return list(flat_views(self.ema, self.param_groups[0]["params"]))

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
        if self.ema_active:
            raise RuntimeError("FlatAdam.guard: the parameters hold the averaged weights (swap_ema / ema_scope is active)")
        self._need_gpu("guard", "guard")
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
        st = self.host_state()
        kept, sumsq = st.kept, st.last_sumsq
        self._steps = kept
        self._step_t.fill_(float(kept))
        if self._lr_table is not None:
            fields = scheduler_fields(kept, self._lr_table, self._milestones)
            self.param_groups[0]["lr"] = fields["_last_lr"][0]
            if self.scheduler is not None:
                for k, v in fields.items():
                    setattr(self.scheduler, k, v)
        return {"kept": kept, "skipped": st.skipped, "last_keep": st.last_keep, "last_reason": st.last_reason,
                "last_grad_norm": None if sumsq == -1.0 else math.sqrt(sumsq) if sumsq < math.inf else sumsq,
                "last_clip": st.last_clip, "last_lr": st.last_lr}

    def host_state(self) -> "_lib.StepState":
        """A host copy of the rdst_step_state, read by field name (one device-to-host copy)."""
        self._need_device_state("host_state")
        return _lib.StepState.from_buffer_copy(self._dev_state.cpu().numpy().tobytes())

    def state_field(self, name: str) -> torch.Tensor:
        """The 0-dim view of one field of the rdst_step_state where it lives (no copy, nothing read back)."""
        self._need_device_state("state_field")
        f = getattr(_lib.StepState, name)
        dtype = _TORCH_DTYPE[dict(_lib.StepState._fields_)[name]]
        return self._dev_state.view(torch.uint8)[f.offset:f.offset + f.size].view(dtype)[0]

    def _push_state(self, kept: int) -> None:
        st = _lib.StepState(kept=int(kept), last_keep=1, last_clip=1.0, last_sumsq=-1.0)     # the rest 0
        self._dev_state.copy_(torch.frombuffer(bytearray(st), dtype=torch.int64))
        self._guard_pending = False

    def state_dict(self):
        """torch.optim.Adam's layout.  The EMA is NOT in it, so reference checkpoints cross-load (the trainer saves it
        under a key of its own)."""
        if self.device_state:
            self.sync_host()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        """Accepts a torch.optim.Adam state dict (same layout as ours) and re-flattens it."""
        super().load_state_dict(state_dict)
        steps = 0
        params = self.param_groups[0]["params"]
        with torch.no_grad():
            for p, m, v in zip(params, flat_views(self.exp_avg, params), flat_views(self.exp_avg_sq, params)):
                st = self.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"].reshape(m.shape))
                    v.copy_(st["exp_avg_sq"].reshape(v.shape))
                    steps = max(steps, int(float(st["step"])))
                else:
                    m.zero_()
                    v.zero_()
        self._steps = steps
        self._point_state()
        if self.device_state:
            self._push_state(steps)
