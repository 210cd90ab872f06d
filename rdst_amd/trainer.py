"""Data-parallel training-step shell: the inner loop of the reference trainer
(models/trans_sr_trainer.py:141-173) around the HIP hot path, plus the reference's checkpoint layout.

    forward -> loss -> [loss-threshold guard] -> zero_grad -> backward -> (grad all-reduce) -> Adam -> scheduler

What changes against the reference loop is only what data parallelism and the flat buffers need:
  * gradients live in one ``FlatGradBucket`` (one RCCL all-reduce per step, rdst_amd/dp.py);
  * the optimizer is ``FlatAdam`` (one HIP launch per step, rdst_amd/optim.py) with the reference's
    hyper-parameters (utils/optim.py:30-53) and scheduler (utils/optim.py:56-75);
  * the loss-threshold guard (trans_sr_trainer.py:162, ``loss.item() < loss_threshold``) costs a host
    sync per step; it is evaluated only when the threshold is below ``GUARD_OFF`` (the shipped ini sets
    1e8, i.e. "never skip"), otherwise the step never leaves the device;
  * ``device_guard=True`` makes the same decision in device memory (rdst_step_guard, include/rdst_hip.h): the step count,
    the MultiStepLR rate and the keep / skip flag live there, so a guarded step reads nothing back and, on one rank, the
    whole step (forward, loss, backward, guard, Adam) is ONE graph replay.  The order then is the fast path's — forward,
    loss, backward, collectives, guard, Adam — so on several ranks the bucket all-reduce ALWAYS runs and its result is
    discarded on a skipped step (the host cannot branch on a flag it never reads; the host guard skips the collective).
``save_checkpoint`` / ``load_checkpoint`` use the key layout of models/basic_trainer.py:164-208
(``model_g``, ``optimizer_g``, ``scheduler_g``, ``loss`` state dicts + the training-state fields), so a
reference ``checkpoint.tar`` resumes here and vice versa (FlatAdam keeps torch.optim.Adam's state layout).
"""
from __future__ import annotations

import contextlib
import math
import time
from typing import Callable, Dict, Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import dp, side
from .optim import FlatAdam

GUARD_OFF = 1e8   # config_files/RDST_E1_OASIS_example_SRx4.ini:136


class DPTrainStep:
    """``loss_fn``: a callable ``(pred, target) -> loss`` (default L1) or an ``SRLoss``-shaped object returning
    ``(loss, report)`` (rdst_amd.loss.SRLoss: the weighted 'L1' / 'UNet-F' states of the reference trainer).
    ``graph=True``: after ``graph_warmup`` eager steps on one input shape, forward + loss + backward are captured into ONE
    HIP graph and every later step of that shape replays it (the collective and the optimizer stay outside, so RCCL
    keeps its own streams); other shapes, and steps under an active loss-threshold guard, run eagerly.  This is the
    step ``bench.py`` times.
    ``device_guard=True``: the loss-threshold guard (every threshold, GUARD_OFF included: a NaN loss always skips), a skip on
    a non-finite averaged gradient (``skip_nonfinite``) and global-norm clipping (``max_grad_norm``, clip_grad_norm_'s
    rule) are decided on the device; ``step()`` never takes the eager guarded branch and, on one rank, the captured graph
    holds guard and Adam too.  ``guard_stats()`` / ``checkpoint()`` are the only reads of the step state.
    ``ema_decay=d`` (BasicSR / SwinIR: 0.999; ``ema_warmup``: d_t = min(d, (1 + t) / (10 + t))): an exponential moving
    average of the trainable parameters, updated inside the Adam launch (FlatAdam), so the captured step keeps its one
    linear chain and gains no launch; a skipped step moves neither the parameters nor the average.  ``ema_scope()``,
    ``ema_state_dict()``, ``quick_eva()`` and the checkpoint's ``model_g_ema`` read it.  Several ranks need no collective
    for it: the average is a deterministic function of parameters that are already equal on every rank.  The reference
    keeps no EMA; it is off by default, and no PSNR gain is claimed for it here (no trained weights, no real volumes)."""

    RECORD_FLUSH = 4096   # parked device scalars before they are converted in one batch (bounds the memory they hold)

    def __init__(self, net: torch.nn.Module, lr: float = 1e-4, betas=(0.9, 0.99), eps: float = 1e-8,
                 weight_decay: float = 0.0, milestones: Optional[Sequence[int]] = None, gamma: float = 0.5,
                 loss_threshold: float = GUARD_OFF, loss_fn: Optional[Callable] = None, group=None,
                 graph: bool = False, graph_warmup: int = 2, device_guard: bool = False,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False):
        self.device_guard = bool(device_guard)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.device_guard and not all(p.is_cuda for p in net.parameters()):
            raise ValueError("DPTrainStep(device_guard=True): the guard is a HIP kernel, the network must be on a GPU")
        if not self.device_guard and (self.max_grad_norm is not None or self.skip_nonfinite):
            raise ValueError("DPTrainStep: max_grad_norm and skip_nonfinite need device_guard=True")
        self.net = net
        self.group = group
        dp.broadcast_parameters(net, group=group)
        self.bucket = dp.FlatGradBucket(net.parameters())
        self.optimizer = FlatAdam(self.bucket.params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                  bucket=self.bucket, device_state=self.device_guard, ema_decay=ema_decay,
                                  ema_warmup=ema_warmup)
        self.scheduler = (torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=list(milestones), gamma=gamma)
                          if milestones else None)
        if self.device_guard and self.scheduler is not None:
            # the object stays for the checkpoint layout; the rate comes from the device table, it is never stepped per step
            self.optimizer.set_schedule(list(milestones), gamma)
            self.optimizer.attach_scheduler(self.scheduler)
        self._peer_skip = None         # device int32: MAX over the ranks of "my loss is not below the threshold"
        self._graph_has_update = False  # the captured graph ends with guard + Adam (device_guard on one rank)
        self.loss_fn = loss_fn if loss_fn is not None else F.l1_loss      # SRLoss 'L1' (loss/sr_loss.py)
        # what the reference saves under 'loss' (basic_trainer.py:195): the loss object's own state_dict()
        self.loss_module = loss_fn if hasattr(loss_fn, "state_dict") else torch.nn.Module()
        self.loss_threshold = float(loss_threshold)
        self.last_report = None        # the (lazy) per-component report of the last step, SRLoss-shaped losses only
        self.last_batch = None         # the batch of the last step_from()
        # graph capture
        self.use_graph = bool(graph)
        self.graph_warmup = int(graph_warmup)
        self.graph = None
        self._graph_report = None      # the report object whose tensors the captured graph rewrites on every replay
        self._static = None            # (inputs, targets) the graph reads
        self._eager_seen = 0
        self._loss_buf = None
        self.capture_hook = None       # optional context-manager factory wrapped around the capture (bench.py's Recorder)
        # training state carried by the reference's checkpoints
        self.training_loss_names = ["L1"] if loss_fn is None else list(getattr(loss_fn, "loss_components", ["loss"]))
        self.training_loss_records: Dict[str, list] = {n: [] for n in self.training_loss_names}
        self._pending: Dict[str, list] = {}      # device scalars of the steps since the last flush (see _record)
        self._pending_keep: Dict[str, list] = {}  # device_guard: the decision of each parked step, next to its loss
        self.quick_validation_reports: list = []
        self.current_training_state_id = 0
        self.current_epoch = 0
        self.training_epoch_costs: list = []

    def _refuse_averaged(self, what: str) -> None:
        """Inside ema_scope() the network holds the averaged weights: gradients of them, or a graph captured with them
        under it, are never what a training step wants."""
        if self.optimizer.ema_active:
            raise RuntimeError(f"DPTrainStep.{what}: inside ema_scope() the network holds the averaged weights; "
                               "it must not train on them")

    def _keep_step(self, loss: torch.Tensor) -> bool:
        """The loss-threshold decision of trans_sr_trainer.py:162, made COLLECTIVELY: every rank must take the same
        branch, or the ranks that skip would leave the others waiting in the gradient all-reduce.  The group skips
        when ANY rank's local loss is not below the threshold (MAX over ranks of the "skip" flag; a NaN loss skips)."""
        skip = torch.logical_not(loss.detach() < self.loss_threshold).to(torch.float32).reshape(1)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(skip, op=dist.ReduceOp.MAX, group=self.group)
        return float(skip.item()) == 0.0

    def _loss(self, out, targets):
        r = self.loss_fn(out, targets)
        if isinstance(r, tuple):
            self.last_report = r[1]
            return r[0]
        return r

    def _record(self, loss: torch.Tensor) -> None:
        """trans_sr_trainer.py:165-167 appends ``report[name]`` (a Python float: one host sync per component and step).
        Here the DEVICE scalars of the step are parked (a clone each: the graph step overwrites its buffers) and become
        floats only when a checkpoint is written (`_flush_records`), so a step never leaves the device."""
        rep = self.last_report
        # device_guard: the step's decision (rdst_step_state.last_keep) is parked next to the loss; _flush_records drops
        # the steps that were skipped, which the reference never records (trans_sr_trainer.py:162-167)
        keep = self.optimizer.state_field("last_keep").clone() if self.device_guard else None
        if isinstance(rep, dict) and rep:
            for n in self.training_loss_names:
                if n in rep:
                    v = rep.raw(n) if hasattr(rep, "raw") else dict.__getitem__(rep, n)
                    self._pending.setdefault(n, []).append(v.detach().clone() if torch.is_tensor(v) else float(v))
                    self._pending_keep.setdefault(n, []).append(keep)
        elif len(self.training_loss_names) == 1:
            self._pending.setdefault(self.training_loss_names[0], []).append(loss.detach().clone())
            self._pending_keep.setdefault(self.training_loss_names[0], []).append(keep)
        if sum(len(v) for v in self._pending.values()) >= self.RECORD_FLUSH:
            self._flush_records()

    @staticmethod
    def _filter_records(vals: list, keeps: list) -> list:
        """The parked values of one loss component as floats, without the steps whose keep flag is 0 (a flag of None
        keeps: the step ran without the device guard).  One copy for the values, one for the flags."""
        ts = [v for v in vals if torch.is_tensor(v)]
        host = torch.stack([t.reshape(()).float() for t in ts]).cpu().tolist() if ts else []
        ks = [k for k in keeps if torch.is_tensor(k)]
        flags = iter(torch.stack([k.reshape(()) for k in ks]).cpu().tolist() if ks else [])
        it = iter(host)
        out = []
        for v, k in zip(vals, keeps):
            x = next(it) if torch.is_tensor(v) else v
            if (next(flags) if torch.is_tensor(k) else (1 if k is None else k)) != 0:
                out.append(x)
        return out

    def _flush_records(self) -> None:
        for n, vals in self._pending.items():
            if not vals:
                continue
            keeps = self._pending_keep.get(n) or [None] * len(vals)
            self.training_loss_records.setdefault(n, []).extend(self._filter_records(vals, keeps))
        self._pending = {}
        self._pending_keep = {}

    def loss_records(self) -> Dict[str, list]:
        """``training_loss_records`` with every parked step converted (the reference reads the attribute directly,
        basic_trainer.py:440; here the attribute lags by up to RECORD_FLUSH steps until this or checkpoint() runs)."""
        self._flush_records()
        return self.training_loss_records

    def fwd_bwd(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """forward + loss + backward with the gradients written straight into the flat bucket (no host sync inside:
        capturable).  Returns the loss as a device scalar that is overwritten by the next call."""
        self._refuse_averaged("fwd_bwd")
        self.bucket.detach_grads()       # autograd assigns fresh gradients; the HIP ops take the bucket views as destinations
        out = self.net(inputs)
        loss = self._loss(out, targets)
        if self._loss_buf is None:
            self._loss_buf = torch.zeros((), dtype=torch.float32, device=inputs.device)
        self._loss_buf.copy_(loss.detach())
        # (One reduction batch around the WHOLE backward — 6 + 3 slab-sum launches instead of 24 + 24 — was measured in round 4:
        # 17.6 -> 20.0 ms/step.  The ~1.7 GB of slabs then stay allocated until the end of the pass; per DenseSTLayer they are
        # 22-30 MB buffers that the caching allocator hands out again and again, written and summed while still in the 256 MiB
        # Infinity Cache.)
        # The layers' slab sums and LayerNorm finishes, and the convs' weight gradients, feed nothing before the optimizer: they
        # run on a side stream beside the dX chain (rdst_amd.side; RDST_SIDE_BRANCH=0 / RDST_SIDE_CONV=0 keep them on it).  The
        # join orders this stream behind them before the bucket is touched, and inside a capture it is what rejoins the branch.
        side.enable()
        try:
            loss.backward()
        finally:
            try:
                side.join()
            finally:
                side.disable()
        self.bucket.gather()             # whatever was not written in place is flattened into the bucket
        return self._loss_buf

    def capture(self, inputs: torch.Tensor, targets: torch.Tensor) -> bool:
        """Capture fwd_bwd on (copies of) these tensors into a HIP graph.  False (and eager from then on) if the capture
        fails; the parameters and BatchNorm statistics are not touched by a failed capture."""
        self._refuse_averaged("capture")   # before the try below: it is a caller's mistake, not a capture that failed
        self._static = (inputs.detach().clone(), targets.detach().clone())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with (self.capture_hook() if self.capture_hook is not None else contextlib.nullcontext()):
                with torch.cuda.graph(g):
                    self.fwd_bwd(*self._static)
                    if self._update_in_graph():     # one linear chain on the capture stream: ..., backward, guard, Adam
                        self._finish_step()
        except Exception as e:  # noqa: BLE001 - fall back to eager, loudly
            import warnings
            warnings.warn(f"rdst_amd.trainer: HIP-graph capture failed ({type(e).__name__}: {e}); running eagerly")
            torch.cuda.synchronize()
            # a backward that died half way leaves a reduction batch open and bucket views on offer: drop both (the
            # queued reductions name workspaces of the failed capture; running them later would write through freed memory)
            # (the batch lives on autograd's device thread: reset_backward_state() reaches it through an epoch counter)
            from . import ops
            ops.reset_backward_state()
            dp._OFFERED = {}
            self.bucket.gather()
            self.use_graph, self.graph, self._static, self._graph_report = False, None, None, None
            self._graph_has_update = False
            return False
        if not self.bucket.check_views():
            self.use_graph, self.graph, self._static, self._graph_report = False, None, None, None
            return False
        self.graph = g
        self._graph_has_update = self._update_in_graph()
        # the report the capture produced: its tensors are the graph's own buffers, refreshed by every replay.  An eager
        # step in between (another shape) rebinds last_report to ITS tensors; step() re-points it before recording a replay.
        self._graph_report = self.last_report
        return True

    def _graph_fits(self, inputs, targets) -> bool:
        return (self._static is not None and inputs.shape == self._static[0].shape and targets.shape == self._static[1].shape
                and inputs.dtype == self._static[0].dtype and targets.dtype == self._static[1].dtype)

    def step(self, inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """One iteration of trans_sr_trainer.py:131-178; returns the (device) loss."""
        self._refuse_averaged("step")                  # a replayed graph would not pass FlatAdam.step's own check
        t0 = time.time()                               # :132
        self.current_epoch += 1                        # :134 — advanced whether or not the update is skipped
        self.net.train()
        guarded = self.loss_threshold < GUARD_OFF and not self.device_guard
        if guarded:
            # the reference's order: forward, loss, decide, then backward (trans_sr_trainer.py:149-174); one host sync
            self.bucket.detach_grads()
            out = self.net(inputs)
            loss = self._loss(out, targets)
            if self._keep_step(loss):                  # :162
                self._record(loss)                     # :165-167
                loss.backward()
                self.bucket.gather()
                self._finish_step()
            else:
                self.bucket.gather()                   # restore p.grad = bucket views (zeros for this step)
            self.training_epoch_costs.append(time.time() - t0)
            return loss.detach()
        if self.use_graph and self.graph is None and self._eager_seen >= self.graph_warmup:
            self.capture(inputs, targets)
        if self.graph is not None and self._graph_fits(inputs, targets):
            if inputs.data_ptr() != self._static[0].data_ptr():
                self._static[0].copy_(inputs)
            if targets.data_ptr() != self._static[1].data_ptr():
                self._static[1].copy_(targets)
            self.graph.replay()
            self.last_report = self._graph_report
            loss = self._loss_buf
            in_graph = self._graph_has_update
        else:
            loss = self.fwd_bwd(inputs, targets)
            self._eager_seen += 1
            in_graph = False
        if self.device_guard:
            if not in_graph:
                self._finish_step()
            self._record(loss)                         # after the guard: the decision is parked next to the loss
        else:
            self._record(loss)                         # :165-167 (lazy: no host sync)
            self._finish_step()
        self.training_epoch_costs.append(time.time() - t0)   # :176-178 (host-side enqueue time: nothing synced)
        return loss

    def step_from(self, sampler) -> torch.Tensor:
        """``step()`` on a fresh batch of a ``rdst_amd.data.DevicePatchSampler`` (``last_batch`` keeps it).  Once a graph is
        captured and the batch has its shapes, the sampler writes straight into the tensors the graph reads, so ``step()``
        finds them in place and copies nothing; the sampler's launch is on the stream of the replay, so the previous replay
        has finished reading them.  Labels stay in the batch for the caller's own loop: ``step()`` takes none.  An augmenting
        sampler (``augment=True``) is taken as it is: its transformed batch lands in the same tensors.  So is a sampler with a
        ``degradation`` (blurred, antialiased or Fourier-truncated inputs): the batch has the same shapes and nothing here
        depends on how ``'in'`` was made.  A sampler with ``noise=`` likewise: every call draws a new seed and new levels with
        the origins, the one launch writes the noisy ``'in'`` into the graph's tensor, and ``last_batch`` carries
        ``'noise_seed'`` / ``'noise_levels'``, from which ``rdst_amd.data.add_noise`` reproduces that input bit for bit."""
        draw = sampler.draw()
        out = None
        if (self.graph is not None and (self.device_guard or self.loss_threshold >= GUARD_OFF)
                and self._static is not None):
            lr_shape, hr_shape = sampler.batch_shapes(draw)
            if (tuple(self._static[0].shape) == lr_shape and tuple(self._static[1].shape) == hr_shape
                    and self._static[0].dtype == torch.float32 and self._static[1].dtype == torch.float32
                    and self._static[0].device == sampler.device):
                out = self._static
        self.last_batch = sampler.sample(out=out, draw=draw)
        return self.step(self.last_batch["in"], self.last_batch["out"])

    def quick_eva(self, lr: torch.Tensor, hr: torch.Tensor, sr_scale: Optional[float] = None, metrics: str = "psnr ssim",
                  num_samples: int = 64, batch_size: int = 16, generator: Optional[torch.Generator] = None,
                  return_mode: str = "mean", use_ema: Optional[bool] = None) -> dict:
        """The quick validation of models/basic_trainer.py:257-286 (run every ``check_every`` iterations,
        trans_sr_trainer.py:180-181) on validation slices the caller loaded: ``num_samples`` random slices of ``lr`` (N, C, h, w)
        / ``hr`` (N, C, h*s, w*s) (torch.randperm with ``generator``; the reference shuffles with numpy) are super-resolved as
        SRTester.inference does (eval mode, no_grad, chunks of batch_size * 4, the network's own compute mode) and scored on the
        GPU (metrics.device_scores) after cropping ceil(s) border pixels.  The report, keyed as MetaSREvaluation keys it
        (``psnr_4.0``, metrics/sr_evaluation.py:142-156), is appended to ``quick_validation_reports`` and returned.
        The optimizer, the gradient bucket, the loss records, the packed weights and a captured graph are left as they were:
        the next step() computes what it would have computed without this call.
        ``use_ema``: None = the averaged weights when the trainer keeps an EMA, False = the live weights, True without an EMA
        raises.  The averaged weights are put under the network by ``ema_scope()`` (an in-place exchange) and taken out again
        before this returns, so the promise above holds for them too."""
        from . import ops
        from .metrics import SRMetrics
        if use_ema and not self.ema_enabled:
            raise RuntimeError("DPTrainStep.quick_eva(use_ema=True): needs DPTrainStep(ema_decay=...)")
        want_ema = self.ema_enabled if use_ema is None else bool(use_ema)
        if self.ema_enabled and self.optimizer.ema_active and not want_ema:
            raise RuntimeError("DPTrainStep.quick_eva(use_ema=False) inside ema_scope(): the network holds the averaged weights")
        scope = self.ema_scope if want_ema and not self.optimizer.ema_active else contextlib.nullcontext
        scorer = SRMetrics(metrics, return_mode, device="cuda")
        s = float(sr_scale if sr_scale is not None else getattr(self.net, "sr_scale", getattr(self.net, "upscale", 1)))
        idx = torch.randperm(len(lr), generator=generator)[:int(num_samples)]
        dev = next(self.net.parameters()).device
        modes = [(m, m.training) for m in self.net.modules()]
        self.net.eval()
        try:
            with torch.no_grad(), ops.keep_pack_plan(self.net), scope():
                rec = torch.cat([self.net(p.to(dev)) for p in lr[idx.to(lr.device)].split(int(batch_size) * 4)])
        finally:
            for m, t in modes:
                m.training = t
        rep = scorer(hr[idx.to(hr.device)].to(dev), rec, int(math.ceil(s)))
        report = {f"{m}_{s}": v for m, v in rep.items()}
        self.quick_validation_reports.append(report)
        return report

    # ---- the weight EMA (ema_decay=...) ------------------------------------------------------------------------------
    @property
    def ema_enabled(self) -> bool:
        return self.optimizer.ema is not None

    def ema_scope(self):
        """``with trainer.ema_scope():`` the network computes from the averaged weights (FlatAdam.ema_scope: one in-place
        exchange on entry, one on exit, also when the body raises).  No parameter moves, so the pack plan, the trainer's
        captured graph and an ``SRTester`` graph captured on the live weights stay valid; ``step()`` raises inside."""
        return self.optimizer.ema_scope()

    def ema_state_dict(self) -> dict:
        """``net.state_dict()`` (its keys, its order) with every trainable parameter's entry replaced by a clone of its
        averaged value; buffers and frozen parameters as they are.  Loads strictly into a plain network."""
        if not self.ema_enabled:
            raise RuntimeError("DPTrainStep.ema_state_dict: needs DPTrainStep(ema_decay=...)")
        opt = self.optimizer
        # inside ema_scope() the buffers are exchanged: the averaged values then sit under the parameters themselves
        avg = {id(p): (p if opt.ema_active else v) for p, v in zip(opt.param_groups[0]["params"], opt.ema_views())}
        sd = self.net.state_dict()
        for name, p in self.net.named_parameters():
            if id(p) in avg:
                sd[name] = avg[id(p)].detach().clone()
        return sd

    def _load_ema(self, sd: dict) -> None:
        opt = self.optimizer
        views = {id(p): v for p, v in zip(opt.param_groups[0]["params"], opt.ema_views())}
        with torch.no_grad():
            for name, p in self.net.named_parameters():
                if id(p) in views:
                    views[id(p)].copy_(sd[name])

    def _collective(self) -> bool:
        return (dist.is_available() and dist.is_initialized()
                and (dist.get_world_size(self.group) > 1 or dp.FORCE_COLLECTIVES))

    def _update_in_graph(self) -> bool:
        """device_guard without collectives: guard and Adam take no per-step arguments, so they are captured too."""
        return self.device_guard and not self._collective()

    def _finish_step(self) -> None:
        if self.device_guard:
            # _keep_step's rule without its .item(): any rank's skip (a NaN loss included) skips the whole group.  The flag
            # is 4 bytes, computed and reduced on the device; the bucket all-reduce ALWAYS runs (its result is discarded on
            # a skipped step) and the non-finite test sees the AVERAGED bucket, so every rank decides alike.
            peer = None
            if self._collective() and dist.get_world_size(self.group) > 1:
                peer = torch.logical_not(self._loss_buf.double() < self.loss_threshold).to(torch.int32).reshape(1)
                dist.all_reduce(peer, op=dist.ReduceOp.MAX, group=self.group)
                self._peer_skip = peer
            self.bucket.all_reduce_mean(self.group)
            self.optimizer.guard(self._loss_buf, self.loss_threshold, max_grad_norm=self.max_grad_norm,
                                 skip_nonfinite=self.skip_nonfinite, peer_skip=peer)
            self.optimizer.step()                      # rdst_adam_step_dev: rate and step count come from the device
            return
        self.bucket.all_reduce_mean(self.group)        # no-op on one rank
        self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()

    def guard_stats(self) -> dict:
        """The device guard's counters and latest decision (FlatAdam.sync_host(): one copy, the step's only read-back)."""
        if not self.device_guard:
            raise RuntimeError("DPTrainStep.guard_stats: needs device_guard=True")
        return self.optimizer.sync_host()

    # ---- models/basic_trainer.py:164-208 -----------------------------------------------------------
    def checkpoint(self) -> dict:
        """The reference's keys.  A trainer with an EMA adds two: ``model_g_ema`` (``ema_state_dict()``) and ``ema``
        (``{"decay", "warmup"}``); without one the keys are exactly the reference's."""
        if self.ema_enabled and self.optimizer.ema_active:
            raise RuntimeError("DPTrainStep.checkpoint: inside ema_scope() 'model_g' would hold the averaged weights")
        self._flush_records()
        if self.device_guard:
            self.optimizer.sync_host()                 # step count, rate and scheduler fields as `kept` updates leave them
        ck = {"Time": time.strftime("%Y-%m-%d %H:%M:%S"),
              "model_g": self.net.state_dict(),
              "optimizer_g": self.optimizer.state_dict(),
              "loss": self.loss_module.state_dict(),
              "training_loss_names": self.training_loss_names,
              "training_loss_records": self.training_loss_records,
              "quick_validation_reports": self.quick_validation_reports,
              "current_training_state_id": self.current_training_state_id,
              "current_epoch": self.current_epoch,
              "training_epoch_costs": self.training_epoch_costs}
        if self.scheduler is not None:
            ck["scheduler_g"] = self.scheduler.state_dict()
        if self.ema_enabled:
            ck["model_g_ema"] = self.ema_state_dict()
            ck["ema"] = {"decay": self.optimizer.ema_decay, "warmup": self.optimizer.ema_warmup}
        return ck

    def save_checkpoint(self, path: str) -> None:
        torch.save(self.checkpoint(), path)

    def load_checkpoint(self, path_or_dict, map_location=None) -> None:
        """With an EMA, ``model_g_ema`` is loaded into the averaged buffer when the checkpoint has it; when it has not (a
        reference checkpoint, or one written without an EMA) the average restarts from the loaded parameters
        (``reset_ema()``).  The decay stays the constructor's.  A trainer without an EMA ignores both keys."""
        ck = path_or_dict if isinstance(path_or_dict, dict) else torch.load(path_or_dict, map_location=map_location,
                                                                            weights_only=False)
        if self.ema_enabled and self.optimizer.ema_active:
            raise RuntimeError("DPTrainStep.load_checkpoint: inside ema_scope()")
        # parameters are views of the optimizer's flat buffer: load_state_dict copies in place and keeps them
        self.net.load_state_dict(ck["model_g"])
        if self.ema_enabled:
            if "model_g_ema" in ck:
                self._load_ema(ck["model_g_ema"])
            else:
                self.optimizer.reset_ema()
        self.optimizer.load_state_dict(ck["optimizer_g"])
        if self.scheduler is not None and "scheduler_g" in ck:
            self.scheduler.load_state_dict(ck["scheduler_g"])
        if self.device_guard and self.scheduler is not None:
            # the loaded schedule may differ from the constructor's: rebuild the rate table, and drop a graph that holds
            # the old one by value (the next step captures again).  The step count went to the device in load_state_dict.
            old = (self.optimizer._milestones, self.optimizer._lr_table)
            self.optimizer.set_schedule(sorted(self.scheduler.milestones.elements()), self.scheduler.gamma,
                                        base_lr=self.scheduler.base_lrs[0])
            if old != (self.optimizer._milestones, self.optimizer._lr_table) and self._graph_has_update:
                self.graph, self._static, self._graph_report, self._graph_has_update = None, None, None, False
        if "loss" in ck and len(ck["loss"]) and hasattr(self.loss_module, "load_state_dict"):
            self.loss_module.load_state_dict(ck["loss"])
        self.training_loss_names = ck.get("training_loss_names", self.training_loss_names)
        self.training_loss_records = ck.get("training_loss_records", self.training_loss_records)
        self._pending = {}             # steps taken before the load belong to the history that was just replaced
        self._pending_keep = {}
        self.quick_validation_reports = ck.get("quick_validation_reports", [])
        self.current_training_state_id = ck.get("current_training_state_id", 0)
        self.current_epoch = ck.get("current_epoch", 0)
        self.training_epoch_costs = ck.get("training_epoch_costs", [])
