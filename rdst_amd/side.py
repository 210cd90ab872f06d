"""The Python half of the side branch of the deferred reductions (include/rdst_hip.h, "the side branch").

With the branch enabled, ``rdst_reduce_batch_end`` issues a DenseSTLayer's slab sums and LayerNorm finishes on a side stream
and returns; the backward chain goes on with the next layer while they run.  Two things follow for the host side:

  * what those launches read (the ops' slab workspaces, scratch destinations, copies: ``_ReduceBatch.keep``) must outlive
    them.  A flush ``park``s its list as one generation instead of dropping it; ``release_older`` drops every generation but
    the newest once the NEXT ``rdst_reduce_batch_end`` has returned (its first step orders the caller's stream behind the
    previous generation, so the caching allocator may hand the memory out again on that stream); ``join`` drops all of them.
    At most two layers' slabs are alive, never the whole pass.
  * what they write (parameter gradients) is complete only after ``join``: `DPTrainStep.fwd_bwd` enables the branch around
    ``loss.backward()`` and joins before it touches the bucket; inside a stream capture that join is what rejoins the branch.
    A flush whose destinations autograd may read as soon as the node returns joins at once (rdst_amd.ops).

The switch is process-wide, as it is in the library: the trainer sets it on its own thread, autograd's device thread runs the
backward.  The parked generations are kept per device.

Two switches, read once: ``RDST_SIDE_BRANCH`` (the reductions) and ``RDST_SIDE_CONV`` (a conv's weight gradient beside its data
gradient, `csrc/conv.hip`).  Both default to on: measured, only the two together are faster than the serial step
(profiles/side_branch_bench.txt).  With both 0 ``enable`` is a no-op and the step is the serial step, node for node.
"""
from __future__ import annotations

import os
import threading

import torch

from . import _lib

SIDE_BRANCH = os.environ.get("RDST_SIDE_BRANCH", "1") != "0"
# stage 2: a conv's weight gradient (and its reduce) beside its data gradient, where both are wanted (csrc/conv.hip: bwd_t)
SIDE_CONV = os.environ.get("RDST_SIDE_CONV", "1") != "0"

_lock = threading.Lock()
_on = False       # between enable() and disable()
_handle = None    # the library enable() reached first; join() / reset() make no call before that
_parked: dict = {}   # device index -> generations (lists of tensors), oldest first


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def enabled() -> bool:
    return _on


def conv_enabled() -> bool:
    return _on and SIDE_CONV


def enable() -> bool:
    """Turn on the stages the switches name (a no-op with both off).  Returns whether anything is on now."""
    global _on, _handle
    bits = (1 if SIDE_BRANCH else 0) | (2 if SIDE_CONV else 0)
    if not bits:
        return False
    if _handle is None:
        _handle = _lib.load()
    _handle.rdst_side_enable(bits)
    _on = True
    return True


def disable() -> bool:
    """Turn the branch off; returns whether it was on.  Work already issued stays pending until join()."""
    global _on
    was = _on
    if _handle is not None:
        was = bool(_handle.rdst_side_enable(0)) or was
    _on = False
    return was


def park(tensors) -> None:
    """Keep these tensors alive as the newest generation of the current device."""
    with _lock:
        _parked.setdefault(torch.cuda.current_device(), []).append(list(tensors))


def park_current(tensors) -> None:
    """Keep these tensors alive with the newest generation of the current device (a launch site between two flushes:
    the flush after the next one releases them, when its stream is ordered behind them)."""
    with _lock:
        gens = _parked.setdefault(torch.cuda.current_device(), [])
        if not gens:
            gens.append([])
        gens[-1].extend(t for t in tensors if t is not None)


def release_older() -> None:
    """Drop every generation of the current device but the newest: the caller's stream is ordered behind them."""
    with _lock:
        gens = _parked.get(torch.cuda.current_device())
        if gens and len(gens) > 1:
            del gens[:-1]


def join() -> None:
    """The current stream waits for everything issued on the side stream; the parked generations are released."""
    if _handle is None:
        return
    try:
        _lib.check(_handle.rdst_side_join(_stream()), "rdst_side_join")
    finally:
        with _lock:
            _parked.pop(torch.cuda.current_device(), None)


def reset() -> None:
    """After a backward that did not run to its end: no generation stays pending, nothing stays parked."""
    if _handle is not None:
        try:
            _lib.check(_handle.rdst_side_reset(), "rdst_side_reset")
        finally:
            with _lock:
                _parked.clear()
