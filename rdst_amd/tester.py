"""Whole-slice inference shell: the inner loop of the reference tester
(models/trans_sr_tester.py:124-166) around the HIP network, plus the scoring of metrics/sr_evaluation.py:143-156.

    net.eval(); with torch.no_grad(): for p in lr_img.split(batch_size * 4): rec.append(net(p)); rec = torch.cat(rec)

The network itself runs on any H x W that is a multiple of the window size (non-square, other than the constructor's img_size)
and any batch size; the shifted-window mask is analytic, so nothing is rebuilt per shape.  Slices of ANY size go through the
tiled path (``SRTester(tile=...)``, rdst_amd/tiling.py): the slices are unfolded into overlapping fixed-size tiles on the
device, the network runs on ``tile_batch`` tiles at a time, and the SR tiles are folded back with their overlaps averaged, as
the reference's ImageFolder / UnFolder / Folder do (datasets/basic_dataset.py:347-449).  Every tile batch has one shape
whatever the slice size, so with ``graph=True`` the eval forward is captured into a HIP graph once and replayed for every
batch."""
from __future__ import annotations

import math
import warnings
from typing import Dict, List, Optional, Sequence

import torch

from .metrics import SRMetrics


def _window_sizes(net: torch.nn.Module) -> List[int]:
    """The window sizes of the network's attention blocks (RDSTSR keeps one per stage, SwinIR one in every block)."""
    ws = getattr(net, "window_size", None)
    if ws is None:
        ws = [m.window_size for m in net.modules() if isinstance(getattr(m, "window_size", None), int)]
    return sorted({int(w) for w in (ws if isinstance(ws, (list, tuple)) else [ws])}) or [1]


class SRTester:
    """``tile=None``: ``inference`` runs the network on whole slices (H and W multiples of the window size).

    ``tile=p`` (a multiple of the network's window size; ``tile_stride`` defaults to ``p``): ``inference`` takes slices of any
    size.  ``tile_batch`` tiles go through the network at a time, in eval mode under ``no_grad`` in the network's own compute
    mode; the SR tiles of a chunk of whole slices (at most ``tile_buffer_bytes`` of them, one slice at least) are collected in
    one buffer and folded by one launch.  ``pad_mode``: what the tiles see outside the slice, ``'zero'`` (the reference) or
    ``'edge'``.  The packed weights and a captured training graph of the network are left as they were
    (``ops.keep_pack_plan``), so the call may sit between training steps.

    ``graph=True``: the first full tile batch (the first two, if the first leaves no packed weights behind) runs eagerly, then
    ``net(static_in)`` is captured into one HIP graph and every
    later batch, of any slice size, is ``unfold_tiles(out=static_in)`` + replay + a device copy of the static output into the
    tile buffer; a last batch with fewer tiles is replayed too, its unused slots filled with zeros.  The refresh of the packed
    weights is a node of the captured forward, so the graph reads the live parameters: ``load_state_dict`` between calls needs
    no recapture.  The graph is dropped, and captured again on the next full batch, when the parameters move or change dtype or
    the compute mode changes (``PackPlan.valid``).  A failed capture warns and the tester runs eagerly from then on.
    ``graph_captures`` / ``graph_replays`` count what happened.

    ``self_ensemble=True`` (the tiled path only; ``tile_batch`` a multiple of 8): the x8 geometric self-ensemble, the "+" of
    EDSR / RCAN / SwinIR, per tile.  A network call carries ``tile_batch / 8`` tiles, each under its eight flips and
    transposes (``tiling.unfold_tiles_d8``, slot ``8 t + k``); the eight outputs are transformed back and averaged in fp32
    (``tiling.merge_tiles_d8``) straight into the tile buffer, which is folded as before.  Tiles are square, so the tile batch
    and the captured graph are the ones of the plain path: 8x the network calls, one unfold and one merge launch per call.

    ``back_project=k`` (an integer scale only): ``k`` Landweber steps ``P <- P - tau A^T(A P - lr)`` on every chunk of whole SR
    slices against its LR slices, on both paths, so the output agrees with the slices that were measured; ``A`` is
    ``degradation`` (default ``'cubic'``; ``data.operator_table(d, h s, h)`` along each axis) and ``tau`` is ``bp_step`` or
    ``1 / (|A_y|^2 |A_x|^2)`` (``data.operator_norm``; the iteration contracts for ``tau < 2 / |A|^4``).  The steps run in fp32, so with
    ``back_project > 0`` the result is fp32 whatever dtype the network returns; ``0`` takes no step and keeps the network's dtype."""

    def __init__(self, net: torch.nn.Module, batch_size: int = 16, sr_scale: Optional[float] = None,
                 metrics: str = "psnr ssim", compute_dtype: Optional[torch.dtype] = None, *, tile: Optional[int] = None,
                 tile_stride: Optional[int] = None, tile_batch: int = 32, pad_mode: str = "zero", graph: bool = False,
                 tile_buffer_bytes: int = 1 << 30, self_ensemble: bool = False, back_project: int = 0, degradation=None,
                 bp_step: Optional[float] = None):
        self.net = net
        self.batch_size = int(batch_size)
        self.sr_scale = float(sr_scale if sr_scale is not None else getattr(net, "sr_scale", getattr(net, "upscale", 1)))
        self.metrics = SRMetrics(metrics, "full")
        self.device_metrics = SRMetrics(metrics, "full", device="cuda")
        if compute_dtype is not None and hasattr(net, "set_compute_dtype"):
            net.set_compute_dtype(compute_dtype)
        # the tiled path
        self.tile = None if tile is None else int(tile)
        self.tile_stride = self.tile if tile_stride is None else int(tile_stride)
        self.tile_batch, self.pad_mode, self.tile_buffer_bytes = int(tile_batch), pad_mode, int(tile_buffer_bytes)
        self.use_graph = bool(graph) and self.tile is not None
        self.self_ensemble = bool(self_ensemble)
        if self.self_ensemble and self.tile is None:
            raise ValueError("SRTester: self_ensemble=True needs the tiled path (tile=...); a square slice that is a multiple of "
                             "the window size can be run as one tile (tile=H, tile_stride=H)")
        # back-projection
        if isinstance(back_project, bool) or int(back_project) != back_project or back_project < 0:
            raise ValueError(f"SRTester: back_project={back_project!r} must be a non-negative number of steps")
        self.back_project = int(back_project)
        self.degradation = self.bp_step = None
        if self.back_project:
            from .data import Degradation
            self.degradation = Degradation.of("cubic" if degradation is None else degradation)
            if self.sr_scale != int(self.sr_scale) or self.sr_scale < 1:
                raise ValueError(f"SRTester: back-projection needs an integer scale, got {self.sr_scale}")
            if bp_step is not None:
                if not (math.isfinite(float(bp_step)) and float(bp_step) > 0):
                    raise ValueError(f"SRTester: bp_step={bp_step!r} must be positive and finite")
                self.bp_step = float(bp_step)
        self.graph = None
        self.graph_captures = self.graph_replays = 0
        self._static_in = self._static_out = self._graph_plan = self._graph_sig = None
        self._eager_full = 0           # full tile batches run eagerly since the last (attempted) capture
        self._plan = None              # the packed weights the tiled forwards of the last call ended with
        self._tile_plans: dict = {}
        if self.tile is not None:
            from .tiling import PAD_MODES
            ws = _window_sizes(net)
            if self.tile <= 0 or any(self.tile % w for w in ws):
                raise ValueError(f"SRTester: tile={self.tile} must be a positive multiple of the window size {ws}")
            if not 0 < self.tile_stride <= self.tile:
                raise ValueError(f"SRTester: tile_stride={self.tile_stride} must lie in 1..tile={self.tile}")
            if self.tile_batch <= 0 or self.tile_buffer_bytes <= 0:
                raise ValueError("SRTester: tile_batch and tile_buffer_bytes must be positive")
            if pad_mode not in PAD_MODES:
                raise ValueError(f"SRTester: pad_mode must be one of {sorted(PAD_MODES)}, got {pad_mode!r}")
            if self.sr_scale != int(self.sr_scale) or self.sr_scale < 1:
                raise ValueError(f"SRTester: the tiled path needs an integer scale, got {self.sr_scale}")
            if self.self_ensemble and self.tile_batch % 8:
                raise ValueError(f"SRTester: self_ensemble=True fills a network call with the eight variants of whole tiles; "
                                 f"tile_batch={self.tile_batch} must be a multiple of 8")

    @torch.no_grad()
    def inference(self, lr_img: torch.Tensor) -> torch.Tensor:
        """trans_sr_tester.py:141-160: (N, C, H, W) low-resolution slices -> (N, C, H*s, W*s)."""
        self.net.eval()
        dev = next(self.net.parameters()).device
        if self.tile is not None:
            return self._tiled(lr_img, dev)
        if self.back_project:
            rec = []
            for p in lr_img.split(self.batch_size * 4):
                p = p.to(dev)
                rec.append(self._back_projected(self.net(p), p))
        else:
            rec = [self.net(p.to(dev)) for p in lr_img.split(self.batch_size * 4)]
        return torch.cat(rec, dim=0)

    # ---- back-projection ---------------------------------------------------------------------------------------------
    def _back_projected(self, P: torch.Tensor, lr: torch.Tensor, own: bool = False) -> torch.Tensor:
        """``back_project`` Landweber steps ``P <- P - tau A^T(A P - lr)`` on the SR slices ``P`` (N, C, h s, w s) of the LR
        slices ``lr`` (N, C, h, w): two launches per step, the residual of the degraded slices (rdst_lrc_residual) and the
        adjoint with ``P`` as its base, in place (rdst_lrc_adjoint).  ``tau`` is ``bp_step`` or ``1 / (|A_y|^2 |A_x|^2)``."""
        from .data import operator_norm
        from .loss.consistency import lrc_adjoint, lrc_residual
        s, d = int(self.sr_scale), self.degradation
        h, w = lr.shape[-2:]
        if tuple(P.shape[-2:]) != (h * s, w * s) or P.shape[:2] != lr.shape[:2]:
            raise RuntimeError(f"SRTester.inference: back-projection expects {(h * s, w * s)} SR slices of {(h, w)} LR slices, "
                               f"the network gave {tuple(P.shape)} for {tuple(lr.shape)}")
        tau = self.bp_step
        if tau is None:
            tau = 1.0 / (operator_norm(d, h * s, h) ** 2 * operator_norm(d, w * s, w) ** 2)
        out = P.detach().to(torch.float32).contiguous()
        if out.data_ptr() == P.data_ptr() and not own:
            out = out.clone()           # the network's output may be a buffer it keeps
        lr = lr.detach().to(torch.float32).contiguous()
        for _ in range(self.back_project):
            resid, _, _ = lrc_residual(out, lr, d)
            lrc_adjoint(resid, (h * s, w * s), d, scale=-tau, base=out, out=out)
        return out

    # ---- the tiled path ----------------------------------------------------------------------------------------------
    def _tile_plan(self, h: int, w: int):
        from .tiling import TilePlan
        plan = self._tile_plans.get((h, w))
        if plan is None:
            plan = self._tile_plans[(h, w)] = TilePlan(h, w, self.tile, self.tile_stride, int(self.sr_scale), self.pad_mode)
        return plan

    def _tiled(self, lr_img: torch.Tensor, dev) -> torch.Tensor:
        from . import ops
        from .tiling import fold_tiles, merge_tiles_d8
        if lr_img.dim() != 4 or min(lr_img.shape) <= 0:
            raise ValueError(f"SRTester.inference: lr_img must be a non-empty (N, C, h, w), got {tuple(lr_img.shape)}")
        N, C, h, w = lr_img.shape
        plan = self._tile_plan(h, w)
        T, P = plan.tiles_per_slice, plan.hr.patch
        E = 8 if self.self_ensemble else 1              # network inputs per tile
        B = self.tile_batch // E                        # tiles per network call
        per_chunk = max(1, self.tile_buffer_bytes // (T * C * P * P * 4))
        rec = []
        with torch.cuda.device(dev), ops.keep_pack_plan(self.net):
            # these forwards use the packed weights of the tester's last call while they are still good (the caller's own
            # otherwise); whatever the network had on entry comes back on exit
            if self.graph is not None and not self._graph_valid():
                self._drop_graph()
            if self._plan is not None and self._plan.valid(self.net):
                ops.install_pack_plan(self.net, self._plan)
            try:
                for chunk in lr_img.split(per_chunk):
                    x = chunk.to(dev, torch.float32)
                    n = x.shape[0]
                    tiles = torch.empty(n * T, C, P, P, dtype=torch.float32, device=dev)
                    for f in range(0, n * T, B):
                        m = min(B, n * T - f)
                        y = self._forward_tiles(x, plan, f, m)
                        if tuple(y.shape[1:]) != (C, P, P):
                            raise RuntimeError(f"SRTester.inference: the network maps a {(C, self.tile, self.tile)} tile to "
                                               f"{tuple(y.shape[1:])}, the plan expects {(C, P, P)}")
                        if self.self_ensemble:
                            merge_tiles_d8(y[:E * m] if y.dtype == torch.float32 else y[:E * m].float(), out=tiles[f:f + m])
                        else:
                            tiles[f:f + m].copy_(y[:m])
                    sr = fold_tiles(tiles, plan, n)
                    rec.append(self._back_projected(sr, x, own=True) if self.back_project else sr)
            finally:
                self._plan = ops.pack_plan_of(self.net)
        return rec[0] if len(rec) == 1 else torch.cat(rec, dim=0)

    def _forward_tiles(self, x: torch.Tensor, plan, first: int, m: int) -> torch.Tensor:
        """The SR tiles of tiles ``[first, first + m)`` of ``x``: at least ``m`` rows (``8 m`` with the self-ensemble, row
        ``8 t + k`` for variant ``k`` of tile ``first + t``), the network's output or the graph's."""
        from .tiling import unfold_tiles, unfold_tiles_d8
        C = x.shape[1]
        if self.self_ensemble:
            unfold_tiles, m = unfold_tiles_d8, 8 * m    # m network inputs, eight per tile
        B = self.tile_batch
        if self.use_graph and self.graph is None and m == B and self._eager_full >= 1:
            self._capture(C, x.device)
        if self.graph is not None and tuple(self._static_in.shape[1:2]) == (C,) and self._static_in.device == x.device:
            unfold_tiles(x, plan, out=self._static_in, first_tile=first)      # slots past the last tile are zeros
            self.graph.replay()
            self.graph_replays += 1
            return self._static_out
        if m == B:
            self._eager_full += 1
        return self.net(unfold_tiles(x, plan, first_tile=first, n_slots=m))

    def _drop_graph(self) -> None:
        self.graph = self._graph_plan = self._graph_sig = self._static_in = self._static_out = None
        self._eager_full = 0

    def _graph_valid(self) -> bool:
        """The parameters are where and what they were at the capture, in the same compute mode, and the packed weights the
        graph refreshes and reads (if the network packs any) are still theirs."""
        from . import ops
        return (ops.PackPlan.signature(self.net) == self._graph_sig
                and (self._graph_plan is None or self._graph_plan.valid(self.net)))

    def _capture(self, C: int, dev) -> bool:
        """Capture ``net(static_in)`` into a HIP graph.  The forward it records starts with the refresh of the network's packed
        weights from the live parameters (ops.pack_scope), so their plan should exist before the capture: a first eager batch
        records it, and if that batch dropped an older plan instead, a second one does; a network that has none after two
        packs nothing ahead and its ops read the parameters themselves.  False, and eager from then on, if the capture fails."""
        from . import ops
        pack = ops.pack_plan_of(self.net)
        if pack is not None and not pack.valid(self.net):
            pack = None
        if pack is None and self._eager_full < 2:
            return False
        static_in = torch.zeros(self.tile_batch, C, self.tile, self.tile, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                static_out = self.net(static_in)
        except Exception as e:  # noqa: BLE001 - fall back to eager, loudly
            warnings.warn(f"rdst_amd.tester: HIP-graph capture failed ({type(e).__name__}: {e}); running eagerly")
            torch.cuda.synchronize()
            ops.reset_backward_state()
            self.use_graph = False
            self._drop_graph()
            return False
        # the graph refreshes and reads the arena of `pack`: it stays good while `pack` is valid, whatever plan the network's
        # eager forwards use by then
        self.graph, self._graph_plan, self._graph_sig = g, pack, ops.PackPlan.signature(self.net)
        self._static_in, self._static_out = static_in, static_out
        self.graph_captures += 1
        return True

    def evaluate(self, lr_img: torch.Tensor, gt_img: torch.Tensor, on_device: bool = False) -> Dict[str, List[float]]:
        """Scores of metrics/sr_evaluation.py:152: per-image metrics after cropping ceil(sr_scale) border pixels.
        ``on_device=True``: the reconstruction stays on the GPU, ``gt_img`` is moved there once and both are scored there
        (metrics.device_scores); only the per-image scores come back to the host."""
        rec = self.inference(lr_img)
        if on_device:
            return self.device_metrics(gt_img.to(rec.device), rec, int(math.ceil(self.sr_scale)))
        return self.metrics(gt_img, rec, int(math.ceil(self.sr_scale)))
