#!/usr/bin/env python3
"""Tiled whole-slice inference on the device (rdst_amd/tiling.py, SRTester(tile=...)): the two copy kernels against the torch
device-op compositions they replace, and slices/s of the tiled tester, eager and graph-replayed.

    python tools/tiled_infer_bench.py [--iters 50] [--reps 5] [--slices 64] [--passes 3] [--kernels-only]

RDST-E1 x4 in bf16 (bench.py's network), 64 slices of 1 x 34x42 (the reference-shaped OASIS slice, 176x208 less 20 pixels a
side, at x4), tiles of 24 at stride 16, 32 tiles per network call.  On seeded synthetic slices, after a warm-up, HIP events,
medians of `reps` alternating blocks in one process:
  (a) unfold_tiles          against nn.Unfold(padding=...) (pad + im2col) + the transposed copy on the device, same shapes;
  (b) fold_tiles            against the transposed copy + nn.Fold + multiply by a resident reciprocal divisor image;
  (c) SRTester.inference    tiled eager and tiled graph at 34x42, in slices/s (whole passes over the 64 slices);
  (d) for scale             whole-slice SRTester.inference at 40x48 (the next multiples of the window size: the only way such
                            a slice could be run without tiling, by padding it), untouched by this change.
One JSON line per measurement.  `--kernels-only` stops after (a) and (b): the run to put under `rocprofv3 --kernel-trace --stats`
for the durations of the kernels themselves."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rdst_amd import tiling as T  # noqa: E402
from rdst_amd.tester import SRTester  # noqa: E402


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiled_infer_bench: no GPU")
    dev = torch.device("cuda:0")
    N, C, h, w, p, s, scale, tile_batch = a.slices, 1, 34, 42, 24, 16, 4, 32
    plan = T.TilePlan(h, w, p, s, scale=scale)
    lr, hr = plan.lr, plan.hr
    x = torch.rand(N, C, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    sr_tiles = torch.rand(N * plan.tiles_per_slice, C, hr.patch, hr.patch, generator=torch.Generator().manual_seed(2)).to(dev)

    # (a) / (b): the kernels against the compositions of torch device ops
    unfold = nn.Unfold(kernel_size=p, stride=s, padding=(lr.pad_y, lr.pad_x))
    fold = nn.Fold(output_size=(hr.H, hr.W), kernel_size=hr.patch, stride=hr.stride, padding=(hr.pad_y, hr.pad_x))
    recip = (1.0 / torch.from_numpy(plan.cover(hr=True)).float()).to(dev)

    def torch_unfold():
        return unfold(x).transpose(1, 2).reshape(-1, C, p, p).contiguous()

    def torch_fold():
        return fold(sr_tiles.reshape(N, plan.tiles_per_slice, -1).transpose(1, 2)) * recip

    assert torch.equal(T.unfold_tiles(x, plan), torch_unfold())
    dmax = (T.fold_tiles(sr_tiles, plan, N) - torch_fold()).abs().max().item()
    for name, ours, theirs, nbytes in (
            ("unfold_tiles", lambda: T.unfold_tiles(x, plan), torch_unfold, (x.numel() + N * plan.tiles_per_slice * C * p * p) * 4),
            ("fold_tiles", lambda: T.fold_tiles(sr_tiles, plan, N), torch_fold, (sr_tiles.numel() + N * C * hr.H * hr.W) * 4)):
        for _ in range(5):
            ours(), theirs()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(events(ours, a.iters))
            tb.append(events(theirs, a.iters))
        print(json.dumps({"kernel": name, "slices": [N, C, h, w], "patch": p, "stride": s, "scale": scale, "bytes": nbytes,
                          "hip_ms": spread(ta), "torch_ops_ms": spread(tb),
                          "torch_over_hip": round(statistics.median(tb) / statistics.median(ta), 2),
                          **({"max_abs_diff_to_torch_fp32": dmax} if name == "fold_tiles" else {})}), flush=True)

    if a.kernels_only:
        return
    # (c) / (d): the tester
    import bench
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    eager = SRTester(net, tile=p, tile_stride=s, tile_batch=tile_batch)
    graph = SRTester(net, tile=p, tile_stride=s, tile_batch=tile_batch, graph=True)
    whole = SRTester(net, batch_size=tile_batch // 4)          # chunks of batch_size * 4 = 32 slices
    xw = torch.rand(N, C, 40, 48, generator=torch.Generator().manual_seed(3)).to(dev)
    for _ in range(2):
        eager.inference(x), graph.inference(x), whole.inference(xw)
    torch.cuda.synchronize()
    if graph.graph is None:
        raise SystemExit("tiled_infer_bench: the tile batch was not captured")
    same = torch.equal(eager.inference(x), graph.inference(x))
    te, tg, tw = [], [], []
    for _ in range(a.reps):
        te.append(events(lambda: eager.inference(x), a.passes))
        tg.append(events(lambda: graph.inference(x), a.passes))
        tw.append(events(lambda: whole.inference(xw), a.passes))
    for name, t, shape in (("tiled eager", te, (h, w)), ("tiled graph", tg, (h, w)), ("whole slice", tw, (40, 48))):
        print(json.dumps({"inference": name, "net": "RDST-E1 x4 bf16", "slices": [N, C, *shape],
                          "tiles_per_slice": plan.tiles_per_slice if name != "whole slice" else None,
                          "per_call": tile_batch, "ms_per_pass": spread(t),
                          "slices_per_s": round(N / statistics.median(t) * 1e3, 1)}), flush=True)
    print(json.dumps({"graph_equals_eager": same, "graph_captures": graph.graph_captures, "graph_replays": graph.graph_replays,
                      "graph_over_eager_time": round(statistics.median(tg) / statistics.median(te), 3)}), flush=True)


if __name__ == "__main__":
    main()
