#!/usr/bin/env python3
"""The x8 geometric self-ensemble of the tiled tester (rdst_amd/tiling.py unfold_tiles_d8 / merge_tiles_d8,
SRTester(self_ensemble=True)): the two kernels against the torch device-op compositions they replace, and slices/s of the tiled
tester plain and ensembled, eager and graph-replayed.

    python tools/self_ensemble_bench.py [--iters 50] [--reps 5] [--slices 64] [--passes 3] [--kernels-only]

The set-up of tools/tiled_infer_bench.py: RDST-E1 x4 in bf16 (bench.py's network), 64 slices of 1 x 34x42, tiles of 24 at stride
16, 32 network inputs per call (four tiles per call with the ensemble).  On seeded synthetic slices, after a warm-up, HIP
events, medians of `reps` alternating blocks in one process:
  (a) unfold_tiles_d8       against unfold_tiles + eight dihedral(...) views + stack(dim=1).reshape(...).contiguous();
  (b) merge_tiles_d8        against eight dihedral_inverse(...) of the strided views y[k::8], added up in ascending k and scaled
                            (torch.equal to both is asserted before anything is timed);
  (c) SRTester.inference    tiled plain and ensembled, eager and graph, in slices/s (whole passes over the 64 slices), and the
                            ensembled-over-plain time of the graph path (8 by construction: eight times the replays at one
                            batch shape).
One JSON line per measurement.  `--kernels-only` stops after (a) and (b): the run to put under `rocprofv3 --kernel-trace --stats`
for the durations of the kernels themselves."""
import argparse
import json
import os
import statistics
import sys

import torch

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
        raise SystemExit("self_ensemble_bench: no GPU")
    dev = torch.device("cuda:0")
    N, C, h, w, p, s, scale, tile_batch = a.slices, 1, 34, 42, 24, 16, 4, 32
    plan = T.TilePlan(h, w, p, s, scale=scale)
    P, tiles = plan.hr.patch, N * plan.tiles_per_slice
    x = torch.rand(N, C, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    y = torch.rand(8 * tiles, C, P, P, generator=torch.Generator().manual_seed(2)).to(dev)

    # (a) / (b): the kernels against the compositions of torch device ops
    def torch_unfold_d8():
        t = T.unfold_tiles(x, plan)
        return torch.stack([T.dihedral(t, k) for k in range(8)], dim=1).reshape(-1, C, p, p).contiguous()

    def torch_merge_d8():
        acc = T.dihedral_inverse(y[0::8], 0).clone()
        for k in range(1, 8):
            acc += T.dihedral_inverse(y[k::8], k)
        return acc * 0.125

    assert torch.equal(T.unfold_tiles_d8(x, plan), torch_unfold_d8())
    assert torch.equal(T.merge_tiles_d8(y), torch_merge_d8())
    for name, ours, theirs, nbytes in (
            ("unfold_tiles_d8", lambda: T.unfold_tiles_d8(x, plan), torch_unfold_d8, (x.numel() + 8 * tiles * C * p * p) * 4),
            ("merge_tiles_d8", lambda: T.merge_tiles_d8(y), torch_merge_d8, (y.numel() + tiles * C * P * P) * 4)):
        for _ in range(5):
            ours(), theirs()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(events(ours, a.iters))
            tb.append(events(theirs, a.iters))
        print(json.dumps({"kernel": name, "slices": [N, C, h, w], "patch": p, "stride": s, "scale": scale, "tiles": tiles,
                          "bytes": nbytes, "equal_to_torch": True, "hip_ms": spread(ta), "torch_ops_ms": spread(tb),
                          "torch_over_hip": round(statistics.median(tb) / statistics.median(ta), 2)}), flush=True)

    if a.kernels_only:
        return
    # (c): the tester
    import bench
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    kw = dict(tile=p, tile_stride=s, tile_batch=tile_batch)
    testers = {"plain eager": SRTester(net, **kw), "plain graph": SRTester(net, graph=True, **kw),
               "x8 eager": SRTester(net, self_ensemble=True, **kw), "x8 graph": SRTester(net, graph=True, self_ensemble=True, **kw)}
    for _ in range(2):
        for t in testers.values():
            t.inference(x)
    torch.cuda.synchronize()
    for name in ("plain graph", "x8 graph"):
        if testers[name].graph is None:
            raise SystemExit(f"self_ensemble_bench: the tile batch of '{name}' was not captured")
    same = {k: torch.equal(testers[f"{k} eager"].inference(x), testers[f"{k} graph"].inference(x)) for k in ("plain", "x8")}
    times = {name: [] for name in testers}
    for _ in range(a.reps):
        for name, t in testers.items():
            times[name].append(events(lambda t=t: t.inference(x), a.passes))
    for name, v in times.items():
        print(json.dumps({"inference": name, "net": "RDST-E1 x4 bf16", "slices": [N, C, h, w],
                          "tiles_per_slice": plan.tiles_per_slice, "per_call": tile_batch,
                          "tiles_per_call": tile_batch // (8 if name.startswith("x8") else 1), "ms_per_pass": spread(v),
                          "slices_per_s": round(N / statistics.median(v) * 1e3, 1)}), flush=True)
    med = {name: statistics.median(v) for name, v in times.items()}
    print(json.dumps({"graph_equals_eager": same, "graph_replays": {k: testers[f"{k} graph"].graph_replays for k in same},
                      "graph_captures": {k: testers[f"{k} graph"].graph_captures for k in same},
                      "x8_over_plain_time_graph": round(med["x8 graph"] / med["plain graph"], 3),
                      "x8_over_plain_time_eager": round(med["x8 eager"] / med["plain eager"], 3)}), flush=True)


if __name__ == "__main__":
    main()
