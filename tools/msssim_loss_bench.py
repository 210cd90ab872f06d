#!/usr/bin/env python3
"""What the MS-SSIM training loss costs: the HIP pyramid against the same loss composed of torch ops and against the
single-scale SSIM loss, eager and graph-replayed, and the training step with either.

    python tools/msssim_loss_bench.py [--steps 20] [--reps 5] [--warmup 6] [--cases abcde] [--out profiles/msssim_loss_bench.txt]
                                      [--commit NAME] [--parent NAME]

The protocol of tools/ssim_loss_bench.py, HIP events around every block.  Forward + backward at 32 x 1 x 256 x 256 with 5
levels and at 32 x 1 x 96 x 96 with 4 levels, Gaussian window of 11 taps:
  (a) rdst_amd.loss.ms_ssim_loss: 2 levels + 1 kernel launches + the upstream multiply;
  (b) the same loss composed of torch fp32 device ops (separable depthwise conv2d, avg_pool2d, pow, prod) under autograd;
  (c) single-scale rdst_amd.loss.ssim_loss, gaussian 11, at the same shape: the pyramid holds 4/3 of its pixels, so this is the
      yardstick for what the extra levels and launches cost;
  (d) (a) and (c) again, each captured into a HIP graph and replayed;
  (e) the graph step of RDST-E1 x4 bf16 at batch 32 (bench.py's network and batch, one fixed batch) with SRLoss
      {'L1': 0.16, 'SSIM': 0.84} (gaussian 11) against {'L1': 0.16, 'MSSSIM': 0.84} (5 levels).
After `warmup` calls each, blocks of `steps` calls alternate over the variants of a group `reps` times; min / median / max over
the blocks, one JSON line per case.  The lines are printed and written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def git(*args):
    try:
        return subprocess.run(["git", "-C", ROOT, *args], capture_output=True, text=True, timeout=10).stdout.strip() or None
    except (OSError, subprocess.SubprocessError):
        return None


def timed(fn, n):
    """ms per call of ``fn`` over ``n`` calls, between two HIP events on the current stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def torch_ms_ssim_loss(pred, target, taps, weights, data_range=1.0):
    """1 - mean MS-SSIM from torch fp32 ops (cov_norm 1): every window sum is a vertical and a horizontal depthwise conv2d."""
    C = pred.shape[1]
    wv = taps.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1)
    wh = taps.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)
    f = lambda t: F.conv2d(F.conv2d(t, wv, groups=C), wh, groups=C)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ms = None
    M = len(weights)
    for j in range(M):
        if j:
            pred, target = F.avg_pool2d(pred, 2), F.avg_pool2d(target, 2)
        ux, uy, uxx, uyy, uxy = f(target), f(pred), f(target * target), f(pred * pred), f(target * pred)
        term = (2 * (uxy - ux * uy) + C2) / ((uxx - ux * ux) + (uyy - uy * uy) + C2)
        if j == M - 1:
            term = term * (2 * ux * uy + C1) / (ux * ux + uy * uy + C1)
        m = term.mean(dim=(2, 3)) ** weights[j]
        ms = m if ms is None else ms * m
    return 1.0 - ms.mean(dim=1).mean()


def capture(fn):
    """``fn`` captured into a HIP graph after a warm-up on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_loss_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_loss_bench: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    lines = [json.dumps({"tool": "tools/msssim_loss_bench.py", "commit": a.commit or git("rev-parse", "--short", "HEAD"),
                         "parent": a.parent or git("rev-parse", "--short", "HEAD^"),
                         "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                         "workload": "loss: 32 x 1 x 256x256 fp32 (5 levels) and 32 x 1 x 96x96 (4 levels), gaussian 11, forward + "
                                     "backward; step: RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, FlatAdam lr 1e-4, graph",
                         "steps_per_block": a.steps, "blocks": a.reps, "warmup": a.warmup, "cases": a.cases})]
    print(lines[0], flush=True)

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    if set(a.cases) & set("abcd"):
        from rdst_amd.loss import level_weights, ms_ssim_loss, ssim_loss, window_taps
        taps64, _ = window_taps("gaussian", 11)
        taps32 = torch.from_numpy(taps64).to(dev, torch.float32)
        for side_px, levels in ((256, 5), (96, 4)):
            tgt = torch.rand(32, 1, side_px, side_px, generator=g).to(dev)
            pred = (tgt + 0.1 * torch.randn(tgt.shape, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
            wts = [float(v) for v in level_weights(levels)]

            def fused():
                pred.grad = None
                ms_ssim_loss(pred, tgt, levels).backward()

            def composed():
                pred.grad = None
                torch_ms_ssim_loss(pred, tgt, taps32, wts).backward()

            def single():
                pred.grad = None
                ssim_loss(pred, tgt, "gaussian", 11).backward()
            what = {"a": f"rdst_amd.loss.ms_ssim_loss ({2 * levels + 1} launches), forward + backward",
                    "b": "torch fp32 composition (separable depthwise conv2d, avg_pool2d), forward + backward",
                    "c": "rdst_amd.loss.ssim_loss gaussian 11 (single scale, 2 launches), forward + backward",
                    "d_a": "(a) replayed from a HIP graph", "d_c": "(c) replayed from a HIP graph"}
            runs = [(k, fn, []) for k, fn in (("a", fused), ("b", composed), ("c", single)) if k in a.cases]
            got = {}
            for k, fn, _ in runs:
                for _ in range(a.warmup):
                    fn()
                got[k] = pred.grad.clone()
            if "d" in a.cases:
                pred.grad = None
                for k, fn in (("d_a", fused), ("d_c", single)):
                    replay = capture(fn)
                    for _ in range(a.warmup):
                        replay()
                    runs.append((k, replay, []))
            for _ in range(a.reps):
                for _, fn, ms in runs:
                    ms.append(timed(fn, a.steps))
            sp = {}
            for k, _, ms in runs:
                sp[k] = spread(ms)
                emit({"case": k, "shape": [32, 1, side_px, side_px], "levels": levels, "what": what[k], "ms_per_call": sp[k],
                      "blocks_ms": [round(v, 4) for v in ms]})
            if "a" in sp and "b" in sp:
                ga, gb = got["a"], got["b"]
                emit({"shape": [32, 1, side_px, side_px], "levels": levels,
                      "b_over_a_at_median": round(sp["b"]["median"] / sp["a"]["median"], 2),
                      "b_min_minus_a_max_ms": round(sp["b"]["min"] - sp["a"]["max"], 4),
                      "loss_a": float(ms_ssim_loss(pred.detach(), tgt, levels)),
                      "loss_b": float(torch_ms_ssim_loss(pred.detach(), tgt, taps32, wts)),
                      "grad_b_vs_a_max_rel": float((ga - gb).abs().max() / ga.abs().max())})
            if "a" in sp and "c" in sp:
                emit({"shape": [32, 1, side_px, side_px], "levels": levels,
                      "a_over_c_at_median": round(sp["a"]["median"] / sp["c"]["median"], 2),
                      "a_minus_c_ms": round(sp["a"]["median"] - sp["c"]["median"], 4)})
            if "d_a" in sp and "d_c" in sp:
                emit({"shape": [32, 1, side_px, side_px], "levels": levels, "replayed": True,
                      "a_over_c_at_median": round(sp["d_a"]["median"] / sp["d_c"]["median"], 2),
                      "a_minus_c_ms": round(sp["d_a"]["median"] - sp["d_c"]["median"], 4)})

    if "e" in a.cases:
        import bench
        from rdst_amd.loss import SRLoss
        from rdst_amd.trainer import DPTrainStep
        x = torch.rand(32, 1, 64, 64, generator=g).to(dev)
        tgt = torch.rand(32, 1, 256, 256, generator=g).to(dev)

        def trainer(name, **kw):
            sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=["L1", name],
                                              loss_scalars={"S": {"L1": 0.16, name: 0.84}}, training_states=["S"], **kw))
            tr = DPTrainStep(bench.build_net(dev, torch.bfloat16, bench.E1), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0,
                             graph=True, graph_warmup=2, loss_fn=sl)
            for _ in range(a.warmup):
                tr.step(x, tgt)
            torch.cuda.synchronize()
            if tr.graph is None:
                raise SystemExit("msssim_loss_bench: the step was not captured")
            return tr
        runs = [("e_ssim", "graph step, SRLoss {'L1': 0.16, 'SSIM': 0.84} (gaussian 11)", trainer("SSIM", ssim_window="gaussian"), []),
                ("e_msssim", "graph step, SRLoss {'L1': 0.16, 'MSSSIM': 0.84} (5 levels, gaussian 11)", trainer("MSSSIM"), [])]
        for _ in range(a.reps):
            for _, _, tr, ms in runs:
                ms.append(timed(lambda: tr.step(*tr._static), a.steps))
        for key, what, tr, ms in runs:
            emit({"case": key, "what": what, "ms_per_step": spread(ms), "blocks_ms": [round(v, 4) for v in ms],
                  "last_loss": float(tr._loss_buf)})
        s0, s1 = spread(runs[0][3]), spread(runs[1][3])
        emit({"msssim_minus_ssim_ms": round(s1["median"] - s0["median"], 4), "spread_ssim_ms": round(s0["max"] - s0["min"], 4),
              "spread_msssim_ms": round(s1["max"] - s1["min"], 4)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
