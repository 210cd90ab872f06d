#!/usr/bin/env python3
"""What the SSIM training loss costs: the fused kernel against the same loss composed of torch ops, and the training step
with and without it.

    python tools/ssim_loss_bench.py [--steps 20] [--reps 5] [--warmup 6] [--cases abcd] [--out profiles/ssim_loss_bench.txt]
                                    [--commit NAME] [--parent NAME]

The protocol of tools/ema_bench.py, HIP events around every block:
  (a) rdst_amd.loss.ssim_loss forward + backward at 32 x 1 x 256 x 256, uniform 7 and gaussian 11: 2 kernel launches + the
      upstream multiply;
  (b) the same loss composed of torch fp32 device ops (five depthwise separable conv2d pairs and the SSIM expression),
      forward + backward through autograd;
  (c) the graph step of RDST-E1 x4 bf16 at batch 32 (bench.py's network and batch, one fixed batch) with L1 alone;
  (d) the same step with SRLoss {'L1': 0.16, 'SSIM': 0.84}.
After `warmup` calls each, blocks of `steps` calls alternate over the variants of a group ((a) and (b); (c) and (d)) `reps`
times; min / median / max over the blocks, one JSON line per case.  `--cases c` runs on a tree without the loss too: (c) of
the parent commit and (c) of this tree, measured in one session, must agree within the spread the blocks show among
themselves.  The lines are printed and written to --out."""
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


def torch_ssim_loss(pred, target, taps, cov_norm, data_range=1.0):
    """1 - mean SSIM from torch fp32 ops: every window sum is a vertical and a horizontal depthwise conv2d."""
    C = pred.shape[1]
    wv = taps.reshape(1, 1, -1, 1).repeat(C, 1, 1, 1)
    wh = taps.reshape(1, 1, 1, -1).repeat(C, 1, 1, 1)
    f = lambda t: F.conv2d(F.conv2d(t, wv, groups=C), wh, groups=C)
    ux, uy, uxx, uyy, uxy = f(target), f(pred), f(target * target), f(pred * pred), f(target * pred)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return 1.0 - S.mean(dim=(1, 2, 3)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_loss_bench: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(32, 1, 64, 64, generator=g).to(dev)
    tgt = torch.rand(32, 1, 256, 256, generator=g).to(dev)
    lines = [json.dumps({"tool": "tools/ssim_loss_bench.py", "commit": a.commit or git("rev-parse", "--short", "HEAD"),
                         "parent": a.parent or git("rev-parse", "--short", "HEAD^"),
                         "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                         "workload": "loss: 32 x 1 x 256x256 fp32, forward + backward; step: RDST-E1 x4 bf16, 32 x 1 x 64x64 -> "
                                     "256x256, FlatAdam lr 1e-4, graph",
                         "steps_per_block": a.steps, "blocks": a.reps, "warmup": a.warmup, "cases": a.cases})]
    print(lines[0], flush=True)

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    if set(a.cases) & set("ab"):
        from rdst_amd.loss import ssim_loss, window_taps
        pred = (tgt + 0.1 * torch.randn(tgt.shape, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
        for window, win in (("uniform", 7), ("gaussian", 11)):
            taps64, cn = window_taps(window, win)
            taps32 = torch.from_numpy(taps64).to(dev, torch.float32)

            def fused():
                pred.grad = None
                ssim_loss(pred, tgt, window, win).backward()

            def composed():
                pred.grad = None
                torch_ssim_loss(pred, tgt, taps32, cn).backward()
            runs = [(k, fn, []) for k, fn in (("a", fused), ("b", composed)) if k in a.cases]
            got = {}
            for k, fn, _ in runs:
                for _ in range(a.warmup):
                    fn()
                got[k] = (float(ssim_loss(pred.detach(), tgt, window, win)) if k == "a" else
                          float(torch_ssim_loss(pred.detach(), tgt, taps32, cn)), pred.grad.clone())
            for _ in range(a.reps):
                for _, fn, ms in runs:
                    ms.append(timed(fn, a.steps))
            what = {"a": "rdst_amd.loss.ssim_loss (one HIP kernel + finish), forward + backward",
                    "b": "torch fp32 composition (separable depthwise conv2d), forward + backward"}
            for k, _, ms in runs:
                emit({"case": k, "window": window, "win": win, "what": what[k], "ms_per_call": spread(ms),
                      "blocks_ms": [round(v, 4) for v in ms], "loss": got[k][0]})
            if len(runs) == 2:
                sa, sb = spread(runs[0][2]), spread(runs[1][2])
                ga, gb = got["a"][1], got["b"][1]
                emit({"window": window, "win": win, "b_over_a_at_median": round(sb["median"] / sa["median"], 2),
                      "b_min_minus_a_max_ms": round(sb["min"] - sa["max"], 4),
                      "spread_a_ms": round(sa["max"] - sa["min"], 4), "spread_b_ms": round(sb["max"] - sb["min"], 4),
                      "grad_b_vs_a_max_rel": float((ga - gb).abs().max() / ga.abs().max())})

    if set(a.cases) & set("cd"):
        import bench
        from rdst_amd.trainer import DPTrainStep

        def trainer(loss_fn):
            tr = DPTrainStep(bench.build_net(dev, torch.bfloat16, bench.E1), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0,
                             graph=True, graph_warmup=2, loss_fn=loss_fn)
            for _ in range(a.warmup):
                tr.step(x, tgt)
            torch.cuda.synchronize()
            if tr.graph is None:
                raise SystemExit("ssim_loss_bench: the step was not captured")
            return tr
        runs = []
        if "c" in a.cases:
            runs.append(("c", "graph step, L1 alone", trainer(None), []))
        if "d" in a.cases:
            from rdst_amd.loss import SRLoss
            sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=["L1", "SSIM"],
                                              loss_scalars={"S": {"L1": 0.16, "SSIM": 0.84}}, training_states=["S"]))
            runs.append(("d", "graph step, SRLoss {'L1': 0.16, 'SSIM': 0.84} (uniform 7)", trainer(sl), []))
        for _ in range(a.reps):
            for _, _, tr, ms in runs:
                ms.append(timed(lambda: tr.step(*tr._static), a.steps))
        for key, what, tr, ms in runs:
            emit({"case": key, "what": what, "ms_per_step": spread(ms), "blocks_ms": [round(v, 4) for v in ms],
                  "last_loss": float(tr._loss_buf)})
        if len(runs) == 2:
            sc, sd = spread(runs[0][3]), spread(runs[1][3])
            emit({"d_minus_c_ms": round(sd["median"] - sc["median"], 4), "spread_c_ms": round(sc["max"] - sc["min"], 4),
                  "spread_d_ms": round(sd["max"] - sd["min"], 4)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
