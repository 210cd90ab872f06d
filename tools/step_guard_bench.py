#!/usr/bin/env python3
"""What the update guard of the reference's inner loop (models/trans_sr_trainer.py:162-174) costs a training step, on the
host and on the device.

    python tools/step_guard_bench.py [--steps 20] [--reps 5] [--warmup 6] [--out profiles/step_guard_bench.txt]
                                     [--commit NAME] [--parent NAME]

ms/step of RDST-E1 x4 in bf16 at batch 32 (bench.py's network and batch, one fixed batch) for five trainers in one process:
  (a) DPTrainStep(graph=True):                                   today's unguarded step, graph replay + one Adam launch;
  (b) DPTrainStep(loss_threshold=1e7):                           today's host guard: eager, one loss.item() per step;
  (c) DPTrainStep(device_guard=True, graph=True, loss_threshold=1e7):   the decision, Adam and the schedule in the graph;
  (d) as (c) + skip_nonfinite=True:                              adds the fp64 sum-of-squares pass over the bucket;
  (e) as (d) + max_grad_norm=1.0:                                the same pass, the coefficient applied inside Adam.
After `warmup` steps each (lazy initialisation, graph capture), blocks of `steps` steps alternate over the five trainers
`reps` times; wall time around a block with a device synchronisation on both sides.  min / median / max over the blocks,
one JSON line per case, then the ratios.  The lines are printed and written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    ("a", "unguarded graph step", dict(graph=True)),
    ("b", "host guard, eager (loss_threshold=1e7)", dict(loss_threshold=1e7)),
    ("c", "device guard in the graph (loss_threshold=1e7)", dict(device_guard=True, graph=True, loss_threshold=1e7)),
    ("d", "(c) + skip_nonfinite", dict(device_guard=True, graph=True, loss_threshold=1e7, skip_nonfinite=True)),
    ("e", "(d) + max_grad_norm=1.0", dict(device_guard=True, graph=True, loss_threshold=1e7, skip_nonfinite=True,
                                          max_grad_norm=1.0)),
]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def git(*args):
    try:
        return subprocess.run(["git", "-C", ROOT, *args], capture_output=True, text=True, timeout=10).stdout.strip() or None
    except (OSError, subprocess.SubprocessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_guard_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_guard_bench: no GPU")
    import bench
    from rdst_amd.trainer import DPTrainStep
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(32, 1, 64, 64, generator=g).to(dev)
    tgt = torch.rand(32, 1, 256, 256, generator=g).to(dev)
    lines = [json.dumps({"tool": "tools/step_guard_bench.py", "commit": a.commit or git("rev-parse", "--short", "HEAD"),
                         "parent": a.parent or git("rev-parse", "--short", "HEAD^"),
                         "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                         "workload": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, L1, FlatAdam lr 1e-4",
                         "steps_per_block": a.steps, "blocks": a.reps, "warmup": a.warmup})]
    print(lines[0], flush=True)
    runs = []
    for key, what, kw in CASES:
        tr = DPTrainStep(bench.build_net(dev, torch.bfloat16, bench.E1), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0,
                         graph_warmup=2, **kw)
        for _ in range(a.warmup):
            tr.step(x, tgt)
        torch.cuda.synchronize()
        if kw.get("graph") and tr.graph is None:
            raise SystemExit(f"step_guard_bench: case ({key}) was not captured")
        runs.append((key, what, tr, tr._static if tr.graph is not None else (x, tgt), []))

    def block(tr, batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step(*batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    for _ in range(a.reps):
        for _, _, tr, batch, ms in runs:
            ms.append(block(tr, batch))
    med = {}
    for key, what, tr, _, ms in runs:
        med[key] = statistics.median(ms)
        rec = {"case": key, "what": what, "ms_per_step": spread(ms), "graph": tr.graph is not None,
               "update_in_graph": bool(tr._graph_has_update)}
        if tr.device_guard:
            st = tr.guard_stats()
            rec.update(kept=st["kept"], skipped=st["skipped"], last_grad_norm=st["last_grad_norm"], last_clip=st["last_clip"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"c_over_a": round(med["c"] / med["a"], 4), "c_over_b": round(med["c"] / med["b"], 4),
                             "d_minus_c_ms": round(med["d"] - med["c"], 4), "e_minus_d_ms": round(med["e"] - med["d"], 4),
                             "b_minus_a_ms": round(med["b"] - med["a"], 4)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
