#!/usr/bin/env python3
"""What the weight EMA costs a training step, an exchange and a quick validation.

    python tools/ema_bench.py [--steps 20] [--reps 5] [--warmup 6] [--cases abcd] [--out profiles/ema_bench.txt]
                              [--commit NAME] [--parent NAME]

RDST-E1 x4 in bf16 at batch 32 (bench.py's network and batch, one fixed batch), the protocol of tools/step_guard_bench.py
with HIP events around every block:
  (a) DPTrainStep(device_guard=True, graph=True):                  the whole step is one graph replay, no EMA;
  (b) as (a) + ema_decay=0.999:                                    the Adam node reads and writes one more flat buffer;
  (c) one swap_ema() pair on (b)'s optimizer:                      2 launches, 2 x 16 bytes per parameter;
  (d) quick_eva on (b)'s trainer, live against averaged weights:   the same forwards, plus (c) around them.
After `warmup` steps each (lazy initialisation, graph capture), blocks of `steps` steps alternate over (a) and (b) `reps`
times; (c) and (d) alternate their two variants the same way.  min / median / max over the blocks, one JSON line per case.
`--cases a` runs on a tree without the EMA too: (a) of the parent commit and (a) of this tree, measured in one session, must
agree within the spread the blocks show among themselves.  The lines are printed and written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no GPU")
    import bench
    from rdst_amd.trainer import DPTrainStep
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(32, 1, 64, 64, generator=g).to(dev)
    tgt = torch.rand(32, 1, 256, 256, generator=g).to(dev)
    lines = [json.dumps({"tool": "tools/ema_bench.py", "commit": a.commit or git("rev-parse", "--short", "HEAD"),
                         "parent": a.parent or git("rev-parse", "--short", "HEAD^"),
                         "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                         "workload": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, L1, FlatAdam lr 1e-4, device guard, graph",
                         "steps_per_block": a.steps, "blocks": a.reps, "warmup": a.warmup, "cases": a.cases})]
    print(lines[0], flush=True)

    def trainer(**kw):
        tr = DPTrainStep(bench.build_net(dev, torch.bfloat16, bench.E1), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0,
                         graph=True, graph_warmup=2, device_guard=True, **kw)
        for _ in range(a.warmup):
            tr.step(x, tgt)
        torch.cuda.synchronize()
        if tr.graph is None or not tr._graph_has_update:
            raise SystemExit("ema_bench: the step was not captured with its update")
        return tr
    runs = []
    if "a" in a.cases:
        runs.append(("a", "device-guard graph step, no EMA", trainer(), []))
    ema_tr = None
    if set(a.cases) & set("bcd"):
        ema_tr = trainer(ema_decay=0.999)
        if "b" in a.cases:
            runs.append(("b", "(a) + ema_decay=0.999", ema_tr, []))
    for _ in range(a.reps):
        for _, _, tr, ms in runs:
            ms.append(timed(lambda: tr.step(*tr._static), a.steps))
    med = {}
    for key, what, tr, ms in runs:
        med[key] = statistics.median(ms)
        n = tr.optimizer.flat_param.numel()
        lines.append(json.dumps({"case": key, "what": what, "ms_per_step": spread(ms), "blocks_ms": [round(v, 4) for v in ms],
                                 "parameters": n, "adam_bytes_per_step": n * (36 if getattr(tr.optimizer, "ema", None) is not None else 28),
                                 "kept": tr.guard_stats()["kept"]}))
        print(lines[-1], flush=True)
    if "a" in med and "b" in med:
        sa, sb = spread(runs[0][3]), spread(runs[1][3])
        lines.append(json.dumps({"b_minus_a_ms": round(med["b"] - med["a"], 4),
                                 "spread_a_ms": round(sa["max"] - sa["min"], 4), "spread_b_ms": round(sb["max"] - sb["min"], 4)}))
        print(lines[-1], flush=True)
    if "c" in a.cases:
        opt = ema_tr.optimizer
        n = opt.flat_param.numel()

        def pair():
            opt.swap_ema()
            opt.swap_ema()
        pair()
        ms = [timed(pair, a.steps) for _ in range(a.reps)]
        s = spread(ms)
        lines.append(json.dumps({"case": "c", "what": "one swap_ema() pair", "ms_per_pair": s, "bytes_per_pair": 32 * n,
                                 "GB_per_s_at_median": round(32 * n / s["median"] / 1e6, 1)}))
        print(lines[-1], flush=True)
    if "d" in a.cases:
        gv = torch.Generator().manual_seed(7)
        lr_v, hr_v = torch.rand(16, 1, 64, 64, generator=gv).to(dev), torch.rand(16, 1, 256, 256, generator=gv).to(dev)
        ms = {False: [], True: []}
        for use in (False, True):          # lazy initialisation of the eval forward and the scorer
            ema_tr.quick_eva(lr_v, hr_v, num_samples=16, batch_size=4, generator=torch.Generator().manual_seed(0), use_ema=use)
        for _ in range(a.reps):
            for use in (False, True):
                ms[use].append(timed(lambda: ema_tr.quick_eva(lr_v, hr_v, num_samples=16, batch_size=4,
                                                              generator=torch.Generator().manual_seed(0), use_ema=use), 2))
        lines.append(json.dumps({"case": "d", "what": "quick_eva, 16 slices 64x64 -> 256x256, one chunk",
                                 "live_ms": spread(ms[False]), "ema_ms": spread(ms[True]),
                                 "ema_minus_live_ms": round(statistics.median(ms[True]) - statistics.median(ms[False]), 4)}))
        print(lines[-1], flush=True)
        ema_tr.step(*ema_tr._static)       # the captured step still replays after the evaluations
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
