#!/usr/bin/env python3
"""What the LR-consistency loss and the back-projection cost: the fused kernels against the composed path and against torch's
own bicubic, the training step with and without the loss, and the tester with and without back-projection.

    python tools/consistency_bench.py [--steps 20] [--reps 5] [--warmup 6] [--cases abcdef]
                                      [--out profiles/consistency_bench.txt] [--commit NAME] [--parent NAME]

The protocol of tools/ssim_loss_bench.py, HIP events around every block:
  (f) rdst_amd.loss.lr_consistency_loss forward + backward at 32 x 1 x 256 x 256 -> 64 x 64, L1, per degradation: 3 launches;
  (a) the composed path: data.degrade (rdst_resample_sep forwards, the transposed tables backwards: 4 launches) and torch
      elementwise operations for |.|, the mean and their gradient;
  (b) 'cubic' only: F.interpolate(mode='bicubic') + F.l1_loss under torch autograd;
  (c) the graph step of RDST-E1 x4 bf16 at batch 32 (bench.py's network and batch, one fixed batch) with SRLoss {'L1': 1};
  (d) the same step with SRLoss {'L1': 1, 'LRC': 0.1};
  (e) SRTester.inference of 32 slices of 64 x 64 (RDST-E1 x4 bf16, whole slices) with back_project 0 and 3, 'cubic'.
(f), (a) and (b) are timed twice: called eagerly (`ms_per_call`: at these sizes the host's share, not the device's) and as replays
of one HIP graph each (`ms_per_graph_replay`: what the training step pays).
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


def captured(fn):
    """``fn`` as a replay of ONE HIP graph (what the loss costs the device, without the host's share), or None."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            fn()
    except Exception as e:  # noqa: BLE001 - reported, not fatal
        print(f"consistency_bench: capture failed ({type(e).__name__}: {e})", file=sys.stderr)
        torch.cuda.synchronize()
        return None
    return graph.replay


def alternate(runs, reps, steps):
    for _ in range(reps):
        for *_, fn, ms in runs:
            ms.append(timed(fn, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--cases", default="abcdef")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench: no GPU")
    from rdst_amd import data as D
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(32, 1, 64, 64, generator=g).to(dev)
    tgt = torch.rand(32, 1, 256, 256, generator=g).to(dev)
    lines = [json.dumps({"tool": "tools/consistency_bench.py", "commit": a.commit or git("rev-parse", "--short", "HEAD"),
                         "parent": a.parent or git("rev-parse", "--short", "HEAD^"),
                         "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                         "workload": "loss: 32 x 1 x 256x256 -> 64x64 fp32, L1, forward + backward; step: RDST-E1 x4 bf16, 32 x 1 x "
                                     "64x64 -> 256x256, FlatAdam lr 1e-4, graph; tester: 32 slices of 64x64, whole slices",
                         "steps_per_block": a.steps, "blocks": a.reps, "warmup": a.warmup, "cases": a.cases})]
    print(lines[0], flush=True)

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    if set(a.cases) & set("abf"):
        from rdst_amd.loss import lr_consistency_loss
        pred = (tgt + 0.1 * torch.randn(tgt.shape, generator=g).to(dev)).requires_grad_(True)
        for kind in D.KINDS:
            lr = D.resample(tgt, (64, 64), kind)

            def fused():
                pred.grad = None
                lr_consistency_loss(pred, lr, kind).backward()

            def composed():
                pred.grad = None
                (D.degrade(pred, (64, 64), kind) - lr).abs().mean().backward()

            def torch_bicubic():
                pred.grad = None
                F.l1_loss(F.interpolate(pred, size=(64, 64), mode="bicubic", align_corners=False), lr).backward()
            what = {"f": "rdst_amd.loss.lr_consistency_loss (residual + finish, adjoint), forward + backward",
                    "a": "data.degrade (resample / resample_adjoint) + torch elementwise, forward + backward",
                    "b": "F.interpolate(bicubic) + F.l1_loss under torch autograd, forward + backward"}
            fns = {"f": fused, "a": composed, "b": torch_bicubic}
            runs = [(k, fns[k], []) for k in "fab" if k in a.cases and (k != "b" or kind == "cubic")]
            grads = {}
            for k, fn, _ in runs:
                for _ in range(a.warmup):
                    fn()
                grads[k] = pred.grad.clone()
            alternate(runs, a.reps, a.steps)
            replays = [(k, r, []) for k, r in ((k, captured(fn)) for k, fn, _ in runs) if r is not None]
            for _, r, _ in replays:
                r()
            alternate(replays, a.reps, a.steps)
            in_graph = {k: spread(ms) for k, _, ms in replays}
            for k, _, ms in runs:
                emit({"case": k, "degradation": kind, "what": what[k], "ms_per_call": spread(ms),
                      "blocks_ms": [round(v, 4) for v in ms], "ms_per_graph_replay": in_graph.get(k)})
            sp = {k: spread(ms) for k, _, ms in runs}
            if "f" in sp:
                for k in sp:
                    if k != "f":
                        emit({"degradation": kind, f"{k}_over_f_at_median": round(sp[k]["median"] / sp["f"]["median"], 2),
                              f"{k}_min_minus_f_max_ms": round(sp[k]["min"] - sp["f"]["max"], 4),
                              f"{k}_over_f_in_graph": (round(in_graph[k]["median"] / in_graph["f"]["median"], 2)
                                                       if k in in_graph and "f" in in_graph else None),
                              f"grad_{k}_equals_f": bool(torch.equal(grads[k], grads["f"])),
                              f"grad_{k}_vs_f_max_rel": float((grads[k] - grads["f"]).abs().max() / grads["f"].abs().max())})

    if set(a.cases) & set("cd"):
        import bench
        from rdst_amd.loss import SRLoss
        from rdst_amd.trainer import DPTrainStep

        def trainer(names, scalars):
            sl = SRLoss(types.SimpleNamespace(gpu_id=0, precision=False, training_losses=names, sr_scale=4,
                                              loss_scalars={"S": scalars}, training_states=["S"]))
            tr = DPTrainStep(bench.build_net(dev, torch.bfloat16, bench.E1), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0,
                             graph=True, graph_warmup=2, loss_fn=sl)
            for _ in range(a.warmup):
                tr.step(x, tgt)
            torch.cuda.synchronize()
            if tr.graph is None:
                raise SystemExit("consistency_bench: the step was not captured")
            return tr
        runs = []
        if "c" in a.cases:
            tr_c = trainer(["L1"], {"L1": 1.0})
            runs.append(("c", "graph step, SRLoss {'L1': 1}", tr_c, lambda: tr_c.step(*tr_c._static), []))
        if "d" in a.cases:
            tr_d = trainer(["L1", "LRC"], {"L1": 1.0, "LRC": 0.1})
            runs.append(("d", "graph step, SRLoss {'L1': 1, 'LRC': 0.1} ('cubic', L1)", tr_d, lambda: tr_d.step(*tr_d._static), []))
        alternate(runs, a.reps, a.steps)
        for key, what, tr, _, ms in runs:
            emit({"case": key, "what": what, "ms_per_step": spread(ms), "blocks_ms": [round(v, 4) for v in ms],
                  "last_loss": float(tr._loss_buf)})
        if len(runs) == 2:
            sc, sd = spread(runs[0][4]), spread(runs[1][4])
            emit({"d_minus_c_ms": round(sd["median"] - sc["median"], 4), "spread_c_ms": round(sc["max"] - sc["min"], 4),
                  "spread_d_ms": round(sd["max"] - sd["min"], 4)})

    if "e" in a.cases:
        import bench
        from rdst_amd.tester import SRTester
        net = bench.build_net(dev, torch.bfloat16, bench.E1)
        lr = D.resample(tgt, (64, 64), "cubic")
        testers = {k: SRTester(net, batch_size=8, back_project=k, degradation="cubic") for k in (0, 3)}
        runs = [(k, (lambda t=t: t.inference(lr)), []) for k, t in testers.items()]
        rms = {}
        for k, fn, _ in runs:
            for _ in range(max(2, a.warmup // 2)):
                out = fn()
            rms[k] = float((D.resample(out.float(), (64, 64), "cubic") - lr).double().pow(2).mean().sqrt())
        alternate(runs, a.reps, a.steps)
        for k, _, ms in runs:
            sp = spread(ms)
            emit({"case": "e", "back_project": k, "ms_per_call": sp, "blocks_ms": [round(v, 4) for v in ms],
                  "slices_per_s": {"median": round(32e3 / sp["median"], 1), "min": round(32e3 / sp["max"], 1),
                                   "max": round(32e3 / sp["min"], 1)}, "rms_lr_residual": rms[k]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
