#!/usr/bin/env python3
"""What a degradation other than the plain cubic resize costs the device data path (rdst_amd.data.Degradation,
rdst_sample_patches_op): DevicePatchSampler.sample() and DPTrainStep.step_from per kind, at the benchmark's batch,
32 x 1 x 256x256 -> 64x64 from 512 slices of 320x320.

    python tools/degrade_bench.py [--parent DIR] [--iters 20] [--reps 5] [--steps 20] [--no-step] [--out profiles/degrade_bench.txt]

  (a) sample() per kind:   HIP events around blocks of `iters` calls (draw, the pinned copy and the launch included); per kind the
                           blocks alternate `reps` times between the kind, the 'cubic' sampler of this tree and the same batch
                           composed of torch device ops (advanced-index crop, then F.interpolate(bicubic) + a reflect-padded
                           conv2d, F.interpolate(bicubic, antialias=True), or torch.fft.rfft2 / irfft2 with the kept bins); the
                           median and the range of the blocks are printed, and the largest difference to the torch composition;
  (b) step_from per kind:  ms/step of RDST-E1 x4 bf16 (bench.py's network, graph replay) through step_from(sampler of the
                           kind) against step_from('cubic' sampler), blocks of `steps` alternating `reps` times on ONE trainer;
                           `cubic_spread_ms` is the cubic blocks' own max - min: what a kind adds is to be read against it;
  (c) --parent DIR:        sample() with 'cubic' from a built checkout of the parent commit in DIR and from this tree, each in a
                           child process of its own (one GPU, one session), in the order parent / tree / parent / tree, `reps`
                           blocks each; the children also hash one seeded batch: the two trees must give the same bits.
One JSON line per row, to stdout and appended to --out."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, LP, SCALE, S, H, W = 32, 1, 64, 4.0, 512, 320, 320
KINDS = ("cubic+gaussian", "cubic_aa", "fourier")


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


def sampler(D, dev, seed=2, **kw):
    host = torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(1))
    return D.DevicePatchSampler(host, B, LP, sr_scales=(SCALE,), device=dev, generator=torch.Generator().manual_seed(seed), **kw)


def cubic_child(a):
    """--child ROOT: the plain sampler of the tree in ROOT (the parent has no `degradation`): one hash, `reps` blocks."""
    sys.path.insert(0, a.child)
    from rdst_amd import data as D
    assert os.path.dirname(os.path.dirname(os.path.abspath(D.__file__))) == os.path.abspath(a.child)
    dev = torch.device("cuda:0")
    s = sampler(D, dev)
    b = s.sample()
    digest = hashlib.sha256(b["in"].cpu().numpy().tobytes() + b["out"].cpu().numpy().tobytes()).hexdigest()
    for _ in range(5):
        s.sample()
    print(json.dumps({"root": a.child, "sha256": digest, "blocks_ms": [events(s.sample, a.iters) for _ in range(a.reps)]}))


def torch_degrade(kind, hr, lp, gk):
    if kind == "cubic":
        return F.interpolate(hr, size=(lp, lp), mode="bicubic", align_corners=False)
    if kind == "cubic+gaussian":
        r = F.interpolate(hr, size=(lp, lp), mode="bicubic", align_corners=False)
        return F.conv2d(F.pad(r, (1, 1, 1, 1), mode="reflect"), gk)
    if kind == "cubic_aa":
        return F.interpolate(hr, size=(lp, lp), mode="bicubic", align_corners=False, antialias=True)
    n, h = hr.shape[-1], lp // 2                     # 'fourier', even lp < n: rows 0..h-1, the folded row h, rows -h+1..-1
    X = torch.fft.rfft2(hr)
    rows = torch.cat([X[..., :h, :], X[..., h:h + 1, :] + X[..., n - h:n - h + 1, :], X[..., n - h + 1:, :]], dim=-2)
    Y = rows[..., :h + 1].clone()
    Y[..., h] *= 2
    return torch.fft.irfft2(Y, s=(lp, lp)) * (lp * lp / (n * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "degrade_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench: no GPU")
    if a.child:
        return cubic_child(a)
    log = open(a.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    if a.parent:      # before this process opens the GPU for long: children one at a time
        runs = []
        for root in (a.parent, HERE, a.parent, HERE):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(root), "--iters", str(a.iters),
                                "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"degrade_bench: the child for {root} failed:\n{r.stdout}\n{r.stderr}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        par = runs[0]["blocks_ms"] + runs[2]["blocks_ms"]
        tree = runs[1]["blocks_ms"] + runs[3]["blocks_ms"]
        emit({"row": "sample() 'cubic', parent / tree / parent / tree", "batch": [B, C, int(LP * SCALE), int(LP * SCALE)],
              "parent_ms": spread(par), "tree_ms": spread(tree), "parent_spread_ms": round(max(par) - min(par), 4),
              "tree_minus_parent_ms": round(statistics.median(tree) - statistics.median(par), 4),
              "bit_equal": len({r["sha256"] for r in runs}) == 1})
    sys.path.insert(0, HERE)
    from rdst_amd import data as D
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    hp = int(LP * SCALE)
    cubic = sampler(D, dev)
    ar_c, ar_p = torch.arange(C, device=dev), torch.arange(hp, device=dev)
    g = torch.tensor([0.25, 0.5, 0.25], device=dev)
    gk = (g[:, None] * g[None, :])[None, None]

    def torch_batch(kind, d):
        idx = d.indices.to(dev, non_blocking=True).long()
        rows, cols = idx[:, 1, None] + ar_p, idx[:, 2, None] + ar_p
        hr = cubic.hr_images[idx[:, 0, None, None, None], ar_c[None, :, None, None], rows[:, None, :, None], cols[:, None, None, :]]
        return torch_degrade(kind, hr, LP, gk), hr

    samplers = {}
    for kind in KINDS:
        s = samplers[kind] = sampler(D, dev, degradation=kind)
        s.hr_images = cubic.hr_images           # one resident stack
        d = s.draw()
        b = s.sample(draw=d)
        tl, th = torch_batch(kind, d)
        assert torch.equal(th, b["out"]) and torch.equal(b["in"], D.resample(b["out"], LP, kind))
        dmax = (tl - b["in"]).abs().max().item()
        for _ in range(5):
            s.sample(), cubic.sample(), torch_batch(kind, s.draw())
        tk, tc, tt = [], [], []
        for _ in range(a.reps):
            tk.append(events(s.sample, a.iters))
            tc.append(events(cubic.sample, a.iters))
            tt.append(events(lambda: torch_batch(kind, s.draw()), a.iters))
        emit({"row": f"sample() {kind!r}", "batch": [B, C, hp, hp], "taps": D.operator_table(kind, hp, LP)[0].shape[1],
              "kind_ms": spread(tk), "cubic_ms": spread(tc), "torch_ops_ms": spread(tt),
              "kind_minus_cubic_ms": round(statistics.median(tk) - statistics.median(tc), 4),
              "torch_over_kind": round(statistics.median(tt) / statistics.median(tk), 2), "max_abs_diff_to_torch_fp32": dmax})
    if a.no_step:
        return
    import bench
    from rdst_amd.trainer import DPTrainStep
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    tr = DPTrainStep(net, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0, graph=True, graph_warmup=2)
    for _ in range(4):
        tr.step_from(cubic)
    for s in samplers.values():
        tr.step_from(s)
    torch.cuda.synchronize()
    if tr.graph is None:
        raise SystemExit("degrade_bench: the step was not captured")

    def block(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step_from(s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    for kind, s in samplers.items():
        tc, tk = [], []
        for _ in range(a.reps):
            tc.append(block(cubic))
            tk.append(block(s))
        emit({"row": f"step_from {kind!r}", "step": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, graph replay",
              "step_from_cubic_ms": spread(tc), "step_from_kind_ms": spread(tk), "cubic_spread_ms": round(max(tc) - min(tc), 4),
              "kind_minus_cubic_ms": round(statistics.median(tk) - statistics.median(tc), 4)})


if __name__ == "__main__":
    main()
