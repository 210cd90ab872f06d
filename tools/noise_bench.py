#!/usr/bin/env python3
"""What the noise term costs the device data path (rdst_amd.data.Noise, rdst_sample_patches_noise, rdst_add_noise):
DevicePatchSampler.sample() and DPTrainStep.step_from with the noise off and with each kind, at the benchmark's batch,
32 x 1 x 256x256 -> 64x64 from 512 slices of 320x320.

    python tools/noise_bench.py [--parent DIR] [--iters 20] [--reps 5] [--steps 20] [--no-step] [--bench-steps 20] [--out profiles/noise_bench.txt]

  (a) sample() per degradation ('cubic', 'cubic+gaussian') and noise kind: HIP events around blocks of `iters` calls (draw, the
      pinned copy and the launch included); the blocks alternate `reps` times between the noise-off sampler, the noisy one,
  (b) the same batch composed the other ways: the noise-off sample() followed by torch device ops (torch.randn_like and
      elementwise arithmetic under per-patch levels on the device; this consumes the device generator), and the noise-off
      sample() followed by the whole-image add_noise (two launches and a second pinned copy); medians and ranges are printed;
  (c) step_from: ms/step of RDST-E1 x4 bf16 (bench.py's network, graph replay) through step_from(noisy sampler) against
      step_from(noise-off sampler), blocks of `steps` alternating `reps` times on ONE trainer; `off_spread_ms` is the noise-off
      blocks' own max - min: what the noise adds is to be read against it;
  (d) --parent DIR (a built checkout of the parent commit): plain `python bench.py --gpus 1`, parent / tree alternating three
      times, each run a child process of its own; and sample() with noise=None from both trees (tools/degrade_bench.py
      --child, which both trees have), parent / tree / parent / tree, with one seeded batch hashed: the same bits.
One JSON line per row, to stdout and appended to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tools")]
from degrade_bench import B, LP, SCALE, events, sampler, spread      # noqa: E402  (the batch and the timing of that tool)

DEGRADATIONS = ("cubic", "cubic+gaussian")


def noises(D):
    return {"gaussian": D.Noise("gaussian", sigma=(0.01, 0.05)),
            "poisson-gaussian": D.Noise("poisson-gaussian", gain=(0.0, 0.02), sigma=(0.0, 0.02)),
            "rician": D.Noise("rician", sigma=(0.01, 0.05))}


def torch_noise(kind, lr, lv):
    """The model of `kind` from torch device ops; lv (B, 2) on the device."""
    p0, p1 = lv[:, 0].view(-1, 1, 1, 1), lv[:, 1].view(-1, 1, 1, 1)
    if kind == "rician":
        return torch.sqrt((lr + p0 * torch.randn_like(lr)) ** 2 + (p0 * torch.randn_like(lr)) ** 2)
    return lr + torch.sqrt(p0 * lr.clamp_min(0) + p1 * p1) * torch.randn_like(lr)


def child(root, script, args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(root, script), *args], capture_output=True, text=True, timeout=timeout,
                       cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"noise_bench: {script} in {root} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "noise_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench: no GPU")
    log = open(a.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    if a.parent:      # before this process opens the GPU for long: children one at a time
        par, tree = [], []
        for _ in range(3):
            for root, into in ((a.parent, par), (HERE, tree)):
                into.append(child(os.path.abspath(root), "bench.py", ["--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5"])["ms_per_step"])
        emit({"row": "python bench.py --gpus 1, parent / tree alternating three times", "steps": a.bench_steps,
              "parent_ms_per_step": par, "tree_ms_per_step": tree,
              "ranges_overlap": max(min(par), min(tree)) <= min(max(par), max(tree))})
        runs = [child(os.path.abspath(root), os.path.join("tools", "degrade_bench.py"),
                      ["--child", os.path.abspath(root), "--iters", str(a.iters), "--reps", str(a.reps)], timeout=300)
                for root in (a.parent, HERE, a.parent, HERE)]
        p, t = runs[0]["blocks_ms"] + runs[2]["blocks_ms"], runs[1]["blocks_ms"] + runs[3]["blocks_ms"]
        emit({"row": "sample() noise=None, parent / tree / parent / tree", "batch": [B, 1, int(LP * SCALE), int(LP * SCALE)],
              "parent_ms": spread(p), "tree_ms": spread(t), "parent_spread_ms": round(max(p) - min(p), 4),
              "tree_minus_parent_ms": round(statistics.median(t) - statistics.median(p), 4),
              "bit_equal": len({r["sha256"] for r in runs}) == 1})
    from rdst_amd import data as D
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    hp = int(LP * SCALE)
    kinds = noises(D)
    off = {deg: sampler(D, dev, degradation=deg) for deg in DEGRADATIONS}
    for s in off.values():
        s.hr_images = off["cubic"].hr_images           # one resident stack
    on = {}
    for deg in DEGRADATIONS:
        for kind, nz in kinds.items():
            s = on[deg, kind] = sampler(D, dev, degradation=deg, noise=nz)
            s.hr_images = off["cubic"].hr_images
            b = s.sample()
            lr = D.resample(b["out"], LP, deg)
            assert torch.equal(b["in"], D.add_noise(lr, nz, levels=b["noise_levels"], seed=b["noise_seed"]))
            lv = nz.levels_from(torch.rand(B, 2)).to(dev)

            def torch_way(o=off[deg], kind=kind, lv=lv):
                return torch_noise(kind, o.sample()["in"], lv)

            def two_launches(o=off[deg], nz=nz, g=s.generator):
                x = o.sample()["in"]
                return D.add_noise(x, nz, generator=g, out=x)
            for _ in range(5):
                s.sample(), off[deg].sample(), torch_way(), two_launches()
            tn, to, tt, t2 = [], [], [], []
            for _ in range(a.reps):
                to.append(events(off[deg].sample, a.iters))
                tn.append(events(s.sample, a.iters))
                tt.append(events(torch_way, a.iters))
                t2.append(events(two_launches, a.iters))
            emit({"row": f"sample() {deg!r} + {kind!r}", "batch": [B, 1, hp, hp], "off_ms": spread(to), "noisy_ms": spread(tn),
                  "off_plus_torch_ops_ms": spread(tt), "off_plus_add_noise_ms": spread(t2),
                  "off_spread_ms": round(max(to) - min(to), 4),
                  "noisy_minus_off_ms": round(statistics.median(tn) - statistics.median(to), 4),
                  "torch_over_noisy": round(statistics.median(tt) / statistics.median(tn), 2),
                  "add_noise_way_over_noisy": round(statistics.median(t2) / statistics.median(tn), 2)})
    if a.no_step:
        return
    import bench
    from rdst_amd.trainer import DPTrainStep
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    tr = DPTrainStep(net, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0, graph=True, graph_warmup=2)
    for _ in range(4):
        tr.step_from(off["cubic"])
    for s in on.values():
        tr.step_from(s)
    torch.cuda.synchronize()
    if tr.graph is None:
        raise SystemExit("noise_bench: the step was not captured")

    def block(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step_from(s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    for kind in kinds:
        to, tn = [], []
        for _ in range(a.reps):
            to.append(block(off["cubic"]))
            tn.append(block(on["cubic", kind]))
        emit({"row": f"step_from 'cubic' + {kind!r}", "step": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, graph replay",
              "step_from_off_ms": spread(to), "step_from_noisy_ms": spread(tn), "off_spread_ms": round(max(to) - min(to), 4),
              "noisy_minus_off_ms": round(statistics.median(tn) - statistics.median(to), 4)})


if __name__ == "__main__":
    main()
