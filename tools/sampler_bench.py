#!/usr/bin/env python3
"""A training batch cut and degraded on the device: rdst_amd.data.DevicePatchSampler.sample() (one HIP launch) against the
same batch from torch device ops and against the reference's recipe on the CPU.

    python tools/sampler_bench.py [--iters 50] [--reps 5] [--cpu-iters 5] [--steps 20] [--no-step]

Per setting, on seeded synthetic slices:
  (a) sample():            HIP events around `iters` calls (index draw, the 3 B integers' copy and the launch included);
  (b) torch device ops:    the same draws, advanced-index crop + F.interpolate(bicubic) on the resident stack, timed the same
                           way; (a) and (b) alternate `reps` times in one process, the median and the range are printed;
  (c) the CPU recipe:      wall time of datasets/basic_dataset.py:190-217 with torch's CPU interpolate at 16 threads in place of
                           cv2.resize (per-slice crop, per-patch resize, stack) plus the copy of both tensors to the device.
Settings: 32 x 1 x 256x256 at ratio 4 from 512 slices of 320x320 (the benchmark's patch), 32 x 1 x 96x96 at ratio 4 from 256
slices of 176x208 (the shipped ini's), 8 x 3 x 256x256 at ratio 2 from 64 slices of 320x320.  `bytes` is what a batch must move
at least: B C (2 hp^2 + lp^2) 4.  One JSON line per setting.
Then ms/step of RDST-E1 x4 in bf16 (bench.py's network and batch, graph replay) through step_from(sampler) against step()
on a fixed batch already in the graph's tensors, alternating blocks of `steps` in one process: the difference is what a
sampled batch costs a training step."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rdst_amd import data as D  # noqa: E402

# (B, C, lp, scale, S, H, W)
SETTINGS = [(32, 1, 64, 4.0, 512, 320, 320), (32, 1, 24, 4.0, 256, 176, 208), (8, 3, 128, 2.0, 64, 320, 320)]


def torch_batch(s, d, ar_c, ar_p):
    """The batch of draw `d` from torch device ops on the sampler's resident stack."""
    idx = d.indices.to(s.device, non_blocking=True).long()
    rows = idx[:, 1, None] + ar_p
    cols = idx[:, 2, None] + ar_p
    hr = s.hr_images[idx[:, 0, None, None, None], ar_c[None, :, None, None], rows[:, None, :, None], cols[:, None, None, :]]
    lr = F.interpolate(hr, size=(s.lr_patch_size, s.lr_patch_size), mode="bicubic", align_corners=False)
    return lr, hr


def cpu_batch(host, d, lp, dev):
    """BasicMultiSRTrain.__getitem__ on the host (torch's CPU bicubic for cv2.resize) + the copy to the device."""
    hp = d.hr_patch_size
    outs = [host[sl, :, t:t + hp, l:l + hp] for sl, t, l in d.indices.tolist()]
    ins = [F.interpolate(o[None], size=(lp, lp), mode="bicubic", align_corners=False)[0] for o in outs]
    return torch.stack(ins).to(dev), torch.stack(outs).to(dev)


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
    ap.add_argument("--cpu-iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench: no GPU")
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    for B, C, lp, scale, S, H, W in SETTINGS:
        host = torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(1))
        s = D.DevicePatchSampler(host, B, lp, sr_scales=(scale,), device=dev, generator=torch.Generator().manual_seed(2))
        hp = int(lp * scale)
        ar_c, ar_p = torch.arange(C, device=dev), torch.arange(hp, device=dev)
        d = s.draw()
        b = s.sample(draw=d)
        tl, th = torch_batch(s, d, ar_c, ar_p)
        assert torch.equal(th, b["out"])
        dmax = (tl - b["in"]).abs().max().item()
        for _ in range(5):
            s.sample()
            torch_batch(s, s.draw(), ar_c, ar_p)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(events(s.sample, a.iters))
            tb.append(events(lambda: torch_batch(s, s.draw(), ar_c, ar_p), a.iters))
        # the launch alone: a fixed draw, outputs the caller owns (no allocation)
        out = (b["in"], b["out"])
        tk = [events(lambda: s.sample(out=out, draw=d), a.iters) for _ in range(a.reps)]
        cpu_batch(host, d, lp, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.cpu_iters):
            cpu_batch(host, s.draw(), lp, dev)
        torch.cuda.synchronize()
        cpu_ms = (time.perf_counter() - t0) * 1e3 / a.cpu_iters
        nbytes = B * C * (2 * hp * hp + lp * lp) * 4
        print(json.dumps({"batch": [B, C, hp, hp], "ratio": scale, "slices": [S, H, W], "bytes": nbytes,
                          "sample_ms": spread(ta), "torch_ops_ms": spread(tb), "sample_fixed_draw_ms": spread(tk),
                          "cpu_recipe_ms": round(cpu_ms, 3), "gbs_at_median": round(nbytes / statistics.median(ta) / 1e6, 1),
                          "torch_over_sample": round(statistics.median(tb) / statistics.median(ta), 2),
                          "max_abs_diff_to_torch_fp32": dmax}), flush=True)
        del s, host
    if a.no_step:
        return
    import bench
    from rdst_amd.trainer import DPTrainStep
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    tr = DPTrainStep(net, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0, graph=True, graph_warmup=2)
    B, C, lp, scale, S, H, W = SETTINGS[0]
    s = D.DevicePatchSampler(torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(1)), B, lp, sr_scales=(scale,),
                             device=dev, generator=torch.Generator().manual_seed(2))
    for _ in range(4):
        tr.step_from(s)
    torch.cuda.synchronize()
    if tr.graph is None:
        raise SystemExit("sampler_bench: the step was not captured")
    x, tgt = tr._static

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    fixed, sampled = [], []
    for _ in range(a.reps):
        fixed.append(block(lambda: tr.step(x, tgt)))
        sampled.append(block(lambda: tr.step_from(s)))
    print(json.dumps({"step": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, graph replay", "step_fixed_batch_ms": spread(fixed),
                      "step_from_sampler_ms": spread(sampled),
                      "difference_ms": round(statistics.median(sampled) - statistics.median(fixed), 4)}), flush=True)


if __name__ == "__main__":
    main()
