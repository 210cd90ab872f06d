#!/usr/bin/env python3
"""A training batch cut and degraded on the device: rdst_amd.data.DevicePatchSampler.sample() (one HIP launch) against the
same batch from torch device ops and against the reference's recipe on the CPU.

    python tools/sampler_bench.py [--iters 50] [--reps 5] [--cpu-iters 5] [--steps 20] [--no-step]
    python tools/sampler_bench.py --augment [--mix uniform|identity|flips|transposed] [--iters 50] [--reps 5] [--steps 20] [--no-step]

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
sampled batch costs a training step.

--augment: what DevicePatchSampler(augment=True) (rdst_sample_patches_d8: a flip / transpose per patch, then the degradation) costs
beside the plain sampler of the same tree, per setting, the blocks of a row alternating `reps` times in one process:
  (a) sample() of the augmenting sampler against sample() of the plain one, and against the torch device-op composition: the
      plain batch, then per patch tiling.dihedral(...).contiguous(), a stack and a second F.interpolate(bicubic);
  (b) the host wall time of draw() with and without the B variants (no device involved), per call;
  (c) the launch alone (a fixed draw into the caller's tensors), plain against augmented with the variants of `--mix`:
      `uniform` 0..7 in turn, `identity` all 0, `flips` 0..3 in turn, `transposed` 4..7 in turn.  Under
      `rocprofv3 --kernel-trace --stats -- python tools/sampler_bench.py --augment --mix M --fixed-only --no-step --reps 2`
      the d8 kernel's durations are those of mix M (--fixed-only leaves out the free-running rows, which draw uniformly).
Then ms/step of the graph-replayed E1 bf16 step through step_from(augmenting sampler) against step_from(plain sampler), blocks
of `steps` alternating `reps` times on ONE trainer (both samplers write into the graph's tensors)."""
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


MIXES = {"uniform": range(8), "identity": (0,), "flips": range(4), "transposed": range(4, 8)}


def augment_main(a, dev):
    from rdst_amd.tiling import dihedral
    for B, C, lp, scale, S, H, W in SETTINGS:
        host = torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(1))
        p = D.DevicePatchSampler(host, B, lp, sr_scales=(scale,), device=dev, generator=torch.Generator().manual_seed(2))
        s = D.DevicePatchSampler(host, B, lp, sr_scales=(scale,), device=dev, generator=torch.Generator().manual_seed(2),
                                 augment=True)
        s.hr_images = p.hr_images           # one resident stack
        hp = int(lp * scale)

        def torch_aug():
            d = s.draw()
            b = p.sample(draw=D.Draw(d.sr_factor, d.hr_patch_size, d.indices))
            hr = torch.stack([dihedral(b["out"][i], k).contiguous() for i, k in enumerate(d.variants.tolist())])
            return F.interpolate(hr, size=(lp, lp), mode="bicubic", align_corners=False), hr, d

        tl, th, d = torch_aug()
        b = s.sample(draw=d)
        assert torch.equal(th, b["out"]) and torch.equal(b["in"], D.bicubic_resize(b["out"], lp))
        dmax = (tl - b["in"]).abs().max().item()
        mix = torch.tensor([MIXES[a.mix][i % len(MIXES[a.mix])] for i in range(B)], dtype=torch.int32)
        fixed = D.Draw(d.sr_factor, d.hr_patch_size, d.indices, mix)
        plain_fixed = D.Draw(d.sr_factor, d.hr_patch_size, d.indices)
        out = (b["in"], b["out"])
        for _ in range(5):
            s.sample(out=out, draw=fixed), p.sample(out=out, draw=plain_fixed)
            if not a.fixed_only:
                p.sample(), s.sample(), torch_aug(), p.draw(), s.draw()
        tp, ta, tt, kp, ka, dp, da = [], [], [], [], [], [], []
        for _ in range(a.reps):
            if not a.fixed_only:
                tp.append(events(p.sample, a.iters))
                ta.append(events(s.sample, a.iters))
                tt.append(events(torch_aug, a.iters))
                for sampler, acc in ((p, dp), (s, da), (p, dp), (s, da)):     # twice each, in turn: the host clock is noisy
                    t0 = time.perf_counter()
                    for _ in range(4 * a.iters):
                        sampler.draw()
                    acc.append((time.perf_counter() - t0) * 1e3 / (4 * a.iters))
            kp.append(events(lambda: p.sample(out=out, draw=plain_fixed), a.iters))
            ka.append(events(lambda: s.sample(out=out, draw=fixed), a.iters))
        row = {"batch": [B, C, hp, hp], "ratio": scale, "slices": [S, H, W], "mix": a.mix,
               "plain_fixed_draw_ms": spread(kp), "augment_fixed_draw_ms": spread(ka)}
        if not a.fixed_only:
            row.update({"plain_sample_ms": spread(tp), "augment_sample_ms": spread(ta), "torch_composition_ms": spread(tt),
                        "plain_draw_host_ms": spread(dp), "augment_draw_host_ms": spread(da),
                        "augment_minus_plain_ms": round(statistics.median(ta) - statistics.median(tp), 4),
                        "draw_difference_host_ms": round(statistics.median(da) - statistics.median(dp), 4),
                        "torch_over_augment": round(statistics.median(tt) / statistics.median(ta), 2),
                        "equal_to_torch_hr": True, "max_abs_diff_to_torch_fp32": dmax})
        print(json.dumps(row), flush=True)
        del p, s, host
    if a.no_step:
        return
    import bench
    from rdst_amd.trainer import DPTrainStep
    net = bench.build_net(dev, torch.bfloat16, bench.E1)
    tr = DPTrainStep(net, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0, graph=True, graph_warmup=2)
    B, C, lp, scale, S, H, W = SETTINGS[0]
    host = torch.rand(S, C, H, W, generator=torch.Generator().manual_seed(1))
    p = D.DevicePatchSampler(host, B, lp, sr_scales=(scale,), device=dev, generator=torch.Generator().manual_seed(2))
    s = D.DevicePatchSampler(host, B, lp, sr_scales=(scale,), device=dev, generator=torch.Generator().manual_seed(2), augment=True)
    s.hr_images = p.hr_images
    for _ in range(4):
        tr.step_from(p)
        tr.step_from(s)
    torch.cuda.synchronize()
    if tr.graph is None:
        raise SystemExit("sampler_bench: the step was not captured")

    def block(sampler):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step_from(sampler)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps
    plain, aug = [], []
    for _ in range(a.reps):
        plain.append(block(p))
        aug.append(block(s))
    print(json.dumps({"step": "RDST-E1 x4 bf16, 32 x 1 x 64x64 -> 256x256, graph replay", "step_from_plain_ms": spread(plain),
                      "step_from_augment_ms": spread(aug), "plain_spread_ms": round(max(plain) - min(plain), 4),
                      "difference_ms": round(statistics.median(aug) - statistics.median(plain), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--mix", choices=sorted(MIXES), default="uniform")
    ap.add_argument("--fixed-only", action="store_true", help="--augment: only the fixed-draw launches (for a kernel trace)")
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
    if a.augment:
        return augment_main(a, dev)
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
