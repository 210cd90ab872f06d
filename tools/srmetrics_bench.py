#!/usr/bin/env python3
"""PSNR + SSIM of a batch of super-resolved images: rdst_amd.metrics.device_scores (HIP, fp64) against the host path
SRMetrics("psnr ssim") (numpy / scipy in float64) that SRTester.evaluate uses by default.

    python tools/srmetrics_bench.py [--iters 20]

Device: HIP events around `iters` back-to-back calls (the two kernels; the inputs already on the GPU), and the wall time of
one call plus the host copy of its 2 N doubles.  Host: wall time of SRMetrics("psnr ssim") on the device tensors, the
.cpu() copy of both batches (after a device sync) included.  Settings: 64 x 1 x 176 x 208 at margin 4 (the OASIS slice at
x4) and 16 x 3 x 256 x 256 at margin 0.  One JSON line per setting; the largest score difference of the two paths is
printed with it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdst_amd import metrics as M  # noqa: E402

SETTINGS = [((64, 1, 176, 208), 4), ((16, 3, 256, 256), 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("srmetrics_bench: no GPU")
    dev = torch.device("cuda:0")
    for shape, margin in SETTINGS:
        g = torch.Generator(device=dev).manual_seed(1)
        gt = torch.rand(shape, generator=g, device=dev)
        pred = (gt + 0.05 * torch.randn(shape, generator=g, device=dev)).clamp_(0, 1)
        for _ in range(3):
            M.device_scores(gt, pred, margin)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            M.device_scores(gt, pred, margin)
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.iters
        t0 = time.perf_counter()
        for _ in range(a.iters):
            mse, ss = M.device_scores(gt, pred, margin)
            dev_scores = torch.stack((mse, ss)).cpu()
        dev_wall_ms = (time.perf_counter() - t0) * 1e3 / a.iters
        host = M.SRMetrics("psnr ssim")
        rep = host(gt, pred, margin)          # warm-up (scipy import, page-in)
        t0 = time.perf_counter()
        for _ in range(a.host_iters):
            torch.cuda.synchronize()
            rep = host(gt, pred, margin)
        host_ms = (time.perf_counter() - t0) * 1e3 / a.host_iters
        dpsnr = max(abs(M.psnr_from_mse(m) - h) for m, h in zip(dev_scores[0].tolist(), rep["psnr"]))
        dssim = float(np.max(np.abs(dev_scores[1].numpy() - np.asarray(rep["ssim"]))))
        print(json.dumps({"shape": list(shape), "margin": margin, "device_ms": round(dev_ms, 4),
                          "device_with_copy_ms": round(dev_wall_ms, 4), "host_numpy_ms": round(host_ms, 2),
                          "speedup": round(host_ms / dev_ms, 1), "max_dpsnr_db": dpsnr, "max_dssim": dssim}), flush=True)


if __name__ == "__main__":
    main()
