#!/usr/bin/env python3
"""usage: tools/op_hashes.py OUT
sha256 (16 hex digits) of what the fp32x3 ops on the register-stationary kernels and their pack kernels return: forward and every
gradient of the three conv3x shapes, at (33, 6, 256) and at the E1 sizes, and of four LayerNorm -> Linear shapes, each op twice (is
it repeatable?).  For comparing two builds of the library bit for bit where a whole fp32x3 training step cannot be (its backward is
not reproducible run to run): run it once per build (RDST_HIP_LIB=<the other library>) and compare the two files."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rdst_amd import ops

dev = torch.device("cuda:0")


def rnd(shape, seed, s=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * s).to(dev)


def h(t):
    return hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:16]


lines = []
ops.set_f32_split(True)
for (B, H, W, Cin, Cout, res, r) in [(33, 6, 256, 150, 60, 1, 1), (33, 6, 256, 60, 60, 1, 1), (33, 6, 256, 60, 240, 0, 2),
                                     (3, 64, 64, 150, 60, 1, 1), (2, 64, 64, 60, 60, 0, 1), (1, 128, 128, 60, 240, 0, 2)]:
    for rep in range(2):   # twice: is the op itself repeatable?
        x, w, b = rnd((B, H, W, Cin), 1).requires_grad_(True), rnd((Cout, Cin, 3, 3), 2, (Cin * 9) ** -0.5).requires_grad_(True), \
            rnd((Cout,), 3, 0.1).requires_grad_(True)
        cy = Cout // (r * r)
        rr = rnd((B, H * r, W * r, cy), 4) if res else None
        y = ops.conv_rows(x, w, b, residual=rr, out_scale=0.7, shuffle=r)
        y.backward(rnd((B, H * r, W * r, cy), 5))
        torch.cuda.synchronize()
        lines.append(f"conv {B}x{H}x{W} {Cin}->{Cout} r{r} rep{rep}: y {h(y)} dx {h(x.grad)} dW {h(w.grad)} db {h(b.grad)}")
for (M, K, N) in [(4096, 60, 180), (4096, 120, 360), (4096, 90, 90), (4096, 120, 30)]:
    for rep in range(2):
        x, w, b = rnd((M, K), 1).requires_grad_(True), rnd((N, K), 2, K ** -0.5).requires_grad_(True), rnd((N,), 3, 0.1).requires_grad_(True)
        lw, lb = rnd((K,), 6).requires_grad_(True), rnd((K,), 7, 0.1).requires_grad_(True)
        y = ops.ln_linear(x, lw, lb, w, b)
        y.backward(rnd((M, N), 5))
        torch.cuda.synchronize()
        lines.append(f"ln_linear {M}x{K}->{N} rep{rep}: y {h(y)} dx {h(x.grad)} dW {h(w.grad)} db {h(b.grad)} dg {h(lw.grad)} dbeta {h(lb.grad)}")
open(sys.argv[1], "w").write("\n".join(lines) + "\n")
