#!/usr/bin/env python3
"""usage: tools/op_hashes.py OUT [REPS]      (REPS: how often the launch_trace.py calls are repeated, default twice)
sha256 (16 hex digits) of what the fp32x3 ops on the register-stationary kernels and their pack kernels return: forward and every
gradient of the three conv3x shapes, at (33, 6, 256) and at the E1 sizes, and of four LayerNorm -> Linear shapes, each op twice (is
it repeatable?), and of every call of tools/launch_trace.py (bf16 / fp32 / fp32x3 window attention, the bf16 fused Mlp and one-pass
Linear backward at the shapes that decide their kernels).  For comparing two builds of the library bit for bit where a whole fp32x3 training step cannot be (its backward is
not reproducible run to run): run it once per build (RDST_HIP_LIB=<the other library>) and compare the two files:
tools/op_hashes.py --compare PARENT_OUT TREE_OUT (no GPU) holds the tree to every value that repeats in the parent's file; d(table)
of the window-attention kernels that add it up with float atomics in LDS does not."""
import hashlib
import os
import re
import sys


def compare(parent, tree):
    """Every value that is the same in all repetitions of the parent's file must be that value in all of the tree's."""
    def load(path):
        vals = {}
        for line in open(path):
            label, rest = line.rstrip("\n").split(": ", 1)
            op, rep = label.rsplit(" rep", 1)
            words = re.sub(r"^rc ((-?\d+ ?)+)", lambda m: "rc " + m.group(1).strip().replace(" ", ",") + " ", rest).split()
            for name, v in zip(words[0::2], words[1::2]):
                vals.setdefault((op, name), []).append(v)
        return vals
    P, T = load(parent), load(tree)
    assert P.keys() == T.keys(), "the two files list different ops"
    stable = {k: v for k, v in P.items() if len(set(v)) == 1}
    bad = [k for k, v in stable.items() if set(T[k]) != set(v)]
    for k in P:
        if k not in stable:
            print(f"not repeatable in the parent: {k[0]}: {k[1]} ({len(set(P[k]))} values in {len(P[k])} runs; tree {len(set(T[k]))} in {len(T[k])})")
    for k in bad:
        print(f"DIFFERS: {k[0]}: {k[1]}: parent {stable[k][0]}, tree {' '.join(T[k])}")
    print(f"{len(P)} values; {len(stable)} repeat in the parent; {len(bad)} of those differ in the tree")
    return 1 if bad else 0


if sys.argv[1:2] == ["--compare"]:
    sys.exit(compare(sys.argv[2], sys.argv[3]))

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
ops.set_f32_split(False)
# every call of tools/launch_trace.py (window attention in the three modes at the shapes that decide its kernel, the bf16 fused
# Mlp, the bf16 one-pass Linear backward): return codes and every output, each call twice
import launch_trace
from rdst_amd import _lib
for rep in range(int(sys.argv[2]) if len(sys.argv) > 2 else 2):
    for label, rcs, tensors in launch_trace.calls(torch, _lib.load()):
        lines.append(f"{label} rep{rep}: rc {' '.join(map(str, rcs))} " + " ".join(f"{k} {h(t)}" for k, t in tensors.items()))
open(sys.argv[1], "w").write("\n".join(lines) + "\n")
