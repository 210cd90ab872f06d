#!/usr/bin/env python3
"""Do two builds of the library compute the same bits in the optimizer kernels?

    python tools/adam_bits.py --old-lib PATH/librdst_hip.so [--new-lib PATH] [--out profiles/refactor_adam.txt]

The tests hold the four Adam entry points to one another; this holds them to ANOTHER BUILD (the parent commit's library, built
into a directory of its own).  One seeded sequence goes through the C ABI of each library in a child process of its own
(RDST_HIP_LIB selects the library; the children run one after the other, each under a time limit, the second only if the
first succeeded), and this process, which never opens the GPU, compares what they left with exact equality:
  rdst_adam_step, rdst_adam_step_ema, rdst_adam_step_dev, rdst_adam_step_dev_ema
  n = 3 (tail only), 4 (one quad), 1027 (tail of 3), 2^21 + 2^10 + 3 (grid-stride wrap plus tail); weight_decay 0 and 0.01
  six steps, gradients of scale 1e-3 .. 1e2 (tests/test_ema_gpu.py's _grads)
  device count: rdst_step_guard before every step, no clipping on the first and max_grad_norm 1e-4 (a coefficient below 1)
                on the others, the fourth step skipped by its loss, milestones (2, 4) with three rates: both are crossed
  EMA:          decay 0.999 and 0.5, warm-up on and off
  rdst_swap_f32 at the four n.
Compared: param, exp_avg, exp_avg_sq, ema after the last step, a bit-pattern sum of each of them after EVERY step, and the 48
bytes of the step state after every step.  Exit status 1 if one element differs."""
import argparse
import itertools
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [3, 4, 1027, 2 ** 21 + 2 ** 10 + 3]
STEPS = 6
HYPER = (0.9, 0.99, 1e-8)                       # beta1, beta2, eps
LR, MILESTONES, RATES = 1e-3, (2, 4), (1e-3, 3e-4, 9e-5)
CHILD_SECONDS = 240


def cases():
    for dev, ema in itertools.product((False, True), repeat=2):
        for n, wd in itertools.product(SIZES, (0.0, 0.01)):
            for decay, warmup in (itertools.product((0.999, 0.5), (0, 1)) if ema else [(None, 0)]):
                name = "rdst_adam_step" + ("_dev" if dev else "") + ("_ema" if ema else "")
                yield name, dev, ema, n, wd, decay, warmup


def label(name, n, wd, decay, warmup):
    return f"{name} n={n} wd={wd}" + (f" decay={decay} warmup={warmup}" if decay is not None else "")


def bit_sum(t):
    return int(t.view(torch.int32).to(torch.int64).sum().item())


def run(out_dir):
    """The child: every case through the loaded library, results to out_dir."""
    from rdst_amd import _lib
    lib = _lib.load()
    dev0 = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for idx, (name, dev, ema, n, wd, decay, warmup) in enumerate(cases()):
        p = torch.randn(n, device=dev0, generator=torch.Generator(device=dev0).manual_seed(11))
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        e = p.clone()
        gen = torch.Generator(device=dev0).manual_seed(0)
        grads = [torch.randn(n, device=dev0, generator=gen) * 10.0 ** float(i - 3) for i in range(STEPS)]
        bufs = [p, m, v] + ([e] if ema else [])
        ptrs = [p.data_ptr(), None, m.data_ptr(), v.data_ptr()] + ([e.data_ptr()] if ema else [])
        ema_args = [decay, warmup] if ema else []
        sums, states = [], []
        if dev:
            state = torch.zeros(_lib.STEP_STATE_BYTES // 8, dtype=torch.int64, device=dev0)
            st0 = _lib.StepState(last_keep=1, last_clip=1.0, last_sumsq=-1.0)
            state.copy_(torch.frombuffer(bytearray(st0), dtype=torch.int64))
            ws = torch.empty(max(int(lib.rdst_step_guard_workspace(n)), 16) // 8, dtype=torch.float64, device=dev0)
            sched = _lib.LrSchedule()
            sched.count = len(MILESTONES)
            for i, ms in enumerate(MILESTONES):
                sched.milestones[i] = ms
            for i, r in enumerate(RATES):
                sched.lr[i] = r
        for i, g in enumerate(grads):
            ptrs[1] = g.data_ptr()
            if dev:
                loss = torch.tensor([9.0 if i == 3 else 0.5], dtype=torch.float32, device=dev0)
                _lib.check(lib.rdst_step_guard(loss.data_ptr(), 1.0, None, g.data_ptr(), n, 1e-4 if i else 0.0, 1, ws.data_ptr(),
                                               ws.numel() * 8, state.data_ptr(), stream), "rdst_step_guard")
                _lib.check(getattr(lib, name)(*ptrs, n, sched, *HYPER, wd, *ema_args, state.data_ptr(), stream), name)
                states.append(state.cpu().view(torch.uint8).tolist())
            else:
                _lib.check(getattr(lib, name)(*ptrs, n, LR, *HYPER, wd, i + 1, *ema_args, stream), name)
            sums.append([bit_sum(b) for b in bufs])
        torch.cuda.synchronize()
        torch.save({"label": label(name, n, wd, decay, warmup), "bufs": [b.cpu() for b in bufs], "sums": sums, "states": states},
                   os.path.join(out_dir, f"case_{idx:03d}.pt"))
    for n in SIZES:
        gen = torch.Generator(device=dev0).manual_seed(5)
        a, b = torch.randn(n, device=dev0, generator=gen), torch.randn(n, device=dev0, generator=gen)
        _lib.check(lib.rdst_swap_f32(a.data_ptr(), b.data_ptr(), n, stream), "rdst_swap_f32")
        torch.cuda.synchronize()
        torch.save({"label": f"rdst_swap_f32 n={n}", "bufs": [a.cpu(), b.cpu()], "sums": [], "states": []},
                   os.path.join(out_dir, f"swap_{n}.pt"))
    print(f"adam_bits: {_lib.LIB_PATH}: {idx + 1} Adam cases and {len(SIZES)} exchanges on {torch.cuda.get_device_name(0)}", flush=True)


def final_state(states):
    """What the sequence did to the step state (of the new library's run): the skip, the last coefficient and rate."""
    if not states:
        return ""
    from rdst_amd import _lib
    st = _lib.StepState.from_buffer_copy(bytes(states[-1]))
    clips = [_lib.StepState.from_buffer_copy(bytes(s)).last_clip for s in states]
    return f" (kept {st.kept}, skipped {st.skipped}, last_lr {st.last_lr:.3g}, clip per step {' '.join(f'{c:.3g}' for c in clips)})"


def compare(dir_old, dir_new, lines):
    names = sorted(os.listdir(dir_old))
    if names != sorted(os.listdir(dir_new)) or not names:
        raise SystemExit("adam_bits: the two runs left different sets of cases")
    bad = elements = 0
    for f in names:
        o, w = (torch.load(os.path.join(d, f)) for d in (dir_old, dir_new))
        assert o["label"] == w["label"] and len(o["bufs"]) == len(w["bufs"])
        count = sum(b.numel() for b in o["bufs"])
        diff = sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(o["bufs"], w["bufs"]))
        steps = sum(a != b for a, b in zip(o["sums"], w["sums"])) + (len(o["sums"]) != len(w["sums"]))
        state = sum(sum(x != y for x, y in zip(a, b)) for a, b in zip(o["states"], w["states"]))
        lines.append(f"{o['label']}: {count} elements, {diff} differ; {len(o['sums'])} per-step bit sums, {steps} differ; "
                     f"{48 * len(o['states'])} state bytes, {state} differ" + final_state(w["states"]))
        elements += count
        bad += diff + steps + state
    lines.append(f"# {len(names)} cases, {elements} elements compared bit for bit: {bad} differences")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old-lib")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "rdst_amd", "librdst_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--run", default=None, help=argparse.SUPPRESS)      # the child: the directory to fill
    a = ap.parse_args()
    if a.run:
        return run(a.run)
    if not a.old_lib:
        ap.error("--old-lib is required")
    tmp = tempfile.mkdtemp(prefix="adam_bits_")
    lines = [f"# tools/adam_bits.py: old = {a.old_lib}, new = {os.path.relpath(a.new_lib, ROOT)}"]
    try:
        for side, lib in (("old", a.old_lib), ("new", a.new_lib)):
            os.mkdir(os.path.join(tmp, side))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", os.path.join(tmp, side)],
                               env={**os.environ, "RDST_HIP_LIB": os.path.abspath(lib)}, timeout=CHILD_SECONDS)
            if r.returncode != 0:       # nothing more is started on the GPU after a child that failed
                raise SystemExit(f"adam_bits: the run on the {side} library ended with status {r.returncode}")
        bad = compare(os.path.join(tmp, "old"), os.path.join(tmp, "new"), lines)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
